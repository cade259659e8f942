"""Record apply_bits_parent.json, the fixture of tests/test_gpu_apply_parity.py: digests of what H.apply and
H.apply_multi give for that test's cases, from the library that is built in this tree, on the device (an MI355X).  Run
at the commit whose bits are to be kept; a change that alters the arithmetic of an entry on purpose runs it again and
says so.  An argument names another output file."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "dune-hdd_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

if __name__ == "__main__":
    import torch

    import hdd_amd as H
    import test_gpu_apply_parity as T
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "apply_bits_parent.json")
    ctx = H.Context(0)
    cases = {}
    for case in T.CASES:
        inputs, result = T.record(ctx, case)
        again = T.record(ctx, case)
        assert again == (inputs, result), (T.case_id(case), "not reproducible from call to call")
        cases[T.case_id(case)] = dict(inputs=inputs, result=result)
        print(T.case_id(case), result["kernel"], result["y_head"], flush=True)
    with open(path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), cases=cases), f, indent=1)
        f.write("\n")
    print(path, len(cases))
