"""Record rhs_bits_parent.json, the fixture of tests/test_gpu_rhs_parity.py: digests of what H.rhs and the generic
family of H.product give for that test's cases, from the library that is built in this tree, on the device (an
MI355X).  Run at the commit whose bits are to be kept; a change that alters the arithmetic of an entry on purpose runs
it again and says so.  Arguments: another output file, and the name of the commit the library was built from."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "dune-hdd_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

if __name__ == "__main__":
    import torch

    import test_gpu_rhs_parity as T
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "rhs_bits_parent.json")
    commit = sys.argv[2] if len(sys.argv) > 2 else "unknown"
    cases = {}
    for case in T.CASES:
        inputs, result = T.record(case)
        again = T.record(case)
        assert again == (inputs, result), (T.case_id(case), "not reproducible from call to call")
        cases[T.case_id(case)] = dict(inputs=inputs, result=result)
        print(T.case_id(case), result["y_head"], flush=True)
    with open(path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), commit=commit, cases=cases), f, indent=1)
        f.write("\n")
    print(path, len(cases))
