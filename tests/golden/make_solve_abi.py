"""Record solve_abi_parent.json, the fixture of tests/test_abi_solve_parity.py: the workspace sizes and the error
texts of the rejected calls, from the library that is built in this tree.  Run at the commit whose answers are to be
kept (the one before hdd_operator_solve and hdd_operator_solve_batched were given one driver; for the sections of the
later entries -- multi, blocks and the two estimate calls -- the one before every entry was given one call path per
layer, at which the first sections come out as they were); needs no device.
An argument names another output file."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "dune-hdd_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

if __name__ == "__main__":
    import test_abi_solve_parity as T
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "solve_abi_parent.json")
    rec = {**T.record(), **T.record_later()}
    assert rec == {**T.record(), **T.record_later()}          # nothing in a message varies from call to call
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(path, {k: len(v) for k, v in rec.items()})
