"""Record apply_abi_parent.json, the fixture of tests/test_abi_apply_parity.py: the error texts of the rejected calls
of hdd_operator_apply, hdd_operator_apply2 and hdd_operator_apply_multi, from the library that is built in this tree.
Run at the commit whose answers are to be kept (the one before the two applies were given shared argument checks);
needs no device.  An argument names another output file."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "dune-hdd_amd", "python"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

if __name__ == "__main__":
    import test_abi_apply_parity as T
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "apply_abi_parent.json")
    rec = T.record()
    assert rec == T.record()          # nothing in a message varies from call to call
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(path, {k: len(v) for k, v in rec.items()})
