"""examples/solve_blocks_main.cpp: BlockSWIPDG::solve_locals on the 16 local problems of ESV2007 (32 x 32 Q1 grid in
4 x 4 subdomains) in one device solve, BlockSWIPDG::apply_local_operators in one launch, and the linear-solver
exception naming the first subdomain that failed -- every subdomain compared byte for byte with solve_local /
apply_local_operator by the program itself; run as a child process."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(os.environ.get("HDD_EXAMPLES_BIN") or os.path.join(ROOT, "examples", "bin"), "solve_blocks_main")


def test_solve_blocks_example_is_built():
    assert os.access(EXE, os.X_OK), "examples/bin/solve_blocks_main missing: run make -C dune-hdd_amd"


@pytest.mark.gpu
def test_solve_blocks_example_converges():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "solve kernels apply_tile_blocks_kernel<4, 4, dot> + cg_update_blocks<4> + cg_direction_blocks" in out, out
    assert "apply kernel apply_tile_blocks_kernel<4, 4>" in out, out
    subs = re.findall(r"^converged: subdomain (\d+), (\d+) iterations, residual (\S+), \|\|b\|\| (\S+), bit-identical to the local solve$",
                      r.stdout, re.M)
    assert [int(m[0]) for m in subs] == list(range(16)), out
    for m in subs:
        assert 0 < int(m[1]) < 10000 and float(m[2]) <= 1e-8 * float(m[3].rstrip(","))
    assert "max_iter = 2 rejected: apply_inverse: linear solver failed for segment 0 of 16 (rows 0 .. 256) (max_iter reached, status 1) " \
           "after 2 iterations" in out, out
    assert "DIFFERS" not in out and "NOT converged" not in out
    assert "solve blocks ok" in out
