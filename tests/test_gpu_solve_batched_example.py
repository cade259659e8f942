"""examples/solve_batched_main.cpp: SWIPDG::solve on three right-hand sides of ESV2007 32 x 32 Q1 in one batched
device solve, the linear-solver exception naming the first column that failed, and two local right-hand sides through
BlockSWIPDG::solve_local -- every column compared byte for byte with its single solve by the program itself; run as a
child process."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(os.environ.get("HDD_EXAMPLES_BIN") or os.path.join(ROOT, "examples", "bin"), "solve_batched_main")


def test_solve_batched_example_is_built():
    assert os.access(EXE, os.X_OK), "examples/bin/solve_batched_main missing: run make -C dune-hdd_amd"


@pytest.mark.gpu
def test_solve_batched_example_converges():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "solve kernels apply_tile_kernel<4, 4, 4, dot> + cg_update<4, 4> + cg_direction<4>" in out, out
    cols = re.findall(r"^converged: column (\d), (\d+) iterations, residual (\S+), \|\|b\|\| (\S+), bit-identical to the single solve$",
                      r.stdout, re.M)
    assert [int(m[0]) for m in cols] == [0, 1, 2], out
    for m in cols:
        assert 0 < int(m[1]) < 10000 and float(m[2]) <= 1e-8 * float(m[3].rstrip(","))
    assert "max_iter = 2 rejected: apply_inverse: linear solver failed for right-hand side 0 of 3 (max_iter reached, status 1) " \
           "after 2 iterations" in out, out
    local = re.findall(r"^converged: local column (\d), \d+ iterations.*bit-identical to the single solve$", r.stdout, re.M)
    assert local == ["0", "1"], out
    assert "DIFFERS" not in out and "NOT converged" not in out
    assert "solve batched ok" in out
