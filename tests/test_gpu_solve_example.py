"""examples/solve_main.cpp: SWIPDG::solve (uncached_solve on the device: theta-fused operator, block-Jacobi PCG) on
ESV2007 32 x 32 Q1, the linear-solver exception for a max_iter that is too small, and BlockSWIPDG::solve_local --
run as a child process."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(os.environ.get("HDD_EXAMPLES_BIN") or os.path.join(ROOT, "examples", "bin"), "solve_main")


def test_solve_example_is_built():
    assert os.access(EXE, os.X_OK), "examples/bin/solve_main missing: run make -C dune-hdd_amd"


@pytest.mark.gpu
def test_solve_example_converges():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    m = re.search(r"^converged: (\d+) iterations, residual (\S+), \|\|b\|\| (\S+), 4096 dofs", r.stdout, re.M)
    assert m, out
    assert 0 < int(m.group(1)) < 10000 and float(m.group(2)) <= 1e-8 * float(m.group(3))
    assert "solve kernels apply_tile_kernel<4, 4, 1, dot> + cg_update<4> + cg_direction" in out, out
    assert "max_iter = 2 rejected: apply_inverse: linear solver failed (max_iter reached, status 1) after 2 iterations" in out
    assert re.search(r"^local solve: \d+ iterations.*apply_tile_kernel<3, 3, 1, dot>", r.stdout, re.M), out
    assert "solve ok" in out
