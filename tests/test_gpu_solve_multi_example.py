"""examples/solve_multi_main.cpp: SWIPDG::solve at four mu of OS2014 (12 x 11 Kuhn grid) in one device solve with a
theta per column, the linear-solver exception naming the first column that failed and its mu, and two local
right-hand sides at a mu each through BlockSWIPDG::solve_local -- every column compared byte for byte with its single
solve by the program itself; run as a child process."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(os.environ.get("HDD_EXAMPLES_BIN") or os.path.join(ROOT, "examples", "bin"), "solve_multi_main")


def test_solve_multi_example_is_built():
    assert os.access(EXE, os.X_OK), "examples/bin/solve_multi_main missing: run make -C dune-hdd_amd"


@pytest.mark.gpu
def test_solve_multi_example_converges():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "solve kernels apply_tile_multi_kernel<3, 3, 4, dot> + cg_update<3, 4, own> + cg_direction<4>" in out, out
    cols = re.findall(r"^converged: mu (\S+), (\d+) iterations, residual (\S+), \|\|b\|\| (\S+), bit-identical to the single solve$",
                      r.stdout, re.M)
    assert [m[0] for m in cols] == ["0.10", "0.30", "0.50", "1.00"], out
    for m in cols:
        assert 0 < int(m[1]) < 10000 and float(m[2]) <= 1e-8 * float(m[3].rstrip(","))
    assert "max_iter = 2 rejected: apply_inverse: linear solver failed for column 0 of 4 (mu = 0.100000) (max_iter reached, status 1) " \
           "after 2 iterations" in out, out
    local = re.findall(r"^converged: local mu (\S+), \d+ iterations.*bit-identical to the single solve$", r.stdout, re.M)
    assert local == ["0.60", "1.00"], out
    assert "DIFFERS" not in out and "NOT converged" not in out
    assert "solve multi ok" in out
