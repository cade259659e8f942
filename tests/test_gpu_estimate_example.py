"""examples/estimate_main.cpp: solve and certify through the C++ surface (SWIPDG::solve, SWIPDG::estimate for every
available estimator) on level 1 of the reference's conforming ladder -- the seven rows it prints against
test/linearelliptic-swipdg-expectations_esv2007_2daluconform.cxx:38-57, 3 significant figures; run as a child process."""
import os
import re
import subprocess

import pytest

from test_estimator_ref import TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(os.environ.get("HDD_EXAMPLES_BIN") or os.path.join(ROOT, "examples", "bin"), "estimate_main")
ROWS = dict(eta_NC="eta_NC_ESV2007", eta_R="eta_R_ESV2007", eta_DF="eta_DF_ESV2007", eta="eta_ESV2007", eff="eff_ESV2007",
            eta_alt="eta_ESV2007_alt", eff_alt="eff_ESV2007_alt")


def test_estimate_example_is_built():
    assert os.access(EXE, os.X_OK), "examples/bin/estimate_main missing: run make -C dune-hdd_amd"


@pytest.mark.gpu
def test_estimate_example_prints_the_level_1_rows():
    r = subprocess.run([EXE, "1"], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert re.search(r"^level 1: 512 triangles, 1536 dofs", r.stdout, re.M), out
    for key, name in ROWS.items():
        m = re.search(r"^%s (\S+)$" % re.escape(name), r.stdout, re.M)
        assert m, (name, out)
        assert float(m.group(1)) == TABLE[key][1], (name, m.group(1), TABLE[key][1])
    assert "estimate kernels oswald_vertex_kernel + esv2007_element_kernel<beta1, " in out, out
    assert re.search(r"^eta_R_ESV2007_\* \S+$", r.stdout, re.M), out
    assert "estimate ok" in out
