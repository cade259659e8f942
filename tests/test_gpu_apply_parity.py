"""The operator application gives the bits it gave before its kernels were folded into one tile body, one CSR body
and one launcher for all theta modes: tests/golden/apply_bits_parent.json, recorded on an MI355X by
tests/golden/make_apply_bits.py at the commit before that change, holds per case the SHA-256 of y and the
last_apply_kernel() string -- digests, not vectors; the first four values of y are there for a readable failure.

Cases: the assembled operators of test_gpu_apply_multi.py (the smallest that have full tiles, a partial tile and an
odd image origin).  H.apply on two value arrays at theta = (1, 0.3): P1 on both paths and Q1 on the tile path with
n_vec 1 and 5 (the NV = 1 instantiation, a full group of four and a partial one), the hexahedra (a wave per row;
their one value array twice) and a coupling and a diagonal block of a 2 x 2 partition with n_vec 5.  H.apply_multi
with n_vec 5 at thetas_for: P1 tiles with one, two and three component images, Q1 tiles with one, P1 with four
arrays (the CSR kernel although the mesh is given) and the hexahedra.  Without DOT nothing is summed across tiles or
rows, so y depends neither on the grid nor on the device's size.  The DOT variants need no cases here:
test_gpu_solve_parity.py, test_gpu_solve_batched.py and test_gpu_solve_multi.py pin them to the parent's bits and to
each other.

The fixture also holds, as an input condition, the SHA-256 of the downloaded value arrays and of X: when one of
these differs the test fails saying that the inputs differ (the assembly or the host's numpy changed), not the apply.

A later change that alters the arithmetic of an entry or the order of a row's sum on purpose regenerates the fixture
with make_apply_bits.py and says so in its description."""
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_apply import strided
from test_gpu_apply_multi import case, thetas_for

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "apply_bits_parent.json")
THETA = (1.0, 0.3)

# entry, operator, apply path, value arrays, n_vec, block
CASES = [
    ("apply", "p1", "tile", (0, 1), 1, None),
    ("apply", "p1", "tile", (0, 1), 5, None),
    ("apply", "p1", "csr", (0, 1), 1, None),
    ("apply", "p1", "csr", (0, 1), 5, None),
    ("apply", "q1", "tile", (0, 1), 1, None),
    ("apply", "q1", "tile", (0, 1), 5, None),
    ("apply", "hex", "csr", (0, 0), 5, None),
    ("apply", "p1_block", "tile", (0, 1), 5, (0, 1)),
    ("apply", "p1_block", "tile", (0, 1), 5, (3, 3)),
    ("apply_multi", "p1", "tile", (0,), 5, None),
    ("apply_multi", "p1", "tile", (0, 1), 5, None),
    ("apply_multi", "p1", "tile", (0, 1, 2), 5, None),
    ("apply_multi", "q1", "tile", (0,), 5, None),
    ("apply_multi", "p1", "csr", (0, 1, 0, 1), 5, None),
    ("apply_multi", "hex", "csr", (0,), 5, None),
]
# what the path of a case means: the kernel family it must have run
KERNELS = {("apply", "tile"): "apply_tile_kernel<", ("apply", "csr"): "apply_csr_kernel<",
           ("apply_multi", "tile"): "apply_tile_multi_kernel<", ("apply_multi", "csr"): "apply_csr_multi_kernel<"}


def case_id(c):
    entry, name, path, sel, n_vec, block = c
    return "%s-%s-%s-c%d-v%d%s" % (entry, name, path, len(sel), n_vec, "-b%d%d" % block if block else "")


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def record(ctx, c):
    """(inputs, result) of one case: what the fixture holds for it"""
    entry, name, path, sel, n_vec, block = c
    op = case(ctx, name)
    cols = op.n_cols
    if block:
        d, e = op.grid.subdomain_range(block[1], block[1] + 1)
        cols = 3 * (e - d)
    X = np.random.default_rng(90 + CASES.index(c)).standard_normal((n_vec, cols))
    inputs = dict(cols=int(cols), vals_sha256=_sha(*[op.hvals[q] for q in sel]), x_sha256=_sha(X))
    vals = [op.vals[q] for q in sel]
    # the mesh is given wherever the tile kernel is wanted -- and to apply_multi's four arrays and to the hexahedra,
    # which take the CSR kernel although they have it
    dm = None if (entry, name, path) == ("apply", "p1", "csr") else op.dm
    xd = strided(X, 5)
    if entry == "apply":
        Y = H.apply(ctx, op.dp, vals, xd if n_vec > 1 else xd[0], theta=THETA, dmesh=dm, block=block)
    else:
        Y = H.apply_multi(ctx, op.dp, vals, xd, thetas_for(n_vec, len(sel)), dmesh=dm, block=block)
    kernel = H.last_apply_kernel()
    y = Y.cpu().numpy().reshape(n_vec, -1)
    result = dict(kernel=kernel, shape=list(y.shape), y_head=[float(v) for v in y[0, :4]], y_sha256=_sha(y))
    return inputs, result


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_has_exactly_the_cases(parent):
    assert sorted(parent["cases"]) == sorted(case_id(c) for c in CASES)
    assert len(set(case_id(c) for c in CASES)) == len(CASES)
    for c in CASES:
        rec = parent["cases"][case_id(c)]["result"]
        assert rec["kernel"].startswith(KERNELS[c[0], c[2]]), (case_id(c), rec["kernel"])
        # the name is the last group's: apply's one-vector instantiation when n_vec = 4 k + 1, apply_multi's only one
        assert rec["kernel"].endswith(", %d>" % (4 if c[0] == "apply_multi" or c[4] % 4 != 1 else 1)), (case_id(c), rec["kernel"])
        assert rec["shape"][0] == c[4] and rec["y_sha256"] != _sha(np.zeros(rec["shape"])), case_id(c)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_bits_are_the_parents(ctx, parent, c):
    want = parent["cases"][case_id(c)]
    inputs, got = record(ctx, c)
    if inputs != want["inputs"]:
        pytest.fail("the INPUTS differ from the recorded ones (assembled values or X), not the apply: %r != %r"
                    % (inputs, want["inputs"]))
    print(got)
    for key in ("kernel", "shape", "y_head", "y_sha256"):
        assert got[key] == want["result"][key], (key, got, want["result"])
