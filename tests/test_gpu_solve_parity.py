"""The device solve gives the bits it gave before its kernels were factored into shared column steps
(solve_init_column, solve_update_block, solve_direction_column): tests/golden/solve_bits_parent.json, recorded on an
MI355X by tests/golden/make_solve_bits.py at the commit before that change, holds per case the SHA-256 of x and of
history[:iterations + 1], the iteration count, the status and the bit patterns of residual and rhs_norm -- digests,
not vectors; the first four values of x are there for a readable failure.

Cases: single solves through H.solve on problem() of test_gpu_solve.py at rtol = 1e-8 with the history, over both
apply paths, with and without the preconditioner, an initial guess, and the block sizes 1, 2, 3, 4, 6, 7, 8 (the odd,
the even, the 16-byte and the scalar instantiations of cg_init / cg_update).  The tile grid of these meshes is their
tile count on every device with two compute units or more, so no sum depends on the device's size.  The batched solve
needs no cases here: test_gpu_solve_batched.py ties every column of it bit for bit to the single solve.

The fixture also holds, as an input condition, the SHA-256 of the downloaded value arrays and of b (and x0): when one
of these differs the test fails saying that the inputs differ (the assembly or the host's numpy changed), not the
solve.

A later change that alters a summation order on purpose (another grid, another reduction tree, another association
in an update) regenerates the fixture with make_solve_bits.py and says so in its description."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from test_gpu_solve import RTOL, dev, problem

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_bits_parent.json")

# problem, apply path, block size, preconditioner, initial guess
CASES = [
    ("p1", "tile", 3, "block_jacobi", False),
    ("p1", "tile", 3, "none", False),
    ("p1", "csr", 3, "block_jacobi", True),
    ("p1", "csr", 1, "block_jacobi", False),
    ("p1", "csr", 6, "block_jacobi", False),
    ("p1", "csr", 7, "block_jacobi", False),
    ("q1", "tile", 4, "block_jacobi", False),
    ("q1", "csr", 2, "block_jacobi", False),
    ("hex_q1", "csr", 8, "block_jacobi", False),
]


def case_id(case):
    name, path, bs, pre, x0 = case
    return "%s-%s-bs%d-%s%s" % (name, path, bs, pre, "-x0" if x0 else "")


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def record(ctx, case):
    """(inputs, result) of one case: what the fixture holds for it"""
    name, path, bs, pre, with_x0 = case
    P = problem(ctx, name)
    c = P.c
    x0 = np.random.default_rng(77).standard_normal(c.n_rows) if with_x0 else None
    inputs = dict(rows=int(c.n_rows), vals_sha256=_sha(*c.hvals), b_sha256=_sha(P.b))
    if with_x0:
        inputs["x0_sha256"] = _sha(x0)
    x, info = H.solve(ctx, c.dp, c.vals, dev(P.b), theta=P.theta, dmesh=c.dm if path == "tile" else None,
                      x0=dev(x0) if with_x0 else None, block_size=bs, precond=pre, rtol=RTOL, history=True)
    xh, hist = x.cpu().numpy(), info.history.cpu().numpy()
    result = dict(kernels=H.last_solve_kernels(), status=int(info.status), iterations=int(info.iterations),
                  residual_bits=_bits(info.residual), rhs_norm_bits=_bits(info.rhs_norm),
                  x_head=[float(v) for v in xh[:4]], x_sha256=_sha(xh), history_sha256=_sha(hist))
    return inputs, result


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_has_exactly_the_cases(parent):
    assert sorted(parent["cases"]) == sorted(case_id(c) for c in CASES)
    for k, rec in parent["cases"].items():
        assert rec["result"]["status"] == H.SOLVE_CONVERGED and rec["result"]["iterations"] > 20, k


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bits_are_the_parents(ctx, parent, case):
    want = parent["cases"][case_id(case)]
    inputs, got = record(ctx, case)
    if inputs != want["inputs"]:
        pytest.fail("the INPUTS differ from the recorded ones (assembled values, b or x0), not the solve: %r != %r"
                    % (inputs, want["inputs"]))
    print(got)
    for key in ("kernels", "status", "iterations", "rhs_norm_bits", "residual_bits", "x_head", "history_sha256", "x_sha256"):
        assert got[key] == want["result"][key], (key, got, want["result"])
