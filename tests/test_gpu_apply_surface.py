"""apply / apply2 / apply_local_operator / apply_coupling_operator of the C++ surface (include/hdd_discretizations.hh)
driven by examples/apply_main.cpp, against the CPU oracle's matrices times the same vectors.

Tolerance: the rounding bound of tests/test_gpu_apply.py -- 2 gamma_K (|A| |x|)_r with K = n_comp len_r + n_comp + 2
terms per row (apply2: K + n_rows on |v|^T |A| |x|) -- plus the assembly parity 1e-12 (the device
matrix agrees with the oracle's to 1e-12) scaled by the same |A| |x|."""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle as O

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(os.environ.get("HDD_EXAMPLES_BIN") or os.path.join(ROOT, "examples", "bin"), "apply_main")
U = 2.0 ** -53
PARITY = 1e-12


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def test_apply_example_is_built():
    assert os.access(EXE, os.X_OK), "examples/bin/apply_main missing: run make -C dune-hdd_amd"


@pytest.fixture(scope="module")
def apply_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("apply"))
    r = subprocess.run([EXE, d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, (lambda n, t=np.float64: np.fromfile(os.path.join(d, n + ".bin"), dtype=t))


def check_apply(y, A, absA, x, n_comp, what):
    K = n_comp * np.diff(A.indptr) + n_comp + 2
    ref, scale = A @ x, absA @ np.abs(x)
    bound = (2.0 * gamma(K) + PARITY) * scale
    err = np.abs(y - ref)
    assert y.shape == ref.shape and np.isfinite(y).all(), what
    assert (err <= bound).all(), (what, float((err / np.maximum(scale, 1e-300)).max()))
    return K


def check_apply2(got, A, absA, v, x, n_comp, what):
    K = A.shape[0] + (n_comp * np.diff(A.indptr) + n_comp + 2).max()
    ref, scale = v @ (A @ x), np.abs(v) @ (absA @ np.abs(x))
    assert abs(got - ref) <= (2.0 * gamma(K) + PARITY) * scale, (what, got, ref, scale)


@pytest.mark.gpu
def test_block_operators_applied_in_place(apply_run):
    out, ld = apply_run
    assert "apply ok" in out
    # the system matrix of the whole-grid view takes the tile kernel, also through a block range; extracted
    # operators take the CSR kernel
    assert "block apply kernel apply_tile_kernel<3, 3, 1>" in out, out
    assert "local apply kernel apply_tile_kernel<3, 3, 1>" in out, out
    assert "extracted apply kernel apply_csr_kernel<8, 1>" in out, out
    assert "coupling(0,3) rejected: Subdomain 3 is not a neighbour of subdomain 0" in out, out
    assert "short vector rejected" in out
    g = H.Grid.structured(H.SIMPLEX, 16, 16, (-1, -1), (1, 1), px=2, py=2)
    pc, pev, psd = g.connectivity()
    et, oc, oev = O.kuhn_grid(16, 16, (-1, -1), (1, 1))
    key = {tuple(r): i for i, r in enumerate(oev)}
    perm = np.array([key[tuple(r)] for r in pev])
    sub = np.empty(g.ne, np.int32)
    sub[perm] = psd
    _, rp, col, val = O.assemble_block(O.Grid(et, oc, oev), sub, 4, O.scalar(), O.tensor(), O.params())
    n = rp.shape[0] - 1
    A = sp.csr_matrix((val, col, rp), shape=(n, n))
    absA = sp.csr_matrix((np.abs(val), col, rp), shape=(n, n))
    x, v = ld("block_x"), ld("block_v")
    assert x.shape == (n,) and np.abs(x).max() < 1 and np.abs(x).std() > 0.2
    check_apply(ld("block_y"), A, absA, x, 1, "system_matrix().apply")
    check_apply2(ld("block_vAx")[0], A, absA, v, x, 1, "system_matrix().apply2")
    nn = int(ld("neighbour0", np.int32)[0])
    a0, b0 = g.subdomain_range(0, 1)
    an, bn = g.subdomain_range(nn, nn + 1)
    r0, rn = slice(3 * a0, 3 * b0), slice(3 * an, 3 * bn)
    for name, cols in (("local0", r0), ("coupling0", rn)):
        B, absB = A[r0, cols], absA[r0, cols]
        for suffix in ("_y", "_y_extracted"):
            check_apply(ld(name + suffix), B, absB, x[cols], 1, name + suffix)
    assert np.any(ld("coupling0_y"))


@pytest.mark.gpu
def test_parametric_operator_applied_at_mu(apply_run):
    out, ld = apply_run
    assert "os2014 apply kernel apply_tile_kernel<3, 3, 1>" in out, out
    g2 = O.Grid(*O.kuhn_grid(8, 8, (-1, -1), (1, 1)))
    kx, ky = 4 * math.pi, 2 * math.pi
    rp, col, va = O.assemble(g2, O.scalar(O.FN_SINUSOID, 1.0, 0.75, kx, ky, order=3), O.tensor(), O.params())
    _, _, vc = O.assemble(g2, O.scalar(O.FN_SINUSOID, 0.0, -0.75, kx, ky, order=3), O.tensor(), O.params())
    n = rp.shape[0] - 1
    x, v = ld("os_x"), ld("os_v")
    for mu, name in ((0.0, "os_y_0"), (0.3, "os_y_0.3")):
        A = sp.csr_matrix((va + mu * vc, col, rp), shape=(n, n))
        absA = sp.csr_matrix((np.abs(va) + abs(mu) * np.abs(vc), col, rp), shape=(n, n))
        check_apply(ld(name), A, absA, x, 2, name)
    check_apply2(ld("os_vAx_0.3")[0], A, absA, v, x, 2, "apply2(mu = 0.3)")
    assert not np.array_equal(ld("os_y_0"), ld("os_y_0.3"))
