"""The device solve with a theta per column (hdd_operator_solve_multi: H.solve_multi) against the single solve, column
by column, and against the host matrices A(theta_j).

The contract: column j ends with exactly the x, iterations, status, residual, rhs_norm and history that H.solve gives
for (thetas[j], b_j, x0_j) with the same options on the same path -- bit for bit (int64 views), whatever the other
columns and their thetas are, however the columns fall into groups of four, whatever check_every is.  A finished
column is frozen: were its x touched by a later launch, its bits would differ from the single solve's.  What the tile
kernel does not take (Q1 with two components, more than three components) runs the CSR kernel even with the mesh
given and is compared with the single solve without the mesh.

Matrices: OS2014's two components A_0 + mu A_1 at the reference's penalties, P1 on the Kuhn grid 12 x 11 (264
elements: 4 tiles + 8) and Q1 13 x 10 (130 elements: 2 tiles + 2) on (-1, 1)^2, mu in [0.1, 1]; the local solves on
Kuhn 16 x 16 in 2 x 2 subdomains with mu in {0.5, 0.6, 0.8, 1.0} (the whole 16 x 16 matrix is indefinite below 0.5).
Input condition, asserted per column from the dense host matrix: lambda_min(A(theta_j)) > 0 (numpy.linalg.eigvalsh).
b_j = A(theta_j) xs_j on the host; check_solution's assertions (test_gpu_solve.py: true residual, error bound from
lambda_min, iteration count against a numpy PCG on A(theta_j)) tie every column to the host, not only to the single
solve."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_apply_multi import case
from test_gpu_solve import RTOL, check_solution, dev, numpy_pcg
from test_gpu_solve_batched import assert_columns_equal_singles, bits, same_info, smooth

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

MUS = np.array([0.1, 0.3, 0.5, 1.0, 0.2, 0.4, 0.7, 0.85])
MUS_16 = np.array([0.5, 0.6, 0.8, 1.0])


def _torch():
    import torch
    return torch


def kernels(apply, bs, pre=True):
    """the spelling hdd.h documents"""
    return "%s + cg_update<%d, %s> + cg_direction<4>" % (apply, bs, "4, own" if pre else "none, 4")


TILE_P1, TILE_Q1 = "apply_tile_multi_kernel<3, 3, 4, dot>", "apply_tile_multi_kernel<4, 4, 4, dot>"
CSR8 = "apply_csr_multi_kernel<8, 4, dot>"

_HOST = {}


class Columns:
    """A(theta_j), lambda_min, xs_j, b_j = A(theta_j) xs_j for the rows of thetas, on the host arrays of a case
    (restricted to the square range rng)"""

    def __init__(self, c, sel, thetas, rng=None, seed=0):
        self.c, self.sel = c, tuple(sel)
        self.vals = [c.vals[q] for q in sel]
        self.thetas = np.asarray(thetas, np.float64)
        r0, r1 = rng if rng is not None else (0, c.n_rows)
        self.A, self.lmin = [], []
        for th in self.thetas:
            A = sp.csr_matrix((sum(t * c.hvals[q] for t, q in zip(th, sel)), c.col, c.rp), shape=(c.n_rows, c.n_cols))
            A = A[r0:r1, r0:r1].tocsr()
            self.A.append(A)
            self.lmin.append(float(np.linalg.eigvalsh(A.toarray())[0]))
        n = r1 - r0
        self.XS = np.stack([smooth(n) if j == 1 else np.random.default_rng(100 * seed + j).standard_normal(n)
                            for j in range(len(self.thetas))])
        self.B = np.stack([A @ x for A, x in zip(self.A, self.XS)])
        self._ref = {}

    def assert_definite(self):
        print("lambda_min per column:", ["%.3e" % l for l in self.lmin])
        assert all(l > 0 for l in self.lmin), self.lmin      # input condition

    def ref_iterations(self, j, bs):
        if (j, bs) not in self._ref:
            self._ref[j, bs] = numpy_pcg(self.A[j], self.B[j], bs, RTOL)[1]
        return self._ref[j, bs]


def host(ctx, name, sel, thetas, rng=None):
    key = (name, tuple(sel), np.asarray(thetas, np.float64).tobytes(), rng)
    if key not in _HOST:
        _HOST[key] = Columns(case(ctx, name), sel, thetas, rng, seed=1 + len(sel) + (0 if rng is None else 10 + rng[0] % 7))
    return _HOST[key]


def one_mu(mus):
    """theta_j = (1, mu_j)"""
    return np.stack([np.ones(len(mus)), np.asarray(mus)], axis=1)


def run_both(ctx, P, dm, tile, n=None, B=None, X0=None, **kw):
    """the multi solve of the first n columns and, after it, its single solves on the same path"""
    n = len(P.thetas) if n is None else n
    B = P.B if B is None else B
    Bd = dev(B[:n])
    X, infos = H.solve_multi(ctx, P.c.dp, P.vals, Bd, P.thetas[:n], dmesh=dm, X0=None if X0 is None else dev(X0[:n]),
                             history=True, **kw)
    names = H.last_solve_kernels()
    assert names.startswith("apply_tile_multi_kernel<" if tile else "apply_csr_multi_kernel<"), names
    singles = [H.solve(ctx, P.c.dp, P.vals, Bd[j], theta=P.thetas[j], dmesh=dm if tile else None,
                       x0=None if X0 is None else dev(X0[j]), history=True, **kw) for j in range(n)]
    assert H.last_solve_kernels().startswith("apply_tile_kernel<" if tile else "apply_csr_kernel<")
    return X, infos, singles, names


CASES = [("p1", (0, 1), "tile", kernels(TILE_P1, 3)), ("p1", (0, 1), "csr", kernels(CSR8, 3)),
         ("q1", (0,), "tile", kernels(TILE_Q1, 4)), ("q1", (0, 1), "mesh-csr", kernels(CSR8, 4)),
         ("q1", (0, 1), "csr", kernels(CSR8, 4))]
SHAPES = [(c, n) for c in CASES for n in ((1, 3, 4, 5, 8) if c[0] == "p1" else (3, 5))]


def case_thetas(sel):
    return one_mu(MUS) if len(sel) == 2 else (0.5 + MUS).reshape(-1, 1)     # one component: a scalar per column


@pytest.mark.parametrize("cs,n_rhs", SHAPES, ids=["%s-%d-%s-%d" % (c[0], len(c[1]), c[2], n) for c, n in SHAPES])
def test_columns_are_the_single_solves(ctx, cs, n_rhs):
    name, sel, path, expected = cs
    P = host(ctx, name, sel, case_thetas(sel))
    P.assert_definite()
    c = P.c
    X, infos, singles, names = run_both(ctx, P, None if path == "csr" else c.dm, path == "tile", n=n_rhs, rtol=RTOL)
    assert names == expected
    assert X.shape == (n_rhs, c.n_rows)
    assert_columns_equal_singles(X, infos, singles, "%s %s" % (name, path))
    if n_rhs >= 3:   # input condition: the columns end at different iterations, one is frozen while others go on
        assert len({i.iterations for _, i in singles}) >= 2, [i.iterations for _, i in singles]
    for j in range(n_rhs):
        check_solution(P.A[j], P.lmin[j], P.B[j], P.XS[j], X[j], infos[j], P.ref_iterations(j, c.grid.nb))


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_frozen_columns(ctx, path):
    """rtol = 1e-2; column 2 starts at 0.98 xs_2 and ends several times sooner than the others, which start at zero:
    its x and its history end there"""
    P = host(ctx, "p1", (0, 1), one_mu(MUS))
    P.assert_definite()
    X0 = np.zeros_like(P.XS[:4])
    X0[2] = 0.98 * P.XS[2]
    X, infos, singles, _ = run_both(ctx, P, P.c.dm if path == "tile" else None, path == "tile", n=4, X0=X0, rtol=1e-2)
    its = [i.iterations for _, i in singles]
    assert all(i.status == H.SOLVE_CONVERGED for _, i in singles)
    assert 0 < 2 * its[2] < min(its[:2] + its[3:]), its       # input condition
    assert_columns_equal_singles(X, infos, singles, "frozen")
    assert infos[2].history.shape == (its[2] + 1,)


@pytest.mark.parametrize("cs", [("p1", (0, 1), "tile"), ("q1", (0, 1), "csr")])
def test_check_every(ctx, cs):
    """1, 7 or 32 (the default) iterations enqueued between two looks: the same bits in every column"""
    torch = _torch()
    name, sel, path = cs
    P = host(ctx, name, sel, case_thetas(sel))
    P.assert_definite()
    dm = P.c.dm if path == "tile" else None
    runs = [H.solve_multi(ctx, P.c.dp, P.vals, dev(P.B[:5]), P.thetas[:5], dmesh=dm, rtol=RTOL, check_every=ce, history=True)
            for ce in (1, 7, 0)]
    X1, I1 = runs[0]
    assert all(i.status == H.SOLVE_CONVERGED and i.iterations > 32 for i in I1), [i.iterations for i in I1]
    for X, I in runs[1:]:
        assert torch.equal(bits(X), bits(X1))
        assert all(same_info(a, b) for a, b in zip(I, I1))
    singles = [H.solve(ctx, P.c.dp, P.vals, dev(P.B[j]), theta=P.thetas[j], dmesh=dm, rtol=RTOL, check_every=50, history=True)
               for j in range(5)]
    assert_columns_equal_singles(X1, I1, singles, "check_every")


@pytest.mark.parametrize("cs", [("p1", (0, 1), "tile"), ("p1", (0, 1), "csr"), ("q1", (0,), "tile")])
def test_warm_start(ctx, cs):
    """r_0 = b_j - A(theta_j) x0_j by the plain multi-theta apply: a good guess, zero, a random one, the solution, half"""
    name, sel, path = cs
    P = host(ctx, name, sel, case_thetas(sel))
    P.assert_definite()
    X0 = np.zeros_like(P.XS[:5])
    X0[0] = P.XS[0] * (1.0 + 1e-5)
    X0[2] = np.random.default_rng(9).standard_normal(P.c.n_rows)
    X0[3] = P.XS[3]
    X0[4] = 0.5 * P.XS[4]
    X, infos, singles, _ = run_both(ctx, P, P.c.dm if path == "tile" else None, path == "tile", n=5, X0=X0, rtol=RTOL)
    assert_columns_equal_singles(X, infos, singles, "X0")
    assert infos[3].iterations == 0 and all(i.status == H.SOLVE_CONVERGED for i in infos)
    for j in range(5):
        assert np.linalg.norm(P.B[j] - P.A[j] @ X[j].cpu().numpy()) <= 2 * RTOL * np.linalg.norm(P.B[j])


def _raw_multi(ctx, P, n_rhs, dm, bs, ldb=None, ldx=None, ldh_pad=0, ldt_pad=0, shift=0, rtol=RTOL, max_iter=2000):
    """hdd_operator_solve_multi through ctypes: b with row stride ldb inside NaN; x with row stride ldx and the
    workspace `shift` doubles past a 16-byte boundary, inside NaN; thetas with row stride n_comp + ldt_pad inside
    NaN; the history with row stride max_iter + 1 + ldh_pad.  Returns X, the info tuples and the history after
    checking that nothing around x (its padding included) and the workspace was written."""
    torch = _torch()
    c = P.c
    B = P.B[:n_rhs]
    rows = B.shape[1]
    ldb, ldx = ldb or rows, ldx or rows
    n_work = int(H.lib().hdd_operator_solve_multi_workspace(rows, bs, n_rhs))
    nan = float("nan")
    bbuf = torch.full((n_rhs, ldb), nan, dtype=torch.float64, device="cuda")
    bbuf[:, :rows] = dev(B)
    xbuf = torch.full((n_rhs * ldx + 8,), nan, dtype=torch.float64, device="cuda")
    wbuf = torch.full((n_work + 8,), nan, dtype=torch.float64, device="cuda")
    x, w = xbuf[2 + shift:2 + shift + n_rhs * ldx], wbuf[2 + shift:2 + shift + n_work]
    assert x.data_ptr() % 16 == 8 * shift and w.data_ptr() % 16 == 8 * shift
    X = x.view(n_rhs, ldx)
    n_comp = len(P.vals)
    th = np.full((n_rhs, n_comp + ldt_pad), nan)
    th[:, :n_comp] = P.thetas[:n_rhs]
    ldh = max_iter + 1 + ldh_pad
    hist = torch.zeros((n_rhs, ldh), dtype=torch.float64, device="cuda")
    ptrs = (C.c_void_p * n_comp)(*[v.data_ptr() for v in P.vals])
    opt = H.SolveOptions(rtol, 0.0, max_iter, 0, H.PRECOND_BLOCK_JACOBI, bs, 0, 0)
    infos = (H.SolveInfo * n_rhs)()
    rc = H.lib().hdd_operator_solve_multi(ctx.h, None if dm is None else C.addressof(dm.t), C.addressof(c.dp.t), ptrs,
                                          n_comp, th.ctypes.data, n_comp + ldt_pad, None, bbuf.data_ptr(), ldb,
                                          x.data_ptr(), ldx, n_rhs, C.addressof(opt), w.data_ptr(), n_work,
                                          hist.data_ptr(), ldh, C.addressof(infos),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, H.lib().hdd_last_error(None)
    torch.cuda.synchronize()
    for buf, n in ((xbuf, n_rhs * ldx), (wbuf, n_work)):
        assert bool(torch.isnan(buf[:2 + shift]).all()) and bool(torch.isnan(buf[2 + shift + n:]).all())
    if ldx > rows:
        assert bool(torch.isnan(X[:, rows:]).all())            # the sentinel in the padding of every column
    assert bool(torch.isnan(bbuf[:, rows:]).all()) and torch.equal(bbuf[:, :rows], dev(B))
    return X[:, :rows].clone(), [(i.status, i.iterations, i.residual, i.rhs_norm) for i in infos], hist


@pytest.mark.parametrize("cs,bs", [(("p1", (0, 1), "tile"), 3), (("p1", (0, 1), "tile"), 2), (("p1", (0, 1), "csr"), 6),
                                   (("q1", (0,), "tile"), 4), (("q1", (0, 1), "csr"), 4)])
@pytest.mark.parametrize("n_rhs", [3, 5])
def test_leading_dimensions_and_alignment(ctx, cs, bs, n_rhs):
    """ldb, ldx = rows + 1 (odd: every other column of x is 8 bytes off) and rows + 6, padded ldh and ldt; x and the
    workspace 8 bytes off a 16-byte boundary (the scalar-load instantiations of the even block sizes): the bits of
    the aligned, densely packed call, which are those of the single solves"""
    torch = _torch()
    name, sel, path = cs
    P = host(ctx, name, sel, case_thetas(sel))
    P.assert_definite()
    rows = P.c.n_rows
    assert rows % bs == 0
    dm = P.c.dm if path == "tile" else None
    Xa, ia, ha = _raw_multi(ctx, P, n_rhs, dm, bs)
    assert H.last_solve_kernels().endswith("cg_update<%d, 4, own> + cg_direction<4>" % bs)
    assert all(i[0] == H.SOLVE_CONVERGED for i in ia) and bool(torch.isfinite(Xa).all())
    for ldb, ldx, shift, hp, tp in [(rows + 1, rows + 1, 0, 3, 1), (rows + 6, rows + 6, 0, 0, 6), (rows, rows, 1, 0, 0),
                                    (rows + 1, rows + 6, 1, 5, 2), (rows + 6, rows + 1, 1, 1, 0)]:
        X, i, h = _raw_multi(ctx, P, n_rhs, dm, bs, ldb=ldb, ldx=ldx, ldh_pad=hp, ldt_pad=tp, shift=shift)
        assert torch.equal(bits(X), bits(Xa)), (ldb, ldx, shift)
        assert i == ia, (ldb, ldx, shift)
        assert torch.equal(bits(h[:, :ha.shape[1]]), bits(ha)) and not bool(bits(h[:, ha.shape[1]:]).any())
    singles = [H.solve(ctx, P.c.dp, P.vals, dev(P.B[j]), theta=P.thetas[j], dmesh=dm, block_size=bs, rtol=RTOL, max_iter=2000,
                       history=True) for j in range(n_rhs)]
    for j, (x1, i1) in enumerate(singles):
        assert torch.equal(bits(Xa[j]), bits(x1)) and ia[j] == (i1.status, i1.iterations, i1.residual, i1.rhs_norm), j
        assert torch.equal(bits(ha[j, :i1.iterations + 1]), bits(i1.history)) and not bool(bits(ha[j, i1.iterations + 1:]).any())


def test_no_preconditioner(ctx):
    P = host(ctx, "p1", (0, 1), one_mu(MUS))
    P.assert_definite()
    X, infos, singles, names = run_both(ctx, P, P.c.dm, True, n=5, precond="none", block_size=1, rtol=RTOL)
    assert names == kernels(TILE_P1, 1, pre=False)
    assert_columns_equal_singles(X, infos, singles, "none")
    pre = H.solve(ctx, P.c.dp, P.vals, dev(P.B[0]), theta=P.thetas[0], dmesh=P.c.dm, rtol=RTOL)[1]
    assert infos[0].iterations > pre.iterations          # it is the iteration without the preconditioner
    for j in range(5):
        assert infos[j].status == H.SOLVE_CONVERGED
        assert np.linalg.norm(P.B[j] - P.A[j] @ X[j].cpu().numpy()) <= 2 * RTOL * np.linalg.norm(P.B[j])


@pytest.mark.parametrize("bs", [1, 2, 3, 6])
def test_block_sizes_on_the_csr_path(ctx, bs):
    P = host(ctx, "p1", (0, 1), one_mu(MUS))
    P.assert_definite()
    X, infos, singles, names = run_both(ctx, P, None, False, n=5, block_size=bs, rtol=RTOL)
    assert names == kernels(CSR8, bs)
    assert_columns_equal_singles(X, infos, singles, "block size %d" % bs)
    for j in range(5):
        check_solution(P.A[j], P.lmin[j], P.B[j], P.XS[j], X[j], infos[j], P.ref_iterations(j, bs))


@pytest.mark.parametrize("path", ["tile", "csr"])
@pytest.mark.parametrize("ss", [0, 3])
def test_local_solves(ctx, ss, path):
    """the local solve (ss, ss) on Kuhn 16 x 16 in 2 x 2 subdomains, in place through the block range"""
    c = case(ctx, "p1_block")
    a, b = c.grid.subdomain_range(ss, ss + 1)
    P = host(ctx, "p1_block", (0, 1), one_mu(MUS_16), rng=(3 * a, 3 * b))
    P.assert_definite()
    X, infos, singles, names = run_both(ctx, P, c.dm if path == "tile" else None, path == "tile", block=(ss, ss), rtol=RTOL)
    assert names == kernels(TILE_P1 if path == "tile" else CSR8, 3)
    assert X.shape == P.B.shape
    assert_columns_equal_singles(X, infos, singles, "local %d" % ss)
    for j in range(4):
        check_solution(P.A[j], P.lmin[j], P.B[j], P.XS[j], X[j], infos[j], P.ref_iterations(j, 3))


def test_three_components_on_the_tile_path(ctx):
    """A_0 + mu_j A_1 + nu_j A_2, A_2 the kappa = 1 matrix: three LDS images per wave"""
    th = np.stack([np.ones(5), MUS[:5], np.array([0.0, 0.5, 1.0, 2.0, 0.25])], axis=1)
    P = host(ctx, "p1", (0, 1, 2), th)
    P.assert_definite()
    X, infos, singles, names = run_both(ctx, P, P.c.dm, True, rtol=RTOL)
    assert names == kernels(TILE_P1, 3)
    assert_columns_equal_singles(X, infos, singles, "three components")
    for j in range(5):
        check_solution(P.A[j], P.lmin[j], P.B[j], P.XS[j], X[j], infos[j], P.ref_iterations(j, 3))


def test_eight_components_on_the_csr_path(ctx):
    """the two arrays four times over, theta_j = (w_k, w_k mu_j) for weights w that sum to one; the mesh is given"""
    w = np.array([0.5, 0.25, 0.125, 0.125])
    th = np.stack([np.stack([w, w * mu], axis=1).reshape(-1) for mu in MUS[:5]])
    P = host(ctx, "p1", (0, 1) * 4, th)
    P.assert_definite()
    X, infos, singles, names = run_both(ctx, P, P.c.dm, False, rtol=RTOL)
    assert names == kernels(CSR8, 3)
    assert_columns_equal_singles(X, infos, singles, "eight components")
    for j in range(5):
        check_solution(P.A[j], P.lmin[j], P.B[j], P.XS[j], X[j], infos[j], P.ref_iterations(j, 3))


@pytest.mark.parametrize("path", ["tile", "csr"])
@pytest.mark.parametrize("col", [0, 2])
def test_indefinite_theta_breaks_only_its_column_down(ctx, path, col):
    """theta = (-1, 0) in one column: -A_0 has no positive definite diagonal block.  That column reports BREAKDOWN with
    0 iterations as the single solve does (an ordinary status); the three others are their single solves"""
    torch = _torch()
    good = host(ctx, "p1", (0, 1), one_mu(MUS))
    good.assert_definite()
    th = good.thetas[:4].copy()
    th[col] = (-1.0, 0.0)
    c = good.c
    dm = c.dm if path == "tile" else None
    Bd = dev(good.B[:4])
    X, infos = H.solve_multi(ctx, c.dp, good.vals, Bd, th, dmesh=dm, rtol=RTOL, history=True)
    singles = [H.solve(ctx, c.dp, good.vals, Bd[j], theta=th[j], dmesh=dm, rtol=RTOL, history=True) for j in range(4)]
    assert (singles[col][1].status, singles[col][1].iterations) == (H.SOLVE_BREAKDOWN, 0)
    assert (infos[col].status, infos[col].iterations) == (H.SOLVE_BREAKDOWN, 0)
    assert_columns_equal_singles(X, infos, singles, "theta = (-1, 0) in column %d" % col)
    assert bool(torch.isfinite(X).all())
    for j in range(4):
        if j != col:
            check_solution(good.A[j], good.lmin[j], good.B[j], good.XS[j], X[j], infos[j], good.ref_iterations(j, 3))


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_zero_column(ctx, path):
    P = host(ctx, "p1", (0, 1), one_mu(MUS))
    P.assert_definite()
    B = P.B[:5].copy()
    B[2] = 0.0
    X0 = np.stack([np.full(P.c.n_rows, 0.25)] * 5)     # b = 0 gives x = 0 whatever the initial guess was
    for x0 in (None, X0):
        X, infos, singles, _ = run_both(ctx, P, P.c.dm if path == "tile" else None, path == "tile", n=5, B=B, X0=x0, rtol=RTOL)
        assert not bool(bits(X[2]).any())            # exactly +0.0
        assert (infos[2].status, infos[2].iterations, infos[2].residual, infos[2].rhs_norm) == (H.SOLVE_CONVERGED, 0, 0.0, 0.0)
        assert_columns_equal_singles(X, infos, singles, "zero column")
        for j in (0, 1, 3, 4):
            assert infos[j].status == H.SOLVE_CONVERGED and infos[j].iterations > 0


@pytest.mark.parametrize("cs", [("p1", (0, 1, 2), "tile"), ("p1", (0, 1), "csr"), ("q1", (0,), "tile"), ("q1", (0, 1), "csr")])
def test_no_thetas_is_the_batched_solve(ctx, cs):
    torch = _torch()
    name, sel, path = cs
    P = host(ctx, name, sel, np.ones((5, len(sel))))
    P.assert_definite()
    dm = P.c.dm if path == "tile" else None
    X, infos = H.solve_multi(ctx, P.c.dp, P.vals, dev(P.B), None, dmesh=dm, rtol=RTOL, history=True)
    Xb, infos_b = H.solve_batched(ctx, P.c.dp, P.vals, dev(P.B), dmesh=dm, rtol=RTOL, history=True)
    assert torch.equal(bits(X), bits(Xb)) and all(same_info(a, b) for a, b in zip(infos, infos_b))
    assert all(i.status == H.SOLVE_CONVERGED for i in infos)
    # and with the ones spelled out
    X1, infos_1 = H.solve_multi(ctx, P.c.dp, P.vals, dev(P.B), P.thetas, dmesh=dm, rtol=RTOL, history=True)
    assert torch.equal(bits(X1), bits(Xb)) and all(same_info(a, b) for a, b in zip(infos_1, infos_b))


def test_front_end_rejects(ctx):
    P = host(ctx, "p1", (0, 1), one_mu(MUS))
    c = P.c
    with pytest.raises(H.HddError):
        H.solve_multi(ctx, c.dp, P.vals, dev(P.B[:3]), P.thetas[:2], dmesh=c.dm)         # a theta row is missing
    with pytest.raises(H.HddError):
        H.solve_multi(ctx, c.dp, P.vals, dev(P.B[:3]), P.thetas[:3, :1], dmesh=c.dm)     # a component is missing
    with pytest.raises(H.HddError):
        H.solve_multi(ctx, c.dp, P.vals, dev(P.B[0]), P.thetas[:1], dmesh=c.dm)          # one dimension
