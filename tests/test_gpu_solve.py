"""The device solve (hdd_operator_solve: H.solve) -- block-Jacobi preconditioned conjugate gradients on the theta-fused
operator -- against the downloaded host arrays.

Reference: the dense / scipy matrix of sum_q theta_q vals_q of the downloaded arrays (sliced for a block), and a plain
numpy PCG on it with the same preconditioner (inverse diagonal blocks) and the same stopping rule (recurrence residual
||r|| <= rtol ||b||).  CG needs a positive definite matrix and SWIPDG with the reference's penalties is indefinite on
stretched elements under the SPE10 contrast, so every case asserts lambda_min > 0 of its dense host
matrix itself (numpy.linalg.eigvalsh): an input condition.

Per case:  status CONVERGED;  true residual ||b - A x|| <= 2 rtol ||b|| on the host (true and recurrence residual of
the reference agree to 3 digits on these matrices: the 2 is slack for the rounding order);  the derived error bound
||x - x*|| <= ||b - A x|| / lambda_min;  info.residual == history[iterations];  history[0] == ||b|| within
gamma_n ||b||;  iterations <= it_ref + max(3, it_ref / 10) of the numpy PCG on the same arrays (rounding order moves
the count by a few iterations -- 608 and 586 on the two paths against 614 on SPE10 P1, equal counts on the other
cases; a preconditioner that is not applied, a stale beta or a dropped partial sum move it by factors: on OS2014 151
iterations with the block-Jacobi preconditioner, 308 without).  The homogeneous ESV2007 matrix is not used for this
assertion (the preconditioner makes too little difference there).
"""
import numpy as np
import pytest

from cases import SPE10_LOWER, SPE10_UPPER, os2014_components
from test_gpu_apply import Case, gamma

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

RTOL = 1e-8


def _torch():
    import torch
    return torch


def numpy_pcg(A, b, bs, rtol, max_iter=20000, x0=None):
    """PCG with the inverse diagonal blocks of bs rows (bs None: no preconditioner); stops when the recurrence
    residual ||r|| <= rtol ||b||.  Returns x, iterations."""
    n = b.shape[0]
    if bs:
        D = np.stack([A[i:i + bs, i:i + bs].toarray() for i in range(0, n, bs)])
        Dinv = np.linalg.inv(D)
        prec = lambda r: np.einsum("bij,bj->bi", Dinv, r.reshape(-1, bs)).reshape(-1)
    else:
        prec = lambda r: r
    x = np.zeros(n) if x0 is None else x0.copy()
    r = b - A @ x
    z = prec(r)
    p = z.copy()
    rho = r @ z
    stop = rtol * np.linalg.norm(b)
    it = 0
    while np.linalg.norm(r) > stop and it < max_iter:
        q = A @ p
        alpha = rho / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = prec(r)
        rho_new = r @ z
        p = z + (rho_new / rho) * p
        rho = rho_new
        it += 1
    return x, it


class Problem:
    """a case with its host matrix at theta, lambda_min, x*, b = A x* and the numpy reference counts (computed once)"""

    def __init__(self, c, theta, bs, seed):
        self.c, self.theta, self.bs = c, theta, bs
        th = np.ones(len(c.hvals)) if theta is None else np.asarray(theta, np.float64)
        self.A = sp.csr_matrix((sum(t * v for t, v in zip(th, c.hvals)), c.col, c.rp), shape=(c.n_rows, c.n_cols))
        self.lmin = float(np.linalg.eigvalsh(self.A.toarray())[0])
        self.xs = np.random.default_rng(seed).standard_normal(c.n_rows)
        self.b = self.A @ self.xs
        self._ref = {}

    def ref_iterations(self, bs):
        if bs not in self._ref:
            self._ref[bs] = numpy_pcg(self.A, self.b, bs, RTOL)[1]
        return self._ref[bs]


_PROBLEMS = {}


def problem(ctx, name):
    if name in _PROBLEMS:
        return _PROBLEMS[name]
    if name == "p1":        # 672 elements: 10.5 tiles
        p = Problem(Case(ctx, H.Grid.structured(H.SIMPLEX, 42, 8, SPE10_LOWER, SPE10_UPPER)), None, 3, 1)
    elif name == "q1":      # 387 elements: 6 tiles + 3 elements
        p = Problem(Case(ctx, H.Grid.structured(H.CUBE, 43, 9, SPE10_LOWER, SPE10_UPPER)), None, 4, 2)
    elif name == "os2014":  # two components, never lincombed
        fns = [H.scalar_fn(H.FN_SINUSOID, a, b, kx, ky, order=3) for (a, b, kx, ky) in os2014_components()]
        c = Case(ctx, H.Grid.structured(H.SIMPLEX, 16, 16, (-1, -1), (1, 1)), kappas=fns, tensor=H.tensor_fn())
        p = Problem(c, [1.0, 0.5], 3, 3)
    elif name == "hex_q1":
        c = Case(ctx, H.Grid.structured3d((4, 4, 4), degree=1), tensor=H.tensor_fn(dim=3), prm=H.params_for(1, 3))
        p = Problem(c, None, 8, 4)
    elif name == "hex_q2":
        c = Case(ctx, H.Grid.structured3d((3, 3, 3), degree=2), tensor=H.tensor_fn(dim=3), prm=H.params_for(2, 3))
        p = Problem(c, None, 1, 5)
    elif name == "p1_block":
        p = Problem(Case(ctx, H.Grid.structured(H.SIMPLEX, 40, 8, SPE10_LOWER, SPE10_UPPER, px=2, py=2)), None, 3, 6)
    elif name == "esv8":
        p = Problem(Case(ctx, H.Grid.structured(H.SIMPLEX, 8, 8, (-1, -1), (1, 1)), tensor=H.tensor_fn()), None, 3, 7)
    else:
        raise KeyError(name)
    _PROBLEMS[name] = p
    return p


def dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def check_solution(A, lmin, b, xs, x, info, it_ref, rtol=RTOL):
    """the per-case assertions of the module docstring"""
    assert lmin > 0, "input condition: the host matrix is not positive definite (lambda_min %g)" % lmin
    xh = x.cpu().numpy()
    nb = np.linalg.norm(b)
    true_res = np.linalg.norm(b - A @ xh)
    err = np.linalg.norm(xh - xs)
    print("iterations %d (numpy %d), ||r|| %.3e, true %.3e, 2 rtol ||b|| %.3e, error %.3e <= %.3e"
          % (info.iterations, it_ref, info.residual, true_res, 2 * rtol * nb, err, true_res / lmin))
    assert info.status == H.SOLVE_CONVERGED, (info.status, info.iterations, info.residual)
    assert np.isfinite(xh).all()
    assert true_res <= 2.0 * rtol * nb, (true_res, rtol * nb)
    assert err <= true_res / lmin, (err, true_res / lmin)
    assert info.residual <= rtol * nb * (1 + 1e-12)
    assert info.iterations <= it_ref + max(3, it_ref / 10), (info.iterations, it_ref)
    assert abs(info.rhs_norm - nb) <= gamma(b.shape[0] + 2) * nb
    if info.history is not None:
        h = info.history.cpu().numpy()
        assert h.shape == (info.iterations + 1,)
        assert h[info.iterations] == info.residual
        assert abs(h[0] - nb) <= gamma(b.shape[0] + 2) * nb


@pytest.mark.parametrize("name,path,bs,kernels", [
    ("p1", "tile", 0, "apply_tile_kernel<3, 3, 1, dot> + cg_update<3> + cg_direction"),
    ("p1", "csr", 0, "apply_csr_kernel<8, 1, dot> + cg_update<3> + cg_direction"),
    ("q1", "tile", 0, "apply_tile_kernel<4, 4, 1, dot> + cg_update<4> + cg_direction"),
    ("q1", "csr", 0, "apply_csr_kernel<8, 1, dot> + cg_update<4> + cg_direction"),
    ("os2014", "tile", 0, "apply_tile_kernel<3, 3, 1, dot> + cg_update<3> + cg_direction"),
    ("hex_q1", "csr", 8, "apply_csr_kernel<64, 1, dot> + cg_update<8> + cg_direction"),
    ("hex_q2", "csr", 1, "apply_csr_kernel<64, 1, dot> + cg_update<1> + cg_direction"),
])
def test_solve(ctx, name, path, bs, kernels):
    """SPE10 Kuhn P1 42 x 8 (10.5 tiles) and Q1 43 x 9 (6 tiles + 3 elements) on both paths; OS2014 16 x 16 with
    theta = (1, 0.5) fused; hexahedra Q1 4^3 with blocks of 8 and Q2 3^3 with the point Jacobi (block_size 1)"""
    P = problem(ctx, name)
    c = P.c
    if name == "p1":
        assert c.local.n_own == 672 and c.local.n_own % 64 == 32
    if name == "q1":
        assert c.local.n_own == 387 and c.local.n_own % 64 == 3
    x, info = H.solve(ctx, c.dp, c.vals, dev(P.b), theta=P.theta, dmesh=c.dm if path == "tile" else None,
                      block_size=bs, rtol=RTOL, history=True)
    assert H.last_solve_kernels() == kernels
    check_solution(P.A, P.lmin, P.b, P.xs, x, info, P.ref_iterations(P.bs))


@pytest.mark.parametrize("ss", [0, 1, 2, 3])
def test_local_solves(ctx, ss):
    """SPE10 Kuhn 40 x 8 in 2 x 2 subdomains: the local solve on get_local_operator(ss) through the block range, on
    the global arrays, against the sliced host matrix"""
    P = problem(ctx, "p1_block")
    c = P.c
    a, b = c.grid.subdomain_range(ss, ss + 1)
    A = P.A[3 * a:3 * b, 3 * a:3 * b].tocsr()
    lmin = float(np.linalg.eigvalsh(A.toarray())[0])
    xs = np.random.default_rng(20 + ss).standard_normal(A.shape[0])
    rhs = A @ xs
    x, info = H.solve(ctx, c.dp, c.vals, dev(rhs), dmesh=c.dm, block=(ss, ss), rtol=RTOL, history=True)
    assert H.last_solve_kernels().startswith("apply_tile_kernel<3, 3, 1, dot>")
    assert x.shape == (3 * (b - a),)
    check_solution(A, lmin, rhs, xs, x, info, numpy_pcg(A, rhs, 3, RTOL)[1])


@pytest.mark.parametrize("name,path", [("p1", "tile"), ("q1", "csr")])
def test_check_every_and_determinism(ctx, name, path):
    """the number of iterations enqueued between two looks changes only the number of empty launches"""
    torch = _torch()
    P = problem(ctx, name)
    c = P.c
    dm = c.dm if path == "tile" else None
    runs = [H.solve(ctx, c.dp, c.vals, dev(P.b), dmesh=dm, rtol=RTOL, check_every=ce) for ce in (1, 50, 50, 0)]
    x1, i1 = runs[0]
    assert i1.status == H.SOLVE_CONVERGED and i1.iterations > 50
    for x, i in runs[1:]:
        assert torch.equal(x, x1)
        assert (i.status, i.iterations, i.residual, i.rhs_norm) == (i1.status, i1.iterations, i1.residual, i1.rhs_norm)


def test_no_preconditioner(ctx):
    P = problem(ctx, "os2014")
    c = P.c
    x, info = H.solve(ctx, c.dp, c.vals, dev(P.b), theta=P.theta, dmesh=c.dm, precond="none", rtol=RTOL, history=True)
    assert H.last_solve_kernels() == "apply_tile_kernel<3, 3, 1, dot> + cg_update<3, none> + cg_direction"
    it_none = P.ref_iterations(None)
    check_solution(P.A, P.lmin, P.b, P.xs, x, info, it_none)
    assert it_none > 1.5 * P.ref_iterations(3)          # the gap the preconditioner makes on this matrix
    assert info.iterations > P.ref_iterations(3) + max(3, P.ref_iterations(3) / 10)
    # ... and on the CSR path without any mesh (block_size 1 implied)
    x2, info2 = H.solve(ctx, H.CsrPattern(c.dp.row_ptr, c.dp.col, c.n_cols), c.vals, dev(P.b), theta=P.theta,
                        precond="none", rtol=RTOL)
    assert H.last_solve_kernels() == "apply_csr_kernel<8, 1, dot> + cg_update<1, none> + cg_direction"
    check_solution(P.A, P.lmin, P.b, P.xs, x2, info2, it_none)


def test_warm_start(ctx):
    torch = _torch()
    P = problem(ctx, "p1")
    c = P.c
    b = dev(P.b)
    # x0 = x*: ||b - A x0|| is the rounding of one apply, far below rtol ||b||
    x, info = H.solve(ctx, c.dp, c.vals, b, dmesh=c.dm, x0=dev(P.xs), rtol=RTOL)
    assert (info.status, info.iterations) == (H.SOLVE_CONVERGED, 0)
    assert torch.equal(x, dev(P.xs))
    K = np.diff(P.A.indptr).max() + 3
    assert info.residual <= 2 * gamma(K) * np.linalg.norm(abs(P.A) @ np.abs(P.xs)) + gamma(K) * np.linalg.norm(P.b)
    # a looser solve's x as the initial guess: fewer iterations than from zero, same answer quality
    cold, icold = H.solve(ctx, c.dp, c.vals, b, dmesh=c.dm, rtol=RTOL)
    loose, iloose = H.solve(ctx, c.dp, c.vals, b, dmesh=c.dm, rtol=1e-4)
    warm, iwarm = H.solve(ctx, c.dp, c.vals, b, dmesh=c.dm, x0=loose, rtol=RTOL, history=True)
    assert iloose.status == iwarm.status == H.SOLVE_CONVERGED
    assert 0 < iwarm.iterations < icold.iterations
    assert np.linalg.norm(P.b - P.A @ warm.cpu().numpy()) <= 2 * RTOL * np.linalg.norm(P.b)
    loose_res = np.linalg.norm(P.b - P.A @ loose.cpu().numpy())
    assert abs(iwarm.history[0].item() - loose_res) <= 1e-6 * loose_res      # r0 = b - A x0
    # b = 0
    for x0 in (None, dev(P.xs)):
        x, info = H.solve(ctx, c.dp, c.vals, torch.zeros_like(b), dmesh=c.dm, x0=x0, rtol=RTOL)
        assert (info.status, info.iterations, info.residual, info.rhs_norm) == (H.SOLVE_CONVERGED, 0, 0.0, 0.0)
        assert not bool(x.any())


def test_breakdown_and_max_iter_without_any_fault(ctx):
    torch = _torch()
    E = problem(ctx, "esv8")
    c = E.c
    assert E.lmin > 0                         # so -A is negative definite: every pivot of every block is negative
    for dm in (c.dm, None):
        x, info = H.solve(ctx, c.dp, c.vals, dev(E.b), theta=[-1.0], dmesh=dm, rtol=RTOL)
        assert (info.status, info.iterations) == (H.SOLVE_BREAKDOWN, 0)
        assert bool(torch.isfinite(x).all())
    # without the preconditioner the breakdown is p . Ap <= 0 in the first iteration: x stays the initial guess
    x, info = H.solve(ctx, c.dp, c.vals, dev(E.b), theta=[-1.0], dmesh=c.dm, precond="none", rtol=RTOL)
    assert (info.status, info.iterations) == (H.SOLVE_BREAKDOWN, 0)
    assert not bool(x.any())
    P = problem(ctx, "p1")
    x, info = H.solve(ctx, P.c.dp, P.c.vals, dev(P.b), dmesh=P.c.dm, rtol=RTOL, max_iter=3, history=True)
    assert (info.status, info.iterations) == (H.SOLVE_MAX_ITER, 3)
    assert info.history.shape == (4,) and info.history[3].item() == info.residual
    ref = numpy_pcg(P.A, P.b, 3, 0.0, max_iter=3)[0]
    assert np.linalg.norm(x.cpu().numpy() - ref) <= 1e-10 * np.linalg.norm(ref)
    x0, info0 = H.solve(ctx, P.c.dp, P.c.vals, dev(P.b), dmesh=P.c.dm, rtol=RTOL, max_iter=0)
    assert (info0.status, info0.iterations) == (H.SOLVE_MAX_ITER, 0) and not bool(x0.any())


@pytest.mark.parametrize("name,path", [("p1", "tile"), ("p1", "csr"), ("q1", "tile")])
def test_padded_right_hand_side(ctx, name, path):
    """b (and x0) inside NaN padding, 8 bytes off a 16-byte boundary: nothing outside the vectors is read -- the
    result is that of the plain call, bit for bit -- and nothing outside is written"""
    torch = _torch()
    P = problem(ctx, name)
    c = P.c
    dm = c.dm if path == "tile" else None
    n = c.n_rows
    plain, iplain = H.solve(ctx, c.dp, c.vals, dev(P.b), dmesh=dm, rtol=RTOL)
    buf = torch.full((n + 8,), float("nan"), dtype=torch.float64, device="cuda")
    buf[1:n + 1] = dev(P.b)
    assert buf[1:].data_ptr() % 16 == 8
    x, info = H.solve(ctx, c.dp, c.vals, buf[1:n + 1], dmesh=dm, rtol=RTOL)
    assert torch.equal(x, plain) and info.iterations == iplain.iterations
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[n + 1:]).all())
    assert torch.equal(buf[1:n + 1], dev(P.b))
    xbuf = torch.full((n + 8,), float("nan"), dtype=torch.float64, device="cuda")
    xbuf[3:n + 3] = 0.0
    x, info = H.solve(ctx, c.dp, c.vals, buf[1:n + 1], dmesh=dm, x0=xbuf[3:n + 3], rtol=RTOL)
    assert bool(torch.isfinite(x).all()) and info.status == H.SOLVE_CONVERGED
    assert abs(info.iterations - iplain.iterations) <= 3
    assert bool(torch.isnan(xbuf[:3]).all()) and bool(torch.isnan(xbuf[n + 3:]).all())
