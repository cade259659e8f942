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

The second half of the file takes the same assertions through what no mesh's own block size reaches: block sizes 1,
2, 5, 6, 7 (numpy PCG with blocks of the same size as the reference), x and the workspace 8 bytes off a 16-byte
boundary through the C ABI (the scalar-load instantiations of the even block sizes), block ranges on the CSR path and
over several subdomains, hexahedral local solves, two fused components without a mesh, and atol.  The reductions past
64 partial sums and the multi-pass grids are test_gpu_solve_grid.py's.
"""
import ctypes as C

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


def diag_blocks_by_slices(A, bs):
    """[n / bs, bs, bs]: the diagonal blocks of A, one scipy slice at a time (minutes beyond 10^5 blocks)"""
    return np.stack([A[i:i + bs, i:i + bs].toarray() for i in range(0, A.shape[0], bs)])


def diag_blocks(A, bs):
    """the same blocks from the block-CSR form of A, without a Python loop; a block row without a diagonal block
    gives zeros (test_diag_blocks_extraction: bit for bit diag_blocks_by_slices)"""
    n_blk = A.shape[0] // bs
    B = A.tobsr(blocksize=(bs, bs))
    row = np.repeat(np.arange(n_blk), np.diff(B.indptr))
    on_diag = B.indices == row
    D = np.zeros((n_blk, bs, bs))
    D[row[on_diag]] = B.data[on_diag]
    return D


def numpy_pcg(A, b, bs, rtol, max_iter=20000, x0=None):
    """PCG with the inverse diagonal blocks of bs rows (bs None: no preconditioner); stops when the recurrence
    residual ||r|| <= rtol ||b||.  Returns x, iterations."""
    n = b.shape[0]
    if bs:
        Dinv = np.linalg.inv(diag_blocks(A, bs))
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
    elif name == "hex_block":   # two x-slabs of 32 hexahedra
        c = Case(ctx, H.Grid.structured3d((4, 4, 4), p=(2, 1, 1), degree=1), tensor=H.tensor_fn(dim=3),
                 prm=H.params_for(1, 3))
        p = Problem(c, None, 8, 8)
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


# ---- every block size of the launch switch, and the dispatch combinations, at the sizes above ----

def test_diag_blocks_extraction(ctx):
    """the reference's vectorised block extraction against the slice loop it replaced, bit for bit"""
    P = problem(ctx, "p1")
    for bs in (1, 2, 3, 6, 7, 8):
        assert P.A.shape[0] % bs == 0
        assert np.array_equal(diag_blocks(P.A, bs), diag_blocks_by_slices(P.A, bs)), bs
    # a block row without its diagonal block: zeros both ways
    A = P.A.tolil()
    A[3:6, 3:6] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    assert np.array_equal(diag_blocks(A, 3), diag_blocks_by_slices(A, 3)) and not diag_blocks(A, 3)[1].any()


@pytest.mark.parametrize("name,path,bs", [
    ("p1", "csr", 2), ("p1", "csr", 6), ("p1", "csr", 7),      # 2,016 rows: multiples of all three
    ("p1", "tile", 6), ("p1", "tile", 1),                      # tile apply, blocks from the CSR arrays (bs != nb)
    ("p1_block", "csr", 5), ("p1_block", "tile", 5),           # 1,920 rows, the whole matrix
    ("q1", "csr", 2), ("q1", "tile", 2),
])
def test_block_sizes(ctx, name, path, bs):
    """cg_init / cg_update / solve_dinv_csr / solve_invert / solve_precond at the block sizes no mesh has, against
    the numpy PCG with blocks of the same size"""
    P = problem(ctx, name)
    c = P.c
    assert c.n_rows % bs == 0 and bs != c.grid.nb
    x, info = H.solve(ctx, c.dp, c.vals, dev(P.b), dmesh=c.dm if path == "tile" else None, block_size=bs, rtol=RTOL,
                      history=True)
    nb = c.grid.nb
    apply = "apply_tile_kernel<%d, %d, 1, dot>" % (nb, nb) if path == "tile" else "apply_csr_kernel<8, 1, dot>"
    assert H.last_solve_kernels() == apply + " + cg_update<%d> + cg_direction" % bs
    check_solution(P.A, P.lmin, P.b, P.xs, x, info, P.ref_iterations(bs))


def _raw_solve(ctx, c, b, dm, bs, shift):
    """hdd_operator_solve through ctypes with x and the workspace `shift` doubles past a 16-byte boundary, inside
    NaN; returns x, (status, iterations, residual, rhs_norm) after checking that nothing around them was written"""
    torch = _torch()
    rows = c.n_rows
    n_work = int(H.lib().hdd_operator_solve_workspace(rows, bs))
    xbuf = torch.full((rows + 8,), float("nan"), dtype=torch.float64, device="cuda")
    wbuf = torch.full((n_work + 8,), float("nan"), dtype=torch.float64, device="cuda")
    x, w = xbuf[2 + shift:2 + shift + rows], wbuf[2 + shift:2 + shift + n_work]
    assert x.data_ptr() % 16 == 8 * shift and w.data_ptr() % 16 == 8 * shift
    ptrs = (C.c_void_p * 1)(c.vals[0].data_ptr())
    opt = H.SolveOptions(RTOL, 0.0, 10000, 0, H.PRECOND_BLOCK_JACOBI, bs, 0, 0)
    info = H.SolveInfo()
    rc = H.lib().hdd_operator_solve(ctx.h, None if dm is None else C.addressof(dm.t), C.addressof(c.dp.t), ptrs, 1, None,
                                    None, b.data_ptr(), x.data_ptr(), C.addressof(opt), w.data_ptr(), n_work, None,
                                    C.addressof(info), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, H.lib().hdd_last_error(None)
    torch.cuda.synchronize()
    for buf, n in ((xbuf, rows), (wbuf, n_work)):
        assert bool(torch.isnan(buf[:2 + shift]).all()) and bool(torch.isnan(buf[2 + shift + n:]).all())
    return x.clone(), (info.status, info.iterations, info.residual, info.rhs_norm)


@pytest.mark.parametrize("path", ["csr", "tile"])
@pytest.mark.parametrize("bs", [2, 4, 8])
def test_unaligned_x_and_workspace(ctx, path, bs):
    """H.solve always allocates x and the workspace 16-byte aligned, so the even block sizes only ever take the
    16-byte loads (A16).  Through the C ABI with both one double off: the scalar-load instantiations -- the same
    arithmetic in the same order, so the same bits; nothing outside x and the workspace is written"""
    torch = _torch()
    P = problem(ctx, "p1")
    c = P.c
    dm = c.dm if path == "tile" else None
    b = dev(P.b)
    xa, ia = _raw_solve(ctx, c, b, dm, bs, 0)
    assert H.last_solve_kernels().endswith("cg_update<%d> + cg_direction" % bs)
    xu, iu = _raw_solve(ctx, c, b, dm, bs, 1)
    assert ia[0] == H.SOLVE_CONVERGED and iu == ia
    assert bool(torch.isfinite(xa).all()) and torch.equal(xu, xa)
    # ... and it is the solution: the front end's (aligned) call gives the same bits, checked in full
    x, info = H.solve(ctx, c.dp, c.vals, b, dmesh=dm, block_size=bs, rtol=RTOL, history=True)
    assert torch.equal(x, xa) and info.iterations == ia[1]
    check_solution(P.A, P.lmin, P.b, P.xs, x, info, P.ref_iterations(bs))


def _range_solve(ctx, P, rng, block, dm, bs, kernels, seed):
    """solve on the rows = columns rng[0]..rng[1] of P's global arrays against the sliced host matrix"""
    c = P.c
    A = P.A[rng[0]:rng[1], rng[0]:rng[1]].tocsr()
    lmin = float(np.linalg.eigvalsh(A.toarray())[0])
    xs = np.random.default_rng(seed).standard_normal(A.shape[0])
    rhs = A @ xs
    x, info = H.solve(ctx, c.dp, c.vals, dev(rhs), dmesh=dm, block=block, block_size=bs, rtol=RTOL, history=True)
    assert H.last_solve_kernels() == kernels + " + cg_direction"
    assert x.shape == (rng[1] - rng[0],)
    check_solution(A, lmin, rhs, xs, x, info, numpy_pcg(A, rhs, bs or c.grid.nb, RTOL)[1])


@pytest.mark.parametrize("ss", [1, 3])
def test_local_solves_on_the_csr_path(ctx, ss):
    """block=(ss, ss) without a mesh: apply_csr_kernel<8, 1, dot> and solve_dinv_csr_kernel with row_begin != 0"""
    P = problem(ctx, "p1_block")
    a, b = P.c.grid.subdomain_range(ss, ss + 1)
    assert a > 0
    _range_solve(ctx, P, (3 * a, 3 * b), (ss, ss), None, 0, "apply_csr_kernel<8, 1, dot> + cg_update<3>", 30 + ss)


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_range_over_two_subdomains(ctx, path):
    """subdomains 1 and 2 together, given as rows and columns"""
    P = problem(ctx, "p1_block")
    a, b = P.c.grid.subdomain_range(1, 3)
    a1, b1 = P.c.grid.subdomain_range(1, 2)
    assert a == a1 > 0 and b > b1
    apply = "apply_tile_kernel<3, 3, 1, dot>" if path == "tile" else "apply_csr_kernel<8, 1, dot>"
    _range_solve(ctx, P, (3 * a, 3 * b), (3 * a, 3 * b, 3 * a, 3 * b), P.c.dm if path == "tile" else None, 0,
                 apply + " + cg_update<3>", 40)


def test_range_off_the_element_boundaries(ctx):
    """a square range that is no multiple of nb, point Jacobi: with the mesh given it still takes the CSR kernel"""
    P = problem(ctx, "p1_block")
    n = P.c.n_rows
    rng = (1, n - 4)
    assert rng[0] % 3 != 0 and rng[1] % 3 != 0
    _range_solve(ctx, P, rng, (rng[0], rng[1], rng[0], rng[1]), P.c.dm, 1, "apply_csr_kernel<8, 1, dot> + cg_update<1>", 41)


@pytest.mark.parametrize("ss", [0, 1])
def test_local_solves_hexahedra(ctx, ss):
    """BlockSWIPDG::solve_local in 3d: Q1 hexahedra 4^3 in two x-slabs, blocks of 8"""
    P = problem(ctx, "hex_block")
    c = P.c
    assert c.grid.n_sub == 2 and c.grid.nb == 8
    a, b = c.grid.subdomain_range(ss, ss + 1)
    assert b - a == 32
    _range_solve(ctx, P, (8 * a, 8 * b), (ss, ss), c.dm, 8, "apply_csr_kernel<64, 1, dot> + cg_update<8>", 50 + ss)


def test_two_components_on_the_csr_path(ctx):
    """OS2014 with theta = (1, 0.5) without a mesh: the fused components through apply_csr_kernel<8, 1, dot> and
    solve_dinv_csr_kernel<3> with n_comp = 2"""
    P = problem(ctx, "os2014")
    c = P.c
    assert len(c.vals) == 2
    x, info = H.solve(ctx, c.dp, c.vals, dev(P.b), theta=P.theta, dmesh=None, rtol=RTOL, history=True)
    assert H.last_solve_kernels() == "apply_csr_kernel<8, 1, dot> + cg_update<3> + cg_direction"
    check_solution(P.A, P.lmin, P.b, P.xs, x, info, P.ref_iterations(3))


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_atol(ctx, path):
    """the threshold is max(rtol ||b||, atol): atol alone, then each of the two deciding"""
    P = problem(ctx, "p1")
    c = P.c
    dm = c.dm if path == "tile" else None
    nb = np.linalg.norm(P.b)
    a = 1e-6 * nb

    def run(rtol, atol):
        x, info = H.solve(ctx, c.dp, c.vals, dev(P.b), dmesh=dm, rtol=rtol, atol=atol, history=True)
        return x, info, info.history.cpu().numpy()

    def stopped_at(info, h, thresh):
        assert info.status == H.SOLVE_CONVERGED and info.iterations > 0
        assert info.residual <= thresh and h[info.iterations] == info.residual
        assert h[info.iterations - 1] > thresh          # not an iteration late

    x, info, h = run(0.0, a)
    stopped_at(info, h, a)
    assert np.linalg.norm(P.b - P.A @ x.cpu().numpy()) <= 2 * a
    # both set: the larger decides
    x2, info2, h2 = run(1e-8, a)                          # atol = 1e-6 ||b|| > 1e-8 ||b||
    assert info2.iterations == info.iterations and _torch().equal(x2, x)
    x3, info3, h3 = run(1e-4, a)                          # rtol ||b|| = 1e-4 ||b|| > atol
    stopped_at(info3, h3, 1e-4 * nb * (1 + 1e-12))        # (the device's ||b|| is nb within gamma_n)
    assert info3.iterations < info.iterations
    x4, info4, _ = run(1e-4, 0.0)
    assert info4.iterations == info3.iterations and _torch().equal(x4, x3)
