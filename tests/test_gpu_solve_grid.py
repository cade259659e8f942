"""hdd_operator_solve where its reductions pass one wave stride: solve_wave_sum over more than 64 partial sums
(part_pq of the DOT apply, part_rr / part_rz / part_bb and the bad-block count of update_grid(n_blk) workgroups),
the DOT applies walking several tiles / several grid-stride passes, on the large cases of test_gpu_apply_grid.py.
test_gpu_solve.py stays at or below 63 partials of every kind but part_pq on its two small hexahedral cases.

Cases (256 CUs; the sizes follow the device, test_gpu_apply_grid.py):
  p1 tile, p1 csr   525,600 rows, 175,200 blocks of 3: ugrid 685; part_pq 2,048 (2,738 tiles / rows > 2048 * 32)
  q1 tile           263,120 rows, 65,780 blocks of 4: ugrid 257; part_pq 1,024 (1,028 tiles)
  hex csr           69,120 rows, 8,640 blocks of 8: part_pq 2,048 (rows > 2048 * 4).  Its ugrid is 34: 64 workgroups
                    of cg_update need 16,385 blocks, which this mesh does not have, so on this case only part_pq
                    (and the apply's second pass) passes 64; the assertion ugrid > 64 is made for the 2d cases.

Positive definiteness (an input condition, asserted): eigvalsh of a dense matrix is not affordable here, so every
diagonal block's Cholesky factorisation must succeed on the host and p.Ap and r.z of the reference PCG must stay
positive over the iterations used.  The large P1 matrix (SPE10 checkerboard tensor, the reference's penalties) and
the hexahedral one pass as they are: neither the x4 penalties of scripts/bench_solve.py nor the homogeneous tensor
was needed.  The Q1 mesh has elements 4.9 times as wide as high; with the reference's penalties 63,191 of its 65,780
diagonal blocks are not positive definite (smallest block eigenvalue -686), with both penalties times 4 (SIGMA_SCALE
in test_gpu_apply_grid.py, as scripts/bench_solve.py does) all are (smallest 3.7e-3) and p.Ap, r.z stay positive.

Nothing iterates to convergence: a dropped or duplicated partial sum changes alpha or beta by a large factor in the
first iteration, while rounding-order differences stay small for a few iterations.

After setup (max_iter = 0): info.rhs_norm and history[0] are ||b|| within gamma_{n+2} ||b|| (n products, n additions
in any order, the root).

After one iteration, against a step in np.longdouble (whose own rounding, 2^-64, is neglected beside 2^-53).  With
x0 = 0: r0 = b, z0 = D^-1 b, p0 = z0, alpha = r0.z0 / p0.A p0, x1 = alpha z0, r1 = b - alpha A z0.  First-order
bounds, u = 2^-53, K the longest row + n_comp + 2 as in test_gpu_apply.py:
  z0      the device inverts each block by Gauss-Jordan elimination in double and applies it with bs fmas:
          |dz| <= ez := 8 bs^3 u |D^-1||D||D^-1||b| + gamma_bs |D^-1||b|
          (Higham, Accuracy and Stability, 14.4: 8 n^3 u kappa for Gauss-Jordan on a definite matrix, here with the
          componentwise condition; the blocks' host inverse is in longdouble)
  r.z     n rounded products summed in some order, and z's own error:  gamma_{n+1} |r|.|z| + |r|.ez
  p.Ap    gamma_{n+K} |p|.|A||p| + 2 ez.|A||p|
  alpha   relative: gamma_{n+1} |r|.|z| / r.z + gamma_{n+K} |p|.|A||p| / p.Ap + (the ez terms) + u for the division
          -- the two condition factors |r|.|z| / r.z and |p|.|A||p| / p.Ap are printed
  x1      |dx1| <= (rel(alpha) + u) |x1| + |alpha| ez                   (one more rounding), per entry
  r1      |dr1| <= rel(alpha) |alpha q| + |alpha| (gamma_K |A||p| + |A| ez) + u |r1|, and
          |history[1] - ||r1||| <= ||dr1||_2 + gamma_{n+2} ||r1||
each times 1.01 for the second-order terms.

After 10 iterations: x against numpy_pcg(..., rtol=0, max_iter=10) in float64.  The tolerance is measured on the
reference, not on the device: d = ||x_float64 - x_longdouble|| / ||x_longdouble|| of the same 10 iterations on the
host, and the device may differ from the float64 reference by max(100 d, 1e-13) ||x_ref|| -- the 100 for the
device's summation order (a two-stage tree against numpy's pairwise sums).  d and the device's difference are
printed.
"""
import numpy as np
import pytest

from test_gpu_apply import gamma
from test_gpu_apply_grid import grid_case, grid_facts, tile_grid
from test_gpu_solve import dev, diag_blocks, numpy_pcg

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
K_ITER = 10
SOLVE_PARTS = 4096
CASES = [("p1", "tile"), ("p1", "csr"), ("q1", "tile"), ("hex", "csr")]


def _torch():
    import torch
    return torch


def update_grid(n_blk):
    """abi_solve.hip: workgroups of cg_init / cg_update / solve_dinv (= partial sums of r.r, r.z, b.b, bad blocks)"""
    return max(1, min((n_blk + 255) // 256, 2048))


def dot_grid(name, path, rows, n_tiles):
    """abi_solve.hip: workgroups of the DOT apply (= partial sums of p.q)"""
    if path == "tile":
        G = tile_grid(8 if name == "p1" else 4, n_tiles)
        return G if G <= SOLVE_PARTS else SOLVE_PARTS & ~7
    per_wg = 4 if name == "hex" else 32
    return min((rows + per_wg - 1) // per_wg, 16384, 2048)


def invert_blocks(D):
    """inverse of every block of D [n, bs, bs] by Gauss-Jordan elimination in D's own precision (numpy.linalg has no
    longdouble); the blocks are positive definite, so no pivoting"""
    n, bs, _ = D.shape
    M = np.concatenate([D.copy(), np.broadcast_to(np.eye(bs, dtype=D.dtype), D.shape).copy()], axis=2)
    for k in range(bs):
        M[:, k, :] /= M[:, k, k][:, None]
        for i in range(bs):
            if i != k:
                M[:, i, :] -= M[:, i, k][:, None] * M[:, k, :]
    return M[:, :, bs:]


def bmv(M, v):
    """block-diagonal M [n, bs, bs] times v [n bs], without einsum's object fallback for longdouble"""
    bs = M.shape[1]
    return (M * v.reshape(-1, 1, bs)).sum(axis=2).reshape(-1)


class GridProblem:
    """host side of one large case, computed once: the matrix, its diagonal blocks (Cholesky checked), b, and the
    reference iterations in float64 and longdouble"""

    def __init__(self, c, name, bs, seed):
        self.c, self.name, self.bs, self._first = c, name, bs, None
        self.rows, self.n_tiles, self.G = grid_facts(c, name)
        self.A = sp.csr_matrix((c.hvals[0], c.col, c.rp), shape=(c.n_rows, c.n_cols))
        self.D = diag_blocks(self.A, bs)
        np.linalg.cholesky(self.D)                       # raises LinAlgError if a block is not positive definite
        self.b = self.A @ np.random.default_rng(seed).standard_normal(c.n_rows)
        self.K = int(np.diff(c.rp).max()) + 3
        # longdouble: the matrix, the inverse blocks, K_ITER iterations of PCG with p.Ap and r.z of every iteration
        self.Al = self.A.astype(LD)
        self.Dinv_l = invert_blocks(self.D.astype(LD))
        self.bl = self.b.astype(LD)
        self.xl, self.pq, self.rz = self.pcg_longdouble(K_ITER)
        assert all(v > 0 for v in self.pq) and all(v > 0 for v in self.rz), (self.pq, self.rz)
        self.x64 = numpy_pcg(self.A, self.b, bs, 0.0, max_iter=K_ITER)[0]
        self.d = float(np.sqrt(((self.x64 - self.xl) ** 2).sum()) / np.sqrt((self.xl ** 2).sum()))

    def pcg_longdouble(self, iters):
        A, b, Dinv = self.Al, self.bl, self.Dinv_l
        x = np.zeros(b.shape[0], LD)
        r = b.copy()
        z = bmv(Dinv, r)
        p = z.copy()
        rho = r @ z
        pqs, rzs = [], [rho]
        for _ in range(iters):
            q = A @ p
            pq = p @ q
            pqs.append(pq)
            alpha = rho / pq
            x += alpha * p
            r -= alpha * q
            z = bmv(Dinv, r)
            rho_new = r @ z
            rzs.append(rho_new)
            p = z + (rho_new / rho) * p
            rho = rho_new
        assert x.dtype == LD and np.finfo(LD).eps < 2.0 ** -60, "np.longdouble is not wider than float64 here"
        return x, pqs, rzs

    def first_step(self):
        """the first iteration in longdouble with the bounds of the module docstring (computed once)"""
        if self._first is not None:
            return self._first
        P = self
        n, bs, K = P.rows, P.bs, P.K
        b, A = P.bl, P.Al
        absA, absb = abs(A), np.abs(b)
        Dl, Dinv = P.D.astype(LD), P.Dinv_l
        z = bmv(Dinv, b)
        ez = LD(8 * bs ** 3 * U) * bmv(np.abs(Dinv), bmv(np.abs(Dl), bmv(np.abs(Dinv), absb))) \
            + LD(gamma(bs)) * bmv(np.abs(Dinv), absb)
        q = A @ z
        Aabsz = absA @ np.abs(z)
        rho, pq = b @ z, z @ q
        assert rho > 0 and pq > 0
        c1, c2 = (absb @ np.abs(z)) / rho, (np.abs(z) @ Aabsz) / pq
        rel_alpha = (LD(gamma(n + 1)) * c1 + (absb @ ez) / rho) + (LD(gamma(n + K)) * c2 + 2 * (ez @ Aabsz) / pq) + U
        alpha = rho / pq
        x1 = alpha * z
        r1 = b - alpha * q
        h1 = np.sqrt((r1 * r1).sum())
        bound_x = 1.01 * ((rel_alpha + U) * np.abs(x1) + abs(alpha) * ez)
        dr1 = rel_alpha * np.abs(alpha * q) + abs(alpha) * (LD(gamma(K)) * Aabsz + absA @ ez) + U * np.abs(r1)
        bound_h = 1.01 * (np.sqrt((dr1 * dr1).sum()) + LD(gamma(n + 2)) * h1)
        self._first = (c1, c2, rel_alpha, x1, h1, bound_x, bound_h)
        return self._first

    def solve(self, ctx, path, **kw):
        c = self.c
        return H.solve(ctx, c.dp, c.vals, dev(self.b), dmesh=c.dm if path == "tile" else None, block_size=self.bs,
                       rtol=0.0, **kw)


_PROBLEMS = {}


def grid_problem(ctx, name):
    if name not in _PROBLEMS:
        bs, seed = {"p1": (3, 61), "q1": (4, 62), "hex": (8, 63)}[name]
        _PROBLEMS[name] = GridProblem(grid_case(ctx, name), name, bs, seed)
    return _PROBLEMS[name]


def partial_counts(P, name, path):
    """(ugrid, part_pq count) with the input conditions of the module docstring"""
    ugrid = update_grid(P.rows // P.bs)
    n_pq = dot_grid(name, path, P.rows, P.n_tiles)
    assert n_pq > 64, n_pq
    if name != "hex":
        assert ugrid > 64, ugrid
    if path == "csr":       # the DOT launch is capped at 2,048 workgroups: more than one pass
        assert n_pq == 2048 and P.rows > 2048 * (4 if name == "hex" else 32)
    else:
        assert P.n_tiles > n_pq
    return ugrid, n_pq


def expected_kernels(name, path, bs):
    apply = {"p1": "apply_tile_kernel<3, 3, 1, dot>", "q1": "apply_tile_kernel<4, 4, 1, dot>"}[name] if path == "tile" \
        else ("apply_csr_kernel<64, 1, dot>" if name == "hex" else "apply_csr_kernel<8, 1, dot>")
    return apply + " + cg_update<%d> + cg_direction" % bs


@pytest.mark.parametrize("name,path", CASES)
def test_setup_norms(ctx, name, path):
    """max_iter = 0: ||b|| from part_bb and history[0] from part_rr, each summed over ugrid partials"""
    P = grid_problem(ctx, name)
    ugrid, n_pq = partial_counts(P, name, path)
    x, info = P.solve(ctx, path, max_iter=0, history=True)
    assert H.last_solve_kernels() == expected_kernels(name, path, P.bs)
    assert (info.status, info.iterations) == (H.SOLVE_MAX_ITER, 0) and not bool(x.any())
    nb = float(np.sqrt((P.bl * P.bl).sum()))
    tol = float(gamma(P.rows + 2)) * nb
    h0 = info.history[0].item()
    print("%s %s: rows %d, ugrid %d, part_pq %d, ||b|| error %.3e, history[0] error %.3e, bound %.3e"
          % (name, path, P.rows, ugrid, n_pq, abs(info.rhs_norm - nb), abs(h0 - nb), tol))
    assert abs(info.rhs_norm - nb) <= tol
    assert abs(h0 - nb) <= tol and info.residual == h0


@pytest.mark.parametrize("name,path", CASES)
def test_first_iteration(ctx, name, path):
    """max_iter = 1 against the longdouble step, under the bounds derived in the module docstring"""
    P = grid_problem(ctx, name)
    partial_counts(P, name, path)
    c1, c2, rel_alpha, x1, h1, bound_x, bound_h = P.first_step()

    x, info = P.solve(ctx, path, max_iter=1, history=True)
    assert (info.status, info.iterations) == (H.SOLVE_MAX_ITER, 1)
    xh = x.cpu().numpy()
    assert np.isfinite(xh).all()
    err = np.abs(xh.astype(LD) - x1)
    hd = info.history[1].item()
    print("%s %s: |r|.|z| / r.z = %.3f, |p|.|A||p| / p.Ap = %.3f, rel(alpha) bound %.3e; worst |dx1| / bound %.3e; "
          "history[1] %.6e, off by %.3e, bound %.3e"
          % (name, path, float(c1), float(c2), float(rel_alpha), float((err[bound_x > 0] / bound_x[bound_x > 0]).max()),
             hd, float(abs(LD(hd) - h1)), float(bound_h)))
    bad = err > bound_x
    assert not bad.any(), (int(bad.sum()), float(err[bad].max()), float(bound_x[bad].min()))
    assert abs(LD(hd) - h1) <= bound_h
    assert info.residual == hd


@pytest.mark.parametrize("name,path", CASES)
def test_ten_iterations(ctx, name, path):
    """K_ITER iterations against numpy_pcg, within 100 times what float64 itself costs the reference"""
    P = grid_problem(ctx, name)
    partial_counts(P, name, path)
    x, info = P.solve(ctx, path, max_iter=K_ITER, history=True)
    assert (info.status, info.iterations) == (H.SOLVE_MAX_ITER, K_ITER)
    xh = x.cpu().numpy()
    assert np.isfinite(xh).all()
    diff = float(np.linalg.norm(xh - P.x64) / np.linalg.norm(P.x64))
    tol = max(100.0 * P.d, 1e-13)
    print("%s %s: d(float64, longdouble) = %.3e, device - float64 = %.3e, allowed %.3e; p.Ap %.3e .. %.3e, r.z %.3e .. %.3e"
          % (name, path, P.d, diff, tol, float(min(P.pq)), float(max(P.pq)), float(min(P.rz)), float(max(P.rz))))
    assert diff <= tol
    assert info.history.shape == (K_ITER + 1,) and info.history[K_ITER].item() == info.residual


@pytest.mark.parametrize("name,path", CASES)
def test_check_every_at_this_size(ctx, name, path):
    """1, 7 or 32 (the default) iterations enqueued between two looks: the same bits"""
    torch = _torch()
    P = grid_problem(ctx, name)
    runs = [P.solve(ctx, path, max_iter=K_ITER, check_every=ce) for ce in (1, 7, 0)]
    x1, i1 = runs[0]
    assert (i1.status, i1.iterations) == (H.SOLVE_MAX_ITER, K_ITER) and bool(torch.isfinite(x1).all())
    for x, i in runs[1:]:
        assert torch.equal(x, x1)
        assert (i.status, i.iterations, i.residual, i.rhs_norm) == (i1.status, i1.iterations, i1.residual, i1.rhs_norm)


@pytest.mark.parametrize("path", ["tile", "csr"])
def test_breakdown_with_many_workgroups(ctx, path):
    """theta = -1 on the large P1 case: every block is bad and the count is summed over ugrid > 64 partials.  Then
    one bad block only, in the last workgroup's share (partial ugrid - 1 > 64): still a breakdown.  A status, not a
    fault: x stays finite"""
    torch = _torch()
    P = grid_problem(ctx, "p1")
    c = P.c
    ugrid, _ = partial_counts(P, "p1", path)
    dm = c.dm if path == "tile" else None
    x, info = H.solve(ctx, c.dp, c.vals, dev(P.b), theta=[-1.0], dmesh=dm, rtol=1e-8)
    assert (info.status, info.iterations) == (H.SOLVE_BREAKDOWN, 0)
    assert bool(torch.isfinite(x).all())
    # the diagonal block of the last element negated: block n_blk - 1 belongs to workgroup ugrid - 1
    n_blk = P.rows // 3
    assert (n_blk - 1) // 256 == ugrid - 1 > 64
    r0 = 3 * (n_blk - 1)
    k = np.arange(c.rp[r0], c.rp[r0 + 3])
    k = k[c.col[k] >= r0]
    assert k.shape == (9,)
    vals = c.vals[0].clone()
    vals[torch.from_numpy(k).cuda()] *= -1.0
    x, info = H.solve(ctx, c.dp, [vals], dev(P.b), dmesh=dm, rtol=1e-8)
    assert (info.status, info.iterations) == (H.SOLVE_BREAKDOWN, 0)
    assert bool(torch.isfinite(x).all())
