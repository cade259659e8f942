"""hdd_operator_solve_multi where the tile kernel walks several tiles per wave with two LDS images and the per-column
reductions pass one wave stride: the large P1 case of test_gpu_apply_grid.py (sized from the device's CU count).

Component 0 is that case's SPE10 matrix, component 1 the kappa = 1, A = I matrix assembled on the same mesh with the
same penalties; theta_j = (1, nu_j), nu = 0, 0.5, 1, 2.  Four columns, rtol = 0, max_iter = 6 (the host side of the input conditions is what takes the time); the oracle is the
single solve of each column at theta_j (whose arithmetic test_gpu_solve_grid.py pins against longdouble references):
x through an int64 view, the info and the history for equality.

Input conditions, asserted on the host per theta_j as test_gpu_solve_grid.py does for its matrix: every diagonal block
of A(theta_j) has a Cholesky factor, and p . Ap and r . z of a float64 PCG on the downloaded arrays are positive in
every iteration that the device runs."""
import numpy as np
import pytest

from test_gpu_apply_grid import SIGMA_SCALE, grid_case, grid_facts
from test_gpu_solve import dev, diag_blocks
from test_gpu_solve_batched import assert_columns_equal_singles
from test_gpu_solve_batched_grid import right_hand_sides
from test_gpu_solve_grid import dot_grid, update_grid

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

MAX_ITER = 6
NUS = (0.0, 0.5, 1.0, 2.0)


def _torch():
    import torch
    return torch


def host_pcg_scalars(A0, A1, nu, Dinv, b, iters):
    """p . Ap and r . z of `iters` iterations of block-Jacobi PCG on A0 + nu A1"""
    prec = lambda r: np.einsum("bij,bj->bi", Dinv, r.reshape(-1, 3)).reshape(-1)
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rho = r @ z
    pqs, rzs = [], [rho]
    for _ in range(iters):
        q = A0 @ p + nu * (A1 @ p)
        pq = p @ q
        pqs.append(pq)
        alpha = rho / pq
        x += alpha * p
        r -= alpha * q
        z = prec(r)
        rho_new = r @ z
        rzs.append(rho_new)
        p = z + (rho_new / rho) * p
        rho = rho_new
    return pqs, rzs


def test_four_parameters_at_this_size(ctx):
    torch = _torch()
    c = grid_case(ctx, "p1")
    rows, n_tiles, G = grid_facts(c, "p1")
    ugrid, n_pq = update_grid(rows // 3), dot_grid("p1", "tile", rows, n_tiles)
    print("rows %d, tiles %d, part_pq %d per column, update grid %d" % (rows, n_tiles, n_pq, ugrid))
    assert n_tiles > n_pq > 64 and ugrid > 64            # input conditions: several tiles per wave, > 64 partials
    s = SIGMA_SCALE["p1"]
    (v1,) = H.assemble(ctx, c.dm, c.dp, [H.scalar_fn(H.FN_CONST, 1.0)], H.tensor_fn(),
                       H.params(H.SIGMA_INNER_P1 * s, H.SIGMA_BOUNDARY_P1 * s))
    vals = [c.vals[0], v1]
    thetas = np.array([(1.0, nu) for nu in NUS])
    B = right_hand_sides(c, 4, 74)
    # the input conditions on the host
    A0 = sp.csr_matrix((c.hvals[0], c.col, c.rp), shape=(c.n_rows, c.n_cols))
    A1 = sp.csr_matrix((v1.cpu().numpy(), c.col, c.rp), shape=(c.n_rows, c.n_cols))
    # where the diagonal blocks' entries lie in the value arrays (one pass over the pattern for both components)
    where = diag_blocks(sp.csr_matrix((np.arange(1.0, c.col.shape[0] + 1.0), c.col, c.rp), shape=A0.shape), 3).astype(np.int64) - 1
    assert (where >= 0).all()
    D0, D1 = c.hvals[0][where], A1.data[where]
    for j, nu in enumerate(NUS):
        D = D0 + nu * D1
        np.linalg.cholesky(D)                            # raises LinAlgError if a block is not positive definite
        pqs, rzs = host_pcg_scalars(A0, A1, nu, np.linalg.inv(D), B[j], MAX_ITER)
        assert all(v > 0 for v in pqs) and all(v > 0 for v in rzs), (nu, pqs, rzs)
    Bd = dev(B)
    X, infos = H.solve_multi(ctx, c.dp, vals, Bd, thetas, dmesh=c.dm, rtol=0.0, max_iter=MAX_ITER, history=True)
    assert H.last_solve_kernels() == "apply_tile_multi_kernel<3, 3, 4, dot> + cg_update<3, 4, own> + cg_direction<4>"
    singles = [H.solve(ctx, c.dp, vals, Bd[j], theta=thetas[j], dmesh=c.dm, rtol=0.0, max_iter=MAX_ITER, history=True)
               for j in range(4)]
    assert H.last_solve_kernels().startswith("apply_tile_kernel<3, 3, 1, dot>")
    assert_columns_equal_singles(X, infos, singles, "p1 grid")
    assert bool(torch.isfinite(X).all())
    assert [(i.status, i.iterations) for i in infos] == [(H.SOLVE_MAX_ITER, MAX_ITER)] * 4
    assert all(i.history.shape == (MAX_ITER + 1,) for i in infos)
