"""hdd_operator_solve_batched where the per-column reductions pass one wave stride and the launches walk their grids
more than once, on the large cases of test_gpu_apply_grid.py (sized from the device's CU count):

  p1 tile   the Kuhn P1 mesh: several tiles per wave of the DOT apply, part_pq [column][> 64], update_grid > 64
  q1 tile   the Q1 mesh (both penalties times 4, SIGMA_SCALE: its diagonal blocks are positive definite then,
            test_gpu_solve_grid.py)
  p1 tile with block_size 1: rows > 2048 * 256 blocks, so cg_update_batched (and cg_init) make a second grid-stride
            pass, and the inverse "blocks" come from the CSR arrays

n_rhs 4 (one full group) and 5 (a full group and a group of one column), rtol = 0, max_iter = 40 (on the Q1 matrix
the columns end before that, on p . Ap <= 0 -- exactly where their single solves end).  The oracle is the
single solve of each column (whose arithmetic test_gpu_solve_grid.py pins against longdouble references): x through
an int64 view, the info and the history for equality.  No host reference is computed here."""
import numpy as np
import pytest

from test_gpu_apply_grid import grid_case, grid_facts
from test_gpu_solve_batched import assert_columns_equal_singles, kernels, run_both
from test_gpu_solve_grid import dot_grid, update_grid

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

MAX_ITER = 40


def _torch():
    import torch
    return torch


def right_hand_sides(c, n_rhs, seed):
    """random columns of very different sizes, and a smooth one"""
    torch = _torch()
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    B = torch.randn((n_rhs, c.n_rows), dtype=torch.float64, device="cuda", generator=g)
    i = (torch.arange(c.n_rows, dtype=torch.float64, device="cuda") + 0.5) / c.n_rows
    B[1] = torch.cos(np.pi * i) * torch.cos(3.0 * np.pi * i)
    B[2] *= 1e6
    return B.cpu().numpy()


@pytest.mark.parametrize("name,bs,n_rhs", [("p1", 0, 4), ("p1", 0, 5), ("q1", 0, 4), ("q1", 0, 5), ("p1", 1, 5)])
def test_columns_are_the_single_solves_at_this_size(ctx, name, bs, n_rhs):
    torch = _torch()
    c = grid_case(ctx, name)
    rows, n_tiles, G = grid_facts(c, name)
    nb = 3 if name == "p1" else 4
    n_blk = rows // (bs or nb)
    ugrid, n_pq = update_grid(n_blk), dot_grid(name, "tile", rows, n_tiles)
    print("%s: rows %d, tiles %d, part_pq %d per column, update grid %d, blocks %d" % (name, rows, n_tiles, n_pq, ugrid, n_blk))
    assert n_tiles > n_pq > 64 and ugrid > 64            # input conditions: several tiles per wave, > 64 partials
    if bs == 1:
        assert n_blk > 2048 * 256                        # ... and a second pass of the update kernel
    B = right_hand_sides(c, n_rhs, 70 + n_rhs)
    X, infos, singles, names = run_both(ctx, c, B, c.dm, block_size=bs, rtol=0.0, max_iter=MAX_ITER)
    assert names == kernels("apply_tile_kernel<%d, %d, 4, dot>" % (nb, nb), bs or nb)
    assert_columns_equal_singles(X, infos, singles, name)
    assert bool(torch.isfinite(X).all())
    if name == "p1":
        assert [(i.status, i.iterations) for i in infos] == [(H.SOLVE_MAX_ITER, MAX_ITER)] * n_rhs
    else:
        # the Q1 matrix is not positive definite for every right-hand side: p . Ap <= 0 ends a column
        # early, with the single solve's status and count (compared above); enough iterations ran before that
        assert all(i.iterations >= 10 and i.status in (H.SOLVE_MAX_ITER, H.SOLVE_BREAKDOWN) for i in infos)
    assert all(i.history.shape == (i.iterations + 1,) for i in infos)
