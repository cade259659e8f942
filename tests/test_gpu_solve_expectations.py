"""The reference's own expectation tables end to end with the device solve in place of the host's sparse solve: matrix
from the HIP kernel, right-hand side from the oracle's L2 volume functional, H.solve (block-Jacobi PCG on the device,
rtol 1e-10), error norms against the exact ESV2007 solution -- compared to 3 significant figures with
  test/linearelliptic-swipdg-expectations_esv2007_2dsgrid.cxx:31-36        (SGrid, Q1)
  test/linearelliptic-swipdg-expectations_esv2007_2daluconform.cxx:32-37   (ALU conforming, P1, monolithic)
exactly as tests/test_gpu_expectations.py does with spsolve."""
import pytest

import oracle as O
from mesh_tools import nvb_mesh
from test_oracle_pinning import ALU_H1, ALU_L2, SGRID_H1, SGRID_L2, sig3

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu


def _device_solve(ctx, grid, b):
    import torch
    loc = grid.local()
    dm = H.DeviceMesh(loc)
    dp = H.DevicePattern(loc)
    vals = H.assemble(ctx, dm, dp, [H.scalar_fn(H.FN_CONST, 1.0)], H.tensor_fn())
    x, info = H.solve(ctx, dp, vals, torch.from_numpy(b).cuda(), dmesh=dm, rtol=1e-10)
    assert info.status == H.SOLVE_CONVERGED, (info.status, info.iterations, info.residual)
    assert H.last_solve_kernels().startswith("apply_tile_kernel<")
    return x.cpu().numpy()


def test_sgrid_q1_table_from_device_solve(ctx):
    l2s, h1s = [], []
    for lvl in range(4):
        n = 8 * 2 ** lvl
        grid = H.Grid.structured(H.CUBE, n, n, (-1, -1), (1, 1))
        og = O.Grid(*O.cube_grid(n, n, (-1, -1), (1, 1)))
        u = _device_solve(ctx, grid, O.rhs_esv2007(og))
        l2, h1 = O.error_norms_esv2007(og, u)
        l2s.append(sig3(l2)); h1s.append(sig3(h1))
    assert l2s == SGRID_L2 and h1s == SGRID_H1


def test_alu_p1_table_from_device_solve(ctx):
    l2s, h1s = [], []
    for lvl in range(4):
        et, c, ev = nvb_mesh(4, 2 + 2 * lvl)
        grid = H.Grid.from_connectivity(H.SIMPLEX, c, ev)
        og = O.Grid(et, c, ev)
        u = _device_solve(ctx, grid, O.rhs_esv2007(og))
        l2, h1 = O.error_norms_esv2007(og, u)
        l2s.append(sig3(l2)); h1s.append(sig3(h1))
    assert l2s == ALU_L2 and h1s == ALU_H1
