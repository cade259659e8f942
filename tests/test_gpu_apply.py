"""Operator application on the device (hdd_operator_apply / hdd_operator_apply2: H.apply, H.apply2) against the
same arrays on the host.

Reference: scipy.sparse.csr_matrix((vals, col, row_ptr)) of the downloaded arrays, restricted by slicing, times x in
float64; for several components the matrix of sum_q theta_q vals_q.

Tolerance (derived, not tuned).  Row r of the (restricted) operator has len_r entries per component, so the device
result is a sum of K_r = n_comp len_r + n_comp + 2 rounded terms (the theta combination and the products), and so is
the reference's:
    |y_gpu - y_ref|_r <= 2 gamma_{K_r} (sum_q |theta_q| |A_q| |x|)_r,   gamma_n = n 2^-53 / (1 - n 2^-53),
the factor 2 because both sides round.  A row whose scale is 0 must be exactly 0.  apply2 adds the n_rows terms of
the dot product: K = n_rows + max_r K_r on |v|^T |A| |u|.
"""
import numpy as np
import pytest

import oracle as O
from cases import SPE10_LOWER, SPE10_UPPER, os2014_components
from mesh_tools import nvb_mesh, scrambled_quad_mesh

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def _torch():
    import torch
    return torch


class Case:
    """an assembled operator: device mesh / pattern / values and their host copies"""

    def __init__(self, ctx, grid, kappas=None, tensor=None, prm=None, dim=2):
        torch = _torch()
        self.grid = grid
        self.local = loc = grid.local()
        self.dm = H.DeviceMesh(loc)
        self.dp = H.DevicePattern(loc)
        if tensor is None:      # the SPE10 checkerboard tensor, laid over the mesh's bounding box
            lo, hi = loc.coords.reshape(loc.nvpe, 2, -1)[:, 0].min(), loc.coords.reshape(loc.nvpe, 2, -1)[:, 0].max()
            lo2, hi2 = loc.coords.reshape(loc.nvpe, 2, -1)[:, 1].min(), loc.coords.reshape(loc.nvpe, 2, -1)[:, 1].max()
            k = loc.checkerboard((lo, lo2), (hi, hi2), 100, 20, O.spe10_synthetic_permeability())
            tensor = H.tensor_fn(H.TENSOR_ISO_PER_ELEM, per_elem=torch.from_numpy(k).cuda())
        kappas = kappas or [H.scalar_fn(H.FN_CONST, 1.0)]
        self.vals = H.assemble(ctx, self.dm, self.dp, kappas, tensor, prm)
        torch.cuda.synchronize()
        self.rp, self.col, self.ep = self.dp.host
        self.hvals = [v.cpu().numpy() for v in self.vals]
        self.n_rows, self.n_cols = self.dp.t.n_rows, self.dp.t.n_cols


_CASES = {}


def case(ctx, name):
    """the assembled cases, built once per session"""
    if name in _CASES:
        return _CASES[name]
    if name == "p1":
        nx = 50
        while True:     # some tile must be all-interior (64 row blocks of 4 x 9 values)
            c = Case(ctx, H.Grid.structured(H.SIMPLEX, nx, 4, SPE10_LOWER, SPE10_UPPER))
            if (np.diff(c.ep[::64]) == 64 * 36).any():
                break
            nx += 10
    elif name == "q1":
        c = Case(ctx, H.Grid.structured(H.CUBE, 130, 3, SPE10_LOWER, SPE10_UPPER))
    elif name in ("p1_neumann", "q1_neumann"):
        et = H.SIMPLEX if name[0] == "p" else H.CUBE
        c = Case(ctx, H.Grid.structured(et, 13, 7, SPE10_LOWER, SPE10_UPPER, boundary=H.BOUNDARY_ALL_NEUMANN))
    elif name == "p1_shuffled":
        _, coords, tris = nvb_mesh(4, 4)
        perm = np.random.default_rng(11).permutation(tris.shape[0])
        c = Case(ctx, H.Grid.from_connectivity(H.SIMPLEX, coords, tris[perm]))
    elif name == "q1_scrambled":
        _, coords, ev = scrambled_quad_mesh(9, 8, 5)
        c = Case(ctx, H.Grid.from_connectivity(H.CUBE, coords, ev))
    elif name == "os2014":
        fns = [H.scalar_fn(H.FN_SINUSOID, a, b, kx, ky, order=3) for (a, b, kx, ky) in os2014_components()]
        c = Case(ctx, H.Grid.structured(H.SIMPLEX, 16, 16, (-1, -1), (1, 1)), kappas=fns, tensor=H.tensor_fn())
    elif name == "p1_block":
        c = Case(ctx, H.Grid.structured(H.SIMPLEX, 16, 16, SPE10_LOWER, SPE10_UPPER, px=2, py=2))
    elif name == "q1_block":
        c = Case(ctx, H.Grid.structured(H.CUBE, 16, 12, SPE10_LOWER, SPE10_UPPER, px=2, py=2))
    elif name == "hex_q2":
        c = Case(ctx, H.Grid.structured3d((3, 3, 3), degree=2), tensor=H.tensor_fn(dim=3), prm=H.params_for(2, 3))
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


def reference(rp, col, hvals, theta, shape, rng, X):
    """(y_ref, bound) [n_vec, rows] of the restricted operator on the host arrays"""
    theta = np.ones(len(hvals)) if theta is None else np.asarray(theta, np.float64)
    r0, r1, c0, c1 = rng if rng is not None else (0, shape[0], 0, shape[1])
    A = sp.csr_matrix((sum(t * v for t, v in zip(theta, hvals)), col, rp), shape=shape)[r0:r1, c0:c1]
    absA = sp.csr_matrix((sum(abs(t) * np.abs(v) for t, v in zip(theta, hvals)), col, rp), shape=shape)[r0:r1, c0:c1]
    length = np.diff(sp.csr_matrix((np.ones(col.shape[0]), col, rp), shape=shape)[r0:r1, c0:c1].indptr)
    K = len(hvals) * length + len(hvals) + 2
    y = (A @ X.T).T
    scale = (absA @ np.abs(X).T).T
    return y, 2.0 * gamma(K)[None, :] * scale, K


def check(y_gpu, y_ref, bound, what=""):
    y = y_gpu.cpu().numpy().reshape(y_ref.shape)
    assert np.isfinite(y).all(), what
    err = np.abs(y - y_ref)
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))
    assert (y[bound == 0] == 0).all(), what


def strided(a, pad):
    """a [k, n] host array as a device tensor with row stride n + pad"""
    torch = _torch()
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float64, device="cuda")
    t[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return t[:, :a.shape[1]]


def both_paths(ctx, c, X, theta=None, block=None, rng=None, hvals=None, tile=True):
    """apply on the tile path and on the generic path against the reference; returns the two device results"""
    xd = strided(X, 5)
    y_ref, bound, _ = reference(c.rp, c.col, hvals or c.hvals, theta, (c.n_rows, c.n_cols), rng, X)
    yt = H.apply(ctx, c.dp, c.vals, xd, theta=theta, dmesh=c.dm, block=block)
    kt = H.last_apply_kernel()
    yg = H.apply(ctx, c.dp, c.vals, xd, theta=theta, dmesh=None, block=block)
    kg = H.last_apply_kernel()
    _torch().cuda.synchronize()
    assert kt.startswith("apply_tile_kernel<" if tile else "apply_csr_kernel<"), kt
    assert kg.startswith("apply_csr_kernel<"), kg
    check(yt, y_ref, bound, "tile" if tile else "mesh given, generic")
    check(yg, y_ref, bound, "generic")
    return yt, yg


@pytest.mark.parametrize("name,rb", [("p1", 36), ("q1", 80)])
@pytest.mark.parametrize("n_vec", [1, 3, 8])
def test_structured_tiles(ctx, name, rb, n_vec):
    """P1 Kuhn 50 x 4 (boundary tiles, an all-interior tile 128..191, a 16-element tail) and Q1 130 x 3 (all-interior
    tile 192..255, a 6-element tail), n_vec 1 / 3 / 8 (one pass, a masked pass, two passes), ldx != n"""
    c = case(ctx, name)
    tiles = np.diff(c.ep[::64])
    assert (tiles == 64 * rb).any() and (tiles != 64 * rb).any() and c.local.n_own % 64 != 0
    if name == "p1":
        assert c.local.n_own % 64 == 16 and c.ep[192] - c.ep[128] == 64 * 36
    else:
        assert c.local.n_own % 64 == 6 and c.ep[256] - c.ep[192] == 64 * 80
    X = np.random.default_rng(100 + n_vec).standard_normal((n_vec, c.n_cols))
    both_paths(ctx, c, X)


def test_out_argument_and_1d(ctx):
    torch = _torch()
    c = case(ctx, "p1")
    x = np.random.default_rng(1).standard_normal(c.n_cols)
    y_ref, bound, _ = reference(c.rp, c.col, c.hvals, None, (c.n_rows, c.n_cols), None, x[None, :])
    y = H.apply(ctx, c.dp, c.vals, torch.from_numpy(x).cuda(), dmesh=c.dm)
    assert y.shape == (c.n_rows,)
    check(y, y_ref, bound)
    X = np.random.default_rng(2).standard_normal((2, c.n_cols))
    out = torch.full((2, c.n_rows + 3), 7.0, dtype=torch.float64, device="cuda")
    ret = H.apply(ctx, c.dp, c.vals, strided(X, 1), dmesh=c.dm, out=out[:, :c.n_rows])
    y_ref, bound, _ = reference(c.rp, c.col, c.hvals, None, (c.n_rows, c.n_cols), None, X)
    check(ret, y_ref, bound)
    assert (out[:, c.n_rows:] == 7.0).all()     # nothing written beyond the rows


@pytest.mark.parametrize("name", ["p1_neumann", "q1_neumann", "p1_shuffled", "q1_scrambled"])
def test_boundary_codes_and_arbitrary_block_order(ctx, name):
    """Neumann faces (neighbors = -2) and meshes whose element order is arbitrary (shuffled newest-vertex-bisection
    triangles, scrambled quadrilaterals): the blocks inside a row are then in no geometric order"""
    c = case(ctx, name)
    if "neumann" in name:
        assert (c.local.neighbors == H.NBR_NEUMANN).any() and not (c.local.neighbors == H.NBR_DIRICHLET).any()
    else:
        # the neighbour ids are not ascending in face order (the kernel has to sort them as the pattern did), and more
        # than one tile
        nb = np.where(c.local.neighbors >= 0, c.local.neighbors, np.iinfo(np.int32).max).astype(np.int64)
        assert ((np.diff(nb, axis=0) < 0).any(axis=0).sum() > 8) and c.local.n_own > 64
        if name == "p1_shuffled":   # neighbours anywhere in the mesh, not a tile away
            e = np.arange(nb.shape[1])
            assert (np.abs(c.local.neighbors - e)[c.local.neighbors >= 0] > 64).any()
    X = np.random.default_rng(7).standard_normal((3, c.n_cols))
    both_paths(ctx, c, X)


def test_theta_fusion(ctx):
    """OS2014 affine part + mu-component, theta = (1, 0.3): the fused apply == the reference on va + 0.3 vc == the
    lincomb written out and applied as one component, all under the two-component tolerance"""
    c = case(ctx, "os2014")
    theta = [1.0, 0.3]
    X = np.random.default_rng(9).standard_normal((3, c.n_cols))
    both_paths(ctx, c, X, theta=theta)
    y_ref, bound, _ = reference(c.rp, c.col, c.hvals, theta, (c.n_rows, c.n_cols), None, X)
    A = H.affine_lincomb(ctx, c.vals, np.array([theta]))[0]
    assert A.data_ptr() % 16 == 0
    y = H.apply(ctx, c.dp, [A], strided(X, 5), dmesh=c.dm)
    assert H.last_apply_kernel().startswith("apply_tile_kernel<")
    check(y, y_ref, bound, "lincomb then apply")
    # theta = None is all ones
    y1 = H.apply(ctx, c.dp, c.vals, strided(X, 5), dmesh=c.dm)
    y_ref1, bound1, _ = reference(c.rp, c.col, c.hvals, [1.0, 1.0], (c.n_rows, c.n_cols), None, X)
    check(y1, y_ref1, bound1, "theta None")


@pytest.mark.parametrize("name", ["p1_block", "q1_block"])
@pytest.mark.parametrize("ss,nn", [(0, 0), (0, 1), (1, 0), (3, 3)])
def test_block_ranges(ctx, name, ss, nn):
    """the BlockSWIPDG operator (ss, nn) applied in place on the global arrays: == the sliced reference, == the
    extracted operator through the generic path; values outside the column range are never touched"""
    torch = _torch()
    c = case(ctx, name)
    nb = c.grid.nb
    a, b = c.grid.subdomain_range(ss, ss + 1)
    p, q = c.grid.subdomain_range(nn, nn + 1)
    rng = (a * nb, b * nb, p * nb, q * nb)
    X = np.random.default_rng(13 + 4 * ss + nn).standard_normal((3, rng[3] - rng[2]))
    yt, yg = both_paths(ctx, c, X, block=(ss, nn), rng=rng)
    assert yt.shape == (3, rng[1] - rng[0])
    # the extracted operator (H.block_operator) through the generic kernel
    y_ref, bound, _ = reference(c.rp, c.col, c.hvals, None, (c.n_rows, c.n_cols), rng, X)
    orp, ocol, ovals = H.block_operator(ctx, c.grid, c.dp, c.vals, ss, nn)
    if ocol.numel():
        ye = H.apply(ctx, H.CsrPattern(orp, ocol, rng[3] - rng[2]), ovals, strided(X, 5))
        assert H.last_apply_kernel().startswith("apply_csr_kernel<")
        check(ye, y_ref, bound, "extracted")
    else:
        assert not np.any(y_ref)
    # NaN in every value whose column lies outside the range: same result, bit for bit, on both paths
    outside = torch.from_numpy((c.col < rng[2]) | (c.col >= rng[3])).cuda()
    assert bool(outside.any())
    poisoned = [torch.where(outside, torch.full_like(v, float("nan")), v) for v in c.vals]
    xd = strided(X, 5)
    for dm, clean in ((c.dm, yt), (None, yg)):
        y = H.apply(ctx, c.dp, poisoned, xd, dmesh=dm, block=(ss, nn))
        assert bool(torch.isfinite(y).all()) and torch.equal(y, clean)


@pytest.mark.parametrize("name", ["p1_block", "q1_block"])
def test_unaligned_range_takes_the_generic_path(ctx, name):
    """a range that is not aligned to nb cannot be tiled by elements: with dmesh given the call takes the CSR kernel
    (documented in hdd.h), and is right"""
    c = case(ctx, name)
    rng = (1, c.n_rows - 2, 2, c.n_cols - 5)
    X = np.random.default_rng(3).standard_normal((2, rng[3] - rng[2]))
    both_paths(ctx, c, X, block=rng, rng=rng, tile=False)
    with pytest.raises(H.HddError, match="range"):
        H.apply(ctx, c.dp, c.vals, strided(X, 0), dmesh=c.dm, block=(0, c.n_rows + 1, 2, c.n_cols - 5))


def test_hexahedra_take_the_generic_path(ctx):
    """Q2 on 3 x 3 x 3 hexahedra: rows up to 7 x 27 = 189 long, a wave per row"""
    c = case(ctx, "hex_q2")
    assert np.diff(c.rp).max() == 189
    X = np.random.default_rng(5).standard_normal((3, c.n_cols))
    both_paths(ctx, c, X, tile=False)
    assert H.last_apply_kernel().startswith("apply_csr_kernel<64")


def _l2(ctx, c):
    dpv = H.DevicePattern(c.local, volume=True)
    m = H.product(ctx, c.dm, H.PRODUCT_L2, dpv)
    _torch().cuda.synchronize()
    return dpv, m


def test_volume_product_pattern_takes_the_generic_path(ctx):
    c = case(ctx, "p1")
    dpv, m = _l2(ctx, c)
    X = np.random.default_rng(6).standard_normal((2, c.n_cols))
    y = H.apply(ctx, dpv, [m], strided(X, 5), dmesh=c.dm)
    assert H.last_apply_kernel().startswith("apply_csr_kernel<8")
    rp, col, _ = dpv.host
    y_ref, bound, _ = reference(rp, col, [m.cpu().numpy()], None, (c.n_rows, c.n_cols), None, X)
    check(y, y_ref, bound)


def apply2_reference(rp, col, hvals, shape, V, Uv):
    y, _, K = reference(rp, col, hvals, None, shape, None, Uv)
    absA = sp.csr_matrix((np.abs(hvals[0]), col, rp), shape=shape)
    ref = V @ y.T
    bound = 2.0 * gamma(shape[0] + K.max()) * (np.abs(V) @ (absA @ np.abs(Uv).T))
    return ref, bound


@pytest.mark.parametrize("name", ["p1", "q1"])
def test_apply2(ctx, name):
    torch = _torch()
    c = case(ctx, name)
    r = np.random.default_rng(21)
    V, Uv = r.standard_normal((2, c.n_rows)), r.standard_normal((3, c.n_cols))
    ref, bound = apply2_reference(c.rp, c.col, c.hvals, (c.n_rows, c.n_cols), V, Uv)
    for dm in (c.dm, None):
        got = H.apply2(ctx, c.dp, c.vals, strided(V, 3), strided(Uv, 5), dmesh=dm)
        assert got.shape == (2, 3)
        assert H.last_apply_kernel().startswith("apply_tile_kernel<" if dm is not None else "apply_csr_kernel<")
        assert (np.abs(got.cpu().numpy() - ref) <= bound).all(), (got.cpu().numpy() - ref, bound)
        again = H.apply2(ctx, c.dp, c.vals, strided(V, 3), strided(Uv, 5), dmesh=dm)
        assert torch.equal(got, again)
    # the L2 product: positive, symmetric
    dpv, m = _l2(ctx, c)
    rp, col, _ = dpv.host
    hm = [m.cpu().numpy()]
    uv = H.apply2(ctx, dpv, [m], strided(Uv, 1), strided(V, 2))
    vu = H.apply2(ctx, dpv, [m], strided(V, 2), strided(Uv, 1))
    uu = H.apply2(ctx, dpv, [m], strided(Uv, 1), strided(Uv, 1))
    torch.cuda.synchronize()
    assert (torch.diagonal(uu) > 0).all()
    ref_uv, b_uv = apply2_reference(rp, col, hm, (c.n_rows, c.n_cols), Uv, V)
    ref_vu, b_vu = apply2_reference(rp, col, hm, (c.n_rows, c.n_cols), V, Uv)
    assert (np.abs(uv.cpu().numpy() - ref_uv) <= b_uv).all() and (np.abs(vu.cpu().numpy() - ref_vu) <= b_vu).all()
    assert (np.abs(uv.cpu().numpy() - vu.cpu().numpy().T) <= b_uv + b_vu.T).all()


@pytest.mark.parametrize("name", ["p1", "q1", "os2014"])
def test_determinism(ctx, name):
    torch = _torch()
    c = case(ctx, name)
    X = strided(np.random.default_rng(8).standard_normal((5, c.n_cols)), 2)
    theta = [1.0, -0.7] if len(c.vals) == 2 else None
    for dm in (c.dm, None):
        a = H.apply(ctx, c.dp, c.vals, X, theta=theta, dmesh=dm)
        b = H.apply(ctx, c.dp, c.vals, X, theta=theta, dmesh=dm)
        assert torch.equal(a, b)
