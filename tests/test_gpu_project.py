"""Reduced-basis projection on the device (hdd_operator_project / hdd_vectors_inner: H.project, H.inner) against the
same arrays on the host.

Reference: scipy.sparse on the downloaded arrays, as in test_gpu_apply.py: G_ref[q] = V (A_q U^T) in float64.

Tolerance (derived, not tuned): the bound apply2_reference states,
    |G - G_ref|_ij <= 2 gamma_K (|V|^T |A_q| |U|)_ij,   K = n_rows + max_r len_r + 3,
which holds for any order of summation (every term passes through at most K roundings whatever the tree, and the
zeros the kernels add for absent rows and vectors add exactly), so it holds for the MFMA chains, the four waves and
the parts in order.  An entry whose scale is 0 must be exactly 0.  H.inner: 2 gamma_n |V|^T |W|.
"""
import numpy as np
import pytest

from cases import os2014_components
from test_gpu_apply import Case, apply2_reference, case, gamma, strided

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 8), (17, 5), (16, 16), (33, 64), (64, 64)]


def _torch():
    import torch
    return torch


def project_reference(rp, col, hv, shape, rng, V, Uv):
    """(G_ref, bound) of one component on the (restricted) operator: apply2_reference, on the slice where there is one"""
    if rng is None:
        return apply2_reference(rp, col, [hv], shape, V, Uv)
    r0, r1, c0, c1 = rng
    A = sp.csr_matrix((hv, col, rp), shape=shape)[r0:r1, c0:c1]
    absA = sp.csr_matrix((np.abs(hv), col, rp), shape=shape)[r0:r1, c0:c1]
    length = np.diff(sp.csr_matrix((np.ones(col.shape[0]), col, rp), shape=shape)[r0:r1, c0:c1].indptr)
    K = (r1 - r0) + (length.max() if length.size else 0) + 3
    return V @ (A @ Uv.T), 2.0 * gamma(K) * (np.abs(V) @ (absA @ np.abs(Uv).T))


def check(G, refs, what=""):
    g = G.cpu().numpy()
    assert g.shape[0] == len(refs), what
    for q, (ref, bound) in enumerate(refs):
        assert g[q].shape == ref.shape, (what, q)
        assert np.isfinite(g[q]).all(), (what, q)
        err = np.abs(g[q] - ref)
        bad = err > bound
        assert not bad.any(), (what, q, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))
        assert (g[q][bound == 0] == 0).all(), (what, q)


def both_paths(ctx, c, V, Uv, block=None, rng=None, tile=True, pattern=None, vals=None, hvals=None, host=None):
    """project on the tile path and on the CSR path against the reference; returns the two device results"""
    rp, col = host if host is not None else (c.rp, c.col)
    hvals = hvals or c.hvals
    refs = [project_reference(rp, col, hv, (c.n_rows, c.n_cols), rng, V, Uv) for hv in hvals]
    vd, ud = strided(V, 3), strided(Uv, 5)
    out = []
    for dm, want in ((c.dm, "project_tile_kernel<" if tile else "project_csr_kernel<"), (None, "project_csr_kernel<")):
        G = H.project(ctx, pattern or c.dp, vals or c.vals, vd, ud, dmesh=dm, block=block)
        k = H.last_apply_kernel()
        _torch().cuda.synchronize()
        assert k.startswith(want), (k, want)
        assert G.shape == (len(hvals), V.shape[0], Uv.shape[0])
        check(G, refs, k)
        out.append(G)
    return out


def _bases(c, n_v, n_u, seed, rows=None, cols=None):
    r = np.random.default_rng(seed)
    return r.standard_normal((n_v, rows or c.n_rows)), r.standard_normal((n_u, cols or c.n_cols))


@pytest.mark.parametrize("name", ["p1", "q1"])
@pytest.mark.parametrize("n_v,n_u", SHAPES)
def test_structured_tiles(ctx, name, n_v, n_u):
    """P1 Kuhn 50 x 4 (boundary tiles, an all-interior tile, a 16-element tail) and Q1 130 x 3 on both paths; panel
    edges at 16 / 17 / 33, a rectangular case, rows strided with NaN padding"""
    c = case(ctx, name)
    assert c.local.n_own % 64 != 0 and c.local.n_own > 128
    V, Uv = _bases(c, n_v, n_u, 1000 + 64 * n_v + n_u)
    both_paths(ctx, c, V, Uv)


@pytest.mark.parametrize("name", ["p1_neumann", "p1_shuffled", "q1_scrambled"])
def test_singular_and_unordered_neighbours(ctx, name):
    c = case(ctx, name)
    V, Uv = _bases(c, 5, 18, 7)
    both_paths(ctx, c, V, Uv)


_OS2014_4 = []


def os2014_four(ctx):
    """the OS2014 mesh and its two components with two further sinusoids: four value arrays on one pattern"""
    if not _OS2014_4:
        (c0, b0, kx, ky), second = os2014_components()
        comps = [(c0, b0, kx, ky), second, (0.5, 0.3, 2 * kx, ky), (0.2, 0.1, kx, 2 * ky)]
        fns = [H.scalar_fn(H.FN_SINUSOID, a, b, k, l, order=3) for (a, b, k, l) in comps]
        _OS2014_4.append(Case(ctx, H.Grid.structured(H.SIMPLEX, 16, 16, (-1, -1), (1, 1)), kappas=fns, tensor=H.tensor_fn()))
    return _OS2014_4[0]


def test_every_component_against_its_own_reference(ctx):
    c = os2014_four(ctx)
    assert len(c.vals) == 4
    V, Uv = _bases(c, 17, 20, 9)
    Gt, Gc = both_paths(ctx, c, V, Uv)
    assert Gt.shape[0] == len(c.vals)
    # the components differ: no component's result stands in for another's
    g = Gt.cpu().numpy()
    assert all(not np.array_equal(g[0], g[q]) for q in range(1, g.shape[0]))


def test_hexahedra_take_the_wave_per_row_kernel(ctx):
    c = case(ctx, "hex_q2")
    V, Uv = _bases(c, 17, 33, 5)
    both_paths(ctx, c, V, Uv, tile=False)
    assert H.last_apply_kernel() == "project_csr_kernel<64>"


def test_l2_gramian_on_a_volume_pattern(ctx):
    """U = None means U = V: the Gramian V^T M V of the L2 product, symmetric within the bound, positive diagonal"""
    c = case(ctx, "p1")
    dpv = H.DevicePattern(c.local, volume=True)
    m = H.product(ctx, c.dm, H.PRODUCT_L2, dpv)
    _torch().cuda.synchronize()
    rp, col, _ = dpv.host
    V, _ = _bases(c, 20, 1, 6)
    ref, bound = apply2_reference(rp, col, [m.cpu().numpy()], (c.n_rows, c.n_cols), V, V)
    G = H.project(ctx, dpv, [m], strided(V, 2), dmesh=c.dm)
    assert H.last_apply_kernel() == "project_csr_kernel<8>"
    check(G, [(ref, bound)], "l2")
    g = G.cpu().numpy()[0]
    assert (np.diag(g) > 0).all() and (np.abs(g - g.T) <= bound + bound.T).all()
    # a 1-d input counts as one vector
    g1 = H.project(ctx, dpv, [m], _torch().from_numpy(V[3]).cuda())
    assert g1.shape == (1, 1, 1) and abs(g1.item() - ref[3, 3]) <= bound[3, 3]


@pytest.mark.parametrize("name", ["p1_block", "q1_block"])
@pytest.mark.parametrize("ss,nn", [(0, 0), (0, 1)])
def test_block_ranges(ctx, name, ss, nn):
    """the BlockSWIPDG operator (ss, nn) projected in place, v in ss's numbering, u in nn's; NaN in every value
    outside the column range and in the padding of V / U does not reach the result"""
    torch = _torch()
    c = case(ctx, name)
    nb = c.grid.nb
    a, b = c.grid.subdomain_range(ss, ss + 1)
    p, q = c.grid.subdomain_range(nn, nn + 1)
    rng = (a * nb, b * nb, p * nb, q * nb)
    V, Uv = _bases(c, 17, 9, 13 + 4 * ss + nn, rows=rng[1] - rng[0], cols=rng[3] - rng[2])
    Gt, Gc = both_paths(ctx, c, V, Uv, block=(ss, nn), rng=rng)
    if ss != nn:
        assert bool((Gt != 0).any())     # the coupling is there
    outside = torch.from_numpy((c.col < rng[2]) | (c.col >= rng[3])).cuda()
    assert bool(outside.any())
    poisoned = [torch.where(outside, torch.full_like(v, float("nan")), v) for v in c.vals]
    vd, ud = strided(V, 3), strided(Uv, 5)     # NaN behind every row
    for dm, clean in ((c.dm, Gt), (None, Gc)):
        G = H.project(ctx, c.dp, poisoned, vd, ud, dmesh=dm, block=(ss, nn))
        assert bool(torch.isfinite(G).all()) and torch.equal(G, clean)


def test_unaligned_range_takes_the_csr_kernel(ctx):
    c = case(ctx, "p1_block")
    rng = (1, c.n_rows - 2, 2, c.n_cols - 5)
    V, Uv = _bases(c, 3, 17, 3, rows=rng[1] - rng[0], cols=rng[3] - rng[2])
    both_paths(ctx, c, V, Uv, block=rng, rng=rng, tile=False)
    with pytest.raises(H.HddError, match="range outside the matrix"):     # vectors that fit the range asked for
        H.project(ctx, c.dp, c.vals, strided(np.zeros((3, c.n_rows + 1)), 0), strided(Uv, 0), dmesh=c.dm,
                  block=(0, c.n_rows + 1, 2, c.n_cols - 5))


@pytest.mark.parametrize("name,tile", [("p1", True), ("q1", True), ("p1", False), ("q1", False), ("hex_q2", False)])
def test_bit_identity(ctx, name, tile):
    """two calls give equal bits; entry (q, i, j) of a 33 x 64 call has the bits of the 1 x 1 call on (v_i, u_j), of a
    call with the vectors permuted, and of the calls that extend a basis by one vector"""
    torch = _torch()
    c = case(ctx, name)
    dm = c.dm if tile else None
    V, Uv = _bases(c, 33, 64, 77)
    vd, ud = strided(V, 3), strided(Uv, 5)
    G = H.project(ctx, c.dp, c.vals, vd, ud, dmesh=dm)
    assert H.last_apply_kernel().startswith("project_tile_kernel<" if tile else "project_csr_kernel<")
    assert torch.equal(G, H.project(ctx, c.dp, c.vals, vd, ud, dmesh=dm))
    for i, j in [(0, 0), (15, 15), (16, 16), (32, 63), (1, 47), (17, 16), (31, 0), (0, 63)]:
        one = H.project(ctx, c.dp, c.vals, vd[i], ud[j], dmesh=dm)
        assert torch.equal(one[:, 0, 0], G[:, i, j]), (i, j)
    r = np.random.default_rng(5)
    pv, pu = r.permutation(33), r.permutation(64)
    Gp = H.project(ctx, c.dp, c.vals, strided(V[pv], 1), strided(Uv[pu], 2), dmesh=dm)
    assert torch.equal(Gp, G[:, torch.from_numpy(pv).cuda()][:, :, torch.from_numpy(pu).cuda()])
    # a basis extended by one vector: the new row and column alone
    small = H.project(ctx, c.dp, c.vals, vd[:32], ud[:32], dmesh=dm)
    row = H.project(ctx, c.dp, c.vals, vd[32], ud[:33], dmesh=dm)
    colm = H.project(ctx, c.dp, c.vals, vd[:33], ud[32], dmesh=dm)
    assert torch.equal(small, G[:, :32, :32]) and torch.equal(row[:, 0], G[:, 32, :33]) and torch.equal(colm[:, :, 0], G[:, :33, 32])


@pytest.mark.parametrize("n", [1, 63, 4097])
@pytest.mark.parametrize("n_v,n_w", [(1, 1), (5, 64), (64, 3)])
def test_inner(ctx, n_v, n_w, n):
    torch = _torch()
    r = np.random.default_rng(n + 64 * n_v + n_w)
    V, W = r.standard_normal((n_v, n)), r.standard_normal((n_w, n))
    vd, wd = strided(V, 3), strided(W, 1)
    G = H.inner(ctx, vd, wd)
    assert G.shape == (n_v, n_w)
    bound = 2.0 * gamma(n) * (np.abs(V) @ np.abs(W).T)
    err = np.abs(G.cpu().numpy() - V @ W.T)
    assert (err <= bound).all(), (float(err.max()), float(bound.min()))
    assert torch.equal(G, H.inner(ctx, vd, wd))
    if n_v == 1 and n_w == 1:     # 1-d inputs
        assert torch.equal(H.inner(ctx, vd[0], wd[0]), G)


@pytest.mark.parametrize("name", ["p1", "q1", "os2014"])
def test_agrees_with_the_apply2_route(ctx, name):
    """H.project against one H.apply2 call per component on 8 x 8: both lie within one bound of the exact value"""
    c = case(ctx, name)
    V, Uv = _bases(c, 8, 8, 21)
    vd, ud = strided(V, 3), strided(Uv, 5)
    for dm in (c.dm, None):
        G = H.project(ctx, c.dp, c.vals, vd, ud, dmesh=dm).cpu().numpy()
        for q, v in enumerate(c.vals):
            old = H.apply2(ctx, c.dp, [v], vd, ud, dmesh=dm).cpu().numpy()
            _, bound = apply2_reference(c.rp, c.col, [c.hvals[q]], (c.n_rows, c.n_cols), V, Uv)
            assert (np.abs(G[q] - old) <= 2.0 * bound).all(), (name, q)


def test_argument_errors(ctx):
    c = case(ctx, "p1")
    V, Uv = _bases(c, 2, 2, 1)
    with pytest.raises(H.HddError):
        H.project(ctx, c.dp, c.vals, strided(V, 0)[:, :-1], strided(Uv, 0))
    with pytest.raises(H.HddError):
        H.project(ctx, c.dp, c.vals, _torch().zeros((H.MAX_BASIS + 1, c.n_rows), dtype=_torch().float64, device="cuda"))
