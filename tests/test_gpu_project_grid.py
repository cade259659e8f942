"""hdd_operator_project / hdd_vectors_inner past one pass, off the origin and at eight components: what
test_gpu_project.py's small meshes never reach.

  * project_tile_kernel at its 512 parts with two and three tiles per workgroup: the LDS image and the W buffer re-used
    behind lds_wave_sync, a shorter tile after a longer one, a partial last tile that is its wave's second or third,
    tile_range's XCD sweep over uneven eighths, project_final_kernel over 512 parts;
  * project_csr_kernel<8> / <64> with more chunks than waves; inner_kernel with more than one sweep;
  * ranges that start inside a tile of the global numbering (a.e_begin != own_begin, the offsets into V and elem_ptr,
    an odd base - base_al), against the lower- and the higher-numbered neighbour;
  * HDD_MAX_COMP = 8 components (blockIdx.y = q n_panels + panel up to 8 x 3 rows);
  * U = None on the tile path, out=, ranges without rows or without columns.

Sizes: project_grid_cases.py derives the meshes from the device's CU count and returns their facts
(test_project_grid_cases.py asserts them on the host); every test asserts the facts it needs before the call it guards.
On 256 CUs: p1 / p1_block Kuhn 130 x 255 (px = 2), q1 cube 182 x 181, hex 16 x 16 x 17.

Reference and tolerance are test_gpu_project.py's, nothing tuned: scipy on the downloaded arrays in float64,
|G - G_ref| <= 2 gamma_K |V|^T |A_q| |U| with K = rows + max row length + 3, exact zeros where the scale is zero;
H.inner: 2 gamma_n |V| |W|^T.  Every large case is assembled once per session, every reference computed once."""
import ctypes as C

import numpy as np
import pytest

import project_grid_cases as PG
import test_gpu_apply_grid as AG
import test_gpu_project as TP
from cases import SPE10_LOWER, SPE10_UPPER, os2014_components
from test_gpu_apply import Case, case, gamma, strided
from test_gpu_project import both_paths, check

H = pytest.importorskip("hdd_amd")
sp = pytest.importorskip("scipy.sparse")
pytestmark = pytest.mark.gpu

TILE_KERNEL = {"p1": "project_tile_kernel<3, 3>", "p1_block": "project_tile_kernel<3, 3>", "q1": "project_tile_kernel<4, 4>"}


def _torch():
    import torch
    return torch


def n_cu():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _kappas():
    """two smooth components on the SPE10 box"""
    return [H.scalar_fn(H.FN_SINUSOID, 1.0, b=0.5, kx=3.0, ky=2.0, order=3),
            H.scalar_fn(H.FN_SINUSOID, 0.3, b=1.0, kx=2.0, ky=5.0, order=3)]


_CASES = {}


def grid_case(ctx, name):
    """(case, facts) of the large cases, assembled once per session"""
    if name in _CASES:
        return _CASES[name]
    if name in ("p1", "p1_block"):
        f = PG.p1_size(n_cu())
        part = dict(px=2, py=1) if name == "p1_block" else {}
        c = Case(ctx, H.Grid.structured(H.SIMPLEX, f["nx"], f["ny"], SPE10_LOWER, SPE10_UPPER, **part), kappas=_kappas())
    elif name == "q1":
        f = PG.q1_size(n_cu())
        c = Case(ctx, H.Grid.structured(H.CUBE, f["nx"], f["ny"], SPE10_LOWER, SPE10_UPPER), kappas=_kappas())
    elif name == "hex":
        f = PG.hex_size(n_cu())
        c = Case(ctx, H.Grid.structured3d(f["n"], degree=1), tensor=H.tensor_fn(dim=3), prm=H.params_for(1, 3))
    elif name == "p1_small_block":
        nx, ny, px = PG.P1_SMALL_BLOCK
        f = None
        c = Case(ctx, H.Grid.structured(H.SIMPLEX, nx, ny, SPE10_LOWER, SPE10_UPPER, px=px, py=1))
    elif name == "os2014_eight":
        (c0, b0, kx, ky), second = os2014_components()
        comps = [(c0, b0, kx, ky), second, (0.5, 0.3, 2 * kx, ky), (0.2, 0.1, kx, 2 * ky), (0.7, -0.2, 0.5 * kx, ky),
                 (0.9, 0.4, kx, 0.5 * ky), (0.4, 0.25, 3 * kx, 2 * ky), (0.6, -0.35, 0.5 * kx, 3 * ky)]
        f = None
        c = Case(ctx, H.Grid.structured(H.SIMPLEX, 16, 16, (-1, -1), (1, 1)),
                 kappas=[H.scalar_fn(H.FN_SINUSOID, a, b, k, l, order=3) for (a, b, k, l) in comps], tensor=H.tensor_fn())
    else:
        raise KeyError(name)
    _CASES[name] = (c, f)
    return c, f


def tile_facts_hold(c, t, kind, min_tiles, max_tiles, n_el=None):
    """the input conditions of a tile-path call on n_el elements (default: the whole mesh): the 512-part cap below the
    tile count, min .. max tiles per workgroup, uneven eighths, a partial last tile that is not its wave's first"""
    n_el = c.local.n_own if n_el is None else n_el
    assert H.project_workspace(1, 1, 1) == PG.PROJECT_BLOCKS
    assert n_el == t["n_el"] and t["n_tiles"] == -(-n_el // 64)
    assert t["parts"] == PG.project_parts(n_cu(), kind, t["n_tiles"]) == PG.PROJECT_BLOCKS < t["n_tiles"]
    per_wave = PG.tiles_per_wave(t["parts"], t["n_tiles"])
    assert np.array_equal(per_wave, AG.tiles_per_wave(t["parts"], t["n_tiles"])) and per_wave.sum() == t["n_tiles"]
    assert (per_wave.min(), per_wave.max()) == (t["min_tiles"], t["max_tiles"]) == (min_tiles, max_tiles)
    assert t["n_tiles"] % 8 != 0 and len(set(t["eighths"])) > 1
    assert 0 < t["last_tile"] == n_el - 64 * (t["n_tiles"] - 1) < 64 and t["last_tile_position"] > 0
    assert PG.tile_conditions(t, min_tiles, max_tiles)


def csr_facts_hold(c, s, group, rows=None):
    """the input conditions of a CSR-path call: the kernel taken, its 512 parts, a second chunk for some wave"""
    rows = c.n_rows if rows is None else rows
    assert (c.dp.nnz // c.n_rows > 32) == (group == 64)                     # plan_apply's short_rows
    rw = PG.CSR_ROWS["csr%d" % group]
    assert s["rows"] == rows and s["parts"] == PG.project_parts(n_cu(), "csr%d" % group, rows) == PG.PROJECT_BLOCKS
    per_wave = PG.chunks_per_wave(s["parts"], rows, rw)
    assert per_wave.sum() == s["chunks"] == -(-rows // rw) > s["waves"] == 4 * s["parts"]
    assert per_wave.max() == s["max_chunks"] >= 2 and per_wave.min() == s["min_chunks"]


def grid_facts(c, f, name):
    """asserts the facts of the module docstring for a whole-mesh call on a large case"""
    if name == "hex":
        assert PG.hex_conditions(f) and c.n_rows == f["rows"] == 8 * c.local.n_own and c.dp.nnz == f["nnz"]
        csr_facts_hold(c, f["csr"], 64)
        return
    nb = 3 if name.startswith("p1") else 4
    assert c.n_rows == nb * c.local.n_own == c.n_cols and len(c.vals) == 2
    if nb == 3:
        assert PG.p1_conditions(f)
        tile_facts_hold(c, f["tile"], "p1", 2, 3)
        assert f["csr"]["min_chunks"] >= 2
    else:
        assert PG.q1_conditions(f)
        tile_facts_hold(c, f["tile"], "q1", 1, 2)
        assert f["csr"]["chunks"] > 2 * f["csr"]["waves"]
    csr_facts_hold(c, f["csr"], 8)


_REFERENCES = {}


@pytest.fixture(autouse=True)
def shared_references(monkeypatch):
    """both_paths computes its references through test_gpu_project.project_reference: the same function, remembered
    per (value array, range, bases), so that every reference is computed once"""
    plain = TP.project_reference

    def remembered(rp, col, hv, shape, rng, V, Uv):
        key = (id(rp), id(hv), rng, V.shape, Uv.shape, V.tobytes()[:64], Uv.tobytes()[:64])
        if key not in _REFERENCES:
            _REFERENCES[key] = plain(rp, col, hv, shape, rng, V, Uv)
        return _REFERENCES[key]
    monkeypatch.setattr(TP, "project_reference", remembered)
    return remembered


def worst_fraction(G, refs):
    """max over components and entries of error / bound"""
    g = G.cpu().numpy()
    return max(float((np.abs(g[q] - ref)[bound > 0] / bound[bound > 0]).max()) for q, (ref, bound) in enumerate(refs))


def report(what, c, rng, V, Uv, Gt, Gc, remembered, first="tile"):
    """prints the worst error / bound of the two results of both_paths (first: the path taken with the mesh given)"""
    refs = [remembered(c.rp, c.col, hv, (c.n_rows, c.n_cols), rng, V, Uv) for hv in c.hvals]
    print("project %s %d x %d: worst error / bound: %s %.3e, csr %.3e"
          % (what, V.shape[0], Uv.shape[0], first, worst_fraction(Gt, refs), worst_fraction(Gc, refs)))


def _bases(seed, n_v, n_u, rows, cols):
    r = np.random.default_rng(seed)
    return r.standard_normal((n_v, rows)), r.standard_normal((n_u, cols))


@pytest.mark.parametrize("name", ["p1", "q1"])
@pytest.mark.parametrize("n_v,n_u", [(1, 1), (33, 17)])
def test_persistent_tiles_and_csr_passes(ctx, shared_references, name, n_v, n_u):
    """512 parts below the tile count (p1: two and three tiles per workgroup, q1: one and two) and more CSR chunks than
    waves, two components, rows strided with NaN padding (both_paths)"""
    torch = _torch()
    c, f = grid_case(ctx, name)
    grid_facts(c, f, name)
    V, Uv = _bases(2000 + 64 * n_v + n_u, n_v, n_u, c.n_rows, c.n_cols)
    Gt, Gc = both_paths(ctx, c, V, Uv)
    assert H.last_apply_kernel() == "project_csr_kernel<8>"
    again = H.project(ctx, c.dp, c.vals, strided(V, 3), strided(Uv, 5), dmesh=c.dm)
    assert H.last_apply_kernel() == TILE_KERNEL[name] and torch.equal(again, Gt)
    report(name, c, None, V, Uv, Gt, Gc, shared_references)


def test_hexahedra_csr_passes(ctx, shared_references):
    """a wave per row, 2,176 chunks of 16 rows over 2,048 waves"""
    c, f = grid_case(ctx, "hex")
    grid_facts(c, f, "hex")
    V, Uv = _bases(2100, 17, 33, c.n_rows, c.n_cols)
    Gt, Gc = both_paths(ctx, c, V, Uv, tile=False)
    assert H.last_apply_kernel() == "project_csr_kernel<64>"
    report("hex", c, None, V, Uv, Gt, Gc, shared_references, first="csr (mesh given)")


def block_range_on_both_paths(ctx, c, ss, nn, seed, n_v=17, n_u=9):
    """test_gpu_project.test_block_ranges for one pair: the operator (ss, nn) on both paths against the sliced
    reference, then with NaN in every value outside the column range: the same bits"""
    torch = _torch()
    nb = c.grid.nb
    a, b = c.grid.subdomain_range(ss, ss + 1)
    p, q = c.grid.subdomain_range(nn, nn + 1)
    rng = (a * nb, b * nb, p * nb, q * nb)
    V, Uv = _bases(seed, n_v, n_u, rng[1] - rng[0], rng[3] - rng[2])
    Gt, Gc = both_paths(ctx, c, V, Uv, block=(ss, nn), rng=rng)
    if ss != nn:
        assert bool((Gt != 0).any()) and bool((Gc != 0).any())     # the coupling is there
    outside = torch.from_numpy((c.col < rng[2]) | (c.col >= rng[3])).cuda()
    assert bool(outside.any())
    poisoned = [torch.where(outside, torch.full_like(v, float("nan")), v) for v in c.vals]
    vd, ud = strided(V, 3), strided(Uv, 5)     # NaN behind every row
    for dm, clean in ((c.dm, Gt), (None, Gc)):
        G = H.project(ctx, c.dp, poisoned, vd, ud, dmesh=dm, block=(ss, nn))
        assert bool(torch.isfinite(G).all()) and torch.equal(G, clean)
    return rng, V, Uv, Gt, Gc


@pytest.mark.parametrize("ss,nn", [(1, 1), (1, 0), (0, 1)])
def test_block_ranges_off_the_tile_boundary_large(ctx, shared_references, ss, nn):
    """Kuhn 130 x 255 in two slabs: subdomain 1 starts 62 elements into a tile of the global numbering at an odd value
    offset, its 518 tiles meet the 512-part cap (one and two tiles per workgroup); rows and / or columns off the origin"""
    c, f = grid_case(ctx, "p1_block")
    assert c.grid.n_sub == 2 and c.local.own_begin == 0 and PG.p1_conditions(f)
    a, b = c.grid.subdomain_range(ss, ss + 1)
    p, _ = c.grid.subdomain_range(nn, nn + 1)
    off = c.grid.subdomain_range(1, 2)[0]
    assert off == f["sub_start"] and off % 64 != 0 and c.ep[off] % 2 == 1 and (a, p) != (0, 0)
    assert a == (off if ss else 0) and p == (off if nn else 0)          # the row / column range off the tile boundary
    tile_facts_hold(c, f["sub_tile"], "p1", 1, 2, n_el=b - a)
    assert f["sub_tile"]["n_tiles"] > PG.PROJECT_BLOCKS
    csr_facts_hold(c, f["sub_csr"], 8, rows=3 * (b - a))
    rng, V, Uv, Gt, Gc = block_range_on_both_paths(ctx, c, ss, nn, 2200 + 4 * ss + nn)
    report("p1_block (%d, %d)" % (ss, nn), c, rng, V, Uv, Gt, Gc, shared_references)


def _pairs_off_the_origin(c):
    starts = [c.grid.subdomain_range(s, s + 1)[0] for s in range(c.grid.n_sub)]
    return starts, [(ss, nn) for ss, nn in PG.coupled_pairs(c.local.neighbors, starts) if ss != 0]


def test_block_ranges_off_the_tile_boundary_small(ctx):
    """every coupled pair with ss != 0 of the cube 16 x 12 in 2 x 2 (48 elements each) and of Kuhn 18 x 5 in three
    slabs (60 each, odd base - base_al at both inner starts): the lower- and the higher-numbered neighbour"""
    c = case(ctx, "q1_block")
    starts, pairs = _pairs_off_the_origin(c)
    assert starts == [0, 48, 96, 144] and len(pairs) == 9 and all(starts[ss] % 64 != 0 for ss, _ in pairs)
    for ss, nn in pairs:
        block_range_on_both_paths(ctx, c, ss, nn, 2300 + 4 * ss + nn)
    c, _ = grid_case(ctx, "p1_small_block")
    starts, pairs = _pairs_off_the_origin(c)
    assert starts == [0, 60, 120] and pairs == [(1, 0), (1, 1), (1, 2), (2, 1), (2, 2)]
    assert all(starts[ss] % 64 != 0 and c.ep[starts[ss]] % 2 == 1 for ss, _ in pairs)
    assert np.array_equal(c.ep, PG.elem_ptr(c.local.neighbors, 3))
    for ss, nn in pairs:
        block_range_on_both_paths(ctx, c, ss, nn, 2400 + 4 * ss + nn)


def test_eight_components(ctx, shared_references):
    """HDD_MAX_COMP value arrays on the OS2014 mesh, 17 x 33 (three panels: 24 workgroup rows): every component
    against its own reference on both paths, no two components equal"""
    c, _ = grid_case(ctx, "os2014_eight")
    assert len(c.vals) == H.MAX_COMP == PG.MAX_COMP == 8
    assert all(not np.array_equal(c.hvals[i], c.hvals[j]) for i in range(8) for j in range(i))
    V, Uv = _bases(2500, 17, 33, c.n_rows, c.n_cols)
    Gt, Gc = both_paths(ctx, c, V, Uv)
    assert Gt.shape == Gc.shape == (8, 17, 33)
    for g in (Gt.cpu().numpy(), Gc.cpu().numpy()):
        assert all(not np.array_equal(g[i], g[j]) for i in range(8) for j in range(i))
    report("eight components", c, None, V, Uv, Gt, Gc, shared_references)


@pytest.mark.parametrize("name,tile", [("p1", True), ("p1", False), ("hex", False)])
def test_bit_identity_at_scale(ctx, name, tile):
    """two calls give equal bits; entries of the 33 x 17 call have the bits of the 1 x 1 calls on the same vectors;
    permuted vectors give the permuted result -- with several tiles / chunks per wave and 512 parts"""
    torch = _torch()
    c, f = grid_case(ctx, name)
    grid_facts(c, f, name)
    dm = c.dm if tile else None
    want = TILE_KERNEL[name] if tile else ("project_csr_kernel<64>" if name == "hex" else "project_csr_kernel<8>")
    V, Uv = _bases(2600, 33, 17, c.n_rows, c.n_cols)
    vd, ud = strided(V, 3), strided(Uv, 5)
    G = H.project(ctx, c.dp, c.vals, vd, ud, dmesh=dm)
    assert H.last_apply_kernel() == want
    assert G.shape == (len(c.vals), 33, 17) and bool(torch.isfinite(G).all()) and bool((G != 0).all())
    assert torch.equal(G, H.project(ctx, c.dp, c.vals, vd, ud, dmesh=dm))
    for i, j in [(0, 0), (16, 16), (32, 16)]:
        one = H.project(ctx, c.dp, c.vals, vd[i], ud[j], dmesh=dm)
        assert one.shape == (len(c.vals), 1, 1) and torch.equal(one[:, 0, 0], G[:, i, j]), (i, j)
    r = np.random.default_rng(5)
    pv, pu = r.permutation(33), r.permutation(17)
    Gp = H.project(ctx, c.dp, c.vals, strided(V[pv], 1), strided(Uv[pu], 2), dmesh=dm)
    assert H.last_apply_kernel() == want
    assert torch.equal(Gp, G[:, torch.from_numpy(pv).cuda()][:, :, torch.from_numpy(pu).cuda()])


@pytest.mark.parametrize("n", PG.INNER_N)
@pytest.mark.parametrize("n_v,n_w", [(1, 1), (17, 33)])
def test_inner_past_one_sweep(ctx, n_v, n_w, n):
    """inner_kernel at its 512 parts: a second 64-entry pass for one wave (n = 131,073) and three to four passes with a
    ragged end (3 x 131,072 + 77)"""
    torch = _torch()
    assert PG.inner_conditions(n) and H.project_workspace(1, 1, 1) == PG.inner_parts(n) == PG.PROJECT_BLOCKS
    passes = PG.inner_passes_per_wave(n)
    assert passes.max() >= 2 and (n % 64 != 0)
    r = np.random.default_rng(n % 1000 + 64 * n_v + n_w)
    V, W = r.standard_normal((n_v, n)), r.standard_normal((n_w, n))
    vd, wd = strided(V, 3), strided(W, 1)
    G = H.inner(ctx, vd, wd)
    assert G.shape == (n_v, n_w)
    bound = 2.0 * gamma(n) * (np.abs(V) @ np.abs(W).T)
    err = np.abs(G.cpu().numpy() - V @ W.T)
    print("inner n %d, %d x %d, passes per wave %d..%d: worst error / bound %.3e" % (n, n_v, n_w, passes.min(), passes.max(), (err / bound).max()))
    assert (err <= bound).all(), (float(err.max()), float(bound.min()))
    assert torch.equal(G, H.inner(ctx, vd, wd))


def test_gramian_and_out_argument(ctx):
    """U = None on the tile path is project(V, V) bit for bit; a NaN-filled out= comes back as the same object, fully
    overwritten; an out of another shape or layout is refused"""
    torch = _torch()
    c = case(ctx, "p1")
    V, _ = _bases(2700, 20, 1, c.n_rows, c.n_cols)
    vd = strided(V, 3)
    G = H.project(ctx, c.dp, c.vals, vd, dmesh=c.dm)
    assert H.last_apply_kernel() == "project_tile_kernel<3, 3>"
    full = H.project(ctx, c.dp, c.vals, vd, strided(V, 5), dmesh=c.dm)
    assert G.shape == (1, 20, 20) and torch.equal(G, full)
    check(G, [TP.project_reference(c.rp, c.col, c.hvals[0], (c.n_rows, c.n_cols), None, V, V)], "U=None")
    for dm in (c.dm, None):
        clean = H.project(ctx, c.dp, c.vals, vd, dmesh=dm)
        out = torch.full((1, 20, 20), float("nan"), dtype=torch.float64, device="cuda")
        ret = H.project(ctx, c.dp, c.vals, vd, dmesh=dm, out=out)
        assert ret is out and bool(torch.isfinite(out).all()) and torch.equal(out, clean)
    with pytest.raises(H.HddError, match="out must be"):
        H.project(ctx, c.dp, c.vals, vd, dmesh=c.dm, out=torch.zeros((1, 20, 21), dtype=torch.float64, device="cuda"))
    with pytest.raises(H.HddError, match="out must be"):
        H.project(ctx, c.dp, c.vals, vd, dmesh=c.dm, out=torch.zeros((1, 20, 40), dtype=torch.float64, device="cuda")[:, :, ::2])
    with pytest.raises(H.HddError, match="out must be"):
        H.project(ctx, c.dp, c.vals, vd, dmesh=c.dm, out=torch.zeros((1, 20, 20), dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("tile", [True, False])
def test_ranges_without_rows_or_columns(ctx, tile):
    """no rows: no launch, the sum over no parts; no columns: every block skipped.  Exact zeros into a NaN-filled out.
    Through the C ABI: H.project cannot express these ranges -- a tensor without entries has a null data pointer, which
    hdd_operator_project refuses -- so the calls pass the padded buffers' own pointers"""
    torch = _torch()
    c = case(ctx, "p1")
    dm = c.dm if tile else None
    assert len(c.vals) == 1 and c.n_rows > 300 and c.n_cols > 300
    vals = (C.c_void_p * 1)(c.vals[0].data_ptr())
    r = np.random.default_rng(2800)
    for rng in ((192, 192, 0, c.n_cols), (0, c.n_rows, 192, 192), (192, 192, 300, 300)):
        rows, cols = rng[1] - rng[0], rng[3] - rng[2]
        vbuf, ubuf = strided(r.standard_normal((5, rows)), 3)._base, strided(r.standard_normal((18, cols)), 5)._base   # NaN padding
        assert vbuf.shape == (5, rows + 3) and ubuf.shape == (18, cols + 5) and vbuf.data_ptr() and ubuf.data_ptr()
        work = torch.full((H.project_workspace(1, 5, 18),), float("nan"), dtype=torch.float64, device="cuda")
        out = torch.full((1, 5, 18), float("nan"), dtype=torch.float64, device="cuda")
        br = H.BlockRange(*rng)
        rc = H.lib().hdd_operator_project(ctx.h, None if dm is None else C.addressof(dm.t), C.addressof(c.dp.t), vals, 1,
                                          C.addressof(br), vbuf.data_ptr(), vbuf.stride(0), 5, ubuf.data_ptr(), ubuf.stride(0), 18,
                                          work.data_ptr(), work.numel(), out.data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (rng, H.lib().hdd_last_error(None))
        assert H.last_apply_kernel() == ("project_tile_kernel<3, 3>" if tile else "project_csr_kernel<8>")
        torch.cuda.synchronize()
        assert bool((out == 0).all()), rng
