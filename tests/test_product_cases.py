"""Preconditions of the product GPU tests (tests/product_cases.py), on the host.

The GPU tests rely on properties of their meshes that they cannot observe from the values: that full-interior tiles
(the branch-free ALLIN path of the penalty) and a ragged last tile are present, that orientations and face directions
are mixed, that the rank-local views start above element 0 with ghosts on both sides and number their elements in
ascending global order (the generic kernel sorts a penalty row's column blocks by local id, the pattern by global id),
that an all-Neumann mesh carries only the Neumann code, and that the multi-pass meshes have more tiles than the
persistent grid has workgroups.  These tests assert them, that every oracle reference is nonzero where it should be,
and that the oracle's own products pass the invariants the GPU values are held to.  CPU only."""
import numpy as np
import pytest

import hdd_amd as H
import oracle as O
import product_cases as P

ETS = list(P.ETS)
VIEWS = [("slab", 9, 18, 144), ("split", 10, 20, None)]


@pytest.mark.parametrize("et", ETS)
def test_scrambled_mesh(et):
    c = P.case("scrambled", et)
    loc = c.local()
    assert loc.own_begin == 0 and np.array_equal(loc.global_id, np.arange(c.grid.ne))
    _, coords, ev = P.scrambled_connectivity(et)
    assert np.array_equal(c.pc, coords) and np.array_equal(c.pev, ev)       # element order kept
    assert np.array_equal(loc.coords, P.element_major(coords, ev))
    det = P.signed_dets(coords, ev)
    neg = float((det < 0).mean())
    rev, slots = P.reversed_faces(loc)
    print("scrambled %s: %d elements, tiles %s, det < 0 on %.1f %%, %d elements with a reversed face (%d slots)"
          % (P.ET_NAME[et], c.grid.ne, P.full_interior_tiles(loc), 100 * neg, rev, slots))
    if et == H.SIMPLEX:
        assert c.grid.ne == 308 and P.full_interior_tiles(loc) == (4, 4, 52)
        assert rev == 251 and slots == 408 and 0.53 < neg < 0.55
    else:
        assert c.grid.ne == 300 and P.full_interior_tiles(loc) == (3, 4, 44)
        assert rev == 282 and slots == 614 and 0.48 < neg < 0.50
    # the neighbour blocks of a row take more than one order: in a full-interior tile, neighbours sort differently
    nbr = loc.neighbors[:, :64]
    orders = {tuple(np.argsort(np.r_[e, nbr[:, e]], kind="stable")) for e in range(64)}
    assert len(orders) > 4
    # a general Jacobian: all four entries nonzero on every element
    cm = loc.coords
    assert np.all(np.abs(np.stack([cm[2] - cm[0], cm[3] - cm[1], cm[4] - cm[0], cm[5] - cm[1]])).min(axis=0) > 0)


def test_nvb_mesh():
    c = P.case("nvb", H.SIMPLEX)
    loc = c.local()
    assert np.array_equal(loc.global_id, np.arange(c.grid.ne))
    assert P.reversed_faces(loc)[0] > 0
    det = P.signed_dets(c.pc, c.pev)
    assert np.any(det < 0) and np.any(det > 0)
    assert c.tiles() > 1 and loc.n_own % 64 == 0                    # bisection doubles: 256 triangles, full tiles only


@pytest.mark.parametrize("et", ETS)
@pytest.mark.parametrize("name,own_begin,ghosts,n_own", VIEWS)
def test_local_views(name, own_begin, ghosts, n_own, et):
    c = P.case(name, et)
    loc = c.local()
    a, b = c.rows
    assert loc.own_begin == own_begin > 0 and loc.n_ghost == ghosts and loc.own_end < loc.n_local
    assert loc.n_own == b - a and (n_own is None or loc.n_own == n_own)
    assert np.all(np.diff(loc.global_id) > 0)                       # local order = global order: block orders agree
    assert np.array_equal(loc.global_id[loc.own_begin:loc.own_end], np.arange(a, b))
    gh = np.r_[loc.global_id[:loc.own_begin], loc.global_id[loc.own_end:]]
    assert np.any(gh < a) and np.any(gh >= b)                       # ghosts on both sides of the owned range
    own_nbr = loc.neighbors[:, loc.own_begin:loc.own_end]
    ghost_nbr = (own_nbr >= 0) & ((own_nbr < loc.own_begin) | (own_nbr >= loc.own_end))
    assert ghost_nbr.any()
    if name == "slab":
        nfull_int, nfull, ragged = P.full_interior_tiles(loc)
        assert (nfull, ragged) == (2, 16) and nfull_int >= 1
        tiles_int = (own_nbr >= 0).all(axis=0)[:128].reshape(2, 64).all(axis=1)
        assert np.any(tiles_int & ghost_nbr.any(axis=0)[:128].reshape(2, 64).any(axis=1))   # a full-interior tile
        #                                                                     with ghost neighbours
    assert np.any(own_nbr == H.NBR_DIRICHLET)                       # and the domain boundary is in the view
    # the view's host patterns are the row slices of the oracle's, columns included
    for kind in (H.PRODUCT_L2, H.PRODUCT_PENALTY):
        rp, col, _ = loc.pattern(volume=kind != H.PRODUCT_PENALTY)
        orp, ocol, _ = P.reference(name, et, kind)
        assert np.array_equal(rp, orp) and np.array_equal(col, ocol)


@pytest.mark.parametrize("et", ETS)
@pytest.mark.parametrize("shape", P.EDGE_SHAPES)
def test_edge_meshes(shape, et):
    c = P.case("edge_%dx%d" % shape, et)
    per = 2 if et == H.SIMPLEX else 1
    assert c.grid.ne == per * shape[0] * shape[1]
    loc = c.local()
    assert np.all((loc.neighbors < 0).sum(axis=0) >= 1)             # every element touches the boundary
    s = P.case("single", et)                                        # (a Kuhn 1 x 1 grid has two triangles)
    assert s.grid.ne == 1 and np.all(s.local().neighbors < 0)
    for k in (c, s):
        if k.grid.ne == 1:                                          # no interior face: penalty pattern = volume pattern
            rp, col, _ = k.local().pattern()
            vrp, vcol, _ = k.local().pattern(volume=True)
            assert np.array_equal(rp, vrp) and np.array_equal(col, vcol) and col.shape[0] == k.nb * k.nb


@pytest.mark.parametrize("et", ETS)
def test_multipass_mesh(et):
    c = P.case("multipass", et)
    want = {H.SIMPLEX: (68400, 1069), H.CUBE: (68640, 1073)}[et]
    assert (c.grid.ne, c.tiles()) == want
    assert c.tiles() > 4 * P.MI355X_CUS                   # VolProductPolicy, vertex-indexed P1PwcPolicy: 4 per CU
    loc = c.local()
    assert np.array_equal(loc.global_id, np.arange(c.grid.ne))
    nfull_int, nfull, ragged = P.full_interior_tiles(loc)
    assert nfull_int > 0 and nfull_int < nfull and ragged > 0


@pytest.mark.parametrize("name", ["scrambled", "nvb", "slab", "split", "single", "edge_1x1", "edge_1x9", "edge_9x1"])
def test_neumann_meshes_carry_only_the_neumann_code(name):
    for et in P.mesh_ets(name):
        ld, ln = P.case(name, et, False).local(), P.case(name, et, True).local()
        d, n = (l.neighbors[:, l.own_begin:l.own_end] for l in (ld, ln))        # (ghost columns carry no faces)
        assert np.array_equal(d >= 0, n >= 0) and np.array_equal(d[d >= 0], n[n >= 0])
        assert np.all(d[d < 0] == H.NBR_DIRICHLET)
        assert np.all(n[n < 0] == H.NBR_NEUMANN) and H.NBR_NEUMANN == -2
        assert np.any(n < 0)


def test_coefficients():
    d = P.coeff_data("scrambled", H.SIMPLEX)
    a, b, c = d["sym"]
    assert np.all(a * c - b * b > 0) and np.all(a > 0) and np.any(np.abs(b) > 0.1)          # SPD, anisotropic
    assert d["iso"].max() / d["iso"].min() > 1e3 and d["kap"].max() / d["kap"].min() > 10
    t = P.TENSOR_CONST
    assert t[0] * t[2] - t[1] ** 2 > 0 and t[1] != 0
    loc = P.case("slab", H.CUBE).local()
    tv, kv = P.view_coeffs("slab", H.CUBE, "sym", "per_elem", loc.global_id)
    full = P.coeff_data("slab", H.CUBE)
    assert np.array_equal(tv[:, loc.own_begin], full["sym"][:, P.case("slab", H.CUBE).rows[0]])
    assert kv.shape == (loc.n_local,) and tv.shape == (3, loc.n_local)


@pytest.mark.parametrize("name", ["scrambled", "nvb", "slab", "split", "single", "edge_1x1", "edge_1x9", "edge_9x1"])
def test_references_are_nonzero_and_distinct(name):
    for et in P.mesh_ets(name):
        single = P.case(name, et).grid.ne == 1
        for kind in P.KINDS:
            for neumann in (False, True):
                _, _, v = P.reference(name, et, kind, neumann)
                zero_ok = kind == H.PRODUCT_PENALTY and neumann and single      # no face carries a penalty there
                assert (np.max(np.abs(v)) > 0) != zero_ok, (name, et, kind, neumann)
        # boundary_l2 keeps Neumann faces; the penalty drops them
        bd, bn = (P.reference(name, et, H.PRODUCT_BOUNDARY_L2, n)[2] for n in (False, True))
        assert np.array_equal(bd, bn) and (np.any(bd == 0.0) or single)
        pd, pn = (P.reference(name, et, H.PRODUCT_PENALTY, n)[2] for n in (False, True))
        assert not np.array_equal(pd, pn)
        # beta enters (|F| != 1), and so does every coefficient kind
        for neumann, p1 in ((False, pd), (True, pn)):
            if np.max(np.abs(p1)) > 0:                                          # (one element, all Neumann: all zero)
                p5 = P.reference(name, et, H.PRODUCT_PENALTY, neumann, beta=0.5)[2]
                assert np.max(np.abs(p5 - p1)) > 1e-3 * np.max(np.abs(p1)), (name, et, neumann)
        for kind in P.COEFF_KINDS:
            vals = [P.reference(name, et, kind, False, tk, kk)[2] for tk in P.TENSOR_KINDS
                    for kk in P.KAPPA_KINDS + (P.SMOOTH,)]
            for i in range(len(vals)):
                for j in range(i):
                    assert np.max(np.abs(vals[i] - vals[j])) > 1e-3 * np.max(np.abs(vals[i]))


def test_block_scale_sees_what_the_row_scale_hides():
    """one triangle's row block with a neighbour block 1e4 times weaker than its own, wrong by 1e-9 of itself; and the
    oracle's rounding in a neighbour block's mathematically zero row does not count"""
    rp = np.array([0, 6, 12, 18])
    ref = np.tile(np.r_[1e4, 5e3, 1e3, 1.0, 0.5, 0.0], 3)
    ref[12:15], ref[15:18] = [2e3, 1e3, 7e3], [0.0, 4e-15, 0.0]        # (row of the vertex opposite the weak face)
    got = ref.copy()
    got[9] *= 1 + 1e-9
    assert P.compare_rows(rp, got, ref, P.RTOL)[1]
    assert P.block_ratio(rp, got, ref, 3) > 1e-10 and P.block_ratio(rp, ref, ref, 3) == 0.0
    with pytest.raises(AssertionError):
        P.check_blocks("synthetic", rp, got, ref, 3)
    clean = ref.copy()
    clean[16] = 0.0
    assert P.block_ratio(rp, clean, ref, 3) <= 1e-14
    bad = ref.copy()
    bad[5] = 1e-300
    with pytest.raises(AssertionError):
        P.check_exact_zeros("synthetic", bad, ref)
    nan = ref.copy()
    nan[0] = np.nan
    with pytest.raises(AssertionError):
        P.check_rows("synthetic", rp, nan, ref)
    # two elements with different block counts
    rp2 = np.r_[np.arange(0, 19, 6), 18 + np.arange(3, 10, 3)]
    ref2 = np.r_[ref, np.arange(1.0, 10.0)]
    got2 = ref2.copy()
    got2[-1] += 1e-6
    assert abs(P.block_ratio(rp2, got2, ref2, 3) - 1e-6 / 9.0) < 1e-12


@pytest.mark.parametrize("name", ["scrambled", "nvb", "slab", "split", "single", "edge_1x1", "edge_1x9", "edge_9x1",
                                  "multipass"])
def test_penalty_zero_rows(name):
    """the rows that the mesh says vanish are the rows where the oracle holds nothing but rounding, and no others: none
    under all-Dirichlet; under all-Neumann the corner elements' vertices off every interior face"""
    for et in P.mesh_ets(name):
        for neumann in (False, True):
            c = P.case(name, et, neumann)
            z = P.penalty_zero_rows(c)
            rp, _, ref = P.reference(name, et, H.PRODUCT_PENALTY, neumann)
            assert z.shape == (rp.shape[0] - 1,)
            scale = np.maximum.reduceat(np.abs(ref), rp[:-1])
            elem = np.repeat(scale.reshape(-1, c.nb).max(axis=1), c.nb)
            if c.grid.ne == 1 and neumann:
                assert z.all() and not ref.any()
                continue
            assert z.sum() <= (4 if neumann else 0)                              # (at most the domain's corners)
            assert z.any() == (neumann and name in ("scrambled", "edge_1x1", "edge_1x9", "edge_9x1", "multipass"))
            assert np.all(scale[z] <= 1e-12 * elem[z]) and np.all(scale[~z] > 1e-6 * elem[~z])
            got = ref.copy()
            got[rp[:-1][z]] = 0.0                                      # exact zeros where the oracle has noise
            assert P.row_ratio(rp, got, ref, c.nb, z) <= P.RTOL
            assert P.row_ratio(rp, ref, ref, c.nb) == 0.0
            bad = ref * (1 + 1e-9)                                               # every other row: compare_rows' ratio
            assert abs(P.row_ratio(rp, bad, ref, c.nb, z) - 1e-9) < 1e-12
            assert abs(P.row_ratio(rp, bad, ref, c.nb) - P.compare_rows_fast(rp, bad, ref)[0]) < 1e-20
            if z.any():
                wrong = ref.copy()
                wrong[rp[:-1][z]] = elem[z] * 1e-9                               # something real in such a row is seen
                assert P.row_ratio(rp, wrong, ref, c.nb, z) > 1e-10


@pytest.mark.parametrize("name", ["scrambled", "nvb", "slab", "split"])
def test_oracle_passes_the_invariants(name):
    worst = {}
    for et in P.mesh_ets(name):
        for neumann in (False, True):
            c = P.case(name, et, neumann)
            for kind in P.KINDS:
                rp, col, val = P.reference(name, et, kind, neumann)
                P.check_invariants("oracle %s %s" % (c.label(), P.KIND_NAME[kind]), c, kind, rp, col, val, worst)
    print("oracle invariants %s: worst %.3g" % (name, worst["invariants"]))


def test_invariants_catch_a_wrong_product():
    c = P.case("nvb", H.SIMPLEX, True)
    rp, col, val = P.reference("nvb", H.SIMPLEX, H.PRODUCT_PENALTY, True)
    rd = P.reference("nvb", H.SIMPLEX, H.PRODUCT_PENALTY, False)[2]
    with pytest.raises(AssertionError):                              # Neumann faces penalised like Dirichlet ones
        P.check_invariants("dirichlet values on the neumann mesh", c, H.PRODUCT_PENALTY, rp, col, rd)
    rp, col, val = P.reference("nvb", H.SIMPLEX, H.PRODUCT_ELLIPTIC)
    flipped = val.copy().reshape(-1, 9)
    flipped[P.signed_dets(c.pc, c.pev) < 0] *= -1.0                  # det where |det| belongs
    r = P.invariant_ratios(c, H.PRODUCT_ELLIPTIC, rp, col, flipped.reshape(-1))
    assert r["symmetry"] <= P.RTOL and r["constants"] <= P.RTOL     # (invisible to the invariants: the oracle sees it)
    assert not P.compare_rows(rp, flipped.reshape(-1), val, P.RTOL)[1]
