"""The Q_p oracle (oracle/swipdg_oracle_qp.c, C5 = ESV2007 3d structured, SWIPDG p=3) -- CPU only.

Pinning: at d=2, p=1 it must reproduce the 2D oracle (pinned to the reference's ESV2007 expectation
tables, test_oracle_pinning.py) entry for entry, and it reproduces the SGrid table itself.  For p>1 and
d=3 the reference holds no fixture (its ESV2007 testcase is 2D-only, testcases/ESV2007.hh:32): parity
unpinned, checked instead by the known-answer invariants of SURVEY.md 8(c)-3 and by the convergence of
the ESV2007 exact solution.  Also checks the product's 3d host grid and patterns against the oracle.

Graded (rectilinear) grids: QpGrid(nodes=...) replaces the equidistant breakpoints in the oracle's geometry() and
nothing else.  Anchors: equidistant breakpoints reproduce nodes=None bit for bit; at d=2, p=1 a graded grid
reproduces the pinned 2D oracle on the same coordinates (to rounding: that oracle derives its Jacobian from vertex
coordinates along another route); in 3d the invariants above plus A.1 = b(g_D = 1), which couples every face's two
sides (own and neighbour geometry, |F|^beta) with the boundary terms."""
import numpy as np
import pytest

import hdd_amd as H
import oracle as O
from cases import compare_rows
from hex_tools import GRADED_NODES, graded_hex_mesh, lex_to_product, lex_to_product_graded


@pytest.mark.parametrize("nx,ny", [(4, 5), (8, 8)])
def test_qp_d2_p1_equals_pinned_2d_oracle(nx, ny):
    g2 = O.Grid(*O.cube_grid(nx, ny, (-1, -1), (1, 1)))
    q = O.QpGrid(2, 1, (nx, ny), (-1, -1), (1, 1))
    kk = np.random.default_rng(3).uniform(0.1, 5, g2.ne)
    for kap, ten2, tenq in [
        (O.scalar(), O.tensor(), O.qp_tensor(dim=2)),
        (O.scalar(O.FN_SINUSOID, 1.0, 0.5, 3, 2, order=3), O.tensor(O.TENSOR_ISO_PER_ELEM, per_elem=kk),
         O.qp_tensor(O.TENSOR_ISO_PER_ELEM, per_elem=kk, dim=2)),
    ]:
        rp, col, val = O.assemble(g2, kap, ten2, O.params())
        rq, cq, vq = O.qp_assemble(q, kap, tenq, O.qp_params(q))
        assert np.array_equal(rp, rq) and np.array_equal(col, cq)
        assert np.array_equal(val, vq)


def test_qp_reproduces_esv2007_sgrid_table():
    # test/linearelliptic-swipdg-expectations_esv2007_2dsgrid.cxx:31-36 (L2, 3 s.f.)
    for n, ref in [(8, 1.13e-02), (16, 2.90e-03), (32, 7.41e-04)]:
        l2, _ = O.qp_esv2007_errors(O.QpGrid(2, 1, (n, n), (-1, -1), (1, 1)))
        assert abs(l2 - ref) / ref < 5e-3


@pytest.mark.parametrize("dim,p,ns,rate", [(2, 3, (4, 8), 3.5), (3, 2, (2, 4), 2.0), (3, 3, (2, 4), 3.5)])
def test_qp_convergence(dim, p, ns, rate):
    errs = [O.qp_esv2007_errors(O.QpGrid(dim, p, (n,) * dim, (-1,) * dim, (1,) * dim))[0] for n in ns]
    assert np.log2(errs[0] / errs[1]) > rate


@pytest.mark.parametrize("p", [1, 2, 3])
def test_qp_3d_invariants(p):
    """Symmetry, A.1 = 0 on rows of elements without Dirichlet faces, SPD.
    SPD needs an exact volume rule for p >= 2: the reference's integrand order 2(p-1) under-integrates
    Q_p gradients (3 Gauss points per direction at p=3) and the matrix is then indefinite on anisotropic
    hexahedra -- a property of the reference's quadrature choice, kept as is."""
    import scipy.linalg as sl
    q = O.QpGrid(3, p, (3, 3, 3), (0, 0, 0), (1, 1.5, 2))
    rp, col, val = O.qp_assemble(q, O.scalar(), O.qp_tensor(), O.qp_params(q))
    A = O.to_scipy(rp, col, val).toarray()
    assert np.max(np.abs(A - A.T)) <= 1e-12 * np.max(np.abs(A))
    e_int = 1 + 3 * (1 + 3 * 1)                       # the centre element (1,1,1) has no boundary face
    rows = slice(e_int * q.nb, (e_int + 1) * q.nb)
    assert np.max(np.abs(A[rows].sum(axis=1))) <= 1e-11 * np.max(np.abs(A))
    if p == 1:
        assert sl.eigvalsh(A).min() > 0
    rp, col, val = O.qp_assemble(q, O.scalar(), O.qp_tensor(), O.qp_params(q, vol_order=2 * p))
    assert sl.eigvalsh(O.to_scipy(rp, col, val).toarray()).min() > 0


@pytest.mark.parametrize("n,parts,deg", [((3, 4, 5), (1, 1, 1), 1), ((4, 3, 2), (2, 1, 1), 2), ((6, 4, 4), (3, 2, 2), 3)])
def test_structured3d_grid_and_pattern_match_oracle(n, parts, deg):
    lo, up = (-1.0, 0.0, 0.5), (1.0, 2.0, 1.5)
    g = H.Grid.structured3d(n, lo, up, p=parts, degree=deg)
    assert g.dim == 3 and g.nf == 6 and g.nvpe == 8 and g.nb == (deg + 1) ** 3 and g.ne == np.prod(n)
    assert g.n_sub == np.prod(parts)
    ei = lex_to_product(g, n, lo, up)
    assert np.array_equal(np.sort(ei), np.arange(g.ne))
    q = O.QpGrid(3, deg, n, lo, up)
    loc = g.local()
    rp, col, ep = loc.pattern()
    orp, ocol = q.pattern(ei)
    assert np.array_equal(rp, orp) and np.array_equal(col, ocol)
    assert np.array_equal(ep, rp[::g.nb])
    # vertex coordinates: vertex k of the Dune cube = lower corner + (k&1, k>>1&1, k>>2) * h
    h = (np.asarray(up) - np.asarray(lo)) / np.asarray(n)
    c = loc.coords
    for k in range(8):
        off = np.array([k & 1, (k >> 1) & 1, k >> 2]) * h
        assert np.allclose(c[3 * k:3 * k + 3].T, c[0:3].T + off, rtol=0, atol=1e-14)
    tw = np.stack([(loc.face_info.astype(np.int64) >> (4 * f)) & 15 for f in range(6)], 1)
    assert np.array_equal(tw, np.tile(np.arange(6) ^ 1, (g.ne, 1)))
    # subdomains are contiguous x-slabs first
    for s in range(g.n_sub):
        a, b = g.subdomain_range(s, s + 1)
        assert (loc.subdomain[a:b] == s).all()


def test_structured3d_rank_local_slab():
    g = H.Grid.structured3d((8, 3, 2), p=(4, 1, 1), degree=1)
    loc = g.local(1, 3)
    a, b = g.subdomain_range(1, 3)
    assert loc.n_own == b - a == 4 * 3 * 2
    assert loc.n_ghost == 2 * 3 * 2
    rp, col, ep = loc.pattern()
    grp, gcol, _ = g.local().pattern()
    assert np.array_equal(col, gcol[grp[a * g.nb]:grp[b * g.nb]])


# ------------------------------------------------------------------------------------------------------
# graded grids
# ------------------------------------------------------------------------------------------------------
def _linspace_nodes(lo, up, n):
    """the oracle's own equidistant breakpoints (linspace_node of swipdg_oracle_qp.c), same arithmetic"""
    x = np.arange(n + 1, dtype=np.float64) * ((up - lo) / float(n)) + lo
    x[n] = up
    return x


def _graded_coefficients(ne, kind):
    """(kappa, tensor) on the graded 3d grid, oracle (lexicographic) element order"""
    if kind == "const":
        return O.scalar(O.FN_CONST, 1.3), O.qp_tensor(c=(1.5, 0.2, -0.1, 2.0, 0.15, 0.8))
    rng = np.random.default_rng(21)
    d, o = rng.uniform(0.5, 3.0, (ne, 3)), rng.uniform(-0.2, 0.2, (ne, 3))
    T = np.ascontiguousarray(np.stack([d[:, 0], o[:, 0], o[:, 1], d[:, 1], o[:, 2], d[:, 2]], 1))
    return O.scalar(O.FN_PER_ELEM, per_elem=rng.uniform(0.2, 4.0, ne)), O.qp_tensor(O.TENSOR_SYM_PER_ELEM, per_elem=T)


@pytest.mark.parametrize("p", [1, 3])
def test_qp_equidistant_nodes_reproduce_structured(p):
    n, lo, up = (3, 2, 4), (-1.0, 0.0, 0.5), (1.0, 1.5, 2.0)
    q0 = O.QpGrid(3, p, n, lo, up)
    q1 = O.QpGrid(3, p, n, lo, up, nodes=[_linspace_nodes(lo[a], up[a], n[a]) for a in range(3)])
    kap = O.scalar(O.FN_SINUSOID, 1.0, 0.5, 3.0, 2.0, order=3)
    rp0, c0, v0 = O.qp_assemble(q0, kap, O.qp_tensor(), O.qp_params(q0))
    rp1, c1, v1 = O.qp_assemble(q1, kap, O.qp_tensor(), O.qp_params(q1))
    assert np.array_equal(rp0, rp1) and np.array_equal(c0, c1)
    assert np.array_equal(v0, v1)
    kw = dict(force=O.esv2007_force(3), kappa=O.scalar(O.FN_CONST, 2.0),
              dirichlet=O.scalar(O.FN_SINUSOID, 1.0, 0.5, 1.3, 0.7, order=3))
    assert np.array_equal(O.qp_rhs_swipdg(q0, **kw), O.qp_rhs_swipdg(q1, **kw))
    for kind in (O.PRODUCT_L2, O.PRODUCT_PENALTY):
        assert np.array_equal(O.qp_product(q0, kind)[2], O.qp_product(q1, kind)[2])


def test_qp_nodes_are_copied_and_checked():
    x = np.array([0.0, 0.25, 1.0])
    q = O.QpGrid(2, 1, (2, 1), (0, 0), (1, 1), nodes=[x, None])
    # the library reads `nodes` only under the flag in dim; an equidistant grid does not carry it
    assert q.t.dim == 2 | O.QP_GRID_GRADED and q.dim == 2
    assert O.QpGrid(2, 1, (2, 1), (0, 0), (1, 1)).t.dim == 2
    ref = O.qp_assemble(q, O.scalar(), O.qp_tensor(dim=2), O.qp_params(q))[2]
    x[1] = 0.9                                         # the grid keeps its own breakpoints
    del x
    assert np.array_equal(O.qp_assemble(q, O.scalar(), O.qp_tensor(dim=2), O.qp_params(q))[2], ref)
    with pytest.raises(ValueError):
        O.QpGrid(2, 1, (2, 1), (0, 0), (1, 1), nodes=[[0.0, 1.0], None])          # n + 1 breakpoints
    with pytest.raises(ValueError):
        O.QpGrid(2, 1, (2, 1), (0, 0), (1, 1), nodes=[[0.0, 0.7, 0.6], None])     # increasing


def test_qp_graded_d2_p1_equals_pinned_2d_oracle():
    xs, ys = GRADED_NODES[0], GRADED_NODES[1]                # 5 x 4, ratios 1.7 and 1:3:1:2
    nx, ny = len(xs) - 1, len(ys) - 1
    _, _, ev = O.cube_grid(nx, ny)
    X, Y = np.meshgrid(xs, ys)
    g2 = O.Grid(O.CUBE, np.stack([X.ravel(), Y.ravel()], 1), ev)
    q = O.QpGrid(2, 1, (nx, ny), (xs[0], ys[0]), (xs[-1], ys[-1]), nodes=[xs, ys])
    kk = np.random.default_rng(3).uniform(0.1, 5, g2.ne)
    for kap, ten2, tenq in [
        (O.scalar(), O.tensor(), O.qp_tensor(dim=2)),
        (O.scalar(O.FN_SINUSOID, 1.0, 0.5, 3, 2, order=3), O.tensor(O.TENSOR_ISO_PER_ELEM, per_elem=kk),
         O.qp_tensor(O.TENSOR_ISO_PER_ELEM, per_elem=kk, dim=2)),
    ]:
        rp, col, val = O.assemble(g2, kap, ten2, O.params())
        rq, cq, vq = O.qp_assemble(q, kap, tenq, O.qp_params(q))
        assert np.array_equal(rp, rq) and np.array_equal(col, cq)
        worst, ok = compare_rows(rp, vq, val, 1e-14)
        assert ok, worst
        # grading is an O(1) effect on the values, not a perturbation the tolerance could hide
        qe = O.QpGrid(2, 1, (nx, ny), (xs[0], ys[0]), (xs[-1], ys[-1]))
        ve = O.qp_assemble(qe, kap, tenq, O.qp_params(qe))[2]
        assert np.max(np.abs(ve - vq)) > 0.1 * np.max(np.abs(vq))


@pytest.mark.parametrize("p", [1, 2, 3])
def test_qp_3d_graded_invariants(p):
    """test_qp_3d_invariants' symmetry and interior row sums on the graded 5 x 4 x 3 grid, and Dirichlet
    consistency: u = 1 solves the homogeneous problem with g_D = 1, so A.1 = b(g_D = 1) row by row.  (Not for
    sinusoid kappa: matrix and right-hand side integrate it with different rules.)"""
    n = [len(x) - 1 for x in GRADED_NODES]
    lo, up = [x[0] for x in GRADED_NODES], [x[-1] for x in GRADED_NODES]
    q = O.QpGrid(3, p, n, lo, up, nodes=GRADED_NODES)
    e_int = 2 + n[0] * (1 + n[1] * 1)                        # element (2,1,1): no boundary face
    rows = slice(e_int * q.nb, (e_int + 1) * q.nb)
    for kind in ("const", "per_elem"):
        kap, ten = _graded_coefficients(q.ne, kind)
        rp, col, val = O.qp_assemble(q, kap, ten, O.qp_params(q))
        A = O.to_scipy(rp, col, val)
        Ad = A.toarray()
        assert np.max(np.abs(Ad - Ad.T)) <= 1e-12 * np.max(np.abs(Ad)), kind
        assert np.max(np.abs(Ad[rows].sum(axis=1))) <= 1e-11 * np.max(np.abs(Ad)), kind
        b = O.qp_rhs_swipdg(q, kappa=kap, A=ten, dirichlet=O.scalar(O.FN_CONST, 1.0))
        assert np.max(np.abs(b)) > 0
        assert np.max(np.abs(A @ np.ones(A.shape[1]) - b)) <= 1e-12 * np.max(np.abs(b)), kind


@pytest.mark.parametrize("deg", [1, 3])
def test_graded_hex_grid_from_connectivity_matches_oracle(deg):
    """Graded hexahedra through hdd_grid_create_hex_from_connectivity with two uneven x-subdomains (x-columns 0-1
    and 2-4): subdomain-major numbering, the oracle's pattern under lex_to_product_graded, and element coordinates
    that are the breakpoints themselves."""
    n = [len(x) - 1 for x in GRADED_NODES]
    coords, ev = graded_hex_mesh(GRADED_NODES)
    sd = (np.arange(ev.shape[0]) % n[0] >= 2).astype(np.int32)
    g = H.Grid.from_connectivity(H.HEX, coords, ev, subdomain=sd, n_sub=2, degree=deg)
    assert g.ne == 60 and g.n_sub == 2 and g.nb == (deg + 1) ** 3
    assert g.subdomain_range(0, 1) == (0, 24) and g.subdomain_range(1, 2) == (24, 60)
    ei = lex_to_product_graded(g, GRADED_NODES)
    assert np.array_equal(np.sort(ei), np.arange(g.ne))
    assert np.array_equal(ei < 24, sd == 0)
    q = O.QpGrid(3, deg, n, coords.min(0), coords.max(0), nodes=GRADED_NODES)
    loc = g.local()
    rp, col, ep = loc.pattern()
    orp, ocol = q.pattern(ei)
    assert np.array_equal(rp, orp) and np.array_equal(col, ocol)
    assert np.array_equal(ep, rp[::g.nb])
    # vertex k of product element ei[e] = breakpoints (i + (k&1), j + (k>>1&1), l + (k>>2)) of oracle element e
    e = np.arange(g.ne)
    ijk = [e % n[0], (e // n[0]) % n[1], e // (n[0] * n[1])]
    for k in range(8):
        for a in range(3):
            assert np.array_equal(loc.coords[3 * k + a][ei], GRADED_NODES[a][ijk[a] + (k >> a & 1)]), (k, a)
    tw = np.stack([(loc.face_info.astype(np.int64) >> (4 * f)) & 15 for f in range(6)], 1)
    assert np.array_equal(tw, np.tile(np.arange(6) ^ 1, (g.ne, 1)))
    # the slab of subdomain 1 sees the 12 smaller elements of x-column 1 as ghosts
    sl = g.local(1, 2)
    assert sl.n_own == 36 and sl.n_ghost == 12
