"""Cases of the product tests (test_product_cases.py on the host, test_gpu_products_grid.py on the device): the
meshes on which the two kernel families of hdd_product_assemble can go wrong (scrambled numbering and orientation,
reversed faces, rank-local views with ghosts, single elements and strips, more tiles than one pass of the persistent
grid), per-element coefficients drawn once in global element order, the oracle references (computed once per case and
shared, read-only), the comparisons (rows, penalty column blocks, exact zeros of boundary_l2) and the invariants that
need no oracle.

Only host functions of the product (grids, rank-local views, host patterns) and the oracle are used here; nothing
needs a GPU."""
import functools
import math

import numpy as np

import hdd_amd as H
import oracle as O
from cases import compare_rows, compare_rows_fast

RTOL = 1e-12
KINDS = (H.PRODUCT_L2, H.PRODUCT_H1_SEMI, H.PRODUCT_ELLIPTIC, H.PRODUCT_BOUNDARY_L2, H.PRODUCT_PENALTY)
KIND_NAME = {H.PRODUCT_L2: "l2", H.PRODUCT_H1_SEMI: "h1_semi", H.PRODUCT_ELLIPTIC: "elliptic",
             H.PRODUCT_BOUNDARY_L2: "boundary_l2", H.PRODUCT_PENALTY: "penalty"}
COEFF_KINDS = (H.PRODUCT_ELLIPTIC, H.PRODUCT_PENALTY)            # the kinds that read kappa and the tensor
ETS = (H.SIMPLEX, H.CUBE)
ET_NAME = {H.SIMPLEX: "P1", H.CUBE: "Q1"}
OGRID = {H.SIMPLEX: O.kuhn_grid, H.CUBE: O.cube_grid}
TENSOR_KINDS = ("const", "iso", "sym")
KAPPA_KINDS = ("const", "per_elem")                              # piecewise constant: both families
SMOOTH = "sinusoid"                                              # the generic kernel only
TENSOR_CONST = (1.7, 0.3, 0.6)                                   # SPD, off-diagonal nonzero
KAPPA_CONST = 2.5
SINUSOID = dict(c=1.0, b=0.5, kx=3.0, ky=2.0, order=3)
BETAS = (1.0, 0.5)
SHEAR = np.array([[1.3, 0.45], [-0.2, 0.9]])
SHIFT = np.array([0.3, -0.1])
AFFINE_U = (0.3, 1.7, -0.9)                                      # u = 0.3 + 1.7 x - 0.9 y
MI355X_CUS = 256
FACES = {H.SIMPLEX: ((0, 1), (0, 2), (1, 2)), H.CUBE: ((0, 2), (1, 3), (0, 1), (2, 3))}     # Dune face -> vertices


# ------------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------------
SCRAMBLED_N = {H.SIMPLEX: (14, 11), H.CUBE: (20, 15)}
SLAB_NX = {H.SIMPLEX: 24, H.CUBE: 48}
MULTIPASS_N = {H.SIMPLEX: (190, 180), H.CUBE: (264, 260)}
EDGE_SHAPES = ((1, 1), (1, 9), (9, 1))
MESHES = ("scrambled", "nvb", "slab", "split", "multipass", "single") + tuple("edge_%dx%d" % s for s in EDGE_SHAPES)


def scrambled_connectivity(et, seed=11):
    """test_scrambled_numbering_full_tiles' mesh at the smallest size that keeps full interior tiles: interior
    elements first (shuffled), then the boundary elements (shuffled), a random symmetry of the reference element per
    element (Dune vertex order kept valid), then the affine map x -> SHEAR x + SHIFT"""
    simplex = et == H.SIMPLEX
    et_, coords, ev = OGRID[et](*SCRAMBLED_N[et], (0, 0), (3, 2))
    rng = np.random.default_rng(seed)
    sides = [list(s) for s in FACES[et]]
    edges = np.sort(np.stack([ev[:, e] for e in sides], 1), axis=2).reshape(-1, 2)
    _, inv, cnt = np.unique(edges, axis=0, return_inverse=True, return_counts=True)
    bnd = (cnt[inv.reshape(-1)].reshape(-1, len(sides)) == 1).any(axis=1)
    order = np.concatenate([rng.permutation(np.flatnonzero(~bnd)), rng.permutation(np.flatnonzero(bnd))])
    perms = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]] if simplex else
                     [[0, 1, 2, 3], [1, 3, 0, 2], [3, 2, 1, 0], [2, 0, 3, 1],     # the square's rotations
                      [1, 0, 3, 2], [2, 3, 0, 1], [0, 2, 1, 3], [3, 1, 2, 0]])    # and reflections
    pick = perms[rng.integers(0, len(perms), len(order))]
    ev = np.ascontiguousarray(np.take_along_axis(ev[order], pick, 1)).astype(np.int32)
    return et_, np.ascontiguousarray(coords @ SHEAR.T + SHIFT), ev


class Case:
    """A mesh with its boundary kind and (for slab / split) the rank-local view the products run on.  pc, pev: the
    product's own vertices and element order (grid.connectivity()), on which the oracle grid og is built, so oracle
    element k is the product's global element k."""

    def __init__(self, name, et, neumann, grid, view=None):
        self.name, self.et, self.neumann, self.grid, self.view = name, et, neumann, grid, view
        self.nb = grid.nb
        self.pc, self.pev, _ = grid.connectivity()
        self.og = O.Grid(O.SIMPLEX if et == H.SIMPLEX else O.CUBE, self.pc, self.pev)
        self.rows = grid.subdomain_range(*view) if view else (0, grid.ne)

    def local(self):
        return self.grid.local(*self.view) if self.view else self.grid.local()

    def label(self):
        return "%s %s %s" % (self.name, ET_NAME[self.et], "neumann" if self.neumann else "dirichlet")

    def oracle_params(self, beta=1.0):
        return O.params(O.BOUNDARY_NEUMANN if self.neumann else O.BOUNDARY_DIRICHLET, beta=beta)

    def tiles(self):
        a, b = self.rows
        return (b - a + 63) // 64


@functools.lru_cache(None)
def case(name, et, neumann=False):
    bnd = H.BOUNDARY_ALL_NEUMANN if neumann else H.BOUNDARY_ALL_DIRICHLET
    if name == "scrambled":
        _, coords, ev = scrambled_connectivity(et)
        return Case(name, et, neumann, H.Grid.from_connectivity(et, coords, ev, boundary=bnd))
    if name == "nvb":
        from mesh_tools import nvb_mesh
        assert et == H.SIMPLEX
        _, coords, ev = nvb_mesh(4, 3)
        return Case(name, et, neumann, H.Grid.from_connectivity(et, coords, ev, boundary=bnd))
    if name == "slab":
        g = H.Grid.structured(et, SLAB_NX[et], 9, (0, 0), (3, 1), px=3, py=1, boundary=bnd)
        return Case(name, et, neumann, g, view=(1, 2))
    if name == "split":
        g = H.Grid.structured(et, 12, 10, (0, 0), (3, 1), px=3, py=2, boundary=bnd)
        return Case(name, et, neumann, g, view=(2, 4))
    if name == "multipass":
        return Case(name, et, neumann, H.Grid.structured(et, *MULTIPASS_N[et], (0.3, -0.1), (2.3, 0.9), boundary=bnd))
    if name == "single":      # one element (a Kuhn 1 x 1 grid has two): no interior face at all
        xy = np.array([[0.3, -0.1], [1.1, 0.2], [0.5, 0.6], [1.3, 0.9]])
        ev = np.array([[0, 1, 2]] if et == H.SIMPLEX else [[0, 1, 2, 3]], np.int32)
        return Case(name, et, neumann, H.Grid.from_connectivity(et, xy[:ev.shape[1]], ev, boundary=bnd))
    assert name.startswith("edge_")
    nx, ny = (int(s) for s in name[5:].split("x"))
    # (no face of length 1: |F|^beta must depend on beta)
    return Case(name, et, neumann, H.Grid.structured(et, nx, ny, (0.3, -0.1), (1.1, 0.4), boundary=bnd))


def mesh_ets(name):
    return (H.SIMPLEX,) if name == "nvb" else ETS


def element_major(coords, ev):
    """[2 nvpe][ne] coordinates as LocalMesh.coords holds them"""
    return np.ascontiguousarray(coords[ev].reshape(ev.shape[0], -1).T)


def signed_dets(coords, ev):
    """det of the map spanned by vertices 0, 1, 2 (what VolProductPolicy and p1_compute form)"""
    c = element_major(coords, ev)
    return (c[2] - c[0]) * (c[5] - c[1]) - (c[4] - c[0]) * (c[3] - c[1])


def full_interior_tiles(loc):
    """(full-interior tiles, full tiles, ragged remainder) of the owned range in 64-element tiles"""
    nb = loc.neighbors[:, loc.own_begin:loc.own_end]
    nfull = loc.n_own // 64
    full = (nb >= 0).all(axis=0)[: nfull * 64].reshape(-1, 64).all(axis=1)
    return int(full.sum()), nfull, loc.n_own - 64 * nfull


def reversed_faces(loc):
    """(owned elements with a reversed face, reversed face slots): bit 3 of a face's nibble in face_info says that the
    twin face runs the other way"""
    fi = loc.face_info[loc.own_begin:loc.own_end].astype(np.uint32)
    bits = np.stack([(fi >> np.uint32(4 * f + 3)) & np.uint32(1) for f in range(loc.nf)])
    return int(bits.any(axis=0).sum()), int(bits.sum())


# ------------------------------------------------------------------------------------------------------
# coefficients, in global element order
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def coeff_data(name, et):
    """dict of per-element arrays in global element order: sym [3][ne] (a11, a12, a22 as test_products_pwc_fast_path
    draws them), iso [ne] = 10**U(-2, 2), kap [ne] = U(0.1, 10)"""
    ne = case(name, et).grid.ne
    rng = np.random.default_rng(23)
    a = rng.uniform(0.5, 2.0, ne); c = rng.uniform(0.5, 2.0, ne); b = rng.uniform(-0.3, 0.3, ne)
    d = dict(sym=np.stack([a, b, c], 0), iso=10.0 ** rng.uniform(-2.0, 2.0, ne), kap=rng.uniform(0.1, 10.0, ne))
    for v in d.values():
        v.setflags(write=False)
    return d


def oracle_coeffs(name, et, tk, kk):
    d = coeff_data(name, et)
    if tk == "const":
        A = O.tensor(O.TENSOR_CONST, c=TENSOR_CONST)
    elif tk == "iso":
        A = O.tensor(O.TENSOR_ISO_PER_ELEM, per_elem=np.ascontiguousarray(d["iso"]))
    else:
        A = O.tensor(O.TENSOR_SYM_PER_ELEM, per_elem=np.ascontiguousarray(d["sym"].T))
    if kk == "const":
        k = O.scalar(O.FN_CONST, KAPPA_CONST)
    elif kk == "per_elem":
        k = O.scalar(O.FN_PER_ELEM, per_elem=np.ascontiguousarray(d["kap"]))
    else:
        s = SINUSOID
        k = O.scalar(O.FN_SINUSOID, s["c"], s["b"], s["kx"], s["ky"], order=s["order"])
    return k, A


def view_coeffs(name, et, tk, kk, global_id):
    """what the product is given on a view: (tensor kind, tensor array or None, kappa array or None), indexed by the
    view's global ids (ghosts included); the device test wraps them"""
    d = coeff_data(name, et)
    t = None if tk == "const" else np.ascontiguousarray(d[tk][..., global_id])
    k = np.ascontiguousarray(d["kap"][global_id]) if kk == "per_elem" else None
    return t, k


# ------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------
def _key(kind, neumann, tk, kk, beta):
    """what a kind does not read is normalised away, so the reference is computed once"""
    if kind not in COEFF_KINDS:
        tk, kk = "const", "const"
    if kind != H.PRODUCT_PENALTY:
        beta = 1.0
    if kind not in (H.PRODUCT_BOUNDARY_L2, H.PRODUCT_PENALTY):
        neumann = False
    return neumann, tk, kk, beta


@functools.lru_cache(None)
def _reference(name, et, kind, neumann, tk, kk, beta):
    c = case(name, et, neumann)
    kap, A = oracle_coeffs(name, et, tk, kk)
    rp, col, val = O.product(c.og, kind, kappa=kap, A=A, prm=c.oracle_params(beta))
    a, b = c.rows
    lo, hi = rp[a * c.nb], rp[b * c.nb]
    out = (np.ascontiguousarray(rp[a * c.nb:b * c.nb + 1] - lo), np.ascontiguousarray(col[lo:hi]),
           np.ascontiguousarray(val[lo:hi]))
    for r in out:
        r.setflags(write=False)
    return out


def reference(name, et, kind, neumann=False, tk="sym", kk="per_elem", beta=1.0):
    """(row_ptr, col, val) of the oracle's product on the case's owned rows (the row slice grid.subdomain_range gives;
    global columns), computed once per distinct input"""
    return _reference(name, et, kind, *_key(kind, neumann, tk, kk, beta))


# ------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------
def _note(worst, group, r):
    if worst is not None:
        worst[group] = max(worst.get(group, 0.0), r)


def penalty_zero_rows(c):
    """Rows of the penalty that are zero in exact arithmetic, from the mesh alone: the DoF's vertex lies only on Neumann
    faces, which carry no penalty (a corner element's vertex opposite its one interior face under all-Neumann).  The
    oracle holds there the rounding of a basis function that vanishes on the penalised faces (1e-14 absolute on
    triangles and sheared quadrilaterals), so the row has no scale of its own.  bool [nb * owned elements]."""
    loc = c.local()
    nbr = loc.neighbors[:, loc.own_begin:loc.own_end]
    zero = np.ones((loc.n_own, c.nb), bool)
    for f, vs in enumerate(FACES[c.et]):
        for i in vs:
            zero[:, i] &= nbr[f] == H.NBR_NEUMANN
    return zero.reshape(-1)


def row_ratio(rp, got, ref, nb, zero_rows=None):
    """compare_rows' ratio, max over rows of max|got - ref| / max|ref| of the row (rows are non-empty).  zero_rows:
    rows that vanish in exact arithmetic (penalty_zero_rows): the reference must say so, |ref| <= 1e-12 of the
    element's nb rows, and they are scaled by the largest reference entry of those nb rows instead of by their own
    rounding noise.  No other row is touched and none is left out."""
    got, ref = np.asarray(got), np.asarray(ref)
    starts = np.asarray(rp[:-1], np.int64)
    err = np.maximum.reduceat(np.abs(got - ref), starts)
    scale = np.maximum.reduceat(np.abs(ref), starts)
    if zero_rows is not None and zero_rows.any():
        elem = np.repeat(scale.reshape(-1, nb).max(axis=1), nb)
        assert np.all(scale[zero_rows] <= RTOL * elem[zero_rows])
        scale = np.where(zero_rows, elem, scale)
    scale = np.where(scale == 0, 1.0, scale)
    return float(np.max(err / scale)) if starts.size else 0.0


def check_rows(label, rp, got, ref, worst=None, group="rows", fast=False, nb=None, zero_rows=None):
    """max over rows of max|got - ref| / max|ref| of the row, printed, then held to 1e-12: no floor, every row
    (cases.compare_rows / compare_rows_fast; with zero_rows, row_ratio, which equals them on all other rows)"""
    got = np.asarray(got)
    assert got.shape == ref.shape and not np.isnan(got).any(), label      # every entry was written
    if zero_rows is not None and zero_rows.any():
        r = row_ratio(rp, got, ref, nb, zero_rows)
        ok = r <= RTOL
    else:
        r, ok = (compare_rows_fast if fast else compare_rows)(rp, got, ref, RTOL)
    print("product %s [%s]: worst row ratio %.3g" % (label, group, r))
    _note(worst, group, r)
    assert ok, (label, r)
    return r


def block_ratio(rp, got, ref, nb):
    """max over (element row block, column block) of max|got - ref| / max|ref| of the nb x nb block.  The nb rows of an
    element's block are taken together: a neighbour block's row of the test function at the vertex opposite the face
    is zero in exact arithmetic and holds the oracle's rounding of a basis function that vanishes on the face (1e-15
    absolute), which is noise at the block's scale and has no scale of its own."""
    got, ref = np.asarray(got), np.asarray(ref)
    ep = np.asarray(rp[::nb], np.int64)                                 # first value of each element's row block
    nblk = np.diff(ep) // (nb * nb)
    assert np.array_equal(nblk * nb * nb, np.diff(ep))
    worst = 0.0
    for m in np.unique(nblk):
        idx = (ep[:-1][nblk == m][:, None] + np.arange(nb * nb * m)[None, :]).reshape(-1, nb, m, nb)
        e = np.max(np.abs(got[idx] - ref[idx]), axis=(1, 3))
        s = np.max(np.abs(ref[idx]), axis=(1, 3))
        s = np.where(s == 0, 1.0, s)
        worst = max(worst, float(np.max(e / s)))
    return worst


def check_blocks(label, rp, got, ref, nb, worst=None, group="blocks"):
    """the penalty per (element row block, column block), each scaled by its own largest reference entry: a weak
    face's block next to a strong one (iso tensors span 1e4) is held to 1e-12 of itself.  Every contribution to a block
    has one sign, so rounding does not need the row's scale."""
    r = block_ratio(rp, got, ref, nb)
    print("product %s [%s]: worst block ratio %.3g" % (label, group, r))
    _note(worst, group, r)
    assert r <= RTOL, (label, r)
    return r


def check_exact_zeros(label, got, ref):
    """boundary_l2: both kernels start from zero and add nothing where the reference is exactly zero"""
    z = ref == 0.0
    bad = int(np.count_nonzero(np.asarray(got)[z]))
    print("product %s: %d exact zeros of the reference, %d of them nonzero" % (label, int(z.sum()), bad))
    assert bad == 0, (label, bad)


def check_product(label, kind, rp, got, ref, nb, worst=None, prefix="", fast=False, zero_rows=None):
    """the comparisons of one product against its reference; zero_rows (penalty only): penalty_zero_rows of the case"""
    check_rows(label, rp, got, ref, worst, prefix + "rows", fast, nb, zero_rows if kind == H.PRODUCT_PENALTY else None)
    if kind == H.PRODUCT_PENALTY:
        check_blocks(label, rp, got, ref, nb, worst, prefix + "blocks")
    if kind == H.PRODUCT_BOUNDARY_L2:
        check_exact_zeros(label, got, ref)


# ------------------------------------------------------------------------------------------------------
# invariants without the oracle
# ------------------------------------------------------------------------------------------------------
def owned_measures(c):
    """(|Omega|, |dOmega|) of the case's owned elements from the vertices alone: shoelace areas, and the lengths of the
    faces that belong to one element only (Dirichlet or Neumann alike)"""
    a, b = c.rows
    faces = FACES[c.et]
    edges = np.sort(np.stack([c.pev[:, list(f)] for f in faces], 1), axis=2)            # [ne][nf][2]
    _, inv, cnt = np.unique(edges.reshape(-1, 2), axis=0, return_inverse=True, return_counts=True)
    on_bnd = (cnt[inv.reshape(-1)] == 1).reshape(-1, len(faces))
    d = c.pc[edges[..., 1]] - c.pc[edges[..., 0]]
    length = np.hypot(d[..., 0], d[..., 1])
    ring = [0, 1, 2] if c.et == H.SIMPLEX else [0, 1, 3, 2]
    p = c.pc[c.pev[:, ring]]
    q = np.roll(p, -1, axis=1)
    area = 0.5 * np.abs(np.sum(p[..., 0] * q[..., 1] - q[..., 0] * p[..., 1], axis=1))
    return math.fsum(area[a:b]), math.fsum(length[a:b][on_bnd[a:b]])


def affine_u(c):
    """u = 0.3 + 1.7 x - 0.9 y at the element vertices, all global DoFs (DoF i of an element sits at its vertex i)"""
    xy = c.pc[c.pev]
    return (AFFINE_U[0] + AFFINE_U[1] * xy[..., 0] + AFFINE_U[2] * xy[..., 1]).reshape(-1)


def _matrix(c, rp, col, val):
    return O.to_scipy(rp, col, np.asarray(val), n=c.grid.ne * c.nb)


def invariant_ratios(c, kind, rp, col, val):
    """dict name -> relative defect of the invariants of one product on the case's owned rows against all global
    columns.  Row-wise invariants (M 1 = 0, symmetry, P u = 0) are relative to max|M| (times max|u|).  The two totals
    (1^T M 1 = |Omega|, 1^T B 1 = |dOmega|) sum nnz entries of one sign, so their rounding scales with sum|M|, the
    total itself, not with one entry: on congruent elements every entry rounds alike and the errors add up linearly
    (the oracle alone leaves 2.2e-12 max|M| on the 300 scrambled parallelograms, which is 8e-16 of the total).  They
    are relative to sum|M|, summed exactly (fsum).  The penalty's affine defect is "affine_neumann" on an all-Neumann
    mesh (must vanish: a continuous function has no jumps) and "affine_dirichlet" otherwise (must not)."""
    val = np.asarray(val)
    M = _matrix(c, rp, col, val)
    a, b = c.rows
    scale = float(np.max(np.abs(val)))
    assert scale > 0 or (kind == H.PRODUCT_PENALTY and c.neumann)
    scale = scale if scale > 0 else 1.0
    own = M[:, a * c.nb:b * c.nb]                                   # owned rows x owned columns
    asym = abs(own - own.T)
    out = {}
    area, length = owned_measures(c)
    if kind == H.PRODUCT_L2:
        out["mass"] = abs(math.fsum(val) - area) / math.fsum(np.abs(val))
    elif kind in (H.PRODUCT_H1_SEMI, H.PRODUCT_ELLIPTIC):
        out["constants"] = float(np.max(np.abs(M @ np.ones(M.shape[1])))) / scale
        out["symmetry"] = (float(asym.max()) if asym.nnz else 0.0) / scale
    elif kind == H.PRODUCT_BOUNDARY_L2:
        out["boundary_length"] = abs(math.fsum(val) - length) / math.fsum(np.abs(val))
    else:
        out["symmetry"] = (float(asym.max()) if asym.nnz else 0.0) / scale
        u = affine_u(c)
        r = float(np.max(np.abs(M @ u))) / (scale * float(np.max(np.abs(u))))
        out["affine_neumann" if c.neumann else "affine_dirichlet"] = r
    return out


AFFINE_DIRICHLET_MIN = 1e-3     # the boundary penalty of u = O(1) on a Dirichlet face is O(max|P| max|u|), not rounding


def check_invariants(label, c, kind, rp, col, val, worst=None, group="invariants"):
    for name, r in invariant_ratios(c, kind, rp, col, val).items():
        print("product %s [%s]: %s %.3g" % (label, group, name, r))
        if name == "affine_dirichlet":
            assert r > AFFINE_DIRICHLET_MIN, (label, name, r)
            continue
        _note(worst, group, r)
        assert r <= RTOL, (label, name, r)
