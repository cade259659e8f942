"""Cases of the right-hand side tests (test_rhs_cases.py on the host, test_gpu_rhs_tiers.py,
test_gpu_rhs_geometry.py and test_gpu_rhs_hex.py on the device): meshes, the restated tier predicate of
rhs2d_kernel<.., HDD_FN_COS_PRODUCT>, element-wise Neumann marking, the oracle references (computed once per
case and shared) and the comparison max|got - ref| <= 1e-12 max|ref| without a floor.

Only host functions of the product (grids, rank-local views) and the oracle are used here; nothing needs a GPU."""
import functools
import os
import re

import numpy as np

import hdd_amd as H
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIG_HEADER = os.path.join(ROOT, "dune-hdd_amd", "csrc", "kernels", "trig_phase.hh")
RTOL = 1e-12
MI355X_CUS = 256            # launch_rhs: min(ceil(n_own / 256), 8 n_cu) workgroups of 256 threads
OGRID = {H.SIMPLEX: O.kuhn_grid, H.CUBE: O.cube_grid}
ET_NAME = {H.SIMPLEX: "P1", H.CUBE: "Q1"}


# ------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------
def ratio(got, ref):
    """max|got - ref| / max|ref| (no floor: force entries are O(|K|), far below 1)"""
    scale = np.max(np.abs(ref))
    assert scale > 0
    return np.max(np.abs(np.asarray(got) - ref)) / scale


def check(label, got, ref, worst=None):
    """print the measured ratio, then assert it against the project's 1e-12; worst: dict collecting the largest
    ratio per group (label up to the first ':')"""
    r = ratio(got, ref)
    print("rhs %s: max|db| / max|b| %.3g" % (label, r))
    if worst is not None:
        key = label.split(":")[0]
        worst[key] = max(worst.get(key, 0.0), r)
    assert r <= RTOL, (label, r)
    return r


# ------------------------------------------------------------------------------------------------------
# the tier predicate, restated
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def phase_thresholds():
    """(SMALL_PHASE, TINY_PHASE) as trig_phase.hh defines them"""
    txt = open(TRIG_HEADER).read()
    out = []
    for name in ("SMALL_PHASE", "TINY_PHASE"):
        m = re.findall(r"constexpr\s+double\s+%s\s*=\s*([0-9.eE+-]+)\s*;" % name, txt)
        assert len(m) == 1, name
        out.append(float(m[0]))
    assert 0.0 < out[1] < out[0]
    return tuple(out)


def element_dm(coords, kx, ky):
    """rhs2d_kernel's dm per element from element-major coordinates [2 nvpe][n] (rows x0 y0 x1 y1 x2 y2 ..):
    max(|kx j00| + |kx j01|, |ky j10| + |ky j11|), columns of J = vertex 1 - vertex 0, vertex 2 - vertex 0"""
    return jacobian_dm(kx, ky, *element_jacobian(coords))


def element_jacobian(coords):
    """(j00, j10, j01, j11) exactly as the kernel forms them"""
    x0, y0, x1, y1, x2, y2 = coords[:6]
    j00 = x1 - x0; j10 = y1 - y0
    j01 = x2 - x0; j11 = y2 - y0
    return j00, j10, j01, j11


def jacobian_dm(kx, ky, j00, j10, j01, j11):
    return np.fmax(np.abs(kx * j00) + np.abs(kx * j01), np.abs(ky * j10) + np.abs(ky * j11))


TINY, NEAR, FAR = 0, 1, 2


def wave_tiers(dm, small=None, tiny=None):
    """Per 64-lane wave of the launch (thread k = owned element k, wave w = elements 64 w .. 64 w + 63; the last
    wave's missing lanes are inactive and do not vote): (tier, pushed).  tier: the evaluation the wave takes,
    __all(dm <= TINY_PHASE) -> TINY, else __all(dm <= SMALL_PHASE) -> NEAR, else FAR.  pushed: a full wave in
    which exactly one element lies above a threshold that the other 63 meet."""
    s, t = phase_thresholds()
    small = s if small is None else small
    tiny = t if tiny is None else tiny
    tiers, pushed = [], []
    for k0 in range(0, dm.shape[0], 64):
        d = dm[k0:k0 + 64]
        above_t, above_s = int((d > tiny).sum()), int((d > small).sum())
        tiers.append(TINY if above_t == 0 else (NEAR if above_s == 0 else FAR))
        pushed.append(d.shape[0] == 64 and (above_s == 1 or (above_t == 1 and above_s == 0)))
    return np.array(tiers), np.array(pushed)


# ------------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------------
SHEAR = np.array([[1.3, 0.45], [-0.2, 0.9]])
SHIFT = np.array([0.3, -0.1])


def sheared_mesh(et, nx=37, ny=11, mirror=False):
    """the affine image of the unit square's structured grid (test_products_pwc_fast_path's map); mirror:
    x -> -x with the vertex order kept, so every element's det J changes sign (the two triangles of a Kuhn
    square already differ in sign; mirrored quadrilaterals all have det J < 0)"""
    et_, coords, ev = OGRID[et](nx, ny, (0, 0), (1, 1))
    coords = coords @ SHEAR.T + SHIFT
    if mirror:
        coords = coords * np.array([-1.0, 1.0])
    return et_, np.ascontiguousarray(coords), ev


def geometry_mesh(name):
    from mesh_tools import nvb_mesh
    if name == "kuhn_sheared":
        return sheared_mesh(H.SIMPLEX)
    if name == "cube_sheared":
        return sheared_mesh(H.CUBE)
    if name == "kuhn_mirrored":
        return sheared_mesh(H.SIMPLEX, mirror=True)
    if name == "cube_mirrored":
        return sheared_mesh(H.CUBE, mirror=True)
    assert name == "nvb"
    return nvb_mesh(4, 3)


GEOMETRY_MESHES = ("kuhn_sheared", "cube_sheared", "nvb", "kuhn_mirrored", "cube_mirrored")


def element_major(coords, ev):
    """[2 nvpe][ne] coordinates as LocalMesh.coords holds them"""
    return np.ascontiguousarray(coords[ev].reshape(ev.shape[0], -1).T)


def signed_dets(coords, ev):
    c = element_major(coords, ev)
    return (c[2] - c[0]) * (c[5] - c[1]) - (c[4] - c[0]) * (c[3] - c[1])


# ------------------------------------------------------------------------------------------------------
# element-wise boundary marking (the oracle's boundary kind is global)
# ------------------------------------------------------------------------------------------------------
def mark_elements(neighbors, seed):
    """A seeded subset of the boundary elements, as a mask over all elements [n]: about half of them, among them
    one element with two (or more) boundary faces -- where the mesh has one: the bisection mesh nvb_mesh(4, 3)
    has none (has_corner tells).  neighbors: [nf][n], boundary faces negative."""
    nbnd = (neighbors < 0).sum(axis=0)
    bnd = np.nonzero(nbnd > 0)[0]
    corner = np.nonzero(nbnd > 1)[0]
    assert bnd.size >= 2
    rng = np.random.default_rng(seed)
    marked = np.zeros(neighbors.shape[1], bool)
    marked[bnd[rng.random(bnd.size) < 0.5]] = True
    if corner.size:
        marked[corner[rng.integers(corner.size)]] = True
    rest = bnd[~marked[bnd]]
    assert rest.size > 0 and marked.any()                  # both groups are there
    return marked


def has_corner(neighbors):
    return bool(np.any((neighbors < 0).sum(axis=0) > 1))


def set_boundary(loc, marked, code):
    """every boundary face of the marked elements of a LocalMesh becomes `code` (before DeviceMesh is built)"""
    for f in range(loc.nf):
        sel = marked & (loc.neighbors[f] < 0)
        loc.neighbors[f][sel] = code


def compose(nb, b_force, b_dir, b_neu, marked):
    """b_force + (marked element ? b_neu : b_dir), rows of element e = [nb e, nb e + nb)"""
    rows = np.repeat(marked, nb)
    return b_force + np.where(rows, b_neu, b_dir)


# ------------------------------------------------------------------------------------------------------
# cos-tier cases
# ------------------------------------------------------------------------------------------------------
TIERS = ("tiny", "near", "far", "mixed", "tiny_sheared", "near_sheared")
MX, MY = 70, 72          # the phases kx x and ky y at the mesh's centre, in units of pi / 2
FORCE_C = 2.5


class TierCase:
    """et, coords [nv][2], ev [ne][nvpe] (element order = launch order), kx, ky of the force, dm per element"""

    def __init__(self, tier, et, coords, ev, kx, ky):
        self.tier, self.et, self.coords, self.ev, self.kx, self.ky = tier, et, coords, ev, kx, ky
        self.dm = element_dm(element_major(coords, ev), kx, ky)
        self.nb = 3 if et == H.SIMPLEX else 4

    def grid(self):
        return H.Grid.from_connectivity(self.et, self.coords, self.ev)

    def ogrid(self):
        return O.Grid(self.et, self.coords, self.ev)

    def force(self, mod):
        """the COS_PRODUCT force, order 3 (6-point / 9-point unrolled templates), for mod = H or O"""
        if mod is H:
            return H.scalar_fn(H.FN_COS_PRODUCT, FORCE_C, kx=self.kx, ky=self.ky, order=3)
        return O.scalar(O.FN_COS_PRODUCT, FORCE_C, 0.0, self.kx, self.ky, order=3)

    def phases(self):
        return self.kx * self.coords[:, 0], self.ky * self.coords[:, 1]

    def data_wave_numbers(self):
        """wave numbers of g_D and g_N: phases of some tens at the mesh (the domains lie far from the origin)"""
        xc, yc = 0.5 * (self.coords.min(axis=0) + self.coords.max(axis=0))
        return 37.0 / xc, 23.0 / yc, 11.0 / xc, 7.0 / yc


def _centre(coords, kx, ky):
    """shift the mesh so that its bounding box's centre has the phases MX pi/2, MY pi/2"""
    mid = 0.5 * (coords.min(axis=0) + coords.max(axis=0))
    return np.ascontiguousarray(coords - mid + np.array([MX * 0.5 * np.pi / kx, MY * 0.5 * np.pi / ky]))


def _uniform_case(tier, et, nx, ny, box, M=None):
    small, tiny = phase_thresholds()
    _, coords, ev = OGRID[et](nx, ny, (0.0, 0.0), box)
    if M is not None:
        coords = coords @ M.T
    kind = tier.split("_")[0]
    em = element_major(coords, ev)
    # ky / kx: the y term of dm reaches 0.8 of the x term, so both directions count and kx != ky
    ratio_k = 0.8 * element_dm(em, 1.0, 0.0).max() / element_dm(em, 0.0, 1.0).max()
    d1 = element_dm(em, 1.0, ratio_k)                         # dm is homogeneous of degree 1 in (kx, ky)
    if kind == "far":
        kx = 1.2 * small / d1.min()                           # every element above SMALL_PHASE
    else:
        kx = 0.9 * (tiny if kind == "tiny" else small) / d1.max()
    ky = ratio_k * kx
    return TierCase(tier, et, _centre(coords, kx, ky), ev, kx, ky)


def _mixed_case(et):
    """Rectilinear, graded breakpoints (as test_graded_rectilinear_q1_full_tiles builds them).  Rows are 65
    quadrilaterals / 66 triangles long, so the 64-element waves drift against the rows: wave 0 misses the wide
    last column, wave 1 holds exactly one element of it.  Rows 0-3 are tiny, 4-7 near, 8-11 far."""
    small, tiny = phase_thresholds()
    tri = et == H.SIMPLEX
    u = 2.0 if tri else 1.0                     # a Kuhn triangle's dm counts one of the two widths twice
    nx, ny = (33 if tri else 65), 12
    kx, ky = 7.0, 4.0
    px = 0.5 * tiny / u * np.array([1.0, 0.8, 0.9, 0.7])[np.arange(nx) % 4]          # kx hx per column
    px[-1] = 0.8 * tiny if tri else 3.0 * tiny  # the wide column: its (first) element alone leaves the tiny tier
    py = np.concatenate([np.array([0.4, 0.8, 0.5, 0.7]) * tiny / u, np.array([0.3, 0.8, 0.45, 0.6]) * small / u,
                         np.array([1.5, 3.0, 2.0, 2.5]) * small])                    # ky hy per row
    xs = np.concatenate([[0.0], np.cumsum(px)]) / kx
    ys = np.concatenate([[0.0], np.cumsum(py)]) / ky
    _, _, ev = OGRID[et](nx, ny)
    X, Y = np.meshgrid(xs, ys)
    coords = np.stack([X.ravel(), Y.ravel()], axis=1).copy()
    return TierCase("mixed", et, _centre(coords, kx, ky), ev, kx, ky)


@functools.lru_cache(None)
def tier_case(tier, et):
    if tier == "mixed":
        return _mixed_case(et)
    if tier.endswith("_sheared"):
        return _uniform_case(tier, et, 37, 11, (1.0, 1.0), SHEAR)
    return _uniform_case(tier, et, 61, 23, (2.0, 1.0))


def tier_data(case):
    """per-element kappa and iso tensor of the boundary run, in element order"""
    rng = np.random.default_rng(29)
    ne = case.ev.shape[0]
    return rng.uniform(0.5, 2.0, ne), rng.uniform(0.5, 2.0, ne)


@functools.lru_cache(None)
def tier_refs(tier, et):
    """oracle references of a tier case, computed once: (b_force, b_force + b_boundary, marked) with the
    element-wise marking composed from all-Dirichlet and all-Neumann oracle calls without the force"""
    case = tier_case(tier, et)
    og = case.ogrid()
    kel, tel = tier_data(case)
    dkx, dky, nkx, nky = case.data_wave_numbers()
    b_f = O.rhs_swipdg(og, force=case.force(O))
    b_d = O.rhs_swipdg(og, kappa=O.scalar(O.FN_PER_ELEM, per_elem=kel), A=O.tensor(O.TENSOR_ISO_PER_ELEM, per_elem=tel),
                       dirichlet=O.scalar(O.FN_SINUSOID, 1.0, 0.5, dkx, dky, order=3))
    b_n = O.rhs_swipdg(og, neumann=O.scalar(O.FN_COS_PRODUCT, 2.0, 0.0, nkx, nky, order=2),
                       prm=O.params(boundary=O.BOUNDARY_NEUMANN))
    nbr, _ = og.neighbors()
    marked = mark_elements(nbr.T, 31)
    for r in (b_f, b_d, b_n):
        r.setflags(write=False)
    return b_f, compose(case.nb, b_f, b_d, b_n, marked), marked


# ------------------------------------------------------------------------------------------------------
# rank-local range
# ------------------------------------------------------------------------------------------------------
BLOCK_N, BLOCK_BOX, BLOCK_P, BLOCK_S = (37, 11), ((0.3, -0.1), (2.3, 0.9)), (3, 2), 1


def block_grid(et):
    """37 x 11 in 3 x 2 subdomains (ragged: 13 + 12 + 12 columns, 6 + 5 rows)"""
    return H.Grid.structured(et, *BLOCK_N, *BLOCK_BOX, px=BLOCK_P[0], py=BLOCK_P[1])


def oracle_elem_index(grid, et):
    """(oracle grid on the lexicographic structured mesh, elem_index: oracle element -> product global id), as
    test_gpu_surface.py maps the multiscale grid"""
    pc, pev, _ = grid.connectivity()
    ot, oc, oev = OGRID[et](*BLOCK_N, *BLOCK_BOX)
    assert np.array_equal(pc, oc)
    key = {tuple(r): i for i, r in enumerate(pev)}
    ei = np.array([key[tuple(r)] for r in oev], np.int64)
    assert np.array_equal(np.sort(ei), np.arange(grid.ne))
    return O.Grid(ot, oc, oev), ei
