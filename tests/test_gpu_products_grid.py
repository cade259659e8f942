"""GPU products (hdd_product_assemble) of both kernel families against the oracle on the cases of product_cases.py.

tile     the closed forms on the persistent tile driver (VolProductPolicy; the PEN instantiations of P1PwcPolicy and
         Q1PwcPolicy): the default DeviceMesh with piecewise-constant data.  hdd_last_tile_kernel() must name the
         expected policy with the expected tensor and kappa kind numbers, which proves that each instantiation ran.
generic  product_kernel of products.hip: a mesh without face_info (piecewise-constant data) or a sinusoid kappa.  The
         tile-kernel name must be the one a sentinel stiffness assembly left before the calls.

Both are compared with the oracle, never with each other: row-wise (compare_rows, 1e-12, no floor, every row), the
penalty also per (element row block, column block), boundary_l2 also for exact zeros; every output array starts
NaN-filled and every entry must have been written; the view's host pattern must equal the oracle's row slice, columns
included.  The host preconditions of the meshes are asserted in test_product_cases.py.  Every comparison prints its
ratio first."""
import re

import numpy as np
import pytest

import oracle as O
import product_cases as P

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

TILE, GENERIC = "tile", "generic"
FAMILIES = [TILE, GENERIC]
TK = {"const": H.TENSOR_CONST, "iso": H.TENSOR_ISO_PER_ELEM, "sym": H.TENSOR_SYM_PER_ELEM}
KK = {"const": H.FN_CONST, "per_elem": H.FN_PER_ELEM}
MESH_ETS = [(m, et) for m in ("scrambled", "nvb", "slab", "split") for et in P.mesh_ets(m)]


def _torch():
    import torch
    return torch


# ------------------------------------------------------------------------------------------------------
# which kernel ran
# ------------------------------------------------------------------------------------------------------
def _policy(name):
    """'swipdg_persistent_kernel<Policy<args>, TL, SKIP>' -> (Policy, [args]); booleans as 0 / 1, and trailing
    arguments that equal the template's defaults (all 0 / false here; the name leaves them out) filled in"""
    m = re.match(r"swipdg_persistent_kernel<(\w+)<(.*)>, (true|false), (true|false)>$", name)
    assert m, name
    args = [{"true": "1", "false": "0"}.get(s.strip(), s.strip()) for s in m.group(2).split(",")]
    return m.group(1), args + ["0"] * (5 - len(args))


def _expect_tile_kernel(kind, et, tk, kk, vx):
    """the tile kernel of a product: VolProductPolicy<E, KIND, TK, KK, VX> (TK, KK constant unless elliptic; VX only on
    triangles) or the PEN instantiation {P1,Q1}PwcPolicy<TK, KK, true, VX ..>"""
    name = H.last_tile_kernel()
    pol, args = _policy(name)
    if kind == H.PRODUCT_PENALTY:
        assert pol == ("P1PwcPolicy" if et == H.SIMPLEX else "Q1PwcPolicy"), name
        assert args[:3] == [str(TK[tk]), str(KK[kk]), "1"], name
        assert args[3:] == ["1" if vx and et == H.SIMPLEX else "0", "0"], name
        return
    assert pol == "VolProductPolicy", name
    assert args[0].endswith("Simplex" if et == H.SIMPLEX else "Cube"), name
    if kind != H.PRODUCT_ELLIPTIC:
        tk, kk = "const", "const"
    assert args[1:] == [str(kind), str(TK[tk]), str(KK[kk]), "1" if vx and et == H.SIMPLEX else "0"], name


_SENTINEL = {}


def _sentinel(ctx):
    """a one-element stiffness assembly: leaves a tile-kernel name that no product launches (PEN = false)"""
    if not _SENTINEL:
        loc = H.Grid.structured(H.CUBE, 1, 1).local()
        _SENTINEL.update(dm=H.DeviceMesh(loc), dp=H.DevicePattern(loc))
    H.assemble(ctx, _SENTINEL["dm"], _SENTINEL["dp"], [H.scalar_fn(H.FN_CONST, 1.0)], H.tensor_fn())
    name = H.last_tile_kernel()
    pol, args = _policy(name)
    assert pol == "Q1PwcPolicy" and args[2] == "0", name
    return name


# ------------------------------------------------------------------------------------------------------
# one view on the device
# ------------------------------------------------------------------------------------------------------
class View:
    """DeviceMesh and the two DevicePatterns of a case's view; family generic with piecewise-constant data: the mesh
    is passed without face_info"""

    def __init__(self, c, family, vertex_indexed=True):
        self.c, self.family, self.vx = c, family, vertex_indexed
        self.loc = c.local()
        self.dm = H.DeviceMesh(self.loc, vertex_indexed=vertex_indexed)
        assert (self.dm.elem_vertices is not None) == vertex_indexed
        if family == GENERIC:
            self.dm.t.face_info = None
        self.dp = {True: H.DevicePattern(self.loc, volume=True), False: H.DevicePattern(self.loc)}
        self.zero_rows = P.penalty_zero_rows(c)

    def coeffs(self, tk, kk):
        torch = _torch()
        t, k = P.view_coeffs(self.c.name, self.c.et, tk, kk, self.loc.global_id)
        if tk == "const":
            ten = H.tensor_fn(H.TENSOR_CONST, c=P.TENSOR_CONST)
        else:
            ten = H.tensor_fn(TK[tk], per_elem=torch.from_numpy(t).cuda())
        if kk == "const":
            kap = H.scalar_fn(H.FN_CONST, P.KAPPA_CONST)
        elif kk == "per_elem":
            kap = H.scalar_fn(H.FN_PER_ELEM, per_elem=torch.from_numpy(k).cuda())
        else:
            s = P.SINUSOID
            kap = H.scalar_fn(H.FN_SINUSOID, s["c"], b=s["b"], kx=s["kx"], ky=s["ky"], order=s["order"])
        return kap, ten

    def run(self, ctx, kind, tk="sym", kk="per_elem", beta=1.0):
        """the product's values (numpy) from a NaN-filled array; the pattern checked against the oracle's slice"""
        torch = _torch()
        c = self.c
        dp = self.dp[kind != H.PRODUCT_PENALTY]
        rp, col, _ = P.reference(c.name, c.et, kind, c.neumann, tk, kk, beta)
        assert np.array_equal(dp.host[0], rp) and np.array_equal(dp.host[1], col), (c.label(), kind)
        kap, ten = self.coeffs(tk, kk)
        out = torch.full((dp.nnz,), float("nan"), dtype=torch.float64, device="cuda")
        H.product(ctx, self.dm, kind, dp, kappa=kap, tensor=ten, prm=H.params(beta=beta), out=out)
        got = out.cpu().numpy()
        if self.family == TILE and kk != P.SMOOTH:
            _expect_tile_kernel(kind, c.et, tk, kk, self.vx)
        return got

    def check(self, ctx, kind, tk="sym", kk="per_elem", beta=1.0, worst=None, fast=False):
        c = self.c
        got = self.run(ctx, kind, tk, kk, beta)
        rp, _, ref = P.reference(c.name, c.et, kind, c.neumann, tk, kk, beta)
        label = "%s %s %s %s/%s beta=%g%s" % (self.family, c.label(), P.KIND_NAME[kind], tk, kk, beta,
                                              "" if self.vx else " element-major")
        fam = GENERIC if kk == P.SMOOTH else self.family
        P.check_product(label, kind, rp, got, ref, c.nb, worst, fam + " ", fast, self.zero_rows)
        return got


def _with_family(ctx, family, body):
    """run body(); for the generic family no tile kernel may have been launched in between"""
    if family == TILE:
        return body()
    before = _sentinel(ctx)
    r = body()
    assert H.last_tile_kernel() == before, (H.last_tile_kernel(), before)
    return r


def _five_kinds_and_exponent(ctx, v, worst=None):
    """all five kinds at beta = 1 (sym / per_elem data) and the penalty at beta = 0.5, which must differ"""
    for kind in P.KINDS:
        got = v.check(ctx, kind, worst=worst)
    half = v.check(ctx, H.PRODUCT_PENALTY, beta=0.5, worst=worst)
    if np.max(np.abs(got)) > 0:                                    # (one element, all Neumann: no penalised face)
        assert np.max(np.abs(half - got)) > 1e-3 * np.max(np.abs(got)), v.c.label()
    else:
        assert v.c.neumann and v.c.grid.ne == 1


# ------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("et,family,vx", [(H.SIMPLEX, TILE, True), (H.SIMPLEX, TILE, False), (H.CUBE, TILE, True),
                                          (H.SIMPLEX, GENERIC, True), (H.CUBE, GENERIC, True)])
def test_instantiation_table(ctx, et, family, vx):
    """scrambled mesh: all five kinds; elliptic and penalty with all 3 x 2 (tensor, kappa) kinds; P1 on the
    vertex-indexed and on the element-major geometry"""
    v = View(P.case("scrambled", et), family, vertex_indexed=vx)

    def body():
        for kind in P.KINDS:
            pairs = [("sym", "per_elem")]
            if kind in P.COEFF_KINDS:
                pairs = [(t, k) for t in P.TENSOR_KINDS for k in P.KAPPA_KINDS]
            for tk, kk in pairs:
                v.check(ctx, kind, tk, kk)
    _with_family(ctx, family, body)


@pytest.mark.parametrize("neumann", [False, True], ids=["dirichlet", "neumann"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mesh,et", [(m, e) for m, e in MESH_ETS if m in ("scrambled", "nvb")])
def test_boundary_and_exponent(ctx, mesh, et, family, neumann):
    """Neumann faces: skipped by the penalty, kept by boundary_l2; beta = 0.5 against beta = 1"""
    v = View(P.case(mesh, et, neumann), family)
    _with_family(ctx, family, lambda: _five_kinds_and_exponent(ctx, v))


@pytest.mark.parametrize("neumann", [False, True], ids=["dirichlet", "neumann"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mesh,et", [(m, e) for m, e in MESH_ETS if m in ("slab", "split")])
def test_local_views(ctx, mesh, et, family, neumann):
    """own_begin > 0, ghosts on both sides, per-element data indexed by the view's global ids: the owned rows equal
    the oracle's row slice, every entry written"""
    v = View(P.case(mesh, et, neumann), family)
    assert v.loc.own_begin > 0 and v.loc.n_ghost > 0
    _with_family(ctx, family, lambda: _five_kinds_and_exponent(ctx, v))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("et", P.ETS)
@pytest.mark.parametrize("shape", P.EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_edge_meshes(ctx, shape, et, family):
    """one element (penalty pattern = volume pattern) and strips one element wide, both boundaries"""
    for neumann in (False, True):
        v = View(P.case("edge_%dx%d" % shape, et, neumann), family)
        _with_family(ctx, family, lambda: _five_kinds_and_exponent(ctx, v))


@pytest.mark.parametrize("et", P.ETS)
def test_multipass(ctx, et):
    """more tiles than workgroup slots of the persistent grid (4 per CU for VolProductPolicy and the vertex-indexed
    P1PwcPolicy, 3 for Q1PwcPolicy): the tile loop goes round more than once"""
    torch = _torch()
    c = P.case("multipass", et)
    assert c.tiles() > 4 * torch.cuda.get_device_properties(0).multi_processor_count
    v = View(c, TILE)
    for kind in P.KINDS:
        v.check(ctx, kind, fast=True)
    for neumann, beta in [(True, 1.0), (False, 0.5), (True, 0.5)]:
        vn = View(P.case("multipass", et, neumann), TILE) if neumann else v
        vn.check(ctx, H.PRODUCT_PENALTY, beta=beta, fast=True)


@pytest.mark.parametrize("mesh,et", [(m, e) for m, e in MESH_ETS if m != "split"])
def test_generic_smooth_kappa(ctx, mesh, et):
    """sinusoid kappa (order 3) sends elliptic and penalty to the generic kernel on the default mesh"""
    for neumann in (False, True):
        v = View(P.case(mesh, et, neumann), TILE)

        def body():
            for tk in P.TENSOR_KINDS:
                v.check(ctx, H.PRODUCT_ELLIPTIC, tk, P.SMOOTH)
                for beta in P.BETAS:
                    v.check(ctx, H.PRODUCT_PENALTY, tk, P.SMOOTH, beta)
        _with_family(ctx, GENERIC, body)


@pytest.mark.parametrize("neumann", [False, True], ids=["dirichlet", "neumann"])
@pytest.mark.parametrize("deg", [1, 2])
def test_hex_local_view(ctx, deg, neumann):
    """the graded hexahedral mesh of test_gpu_hex_graded.py on g.local(1, 2): 36 owned elements behind 24, 12 smaller
    ghosts; all five kinds against the row slice of the Q_p oracle"""
    from test_gpu_hex_graded import _coefficients, _setup
    torch = _torch()
    g, ei, q = _setup(deg, H.BOUNDARY_ALL_NEUMANN if neumann else H.BOUNDARY_ALL_DIRICHLET)
    loc = g.local(1, 2)
    assert loc.own_begin > 0 and loc.n_own == 36 and loc.n_ghost == 12 and np.all(np.diff(loc.global_id) > 0)
    own_nbr = loc.neighbors[:, loc.own_begin:loc.own_end]
    assert np.any(own_nbr == (H.NBR_NEUMANN if neumann else H.NBR_DIRICHLET)) and not np.any(
        own_nbr == (H.NBR_DIRICHLET if neumann else H.NBR_NEUMANN))
    kap, ten, okap, oten = _coefficients("per_elem", g.ne, ei, ids=loc.global_id)
    dm = H.DeviceMesh(loc)
    a, b = g.subdomain_range(1, 2)
    oprm = O.qp_params(q, boundary=O.BOUNDARY_NEUMANN if neumann else O.BOUNDARY_DIRICHLET)
    before = _sentinel(ctx)
    for kind in P.KINDS:
        dp = H.DevicePattern(loc, volume=kind != H.PRODUCT_PENALTY)
        out = torch.full((dp.nnz,), float("nan"), dtype=torch.float64, device="cuda")
        H.product(ctx, dm, kind, dp, kappa=kap, tensor=ten, out=out)
        rp, col, val = O.qp_product(q, kind, kappa=okap, A=oten, prm=oprm, elem_index=ei)
        lo, hi = rp[a * g.nb], rp[b * g.nb]
        assert np.array_equal(dp.host[0], rp[a * g.nb:b * g.nb + 1] - lo), kind
        assert np.array_equal(dp.host[1], col[lo:hi]), kind
        label = "generic hex p=%d %s %s" % (deg, "neumann" if neumann else "dirichlet", P.KIND_NAME[kind])
        assert np.max(np.abs(val[lo:hi])) > 0, label
        P.check_product(label, kind, dp.host[0], out.cpu().numpy(), val[lo:hi], g.nb, None, "hex ")
    assert H.last_tile_kernel() == before


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mesh,et", [(m, e) for m, e in MESH_ETS if m != "split"])
def test_invariants(ctx, mesh, et, family):
    """from the GPU values, the pattern and the mesh alone: 1^T M 1 = |Omega|, M 1 = 0 and symmetry for h1_semi and
    elliptic, 1^T B 1 = |dOmega| with Neumann faces counted, P symmetric, P u = 0 for a global affine u under
    all-Neumann and P u != 0 under all-Dirichlet"""
    for neumann in (False, True):
        c = P.case(mesh, et, neumann)
        v = View(c, family)

        def body():
            for kind in P.KINDS:
                got = v.run(ctx, kind)
                rp, col, _ = P.reference(mesh, et, kind, neumann)
                P.check_invariants("%s %s %s" % (family, c.label(), P.KIND_NAME[kind]), c, kind, rp, col, got,
                                   None, family + " invariants")
        _with_family(ctx, family, body)


def test_pattern_guard(ctx):
    """an element-local kind refuses the SWIPDG pattern (right row count, other layout); the penalty on one element,
    whose SWIPDG pattern has the volume pattern's nnz, still runs"""
    loc = H.Grid.structured(H.SIMPLEX, 6, 5, (-1, -1), (1, 1)).local()
    dm, face, vol = H.DeviceMesh(loc), H.DevicePattern(loc), H.DevicePattern(loc, volume=True)
    assert face.t.n_rows == vol.t.n_rows and face.nnz > vol.nnz == loc.nb * loc.nb * loc.n_own
    for kind in (H.PRODUCT_L2, H.PRODUCT_H1_SEMI, H.PRODUCT_ELLIPTIC, H.PRODUCT_BOUNDARY_L2):
        with pytest.raises(H.HddError):
            H.product(ctx, dm, kind, face, kappa=H.scalar_fn(H.FN_CONST, 1.0), tensor=H.tensor_fn(), prm=H.params())
    H.product(ctx, dm, H.PRODUCT_L2, vol, prm=H.params())
    for et in P.ETS:
        for family in FAMILIES:
            v = View(P.case("single", et), family)
            assert v.dp[False].nnz == v.dp[True].nnz == v.c.nb ** 2
            _with_family(ctx, family, lambda: _five_kinds_and_exponent(ctx, v))
