"""GPU parity of the Q_p hexahedral kernels (hex_qp.hip, rhs.hip, products.hip) on a graded rectilinear mesh, where face
neighbours differ in size, against the graded Q_p oracle (QpGrid(nodes=...), anchored by tests/test_oracle_qp.py).

Every other hexahedral test runs on an equidistant box, on which the neighbour's Jacobian, |F| and h equal the
element's own: taking the wrong side's geometry in a flux, a penalty or a neighbour trace, or congruent but
misplaced ghost coordinates, cannot show there.  Here they are O(1) errors.

Mesh: 5 x 4 x 3 hexahedra on [-1,1] x [0,1.5] x [0.5,2]; x widths in geometric ratio 1.7, y widths 1:3:1:2,
z widths 2:1:3 (hex_tools.GRADED_NODES), so each axis has its own grading and neighbour ratios reach 3.  Built
through hdd_grid_create_hex_from_connectivity with subdomain 0 = x-columns 0-1 (24 elements) and subdomain 1 =
the rest (36): subdomain-major renumbering, and 60 elements = three full 16-element groups of the p = 3 GEMM
kernel plus a ragged one.

Tolerances are the project's: compare_rows(..., 1e-12) for matrices and products, _close of test_gpu_rhs.py
(|db| <= 1e-12 max(1, max|b|)) for vectors.  Every case prints its worst relative difference before asserting."""
import numpy as np
import pytest

import oracle as O
from cases import compare_rows
from hex_tools import GRADED_NODES, graded_hex_mesh, lex_to_product_graded
from test_gpu_hex import _spd_tensors
from test_gpu_rhs import _close

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

RTOL = 1e-12
N = tuple(len(x) - 1 for x in GRADED_NODES)
LO, UP = tuple(x[0] for x in GRADED_NODES), tuple(x[-1] for x in GRADED_NODES)
CONST_TENSOR = (1.5, 0.2, -0.1, 2.0, 0.15, 0.8)            # xx xy xz yy yz zz, SPD, every off-diagonal nonzero
KINDS = [H.PRODUCT_L2, H.PRODUCT_H1_SEMI, H.PRODUCT_ELLIPTIC, H.PRODUCT_BOUNDARY_L2, H.PRODUCT_PENALTY]


def _torch():
    import torch
    return torch


def _setup(deg, boundary=H.BOUNDARY_ALL_DIRICHLET):
    coords, ev = graded_hex_mesh(GRADED_NODES)
    sd = (np.arange(ev.shape[0]) % N[0] >= 2).astype(np.int32)
    g = H.Grid.from_connectivity(H.HEX, coords, ev, subdomain=sd, n_sub=2, boundary=boundary, degree=deg)
    assert g.ne == 60 and g.subdomain_range(0, 1) == (0, 24)
    ei = lex_to_product_graded(g, GRADED_NODES)
    q = O.QpGrid(3, deg, N, LO, UP, nodes=GRADED_NODES)
    return g, ei, q


def _coefficients(name, ne, ei, ids=None):
    """(kappa, tensor) for the product and for the oracle.  Per-element data are drawn in the product's global
    element order; ids = the global ids of a rank-local view's elements (ghosts included), ei maps the oracle's
    lexicographic elements to global ids."""
    torch = _torch()
    ids = np.arange(ne) if ids is None else ids
    if name == "const":
        return (H.scalar_fn(H.FN_CONST, 1.3), H.tensor_fn(c=CONST_TENSOR, dim=3),
                O.scalar(O.FN_CONST, 1.3), O.qp_tensor(c=CONST_TENSOR))
    T = _spd_tensors(ne, 7)
    ten = H.tensor_fn(H.TENSOR_SYM_PER_ELEM, per_elem=torch.from_numpy(np.ascontiguousarray(T[ids].T)).cuda(), dim=3)
    oten = O.qp_tensor(O.TENSOR_SYM_PER_ELEM, per_elem=np.ascontiguousarray(T[ei]))
    if name == "per_elem":
        kel = np.random.default_rng(8).uniform(0.2, 4.0, ne)
        return (H.scalar_fn(H.FN_PER_ELEM, per_elem=torch.from_numpy(np.ascontiguousarray(kel[ids])).cuda()), ten,
                O.scalar(O.FN_PER_ELEM, per_elem=np.ascontiguousarray(kel[ei])), oten)
    assert name == "sinusoid"
    return (H.scalar_fn(H.FN_SINUSOID, 1.0, b=0.5, kx=3.0, ky=2.0, order=3), ten,
            O.scalar(O.FN_SINUSOID, 1.0, 0.5, 3.0, 2.0, order=3), oten)


def _check_rows(label, rp, got, ref):
    worst, ok = compare_rows(rp, got, ref, RTOL)
    print("graded hex %s: worst row rel diff %.3g" % (label, worst))
    assert ok, (label, worst)


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("coef,boundary", [("const", "dirichlet"), ("per_elem", "dirichlet"), ("per_elem", "neumann"),
                                           ("sinusoid", "dirichlet")])
def test_graded_hex_assembly_equals_oracle(ctx, deg, coef, boundary):
    neumann = boundary == "neumann"
    g, ei, q = _setup(deg, H.BOUNDARY_ALL_NEUMANN if neumann else H.BOUNDARY_ALL_DIRICHLET)
    loc = g.local()
    dm, dp = H.DeviceMesh(loc), H.DevicePattern(loc)
    kap, ten, okap, oten = _coefficients(coef, g.ne, ei)
    (val,) = H.assemble(ctx, dm, dp, [kap], ten, H.params_for(deg, 3))
    _torch().cuda.synchronize()
    rp, col, _ = dp.host
    oprm = O.qp_params(q, boundary=O.BOUNDARY_NEUMANN if neumann else O.BOUNDARY_DIRICHLET)
    orp, ocol, oval = O.qp_assemble(q, okap, oten, oprm, elem_index=ei)
    assert np.array_equal(rp, orp) and np.array_equal(col, ocol)
    _check_rows("assembly p=%d %s %s" % (deg, coef, boundary), rp, val.cpu().numpy(), oval)


def test_graded_hex_q3_gemm_and_register_kernels():
    """p = 3, per-element kappa and tensor: the default GEMM kernel and HDD_VARIANT_HEX_Q3_REGISTER (both fed by
    hex_q3_setup_kernel, which reads the neighbour's geometry), each against the oracle and against each other."""
    torch = _torch()
    deg = 3
    g, ei, q = _setup(deg)
    loc = g.local()
    dm, dp = H.DeviceMesh(loc), H.DevicePattern(loc)
    kap, ten, okap, oten = _coefficients("per_elem", g.ne, ei)
    vals = []
    for variant in (0, H.VARIANT_HEX_Q3_REGISTER):
        c = H.Context(0)
        c.set_variant(variant)
        (v,) = H.assemble(c, dm, dp, [kap], ten, H.params_for(deg, 3))
        torch.cuda.synchronize()
        vals.append(v.cpu().numpy())
        del c
    rp = dp.host[0]
    _, _, oval = O.qp_assemble(q, okap, oten, O.qp_params(q), elem_index=ei)
    _check_rows("q3 gemm vs oracle", rp, vals[0], oval)
    _check_rows("q3 register vs oracle", rp, vals[1], oval)
    _check_rows("q3 gemm vs register", rp, vals[0], vals[1])


@pytest.mark.parametrize("deg", [2, 3])
@pytest.mark.parametrize("coef", ["const", "per_elem"])
def test_graded_hex_rank_local_slab(ctx, deg, coef):
    """g.local(1, 2): the 12 ghosts (x-column 1) are smaller than the owned elements of x-column 2 they touch.
    The slab's values equal the global slice bit for bit and the oracle's rows at the parity tolerance."""
    g, ei, q = _setup(deg)
    full = g.local()
    dpg = H.DevicePattern(full)
    kap, ten, okap, oten = _coefficients(coef, g.ne, ei)
    (gval,) = H.assemble(ctx, H.DeviceMesh(full), dpg, [kap], ten, H.params_for(deg, 3))
    loc = g.local(1, 2)
    assert loc.n_own == 36 and loc.n_ghost == 12
    ghost = np.r_[0:loc.own_begin, loc.own_end:loc.n_local]
    own_x0 = loc.coords[0, loc.own_begin:loc.own_end].min()
    assert np.all(loc.coords[3, ghost] == own_x0)              # ghosts' upper x face = the slab's lower x face
    hx_ghost = loc.coords[3, ghost] - loc.coords[0, ghost]
    assert np.all(hx_ghost < 0.6 * (GRADED_NODES[0][3] - GRADED_NODES[0][2]))
    dp = H.DevicePattern(loc)
    lkap, lten, _, _ = _coefficients(coef, g.ne, ei, ids=loc.global_id)
    (val,) = H.assemble(ctx, H.DeviceMesh(loc), dp, [lkap], lten, H.params_for(deg, 3))
    _torch().cuda.synchronize()
    a, b = g.subdomain_range(1, 2)
    grp = dpg.host[0]
    lo, hi = grp[a * g.nb], grp[b * g.nb]
    assert np.array_equal(dp.host[1], dpg.host[1][lo:hi])
    assert np.array_equal(val.cpu().numpy(), gval.cpu().numpy()[lo:hi])
    _, _, oval = O.qp_assemble(q, okap, oten, O.qp_params(q), elem_index=ei)
    _check_rows("slab p=%d %s" % (deg, coef), dp.host[0], val.cpu().numpy(), oval[lo:hi])


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("coef", ["const", "per_elem"])
def test_graded_hex_products(ctx, deg, coef):
    """All five products; the penalty product is the one with face terms on the face pattern: it reads the
    neighbour's geometry for its trace and both sides' kappa and tensor.  const: kappa = 1.5, A = I, as
    test_products_hex; per_elem: per-element kappa and symmetric tensor."""
    torch = _torch()
    g, ei, q = _setup(deg)
    loc = g.local()
    dm = H.DeviceMesh(loc)
    if coef == "const":
        kap, ten, okap, oten = H.scalar_fn(H.FN_CONST, 1.5), H.tensor_fn(dim=3), O.scalar(O.FN_CONST, 1.5), None
    else:
        kap, ten, okap, oten = _coefficients("per_elem", g.ne, ei)
    for kind in KINDS:
        dp = H.DevicePattern(loc, volume=kind != H.PRODUCT_PENALTY)
        val = H.product(ctx, dm, kind, dp, kappa=kap, tensor=ten)
        torch.cuda.synchronize()
        rp, col, oval = O.qp_product(q, kind, kappa=okap, A=oten, elem_index=ei)
        assert np.array_equal(dp.host[0], rp) and np.array_equal(dp.host[1], col), kind
        _check_rows("product %d p=%d %s" % (kind, deg, coef), rp, val.cpu().numpy(), oval)


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_graded_hex_rhs(ctx, deg):
    """The cases of test_rhs_hex: ESV2007 force + sinusoid Dirichlet data with kappa = 2, and ESV2007 force +
    constant Neumann data on the all-Neumann grid."""
    torch = _torch()
    for boundary, bk in [(H.BOUNDARY_ALL_DIRICHLET, O.BOUNDARY_DIRICHLET), (H.BOUNDARY_ALL_NEUMANN, O.BOUNDARY_NEUMANN)]:
        g, ei, q = _setup(deg, boundary)
        dm = H.DeviceMesh(g.local())
        hk = dict(force=H.esv2007_force(3))
        ok = dict(force=O.esv2007_force(3))
        if bk == O.BOUNDARY_DIRICHLET:
            hk.update(dirichlet=H.scalar_fn(H.FN_SINUSOID, 1.0, b=0.5, kx=1.3, ky=0.7, order=3),
                      kappa=H.scalar_fn(H.FN_CONST, 2.0), tensor=H.tensor_fn(dim=3))
            ok.update(dirichlet=O.scalar(O.FN_SINUSOID, 1.0, 0.5, 1.3, 0.7, order=3), kappa=O.scalar(O.FN_CONST, 2.0))
        else:
            hk.update(neumann=H.scalar_fn(H.FN_CONST, 0.75))
            ok.update(neumann=O.scalar(O.FN_CONST, 0.75))
        b = H.rhs(ctx, dm, prm=H.params_for(deg, 3), **hk)
        torch.cuda.synchronize()
        ref = O.qp_rhs_swipdg(q, prm=O.qp_params(q, boundary=bk), elem_index=ei, **ok)
        got = b.cpu().numpy()
        print("graded hex rhs p=%d boundary=%d: max |db| / max(1, max|b|) %.3g"
              % (deg, bk, np.max(np.abs(got - ref)) / max(1.0, np.max(np.abs(ref)))))
        assert _close(got, ref), (deg, boundary)


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_graded_hex_dirichlet_consistency(ctx, deg):
    """u = 1 solves the homogeneous problem with g_D = 1, so A_gpu . 1 = b_gpu(g_D = 1) row by row (piecewise
    constant kappa and tensor: matrix and right-hand side then integrate exactly).  On a graded mesh this holds
    only if every inner face's consistency and penalty blocks cancel between the element's own block and the
    neighbour's, i.e. both see the right side's geometry; it couples the matrix and RHS kernels without the oracle."""
    g, ei, q = _setup(deg)
    loc = g.local()
    dm, dp = H.DeviceMesh(loc), H.DevicePattern(loc)
    kap, ten, _, _ = _coefficients("per_elem", g.ne, ei)
    prm = H.params_for(deg, 3)
    (val,) = H.assemble(ctx, dm, dp, [kap], ten, prm)
    b = H.rhs(ctx, dm, kappa=kap, tensor=ten, dirichlet=H.scalar_fn(H.FN_CONST, 1.0), prm=prm)
    _torch().cuda.synchronize()
    rp, col, _ = dp.host
    b = b.cpu().numpy()
    A1 = O.to_scipy(rp, col, val.cpu().numpy()) @ np.ones(g.ne * g.nb)
    assert np.max(np.abs(b)) > 0
    diff = np.max(np.abs(A1 - b)) / np.max(np.abs(b))
    print("graded hex A.1 - b(g_D=1) p=%d: %.3g of max|b|" % (deg, diff))
    assert diff <= 1e-12
