"""The right-hand side and the generic products give the bits they gave before rhs.hip was split into rhs.hip,
products.hip and the shared element helpers of elem_affine.hh (one geometry, one tensor, one reference face, one
loader, one launcher): tests/golden/rhs_bits_parent.json, recorded on an MI355X by tests/golden/make_rhs_bits.py at
commit acdf956, the commit before that change, holds per case the SHA-256 of the output -- digests, not vectors; the
first four values are there for a readable failure.  No value here sums across threads, so the result depends neither
on the grid nor on the device's size.

rhs2d_kernel (16 instantiations) and rhs2d_face_kernel (4): the sheared 37 x 11 mesh of rhs_cases.py (several waves,
a ragged last one, boundary elements in more than one wave), P1 and Q1, crossed with the vertex-indexed or the
element-major geometry, the cos-product force on the order-4 rule (unrolled) or on the run-time rule
(VARIANT_RHS_GENERIC), and split (boundary data, the default), fused (boundary data, VARIANT_RHS_FUSED) or no
boundary data at all (fused as well).  Boundary data as in test_gpu_rhs_tiers.py: sinusoid g_D, per-element kappa,
Neumann cos product on marked elements; once with the iso and once with the symmetric per-element tensor.  The
mirrored mesh (det J < 0) once per element type and face path.

rhs_kernel: the 60-element graded hexahedral mesh of test_gpu_hex_graded.py at degrees 1, 2 and 3, force + Dirichlet
+ Neumann data with the const, iso and sym tensor.

product_kernel (the generic family; the tile driver's is not touched): a mesh without face_info, as
test_gpu_products_grid.py forces it -- all five kinds on the scrambled and the 1 x 9 mesh of product_cases.py, P1 and
Q1, symmetric tensor and per-element kappa at beta = 1 and 0.5; elliptic and penalty with the sinusoid kappa; all
five kinds on the hexahedral mesh at degrees 1 and 2.  No tile kernel may have run in between.

The fixture also holds, as an input condition, the SHA-256 of the mesh and coefficient arrays: when one of these
differs the test fails saying that the inputs differ (the grid code or the host's numpy changed), not the kernels.

A later change that alters the arithmetic of an entry on purpose regenerates the fixture with make_rhs_bits.py and
says so in its description."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import product_cases as P
import rhs_cases as R

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rhs_bits_parent.json")
G_D = (1.0, 0.5, 1.3, 0.7)                 # sinusoid c, b, kx, ky
G_N = (2.0, 0.9, 0.7, 0.4)                 # cos product c, kx, ky (, kz in 3d)
HEX_CONST_TENSOR = (1.5, 0.2, -0.1, 2.0, 0.15, 0.8)

# ("rhs2d", element type, mirrored, tensor, vertex-indexed, unrolled rule, path)
RHS2D = [("rhs2d", et, False, tk, vx, cos, path) for et in (H.SIMPLEX, H.CUBE) for tk in ("iso", "sym")
         for vx in (True, False) for cos in (True, False) for path in ("split", "fused", "nobnd")
         if path != "nobnd" or tk == "iso"]                                  # (no boundary data: no tensor)
RHS2D += [("rhs2d", et, True, "sym", vx, True, path) for et in (H.SIMPLEX, H.CUBE) for vx in (True, False)
          for path in ("split", "fused")]
# ("rhshex", degree, tensor)
RHSHEX = [("rhshex", deg, tk) for deg in (1, 2, 3) for tk in ("const", "iso", "sym")]
# ("product", mesh, element type, kind, kappa, beta); ("producthex", degree, kind)
PRODUCT = [("product", mesh, et, kind, "per_elem", beta) for mesh in ("scrambled", "edge_1x9") for et in P.ETS
           for kind in P.KINDS for beta in P.BETAS]
PRODUCT += [("product", "scrambled", et, kind, P.SMOOTH, 1.0) for et in P.ETS for kind in P.COEFF_KINDS]
PRODUCTHEX = [("producthex", deg, kind) for deg in (1, 2) for kind in P.KINDS]
CASES = RHS2D + RHSHEX + PRODUCT + PRODUCTHEX


def case_id(c):
    if c[0] == "rhs2d":
        _, et, mirror, tk, vx, cos, path = c
        return "rhs2d-%s%s-%s-%s-%s-%s" % (R.ET_NAME[et], "-mirrored" if mirror else "", tk, "vx" if vx else "em",
                                           "cos" if cos else "rule", path)
    if c[0] == "rhshex":
        return "rhshex-p%d-%s" % c[1:]
    if c[0] == "product":
        _, mesh, et, kind, kk, beta = c
        return "product-%s-%s-%s-%s-beta%g" % (mesh, P.ET_NAME[et], P.KIND_NAME[kind], kk, beta)
    return "producthex-p%d-%s" % (c[1], P.KIND_NAME[c[2]])


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(None)
def _variant_ctx(variant):
    c = H.Context(0)
    c.set_variant(variant)
    return c


def _result(y):
    return dict(shape=list(y.shape), y_head=[float(v) for v in y[:4]], y_sha256=_sha(y))


def _marked_mesh(grid):
    """the grid's whole local mesh with a seeded half of its boundary elements marked Neumann"""
    loc = grid.local()
    R.set_boundary(loc, R.mark_elements(loc.neighbors, 31), H.NBR_NEUMANN)
    return loc


def _rhs_data(loc, tk, dim):
    """per-element kappa and the tensor of a boundary run, in the local mesh's element order: (kappa, tensor,
    the arrays behind them)"""
    n = loc.n_local
    rng = np.random.default_rng(29)
    kel = rng.uniform(0.5, 2.0, n)
    if tk == "const":
        return kel, H.tensor_fn(c=HEX_CONST_TENSOR, dim=3), np.array(HEX_CONST_TENSOR)
    if tk == "iso":
        t = rng.uniform(0.5, 2.0, n)
        return kel, H.tensor_fn(H.TENSOR_ISO_PER_ELEM, per_elem=_dev(t), dim=dim), t
    if dim == 3:
        from test_gpu_hex import _spd_tensors
        t = np.ascontiguousarray(_spd_tensors(n, 7).T)
    else:
        a = rng.uniform(0.5, 2.0, n); c = rng.uniform(0.5, 2.0, n); b = rng.uniform(-0.3, 0.3, n)
        t = np.stack([a, b, c], 0)
    return kel, H.tensor_fn(H.TENSOR_SYM_PER_ELEM, per_elem=_dev(t), dim=dim), t


def _boundary_data(loc, tk, dim):
    kel, ten, t = _rhs_data(loc, tk, dim)
    kw = dict(kappa=H.scalar_fn(H.FN_PER_ELEM, per_elem=_dev(kel)), tensor=ten,
              dirichlet=H.scalar_fn(H.FN_SINUSOID, G_D[0], b=G_D[1], kx=G_D[2], ky=G_D[3], order=3),
              neumann=H.scalar_fn(H.FN_COS_PRODUCT, G_N[0], b=G_N[3] if dim == 3 else 0.0, kx=G_N[1], ky=G_N[2], order=2))
    return kw, (kel, t)


def _record_rhs2d(c):
    _, et, mirror, tk, vx, cos, path = c
    et_, coords, ev = R.sheared_mesh(et, mirror=mirror)
    loc = _marked_mesh(H.Grid.from_connectivity(et_, coords, ev))
    dm = H.DeviceMesh(loc)
    assert dm.elem_vertices is not None
    kw, data = _boundary_data(loc, tk, 2) if path != "nobnd" else ({}, ())
    variant = ((0 if vx else H.VARIANT_ELEMENT_MAJOR) | (0 if cos else H.VARIANT_RHS_GENERIC) |
               (H.VARIANT_RHS_FUSED if path == "fused" else 0))
    b = H.rhs(_variant_ctx(variant), dm, force=H.esv2007_force(), prm=H.params(), **kw)
    inputs = dict(n_own=int(loc.n_own), mesh_sha256=_sha(loc.coords, loc.neighbors, *loc.vertices()), data_sha256=_sha(*data))
    return inputs, _result(b.cpu().numpy())


def _hex_grid(deg):
    from test_gpu_hex_graded import _setup
    g, ei, _ = _setup(deg)
    return g, ei


def _record_rhshex(c):
    _, deg, tk = c
    g, _ = _hex_grid(deg)
    loc = _marked_mesh(g)
    kw, data = _boundary_data(loc, tk, 3)
    b = H.rhs(_variant_ctx(0), H.DeviceMesh(loc), force=H.esv2007_force(3), prm=H.params_for(deg, 3), **kw)
    inputs = dict(n_own=int(loc.n_own), mesh_sha256=_sha(loc.coords, loc.neighbors), data_sha256=_sha(*data))
    return inputs, _result(b.cpu().numpy())


def _run_product(dm, loc, kind, kap, ten, prm):
    """the product's values from a NaN-filled array; no tile kernel may run (the generic family)"""
    import torch
    from test_gpu_products_grid import _sentinel
    ctx = _variant_ctx(0)
    dp = H.DevicePattern(loc, volume=kind != H.PRODUCT_PENALTY)
    out = torch.full((dp.nnz,), float("nan"), dtype=torch.float64, device="cuda")
    before = _sentinel(ctx)
    H.product(ctx, dm, kind, dp, kappa=kap, tensor=ten, prm=prm, out=out)
    assert H.last_tile_kernel() == before, (H.last_tile_kernel(), before)
    y = out.cpu().numpy()
    assert not np.isnan(y).any()
    return y


def _record_product(c):
    _, mesh, et, kind, kk, beta = c
    loc = P.case(mesh, et).local()
    dm = H.DeviceMesh(loc)
    if kk != P.SMOOTH:
        dm.t.face_info = None
    t, k = P.view_coeffs(mesh, et, "sym", kk, loc.global_id)
    s = P.SINUSOID
    kap = (H.scalar_fn(H.FN_SINUSOID, s["c"], b=s["b"], kx=s["kx"], ky=s["ky"], order=s["order"]) if kk == P.SMOOTH
           else H.scalar_fn(H.FN_PER_ELEM, per_elem=_dev(k)))
    y = _run_product(dm, loc, kind, kap, H.tensor_fn(H.TENSOR_SYM_PER_ELEM, per_elem=_dev(t)), H.params(beta=beta))
    inputs = dict(n_own=int(loc.n_own), mesh_sha256=_sha(loc.coords, loc.neighbors),
                  data_sha256=_sha(t, *([] if k is None else [k])))
    return inputs, _result(y)


def _record_producthex(c):
    from test_gpu_hex_graded import _coefficients
    _, deg, kind = c
    g, ei = _hex_grid(deg)
    loc = g.local()
    kap, ten, _, _ = _coefficients("per_elem", g.ne, ei)
    y = _run_product(H.DeviceMesh(loc), loc, kind, kap, ten, H.params_for(deg, 3))
    inputs = dict(n_own=int(loc.n_own), mesh_sha256=_sha(loc.coords, loc.neighbors),
                  data_sha256=_sha(kap._keep[0].cpu().numpy(), ten._keep.cpu().numpy()))
    return inputs, _result(y)


RECORD = dict(rhs2d=_record_rhs2d, rhshex=_record_rhshex, product=_record_product, producthex=_record_producthex)


def record(c):
    """(inputs, result) of one case: what the fixture holds for it"""
    return RECORD[c[0]](c)


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_has_exactly_the_cases(parent):
    assert sorted(parent["cases"]) == sorted(case_id(c) for c in CASES)
    assert len(set(case_id(c) for c in CASES)) == len(CASES)
    # every rhs2d_kernel<TRI, VX, NQ / FK, SPLIT> and rhs2d_face_kernel<TRI, VX> has a case that launches it
    assert len({(c[1], c[4], c[5], c[6] == "split") for c in RHS2D}) == 16
    for c in CASES:
        rec = parent["cases"][case_id(c)]["result"]
        assert rec["y_sha256"] != _sha(np.zeros(rec["shape"])), case_id(c)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_bits_are_the_parents(parent, c):
    want = parent["cases"][case_id(c)]
    inputs, got = record(c)
    if inputs != want["inputs"]:
        pytest.fail("the INPUTS differ from the recorded ones (mesh or coefficient arrays), not the kernels: %r != %r"
                    % (inputs, want["inputs"]))
    print(got)
    for key in ("shape", "y_head", "y_sha256"):
        assert got[key] == want["result"][key], (key, got, want["result"])
