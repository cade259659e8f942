"""The 2d right-hand side (rhs2d_kernel, rhs2d_faces, rhs2d_face_kernel) on general geometry against the oracle on
the same connectivity, at max|db| <= 1e-12 max|b| with no floor: sheared and translated Kuhn / cube grids (a full
Jacobian), a newest-vertex-bisection mesh, mirrored copies (every orientation reversed), each tensor kind, an
all-Neumann boundary, beta != 1 (the pow branch), Dirichlet and Neumann faces on one mesh, and a rank-local range
with own_begin > 0.  Whenever boundary data are present the force is also compared alone, so that the penalty
entries (O(sigma / h)) do not set the scale for the volume part.  Preconditions: tests/test_rhs_cases.py."""
import numpy as np
import pytest

import oracle as O
import rhs_cases as R

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

CONST_TENSOR = (2.0, 0.5, 1.0)
FORCE = (0.3, 1.5, 2.0, -1.0)             # sinusoid c, b, kx, ky: the run-time-rule template
G_D = (1.0, 0.5, 1.3, 0.7)
KAPPA = (1.5, 0.6, 2.2, -1.7)             # sinusoid kappa, b != 0
G_N = (2.0, 0.4, 0.9)                     # cos product c, kx, ky


def _torch():
    import torch
    return torch


def _sin(mod, p):
    if mod is H:
        return H.scalar_fn(H.FN_SINUSOID, p[0], b=p[1], kx=p[2], ky=p[3], order=3)
    return O.scalar(O.FN_SINUSOID, p[0], p[1], p[2], p[3], order=3)


def _g_n(mod):
    if mod is H:
        return H.scalar_fn(H.FN_COS_PRODUCT, G_N[0], kx=G_N[1], ky=G_N[2], order=2)
    return O.scalar(O.FN_COS_PRODUCT, G_N[0], 0.0, G_N[1], G_N[2], order=2)


def _sym_draw(ne, seed):
    """an SPD tensor per element, as test_products_pwc_fast_path draws it: rows a11, a12, a22 of [3][ne]"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 2.0, ne); c = rng.uniform(0.5, 2.0, ne); b = rng.uniform(-0.3, 0.3, ne)
    return np.stack([a, b, c], 0)


def _tensors(kind, ne, ids=None, oids=None):
    """(device tensor, oracle tensor); per-element data drawn in global order: the device takes [ids] (a view's
    global ids, ghosts included), the oracle [oids] (its elements' global ids)"""
    torch = _torch()
    ids = np.arange(ne) if ids is None else ids
    oids = np.arange(ne) if oids is None else oids
    if kind == "const":
        return H.tensor_fn(c=CONST_TENSOR), O.tensor(c=CONST_TENSOR)
    if kind == "iso":
        T = np.random.default_rng(3).uniform(0.5, 2.0, ne)
        return (H.tensor_fn(H.TENSOR_ISO_PER_ELEM, per_elem=torch.from_numpy(np.ascontiguousarray(T[ids])).cuda()),
                O.tensor(O.TENSOR_ISO_PER_ELEM, per_elem=np.ascontiguousarray(T[oids])))
    assert kind == "sym"
    S = _sym_draw(ne, 11)
    return (H.tensor_fn(H.TENSOR_SYM_PER_ELEM, per_elem=torch.from_numpy(np.ascontiguousarray(S[:, ids])).cuda()),
            O.tensor(O.TENSOR_SYM_PER_ELEM, per_elem=np.ascontiguousarray(S[:, oids].T)))


@pytest.mark.parametrize("name", R.GEOMETRY_MESHES)
def test_rhs_general_geometry_equals_oracle(ctx, name):
    """force (sinusoid, order 3), Dirichlet functional with sinusoid g_D and kappa and each tensor kind, all-Neumann
    boundary with a cos-product g_N; vertex-indexed and element-major geometry"""
    torch = _torch()
    et, coords, ev = R.geometry_mesh(name)
    og = O.Grid(et, coords, ev)
    ne = ev.shape[0]
    b_f = O.rhs_swipdg(og, force=_sin(O, FORCE))
    refs, kws = {}, {}
    for kind in ("const", "iso", "sym"):
        ht, ot = _tensors(kind, ne)
        refs[kind] = O.rhs_swipdg(og, force=_sin(O, FORCE), kappa=_sin(O, KAPPA), A=ot, dirichlet=_sin(O, G_D))
        kws[kind] = dict(kappa=_sin(H, KAPPA), tensor=ht, dirichlet=_sin(H, G_D))
    b_n = O.rhs_swipdg(og, force=_sin(O, FORCE), neumann=_g_n(O), prm=O.params(boundary=O.BOUNDARY_NEUMANN))
    assert np.max(np.abs(b_n - b_f)) > 0 and all(np.max(np.abs(r - b_f)) > 0 for r in refs.values())
    loc = H.Grid.from_connectivity(et, coords, ev).local()
    nloc = H.Grid.from_connectivity(et, coords, ev, boundary=H.BOUNDARY_ALL_NEUMANN).local()
    worst = {}
    for vx in (True, False):
        dm, ndm = H.DeviceMesh(loc, vertex_indexed=vx), H.DeviceMesh(nloc, vertex_indexed=vx)
        tag = "geometry %s vx=%d" % (name, vx)
        got = H.rhs(ctx, dm, force=_sin(H, FORCE), prm=H.params())
        R.check("%s: force" % tag, got.cpu().numpy(), b_f, worst)
        for kind in ("const", "iso", "sym"):
            got = H.rhs(ctx, dm, force=_sin(H, FORCE), prm=H.params(), **kws[kind])
            R.check("%s: dirichlet %s" % (tag, kind), got.cpu().numpy(), refs[kind], worst)
        got = H.rhs(ctx, ndm, force=_sin(H, FORCE), neumann=_g_n(H), prm=H.params())
        R.check("%s: neumann" % tag, got.cpu().numpy(), b_n, worst)
    torch.cuda.synchronize()
    for key, r in worst.items():
        print("rhs worst %s %.3g" % (key, r))


@pytest.mark.parametrize("name", ["kuhn_sheared", "cube_sheared"])
def test_rhs_beta_half_equals_oracle(ctx, name):
    """params(beta=0.5): hpow = pow(|F|, beta) in rhs2d_faces (beta = 1 takes |F| itself)"""
    et, coords, ev = R.geometry_mesh(name)
    og = O.Grid(et, coords, ev)
    ht, ot = _tensors("sym", ev.shape[0])
    ref = O.rhs_swipdg(og, kappa=_sin(O, KAPPA), A=ot, dirichlet=_sin(O, G_D), prm=O.params(beta=0.5))
    ref1 = O.rhs_swipdg(og, kappa=_sin(O, KAPPA), A=ot, dirichlet=_sin(O, G_D))
    assert R.ratio(ref1, ref) > 0.1                       # beta matters for the reference
    dm = H.DeviceMesh(H.Grid.from_connectivity(et, coords, ev).local())
    got = H.rhs(ctx, dm, kappa=_sin(H, KAPPA), tensor=ht, dirichlet=_sin(H, G_D), prm=H.params(beta=0.5))
    R.check("beta=0.5 %s: dirichlet sym" % name, got.cpu().numpy(), ref)


@pytest.mark.parametrize("name", R.GEOMETRY_MESHES)
def test_rhs_mixed_boundaries_equal_oracle(ctx, name):
    """Dirichlet and Neumann faces on one mesh.  The oracle's boundary kind is global, so a seeded subset of the
    boundary elements (with a two-face corner element where the mesh has one) gets all its boundary faces marked
    Neumann; the reference is b_force + (marked ? b_N : b_D) from three oracle calls."""
    et, coords, ev = R.geometry_mesh(name)
    og = O.Grid(et, coords, ev)
    ne, nb = ev.shape[0], og.nb
    ht, ot = _tensors("sym", ne)
    b_f = O.rhs_swipdg(og, force=_sin(O, FORCE))
    b_d = O.rhs_swipdg(og, kappa=_sin(O, KAPPA), A=ot, dirichlet=_sin(O, G_D))
    b_n = O.rhs_swipdg(og, neumann=_g_n(O), prm=O.params(boundary=O.BOUNDARY_NEUMANN))
    loc = H.Grid.from_connectivity(et, coords, ev).local()
    marked = R.mark_elements(loc.neighbors, 41)
    nbnd = (loc.neighbors < 0).sum(axis=0)
    assert marked.any() and np.any((nbnd > 0) & ~marked)
    assert np.any(nbnd[marked] > 1) or not R.has_corner(loc.neighbors)
    R.set_boundary(loc, marked, H.NBR_NEUMANN)
    ref = R.compose(nb, b_f, b_d, b_n, marked)
    ref_b = R.compose(nb, 0.0 * b_f, b_d, b_n, marked)
    for vx in (True, False):
        dm = H.DeviceMesh(loc, vertex_indexed=vx)
        kw = dict(kappa=_sin(H, KAPPA), tensor=ht, dirichlet=_sin(H, G_D), neumann=_g_n(H), prm=H.params())
        R.check("mixed %s vx=%d: force" % (name, vx), H.rhs(ctx, dm, force=_sin(H, FORCE), prm=H.params()).cpu().numpy(), b_f)
        R.check("mixed %s vx=%d: boundary" % (name, vx), H.rhs(ctx, dm, **kw).cpu().numpy(), ref_b)
        R.check("mixed %s vx=%d: force+boundary" % (name, vx),
                H.rhs(ctx, dm, force=_sin(H, FORCE), **kw).cpu().numpy(), ref)
        # the Neumann rows alone: the penalty entries of the Dirichlet rows do not set their scale
        rows = np.repeat(marked, nb)
        R.check("mixed %s vx=%d: neumann rows" % (name, vx), H.rhs(ctx, dm, **kw).cpu().numpy()[rows], ref_b[rows])


@pytest.mark.parametrize("et", [H.SIMPLEX, H.CUBE])
def test_rhs_rank_local_range(ctx, et):
    """grid.local(s, s + 1) of a middle subdomain of a ragged 3 x 2 block grid: own_begin > 0, ghosts on both
    sides, per-element force, kappa and symmetric tensor drawn in global order and passed as [loc.global_id];
    the output is indexed by k = e - own_begin.  Equal to the full mesh's slice bit for bit (no cos force: no
    wave-uniform tier can differ) and to the oracle's rows at the tolerance."""
    torch = _torch()
    grid = R.block_grid(et)
    og, ei = R.oracle_elem_index(grid, et)
    ne, nb = grid.ne, grid.nb
    rng = np.random.default_rng(23)
    fel, kel = rng.uniform(-1.0, 1.0, ne), rng.uniform(0.5, 2.0, ne)
    pe = lambda v: O.scalar(O.FN_PER_ELEM, per_elem=np.ascontiguousarray(v[ei]))
    _, ot = _tensors("sym", ne, oids=ei)
    ref_f = O.rhs_swipdg(og, force=pe(fel), elem_index=ei)
    ref = O.rhs_swipdg(og, force=pe(fel), kappa=pe(kel), A=ot, dirichlet=_sin(O, G_D), elem_index=ei)

    def run(loc):
        ids = loc.global_id
        ht, _ = _tensors("sym", ne, ids=ids)
        dev = lambda v: H.scalar_fn(H.FN_PER_ELEM, per_elem=torch.from_numpy(np.ascontiguousarray(v[ids])).cuda())
        dm = H.DeviceMesh(loc)
        only = H.rhs(ctx, dm, force=dev(fel), prm=H.params())
        full = H.rhs(ctx, dm, force=dev(fel), kappa=dev(kel), tensor=ht, dirichlet=_sin(H, G_D), prm=H.params())
        torch.cuda.synchronize()
        return only.cpu().numpy(), full.cpu().numpy()

    g_only, g_full = run(grid.local())
    s = R.BLOCK_S
    loc = grid.local(s, s + 1)
    a, b = grid.subdomain_range(s, s + 1)
    assert loc.own_begin > 0 and loc.own_end < loc.n_local
    assert np.all(loc.global_id[:loc.own_begin] < a) and np.all(loc.global_id[loc.own_end:] >= b)
    l_only, l_full = run(loc)
    assert l_full.shape == ((b - a) * nb,)
    assert np.array_equal(l_only, g_only[a * nb:b * nb]) and np.array_equal(l_full, g_full[a * nb:b * nb])
    tag = "range %s s=%d" % (R.ET_NAME[et], s)
    R.check("%s: force" % tag, l_only, ref_f[a * nb:b * nb])
    R.check("%s: force+dirichlet" % tag, l_full, ref[a * nb:b * nb])
    R.check("%s: full mesh force" % tag, g_only, ref_f)
    R.check("%s: full mesh force+dirichlet" % tag, g_full, ref)
