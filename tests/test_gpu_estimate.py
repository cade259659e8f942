"""The ESV2007 a-posteriori estimator on the device (hdd_swipdg_estimate: oswald_vertex_kernel + esv2007_element_kernel)
against the reference's expectation table and against the numpy restatement tests/estimator_ref.py, which
tests/test_estimator_ref.py pins to that table.

Tolerances of the parity tests come from the restatement itself: it is evaluated in float64 and in np.longdouble, the
largest gap between the two over an output array, relative to the array's maximum, is what float64 rounding alone does
to that array; the device may be 64 times that away (another, equally valid operation order, fused multiply-adds), at
least 1e-14 of the maximum."""
import numpy as np
import pytest

import estimator_ref as R
import oracle as O
from mesh_tools import nvb_mesh
from test_estimator_ref import TABLE, rows_of
from test_oracle_pinning import sig3

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ARRAYS = ("nc", "r", "df", "t", "flux", "oswald", "sums")


def _torch():
    import torch
    return torch


class Mesh:
    """host view, device mesh and estimator of a triangulation; ev [n, 3] / xy in the numbering the device sees"""

    def __init__(self, ctx, grid):
        self.grid = grid
        self.local = grid.local()
        self.dm = H.DeviceMesh(self.local)
        self.est = H.Estimator(ctx, self.local)
        ev, self.xy = self.local.vertices()
        self.ev = np.ascontiguousarray(ev.T)
        self.n = self.local.n_local

    @classmethod
    def of(cls, ctx, coords, ev):
        return cls(ctx, H.Grid.from_connectivity(H.SIMPLEX, coords, ev))


def distorted(seed=3):
    """nvb_mesh(4, 2) with the interior vertices moved by at most 0.2 of their shortest edge, the elements renumbered at
    random and every element's vertex list rotated: every twin face id and both orientations occur"""
    _, c, ev = nvb_mesh(4, 2)
    rng = np.random.default_rng(seed)
    hmin = np.full(c.shape[0], np.inf)
    for a, b in R.FV:
        le = np.hypot(*(c[ev[:, a]] - c[ev[:, b]]).T)
        np.minimum.at(hmin, ev[:, a], le)
        np.minimum.at(hmin, ev[:, b], le)
    inside = (np.abs(c) < 1.0 - 1e-12).all(1)
    phi, rad = rng.uniform(0, 2 * np.pi, c.shape[0]), rng.uniform(0, 0.2, c.shape[0]) * hmin
    c = c + np.where(inside, rad, 0.0)[:, None] * np.stack([np.cos(phi), np.sin(phi)], 1)
    ev = ev[rng.permutation(ev.shape[0])]
    rot = rng.integers(0, 3, ev.shape[0])
    ev = np.stack([np.roll(row, -k) for row, k in zip(ev, rot)]).astype(np.int32)
    return c, ev


def coefficients(case, n, seed=11):
    """(host kappa [n_comp, n], tensor (tuple or [3, n]), theta_mu, theta_bar, theta_hat) of a coefficient case"""
    rng = np.random.default_rng(seed)
    if case == "one":
        return np.ones((1, n)), (1.0, 0.0, 1.0), None, None, None
    if case == "contrast_sym":
        kap = 10.0 ** rng.uniform(-3, 3, (1, n))
        ten = np.stack([rng.uniform(1, 2, n), rng.uniform(-0.5, 0.5, n), rng.uniform(1, 2, n)])
        return kap, ten, None, None, None
    assert case == "two_thetas"
    kap = np.stack([np.ones(n), rng.uniform(0.5, 2.0, n)])
    return kap, (2.0, 0.5, 1.0), (1.0, 0.5), (0.7, 1.3), (1.2, 0.4)


def device_coefficients(kap, ten):
    torch = _torch()
    kappas = []
    for q in range(kap.shape[0]):
        if np.all(kap[q] == kap[q][0]):
            kappas.append(H.scalar_fn(H.FN_CONST, float(kap[q][0])))
        else:
            kappas.append(H.scalar_fn(H.FN_PER_ELEM, per_elem=torch.from_numpy(np.ascontiguousarray(kap[q])).cuda()))
    if isinstance(ten, tuple):
        return kappas, H.tensor_fn(H.TENSOR_CONST, ten)
    return kappas, H.tensor_fn(H.TENSOR_SYM_PER_ELEM, per_elem=torch.from_numpy(np.ascontiguousarray(ten)).cuda())


def reference(m, u, kap, ten, th, force=True):
    """the restatement in float64, and per output array the tolerance: max(64 * gap to longdouble, 1e-14) * maximum"""
    out = []
    for T in (np.float64, np.longdouble):
        out.append(R.estimate(m.xy, m.ev, u, kappa=kap, tensor=None if ten is None else np.asarray(ten), theta_mu=th[0],
                              theta_bar=th[1], theta_hat=th[2], force=R.esv2007_force(T) if force else None, dtype=T))
    r64, rld = out

    def arr(r):
        return dict(nc=r["local"][0], r=r["local"][1], df=r["local"][2], t=r["local"][3], flux=r["flux"], oswald=r["oswald"],
                    sums=r["sums"])
    a64, ald = arr(r64), arr(rld)
    tol, gaps = {}, {}
    for k in ARRAYS:
        top = float(np.abs(ald[k]).max())
        gaps[k] = float(np.abs(a64[k] - ald[k]).max()) / top if top > 0 else 0.0
        tol[k] = max(64 * gaps[k], 1e-14) * top
    # the four sums are compared one by one (they differ by orders of magnitude)
    gs = np.abs(a64["sums"] - ald["sums"]) / np.maximum(np.abs(ald["sums"]).astype(np.float64), 1e-300)
    tol["sums"] = np.maximum(64 * gs.astype(np.float64), 1e-14) * np.abs(a64["sums"])
    return a64, tol, gaps


def device(ctx, m, u, kap, ten, th, force=True, **want):
    kappas, tensor = device_coefficients(kap, ten)
    want = want or dict(local=True, flux=True, oswald=True)
    return H.estimate(ctx, m.est, m.dm, kappas, tensor, _torch().from_numpy(u).cuda(), force=H.esv2007_force() if force else None,
                      theta_mu=th[0], theta_bar=th[1], theta_hat=th[2], **want)


def got_arrays(e):
    loc = e.local.cpu().numpy()
    return dict(nc=loc[0], r=loc[1], df=loc[2], t=loc[3], flux=e.flux.cpu().numpy(), oswald=e.oswald.cpu().numpy(), sums=e.sums)


def check_parity(ctx, m, u, case, label):
    kap, ten, *th = coefficients(case, m.n)
    ref, tol, gaps = reference(m, u, kap, ten, th)
    got = got_arrays(device(ctx, m, u, kap, ten, th))
    report = []
    for k in ARRAYS:
        err = np.abs(got[k] - ref[k])
        report.append("%s %s: gap %.2e, err/max %.2e" % (label, k, gaps[k], float(err.max()) / max(float(np.abs(ref[k]).max()), 1e-300)))
    print("\n".join(report))
    for k in ARRAYS:
        assert np.all(np.abs(got[k] - ref[k]) <= tol[k]), (label, k, report)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes(ctx):
    _, c, ev = nvb_mesh(4, 2)
    return dict(nvb=Mesh.of(ctx, c, ev), distorted=Mesh.of(ctx, *distorted()))


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_table_from_device_solve_and_estimate(ctx, lvl):
    """assemble, solve and estimate on the device: all seven estimator rows of the reference's table, levels 0..3"""
    torch = _torch()
    et, c, ev = nvb_mesh(4, 2 + 2 * lvl)
    m = Mesh.of(ctx, c, ev)
    og = O.Grid(et, c, ev)
    dp = H.DevicePattern(m.local)
    kappas, tensor = [H.scalar_fn(H.FN_CONST, 1.0)], H.tensor_fn()
    vals = H.assemble(ctx, m.dm, dp, kappas, tensor)
    x, info = H.solve(ctx, dp, vals, torch.from_numpy(O.rhs_esv2007(og)).cuda(), dmesh=m.dm, rtol=1e-10)
    assert info.status == H.SOLVE_CONVERGED
    e = H.estimate(ctx, m.est, m.dm, kappas, tensor, x, force=H.esv2007_force())
    h1 = O.error_norms_esv2007(og, x.cpu().numpy())[1]
    rows = rows_of(e.sums, h1)
    assert abs(rows["eta"] - e.eta) <= 4 * EPS * e.eta and abs(rows["eta_alt"] - e.eta_alt) <= 4 * EPS * e.eta_alt
    print("level %d: %s" % (lvl, {k: "%.5e" % v for k, v in rows.items()}))
    for k, v in rows.items():
        assert sig3(v) == TABLE[k][lvl], (k, v)


@pytest.mark.parametrize("case", ["one", "contrast_sym", "two_thetas"])
@pytest.mark.parametrize("mesh", ["nvb", "distorted"])
def test_parity_with_the_restatement(ctx, meshes, mesh, case):
    """every output on a random vector (jumps and nonconformity O(1)), per element"""
    m = meshes[mesh]
    u = np.random.default_rng(7).standard_normal(3 * m.n)
    check_parity(ctx, m, u, case, "%s/%s" % (mesh, case))


def test_distorted_mesh_has_every_twin_and_orientation(meshes):
    m = meshes["distorted"]
    fi, nb = m.local.face_info, m.local.neighbors
    seen = set()
    for f in range(3):
        inner = nb[f] >= 0
        seen |= set(zip(((fi[inner] >> (4 * f)) & 7).tolist(), ((fi[inner] >> (4 * f + 3)) & 1).tolist(), [f] * int(inner.sum())))
    assert len({(t, f) for t, _, f in seen}) == 9 and {r for _, r, _ in seen} == {0, 1}


@pytest.mark.parametrize("nx,ny", [(1, 1), (8, 4), (11, 3), (16, 8), (43, 3), (14, 16), (15, 15), (5, 42)])
def test_size_edges(ctx, nx, ny):
    """2 nx ny = 2, 64, 66, 256, 258 elements (a wave, a workgroup, one more); 255, 256, 258 vertices"""
    m = Mesh(ctx, H.Grid.structured(H.SIMPLEX, nx, ny, (0.0, 0.0), (1.0, 0.75)))
    assert m.n == 2 * nx * ny and m.xy.shape[0] == (nx + 1) * (ny + 1)
    u = np.random.default_rng(nx * 100 + ny).standard_normal(3 * m.n)
    check_parity(ctx, m, u, "two_thetas", "%dx%d" % (nx, ny))


def _twin_sums(m, F):
    fi, nb = m.local.face_info, m.local.neighbors
    worst = 0.0
    for f in range(3):
        inner = np.nonzero(nb[f] >= 0)[0]
        twin = (fi[inner] >> (4 * f)) & 7
        worst = max(worst, float(np.abs(F[f, inner] + F[twin, nb[f, inner]]).max()))
    return worst


def test_flux_is_conservative(ctx, meshes):
    """F_T,e + F_T',e' = 0 on every interior face, for any coefficients"""
    m = meshes["distorted"]
    u = np.random.default_rng(9).standard_normal(3 * m.n)
    for case in ("two_thetas", "contrast_sym"):
        kap, ten, *th = coefficients(case, m.n)
        _, tol, gaps = reference(m, u, kap, ten, th)
        F = device(ctx, m, u, kap, ten, th).flux.cpu().numpy()
        worst = _twin_sums(m, F)
        print("%s: flux gap %.2e, tol %.2e, twin sum %.2e, max |F| %.2e" % (case, gaps["flux"], tol["flux"], worst, np.abs(F).max()))
        assert worst <= tol["flux"], case


def test_flux_sums_are_the_row_sums_of_the_operator(ctx, meshes):
    """sum_e F_T,e = the three summed rows of element T of A(theta_mu) u (the volume and symmetry terms vanish against a
    constant test function).  The scheme takes its weights from the tensor alone and its penalty from kappa- kappa+
    (LocalEvaluation::SWIPDG), the reconstruction both from K = kappa A: the two agree, and the identity holds, for
    kappa = 1 -- here with theta_mu = 0.7 and a per-element symmetric tensor."""
    m = meshes["distorted"]
    u = np.random.default_rng(9).standard_normal(3 * m.n)
    kap, ten = np.ones((1, m.n)), coefficients("contrast_sym", m.n)[1]
    th = ((0.7,), None, None)
    _, tol, gaps = reference(m, u, kap, ten, th)
    F = device(ctx, m, u, kap, ten, th).flux.cpu().numpy()
    kappas, tensor = device_coefficients(kap, ten)
    dp = H.DevicePattern(m.local)
    vals = H.assemble(ctx, m.dm, dp, kappas, tensor)
    Au = H.apply(ctx, dp, vals, _torch().from_numpy(u).cuda(), theta=th[0], dmesh=m.dm).cpu().numpy()
    rows = float(np.abs(F.sum(0) - Au.reshape(-1, 3).sum(1)).max())
    print("flux gap %.2e, tol %.2e, row sums %.2e, twin sum %.2e, max |F| %.2e" % (gaps["flux"], tol["flux"], rows, _twin_sums(m, F), np.abs(F).max()))
    assert rows <= tol["flux"]


def test_flux_of_the_solution_balances_the_right_hand_side(ctx):
    """for the solved ESV2007 vector sum_e F_T,e = the three summed right-hand side entries of T, to the solver's
    residual: |sum of three entries of r| <= sqrt(3) ||r||_2; the factor 2 covers the distance of the recurrence
    residual the solver reports from the true one and the rounding of F"""
    torch = _torch()
    et, c, ev = nvb_mesh(4, 4)
    m = Mesh.of(ctx, c, ev)
    b = O.rhs_esv2007(O.Grid(et, c, ev))
    dp = H.DevicePattern(m.local)
    kappas, tensor = [H.scalar_fn(H.FN_CONST, 1.0)], H.tensor_fn()
    vals = H.assemble(ctx, m.dm, dp, kappas, tensor)
    x, info = H.solve(ctx, dp, vals, torch.from_numpy(b).cuda(), dmesh=m.dm, rtol=1e-10)
    assert info.status == H.SOLVE_CONVERGED
    e = H.estimate(ctx, m.est, m.dm, kappas, tensor, x, force=H.esv2007_force(), flux=True)
    miss = float(np.abs(e.flux.cpu().numpy().sum(0) - b.reshape(-1, 3).sum(1)).max())
    print("flux vs rhs %.2e, solver residual %.2e" % (miss, info.residual))
    assert miss <= 2 * np.sqrt(3.0) * info.residual


def test_oswald_of_a_continuous_vector(ctx, meshes):
    """a vector that is continuous and zero on the boundary comes back within 2 ulp per vertex, its nonconformity is at
    most (4 ulp)^2 of its own energy per element; boundary vertices are exactly 0 for any vector"""
    m = meshes["distorted"]
    on_bnd = (np.abs(m.xy) > 1.0 - 1e-12).any(1)
    w = np.where(on_bnd, 0.0, np.cos(m.xy[:, 0]) + m.xy[:, 1] ** 2 + 3.0)
    u = np.ascontiguousarray(w[m.ev].reshape(-1))
    kap, ten, *th = coefficients("contrast_sym", m.n)
    e = device(ctx, m, u, kap, ten, th)
    osw = e.oswald.cpu().numpy()
    assert np.all(np.abs(osw - w) <= 2 * np.spacing(np.abs(w)))
    assert np.array_equal(osw[on_bnd], np.zeros(int(on_bnd.sum())))
    ref = R.estimate(m.xy, m.ev, u, kappa=kap, tensor=ten)
    K = kap[0] * ten
    g = (u.reshape(-1, 3)[:, :, None] * _grad_lambda(m)).sum(1)
    energy = ref["area"] * (K[0] * g[:, 0] ** 2 + 2 * K[1] * g[:, 0] * g[:, 1] + K[2] * g[:, 1] ** 2)
    assert np.all(e.local[0].cpu().numpy() <= (4 * EPS) ** 2 * energy.max())
    rnd = np.random.default_rng(2).standard_normal(3 * m.n)
    e = device(ctx, m, rnd, kap, ten, th)
    assert np.array_equal(e.oswald.cpu().numpy()[on_bnd], np.zeros(int(on_bnd.sum())))
    assert np.abs(e.oswald.cpu().numpy()[~on_bnd]).min() > 0


def _grad_lambda(m):
    p = m.xy[m.ev]
    det = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])
    return np.stack([np.stack([p[:, 1, 1] - p[:, 2, 1], p[:, 2, 0] - p[:, 1, 0]], 1),
                     np.stack([p[:, 2, 1] - p[:, 0, 1], p[:, 0, 0] - p[:, 2, 0]], 1),
                     np.stack([p[:, 0, 1] - p[:, 1, 1], p[:, 1, 0] - p[:, 0, 0]], 1)], 1) / det[:, None, None]


def test_deterministic_and_independent_of_the_outputs_asked_for(ctx):
    """two calls are bit-identical in every output; the local arrays and the sums do not depend on which of d_local /
    d_flux / d_oswald are NULL; sums[k] is the documented fixed-order sum of the local array"""
    m = Mesh(ctx, H.Grid.structured(H.SIMPLEX, 23, 17, (-1.0, -1.0), (1.0, 1.0)))       # 782 elements: 4 workgroups
    u = np.random.default_rng(4).standard_normal(3 * m.n)
    kap, ten, *th = coefficients("contrast_sym", m.n)
    a = got_arrays(device(ctx, m, u, kap, ten, th))
    b = got_arrays(device(ctx, m, u, kap, ten, th))
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), k
    assert H.last_estimate_kernels() == "oswald_vertex_kernel + esv2007_element_kernel<beta1, cos_product>"
    for want in (dict(local=True), dict(local=True, flux=True), dict(local=True, oswald=True)):
        e = device(ctx, m, u, kap, ten, th, **want)
        loc = e.local.cpu().numpy()
        assert np.array_equal(loc, np.stack([a["nc"], a["r"], a["df"], a["t"]])), want
        assert np.array_equal(e.sums, a["sums"]), want
    none = device(ctx, m, u, kap, ten, th, local=False)
    assert none.local is None and none.flux is None and none.oswald is None and np.array_equal(none.sums, a["sums"])
    for k, name in enumerate(("nc", "r", "df", "t")):
        assert a["sums"][k] == R.fixed_order_sum(a[name]), name
    # estimate_local: the reference's two local indicators
    e = device(ctx, m, u, kap, ten, th)
    loc = e.estimate_local("eta_ESV2007").cpu().numpy()
    assert abs(loc.sum() - 1.0) <= 1e-12
    alt = e.estimate_local("eta_ESV2007_alt").cpu().numpy()
    assert np.allclose(alt, 3 * (a["nc"] + a["r"] + a["df"]) / e.eta_alt ** 2, rtol=1e-14, atol=0)


@pytest.mark.parametrize("force", [True, False])
def test_residual_star(ctx, meshes, force):
    """eta_R_ESV2007_*: div t_h in place of the element mean of f, with the ESV2007 force and without one (f = 0)"""
    m = meshes["distorted"]
    u = np.random.default_rng(12).standard_normal(3 * m.n)
    kap, ten, *th = coefficients("two_thetas", m.n)
    est = H.Estimator(ctx, m.local)
    est.set_residual_star(True)
    kappas, tensor = device_coefficients(kap, ten)
    e = H.estimate(ctx, est, m.dm, kappas, tensor, _torch().from_numpy(u).cuda(), force=H.esv2007_force() if force else None,
                   theta_mu=th[0], theta_bar=th[1], theta_hat=th[2], local=True)
    out = [R.estimate(m.xy, m.ev, u, kappa=kap, tensor=np.asarray(ten), theta_mu=th[0], theta_bar=th[1], theta_hat=th[2],
                      force=R.esv2007_force(T) if force else None, residual_star=True, dtype=T) for T in (np.float64, np.longdouble)]
    got = e.local.cpu().numpy()
    for k in range(4):
        top = float(np.abs(out[1]["local"][k]).max())
        gap = float(np.abs(out[0]["local"][k] - out[1]["local"][k]).max()) / top
        assert np.abs(got[k] - out[0]["local"][k]).max() <= max(64 * gap, 1e-14) * top, (k, gap)
    plain = device(ctx, m, u, kap, ten, th, force=force)          # the estimator of the fixture is untouched
    assert np.array_equal(plain.local[0].cpu().numpy(), got[0]) and np.array_equal(plain.local[2].cpu().numpy(), got[2])
    assert not np.array_equal(plain.local[1].cpu().numpy(), got[1])


def test_other_kernel_instantiations(ctx, meshes):
    """no force (eta_R = 0 exactly), and beta != 1 (the pow path) against the restatement"""
    m = meshes["distorted"]
    u = np.random.default_rng(8).standard_normal(3 * m.n)
    kap, ten, *th = coefficients("two_thetas", m.n)
    e = device(ctx, m, u, kap, ten, th, force=False)
    assert H.last_estimate_kernels().endswith("<beta1, no_force>")
    assert not e.local[1].any().item() and e.sums[1] == 0.0
    kappas, tensor = device_coefficients(kap, ten)
    prm = H.params(beta=1.5)
    e = H.estimate(ctx, m.est, m.dm, kappas, tensor, _torch().from_numpy(u).cuda(), force=H.esv2007_force(), theta_mu=th[0],
                   theta_bar=th[1], theta_hat=th[2], prm=prm, flux=True, local=True)
    assert H.last_estimate_kernels().endswith("<pow, cos_product>")
    out = [R.estimate(m.xy, m.ev, u, kappa=kap, tensor=np.asarray(ten), theta_mu=th[0], theta_bar=th[1], theta_hat=th[2],
                      force=R.esv2007_force(T), beta=1.5, dtype=T) for T in (np.float64, np.longdouble)]
    for key, got in (("flux", e.flux.cpu().numpy()), ("local", e.local.cpu().numpy())):
        for k in range(got.shape[0]):
            top = float(np.abs(out[1][key][k]).max())
            gap = float(np.abs(out[0][key][k] - out[1][key][k]).max()) / top
            assert np.abs(got[k] - out[0][key][k]).max() <= max(64 * gap, 1e-14) * top, (key, k, gap)
