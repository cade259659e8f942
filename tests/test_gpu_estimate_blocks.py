"""The OS2014 localized estimator on the device (hdd_block_swipdg_estimate: oswald_vertex_kernel +
esv2007_element_kernel<.., block> + block_segment_kernel + block_total_kernel) against hdd_swipdg_estimate (bit for
bit where the two compute the same thing), against the numpy restatement tests/estimator_os2014_ref.py, which
tests/test_estimator_os2014_ref.py pins to the reference's table, and against that table itself.

Meshes: those of tests/test_gpu_estimate.py (the 128-element mesh, its distorted copy, Kuhn grids of 258 and 544
elements) and a Kuhn grid of 1296 elements, the smallest here that holds segments of 1, 255, 256, 257 and 513 elements
in one partition.  Tolerances as there: the restatement is evaluated in float64 and in np.longdouble, the
device may be 64 times their gap away, at least 1e-14 of the array's maximum."""
import numpy as np
import pytest

import estimator_os2014_ref as B
import estimator_ref as R
import oracle as O
from mesh_tools import nvb_mesh
from test_estimator_os2014_ref import PARTITIONINGS, TABLE, rows_of
from test_gpu_estimate import Mesh, _torch, coefficients, device, device_coefficients, distorted
from test_oracle_pinning import sig3

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

BLOCK_KERNELS = ("oswald_vertex_kernel + esv2007_element_kernel<beta1, cos_product, block> + block_segment_kernel + "
                 "block_total_kernel")


def thetas(case):
    """(mu, bar, hat, min, max) of a coefficient case: two_thetas has five distinct roles"""
    th = list(coefficients(case, 1)[2:])
    return th + ([(0.5, 0.25), (2.0, 3.0)] if case == "two_thetas" else [None, None])


def device_blocks(ctx, m, u, kap, ten, th, force=True, est=None, **want):
    kappas, tensor = device_coefficients(kap, ten)
    want = want or dict(local=True, flux=True, oswald=True)
    return H.estimate_blocks(ctx, est or m.est, m.dm, kappas, tensor, _torch().from_numpy(u).cuda(),
                             force=H.esv2007_force() if force else None, theta_mu=th[0], theta_bar=th[1], theta_hat=th[2],
                             theta_min=th[3], theta_max=th[4], **want)


def reference(m, u, kap, ten, th, bounds, force=True, residual_star=False):
    """the restatement in float64, and per array the tolerance max(64 * gap to longdouble, 1e-14) * maximum"""
    out = [B.estimate_blocks(m.xy, m.ev, u, bounds, kappa=kap, tensor=np.asarray(ten), theta_mu=th[0], theta_bar=th[1],
                             theta_hat=th[2], theta_min=th[3], theta_max=th[4], force=R.esv2007_force(T) if force else None,
                             residual_star=residual_star, dtype=T) for T in (np.float64, np.longdouble)]

    def arr(r):
        return dict(r=r["local"][1], m=r["local"][3], N=r["segments"][0], R=r["segments"][1], D=r["segments"][2],
                    ind=r["segments"][3], sums=r["sums"])
    a64, ald = arr(out[0]), arr(out[1])
    tol, gaps = {}, {}
    for k in a64:
        top = float(np.abs(ald[k]).max())
        gaps[k] = float(np.abs(a64[k] - ald[k]).max()) / top if top > 0 else 0.0
        tol[k] = max(64 * gaps[k], 1e-14) * top
    # the four sums are compared one by one (they differ by orders of magnitude)
    gs = (np.abs(a64["sums"] - ald["sums"]) / np.maximum(np.abs(ald["sums"]), 1e-300)).astype(np.float64)
    tol["sums"] = np.maximum(64 * gs, 1e-14) * np.abs(a64["sums"])
    return a64, tol, gaps


def got_arrays(e):
    loc, seg = e.local.cpu().numpy(), e.segments.cpu().numpy()
    return dict(r=loc[1], m=loc[3], N=seg[0], R=seg[1], D=seg[2], ind=seg[3], sums=e.sums)


def check_against_the_restatement(got, ref, tol, gaps, label):
    report = ["%s %s: gap %.2e, err/max %.2e" % (label, k, gaps[k], float(np.abs(got[k] - ref[k]).max()) /
                                                   max(float(np.abs(ref[k]).max()), 1e-300)) for k in ref]
    print("\n".join(report))
    for k in ref:
        assert np.all(np.abs(got[k] - ref[k]) <= tol[k]), (label, k, report)


@pytest.fixture(scope="module")
def meshes(ctx):
    _, c, ev = nvb_mesh(4, 2)
    kuhn = lambda nx, ny: Mesh(ctx, H.Grid.structured(H.SIMPLEX, nx, ny, (0.0, 0.0), (1.0, 0.75)))
    return dict(nvb=Mesh.of(ctx, c, ev), distorted=Mesh.of(ctx, *distorted()), kuhn258=kuhn(43, 3), kuhn544=kuhn(16, 17),
                kuhn1296=kuhn(27, 24))


def _bounds(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# mesh, segment sizes: S = 1; one element, a chunk less one, a chunk, a chunk and one, two chunks and one in one partition;
# 272 segments of two (the strided total wraps at 256)
CUTS = [("nvb", (128,)), ("nvb", (1, 2, 37, 88)), ("distorted", (128,)), ("distorted", (5, 1, 64, 58)),
        ("kuhn258", (258,)), ("kuhn258", (1, 255, 2)), ("kuhn258", (257, 1)), ("kuhn544", (544,)),
        ("kuhn544", (2,) * 272), ("kuhn1296", (1, 255, 256, 257, 513, 14)), ("kuhn1296", (1296,))]


@pytest.mark.parametrize("case", ["one", "contrast_sym", "two_thetas"])
@pytest.mark.parametrize("mesh,sizes", CUTS, ids=["%s-%dx%d" % (m, len(s), max(s)) for m, s in CUTS])
def test_blocks_against_the_esv_call_and_the_restatement(ctx, meshes, mesh, sizes, case):
    m = meshes[mesh]
    bounds = _bounds(sizes)
    assert bounds[-1] == m.n
    u = np.random.default_rng(7).standard_normal(3 * m.n)
    kap, ten = coefficients(case, m.n)[:2]
    th = thetas(case)
    m.est.set_segments(bounds)
    e = device_blocks(ctx, m, u, kap, ten, th)
    assert H.last_estimate_kernels() == BLOCK_KERNELS
    esv = device(ctx, m, u, kap, ten, th[:3])
    loc, seg = e.local.cpu().numpy(), e.segments.cpu().numpy()
    esv_loc = esv.local.cpu().numpy()
    # the shared device code: bit for bit
    assert np.array_equal(loc[0], esv_loc[0]) and np.array_equal(loc[2], esv_loc[2])
    assert np.array_equal(e.flux.cpu().numpy(), esv.flux.cpu().numpy())
    assert np.array_equal(e.oswald.cpu().numpy(), esv.oswald.cpu().numpy())
    # the segment sums: the fixed-order sum of the slice, the totals the strided sum over the segments
    for row in (0, 2):
        want = np.array([R.fixed_order_sum(loc[row, a:b]) for a, b in zip(bounds[:-1], bounds[1:])])
        assert np.array_equal(seg[row], want), row
        assert e.sums[row] == B.strided_total(seg[row]), row
    assert e.sums[1] == B.strided_total(seg[1])
    if len(sizes) == 1:
        assert seg[0, 0] == esv.sums[0] and seg[2, 0] == esv.sums[2]
        assert e.sums[0] == esv.sums[0] and e.sums[2] == esv.sums[2]
    # r_T, m_T, R_s, the indicators and the four sums
    ref, tol, gaps = reference(m, u, kap, ten, th, bounds)
    check_against_the_restatement(got_arrays(e), ref, tol, gaps, "%s/%s/%s" % (mesh, len(sizes), case))
    f = B.factors(*[np.ones(kap.shape[0]) if t is None else t for t in th[:3]])
    assert np.allclose([e.alpha_bar, e.gamma_bar, e.gamma_tilde], [f[0], f[1], f[4]], rtol=4e-16, atol=0)
    assert np.array_equal(e.estimate_local().cpu().numpy(), seg[3])
    assert abs(e.eta - np.sqrt(e.sums[3])) == 0.0


def test_a_segment_does_not_depend_on_the_other_cuts(ctx, meshes):
    m = meshes["kuhn544"]
    u = np.random.default_rng(3).standard_normal(3 * m.n)
    kap, ten = coefficients("two_thetas", m.n)[:2]
    th = thetas("two_thetas")
    out = []
    for bounds, s in (([0, 100, 400, 544], 1), ([0, 1, 37, 100, 400, 401, 544], 3), ([0, 100, 400, 543, 544], 1)):
        m.est.set_segments(bounds)
        out.append(device_blocks(ctx, m, u, kap, ten, th, local=True).segments.cpu().numpy()[:3, s])
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    assert np.all(out[0] > 0)


def test_deterministic_and_independent_of_the_outputs_asked_for(ctx, meshes):
    m = meshes["kuhn1296"]
    u = np.random.default_rng(4).standard_normal(3 * m.n)
    kap, ten = coefficients("contrast_sym", m.n)[:2]
    th = thetas("contrast_sym")
    m.est.set_segments(_bounds((1, 255, 256, 257, 513, 14)))
    a = device_blocks(ctx, m, u, kap, ten, th)
    b = device_blocks(ctx, m, u, kap, ten, th)
    for k in ("local", "flux", "oswald", "segments"):
        assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), k
    assert np.array_equal(a.sums, b.sums)
    for want in (dict(local=True), dict(local=True, flux=True), dict(oswald=True), dict(local=False)):
        e = device_blocks(ctx, m, u, kap, ten, th, **want)
        assert np.array_equal(e.segments.cpu().numpy(), a.segments.cpu().numpy()), want
        assert np.array_equal(e.sums, a.sums), want
        if want.get("local"):
            assert np.array_equal(e.local.cpu().numpy(), a.local.cpu().numpy()), want
    none = device_blocks(ctx, m, u, kap, ten, th, local=False)
    assert none.local is None and none.flux is None and none.oswald is None
    # the ESV call on the same estimator is untouched by the segments
    esv = device(ctx, m, u, kap, ten, th[:3])
    assert H.last_estimate_kernels() == "oswald_vertex_kernel + esv2007_element_kernel<beta1, cos_product>"
    assert np.array_equal(esv.local[0].cpu().numpy(), a.local[0].cpu().numpy())


@pytest.mark.parametrize("force", [True, False])
def test_residual_star(ctx, meshes, force):
    """eta_R_OS2014_*: div t_h in place of the element mean of f, with the ESV2007 force and without one (f = 0)"""
    m = meshes["distorted"]
    bounds = _bounds((5, 1, 64, 58))
    u = np.random.default_rng(12).standard_normal(3 * m.n)
    kap, ten = coefficients("two_thetas", m.n)[:2]
    th = thetas("two_thetas")
    est = H.Estimator(ctx, m.local)
    est.set_residual_star(True)
    est.set_segments(bounds)
    e = device_blocks(ctx, m, u, kap, ten, th, force=force, est=est)
    ref, tol, gaps = reference(m, u, kap, ten, th, bounds, force=force, residual_star=True)
    check_against_the_restatement(got_arrays(e), ref, tol, gaps, "star/%s" % force)
    m.est.set_segments(bounds)
    plain = device_blocks(ctx, m, u, kap, ten, th, force=force)
    assert np.array_equal(plain.segments[0].cpu().numpy(), e.segments[0].cpu().numpy())
    assert not np.array_equal(plain.segments[1].cpu().numpy(), e.segments[1].cpu().numpy())
    if not force:
        assert not plain.local[1].any().item() and plain.sums[1] == 0.0


def test_beta_other_than_one(ctx, meshes):
    m = meshes["distorted"]
    bounds = _bounds((5, 1, 64, 58))
    u = np.random.default_rng(8).standard_normal(3 * m.n)
    kap, ten = coefficients("two_thetas", m.n)[:2]
    th = thetas("two_thetas")
    kappas, tensor = device_coefficients(kap, ten)
    m.est.set_segments(bounds)
    args = dict(force=H.esv2007_force(), theta_mu=th[0], theta_bar=th[1], theta_hat=th[2], prm=H.params(beta=1.5), local=True)
    e = H.estimate_blocks(ctx, m.est, m.dm, kappas, tensor, _torch().from_numpy(u).cuda(), theta_min=th[3], theta_max=th[4],
                          **args)
    assert "<pow, cos_product, block>" in H.last_estimate_kernels()
    esv = H.estimate(ctx, m.est, m.dm, kappas, tensor, _torch().from_numpy(u).cuda(), **args)
    assert np.array_equal(e.local[2].cpu().numpy(), esv.local[2].cpu().numpy())


def test_segments_must_be_set(ctx, meshes):
    m = meshes["nvb"]
    m.est.set_segments()
    u = np.zeros(3 * m.n)
    kap, ten = coefficients("one", m.n)[:2]
    with pytest.raises(H.HddError):
        device_blocks(ctx, m, u, kap, ten, thetas("one"))


def test_a_vanishing_estimate_has_vanishing_indicators(ctx, meshes):
    """u_h = 0 without a force: eta = 0, and the indicators are 0, not 0 / 0"""
    m = meshes["kuhn544"]
    m.est.set_segments(_bounds((2,) * 272))
    kap, ten = coefficients("contrast_sym", m.n)[:2]
    e = device_blocks(ctx, m, np.zeros(3 * m.n), kap, ten, thetas("contrast_sym"), force=False)
    assert np.array_equal(e.sums, np.zeros(4)) and e.eta == 0.0
    assert np.array_equal(e.segments.cpu().numpy(), np.zeros((4, 272)))


@pytest.mark.parametrize("lvl", [0, 1, 2, 3])
def test_table_from_device_solve_and_estimate(ctx, lvl):
    """assemble, solve and estimate on the device: the five rows of the reference's table for the four partitionings
    (P x P centroid boxes; the solution renumbered subdomain-major on the device), levels 0..3"""
    torch = _torch()
    et, c, ev = nvb_mesh(4, 2 + 2 * lvl)
    m = Mesh.of(ctx, c, ev)
    og = O.Grid(et, c, ev)
    dp = H.DevicePattern(m.local)
    kappas, tensor = [H.scalar_fn(H.FN_CONST, 1.0)], H.tensor_fn()
    vals = H.assemble(ctx, m.dm, dp, kappas, tensor)
    x, info = H.solve(ctx, dp, vals, torch.from_numpy(O.rhs_esv2007(og)).cuda(), dmesh=m.dm, rtol=1e-10)
    assert info.status == H.SOLVE_CONVERGED
    h1 = O.error_norms_esv2007(og, x.cpu().numpy())[1]
    for name, P in sorted(PARTITIONINGS.items()):
        perm, bounds = B.box_partition(c, ev, P, P)
        mp = Mesh.of(ctx, c, np.asarray(ev)[perm])
        assert np.array_equal(mp.ev, m.ev[perm])
        mp.est.set_segments(bounds)
        xp = x.reshape(-1, 3)[torch.from_numpy(perm).cuda()].reshape(-1).contiguous()
        e = H.estimate_blocks(ctx, mp.est, mp.dm, kappas, tensor, xp, force=H.esv2007_force())
        rows = rows_of(e.sums, h1)
        print("level %d %s: %s" % (lvl, name, {k: "%.5e" % v for k, v in rows.items()}))
        for k, v in rows.items():
            assert sig3(v) == TABLE[name][k][lvl], (name, k, v)
        ind = e.estimate_local().cpu().numpy()
        assert ind.shape == (P * P,) and np.all(ind > 0)
        assert abs(ind.sum() - 3.0 * e.sums[:3].sum() / e.sums[3]) <= 1e-12 * ind.sum()
