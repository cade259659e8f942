"""The entry points of the OS2014 localized estimator (hdd_estimator_set_segments / _segment_diameters /
_blocks_workspace, hdd_os2014_factors, hdd_block_swipdg_estimate): declared, exported, bound by the Python front-end,
additive to ABI 8; every argument check comes before the first device call, so they answer HDD_ERR_INVALID (1) here,
without a GPU, on a host-only estimator; and the host tables: the segment diameters (convex hull) against the
reference's brute-force maximum over all vertex pairs."""
import ctypes as C

import numpy as np
import pytest

import estimator_os2014_ref as B
import hdd_amd as H
from mesh_tools import nvb_mesh
from test_abi_estimate import _Operands
from test_gpu_estimate import distorted

NAMES = ("hdd_estimator_set_segments", "hdd_estimator_segment_diameters", "hdd_estimator_blocks_workspace",
         "hdd_os2014_factors", "hdd_block_swipdg_estimate")
WHO = b"hdd_block_swipdg_estimate:"
INVALID = 1


def _msg():
    return H.lib().hdd_last_error(None)


def test_symbols_exported_and_bound():
    L = H.lib()
    declared = H.declared_symbols()
    for n in NAMES:
        assert n in declared, n
        assert getattr(L, n).argtypes is not None, n
    assert len(L.hdd_block_swipdg_estimate.argtypes) == 22
    assert len(L.hdd_swipdg_estimate.argtypes) == 19
    assert L.hdd_estimator_blocks_workspace.restype is C.c_int64
    assert callable(H.estimate_blocks) and callable(H.os2014_factors) and callable(H.BlockEstimate)
    assert callable(H.Estimator.set_segments) and callable(H.Estimator.segment_diameters)
    assert L.hdd_abi_version() == 8        # additive: the ABI version stays


def test_workspaces():
    """hdd_estimator_workspace does not depend on the segments; the block workspace holds the Oswald values, four
    partials per chunk, the totals and four values per segment"""
    L = H.lib()
    assert L.hdd_estimator_blocks_workspace(None) == 0
    loc = H.Grid.structured(H.SIMPLEX, 16, 17).local()
    est = H.Estimator(None, loc)
    n, nv = 544, 17 * 18
    before = est.n_work
    assert nv + 4 * 3 + 4 <= before <= nv + 1 + 4 * 3 + 4
    assert L.hdd_estimator_blocks_workspace(est.h) == 0
    for bounds, chunks in (([0, n], 3), ([0, 1, 3, 258, 514, n], 1 + 1 + 1 + 1 + 1), ([0, 257, n], 2 + 2)):
        est.set_segments(bounds)
        S = len(bounds) - 1
        assert L.hdd_estimator_workspace(est.h) == before
        assert est.n_work_blocks == L.hdd_estimator_blocks_workspace(est.h)
        assert nv + 4 * chunks + 4 + 4 * S <= est.n_work_blocks <= nv + 1 + 4 * chunks + 4 + 4 * S
    est.set_segments()
    assert L.hdd_estimator_blocks_workspace(est.h) == 0 and est.n_segments == 0
    out = np.zeros(4)
    assert L.hdd_estimator_segment_diameters(est.h, out.ctypes.data) == INVALID and b"no segments" in _msg()


def test_malformed_bounds_are_invalid():
    L = H.lib()
    loc = H.Grid.structured(H.SIMPLEX, 4, 4).local()
    est = H.Estimator(None, loc)
    n = loc.n_local
    good = np.array([0, 5, n], np.int64)
    assert L.hdd_estimator_set_segments(None, 2, good.ctypes.data) == INVALID and b"null" in _msg()
    assert L.hdd_estimator_set_segments(est.h, 2, None) == INVALID and b"null bounds" in _msg()
    assert L.hdd_estimator_set_segments(est.h, -1, good.ctypes.data) == INVALID and b"negative" in _msg()
    for bad, word in (([1, 5, n], b"bounds[0]"), ([0, 5, 5, n], b"ascending"), ([0, 7, 5, n], b"ascending"),
                      ([0, 5, n - 1], b"partition"), ([0, 5, n + 1], b"partition"), ([0, -3, n], b"ascending"),
                      (list(range(n + 2)), b"more segments")):
        b = np.array(bad, np.int64)
        assert L.hdd_estimator_set_segments(est.h, len(bad) - 1, b.ctypes.data) == INVALID, bad
        assert _msg().startswith(b"hdd_estimator_set_segments:") and word in _msg(), (bad, _msg())
        with pytest.raises(H.HddError):
            est.set_segments(bad)
    # a rejected call leaves the tables of the last valid one
    est.set_segments(good)
    with pytest.raises(H.HddError):
        est.set_segments([0, 5, 5, n])
    assert est.segment_diameters().shape == (2,)
    with pytest.raises(H.HddError):
        est.set_segments([0, 5, n], subdomains=(0, 1))


def test_subdomains_are_segments():
    g = H.Grid.structured(H.SIMPLEX, 8, 6, px=2, py=3)
    loc = g.local()
    est = H.Estimator(None, loc)
    est.set_segments(subdomains=(0, 6))
    assert est.n_segments == 6
    bounds = [0] + [g.subdomain_range(s, s + 1)[1] for s in range(6)]
    ev, xy = loc.vertices()
    ref = B.brute_force_diameters(xy, np.ascontiguousarray(ev.T), bounds)
    assert np.all(np.abs(est.segment_diameters() - ref) <= 4 * np.spacing(ref))
    # a subdomain of 4 x 2 cells of 1/8 x 1/6
    assert np.allclose(ref, np.hypot(0.5, 1.0 / 3.0), rtol=1e-14, atol=0)


class _BlockOperands(_Operands):
    def __init__(self, segments=True):
        super().__init__()
        if segments:
            self.est.set_segments([0, 7, self.local.n_local])
        self.theta = {k: None for k in ("mu", "bar", "hat", "min", "max")}

    def call(self, n_work=None, est="est", ctx="fake", sums="sums"):
        g = lambda k: None if k is None else C.addressof(getattr(self, k))
        th = {k: (None if v is None else np.ascontiguousarray(v, np.float64)) for k, v in self.theta.items()}
        if n_work is None:
            n_work = max(self.est.n_work_blocks, 1)
        return H.lib().hdd_block_swipdg_estimate(
            None if ctx is None else self.fake, None if est is None else self.est.h, g("mesh"), g("kappa"), 2, H._p(th["mu"]),
            H._p(th["bar"]), H._p(th["hat"]), H._p(th["min"]), H._p(th["max"]), g("tensor"), g("force"), g("prm"), self.fake,
            self.fake, n_work, None, None, None, None, None if sums is None else self.sums.ctypes.data, None)


def test_block_call_rejects_before_any_device_call():
    o = _BlockOperands(segments=False)
    assert o.call() == INVALID and _msg().startswith(WHO) and b"no segments" in _msg()
    o = _BlockOperands()
    for k in ("ctx", "est", "sums"):
        assert o.call(**{k: None}) == INVALID and b"null" in _msg(), k
    for role in ("mu", "bar", "hat", "min", "max"):
        for bad in ((1.0, 0.0), (-1.0, 1.0), (1.0, float("nan"))):
            o = _BlockOperands()
            o.theta[role] = bad
            assert o.call() == INVALID, (role, bad)
            assert _msg().startswith(WHO) and b"not positive" in _msg(), (role, bad, _msg())
    o = _BlockOperands()
    for n_work in (o.est.n_work_blocks - 1, o.est.n_work, 0, -1):
        assert n_work < o.est.n_work_blocks
        assert o.call(n_work=n_work) == INVALID and b"n_work" in _msg(), n_work
    o.mesh.degree = 2
    assert o.call() == 3 and b"degree" in _msg()          # the scope checks of the ESV call
    # every check passed: what is left is the host-only estimator, still without a device call
    o = _BlockOperands()
    o.theta.update(mu=(1.0, 0.5), bar=(0.7, 1.3), hat=(1.2, 0.4), min=(0.1, 0.2), max=(3.0, 4.0))
    assert o.call() == INVALID and b"host-only" in _msg()


def test_factors_against_numpy():
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, H.MAX_COMP):
        mu, bar, hat = rng.uniform(0.1, 3.0, (3, n))
        got = H.os2014_factors(mu, bar, hat)
        ref = B.factors(mu, bar, hat)
        assert np.allclose(got, ref, rtol=4 * np.finfo(float).eps, atol=0), n
        assert H.os2014_factors(mu) == (1.0, 1.0, 1.0, 1.0, 1.0)
        assert H.os2014_factors(mu, None, hat)[:2] == (1.0, 1.0)
    out = np.zeros(5)
    one, zero = np.array([1.0, 1.0]), np.array([1.0, 0.0])
    L = H.lib()
    assert L.hdd_os2014_factors(2, one.ctypes.data, zero.ctypes.data, None, out.ctypes.data) == INVALID
    assert b"not positive" in _msg()
    assert L.hdd_os2014_factors(2, (-one).ctypes.data, None, None, out.ctypes.data) == INVALID
    assert L.hdd_os2014_factors(0, one.ctypes.data, None, None, out.ctypes.data) == INVALID and b"n_comp" in _msg()
    assert L.hdd_os2014_factors(2, one.ctypes.data, None, None, None) == INVALID
    assert L.hdd_os2014_factors(2, None, None, None, out.ctypes.data) == 0 and np.array_equal(out, np.ones(5))


def _check_diameters(grid, bounds):
    loc = grid.local()
    est = H.Estimator(None, loc)
    est.set_segments(bounds)
    ev, xy = loc.vertices()
    ref = B.brute_force_diameters(xy, np.ascontiguousarray(ev.T), np.asarray(bounds))
    got = est.segment_diameters()
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= 4 * np.spacing(ref)), np.abs(got - ref).max()
    return got


@pytest.mark.parametrize("P", [1, 2, 4, 8])
def test_diameters_of_the_boxes_of_the_128_element_mesh(P):
    _, c, ev = nvb_mesh(4, 2)
    perm, bounds = B.box_partition(c, ev, P, P)
    d = _check_diameters(H.Grid.from_connectivity(H.SIMPLEX, c, np.asarray(ev)[perm]), bounds)
    assert np.allclose(d, 2.0 * np.sqrt(2.0) / P, rtol=1e-15, atol=0)      # rectangles: collinear boundary vertices


@pytest.mark.parametrize("sizes", [(1, 2, 255, 286), (256, 257, 31), (544,)])
def test_diameters_of_ranges_of_the_kuhn_grid(sizes):
    """16 x 17 Kuhn grid, 544 elements: segments of 1 (one triangle), 2, 255, 256, 257 elements"""
    g = H.Grid.structured(H.SIMPLEX, 16, 17, (0.0, 0.0), (1.0, 0.75))
    _check_diameters(g, np.concatenate([[0], np.cumsum(sizes)]))


def test_diameters_of_disconnected_segments():
    """the elements renumbered at random: every contiguous range is scattered over the square"""
    _, c, ev = nvb_mesh(4, 2)
    ev = np.asarray(ev)[np.random.default_rng(5).permutation(128)]
    d = _check_diameters(H.Grid.from_connectivity(H.SIMPLEX, c, ev), [0, 3, 4, 6, 40, 128])
    assert d[1] < d[0] and d[4] > 2.0


def test_diameters_on_the_distorted_mesh():
    c, ev = distorted()
    g = H.Grid.from_connectivity(H.SIMPLEX, c, ev)
    _check_diameters(g, [0, 128])
    _check_diameters(g, [0, 1, 2, 5, 17, 64, 100, 128])
    _check_diameters(g, np.arange(129))
