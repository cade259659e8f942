"""Preconditions of the right-hand side GPU tests (tests/rhs_cases.py), on the host.

The GPU tests cannot observe which evaluation of the cos-product force a wave of rhs2d_kernel took; what they rely
on is the kernel's predicate restated in numpy (rhs_cases.element_dm / wave_tiers) with the thresholds read from
trig_phase.hh.  These tests assert, for every tier case and both element types, that the restated predicate puts
the case's waves where its name says, that both directions' phases are large and cross a multiple of pi/2 inside
the mesh, that the marked boundary groups are non-empty, that the rank-local range starts above 0 with ghosts on
both sides, and that every oracle reference is nonzero.  CPU only."""
import numpy as np
import pytest

import hdd_amd as H
import oracle as O
import rhs_cases as R
from rhs_cases import FAR, NEAR, TINY

ETS = [H.SIMPLEX, H.CUBE]


def test_thresholds_come_from_the_header():
    small, tiny = R.phase_thresholds()
    txt = open(R.TRIG_HEADER).read()
    assert "constexpr double SMALL_PHASE = %r;" % small in txt
    assert "constexpr double TINY_PHASE = %r;" % tiny in txt
    assert tiny < small < 0.5


def test_element_dm_formula():
    """two hand-made elements: kx and ky, and j01 and j10, enter dm asymmetrically"""
    #             x0   y0   x1   y1   x2   y2
    c = np.array([[0.0, 0.0, 0.3, 0.1, 0.2, 0.7], [1.0, 2.0, 1.5, 2.0, 1.0, 2.25]]).T
    dm = R.element_dm(c, 2.0, 3.0)
    assert np.allclose(dm, [max(2 * 0.3 + 2 * 0.2, 3 * 0.1 + 3 * 0.7), max(2 * 0.5, 3 * 0.25)], rtol=1e-15)
    assert not np.allclose(R.element_dm(c, 3.0, 2.0), dm)
    j00, j10, j01, j11 = R.element_jacobian(c)
    assert not np.allclose(R.jacobian_dm(2.0, 3.0, j00, j01, j10, j11)[:1], dm[:1])     # j10 <-> j01
    tiers, pushed = R.wave_tiers(np.r_[np.full(63, 0.01), 0.02, np.full(10, 0.2)], small=0.125, tiny=0.015625)
    assert tiers.tolist() == [NEAR, FAR] and pushed.tolist() == [True, False]


@pytest.mark.parametrize("et", ETS)
@pytest.mark.parametrize("tier", R.TIERS)
def test_tier_case_preconditions(tier, et):
    small, tiny = R.phase_thresholds()
    case = R.tier_case(tier, et)
    grid = case.grid()
    loc = grid.local()
    # the launch order is the element order of the case, thread k = element k (one grid-stride pass)
    assert loc.own_begin == 0 and loc.n_own == case.ev.shape[0] == grid.ne
    assert np.array_equal(loc.global_id, np.arange(grid.ne))
    assert loc.n_own <= 8 * R.MI355X_CUS * 256 and loc.n_own > 64 and loc.n_own % 64 != 0    # multi-wave, ragged
    assert np.array_equal(loc.coords, R.element_major(case.coords, case.ev))
    dm = R.element_dm(loc.coords, case.kx, case.ky)
    assert np.array_equal(dm, case.dm)
    tiers, pushed = R.wave_tiers(dm)
    assert tiers.shape[0] == (loc.n_own + 63) // 64
    waves = [dm[k:k + 64] for k in range(0, dm.shape[0], 64)]
    kind = tier.split("_")[0]
    if kind == "tiny":
        assert np.all(tiers == TINY) and dm.max() >= tiny / 2 and dm.max() <= tiny
    elif kind == "near":
        assert np.all(tiers == NEAR) and dm.max() >= small / 2 and dm.max() <= small
        assert all(np.any(w > tiny) for w in waves)
    elif kind == "far":
        assert np.all(tiers == FAR) and all(np.any(w > small) for w in waves)
    else:
        assert {TINY, NEAR, FAR} <= set(tiers.tolist())
        assert pushed.any()
        # the pushed wave would be tiny (or near) without its one element
        w = int(np.nonzero(pushed)[0][0])
        assert np.sort(waves[w])[-2] <= (tiny if tiers[w] == NEAR else small)
    # no element sits on a threshold: a rounding difference cannot move a wave
    for thr in (small, tiny):
        assert np.all(np.abs(dm - thr) > 0.05 * thr)
    # kx != ky and hx != hy: swapping j01 / j10 or kx / ky changes dm (and the force) at first order
    assert abs(case.kx / case.ky - 1.0) > 0.05
    c = loc.coords
    ext_x = np.max(np.abs(np.stack([c[2] - c[0], c[4] - c[0]])), axis=0)
    ext_y = np.max(np.abs(np.stack([c[3] - c[1], c[5] - c[1]])), axis=0)
    if not tier.endswith("_sheared"):                                   # (axis-aligned: hx and hy themselves)
        assert np.all(np.abs(ext_x / ext_y - 1.0) > 0.05)
    j00, j10, j01, j11 = R.element_jacobian(c)
    swapped = R.jacobian_dm(case.kx, case.ky, j00, j01, j10, j11)      # j10 <-> j01
    if et == H.SIMPLEX or tier.endswith("_sheared"):
        assert np.max(np.abs(swapped - dm)) > 0.05 * dm.max()
    assert np.max(np.abs(R.element_dm(c, case.ky, case.kx) - dm)) > 0.05 * dm.max()
    # phases: away from the origin, 100 <= max|phase| <= 1000, a multiple of pi/2 inside the mesh, per direction
    for ph in case.phases():
        assert 100.0 <= np.max(np.abs(ph)) <= 1000.0
        assert np.floor(ph.max() / (0.5 * np.pi)) > np.floor(ph.min() / (0.5 * np.pi))
    assert np.all(case.coords.min(axis=0) > 1.0)
    # references: nonzero, both boundary groups present, a corner element among the marked
    b_f, b_all, marked = R.tier_refs(tier, et)
    assert np.max(np.abs(b_f)) > 0 and np.max(np.abs(b_all - b_f)) > 0
    nbnd = (loc.neighbors < 0).sum(axis=0)
    assert marked.shape == (loc.n_own,) and np.all(nbnd[marked] > 0)
    assert np.any(nbnd[marked] > 1) and np.any((nbnd > 0) & ~marked)
    onb, _ = case.ogrid().neighbors()
    assert np.array_equal(onb.T < 0, loc.neighbors < 0)
    rows_n, rows_d = np.repeat(marked, case.nb), np.repeat((nbnd > 0) & ~marked, case.nb)
    assert np.max(np.abs((b_all - b_f)[rows_n])) > 0 and np.max(np.abs((b_all - b_f)[rows_d])) > 0


@pytest.mark.parametrize("name", R.GEOMETRY_MESHES)
def test_geometry_mesh_preconditions(name):
    et, coords, ev = R.geometry_mesh(name)
    det = R.signed_dets(coords, ev)
    if name.endswith("_mirrored"):
        # every element's orientation is the opposite of the unmirrored mesh's.  (The two triangles of a Kuhn square
        # differ in orientation to begin with, so det J < 0 for all elements holds for the quadrilaterals only.)
        # Grid.from_connectivity accepts clockwise elements: a mesh comes back, checked below like the others.
        _, c0, ev0 = R.geometry_mesh(name.replace("_mirrored", "_sheared"))
        assert np.array_equal(coords, c0 * np.array([-1.0, 1.0])) and np.array_equal(ev, ev0)
        assert np.array_equal(det, -R.signed_dets(c0, ev0))
        assert np.all(det < 0) if et == H.CUBE else (np.any(det < 0) and np.any(det > 0))
    elif et == H.CUBE:
        assert np.all(det > 0)
    else:
        assert np.any(det < 0) and np.any(det > 0)
    grid = H.Grid.from_connectivity(et, coords, ev)
    loc = grid.local()
    assert np.array_equal(loc.global_id, np.arange(grid.ne)) and loc.own_begin == 0
    assert np.array_equal(loc.coords, R.element_major(coords, ev))
    onb, _ = O.Grid(et, coords, ev).neighbors()
    assert np.array_equal(np.where(onb < 0, H.NBR_DIRICHLET, onb), loc.neighbors.T)
    assert grid.ne > 256 or name == "nvb"                        # more than one workgroup
    if name != "nvb":                                            # general Jacobian: all four entries nonzero
        c = loc.coords
        assert np.all(np.abs(np.stack([c[2] - c[0], c[3] - c[1], c[4] - c[0], c[5] - c[1]])).max(axis=1) > 0)
    marked = R.mark_elements(loc.neighbors, 41)
    nbnd = (loc.neighbors < 0).sum(axis=0)
    assert np.any((nbnd > 0) & ~marked) and np.all(nbnd[marked] > 0) and marked.any()
    assert R.has_corner(loc.neighbors) == (name != "nvb")       # (the bisection mesh has no two-face element)
    assert np.any(nbnd[marked] > 1) or name == "nvb"
    R.set_boundary(loc, marked, H.NBR_NEUMANN)
    assert np.any(loc.neighbors == H.NBR_NEUMANN) and np.any(loc.neighbors == H.NBR_DIRICHLET)
    assert np.array_equal((loc.neighbors == H.NBR_NEUMANN).any(axis=0), marked)


@pytest.mark.parametrize("et", ETS)
def test_block_range_preconditions(et):
    grid = R.block_grid(et)
    assert grid.n_sub == 6
    s = R.BLOCK_S
    loc = grid.local(s, s + 1)
    a, b = grid.subdomain_range(s, s + 1)
    assert loc.own_begin > 0 and loc.own_end < loc.n_local          # ghosts on both sides of the owned range
    assert loc.n_own == b - a and loc.n_ghost == loc.n_local - loc.n_own
    assert np.array_equal(loc.global_id[loc.own_begin:loc.own_end], np.arange(a, b))
    ghosts = np.r_[loc.global_id[:loc.own_begin], loc.global_id[loc.own_end:]]
    assert np.any(ghosts < a) and np.any(ghosts >= b)
    sizes = [np.subtract(*grid.subdomain_range(t, t + 1)[::-1]) for t in range(6)]
    assert len(set(sizes)) > 1                                       # ragged subdomains
    assert np.any(loc.neighbors[:, loc.own_begin:loc.own_end] == H.NBR_DIRICHLET)
    og, ei = R.oracle_elem_index(grid, et)
    full = grid.local()
    assert np.array_equal(full.coords[:, ei], R.element_major(og.coords, og.ev))
