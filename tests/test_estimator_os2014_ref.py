"""Pins the numpy restatement of the OS2014 localized estimator (tests/estimator_os2014_ref.py) against the reference's
expectation table, test/linearelliptic-block-swipdg-expectations_esv2007_2daluconform.cxx:35-134 (the fixture
tests/golden/os2014_esv2007_multiscale.json), on the oracle's solve of the ESV2007 problem on the ALU conforming ladder,
partitioned into P x P centroid boxes of [-1, 1]^2: the five rows of the four partitionings at levels 0..2 to 3
significant figures.  The restatement is the yardstick of the device estimator (tests/test_gpu_estimate_blocks.py)."""
import json
import os

import numpy as np
import pytest

import estimator_os2014_ref as B
import estimator_ref as R
from test_estimator_ref import solves  # noqa: F401 (the module-scoped fixture: the oracle's solves of levels 0..2)
from test_oracle_pinning import sig3

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "os2014_esv2007_multiscale.json")))
TABLE = GOLDEN["partitionings"]
PARTITIONINGS = {"[1 1 1]": 1, "[2 2 1]": 2, "[4 4 1]": 4, "[8 8 1]": 8}


def rows_of(sums, energy):
    """the five rows from (sum N_s, sum R_s, sum D_s, eta^2) and the energy error"""
    eta = float(np.sqrt(sums[3]))
    return dict(eta_NC_OS2014=float(np.sqrt(sums[0])), eta_R_OS2014=float(np.sqrt(sums[1])),
                eta_DF_OS2014=float(np.sqrt(sums[2])), eta_OS2014=eta, eff_OS2014=eta / energy)


def partitioned(c, ev, u, P):
    """the mesh and the vector renumbered subdomain-major for P x P boxes, and the segment bounds"""
    perm, bounds = B.box_partition(c, ev, P, P)
    return np.asarray(ev)[perm], np.asarray(u).reshape(-1, 3)[perm].reshape(-1), bounds


def test_fixture_holds_the_four_partitionings():
    assert sorted(TABLE) == sorted(PARTITIONINGS)
    for rows in TABLE.values():
        assert sorted(rows) == ["eff_OS2014", "eta_DF_OS2014", "eta_NC_OS2014", "eta_OS2014", "eta_R_OS2014"]
        assert all(len(v) == 4 for v in rows.values())


@pytest.mark.parametrize("name", sorted(PARTITIONINGS))
def test_five_rows_match_the_reference_table(solves, name):
    P = PARTITIONINGS[name]
    got = {k: [] for k in TABLE[name]}
    for c, ev, _, _, u, h1 in solves:
        ev2, u2, bounds = partitioned(c, ev, u, P)
        assert len(bounds) == P * P + 1
        r = B.estimate_blocks(c, ev2, u2, bounds, force=R.esv2007_force())
        for k, v in rows_of(r["sums"], h1).items():
            got[k].append(sig3(v))
    for k in TABLE[name]:
        assert got[k] == TABLE[name][k][:3], (name, k, got[k])


def test_one_segment_is_the_fixed_order_sum_of_the_esv_rows(solves):
    c, ev, _, _, u, _ = solves[1]
    ne = np.asarray(ev).shape[0]
    r = B.estimate_blocks(c, ev, u, [0, ne], force=R.esv2007_force())
    esv = R.estimate(c, ev, u, force=R.esv2007_force())
    assert r["segments"][0, 0] == R.fixed_order_sum(esv["local"][0])
    assert r["segments"][2, 0] == R.fixed_order_sum(esv["local"][2])
    assert r["sums"][0] == r["segments"][0, 0] and r["sums"][2] == r["segments"][2, 0]
    assert np.array_equal(r["local"][0], esv["local"][0]) and np.array_equal(r["local"][2], esv["local"][2])


def test_segment_sums_do_not_depend_on_the_other_segments(solves):
    c, ev, _, _, u, _ = solves[1]
    ne = np.asarray(ev).shape[0]                       # 512
    a = B.estimate_blocks(c, ev, u, [0, 100, 400, ne], force=R.esv2007_force())
    b = B.estimate_blocks(c, ev, u, [0, 1, 37, 100, 400, 401, 511, ne], force=R.esv2007_force())
    assert np.array_equal(a["segments"][:3, 1], b["segments"][:3, 3])
    assert a["diam"][1] == b["diam"][3]


def test_strided_total_is_a_sum_and_wraps():
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 272, 1000):
        x = rng.random(n)
        assert abs(B.strided_total(x) - x.sum()) <= 1e-13 * x.sum()
    x = rng.random(272)
    acc = x[:256].copy()
    acc[:16] += x[256:]
    assert B.strided_total(x) == R.fixed_order_sum(acc)


def test_two_triangle_segments_give_the_esv2007_residual(solves):
    """the 8 x 8 boxes at level 0 are 64 segments of two triangles, the two halves of a square whose diagonal is the
    longest edge of both: the diameter is h_T, so eta_R_OS2014 is ESV2007's eta_R to rounding"""
    c, ev, _, _, u, _ = solves[0]
    ev, u, bounds = partitioned(c, ev, u, 8)
    ne = ev.shape[0]
    assert ne == 128 and np.array_equal(bounds, np.arange(0, ne + 1, 2))
    r = B.estimate_blocks(c, ev, u, bounds, force=R.esv2007_force())
    esv = R.estimate(c, ev, u, force=R.esv2007_force())
    p = np.asarray(c)[ev]
    h = np.max([np.hypot(*(p[:, a] - p[:, b]).T) for a, b in R.FV], 0)
    assert np.allclose(r["diam"], h[0::2], rtol=1e-15, atol=0) and np.allclose(r["diam"], h[1::2], rtol=1e-15, atol=0)
    assert abs(r["eta_r"] - np.sqrt(esv["local"][1].sum())) <= 1e-13 * r["eta_r"]
    assert abs(r["segments"][3].sum() - 3.0 * (r["sums"][:3].sum()) / r["sums"][3]) <= 1e-13


def test_a_vanishing_estimate_has_vanishing_indicators(solves):
    c, ev = solves[0][:2]
    r = B.estimate_blocks(c, ev, np.zeros(3 * np.asarray(ev).shape[0]), [0, 5, 128])
    assert r["eta"] == 0.0 and np.array_equal(r["segments"], np.zeros((4, 2))) and np.array_equal(r["sums"], np.zeros(4))


def test_factors():
    f = B.factors([1.0, 0.5], [0.7, 1.3], [1.2, 0.4])
    assert f[0] == min(1 / 0.7, 0.5 / 1.3) and f[1] == max(1 / 0.7, 0.5 / 1.3)
    assert f[2] == min(1 / 1.2, 0.5 / 0.4) and f[3] == max(1 / 1.2, 0.5 / 0.4)
    assert f[4] == max(np.sqrt(f[3]), 1 / np.sqrt(f[2]))
    assert B.factors([2.0]) == (1.0, 1.0, 1.0, 1.0, 1.0)
