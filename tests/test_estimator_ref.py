"""Pins the numpy restatement of the ESV2007 estimator (tests/estimator_ref.py) against the reference's own expectation
table, test/linearelliptic-swipdg-expectations_esv2007_2daluconform.cxx:38-57, on the oracle's solve of the ESV2007
problem (O.assemble, O.rhs_esv2007, spsolve) on the ALU conforming ladder: all seven estimator rows to 3 significant
figures.  The restatement is the yardstick of the device estimator (tests/test_gpu_estimate.py)."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import estimator_ref as R
import oracle as O
from mesh_tools import nvb_mesh
from test_oracle_pinning import sig3

ETA_NC = [1.66e-1, 7.89e-2, 3.91e-2, 1.95e-2]
ETA_R = [7.23e-2, 1.82e-2, 4.54e-3, 1.14e-3]
ETA_DF = [3.55e-1, 1.76e-1, 8.73e-2, 4.35e-2]
ETA = [4.49e-1, 2.07e-1, 9.91e-2, 4.85e-2]
EFF = [1.37, 1.28, 1.23, 1.21]
ETA_ALT = [5.93e-1, 2.73e-1, 1.31e-1, 6.42e-2]
EFF_ALT = [1.81, 1.69, 1.63, 1.60]
TABLE = dict(eta_NC=ETA_NC, eta_R=ETA_R, eta_DF=ETA_DF, eta=ETA, eff=EFF, eta_alt=ETA_ALT, eff_alt=EFF_ALT)


def rows_of(sums, h1):
    """the seven rows from the four sums over T and the H1-semi error (the energy error of kappa = 1, A = I)"""
    nc, r, df = np.sqrt(sums[0]), np.sqrt(sums[1]), np.sqrt(sums[2])
    eta, alt = np.sqrt(sums[3]), nc + r + df
    return dict(eta_NC=nc, eta_R=r, eta_DF=df, eta=eta, eff=eta / h1, eta_alt=alt, eff_alt=alt / h1)


@pytest.fixture(scope="module")
def solves():
    out = []
    for lvl in range(3):
        et, c, ev = nvb_mesh(4, 2 + 2 * lvl)
        g = O.Grid(et, c, ev)
        rp, col, val = O.assemble(g, O.scalar(O.FN_CONST, 1.0), O.tensor(), O.params())
        A = O.to_scipy(rp, col, val)
        b = O.rhs_esv2007(g)
        u = spla.spsolve(A.tocsc(), b)
        out.append((c, ev, A, b, u, O.error_norms_esv2007(g, u)[1]))
    return out


def test_seven_rows_match_the_reference_table(solves):
    got = {k: [] for k in TABLE}
    for c, ev, _, _, u, h1 in solves:
        r = R.estimate(c, ev, u, force=R.esv2007_force())
        for k, v in rows_of(r["sums"], h1).items():
            got[k].append(sig3(v))
    for k in TABLE:
        assert got[k] == TABLE[k][:3], k


def test_flux_is_conservative_and_consistent(solves):
    """F_T,e + F_T',e' = 0 on interior faces; sum_e F_T,e = the three summed rows of A u (the volume and symmetry terms
    vanish against a constant test function), which for the solution are the three summed right-hand side entries"""
    c, ev, A, b, u, _ = solves[0]
    rng = np.random.default_rng(5)
    for vec in (u, rng.standard_normal(u.shape)):
        r = R.estimate(c, ev, vec)
        F, nbr = r["flux"], r["neighbors"]
        scale = np.abs(F).max()
        for f in range(3):
            inner = np.nonzero(nbr[:, f] >= 0)[0]
            N = nbr[inner, f]
            twin = (nbr[N] == inner[:, None]).argmax(1)
            assert np.abs(F[f, inner] + F[twin, N]).max() <= 1e-13 * scale
        assert np.abs(F.sum(0) - (A @ vec).reshape(-1, 3).sum(1)).max() <= 1e-13 * scale
    assert np.abs(R.estimate(c, ev, u)["flux"].sum(0) - b.reshape(-1, 3).sum(1)).max() <= 1e-12


def test_continuous_vector_has_no_nonconformity(solves):
    c, ev = solves[0][:2]
    nbr = R.face_neighbors(ev)
    inside = np.ones(c.shape[0], bool)
    for f in range(3):
        on = nbr[:, f] < 0
        inside[ev[on][:, list(R.FV[f])]] = False
    w = np.where(inside, np.cos(c[:, 0]) + c[:, 1] ** 2, 0.0)
    r = R.estimate(c, ev, w[ev].reshape(-1))
    assert np.array_equal(r["oswald"][~inside], np.zeros((~inside).sum()))
    assert np.abs(r["oswald"] - w).max() <= 4 * np.finfo(float).eps
    assert r["local"][0].max() <= 1e-28


def test_fixed_order_sum_is_a_sum():
    rng = np.random.default_rng(1)
    for n in (0, 1, 255, 256, 257, 70000):
        x = rng.random(n)
        assert abs(R.fixed_order_sum(x) - x.sum()) <= 1e-12 * max(x.sum(), 1.0)
