"""The three evaluations of the cos-product force in rhs2d_kernel<.., NQ, HDD_FN_COS_PRODUCT> (far: cos_phase at
the point; near / tiny: one sincos_phase per element and direction plus Taylor offsets, chosen per 64-lane wave)
and the RHS variants, each against the oracle (libm cos / sin in double, independent of trig_phase.hh) at
max|db| <= 1e-12 max|b| with no floor.

Which tier a wave took cannot be observed from here.  The evidence is the kernel's predicate restated in numpy on
the same coordinates (rhs_cases.wave_tiers), asserted for every case by tests/test_rhs_cases.py: all waves tiny /
near / far, a graded mesh with all three and a wave that one element pushes to the coarser tier, and two sheared
meshes on which the Jacobian's off-diagonal entries enter the offsets of Q1 elements as well.

Every case runs (a) the force alone and (b) the force with Dirichlet data (sinusoid g_D, per-element kappa and
iso tensor) on the unmarked and Neumann data on the marked boundary elements, on six contexts: the default, NO_TINY,
GENERIC (run-time rule, fn_value's switch), FUSED, ELEMENT_MAJOR and FUSED | GENERIC."""
import numpy as np
import pytest

import rhs_cases as R

H = pytest.importorskip("hdd_amd")
pytestmark = pytest.mark.gpu

VARIANTS = [("default", 0), ("no_tiny", H.VARIANT_RHS_NO_TINY), ("generic", H.VARIANT_RHS_GENERIC),
            ("fused", H.VARIANT_RHS_FUSED), ("element_major", H.VARIANT_ELEMENT_MAJOR),
            ("fused_generic", H.VARIANT_RHS_FUSED | H.VARIANT_RHS_GENERIC)]


@pytest.fixture(scope="module")
def variant_ctxs():
    out = {}
    for name, v in VARIANTS:
        out[name] = H.Context(0)
        out[name].set_variant(v)
    return out


@pytest.mark.parametrize("et", [H.SIMPLEX, H.CUBE])
@pytest.mark.parametrize("tier", R.TIERS)
def test_rhs_cos_tier_equals_oracle(variant_ctxs, tier, et):
    import torch
    case = R.tier_case(tier, et)
    b_f, b_all, marked = R.tier_refs(tier, et)
    loc = case.grid().local()
    R.set_boundary(loc, marked, H.NBR_NEUMANN)
    dm = H.DeviceMesh(loc)
    kel, tel = R.tier_data(case)
    dkx, dky, nkx, nky = case.data_wave_numbers()
    force = case.force(H)
    bnd = dict(kappa=H.scalar_fn(H.FN_PER_ELEM, per_elem=torch.from_numpy(kel).cuda()),
               tensor=H.tensor_fn(H.TENSOR_ISO_PER_ELEM, per_elem=torch.from_numpy(tel).cuda()),
               dirichlet=H.scalar_fn(H.FN_SINUSOID, 1.0, b=0.5, kx=dkx, ky=dky, order=3),
               neumann=H.scalar_fn(H.FN_COS_PRODUCT, 2.0, kx=nkx, ky=nky, order=2))
    worst, got = {}, {}
    for name, _ in VARIANTS:
        c = variant_ctxs[name]
        only = H.rhs(c, dm, force=force, prm=H.params())
        full = H.rhs(c, dm, force=force, prm=H.params(), **bnd)
        torch.cuda.synchronize()
        got[name] = (only.cpu().numpy(), full.cpu().numpy())
    for name, (only, full) in got.items():
        label = "%s %s" % (R.ET_NAME[et], tier)
        R.check("tier %s force: %s" % (label, name), only, b_f, worst)
        R.check("tier %s force+boundary: %s" % (label, name), full, b_all, worst)
    for key, r in worst.items():
        print("rhs worst %s %.3g" % (key, r))
    if tier == "far":   # no wave is tiny: the flag has nothing to switch off
        assert np.array_equal(got["no_tiny"][0], got["default"][0])
        assert np.array_equal(got["no_tiny"][1], got["default"][1])
