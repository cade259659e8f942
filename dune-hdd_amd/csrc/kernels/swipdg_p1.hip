// dune-hdd_amd/csrc/kernels/swipdg_p1.hip -- P1 (triangles) instantiations of the persistent tile driver:
// closed-form piecewise-constant stiffness (the C2 kernel), the smooth-kappa moments policy (C3), the
// SWIPDG penalty product.
#include "swipdg_policy_p1.hh"
#include "swipdg_policy_generic.hh"
#include "swipdg_launch.hh"

namespace hdd {
namespace dev {

template <int TK, int KK, bool VX> using P1Pwc = P1PwcPolicy<TK, KK, false, VX>;
template <int TK, int KK, bool VX> using P1Smooth3 = GenericPolicy<Simplex, 6, 3, TK, KK, VX>;

static hipError_t dispatch_smooth_p1(const AssembleArgs& a, hipStream_t s)
{
  if (a.variant & HDD_VARIANT_P1_SMOOTH_QUADRATURE) return dispatch_kinds<P1Smooth3>(a, s, true);
  if (a.kappa[0].kind == HDD_FN_FLATTOP) {   // (the SPE10 FlatTop channel: not a BASELINE kernel, VX only)
    if (!a.ev) return dispatch_kinds<P1Smooth3>(a, s, true);
    return with_tensor_kind(a.tkind, [&](auto tk) {
      return launch_persistent<P1SmoothPolicy<tk.value, true, HDD_FN_FLATTOP>>(a, s);
    });
  }
  return with_tensor_kind(a.tkind, [&](auto tk) {
    return a.ev ? launch_persistent<P1SmoothPolicy<tk.value, true>>(a, s)
                : launch_persistent<P1SmoothPolicy<tk.value>>(a, s);
  });
}

hipError_t launch_p1_pwc(const AssembleArgs& a, hipStream_t s) { return dispatch_kinds<P1Pwc>(a, s, false); }
hipError_t launch_p1_smooth(const AssembleArgs& a, hipStream_t s) { return dispatch_smooth_p1(a, s); }
// two components (OS2014, C3): both emitted in one pass over the geometry (P1SmoothFusedPolicy<.., TWO>); tile lists
// and the sharded SKIP launch included.  More components: one image, emitted one after the other.
hipError_t launch_p1_smooth_fused(const AssembleArgs& a, hipStream_t s)
{
  return with_tensor_kind(a.tkind, [&](auto tk) {
    return a.n_comp == 2 ? launch_persistent<P1SmoothFusedPolicy<tk.value, true, true>>(a, s)
                         : launch_persistent<P1SmoothFusedPolicy<tk.value, true>>(a, s);
  });
}

template <int TK, int KK> using P1Pen = P1PwcPolicy<TK, KK, true>;
template <int TK, int KK> using P1PenVX = P1PwcPolicy<TK, KK, true, 1>;
hipError_t launch_p1_penalty(const AssembleArgs& a, hipStream_t s)
{
  return a.ev ? dispatch_pwc<P1PenVX>(a, s) : dispatch_pwc<P1Pen>(a, s);   // vertex-indexed geometry as the stiffness
}

}  // namespace dev
}  // namespace hdd
