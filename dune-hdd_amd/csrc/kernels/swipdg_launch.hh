// dune-hdd_amd/csrc/kernels/swipdg_launch.hh -- host side of the persistent tile driver: the launch of a policy
// (grid, LDS, tile list / sharded SKIP / element-list variants) and the run-time kind -> policy dispatch helpers.
// The per-family entry points (launch_p1_pwc, ...) are declared in swipdg_kernels.hh.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>

#include "hdd_internal.hh"
#include "swipdg_persistent.hh"

namespace hdd {
namespace dev {

// "swipdg_persistent_kernel<Policy<...>, TL, SKIP>" from the template argument's pretty name (host, once per policy)
template <class P>
static std::string kernel_name(const char* flags)
{
  const std::string f = __PRETTY_FUNCTION__;   // "... [P = hdd::dev::Q1PwcPolicy<1, 0, false, true, true>]"
  const size_t a = f.find("P = "), b = f.rfind(']');
  std::string p = a == std::string::npos ? "?" : f.substr(a + 4, b - a - 4);
  if (p.rfind("hdd::dev::", 0) == 0) p = p.substr(10);
  return "swipdg_persistent_kernel<" + p + ", " + flags + ">";
}

template <class P>
static hipError_t launch_persistent(const AssembleArgs& a, hipStream_t s)
{
  const int64_t n_own = a.own_end - a.own_begin;
  if (n_own <= 0) return hipSuccess;
  const int64_t tiles = a.tile_list ? a.n_tile_list : (n_own + 63) / 64;
  if (tiles <= 0) return hipSuccess;
  const size_t lds = (P::PAD ? size_t(image_blocks<P>()) * P::RB : size_t(64) * P::RB + 2 + P::RB) * sizeof(double) *
                     (P::TWO ? 2 : 1);
  if (P::TWO && a.n_comp != 2) return hipErrorInvalidValue;
  const int cus = a.n_cu;
  // tiles per CU measured per policy (profiles/r01/sweep_wg_per_cu.log, profiles/r01/s2/); a.wgcu > 0 is the
  // HDD_P1_WGCU sweep override, read once per context
  int wgcu = a.wgcu > 0 ? a.wgcu : P::WGCU;
  size_t lds_launch = lds;
#ifdef HDD_ABLATION
  // HDD_P1_WGCU = W + 16 C (C > 0): W tiles per CU with at most C resident per CU -- the dynamic LDS padded to
  // 160 KB / C, so the dispatcher cannot stack more workgroups on one CU than C (residency study)
  if (a.wgcu >= 16) {
    lds_launch = std::max(lds, size_t((160 * 1024) / (a.wgcu >> 4)) & ~size_t(15));
    wgcu = (a.wgcu & 15) ? (a.wgcu & 15) : P::WGCU;
  }
#endif
  wgcu = std::max(1, std::min<int>(wgcu, int((160 * 1024) / lds_launch)));   // resident by LDS (Q1 tiles: 3 per CU)
  // The sharded step's full-range launch (SKIP, or every tile beside the SoA side-buffer pass) runs beside the
  // element pass: the grid is shortened
  // by the pass's workgroups (a multiple of 8 keeps the XCD eighths even), so the pass gets SIMDs of its own
  // instead of slowing the persistent waves it would share them with.  C4 N = 8 middle rank +9.2 -> +7.8 %, C2 N = 8
  // end rank +4.9 -> +2.0 % over one launch (profiles/r04/e_reserve/; ablation bit 4194304: no reserve).
  int64_t slots = int64_t(cus) * wgcu;
  const bool reserve = a.reserve_wg > 0 && !HDD_ABL(a, 4194304);
  if (reserve) slots = std::max<int64_t>(8, (slots - a.reserve_wg) & ~int64_t(7));
  const int64_t G = std::min<int64_t>(tiles, slots);
  if (a.list_elements != LIST_TILES) {   // element-list fixup pass: one lane per element
    const size_t lds_e = size_t(64) * P::RB * sizeof(double);
    const int64_t ge = std::min<int64_t>((a.n_tile_list + 63) / 64, int64_t(cus) * 4);
    if (a.list_elements >= LIST_SIDE_BUFFER) {   // no LDS: into the side buffers (slot RB doubles) or in place
      if (a.list_elements == LIST_SIDE_BUFFER && a.fix_rb != P::RB) return hipErrorInvalidValue;
      if (a.list_elements == LIST_SIDE_SOA && (!P::EMIT || a.fix_ld < a.n_tile_list + 1)) return hipErrorInvalidValue;
      return per_component<P::FUSED>(a, [&](const AssembleArgs& ac) {
        hipLaunchKernelGGL((swipdg_elements_buf_kernel<P>), dim3(unsigned(ge)), dim3(64), 0, s, ac, a.n_tile_list);
      });
    }
    return per_component<P::FUSED>(a, [&](const AssembleArgs& ac) {
      hipLaunchKernelGGL((swipdg_elements_kernel<P>), dim3(unsigned(ge)), dim3(64), lds_e, s, ac, a.n_tile_list);
    });
  }
  // the dispatch's choice, readable through hdd_last_tile_kernel(): "swipdg_persistent_kernel<P, TL, SKIP>"
  static const std::string names[3] = {kernel_name<P>("true, false"), kernel_name<P>("false, true"),
                                       kernel_name<P>("false, false")};
  hdd::last_tile_kernel_slot() = names[a.tile_list ? 0 : (a.skip_ghost ? 1 : 2)].c_str();
  return per_component<P::FUSED>(a, [&](const AssembleArgs& ac) {
    if (a.tile_list)
      hipLaunchKernelGGL((swipdg_persistent_kernel<P, true>), dim3(unsigned(G)), dim3(64), lds_launch, s, ac, tiles);
    else if (a.skip_ghost)
      hipLaunchKernelGGL((swipdg_persistent_kernel<P, false, true>), dim3(unsigned(G)), dim3(64), lds_launch, s, ac, tiles);
    else
      hipLaunchKernelGGL((swipdg_persistent_kernel<P, false>), dim3(unsigned(G)), dim3(64), lds_launch, s, ac, tiles);
  });
}

// f(integral_constant<tensor kind>) for the run-time tensor kind
template <int V> using kind_c = std::integral_constant<int, V>;
template <class F>
static hipError_t with_tensor_kind(int tk, F&& f)
{
  if (tk == HDD_TENSOR_CONST) return f(kind_c<HDD_TENSOR_CONST>{});
  if (tk == HDD_TENSOR_ISO_PER_ELEM) return f(kind_c<HDD_TENSOR_ISO_PER_ELEM>{});
  return f(kind_c<HDD_TENSOR_SYM_PER_ELEM>{});
}
// f(integral_constant<tensor kind>, integral_constant<kappa kind>) for the run-time (tensor kind,
// piecewise-constant kappa kind) pair of the call
template <class F>
static hipError_t with_pwc_kinds(const AssembleArgs& a, F&& f)
{
  const bool pe = a.kappa[0].kind == HDD_FN_PER_ELEM;
  return with_tensor_kind(a.tkind, [&](auto tk) { return pe ? f(tk, kind_c<HDD_FN_PER_ELEM>{}) : f(tk, kind_c<HDD_FN_CONST>{}); });
}

// instantiate a policy for the runtime (tensor kind, piecewise-constant kappa kind) pair
template <template <int, int> class PT>
static hipError_t dispatch_pwc(const AssembleArgs& a, hipStream_t s)
{
  return with_pwc_kinds(a, [&](auto tk, auto kk) { return launch_persistent<PT<tk.value, kk.value>>(a, s); });
}

// instantiate a policy for the runtime (tensor kind, kappa kind) pair; VX: vertex-indexed geometry
template <template <int, int, bool> class PT, bool VX>
static hipError_t dispatch_kinds_vx(const AssembleArgs& a, hipStream_t s, bool smooth)
{
  if (smooth)
    return with_tensor_kind(a.tkind, [&](auto tk) {
      return a.kappa[0].kind == HDD_FN_FLATTOP ? launch_persistent<PT<tk.value, HDD_FN_FLATTOP, VX>>(a, s)
                                               : launch_persistent<PT<tk.value, HDD_FN_SINUSOID, VX>>(a, s);
    });
  return with_pwc_kinds(a, [&](auto tk, auto kk) { return launch_persistent<PT<tk.value, kk.value, VX>>(a, s); });
}
// Vertex-indexed geometry pays on triangles (C2 0.323 -> 0.245 ms, same box: 2 waves per SIMD hide the
// second gather stage); the Q1 tiles run one wave per SIMD (40 KB image), where that stage's latency is
// exposed (C4 0.600 -> 0.690 ms), so quads keep the element-major coords.
template <template <int, int, bool> class PT>
static hipError_t dispatch_kinds(const AssembleArgs& a, hipStream_t s, bool smooth)
{
  if constexpr (PT<HDD_TENSOR_CONST, HDD_FN_CONST, false>::NB == 4) {   // quads: element-major only
    return dispatch_kinds_vx<PT, false>(a, s, smooth);
  } else {
    return a.ev && a.elem_type == HDD_SIMPLEX ? dispatch_kinds_vx<PT, true>(a, s, smooth)
                                              : dispatch_kinds_vx<PT, false>(a, s, smooth);
  }
}

}  // namespace dev
}  // namespace hdd
