// dune-hdd_amd/csrc/kernels/swipdg_policy.hh -- what the persistent tile driver (swipdg_persistent.hh) may ask of
// a policy beyond the mandatory part (NB, NF, RB, WGCU, MINW, PAD, Own, Gat, load_own, load_gat, load_gat2,
// n_interior, compute): optional capabilities, off unless the policy overrides them.
#pragma once
#include <hip/hip_runtime.h>

namespace hdd {
namespace dev {

struct PolicyDefaults {
  // FUSED policies emit several components per tile from one prepare() (P1SmoothFusedPolicy): the driver
  // builds and streams one LDS image per component (a.n_comp of them, into a.vals[c])
  static constexpr bool FUSED = false;
  struct Shared {};   // what prepare() leaves for emit_component() / emit_two()
  // HALF policies (Q1PwcPolicy<.., H2>) stage a tile through an image of 32 row blocks, one half after the other
  static constexpr bool HALF = false;
  // TWO policies (P1SmoothFusedPolicy<.., true>) emit two components per tile into two images (the LDS holds both)
  static constexpr bool TWO = false;
  // FULLTILE policies (P1PwcPolicy) have a compute_full for tiles of 64 elements with every face interior
  static constexpr bool FULLTILE = false;
  // EMIT policies (Q1PwcPolicy) have emit(): the row block one NB x NB block at a time
  static constexpr bool EMIT = false;
};

// What compute() of a PAD policy writes through: one lane's row block in the LDS tile image, written at index
// i -> (i + rot) mod RB (rot = 0: plain).  Uniform Q1 tiles use rot = 2 ((lane >> 1) & 15): see the persistent
// kernel's image comment.
template <int RB>
struct RotImg {
  double* p;
  int rot;
  __device__ __forceinline__ double& operator[](int i) const
  {
    const unsigned q = unsigned(i + rot);
    return p[q < unsigned(RB) ? q : q - unsigned(RB)];
  }
};

// row blocks the LDS tile image holds
template <class P>
constexpr int image_blocks() { return P::HALF ? 32 : 64; }

}  // namespace dev
}  // namespace hdd
