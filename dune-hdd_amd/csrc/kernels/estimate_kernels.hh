// dune-hdd_amd/csrc/kernels/estimate_kernels.hh -- the ESV2007 a-posteriori error estimator of P1 SWIPDG on conforming
// triangles (hdd_swipdg_estimate, abi_estimate.hip): what Estimators::SWIPDG computes after every solve
// (dune/hdd/linearelliptic/estimators/swipdg.hh; test/linearelliptic-swipdg.hh:238-241, 302-315).
//
// Two launches and the final reduction, ordered by the stream alone (no atomics):
//   oswald_vertex_kernel     a lane per vertex: the mean of the DG values around the vertex, gathered through the
//                            vertex -> DoF CSR in ascending element order (0 on the boundary)
//   esv2007_element_kernel   a lane per element: eta_NC^2, eta_R^2, the RT0 flux F_T,e of its three faces (one gather
//                            level: the face neighbours), eta_DF^2, eta_T^2; per-workgroup partial sums
//   estimate_sum_kernel      one workgroup: the partial sums in order
// Sums (ESTIMATE_WG = 256 lanes per workgroup, element e in workgroup e / 256, lane e % 256): within a workgroup the
// halving tree v[t] += v[t + s], s = 128 .. 1 (lanes without an element hold 0); the last kernel's lane t adds the
// partial sums t, t + 256, ... in order, then the same tree.  Bit-identical from call to call.
//
// Block mode (hdd_block_swipdg_estimate: the OS2014 localized estimator of Estimators::BlockSWIPDG,
// estimators/block-swipdg.hh) runs the same element code over segment-aligned chunks, four launches whatever the
// number of segments S:
//   oswald_vertex_kernel      as above
//   esv2007_element_kernel<.., block>   workgroup w finds its segment s by binary search in the chunk prefix [S + 1] and
//                            its chunk c = w - prefix[s]; lane t is element bounds[s] + 256 c + t.  Rows of d_local and of
//                            the per-chunk partials [4][C]: eta_NC,T^2, r_T = int_T (f - P0 f)^2, eta_DF,T^2 (tree sums)
//                            and m_T = min(kappa_T(theta_min), kappa_T(theta_max)) lambda_min(A_T) (tree minimum)
//   block_segment_kernel     a workgroup per segment over its *chunks* (n / 256 + S partials in all, never the
//                            elements): lane t adds the chunk sums t, t + 256, ... in order, then the tree -- a segment
//                            of one chunk is that chunk, adding zeros is exact.  Writes N_s, R_s = diam_s^2 / (pi^2
//                            min m_T) sum r_T, D_s and the indicator 3 / sqrt(alpha) (sqrt(gamma) N_s + R_s + gamma~
//                            D_s) before its division by eta^2
//   block_total_kernel       one workgroup: lane t adds N_s, R_s, D_s of the segments s = t, t + 256, ... in order,
//                            the tree, eta^2, and divides the indicators by it (eta = 0: the indicators are 0)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "swipdg_kernels.hh"

namespace hdd {
namespace dev {

constexpr int ESTIMATE_WG = 256;
constexpr int ESTIMATE_QMAX = 96;   // points of the two simplex rules of the residual together

struct EstimateArgs {
  int64_t n;                      // elements (whole-grid view: own == local)
  int64_t n_vertices;
  const int32_t* ev;              // [3][n]
  const double* vxy;              // [n_vertices][2]
  const int32_t* nbrs;            // [3][n]
  const uint32_t* finfo;          // [n]
  const int64_t* patch_ptr;       // [n_vertices + 1]
  const int32_t* patch_dof;       // DoFs 3 e + i around each vertex, ascending
  const uint8_t* vertex_bnd;      // [n_vertices]: the vertex lies on a boundary face
  const double* u;                // [3 n]
  double* oswald;                 // [n_vertices] (workspace)
  double* partial;                // [4][n_wg] (workspace)
  double* total;                  // [4] (workspace)
  double* out_local;              // nullable [4][n]
  double* out_flux;               // nullable [3][n]
  double* out_oswald;             // nullable [n_vertices]
  int32_t n_comp, tkind;
  const double* kper[HDD_MAX_COMP];   // null: the constant kconst[q]
  double kconst[HDD_MAX_COMP];
  double theta[5][HDD_MAX_COMP];      // mu (flux, residual), bar (nonconformity), hat (diffusive flux); block mode:
                                      // min, max (parameter_range_min / _max of the minimal diffusion)
  double tc[3];
  const double* tper;
  KappaArg force;
  int32_t has_force, nqa, nqb, beta_is_one;   // rule a: q[0, nqa) (element mean), rule b: q[nqa, nqa + nqb)
  int32_t residual_star, pad;       // eta_R_ESV2007_*: div t_h = sum_e F_T,e / |T| in place of P0 f
  double sigma_inner, sigma_boundary, beta;
  double q[ESTIMATE_QMAX][3];     // reference point, weight (sum 1/2)
  // block mode (n_segments > 0): `partial` is [4][n_chunks], `total` [4] = sum N_s, sum R_s, sum D_s, eta^2
  int64_t n_segments, n_chunks;
  const int64_t* seg_bounds;      // [S + 1] element bounds
  const int64_t* chunk_prefix;    // [S + 1] chunks of 256 elements before each segment
  const double* seg_diam;         // [S]
  double* segments;               // [4][S]: N_s, R_s, D_s, indicator (d_segments or workspace)
  double factor[3];               // sqrt(gamma_bar), gamma_tilde, 1 / sqrt(alpha_bar)
};
static_assert(sizeof(EstimateArgs) <= 4096, "EstimateArgs is passed by value: the kernel-argument limit");

inline int64_t estimate_workgroups(int64_t n) { return n > 0 ? (n + ESTIMATE_WG - 1) / ESTIMATE_WG : 1; }

// both kernels and the reduction on `s`; *names: the instantiations that ran
hipError_t launch_estimate(const EstimateArgs& a, hipStream_t s, const char** names);
// block mode: the four launches above
hipError_t launch_estimate_blocks(const EstimateArgs& a, hipStream_t s, const char** names);

}  // namespace dev
}  // namespace hdd
