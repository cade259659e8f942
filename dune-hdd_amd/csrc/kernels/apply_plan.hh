// dune-hdd_amd/csrc/kernels/apply_plan.hh -- the checked plan of an operator application (internal): what
// hdd_operator_apply / _apply2 (abi_apply.hip, which defines these functions) and hdd_operator_solve (abi_solve.hip)
// share, so that the operator arguments are checked and dispatched in one place.
#pragma once
#include <algorithm>
#include <cstdint>

#include "abi_common.hh"
#include "apply_kernels.hh"

#pragma GCC visibility push(hidden)   // internal: none of this is an exported symbol
namespace hdd {
namespace abi {

struct ApplyPlan {
  dev::ApplyArgs a;
  bool tile;
  int nb, nf;        // tile path
  bool short_rows;   // generic path: a group of 8 lanes per row instead of a wave
};

// Every check of hdd_operator_apply's operator arguments (no device call, nothing dereferenced but host structs);
// fills the plan except x / y.
int plan_apply(const char* who, hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
               int32_t n_comp, const double* theta, const hdd_block_range* range, ApplyPlan& P);

// the launches of a checked plan: the values are read once per group of APPLY_NV vectors
int run_apply(const char* who, hdd_ctx* ctx, ApplyPlan& P, const double* d_x, int64_t ldx, double* d_y, int64_t ldy,
              int32_t n_vec, void* stream);

// A theta per vector (hdd_operator_apply_multi / _solve_multi): the plan of (theta row 0 or ones), then the tile path
// only where the n_comp component images fit the LDS a launch gets by default (P1: n_comp <= 3, Q1: n_comp == 1);
// what does not fit takes the CSR kernel, whose arrays the pattern must then have.
int plan_apply_multi(const char* who, hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                     int32_t n_comp, const double* theta, const hdd_block_range* range, ApplyPlan& P);
inline bool apply_multi_tile_fits(int nb, int n_comp) { return nb == 3 ? n_comp <= 3 : n_comp == 1; }

// the kernel arguments of one group: vector v < nv gets theta[(v0 + v) * ldt + q] (theta NULL: ones), the others
// copies of the group's first
void apply_multi_thetas(dev::ApplyMultiArgs& ma, const double* theta, int64_t ldt, int v0);

// the launches of a checked multi plan, the values read once per group of APPLY_NV vectors
int run_apply_multi(const char* who, hdd_ctx* ctx, ApplyPlan& P, const double* theta, int64_t ldt, const double* d_x, int64_t ldx,
                    double* d_y, int64_t ldy, int32_t n_vec, void* stream);

// workgroups of the tile kernel: as many waves per CU as LDS images fit (8 P1, 4 Q1 of the 160 KB); tile_range wants
// a multiple of 8 workgroups
template <int NB, int NF>
inline int64_t apply_tile_grid(const hdd_ctx* ctx, int64_t n_tiles)
{
  using I = dev::ApplyImage<NB, NF>;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / I::BYTES));
  const int64_t G = std::max<int64_t>(8, (int64_t(ctx->n_cu) * per_cu) & ~int64_t(7));
  return G >= n_tiles ? n_tiles : G;
}

// workgroups of the CSR kernel with G lanes per row
template <int G>
inline int64_t apply_csr_grid(int64_t n_rows)
{
  const int64_t per_wg = 256 / G;
  return std::min<int64_t>((n_rows + per_wg - 1) / per_wg, 256 * 64);
}

}  // namespace abi
}  // namespace hdd
#pragma GCC visibility pop
