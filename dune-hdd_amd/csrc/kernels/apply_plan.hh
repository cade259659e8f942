// dune-hdd_amd/csrc/kernels/apply_plan.hh -- the checked plan of an operator application (internal): what
// hdd_operator_apply / _apply_multi / _apply2 (abi_apply.hip, which defines the functions declared here) and
// hdd_operator_solve[_batched / _multi / _blocks] (abi_solve.hip) share, so that the operator arguments are checked in one
// place (plan_apply) and every apply kernel is launched from one place (launch_apply).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>

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
  int64_t rows() const { return a.row_end - a.row_begin; }
  int64_t n_tiles() const { return (a.e_end - a.e_begin + 63) / 64; }
  int image_bytes() const { return nb == 3 ? dev::ApplyImage<3, 3>::BYTES : dev::ApplyImage<4, 4>::BYTES; }
};

// a theta per vector: theta[j * ldt + q] for vector j (theta NULL: ones)
struct ApplyThetas {
  const double* theta;
  int64_t ldt;
};

// Every check of hdd_operator_apply's operator arguments (no device call, nothing dereferenced but host structs);
// fills the plan except x / y.  per_vector (hdd_operator_apply_multi / _solve_multi; theta is then not read: ones):
// the tile path only where the n_comp component images fit the LDS a launch gets by default (P1: n_comp <= 3, Q1:
// n_comp == 1); what does not fit takes the CSR kernel, whose arrays the pattern must then have.
int plan_apply(const char* who, hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
               int32_t n_comp, const double* theta, const hdd_block_range* range, ApplyPlan& P, bool per_vector = false);

// the kernel arguments of one group: vector v < nv gets theta[(v0 + v) * ldt + q] (theta NULL: ones), the others
// copies of the group's first
void apply_multi_thetas(dev::ApplyMultiArgs& ma, const ApplyThetas& T, int v0);

// the launches of a checked plan: the values are read once per group of APPLY_NV vectors.  T NULL: the plan's theta
// for every vector.
int run_apply(const char* who, hdd_ctx* ctx, const ApplyPlan& P, const ApplyThetas* T, const double* d_x, int64_t ldx,
              double* d_y, int64_t ldy, int32_t n_vec, void* stream);

// "apply_tile_kernel<3, 3, 4>", "apply_csr_multi_kernel<8, 4, dot>", ...: the instantiation launch_apply<nv, dot>
// takes for the plan, appended to out
void apply_kernel_name(std::string& out, const ApplyPlan& P, bool per_vector, int nv, bool dot);

// hdd_operator_project (abi_project.hip): names the plan's "project_tile_kernel<3, 3>", "project_csr_kernel<8>", ...
// as this thread's last apply kernel
void name_project_kernel(const ApplyPlan& P);

// Workgroups of a plain launch.  Tile kernel: as many waves per CU as LDS images fit (8 P1, 4 Q1 of the 160 KB),
// tile_range wants a multiple of 8 workgroups; CSR kernel: 256 / G rows per workgroup pass.
inline int64_t apply_grid(const hdd_ctx* ctx, const ApplyPlan& P)
{
  if (P.tile) {
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / P.image_bytes()));
    const int64_t G = std::max<int64_t>(8, (int64_t(ctx->n_cu) * per_cu) & ~int64_t(7));
    return G >= P.n_tiles() ? P.n_tiles() : G;
  }
  const int64_t per_wg = 256 / (P.short_rows ? 8 : 64);
  return std::min<int64_t>((P.rows() + per_wg - 1) / per_wg, 256 * 64);
}

// workgroups of a DOT launch (= partial sums per vector it writes, at most max_parts)
inline int64_t dot_grid(const hdd_ctx* ctx, const ApplyPlan& P, int64_t max_parts)
{
  const int64_t G = apply_grid(ctx, P);
  if (!P.tile) return std::min<int64_t>(G, 2048);
  return G > max_parts ? max_parts & ~int64_t(7) : G;   // tile_range: a multiple of 8 below the tile count
}

// One launch of a checked plan on `grid` workgroups for args.nv <= NV vectors: tile NB 3 / 4 (times the component
// images) or CSR 8 / 64.  Args is dev::ApplyArgs (the plan's theta) or dev::ApplyMultiArgs (a theta per vector).
template <int NV, bool DOT, class Args>
hipError_t launch_apply(const ApplyPlan& P, const Args& args, int64_t grid, hipStream_t s)
{
  constexpr bool PER_VECTOR = std::is_same_v<Args, dev::ApplyMultiArgs>;
  const dim3 g{unsigned(grid)};
  auto tile = [&](auto nb, auto nc) {
    constexpr int NB = decltype(nb)::value, NC = decltype(nc)::value;
    using I = dev::ApplyImage<NB, NB>;   // P1: 3 values, 3 faces; Q1: 4 and 4
    static_assert(std::max(NC, 1) * I::BYTES <= 64 * 1024, "the dynamic LDS a launch gets without raising the kernel's attribute");
    if constexpr (PER_VECTOR)
      hipLaunchKernelGGL((dev::apply_tile_multi_kernel<NB, NB, NV, DOT, NC>), g, dim3(64), NC * I::BYTES, s, args, P.n_tiles());
    else
      hipLaunchKernelGGL((dev::apply_tile_kernel<NB, NB, NV, DOT>), g, dim3(64), I::BYTES, s, args, P.n_tiles());
  };
  auto csr = [&](auto lanes) {
    constexpr int G = decltype(lanes)::value;
    if constexpr (PER_VECTOR) hipLaunchKernelGGL((dev::apply_csr_multi_kernel<G, NV, DOT>), g, dim3(256), 0, s, args);
    else hipLaunchKernelGGL((dev::apply_csr_kernel<G, NV, DOT>), g, dim3(256), 0, s, args);
  };
  using std::integral_constant;
  constexpr integral_constant<int, PER_VECTOR ? 1 : 0> one{};   // NC: the plan's theta has the combined image (0)
  int images = 1;   // component images of a P1 tile (plan_apply: at most 3; Q1: 1)
  if constexpr (PER_VECTOR) images = args.a.n_comp;
  if (P.tile && P.nb == 3) {
    if (images == 1) tile(integral_constant<int, 3>{}, one);
    else if (images == 2) tile(integral_constant<int, 3>{}, integral_constant<int, 2>{});
    else tile(integral_constant<int, 3>{}, integral_constant<int, 3>{});
  } else if (P.tile)
    tile(integral_constant<int, 4>{}, one);
  else if (P.short_rows)
    csr(integral_constant<int, 8>{});
  else
    csr(integral_constant<int, 64>{});
  return hipGetLastError();
}

// ---- the block-diagonal part with respect to row segments (hdd_operator_apply_blocks / _solve_blocks) -------------

// The checks of n_blocks and bounds (host [n_blocks + 1]), then plan_apply on the square range of the whole interval
// (bounds[0], bounds[n_blocks]).  The tile kernel only where every bound is a multiple of nb -- where the single call
// on every segment's range would take it; else the CSR kernel, whose arrays the pattern must then have.
int plan_blocks(const char* who, hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                int32_t n_comp, const double* theta, int32_t n_blocks, const int64_t* bounds, ApplyPlan& P);

// The table of a checked blocks plan (dev::BlockSegment, host memory [n_blocks]): per segment the ranges and, per kind
// of launch, the grid a call on the segment alone has (BLOCKS_APPLY: apply_grid, BLOCKS_DOT: dot_grid with max_parts;
// with block_size > 0 also the solve's update and direction grids, else 1) and their prefix sums.  total: the real
// workgroups of a launch of each kind.
void blocks_table(const hdd_ctx* ctx, const ApplyPlan& P, int32_t n_blocks, const int64_t* bounds, int block_size, int64_t max_parts,
                  dev::BlockSegment* tab, int64_t (&total)[dev::BLOCKS_KINDS]);

// "apply_tile_blocks_kernel<3, 3, dot>", "apply_csr_blocks_kernel<8>", ... appended to out
void apply_blocks_kernel_name(std::string& out, const ApplyPlan& P, bool dot);

// One launch for every segment of the table at B.seg (device), `grid` = total[B.kind] workgroups, one vector
template <bool DOT>
hipError_t launch_apply_blocks(const ApplyPlan& P, const dev::ApplyArgs& a, const dev::BlocksArgs& B, int64_t grid, hipStream_t s)
{
  const dim3 g{unsigned(grid)};
  if (P.tile && P.nb == 3)
    hipLaunchKernelGGL((dev::apply_tile_blocks_kernel<3, 3, DOT>), g, dim3(64), (dev::ApplyImage<3, 3>::BYTES), s, a, B);
  else if (P.tile)
    hipLaunchKernelGGL((dev::apply_tile_blocks_kernel<4, 4, DOT>), g, dim3(64), (dev::ApplyImage<4, 4>::BYTES), s, a, B);
  else if (P.short_rows)
    hipLaunchKernelGGL((dev::apply_csr_blocks_kernel<8, DOT>), g, dim3(256), 0, s, a, B);
  else
    hipLaunchKernelGGL((dev::apply_csr_blocks_kernel<64, DOT>), g, dim3(256), 0, s, a, B);
  return hipGetLastError();
}

// y_s = A_ss x_s for every segment: the plain launch (kind BLOCKS_APPLY) on the device table d_tab; x, y are the
// interval's vectors.  Names the kernel for hdd_last_apply_kernel().
int run_apply_blocks(const char* who, hdd_ctx* ctx, const ApplyPlan& P, const dev::BlockSegment* d_tab, int32_t n_blocks, int64_t grid,
                     const double* d_x, double* d_y, void* stream);

}  // namespace abi
}  // namespace hdd
#pragma GCC visibility pop
