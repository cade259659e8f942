// dune-hdd_amd/csrc/kernels/abi_solve.hip -- C ABI: hdd_operator_solve, block-Jacobi preconditioned conjugate
// gradients on sum_q theta_q A_q (kernels in solve_kernels.hh and the DOT variants of apply_kernels.hh): the
// apply_inverse of ContainerBasedDefault::uncached_solve (base.hh:327-367) on the device.  The operator arguments are
// checked and dispatched by plan_apply (apply_plan.hh), as hdd_operator_apply's.  hdd_operator_solve_batched, the same
// iteration for up to HDD_MAX_VEC right-hand sides in groups of APPLY_NV, is the second half of the file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "apply_plan.hh"
#include "solve_kernels.hh"

using hdd::abi::ApplyPlan;
using hdd::abi::fail;
namespace dev = hdd::dev;

namespace {
std::string& last_solve_kernels_slot()
{
  thread_local std::string names;
  return names;
}

// the build has -ffinite-math-only, under which a test for NaN is folded away, on the value and on its bits alike:
// the bits are read behind an optimisation barrier
bool negative_or_nan(const double* v)
{
  uint64_t u;
  std::memcpy(&u, v, sizeof u);
  asm volatile("" : "+r"(u));
  const bool nan = ((u >> 52) & 0x7ff) == 0x7ff && (u & ((uint64_t(1) << 52) - 1)) != 0;
  return nan || ((u >> 63) != 0 && (u << 1) != 0);
}

int64_t even(int64_t n) { return n + (n & 1); }
int64_t packed(int bs) { return int64_t(bs) * (bs + 1) / 2; }

int64_t workspace_doubles(int64_t rows, int bs)
{
  // state, four kinds of partial sums, p q r z (each starting 16-byte aligned), the packed inverse blocks
  return int64_t(sizeof(dev::SolveState) / 8) + 4 * int64_t(dev::SOLVE_PARTS) + 4 * even(rows) + even(rows / bs * packed(bs));
}

int64_t update_grid(int64_t n_blk) { return std::max<int64_t>(1, std::min<int64_t>((n_blk + 255) / 256, 2048)); }

struct Solve {
  ApplyPlan P;
  dev::SolveVectors v;
  int bs;
  bool pre, a16, dinv_tile;
  hipStream_t s;
};

template <int NB, int NF>
void launch_tile_dot(const hdd_ctx* ctx, const dev::ApplyArgs& a, int64_t G, hipStream_t s)
{
  using I = dev::ApplyImage<NB, NF>;
  const int64_t n_tiles = (a.e_end - a.e_begin + 63) / 64;
  hipLaunchKernelGGL((dev::apply_tile_kernel<NB, NF, 1, true>), dim3(unsigned(G)), dim3(64), I::BYTES, s, a, n_tiles);
}

// workgroups of the DOT apply (= partial sums it writes)
int64_t dot_grid(const hdd_ctx* ctx, const ApplyPlan& P)
{
  const int64_t rows = P.a.row_end - P.a.row_begin;
  int64_t G;
  if (P.tile) {
    const int64_t n_tiles = (P.a.e_end - P.a.e_begin + 63) / 64;
    G = P.nb == 3 ? hdd::abi::apply_tile_grid<3, 3>(ctx, n_tiles) : hdd::abi::apply_tile_grid<4, 4>(ctx, n_tiles);
    if (G > dev::SOLVE_PARTS) G = dev::SOLVE_PARTS & ~7;   // tile_range: a multiple of 8 below the tile count
  } else {
    G = std::min<int64_t>(P.short_rows ? hdd::abi::apply_csr_grid<8>(rows) : hdd::abi::apply_csr_grid<64>(rows), 2048);
  }
  return G;
}

// q = A p with p . q into part_pq, iteration k
hipError_t launch_apply_dot(const hdd_ctx* ctx, const Solve& S, int k)
{
  dev::ApplyArgs a = S.P.a;
  a.nv = 1;
  a.x = S.v.p;
  a.y = S.v.q;
  a.ldx = a.ldy = S.v.n;
  a.partial = S.v.part_pq;
  a.done_at = &S.v.state->done_at;
  a.iteration = k;
  const int64_t G = S.v.n_pq;
  if (S.P.tile) {
    if (S.P.nb == 3) launch_tile_dot<3, 3>(ctx, a, G, S.s);
    else launch_tile_dot<4, 4>(ctx, a, G, S.s);
  } else if (S.P.short_rows) {
    hipLaunchKernelGGL((dev::apply_csr_kernel<8, 1, true>), dim3(unsigned(G)), dim3(256), 0, S.s, a);
  } else {
    hipLaunchKernelGGL((dev::apply_csr_kernel<64, 1, true>), dim3(unsigned(G)), dim3(256), 0, S.s, a);
  }
  return hipGetLastError();
}

template <int BS>
hipError_t launch_dinv(const Solve& S, double* dinv, int64_t grid)
{
  if (S.dinv_tile) {
    if constexpr (BS == 3) hipLaunchKernelGGL((dev::solve_dinv_tile_kernel<3, 3>), dim3(unsigned(grid)), dim3(256), 0, S.s, S.P.a, dinv, S.v.part_pq);
    if constexpr (BS == 4) hipLaunchKernelGGL((dev::solve_dinv_tile_kernel<4, 4>), dim3(unsigned(grid)), dim3(256), 0, S.s, S.P.a, dinv, S.v.part_pq);
  } else {
    hipLaunchKernelGGL((dev::solve_dinv_csr_kernel<BS>), dim3(unsigned(grid)), dim3(256), 0, S.s, S.P.a, dinv, S.v.part_pq);
  }
  return hipGetLastError();
}

template <int BS, bool PRE, bool A16>
hipError_t launch_init(const Solve& S, const double* b, bool x0, int64_t grid)
{
  hipLaunchKernelGGL((dev::cg_init_kernel<BS, PRE, A16>), dim3(unsigned(grid)), dim3(256), 0, S.s, S.v, b, x0);
  return hipGetLastError();
}

template <int BS, bool PRE, bool A16>
hipError_t launch_update(const Solve& S, int k, int64_t grid)
{
  hipLaunchKernelGGL((dev::cg_update_kernel<BS, PRE, A16>), dim3(unsigned(grid)), dim3(256), 0, S.s, S.v, k);
  return hipGetLastError();
}

enum Stage { DINV, INIT, UPDATE };

template <int BS>
hipError_t launch_bs(const Solve& S, Stage st, const double* b, bool x0, int k, int64_t grid)
{
  if (st == DINV) return launch_dinv<BS>(S, const_cast<double*>(S.v.dinv), grid);
  constexpr bool EVEN = BS % 2 == 0;
  if (st == INIT) {
    if (S.pre) return S.a16 && EVEN ? launch_init<BS, true, EVEN>(S, b, x0, grid) : launch_init<BS, true, false>(S, b, x0, grid);
    return S.a16 && EVEN ? launch_init<BS, false, EVEN>(S, b, x0, grid) : launch_init<BS, false, false>(S, b, x0, grid);
  }
  if (S.pre) return S.a16 && EVEN ? launch_update<BS, true, EVEN>(S, k, grid) : launch_update<BS, true, false>(S, k, grid);
  return S.a16 && EVEN ? launch_update<BS, false, EVEN>(S, k, grid) : launch_update<BS, false, false>(S, k, grid);
}

hipError_t launch_stage(const Solve& S, Stage st, const double* b, bool x0, int k, int64_t grid)
{
  switch (S.bs) {
    case 1: return launch_bs<1>(S, st, b, x0, k, grid);
    case 2: return launch_bs<2>(S, st, b, x0, k, grid);
    case 3: return launch_bs<3>(S, st, b, x0, k, grid);
    case 4: return launch_bs<4>(S, st, b, x0, k, grid);
    case 5: return launch_bs<5>(S, st, b, x0, k, grid);
    case 6: return launch_bs<6>(S, st, b, x0, k, grid);
    case 7: return launch_bs<7>(S, st, b, x0, k, grid);
    default: return launch_bs<8>(S, st, b, x0, k, grid);
  }
}
}  // namespace

extern "C" const char* hdd_last_solve_kernels(void) { return last_solve_kernels_slot().c_str(); }

extern "C" int64_t hdd_operator_solve_workspace(int64_t rows, int32_t block_size)
{
  if (rows < 0 || block_size < 0 || block_size > 8) return 0;
  // block_size 0 (the mesh's nb, unknown here): enough for every block size
  int64_t w = 0;
  for (int bs = block_size ? block_size : 1; bs <= (block_size ? block_size : 8); ++bs) w = std::max(w, workspace_doubles(rows, bs));
  return w;
}

extern "C" int hdd_operator_solve(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                  int32_t n_comp, const double* theta, const hdd_block_range* range, const double* d_b,
                                  double* d_x, const hdd_solve_options* opt, double* d_work, int64_t n_work,
                                  double* d_history, hdd_solve_info* info, void* stream)
{
  const char* who = "hdd_operator_solve";
  if (!d_b || !d_x || !opt || !d_work || !info) return fail(HDD_ERR_INVALID, who, "null argument");
  Solve S;
  if (int rc = hdd::abi::plan_apply(who, ctx, mesh, pattern, d_vals, n_comp, theta, range, S.P)) return rc;
  const dev::ApplyArgs& a = S.P.a;
  if (a.row_begin != a.col_begin || a.row_end != a.col_end)
    return fail(HDD_ERR_INVALID, who, "the whole (square) matrix or a square diagonal range expected");
  if (opt->max_iter < 0) return fail(HDD_ERR_INVALID, who, "max_iter negative");
  if (negative_or_nan(&opt->rtol) || negative_or_nan(&opt->atol)) return fail(HDD_ERR_INVALID, who, "rtol / atol negative or NaN");
  if (opt->check_every < 0) return fail(HDD_ERR_INVALID, who, "check_every negative");
  if (opt->precond != HDD_PRECOND_NONE && opt->precond != HDD_PRECOND_BLOCK_JACOBI)
    return fail(HDD_ERR_INVALID, who, "unknown precond");
  if (opt->block_size < 0 || opt->block_size > 8) return fail(HDD_ERR_INVALID, who, "block_size outside 0..8");
  int bs = opt->block_size;
  const int mesh_nb = mesh && hdd::abi::mesh_faces(mesh->elem_type)
                          ? hdd::abi::mesh_nb(mesh->elem_type, mesh->elem_type == HDD_HEX ? std::max(1, int(mesh->degree)) : 1)
                          : 0;
  if (bs == 0) {
    if (mesh_nb < 1 || mesh_nb > 8) return fail(HDD_ERR_INVALID, who, "block_size 0 needs a mesh with nb <= 8");
    bs = mesh_nb;
  }
  const int64_t rows = a.row_end - a.row_begin;
  if (a.row_begin % bs != 0 || rows % bs != 0)
    return fail(HDD_ERR_INVALID, who, "the bounds of the range are not multiples of block_size");
  if (n_work < workspace_doubles(rows, bs)) return fail(HDD_ERR_INVALID, who, "n_work smaller than hdd_operator_solve_workspace");
  S.bs = bs;
  S.pre = opt->precond == HDD_PRECOND_BLOCK_JACOBI;
  S.dinv_tile = S.P.tile && bs == S.P.nb;
  if (S.pre && !S.dinv_tile && (!pattern->row_ptr || !pattern->col))
    return fail(HDD_ERR_INVALID, who, "pattern without row_ptr / col (block_size != nb of the mesh)");
  if (!ctx->solve_state_h) return fail(HDD_ERR_INVALID, who, "context without its state buffer");
  // ---- every argument check is above; device calls from here ----
  *info = hdd_solve_info{HDD_SOLVE_CONVERGED, 0, 0.0, 0.0};
  last_solve_kernels_slot().clear();
  if (rows == 0) return HDD_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  S.s = static_cast<hipStream_t>(stream);
  double* w = d_work;
  dev::SolveVectors& v = S.v;
  v.state = reinterpret_cast<dev::SolveState*>(w); w += sizeof(dev::SolveState) / 8;
  v.part_pq = w; w += dev::SOLVE_PARTS;
  v.part_rz = w; w += dev::SOLVE_PARTS;
  v.part_rr = w; w += dev::SOLVE_PARTS;
  v.part_bb = w; w += dev::SOLVE_PARTS;
  v.p = w; w += even(rows);
  v.q = w; w += even(rows);
  v.r = w; w += even(rows);
  v.z = S.pre ? w : v.r; w += even(rows);
  v.dinv = w;
  v.x = d_x;
  v.n = rows;
  v.n_pq = int32_t(dot_grid(ctx, S.P));
  v.history = d_history;
  S.a16 = reinterpret_cast<uintptr_t>(d_work) % 16 == 0 && reinterpret_cast<uintptr_t>(d_x) % 16 == 0;
  const bool x0 = (opt->flags & HDD_SOLVE_X0) != 0;
  const int64_t n_blk = rows / bs;
  const int64_t ugrid = update_grid(n_blk);
  const int64_t dgrid = std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, 4096));

  // names of the iteration's kernels
  {
    std::string& nm = last_solve_kernels_slot();
    if (S.P.tile) nm = S.P.nb == 3 ? "apply_tile_kernel<3, 3, 1, dot>" : "apply_tile_kernel<4, 4, 1, dot>";
    else nm = S.P.short_rows ? "apply_csr_kernel<8, 1, dot>" : "apply_csr_kernel<64, 1, dot>";
    nm += " + cg_update<" + std::to_string(bs) + (S.pre ? ">" : ", none>") + " + cg_direction";
  }

  // ---- setup: inverse diagonal blocks, r = b - A x0, the state ----
  int n_bad = 0;
  if (S.pre) {
    n_bad = int(ugrid);
    e = launch_stage(S, DINV, nullptr, false, 0, ugrid);
    if (e != hipSuccess) return hip_fail(e, who);
  }
  if (x0)
    if (int rc = hdd::abi::run_apply(who, ctx, S.P, d_x, rows, v.q, rows, 1, stream)) return rc;
  e = launch_stage(S, INIT, d_b, x0, 0, ugrid);
  if (e != hipSuccess) return hip_fail(e, who);
  hipLaunchKernelGGL(dev::cg_init_state_kernel, dim3(1), dim3(64), 0, S.s, v, int(ugrid), n_bad, opt->rtol, opt->atol);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, who);

  // ---- iterations: min(check_every, remaining) enqueued between two looks at the state ----
  const int every = opt->check_every > 0 ? opt->check_every : 32;
  dev::SolveState* h = reinterpret_cast<dev::SolveState*>(ctx->solve_state_h);
  int k = 0;
  for (;;) {
    const int batch = std::min(every, opt->max_iter - k);
    for (int i = 0; i < batch; ++i, ++k) {
      e = launch_apply_dot(ctx, S, k);
      if (e == hipSuccess) e = launch_stage(S, UPDATE, nullptr, false, k, ugrid);
      if (e != hipSuccess) return hip_fail(e, who);
      if (S.pre) hipLaunchKernelGGL(dev::cg_direction_kernel<true>, dim3(unsigned(dgrid)), dim3(256), 0, S.s, v, k, int(ugrid));
      else hipLaunchKernelGGL(dev::cg_direction_kernel<false>, dim3(unsigned(dgrid)), dim3(256), 0, S.s, v, k, int(ugrid));
      e = hipGetLastError();
      if (e != hipSuccess) return hip_fail(e, who);
    }
    e = hipMemcpyAsync(h, v.state, sizeof(dev::SolveState), hipMemcpyDeviceToHost, S.s);
    if (e == hipSuccess) e = hipStreamSynchronize(S.s);
    if (e != hipSuccess) return hip_fail(e, who);
    if (h->done_at <= k || k >= opt->max_iter) break;
  }
  const bool done = h->done_at <= k;
  info->status = done ? h->status : HDD_SOLVE_MAX_ITER;
  info->iterations = h->iteration;
  info->residual = std::sqrt(h->rr);
  info->rhs_norm = std::sqrt(h->bb);
  if (h->flags & dev::SOLVE_FLAG_ZERO_RHS) {   // b = 0: x = 0 whatever the initial guess was
    e = hipMemsetAsync(d_x, 0, size_t(rows) * sizeof(double), S.s);
    if (e == hipSuccess) e = hipStreamSynchronize(S.s);
    if (e != hipSuccess) return hip_fail(e, who);
    info->residual = 0.0;
  }
  return HDD_OK;
}

// ---- several right-hand sides per call ------------------------------------------------------------------------------
// Columns in groups of APPLY_NV (solve_kernels.hh).  Setup and iteration are those of hdd_operator_solve: the inverse
// blocks once, r = b - A x0 by the multi-vector plain apply, cg_init_kernel per column on the single solve's grid; per
// iteration and group the DOT apply on dot_grid, cg_update_batched on update_grid, cg_direction_batched.
namespace {
constexpr int NVB = dev::APPLY_NV;
constexpr int64_t BATCH_HEAD = int64_t(hdd_ctx::SOLVE_STATE_BYTES / 8);   // states of HDD_MAX_VEC columns, the group words

int64_t batched_workspace_doubles(int64_t rows, int bs, int n_rhs)
{
  // states and stop words, four kinds of partial sums per column, p q r z per column (each starting 16-byte
  // aligned), the packed inverse blocks once
  return BATCH_HEAD + int64_t(n_rhs) * (4 * int64_t(dev::SOLVE_PARTS) + 4 * even(rows)) + even(rows / bs * packed(bs));
}

struct Batch {
  ApplyPlan P;
  dev::SolveBatch g;   // group 0; launch_group offsets it
  int bs, n_rhs;
  bool pre, a16;
  int64_t n_parts;     // workgroups of the update launch
  hipStream_t s;
};

dev::SolveBatch group_of(const Batch& B, int g0)
{
  dev::SolveBatch v = B.g;
  v.nv = std::min(NVB, B.n_rhs - g0);
  v.state += g0;
  v.stop += g0 / NVB;
  v.x += int64_t(g0) * v.ldx;
  v.p += int64_t(g0) * v.ldw;
  v.q += int64_t(g0) * v.ldw;
  v.r += int64_t(g0) * v.ldw;
  v.z += int64_t(g0) * v.ldw;
  v.part_pq += int64_t(g0) * v.n_pq;
  v.part_rz += int64_t(g0) * B.n_parts;
  v.part_rr += int64_t(g0) * B.n_parts;
  if (v.history) v.history += int64_t(g0) * v.ldh;
  return v;
}

hipError_t launch_apply_dot_batched(const hdd_ctx* ctx, const Batch& B, const dev::SolveBatch& v, int k)
{
  dev::ApplyArgs a = B.P.a;
  a.nv = v.nv;
  a.x = v.p;
  a.y = v.q;
  a.ldx = a.ldy = v.ldw;
  a.partial = v.part_pq;
  a.done_at = v.stop;
  a.iteration = k;
  const unsigned G = unsigned(v.n_pq);   // dot_grid of the single solve: the bits of p . q rest on it
  if (B.P.tile) {
    const int64_t n_tiles = (a.e_end - a.e_begin + 63) / 64;
    if (B.P.nb == 3)
      hipLaunchKernelGGL((dev::apply_tile_kernel<3, 3, NVB, true>), dim3(G), dim3(64), (dev::ApplyImage<3, 3>::BYTES), B.s, a, n_tiles);
    else
      hipLaunchKernelGGL((dev::apply_tile_kernel<4, 4, NVB, true>), dim3(G), dim3(64), (dev::ApplyImage<4, 4>::BYTES), B.s, a, n_tiles);
  } else if (B.P.short_rows) {
    hipLaunchKernelGGL((dev::apply_csr_kernel<8, NVB, true>), dim3(G), dim3(256), 0, B.s, a);
  } else {
    hipLaunchKernelGGL((dev::apply_csr_kernel<64, NVB, true>), dim3(G), dim3(256), 0, B.s, a);
  }
  return hipGetLastError();
}

template <int BS, bool PRE, bool A16>
hipError_t launch_update_batched(const Batch& B, const dev::SolveBatch& v, int k)
{
  hipLaunchKernelGGL((dev::cg_update_batched_kernel<BS, PRE, A16, NVB>), dim3(unsigned(B.n_parts)), dim3(256), 0, B.s, v, k);
  return hipGetLastError();
}

template <int BS>
hipError_t launch_update_batched_bs(const Batch& B, const dev::SolveBatch& v, int k)
{
  constexpr bool EVEN = BS % 2 == 0;
  if (B.pre) return B.a16 && EVEN ? launch_update_batched<BS, true, EVEN>(B, v, k) : launch_update_batched<BS, true, false>(B, v, k);
  return B.a16 && EVEN ? launch_update_batched<BS, false, EVEN>(B, v, k) : launch_update_batched<BS, false, false>(B, v, k);
}

hipError_t launch_update_batched_any(const Batch& B, const dev::SolveBatch& v, int k)
{
  switch (B.bs) {
    case 1: return launch_update_batched_bs<1>(B, v, k);
    case 2: return launch_update_batched_bs<2>(B, v, k);
    case 3: return launch_update_batched_bs<3>(B, v, k);
    case 4: return launch_update_batched_bs<4>(B, v, k);
    case 5: return launch_update_batched_bs<5>(B, v, k);
    case 6: return launch_update_batched_bs<6>(B, v, k);
    case 7: return launch_update_batched_bs<7>(B, v, k);
    default: return launch_update_batched_bs<8>(B, v, k);
  }
}
}  // namespace

extern "C" int64_t hdd_operator_solve_batched_workspace(int64_t rows, int32_t block_size, int32_t n_rhs)
{
  if (rows < 0 || block_size < 0 || block_size > 8 || n_rhs < 1 || n_rhs > HDD_MAX_VEC) return 0;
  int64_t w = 0;
  for (int bs = block_size ? block_size : 1; bs <= (block_size ? block_size : 8); ++bs)
    w = std::max(w, batched_workspace_doubles(rows, bs, n_rhs));
  return w;
}

extern "C" int hdd_operator_solve_batched(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                          int32_t n_comp, const double* theta, const hdd_block_range* range, const double* d_b,
                                          int64_t ldb, double* d_x, int64_t ldx, int32_t n_rhs, const hdd_solve_options* opt,
                                          double* d_work, int64_t n_work, double* d_history, int64_t ldh, hdd_solve_info* info,
                                          void* stream)
{
  const char* who = "hdd_operator_solve_batched";
  if (!d_b || !d_x || !opt || !d_work || !info) return fail(HDD_ERR_INVALID, who, "null argument");
  if (n_rhs < 1 || n_rhs > HDD_MAX_VEC) return fail(HDD_ERR_INVALID, who, "n_rhs outside 1..HDD_MAX_VEC");
  Batch B;
  if (int rc = hdd::abi::plan_apply(who, ctx, mesh, pattern, d_vals, n_comp, theta, range, B.P)) return rc;
  const dev::ApplyArgs& a = B.P.a;
  if (a.row_begin != a.col_begin || a.row_end != a.col_end)
    return fail(HDD_ERR_INVALID, who, "the whole (square) matrix or a square diagonal range expected");
  if (opt->max_iter < 0) return fail(HDD_ERR_INVALID, who, "max_iter negative");
  if (negative_or_nan(&opt->rtol) || negative_or_nan(&opt->atol)) return fail(HDD_ERR_INVALID, who, "rtol / atol negative or NaN");
  if (opt->check_every < 0) return fail(HDD_ERR_INVALID, who, "check_every negative");
  if (opt->precond != HDD_PRECOND_NONE && opt->precond != HDD_PRECOND_BLOCK_JACOBI)
    return fail(HDD_ERR_INVALID, who, "unknown precond");
  if (opt->block_size < 0 || opt->block_size > 8) return fail(HDD_ERR_INVALID, who, "block_size outside 0..8");
  int bs = opt->block_size;
  const int mesh_nb = mesh && hdd::abi::mesh_faces(mesh->elem_type)
                          ? hdd::abi::mesh_nb(mesh->elem_type, mesh->elem_type == HDD_HEX ? std::max(1, int(mesh->degree)) : 1)
                          : 0;
  if (bs == 0) {
    if (mesh_nb < 1 || mesh_nb > 8) return fail(HDD_ERR_INVALID, who, "block_size 0 needs a mesh with nb <= 8");
    bs = mesh_nb;
  }
  const int64_t rows = a.row_end - a.row_begin;
  if (a.row_begin % bs != 0 || rows % bs != 0)
    return fail(HDD_ERR_INVALID, who, "the bounds of the range are not multiples of block_size");
  if (ldb < rows || ldx < rows) return fail(HDD_ERR_INVALID, who, "ldb / ldx smaller than the range");
  if (d_history && ldh < int64_t(opt->max_iter) + 1) return fail(HDD_ERR_INVALID, who, "ldh smaller than max_iter + 1");
  if (n_work < batched_workspace_doubles(rows, bs, n_rhs))
    return fail(HDD_ERR_INVALID, who, "n_work smaller than hdd_operator_solve_batched_workspace");
  B.bs = bs;
  B.n_rhs = n_rhs;
  B.pre = opt->precond == HDD_PRECOND_BLOCK_JACOBI;
  const bool dinv_tile = B.P.tile && bs == B.P.nb;
  if (B.pre && !dinv_tile && (!pattern->row_ptr || !pattern->col))
    return fail(HDD_ERR_INVALID, who, "pattern without row_ptr / col (block_size != nb of the mesh)");
  if (!ctx->solve_state_h) return fail(HDD_ERR_INVALID, who, "context without its state buffer");
  // ---- every argument check is above; device calls from here ----
  for (int c = 0; c < n_rhs; ++c) info[c] = hdd_solve_info{HDD_SOLVE_CONVERGED, 0, 0.0, 0.0};
  last_solve_kernels_slot().clear();
  if (rows == 0) return HDD_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  B.s = static_cast<hipStream_t>(stream);
  const int64_t ldw = even(rows);
  const int64_t n_blk = rows / bs;
  const int64_t ugrid = update_grid(n_blk);
  const int64_t dgrid = std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, 4096));
  B.n_parts = ugrid;
  double* w = d_work;
  dev::SolveBatch& v = B.g;
  v.state = reinterpret_cast<dev::SolveState*>(w);
  v.stop = reinterpret_cast<int32_t*>(w + HDD_MAX_VEC * (sizeof(dev::SolveState) / 8));
  w += BATCH_HEAD;
  v.part_pq = w; w += int64_t(n_rhs) * dev::SOLVE_PARTS;
  v.part_rz = w; w += int64_t(n_rhs) * dev::SOLVE_PARTS;
  v.part_rr = w; w += int64_t(n_rhs) * dev::SOLVE_PARTS;
  double* part_bb = w; w += int64_t(n_rhs) * dev::SOLVE_PARTS;
  v.p = w; w += n_rhs * ldw;
  v.q = w; w += n_rhs * ldw;
  v.r = w; w += n_rhs * ldw;
  v.z = B.pre ? w : v.r; w += n_rhs * ldw;
  v.dinv = w;
  v.x = d_x;
  v.ldx = ldx;
  v.ldw = ldw;
  v.n = rows;
  v.n_pq = int32_t(dot_grid(ctx, B.P));
  v.nv = std::min(NVB, n_rhs);
  v.history = d_history;
  v.ldh = ldh;
  // the 16-byte paths need every column of x aligned
  B.a16 = reinterpret_cast<uintptr_t>(d_work) % 16 == 0 && reinterpret_cast<uintptr_t>(d_x) % 16 == 0 && (n_rhs == 1 || ldx % 2 == 0);
  const bool x0 = (opt->flags & HDD_SOLVE_X0) != 0;

  // names of the iteration's kernels: the vector count is the instantiation's (APPLY_NV), not n_rhs
  {
    const std::string nv = std::to_string(NVB);
    std::string& nm = last_solve_kernels_slot();
    if (B.P.tile) nm = B.P.nb == 3 ? "apply_tile_kernel<3, 3, " + nv + ", dot>" : "apply_tile_kernel<4, 4, " + nv + ", dot>";
    else nm = B.P.short_rows ? "apply_csr_kernel<8, " + nv + ", dot>" : "apply_csr_kernel<64, " + nv + ", dot>";
    nm += " + cg_update<" + std::to_string(bs) + (B.pre ? ", " : ", none, ") + nv + "> + cg_direction<" + nv + ">";
  }

  // ---- setup: the single solve's stages, a column at a time on its grids (same sums) ----
  Solve S;
  S.P = B.P;
  S.bs = bs;
  S.pre = B.pre;
  S.a16 = B.a16;
  S.dinv_tile = dinv_tile;
  S.s = B.s;
  S.v = dev::SolveVectors{};
  S.v.dinv = v.dinv;
  S.v.n = rows;
  S.v.part_pq = v.part_pq;   // the counts of indefinite blocks, read before the first apply overwrites them
  int n_bad = 0;
  if (B.pre) {
    n_bad = int(ugrid);
    e = launch_stage(S, DINV, nullptr, false, 0, ugrid);
    if (e != hipSuccess) return hip_fail(e, who);
  }
  if (x0)
    if (int rc = hdd::abi::run_apply(who, ctx, B.P, d_x, ldx, v.q, ldw, n_rhs, stream)) return rc;
  for (int c = 0; c < n_rhs; ++c) {
    S.v.x = d_x + c * ldx;
    S.v.p = v.p + c * ldw;
    S.v.q = v.q + c * ldw;
    S.v.r = v.r + c * ldw;
    S.v.z = v.z + c * ldw;
    S.v.part_bb = part_bb + c * ugrid;
    S.v.part_rz = v.part_rz + c * ugrid;
    S.v.part_rr = v.part_rr + c * ugrid;
    e = launch_stage(S, INIT, d_b + c * ldb, x0, 0, ugrid);
    if (e != hipSuccess) return hip_fail(e, who);
  }
  hipLaunchKernelGGL(dev::cg_init_state_batched_kernel, dim3(1), dim3(64), 0, B.s, v.state, v.stop, int(n_rhs), v.part_pq, n_bad,
                     part_bb, v.part_rz, v.part_rr, int(ugrid), opt->rtol, opt->atol, d_history, ldh);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, who);

  // ---- iterations: min(check_every, remaining) enqueued per group between two looks at all the states ----
  const int every = opt->check_every > 0 ? opt->check_every : 32;
  const dev::SolveState* h = reinterpret_cast<const dev::SolveState*>(ctx->solve_state_h);
  int k = 0;
  for (;;) {
    const int batch = std::min(every, opt->max_iter - k);
    for (int i = 0; i < batch; ++i, ++k)
      for (int g0 = 0; g0 < n_rhs; g0 += NVB) {
        const dev::SolveBatch gv = group_of(B, g0);
        e = launch_apply_dot_batched(ctx, B, gv, k);
        if (e == hipSuccess) e = launch_update_batched_any(B, gv, k);
        if (e != hipSuccess) return hip_fail(e, who);
        if (B.pre) hipLaunchKernelGGL((dev::cg_direction_batched_kernel<true, NVB>), dim3(unsigned(dgrid)), dim3(256), 0, B.s, gv, k, int(ugrid));
        else hipLaunchKernelGGL((dev::cg_direction_batched_kernel<false, NVB>), dim3(unsigned(dgrid)), dim3(256), 0, B.s, gv, k, int(ugrid));
        e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, who);
      }
    e = hipMemcpyAsync(ctx->solve_state_h, v.state, hdd_ctx::SOLVE_STATE_BYTES, hipMemcpyDeviceToHost, B.s);
    if (e == hipSuccess) e = hipStreamSynchronize(B.s);
    if (e != hipSuccess) return hip_fail(e, who);
    bool all = true;
    for (int c = 0; c < n_rhs; ++c) all = all && h[c].done_at <= k;
    if (all || k >= opt->max_iter) break;
  }
  bool cleared = false;
  for (int c = 0; c < n_rhs; ++c) {
    info[c].status = h[c].done_at <= k ? h[c].status : HDD_SOLVE_MAX_ITER;
    info[c].iterations = h[c].iteration;
    info[c].residual = std::sqrt(h[c].rr);
    info[c].rhs_norm = std::sqrt(h[c].bb);
    if (h[c].flags & dev::SOLVE_FLAG_ZERO_RHS) {   // b_c = 0: x_c = 0 whatever the initial guess was
      e = hipMemsetAsync(d_x + c * ldx, 0, size_t(rows) * sizeof(double), B.s);
      if (e != hipSuccess) return hip_fail(e, who);
      info[c].residual = 0.0;
      cleared = true;
    }
  }
  if (cleared) {
    e = hipStreamSynchronize(B.s);
    if (e != hipSuccess) return hip_fail(e, who);
  }
  return HDD_OK;
}
