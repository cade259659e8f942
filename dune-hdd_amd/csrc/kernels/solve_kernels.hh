// dune-hdd_amd/csrc/kernels/solve_kernels.hh -- preconditioned conjugate gradients on sum_q theta_q A_q
// (hdd_operator_solve, abi_solve.hip): what ContainerBasedDefault::uncached_solve's apply_inverse does (base.hh:327-367).
//
// One iteration k is three launches, ordered by the stream alone (no atomics, no grid barriers, no flags between
// workgroups of a launch):
//   apply_*_kernel<..., DOT>  q = A p, partial_pq[workgroup] (apply_kernels.hh)
//   cg_update_kernel<BS>      every wave sums partial_pq in the same order (same bits everywhere), alpha = rho / p.q;
//                             one lane owns one block of BS rows: x += alpha p, r -= alpha q, z = D^-1 r; partials of
//                             r.z and r.r per workgroup
//   cg_direction_kernel       sums the partials, beta = rho' / rho, p = z + beta p; one lane of workgroup 0 writes
//                             the state and history[k + 1]
// The state (SolveState) lives in the caller's workspace.  rho is double-buffered by the parity of k and the stop word
// done_at is the iteration count at which the solve ended (SOLVE_RUNNING until then; why the workgroups of a launch
// may read it while one lane writes it: solve_direction_column).  A launch of iteration k returns at once when
// done_at <= k, so the host may enqueue any number of iterations between two looks.
// Every sum is two-stage in a fixed order: bit-identical from call to call, and independent of check_every.
// The build has -ffinite-math-only: non-finite scalars are recognised by their bits, behind an optimisation barrier
// (solve_finite).
// The steps of one column -- solve_init_column, solve_update_block, solve_direction_column -- are shared with the
// kernels for several right-hand sides per call (hdd_operator_solve_batched), the section at the end of this file.
#pragma once
#include <cstdint>

#include "apply_kernels.hh"

namespace hdd {
namespace dev {

constexpr int SOLVE_PARTS = 4096;    // most partial sums of one kind (workgroups of the launch that wrote them)
constexpr int SOLVE_FLAG_ZERO_RHS = 1;
constexpr int32_t SOLVE_RUNNING = 0x7fffffff;   // done_at / the group's stop word while iterating

struct SolveState {
  double rho[2];       // r . z, indexed by the parity of the iteration that reads it
  double rr, bb;       // ||r||^2 (recurrence), ||b||^2
  double thresh2;      // max(rtol ||b||, atol)^2
  int32_t iteration, status, done_at, flags;
  double pad;
};
static_assert(sizeof(SolveState) == 64, "eight doubles of the workspace");

struct SolveVectors {
  SolveState* state;
  double *x, *p, *q, *r, *z;            // z == r without a preconditioner
  const double* dinv;                   // [n_blocks][BS (BS + 1) / 2], the lower triangles of the inverse blocks
  double *part_pq, *part_rz, *part_rr, *part_bb;
  int64_t n;                            // rows
  int32_t n_pq;                         // partial sums the DOT apply wrote
  double* history;                      // nullable
};

__device__ __forceinline__ bool solve_finite(double v)
{
  uint64_t u = uint64_t(__double_as_longlong(v));
  asm volatile("" : "+v"(u));   // opaque: under -ffinite-math-only the test on the bits would be folded to true
  return ((u >> 52) & 0x7ff) != 0x7ff;
}

// b . b == 0 by its bits (either sign of zero): under -ffinite-math-only `bb == 0.0` may hold for a NaN, and a
// right-hand side with a NaN is a breakdown, not the zero right-hand side
__device__ __forceinline__ bool solve_is_zero(double v)
{
  uint64_t u = uint64_t(__double_as_longlong(v));
  asm volatile("" : "+v"(u));
  return (u << 1) == 0;
}

// sum of part[0, n) by one wave, lane l the entries l, l + 64, ... in order, then a butterfly: every lane of every
// wave that calls it gets the same bits
__device__ __forceinline__ double solve_wave_sum(const double* part, int n)
{
  double s = 0.0;
  for (int i = threadIdx.x & 63; i < n; i += 64) s += part[i];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

// the workgroup's sum of one value per thread (256 threads): butterfly, then the four waves in order; thread 0 has it
__device__ __forceinline__ double solve_block_sum(double s, double* red)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

template <int BS>
constexpr int solve_packed() { return BS * (BS + 1) / 2; }

// BS consecutive doubles; A16: BS is even and the address 16-byte aligned
template <int BS, bool A16>
__device__ __forceinline__ void solve_load(const double* p, double (&v)[BS])
{
  if constexpr (A16) {
#pragma unroll
    for (int i = 0; i < BS; i += 2) {
      const dvec2 t = *reinterpret_cast<const dvec2*>(p + i);
      v[i] = t.x;
      v[i + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < BS; ++i) v[i] = p[i];
  }
}
template <int BS, bool A16>
__device__ __forceinline__ void solve_store(double* p, const double (&v)[BS])
{
  if constexpr (A16) {
#pragma unroll
    for (int i = 0; i < BS; i += 2) {
      dvec2 t;
      t.x = v[i];
      t.y = v[i + 1];
      *reinterpret_cast<dvec2*>(p + i) = t;
    }
  } else {
#pragma unroll
    for (int i = 0; i < BS; ++i) p[i] = v[i];
  }
}

// the packed lower triangle of one (symmetric) inverse block
template <int BS>
__device__ __forceinline__ void solve_load_packed(const double* dinv, double (&m)[solve_packed<BS>()])
{
#pragma unroll
  for (int k = 0; k < solve_packed<BS>(); ++k) m[k] = dinv[k];
}

// z = D^-1 r from the packed inverse block in registers
template <int BS>
__device__ __forceinline__ void solve_precond_regs(const double (&m)[solve_packed<BS>()], const double (&r)[BS], double (&z)[BS])
{
#pragma unroll
  for (int i = 0; i < BS; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < BS; ++j) s = __builtin_fma(i >= j ? m[i * (i + 1) / 2 + j] : m[j * (j + 1) / 2 + i], r[j], s);
    z[i] = s;
  }
}
template <int BS>
__device__ __forceinline__ void solve_precond(const double* dinv, const double (&r)[BS], double (&z)[BS])
{
  double m[solve_packed<BS>()];
  solve_load_packed<BS>(dinv, m);
  solve_precond_regs<BS>(m, r, z);
}

// In-place inverse of a symmetric positive definite block (Gauss-Jordan without pivoting: the pivots are the Schur
// complements, positive for a definite block), packed lower triangle to out.  false: a pivot was not positive (or
// not finite); out is then zero.
template <int BS>
__device__ __forceinline__ bool solve_invert(double (&A)[BS][BS], double* out)
{
  bool ok = true;
#pragma unroll
  for (int k = 0; k < BS; ++k) {
    const double piv = A[k][k];
    ok = ok && solve_finite(piv) && piv > 0.0;
    const double d = 1.0 / (ok ? piv : 1.0);
    A[k][k] = 1.0;
#pragma unroll
    for (int j = 0; j < BS; ++j) A[k][j] *= d;
#pragma unroll
    for (int i = 0; i < BS; ++i) {
      if (i == k) continue;
      const double f = A[i][k];
      A[i][k] = 0.0;
#pragma unroll
      for (int j = 0; j < BS; ++j) A[i][j] = __builtin_fma(-f, A[k][j], A[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const double v = 0.5 * (A[i][j] + A[j][i]);
      out[i * (i + 1) / 2 + j] = ok && solve_finite(v) ? v : 0.0;
    }
  return ok;
}

// Diagonal blocks on the tile path (BS == NB): lane = element.  Its own block is block number (interior neighbours
// with a smaller id) of its row block, whose row stride is NB (interior neighbours + 1) -- from elem_ptr and the
// neighbours alone; col is not read.  part_bad[workgroup] = blocks that were not positive definite.
// g: the workgroup's view (apply_kernels.hh) -- its index, the grid and the element range; dinv, part_bad: the range's;
// red: four doubles of the kernel's LDS
template <int NB, int NF, class View, class Grid>
__device__ __forceinline__ void solve_dinv_tile_body(const ApplyArgs& a, const View& g, const Grid& grid, double* dinv, double* part_bad, double* red)
{
  double bad = 0.0;
  const int64_t n_el = g.e_end() - g.e_begin();
  for (int64_t i = int64_t(grid.w()) * 256 + threadIdx.x; i < n_el; i += int64_t(grid.nw()) * 256) {
    const int64_t e = g.e_begin() + i;
    int nint = 0, pos = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int nb = a.nbrs[f * a.n_local + e];
      nint += nb >= 0;
      pos += nb >= 0 && nb < e;
    }
    const int rl = NB * (nint + 1);
    int64_t base = a.elem_ptr[e - a.own_begin] + int64_t(pos) * NB;
    double D[NB][NB];
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        int64_t k = base + r * rl + c;
        k = k < 0 ? 0 : (k >= a.nnz ? a.nnz - 1 : k);   // an index the mesh got wrong stays inside the arrays
        D[r][c] = apply_entry(a, k);
      }
    if (!solve_invert<NB>(D, dinv + i * solve_packed<NB>())) bad += 1.0;
  }
  const double s = solve_block_sum(bad, red);
  if (threadIdx.x == 0) part_bad[grid.w()] = s;
}

template <int NB, int NF>
__global__ void __launch_bounds__(256) solve_dinv_tile_kernel(const ApplyArgs a, double* dinv, double* part_bad)
{
  __shared__ double red[4];
  solve_dinv_tile_body<NB, NF>(a, apply_view(a), LaunchGrid{}, dinv, part_bad, red);
}

// Diagonal blocks on the CSR path: thread = block of BS rows, found in col
template <int BS, class View, class Grid>
__device__ __forceinline__ void solve_dinv_csr_body(const ApplyArgs& a, const View& g, const Grid& grid, double* dinv, double* part_bad, double* red)
{
  double bad = 0.0;
  const int64_t n_blk = (g.row_end() - g.row_begin()) / BS;
  for (int64_t i = int64_t(grid.w()) * 256 + threadIdx.x; i < n_blk; i += int64_t(grid.nw()) * 256) {
    const int64_t r0 = g.row_begin() + i * BS;
    double D[BS][BS];
#pragma unroll
    for (int r = 0; r < BS; ++r) {
#pragma unroll
      for (int c = 0; c < BS; ++c) D[r][c] = 0.0;
      int64_t k0 = a.row_ptr[r0 + r], k1 = a.row_ptr[r0 + r + 1];
      k0 = k0 < 0 ? 0 : k0;
      k1 = k1 > a.nnz ? a.nnz : k1;
      for (int64_t k = k0; k < k1; ++k) {
        const int64_t c = int64_t(a.col[k]) - r0;
        if (c < 0 || c >= BS) continue;
        const double m = apply_entry(a, k);
#pragma unroll
        for (int cc = 0; cc < BS; ++cc)
          if (cc == c) D[r][cc] += m;
      }
    }
    if (!solve_invert<BS>(D, dinv + i * solve_packed<BS>())) bad += 1.0;
  }
  const double s = solve_block_sum(bad, red);
  if (threadIdx.x == 0) part_bad[grid.w()] = s;
}

template <int BS>
__global__ void __launch_bounds__(256) solve_dinv_csr_kernel(const ApplyArgs a, double* dinv, double* part_bad)
{
  __shared__ double red[4];
  solve_dinv_csr_body<BS>(a, apply_view(a), LaunchGrid{}, dinv, part_bad, red);
}

// Setup: r = b (X0: b - q, q = A x0 from a plain apply), x = 0 (X0: kept), z = D^-1 r, p = z; partials of b.b, r.z, r.r
// (grid: the launch's own, or the virtual ones of a segment; red: the kernel's LDS)
template <int BS, bool PRE, bool A16, class Grid>
__device__ __forceinline__ void cg_init_body(const SolveVectors& v, const double* b, bool x0, const Grid& grid, double (&red)[3][4])
{
  double bb = 0.0, rz = 0.0, rr = 0.0;
  const int64_t n_blk = v.n / BS;
  for (int64_t i = int64_t(grid.w()) * 256 + threadIdx.x; i < n_blk; i += int64_t(grid.nw()) * 256) {
    const int64_t o = i * BS;
    double bv[BS], rv[BS], zv[BS];
#pragma unroll
    for (int k = 0; k < BS; ++k) bv[k] = b[o + k];   // the caller's b: no alignment assumed
    if (x0) {
      solve_load<BS, A16>(v.q + o, rv);
#pragma unroll
      for (int k = 0; k < BS; ++k) rv[k] = bv[k] - rv[k];
    } else {
#pragma unroll
      for (int k = 0; k < BS; ++k) rv[k] = bv[k];
      double zero[BS] = {};
      solve_store<BS, A16>(v.x + o, zero);
    }
    if constexpr (PRE) solve_precond<BS>(v.dinv + i * solve_packed<BS>(), rv, zv);
#pragma unroll
    for (int k = 0; k < BS; ++k) {
      if constexpr (!PRE) zv[k] = rv[k];
      bb = __builtin_fma(bv[k], bv[k], bb);
      rz = __builtin_fma(rv[k], zv[k], rz);
      rr = __builtin_fma(rv[k], rv[k], rr);
    }
    solve_store<BS, A16>(v.r + o, rv);
    if constexpr (PRE) solve_store<BS, A16>(v.z + o, zv);
    solve_store<BS, A16>(v.p + o, zv);
  }
  const double s0 = solve_block_sum(bb, red[0]), s1 = solve_block_sum(rz, red[1]), s2 = solve_block_sum(rr, red[2]);
  if (threadIdx.x == 0) {
    v.part_bb[grid.w()] = s0;
    v.part_rz[grid.w()] = s1;
    v.part_rr[grid.w()] = s2;
  }
}

template <int BS, bool PRE, bool A16>
__global__ void __launch_bounds__(256) cg_init_kernel(const SolveVectors v, const double* b, bool x0)
{
  __shared__ double red[3][4];
  cg_init_body<BS, PRE, A16>(v, b, x0, LaunchGrid{}, red);
}

// One column's state before the first iteration and history[0] (nullable), by one lane; bad: the number of
// indefinite diagonal blocks.  Returns done_at: 0 when the column does not iterate.
__device__ __forceinline__ int solve_init_column(SolveState& s, double* history, double bad, double bb, double rz, double rr,
                                                 double rtol, double atol)
{
  const double t = rtol * __builtin_sqrt(bb);
  const double thresh = t > atol ? t : atol;
  s.rho[0] = rz;
  s.rho[1] = 0.0;
  s.rr = rr;
  s.bb = bb;
  s.thresh2 = thresh * thresh;
  s.iteration = 0;
  const bool zero_rhs = solve_is_zero(bb);
  s.flags = zero_rhs ? SOLVE_FLAG_ZERO_RHS : 0;
  s.pad = 0.0;
  int status = HDD_SOLVE_CONVERGED, done_at = SOLVE_RUNNING;
  if (zero_rhs) done_at = 0;                                      // x = 0 (the host clears it)
  else if (bad > 0.0) status = HDD_SOLVE_BREAKDOWN, done_at = 0;  // a diagonal block is not positive definite
  else if (solve_finite(rr) && rr <= s.thresh2) done_at = 0;
  else if (!solve_finite(rr) || !solve_finite(rz) || !(rz > 0.0)) status = HDD_SOLVE_BREAKDOWN, done_at = 0;
  s.status = status;
  s.done_at = done_at;
  if (history) history[0] = __builtin_sqrt(rr);
  return done_at;
}

// Setup, one wave: the state before the first iteration.  n_bad: partial counts of indefinite blocks in part_pq
__global__ void __launch_bounds__(64) cg_init_state_kernel(const SolveVectors v, int n_parts, int n_bad, double rtol, double atol)
{
  const double bad = solve_wave_sum(v.part_pq, n_bad);
  const double bb = solve_wave_sum(v.part_bb, n_parts);
  const double rz = solve_wave_sum(v.part_rz, n_parts);
  const double rr = solve_wave_sum(v.part_rr, n_parts);
  if (threadIdx.x == 0) solve_init_column(*v.state, v.history, bad, bb, rz, rr, rtol, atol);
}

// One block of BS rows of one column (p, q, x, r, z point at it): x += alpha p, r -= alpha q, z = D^-1 r from the
// packed inverse block m (not read without PRE), r . z and r . r added to rz (PRE) and rr
template <int BS, bool PRE, bool A16>
__device__ __forceinline__ void solve_update_block(const double* p, const double* q, double* x, double* r, double* z,
                                                   const double (&m)[solve_packed<BS>()], double alpha, double& rz, double& rr)
{
  double pv[BS], qv[BS], xv[BS], rv[BS], zv[BS];
  solve_load<BS, A16>(p, pv);
  solve_load<BS, A16>(q, qv);
  solve_load<BS, A16>(x, xv);
  solve_load<BS, A16>(r, rv);
#pragma unroll
  for (int j = 0; j < BS; ++j) {
    xv[j] = __builtin_fma(alpha, pv[j], xv[j]);
    rv[j] = __builtin_fma(-alpha, qv[j], rv[j]);
  }
  if constexpr (PRE) solve_precond_regs<BS>(m, rv, zv);
#pragma unroll
  for (int j = 0; j < BS; ++j) {
    if constexpr (PRE) rz = __builtin_fma(rv[j], zv[j], rz);
    rr = __builtin_fma(rv[j], rv[j], rr);
  }
  solve_store<BS, A16>(x, xv);
  solve_store<BS, A16>(r, rv);
  if constexpr (PRE) solve_store<BS, A16>(z, zv);
}

template <int BS, bool PRE, bool A16, class Grid>
__device__ __forceinline__ void cg_update_body(const SolveVectors& v, int k, const Grid& grid, double (&red)[2][4])
{
  if (v.state->done_at <= k) return;   // (uniform)
  const double pq = solve_wave_sum(v.part_pq, v.n_pq);
  if (!solve_finite(pq) || !(pq > 0.0)) return;   // breakdown: cg_direction_kernel sees the same sum and records it
  const double alpha = v.state->rho[k & 1] / pq;
  double rz = 0.0, rr = 0.0;
  const int64_t n_blk = v.n / BS;
  for (int64_t i = int64_t(grid.w()) * 256 + threadIdx.x; i < n_blk; i += int64_t(grid.nw()) * 256) {
    const int64_t o = i * BS;
    [[maybe_unused]] double m[solve_packed<BS>()];
    if constexpr (PRE) solve_load_packed<BS>(v.dinv + i * solve_packed<BS>(), m);
    solve_update_block<BS, PRE, A16>(v.p + o, v.q + o, v.x + o, v.r + o, v.z + o, m, alpha, rz, rr);
  }
  const double s0 = solve_block_sum(rz, red[0]), s1 = solve_block_sum(rr, red[1]);
  if (threadIdx.x == 0) {
    if constexpr (PRE) v.part_rz[grid.w()] = s0;
    v.part_rr[grid.w()] = s1;
  }
}

template <int BS, bool PRE, bool A16>
__global__ void __launch_bounds__(256) cg_update_kernel(const SolveVectors v, int k)
{
  __shared__ double red[2][4];
  cg_update_body<BS, PRE, A16>(v, k, LaunchGrid{}, red);
}

// The end of iteration k for one column that was live (done_at > k) when the launch began: sums the partials
// (n_parts: workgroups of the cg_update launch), decides, p = z + beta p; the writer (one lane of the launch) stores
// the state and history[k + 1] (history: the column's, nullable); workgroup grid.w() of grid.nw() (the launch's own, or the virtual
// ones of a segment: the update of p has no sum in it, so its grid is free).  Returns the column's done_at after this launch:
// k (p . q breakdown: x, r are those of iteration k), k + 1 (converged / r . z breakdown) or SOLVE_RUNNING.
// The other workgroups of launch k read done_at while the writer stores it, and decide the same for the old value
// SOLVE_RUNNING and for the new one: `<= k` is false for k + 1 as well; and a reader of the old value before a new k
// forms the same p . q from the same partial sums and leaves the column alone, too.  The launches before (apply,
// update of iteration k) and after (iteration k + 1) are ordered by the stream.
template <bool PRE, class Grid>
__device__ __forceinline__ int solve_direction_column(SolveState& s, const double* part_pq, int n_pq, const double* part_rz,
                                                      const double* part_rr, int n_parts, double* p, const double* z, int64_t n,
                                                      double* history, int k, bool writer, const Grid& grid)
{
  const double pq = solve_wave_sum(part_pq, n_pq);
  if (!solve_finite(pq) || !(pq > 0.0)) {
    if (writer) s.status = HDD_SOLVE_BREAKDOWN, s.done_at = k;
    return k;
  }
  const double rr = solve_wave_sum(part_rr, n_parts);
  const double rz = PRE ? solve_wave_sum(part_rz, n_parts) : rr;
  const bool converged = solve_finite(rr) && rr <= s.thresh2;
  const bool broken = !converged && (!solve_finite(rr) || !solve_finite(rz) || !(rz > 0.0));
  if (writer) {
    s.rho[(k + 1) & 1] = rz;
    s.rr = rr;
    s.iteration = k + 1;
    if (history) history[k + 1] = __builtin_sqrt(rr);
    if (broken) s.status = HDD_SOLVE_BREAKDOWN;
    if (converged || broken) s.done_at = k + 1;
  }
  if (converged || broken) return k + 1;
  const double beta = rz / s.rho[k & 1];
  for (int64_t i = int64_t(grid.w()) * 256 + threadIdx.x; i < n; i += int64_t(grid.nw()) * 256)
    p[i] = __builtin_fma(beta, p[i], z[i]);
  return SOLVE_RUNNING;
}

template <bool PRE>
__global__ void __launch_bounds__(256) cg_direction_kernel(const SolveVectors v, int k, int n_parts)
{
  if (v.state->done_at <= k) return;   // (uniform)
  solve_direction_column<PRE>(*v.state, v.part_pq, v.n_pq, v.part_rz, v.part_rr, n_parts, v.p, v.z, v.n, v.history, k,
                              blockIdx.x == 0 && threadIdx.x == 0, LaunchGrid{});
}

// ---- several right-hand sides per call (hdd_operator_solve_batched) ----------------------------------------------
// The columns run in groups of up to APPLY_NV, the apply's pass width: one iteration of a group is the same three
// launches with NV = APPLY_NV, the value stream and the inverse blocks read once for the group.  Every column keeps
// the arithmetic of the single solve -- its own FMA chains, its own partial sums [column][workgroup] on the single
// solve's grids, its own SolveState -- so column j ends with the bits hdd_operator_solve gives for (b_j, x0_j).
//
// Two kinds of stop words.  state[c].done_at is column c's (solve_direction_column): a column that is done is frozen,
// no later launch touches its x, r, z or p (the apply still writes its q, which nobody reads).  *stop is the group's
// (cg_direction_batched_kernel): a launch of iteration k returns at once when *stop <= k.

struct SolveBatch {
  SolveState* state;                    // [nv], the group's columns
  int32_t* stop;                        // the group's stop word
  double* x;                            // x[c * ldx + row], the caller's
  int64_t ldx;
  double *p, *q, *r, *z;                // [c * ldw + row]; z == r without a preconditioner
  int64_t ldw;
  const double* dinv;                   // shared by all columns; OWN_BLOCKS: column c's blocks at dinv + c * ld_dinv
  double *part_pq, *part_rz, *part_rr;  // [c * n_pq + workgroup], [c * n_parts + workgroup]
  int64_t n;                            // rows
  int32_t n_pq, nv;
  double* history;                      // nullable, history[c * ldh + k]
  int64_t ldh;
  int64_t ld_dinv;                      // OWN_BLOCKS (a theta per column, hdd_operator_solve_multi) only
};

// Setup, one wave: the states of all n_rhs columns before the first iteration (cg_init_state_kernel's sums and
// solve_init_column per column; the partial sums are [column][n_parts]), then the stop words of the groups of APPLY_NV.
// bad_stride 0: one count of indefinite blocks for all columns (one theta); else column c's own inverse blocks left
// its partial counts at part_bad + c * bad_stride, and a block that is indefinite at theta_c breaks only column c down
__global__ void __launch_bounds__(64) cg_init_state_batched_kernel(SolveState* state, int32_t* stop, int n_rhs, const double* part_bad,
                                                                   int n_bad, const double* part_bb, const double* part_rz,
                                                                   const double* part_rr, int n_parts, double rtol, double atol,
                                                                   double* history, int64_t ldh, int64_t bad_stride)
{
  const double bad_all = solve_wave_sum(part_bad, n_bad);
  unsigned live = 0;   // (lane 0) bit c: column c iterates
  for (int c = 0; c < n_rhs; ++c) {
    const double bb = solve_wave_sum(part_bb + int64_t(c) * n_parts, n_parts);
    const double rz = solve_wave_sum(part_rz + int64_t(c) * n_parts, n_parts);
    const double rr = solve_wave_sum(part_rr + int64_t(c) * n_parts, n_parts);
    const double bad = bad_stride ? solve_wave_sum(part_bad + c * bad_stride, n_bad) : bad_all;
    if (threadIdx.x != 0) continue;
    if (solve_init_column(state[c], history ? history + int64_t(c) * ldh : nullptr, bad, bb, rz, rr, rtol, atol) != 0) live |= 1u << c;
  }
  if (threadIdx.x != 0) return;
  for (int g = 0; g * APPLY_NV < n_rhs; ++g) stop[g] = ((live >> (g * APPLY_NV)) & ((1u << APPLY_NV) - 1)) ? SOLVE_RUNNING : 0;
}

// cg_update_kernel for a group: the grid and the lane -> block mapping are the single solve's; the lane loads its
// packed inverse block once and uses it for every live column -- with OWN_BLOCKS (a theta per column) column c's own
// block inside the column loop instead.  The per-column accumulators are indexed at compile time (unrolled over NV,
// guarded), so they stay in registers.
template <int BS, bool PRE, bool A16, int NV, bool OWN_BLOCKS = false>
__global__ void __launch_bounds__(256) cg_update_batched_kernel(const SolveBatch v, int k)
{
  __shared__ double red[NV][2][4];
  if (*v.stop <= k) return;   // (uniform)
  bool live[NV];
  double alpha[NV], rz[NV], rr[NV];
  bool any = false;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    live[c] = false;
    alpha[c] = rz[c] = rr[c] = 0.0;
    if (c < v.nv && v.state[c].done_at > k) {   // (uniform)
      const double pq = solve_wave_sum(v.part_pq + int64_t(c) * v.n_pq, v.n_pq);
      // a breakdown: cg_direction_batched_kernel sees the same sum and records it
      if (solve_finite(pq) && pq > 0.0) {
        live[c] = true;
        alpha[c] = v.state[c].rho[k & 1] / pq;
      }
    }
    any = any || live[c];
  }
  if (!any) return;
  const int64_t n_blk = v.n / BS;
  const int64_t n_parts = gridDim.x;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n_blk; i += int64_t(gridDim.x) * 256) {
    const int64_t o = i * BS;
    [[maybe_unused]] double m[solve_packed<BS>()];
    if constexpr (PRE && !OWN_BLOCKS) solve_load_packed<BS>(v.dinv + i * solve_packed<BS>(), m);
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      if (!live[c]) continue;
      if constexpr (PRE && OWN_BLOCKS) solve_load_packed<BS>(v.dinv + c * v.ld_dinv + i * solve_packed<BS>(), m);
      const int64_t ow = c * v.ldw + o, ox = c * v.ldx + o;
      solve_update_block<BS, PRE, A16>(v.p + ow, v.q + ow, v.x + ox, v.r + ow, v.z + ow, m, alpha[c], rz[c], rr[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    if (!live[c]) continue;   // (uniform)
    const double s0 = solve_block_sum(rz[c], red[c][0]), s1 = solve_block_sum(rr[c], red[c][1]);
    if (threadIdx.x == 0) {
      if constexpr (PRE) v.part_rz[c * n_parts + blockIdx.x] = s0;
      v.part_rr[c * n_parts + blockIdx.x] = s1;
    }
  }
}

// cg_direction_kernel for a group: solve_direction_column for every live column, then the group's stop word -- the
// iteration at which its last live column ended (SOLVE_RUNNING while one is live), written by the same lane that
// writes the columns' done_at while the other workgroups of launch k read it.  They decide the same for the old
// value SOLVE_RUNNING and for the new one, the largest done_at of the group: that is k + 1 (`<= k` false both ways)
// unless every column that was still live broke down on its p . q in this launch (new value <= k), and a reader of
// the old value then finds every column done or broken and touches nothing either.
template <bool PRE, int NV>
__global__ void __launch_bounds__(256) cg_direction_batched_kernel(const SolveBatch v, int k, int n_parts)
{
  if (*v.stop <= k) return;   // (uniform)
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  int ended = 0;       // (writer) the largest done_at of the group's columns
  bool any = false;    // a column goes on
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    if (c >= v.nv) continue;
    int d = v.state[c].done_at;   // <= k: frozen
    if (d > k)
      d = solve_direction_column<PRE>(v.state[c], v.part_pq + int64_t(c) * v.n_pq, v.n_pq, v.part_rz + int64_t(c) * n_parts,
                                      v.part_rr + int64_t(c) * n_parts, n_parts, v.p + c * v.ldw, v.z + c * v.ldw, v.n,
                                      v.history ? v.history + c * v.ldh : nullptr, k, writer, LaunchGrid{});
    if (d == SOLVE_RUNNING) any = true;
    else ended = ended > d ? ended : d;
  }
  if (writer && !any) *v.stop = ended;
}

// ---- every segment of a partition per call (hdd_operator_solve_blocks) --------------------------------------------
// Solves A_ss x_s = b_s for the segments s of a row interval in the same three launches per iteration, whatever the
// number of segments.  Every workgroup of a launch finds its segment and its virtual index there (BlockSegment,
// apply_kernels.hh) and runs the single solve's body with them, on the segment's slice of the vectors, its own
// partial sums (at the offset first[kind]) and its own SolveState: segment s ends with the bits hdd_operator_solve
// gives on the range (row_begin, row_begin + rows) squared.
//
// Stop words.  state[s].done_at is segment s's, written by the first virtual workgroup of the segment in the
// direction launch and read by the segment's other workgroups of that launch: solve_direction_column's argument
// holds per segment.  *stop is the call's: the largest done_at once no segment iterates (SOLVE_RUNNING before).  It
// is computed from the stored done_at alone (solve_blocks_scan), by a launch of its own before every look of the host
// and by one more workgroup at the end of every update launch, so that the launches behind the end of the last
// segment return without looking their segment up.  That workgroup of update launch k reads only what earlier
// launches stored (direction launch j stores j or j + 1 <= k) and writes while the other workgroups of launch k read:
// it leaves SOLVE_RUNNING unless every segment is done, and then the new value is <= k -- a reader of the old value
// goes on to its segment's done_at <= k and returns, a reader of the new value returns at once: the same decision.

struct SolveBlocks {
  BlocksArgs B;                         // B.kind: BLOCKS_PARTS (the inverse-block launch's view); the others name theirs
  SolveState* state;                    // [n_seg]
  int32_t* stop;                        // the call's stop word
  double *x, *p, *q, *r, *z;            // the interval's; z == r without a preconditioner
  const double* dinv;                   // the interval's packed inverse blocks
  double *part_pq, *part_rz, *part_rr, *part_bb, *part_bad;   // segment s at first[BLOCKS_DOT] / first[BLOCKS_PARTS]
  double* history;                      // nullable, history[s * ldh + k]
  int64_t ldh;
};

// segment s as the single solve's kernels see their one column
template <int BS>
__device__ __forceinline__ SolveVectors blocks_column(const SolveBlocks& v, int s)
{
  const BlockSegment& g = v.B.seg[s];
  const int64_t o = g.row_begin - v.B.row0;
  const int dq = g.first[BLOCKS_DOT], dp = g.first[BLOCKS_PARTS];
  return SolveVectors{v.state + s, v.x + o, v.p + o, v.q + o, v.r + o, v.z + o, v.dinv + o / BS * solve_packed<BS>(),
                      v.part_pq + dq, v.part_rz + dp, v.part_rr + dp, v.part_bb + dp, g.rows, g.grid[BLOCKS_DOT],
                      v.history ? v.history + s * v.ldh : nullptr};
}

// the inverse blocks of the whole interval in one launch, on the segments' update grids; the counts of blocks that
// are not positive definite stay with their segment (part_bad at first[BLOCKS_PARTS]).  B.kind is BLOCKS_PARTS.
template <int NB, int NF>
__global__ void __launch_bounds__(256) solve_dinv_tile_blocks_kernel(const ApplyArgs a, const BlocksArgs B, double* dinv, double* part_bad)
{
  const int s = blocks_find(B.seg, B.n_seg, BLOCKS_PARTS, blockIdx.x);
  const BlockSegment& g = B.seg[s];
  __shared__ double red[4];
  solve_dinv_tile_body<NB, NF>(a, blocks_view(a, B, s), blocks_grid(g, BLOCKS_PARTS), dinv + (g.row_begin - B.row0) / NB * solve_packed<NB>(),
                               part_bad + g.first[BLOCKS_PARTS], red);
}

template <int BS>
__global__ void __launch_bounds__(256) solve_dinv_csr_blocks_kernel(const ApplyArgs a, const BlocksArgs B, double* dinv, double* part_bad)
{
  const int s = blocks_find(B.seg, B.n_seg, BLOCKS_PARTS, blockIdx.x);
  const BlockSegment& g = B.seg[s];
  __shared__ double red[4];
  solve_dinv_csr_body<BS>(a, blocks_view(a, B, s), blocks_grid(g, BLOCKS_PARTS), dinv + (g.row_begin - B.row0) / BS * solve_packed<BS>(),
                          part_bad + g.first[BLOCKS_PARTS], red);
}

template <int BS, bool PRE, bool A16>
__global__ void __launch_bounds__(256) cg_init_blocks_kernel(const SolveBlocks v, const double* b, bool x0)
{
  const int s = blocks_find(v.B.seg, v.B.n_seg, BLOCKS_PARTS, blockIdx.x);
  const BlockSegment& g = v.B.seg[s];
  __shared__ double red[3][4];
  cg_init_body<BS, PRE, A16>(blocks_column<BS>(v, s), b + (g.row_begin - v.B.row0), x0, blocks_grid(g, BLOCKS_PARTS), red);
}

// Setup, one wave per segment: cg_init_state_kernel's sums and solve_init_column
__global__ void __launch_bounds__(64) cg_init_state_blocks_kernel(const SolveBlocks v, bool pre, double rtol, double atol)
{
  const int s = blockIdx.x;
  const BlockSegment& g = v.B.seg[s];
  const int n_parts = g.grid[BLOCKS_PARTS], o = g.first[BLOCKS_PARTS];
  const double bad = solve_wave_sum(v.part_bad + o, pre ? n_parts : 0);
  const double bb = solve_wave_sum(v.part_bb + o, n_parts);
  const double rz = solve_wave_sum(v.part_rz + o, n_parts);
  const double rr = solve_wave_sum(v.part_rr + o, n_parts);
  if (threadIdx.x == 0) solve_init_column(v.state[s], v.history ? v.history + s * v.ldh : nullptr, bad, bb, rz, rr, rtol, atol);
}

// *stop = the largest done_at of the segments (SOLVE_RUNNING, the largest int32_t, while one iterates), by one
// workgroup of 256 threads
__device__ __forceinline__ void solve_blocks_scan(const SolveState* state, int n_seg, int32_t* stop)
{
  __shared__ int32_t red[4];
  int32_t m = 0;
  for (int i = threadIdx.x; i < n_seg; i += 256) {
    const int32_t d = state[i].done_at;
    m = m > d ? m : d;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const int32_t o = __shfl_xor(m, d, 64);
    m = m > o ? m : o;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < 4; ++i) m = m > red[i] ? m : red[i];
    *stop = m;   // other workgroups of an update launch may read the old or the new value: the same decision (above)
  }
}

// before the first iteration and before every look of the host
__global__ void __launch_bounds__(256) cg_stop_blocks_kernel(const SolveState* state, int n_seg, int32_t* stop)
{
  solve_blocks_scan(state, n_seg, stop);
}

// the launch has one workgroup more than the segments' update grids together: the last one renews the stop word
template <int BS, bool PRE, bool A16>
__global__ void __launch_bounds__(256) cg_update_blocks_kernel(const SolveBlocks v, int k)
{
  __shared__ double red[2][4];
  if (*v.stop <= k) return;   // (uniform)
  if (blockIdx.x == gridDim.x - 1) {
    solve_blocks_scan(v.state, v.B.n_seg, v.stop);
    return;
  }
  const int s = blocks_find(v.B.seg, v.B.n_seg, BLOCKS_PARTS, blockIdx.x);
  const BlockSegment& g = v.B.seg[s];
  cg_update_body<BS, PRE, A16>(blocks_column<BS>(v, s), k, blocks_grid(g, BLOCKS_PARTS), red);
}

template <bool PRE>
__global__ void __launch_bounds__(256) cg_direction_blocks_kernel(const SolveBlocks v, int k)
{
  if (*v.stop <= k) return;   // (uniform)
  const int s = blocks_find(v.B.seg, v.B.n_seg, BLOCKS_DIRECTION, blockIdx.x);
  const BlockSegment& g = v.B.seg[s];
  const SolveVectors c = blocks_column<1>(v, s);   // (the inverse blocks are not read here)
  if (c.state->done_at <= k) return;   // (uniform)
  const VirtualGrid grid = blocks_grid(g, BLOCKS_DIRECTION);
  solve_direction_column<PRE>(*c.state, c.part_pq, c.n_pq, c.part_rz, c.part_rr, g.grid[BLOCKS_PARTS], c.p, c.z, c.n, c.history, k,
                              grid.w() == 0 && threadIdx.x == 0, grid);
}

}  // namespace dev
}  // namespace hdd
