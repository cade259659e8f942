// dune-hdd_amd/csrc/kernels/abi_solve.hip -- C ABI: hdd_operator_solve, block-Jacobi preconditioned conjugate
// gradients on sum_q theta_q A_q (kernels in solve_kernels.hh and the DOT variants of apply_kernels.hh): the
// apply_inverse of ContainerBasedDefault::uncached_solve (base.hh:327-367) on the device, and
// hdd_operator_solve_batched, the same iteration for up to HDD_MAX_VEC right-hand sides in groups of APPLY_NV.  The
// operator arguments are checked and dispatched by plan_apply (apply_plan.hh), as hdd_operator_apply's.
// hdd_operator_solve_multi is the batched solve with a theta per column: the multi-theta applies and every column's
// own inverse blocks.
// hdd_operator_solve_blocks is the iteration on every segment of a partition of a row interval at once (the end of
// this file), with its own workspace layout, table upload and setup launches.
// One driver serves every entry.  The extern "C" function puts its arguments into a Call; checked (every argument
// check) fills Solve (what the options resolve to, and the workspace's views: columns, groups, or Solve::seg for the
// segments); name_kernels; iterate enqueues the entry's launches of one iteration check_every at a time between
// the entry's looks; finish turns n states (columns or segments), each owning a slice of x, into infos.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>

#include "apply_plan.hh"
#include "solve_kernels.hh"

using hdd::abi::ApplyPlan;
using hdd::abi::fail;
namespace dev = hdd::dev;

namespace {
constexpr int NVB = dev::APPLY_NV;

// what differs between the entries before the iteration: the names in the messages, the head of the workspace
// (doubles before the partial sums), who gives the leading dimensions and whether every column has a theta, and
// with it inverse blocks, of its own; whether the states are those of segments of one column
struct Entry {
  const char *who, *workspace;
  int64_t head;
  bool dense;      // one column: ldb = ldx = rows, ldh = max_iter + 1 whatever the caller passed
  bool own;        // theta is [n_rhs][ldt]
  bool segments;   // one column over the interval (bounds[0], bounds[n_blocks]), a state and an info per segment
};
constexpr Entry SINGLE{"hdd_operator_solve", "hdd_operator_solve_workspace", int64_t(sizeof(dev::SolveState) / 8), true, false, false};
// states of HDD_MAX_VEC columns, then the group words
constexpr Entry BATCHED{"hdd_operator_solve_batched", "hdd_operator_solve_batched_workspace", int64_t(hdd_ctx::SOLVE_STATE_BYTES / 8), false, false, false};
constexpr Entry MULTI{"hdd_operator_solve_multi", "hdd_operator_solve_multi_workspace", int64_t(hdd_ctx::SOLVE_STATE_BYTES / 8), false, true, false};
// (the segments' states, the stop word and the table: Solve::Segments::carve_blocks)
constexpr Entry BLOCKS{"hdd_operator_solve_blocks", "hdd_operator_solve_blocks_workspace", 0, false, false, true};

// the arguments of an entry as its extern "C" function received them (hdd.h); what an entry does not have is 0
struct Call {
  hdd_ctx* ctx;
  const hdd_mesh* mesh;
  const hdd_csr* pattern;
  const double* const* d_vals;
  int32_t n_comp;
  const double* theta;   // [n_comp], with Entry::own [n_rhs][ldt]
  int64_t ldt;
  const hdd_block_range* range;
  const double* d_b;
  int64_t ldb;
  double* d_x;
  int64_t ldx;
  int32_t n_rhs;
  const hdd_solve_options* opt;
  double* d_work;
  int64_t n_work;
  double* d_history;
  int64_t ldh;
  hdd_solve_info* info;
  void* stream;
  int32_t n_blocks;        // Entry::segments
  const int64_t* bounds;   // [n_blocks + 1]
};

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

// head, four kinds of partial sums [column][SOLVE_PARTS], p q r z [column][even(rows)] (each column starting 16-byte
// aligned), the packed inverse blocks once -- a theta per column: once per column: Solve::carve
// E.segments: per segment a state and a table entry (eight doubles each), the stop word's eight, the partial sums of
// p . q (one per workgroup of the DOT apply: at most rows / 4 + 1 per segment, the CSR kernel with a wave per row) and
// four kinds of one per workgroup of the update (at most rows / (256 bs) + 1 per segment), p q r z and the inverse
// blocks of the interval: Solve::Segments::carve_blocks
int64_t blocks_doubles(int64_t rows, int bs) { return even(rows / bs * packed(bs)); }
int64_t blocks_pq(int64_t rows, int n_blocks) { return even(rows / 4 + n_blocks); }
int64_t blocks_parts(int64_t rows, int bs, int n_blocks) { return even(rows / (256 * int64_t(bs)) + n_blocks); }
int64_t workspace_doubles(const Entry& E, int64_t rows, int bs, int n)   // n: columns, or segments
{
  if (E.segments) return 16 * int64_t(n) + 8 + blocks_pq(rows, n) + 4 * blocks_parts(rows, bs, n) + 4 * even(rows) + blocks_doubles(rows, bs);
  return E.head + int64_t(n) * (4 * int64_t(dev::SOLVE_PARTS) + 4 * even(rows)) + (E.own ? n : 1) * blocks_doubles(rows, bs);
}

// what an entry's workspace function answers; block_size 0 (the mesh's nb, unknown here): enough for every block size
int64_t workspace_any(const Entry& E, int64_t rows, int block_size, int n, int n_max)
{
  if (rows < 0 || block_size < 0 || block_size > 8 || n < 1 || n > n_max) return 0;
  int64_t w = 0;
  for (int bs = block_size ? block_size : 1; bs <= (block_size ? block_size : 8); ++bs) w = std::max(w, workspace_doubles(E, rows, bs, n));
  return w;
}

dim3 grid(int64_t g) { return dim3(unsigned(g)); }

// a checked call: the plan, what the options resolve to, and the workspace
struct Solve {
  ApplyPlan P;
  int bs, n_rhs;
  bool pre, a16, dinv_tile, x0;
  int64_t rows, ldb, ldx, ldw, ldh;
  int64_t n_parts;   // workgroups of the init and update launches (= partial sums of r . z, r . r, b . b per column)
  int64_t dgrid;     // workgroups of the direction launch
  int32_t n_pq;      // workgroups of the DOT apply (= partial sums of p . q per column)
  hipStream_t s;
  dev::SolveState* state;   // [n_rhs]
  int32_t* stop;            // [groups] (batch)
  double *part_pq, *part_rz, *part_rr, *part_bb, *p, *q, *r, *z, *dinv, *x, *history;
  // a theta per column (hdd_operator_solve_multi): the caller's [n_rhs][ldt] (NULL: ones), column c's inverse blocks
  // at dinv + c * ld_dinv, its partial counts of indefinite blocks at part_pq + c * bad_stride; else zeros
  hdd::abi::ApplyThetas thetas;
  int64_t ld_dinv, bad_stride;
  // what only hdd_operator_solve_blocks has: the segments, their table in the workspace, the partial counts of
  // indefinite blocks and the real workgroups per kind of launch; the workspace's view for them
  struct Segments {
    int n_seg;
    const int64_t* bounds;
    dev::BlockSegment* tab;
    double* part_bad;
    int64_t total[dev::BLOCKS_KINDS];

    void carve_blocks(Solve& S, double* w)
    {
      S.state = reinterpret_cast<dev::SolveState*>(w), w += 8 * int64_t(n_seg);
      S.stop = reinterpret_cast<int32_t*>(w), w += 8;
      tab = reinterpret_cast<dev::BlockSegment*>(w), w += 8 * int64_t(n_seg);
      S.part_pq = w, w += blocks_pq(S.rows, n_seg);
      for (double** part : {&S.part_rz, &S.part_rr, &S.part_bb, &part_bad}) *part = w, w += blocks_parts(S.rows, S.bs, n_seg);
      for (double** vec : {&S.p, &S.q, &S.r, &S.z}) *vec = w, w += S.ldw;
      if (!S.pre) S.z = S.r;
      S.dinv = w;
    }
    dev::BlocksArgs blocks_args(const Solve& S, int kind) const { return dev::BlocksArgs{tab, n_seg, kind, S.P.a.row_begin, S.stop, &S.state->done_at}; }
    dev::SolveBlocks blocks(const Solve& S) const
    {
      return dev::SolveBlocks{blocks_args(S, dev::BLOCKS_PARTS), S.state, S.stop, S.x, S.p, S.q, S.r, S.z, S.dinv, S.part_pq, S.part_rz, S.part_rr,
                              S.part_bb, part_bad, S.history, S.ldh};
    }
  } seg;

  void carve(double* w, int64_t head)
  {
    state = reinterpret_cast<dev::SolveState*>(w);
    stop = reinterpret_cast<int32_t*>(w + HDD_MAX_VEC * (sizeof(dev::SolveState) / 8));
    w += head;
    for (double** part : {&part_pq, &part_rz, &part_rr, &part_bb}) *part = w, w += int64_t(n_rhs) * dev::SOLVE_PARTS;
    for (double** vec : {&p, &q, &r, &z}) *vec = w, w += n_rhs * ldw;
    if (!pre) z = r;
    dinv = w;
  }
  // column c alone: the setup kernels of both entries and the single solve's iteration
  dev::SolveVectors column(int c) const
  {
    return dev::SolveVectors{state + c, x + c * ldx, p + c * ldw, q + c * ldw, r + c * ldw, z + c * ldw, dinv + c * ld_dinv,
                             part_pq + int64_t(c) * n_pq, part_rz + c * n_parts, part_rr + c * n_parts, part_bb + c * n_parts,
                             rows, n_pq, history ? history + c * ldh : nullptr};
  }
  // the group of up to APPLY_NV columns that begins at g0
  dev::SolveBatch group(int g0) const
  {
    const dev::SolveVectors v = column(g0);
    return dev::SolveBatch{v.state, stop + g0 / NVB, v.x, ldx, v.p, v.q, v.r, v.z, ldw, v.dinv, v.part_pq, v.part_rz, v.part_rr,
                           rows, n_pq, std::min(NVB, n_rhs - g0), v.history, ldh, ld_dinv};
  }
};

// Every argument check of the entries, in the order of their messages, without a device call; fills S.  The single
// solve has n_rhs = 1 and dense leading dimensions, so the batch's checks pass; the blocks entry likewise, with the
// interval's rows.
int checked(const Entry& E, const Call& C, Solve& S)
{
  const char* who = E.who;
  const hdd_solve_options* opt = C.opt;
  int64_t ldb = C.ldb, ldx = C.ldx, ldh = C.ldh;
  if (!C.d_b || !C.d_x || !C.opt || !C.d_work || !C.info) return fail(HDD_ERR_INVALID, who, "null argument");
  if (C.n_rhs < 1 || C.n_rhs > HDD_MAX_VEC) return fail(HDD_ERR_INVALID, who, "n_rhs outside 1..HDD_MAX_VEC");
  if (E.segments) {
    if (int rc = hdd::abi::plan_blocks(who, C.ctx, C.mesh, C.pattern, C.d_vals, C.n_comp, C.theta, C.n_blocks, C.bounds, S.P)) return rc;
    ldb = ldx = S.P.rows();
  } else if (int rc = hdd::abi::plan_apply(who, C.ctx, C.mesh, C.pattern, C.d_vals, C.n_comp, E.own ? nullptr : C.theta, C.range, S.P, E.own))
    return rc;
  if (E.own && C.theta && C.ldt < C.n_comp) return fail(HDD_ERR_INVALID, who, "ldt smaller than n_comp");
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
  const int mesh_nb = C.mesh && hdd::abi::mesh_faces(C.mesh->elem_type)
                          ? hdd::abi::mesh_nb(C.mesh->elem_type, C.mesh->elem_type == HDD_HEX ? std::max(1, int(C.mesh->degree)) : 1)
                          : 0;
  if (bs == 0) {
    if (mesh_nb < 1 || mesh_nb > 8) return fail(HDD_ERR_INVALID, who, "block_size 0 needs a mesh with nb <= 8");
    bs = mesh_nb;
  }
  const int64_t rows = a.row_end - a.row_begin;
  if (a.row_begin % bs != 0 || rows % bs != 0)
    return fail(HDD_ERR_INVALID, who, "the bounds of the range are not multiples of block_size");
  for (int s = 1; s < C.n_blocks; ++s)
    if (C.bounds[s] % bs != 0) return fail(HDD_ERR_INVALID, who, "the bounds of the segments are not multiples of block_size");
  if (E.dense) ldb = ldx = rows, ldh = int64_t(opt->max_iter) + 1;
  if (ldb < rows || ldx < rows) return fail(HDD_ERR_INVALID, who, "ldb / ldx smaller than the range");
  if (C.d_history && ldh < int64_t(opt->max_iter) + 1) return fail(HDD_ERR_INVALID, who, "ldh smaller than max_iter + 1");
  if (C.n_work < workspace_doubles(E, rows, bs, E.segments ? C.n_blocks : C.n_rhs))
    return fail(HDD_ERR_INVALID, who, (std::string("n_work smaller than ") + E.workspace).c_str());
  S.bs = bs;
  S.n_rhs = C.n_rhs;
  S.pre = opt->precond == HDD_PRECOND_BLOCK_JACOBI;
  S.dinv_tile = S.P.tile && bs == S.P.nb;
  if (S.pre && !S.dinv_tile && (!C.pattern->row_ptr || !C.pattern->col))
    return fail(HDD_ERR_INVALID, who, "pattern without row_ptr / col (block_size != nb of the mesh)");
  if (!C.ctx->solve_state_h) return fail(HDD_ERR_INVALID, who, "context without its state buffer");
  // ---- every argument check is above ----
  for (int c = 0; c < (E.segments ? C.n_blocks : C.n_rhs); ++c) C.info[c] = hdd_solve_info{HDD_SOLVE_CONVERGED, 0, 0.0, 0.0};
  last_solve_kernels_slot().clear();
  S.x0 = (opt->flags & HDD_SOLVE_X0) != 0;
  S.rows = rows, S.ldb = ldb, S.ldx = ldx, S.ldw = even(rows), S.ldh = ldh;
  S.n_parts = std::max<int64_t>(1, std::min<int64_t>((rows / bs + 255) / 256, 2048));
  S.dgrid = std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, 4096));
  S.n_pq = int32_t(hdd::abi::dot_grid(C.ctx, S.P, dev::SOLVE_PARTS));
  S.s = static_cast<hipStream_t>(C.stream);
  S.x = C.d_x;
  S.history = C.d_history;
  S.thetas = hdd::abi::ApplyThetas{E.own ? C.theta : nullptr, C.ldt};
  S.ld_dinv = E.own ? blocks_doubles(rows, bs) : 0;
  S.bad_stride = E.own ? dev::SOLVE_PARTS : 0;
  // the 16-byte paths need every column of x aligned
  S.a16 = reinterpret_cast<uintptr_t>(C.d_work) % 16 == 0 && reinterpret_cast<uintptr_t>(C.d_x) % 16 == 0 && (C.n_rhs == 1 || ldx % 2 == 0);
  if (E.segments) {
    S.seg.n_seg = C.n_blocks;
    S.seg.bounds = C.bounds;
    S.seg.carve_blocks(S, C.d_work);
  } else
    S.carve(C.d_work, E.head);
  return HDD_OK;
}

// the runtime (bs, pre, a16) as compile-time <BS, PRE, A16> for f: A16 only with an even BS
template <int BS, class F>
hipError_t with_block_of(const Solve& S, F&& f)
{
  constexpr std::integral_constant<int, BS> bs{};
  constexpr std::bool_constant<BS % 2 == 0> even_bs{};
  if (S.pre) return S.a16 && even_bs ? f(bs, std::true_type{}, even_bs) : f(bs, std::true_type{}, std::false_type{});
  return S.a16 && even_bs ? f(bs, std::false_type{}, even_bs) : f(bs, std::false_type{}, std::false_type{});
}

template <class F>
hipError_t with_block(const Solve& S, F&& f)
{
  switch (S.bs) {
    case 1: return with_block_of<1>(S, f);
    case 2: return with_block_of<2>(S, f);
    case 3: return with_block_of<3>(S, f);
    case 4: return with_block_of<4>(S, f);
    case 5: return with_block_of<5>(S, f);
    case 6: return with_block_of<6>(S, f);
    case 7: return with_block_of<7>(S, f);
    default: return with_block_of<8>(S, f);
  }
}

// q = A p with p . q into part_pq for nv <= NV columns (leading dimension ldw; with E.own the group's columns begin at
// g0 and have their thetas), iteration k; the launch returns at once when *done_at <= k.  The grid is n_pq for every
// NV: the bits of p . q rest on it.
template <int NV>
hipError_t launch_apply_dot(const Entry& E, const Solve& S, int g0, const double* p, double* q, int nv, double* part_pq,
                            const int32_t* done_at, int k)
{
  dev::ApplyMultiArgs ma;
  dev::ApplyArgs& a = ma.a;
  a = S.P.a;
  a.nv = nv;
  a.x = p;
  a.y = q;
  a.ldx = a.ldy = S.ldw;
  a.partial = part_pq;
  a.done_at = done_at;
  a.iteration = k;
  if constexpr (NV == NVB)   // only the batch has a theta per column: no one-vector instantiation of the multi kernels
    if (E.own) {
      hdd::abi::apply_multi_thetas(ma, S.thetas, g0);
      return hdd::abi::launch_apply<NV, true>(S.P, ma, S.n_pq, S.s);
    }
  return hdd::abi::launch_apply<NV, true>(S.P, a, S.n_pq, S.s);
}

// names of the iteration's kernels; the batch's vector count is the instantiation's (APPLY_NV), not n_rhs
void name_kernels(const Entry& E, const Solve& S)
{
  const bool batched = !E.dense;
  const std::string nv = std::to_string(batched ? NVB : 1);
  std::string& nm = last_solve_kernels_slot();
  nm.clear();
  if (E.segments) {
    hdd::abi::apply_blocks_kernel_name(nm, S.P, true);
    nm += " + cg_update_blocks<" + std::to_string(S.bs) + (S.pre ? "" : ", none") + "> + cg_direction_blocks";
    return;
  }
  hdd::abi::apply_kernel_name(nm, S.P, E.own, batched ? NVB : 1, true);
  nm += " + cg_update<" + std::to_string(S.bs) + (S.pre ? "" : ", none");
  nm += batched ? ", " + nv + (E.own && S.pre ? ", own" : "") + "> + cg_direction<" + nv + ">" : "> + cg_direction";
}

// Setup of the entries: the inverse diagonal blocks once (their counts of indefinite blocks in part_pq, read by
// the init-state kernel before the first apply overwrites them) -- with a theta per column once per column, at
// theta_c, into the column's slice --, r = b - A x0 over all columns, then cg_init_kernel a column at a time on the
// single solve's grid (same sums).  The entry's init-state kernel follows.
int setup(const Entry& E, hdd_ctx* ctx, Solve& S, const double* d_b)
{
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, E.who);
  name_kernels(E, S);
  for (int c = 0; S.pre && c < (E.own ? S.n_rhs : 1); ++c) {
    dev::ApplyArgs a = S.P.a;
    for (int q = 0; E.own && q < a.n_comp; ++q) a.theta[q] = S.thetas.theta ? S.thetas.theta[c * S.thetas.ldt + q] : 1.0;
    double *dinv = S.dinv + c * S.ld_dinv, *part_bad = S.part_pq + c * S.bad_stride;
    e = with_block(S, [&](auto BS, auto, auto) {
      if (!S.dinv_tile) hipLaunchKernelGGL((dev::solve_dinv_csr_kernel<BS()>), grid(S.n_parts), dim3(256), 0, S.s, a, dinv, part_bad);
      if constexpr (BS() == 3 || BS() == 4)
        if (S.dinv_tile) hipLaunchKernelGGL((dev::solve_dinv_tile_kernel<BS(), BS()>), grid(S.n_parts), dim3(256), 0, S.s, a, dinv, part_bad);
      return hipGetLastError();
    });
    if (e != hipSuccess) return hip_fail(e, E.who);
  }
  if (S.x0)
    if (int rc = hdd::abi::run_apply(E.who, ctx, S.P, E.own ? &S.thetas : nullptr, S.x, S.ldx, S.q, S.ldw, S.n_rhs, S.s)) return rc;
  for (int c = 0; c < S.n_rhs; ++c) {
    e = with_block(S, [&](auto BS, auto PRE, auto A16) {
      hipLaunchKernelGGL((dev::cg_init_kernel<BS(), PRE(), A16()>), grid(S.n_parts), dim3(256), 0, S.s, S.column(c), d_b + c * S.ldb, S.x0);
      return hipGetLastError();
    });
    if (e != hipSuccess) return hip_fail(e, E.who);
  }
  return HDD_OK;
}

// `bytes` from the workspace into the context's pinned state buffer, and the wait for them: a look of the host
hipError_t fetch(hdd_ctx* ctx, const Solve& S, const void* from, size_t bytes)
{
  const hipError_t e = hipMemcpyAsync(ctx->solve_state_h, from, bytes, hipMemcpyDeviceToHost, S.s);
  return e == hipSuccess ? hipStreamSynchronize(S.s) : e;
}

// The iterations: min(check_every, remaining) times enqueue(k) between two looks of the entry at what it needs to
// know in the context's host buffer (look(k, done): done when everything has stopped by iteration k); until then or
// max_iter is reached.  k: iterations enqueued.
template <class F, class L>
int iterate(const Entry& E, const hdd_solve_options* opt, int& k, F&& enqueue, L&& look)
{
  const int every = opt->check_every > 0 ? opt->check_every : 32;
  for (k = 0;;) {
    const int batch = std::min(every, opt->max_iter - k);
    for (int i = 0; i < batch; ++i, ++k) {
      const hipError_t e = enqueue(k);
      if (e != hipSuccess) return hip_fail(e, E.who);
    }
    bool done = false;
    const hipError_t e = look(k, done);
    if (e != hipSuccess) return hip_fail(e, E.who);
    if (done || k >= opt->max_iter) return HDD_OK;
  }
}

// info of the n states (columns, segments) in the context's host buffer; state c owns the slice(c) = (offset, length)
// of x.  b_c = 0: x_c = 0 whatever the initial guess was
template <class F>
int finish(const Entry& E, hdd_ctx* ctx, const Solve& S, int k, int n, hdd_solve_info* info, F&& slice)
{
  const dev::SolveState* h = reinterpret_cast<const dev::SolveState*>(ctx->solve_state_h);
  hipError_t e = hipSuccess;
  bool cleared = false;
  for (int c = 0; c < n && e == hipSuccess; ++c) {
    info[c] = hdd_solve_info{h[c].done_at <= k ? h[c].status : HDD_SOLVE_MAX_ITER, h[c].iteration, std::sqrt(h[c].rr), std::sqrt(h[c].bb)};
    if (h[c].flags & dev::SOLVE_FLAG_ZERO_RHS) {
      const auto [at, length] = slice(c);
      e = hipMemsetAsync(S.x + at, 0, size_t(length) * sizeof(double), S.s);
      info[c].residual = 0.0;
      cleared = true;
    }
  }
  if (cleared && e == hipSuccess) e = hipStreamSynchronize(S.s);
  return e == hipSuccess ? HDD_OK : hip_fail(e, E.who);
}

// The entries by column.  One column (E.dense): per iteration the DOT apply, cg_update, cg_direction.  Several: per
// iteration and group of APPLY_NV columns the DOT apply on the single solve's dot grid, cg_update_batched on its update
// grid, cg_direction_batched; with E.own (hdd_operator_solve_multi) the applies are the multi-theta ones and
// cg_update_batched loads column c's own inverse blocks.  A look: the states of the columns.
int solve_columns(const Entry& E, const Call& C)
{
  Solve S;
  if (int rc = checked(E, C, S)) return rc;
  if (S.rows == 0) return HDD_OK;
  if (int rc = setup(E, C.ctx, S, C.d_b)) return rc;
  const dev::SolveVectors v = S.column(0);
  const int n_bad = S.pre ? int(S.n_parts) : 0;
  if (E.dense)
    hipLaunchKernelGGL(dev::cg_init_state_kernel, dim3(1), dim3(64), 0, S.s, v, int(S.n_parts), n_bad, C.opt->rtol, C.opt->atol);
  else
    hipLaunchKernelGGL(dev::cg_init_state_batched_kernel, dim3(1), dim3(64), 0, S.s, S.state, S.stop, int(S.n_rhs), S.part_pq, n_bad, S.part_bb,
                       S.part_rz, S.part_rr, int(S.n_parts), C.opt->rtol, C.opt->atol, S.history, S.ldh, S.bad_stride);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, E.who);
  auto one = [&](int k) {
    hipError_t e = launch_apply_dot<1>(E, S, 0, v.p, v.q, 1, v.part_pq, &v.state->done_at, k);
    if (e != hipSuccess) return e;
    return with_block(S, [&](auto BS, auto PRE, auto A16) {
      hipLaunchKernelGGL((dev::cg_update_kernel<BS(), PRE(), A16()>), grid(S.n_parts), dim3(256), 0, S.s, v, k);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(dev::cg_direction_kernel<PRE()>, grid(S.dgrid), dim3(256), 0, S.s, v, k, int(S.n_parts));
      return hipGetLastError();
    });
  };
  auto groups = [&](int k) {
    hipError_t e = hipSuccess;
    for (int g0 = 0; g0 < S.n_rhs && e == hipSuccess; g0 += NVB) {
      const dev::SolveBatch v = S.group(g0);
      e = launch_apply_dot<NVB>(E, S, g0, v.p, v.q, v.nv, v.part_pq, v.stop, k);
      if (e != hipSuccess) return e;
      e = with_block(S, [&](auto BS, auto PRE, auto A16) {
        if (E.own && PRE()) hipLaunchKernelGGL((dev::cg_update_batched_kernel<BS(), PRE(), A16(), NVB, PRE()>), grid(S.n_parts), dim3(256), 0, S.s, v, k);
        else hipLaunchKernelGGL((dev::cg_update_batched_kernel<BS(), PRE(), A16(), NVB>), grid(S.n_parts), dim3(256), 0, S.s, v, k);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((dev::cg_direction_batched_kernel<PRE(), NVB>), grid(S.dgrid), dim3(256), 0, S.s, v, k, int(S.n_parts));
        return hipGetLastError();
      });
    }
    return e;
  };
  const dev::SolveState* h = reinterpret_cast<const dev::SolveState*>(C.ctx->solve_state_h);
  auto look = [&](int k, bool& done) {
    const hipError_t e = fetch(C.ctx, S, S.state, E.dense ? sizeof(dev::SolveState) : size_t(hdd_ctx::SOLVE_STATE_BYTES));
    done = true;
    for (int c = 0; c < S.n_rhs; ++c) done = done && h[c].done_at <= k;
    return e;
  };
  int k;
  const int rc = E.dense ? iterate(E, C.opt, k, one, look) : iterate(E, C.opt, k, groups, look);
  return rc ? rc : finish(E, C.ctx, S, k, S.n_rhs, C.info, [&](int c) { return std::pair<int64_t, int64_t>(c * S.ldx, S.rows); });
}

// hdd_operator_solve_blocks: the single solve's setup and iteration on the segments' virtual grids (solve_kernels.hh):
// the table goes from the context's pinned buffer into the workspace in one copy, the inverse blocks of the whole
// interval are one launch, an iteration is three launches whatever n_blocks is.  A look: the stop-word launch and its
// 64 bytes; the states of all segments are read once, at the end.
int solve_segments(const Entry& E, const Call& C)
{
  Solve S;
  if (int rc = checked(E, C, S)) return rc;
  hdd_ctx* ctx = C.ctx;
  Solve::Segments& G = S.seg;
  if (!ctx->blocks_tab_h || !ctx->blocks_evt) return fail(HDD_ERR_INVALID, E.who, "context without its segment table");
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipEventSynchronize(ctx->blocks_evt);   // an earlier upload has read the pinned table
  if (e != hipSuccess) return hip_fail(e, E.who);
  auto* tab = static_cast<dev::BlockSegment*>(ctx->blocks_tab_h);
  hdd::abi::blocks_table(ctx, S.P, G.n_seg, G.bounds, S.bs, dev::SOLVE_PARTS, tab, G.total);
  if (G.total[dev::BLOCKS_DOT] > blocks_pq(S.rows, G.n_seg) || G.total[dev::BLOCKS_PARTS] > blocks_parts(S.rows, S.bs, G.n_seg))
    return fail(HDD_ERR_INVALID, E.who, "more partial sums than the workspace holds");
  e = hipMemcpyAsync(G.tab, tab, size_t(G.n_seg) * sizeof(dev::BlockSegment), hipMemcpyHostToDevice, S.s);
  if (e == hipSuccess) e = hipEventRecord(ctx->blocks_evt, S.s);
  if (e != hipSuccess) return hip_fail(e, E.who);
  name_kernels(E, S);

  // setup: the inverse blocks, r = b - A x0, the sums and the states, the stop word
  const dev::SolveBlocks v = G.blocks(S);
  const dim3 parts = grid(G.total[dev::BLOCKS_PARTS]);
  if (S.pre) {
    e = with_block(S, [&](auto BS, auto, auto) {
      if (!S.dinv_tile) hipLaunchKernelGGL((dev::solve_dinv_csr_blocks_kernel<BS()>), parts, dim3(256), 0, S.s, S.P.a, v.B, S.dinv, G.part_bad);
      if constexpr (BS() == 3 || BS() == 4)
        if (S.dinv_tile) hipLaunchKernelGGL((dev::solve_dinv_tile_blocks_kernel<BS(), BS()>), parts, dim3(256), 0, S.s, S.P.a, v.B, S.dinv, G.part_bad);
      return hipGetLastError();
    });
    if (e != hipSuccess) return hip_fail(e, E.who);
  }
  if (S.x0)
    if (int rc = hdd::abi::run_apply_blocks(E.who, ctx, S.P, G.tab, G.n_seg, G.total[dev::BLOCKS_APPLY], S.x, S.q, S.s)) return rc;
  e = with_block(S, [&](auto BS, auto PRE, auto A16) {
    hipLaunchKernelGGL((dev::cg_init_blocks_kernel<BS(), PRE(), A16()>), parts, dim3(256), 0, S.s, v, C.d_b, S.x0);
    return hipGetLastError();
  });
  if (e != hipSuccess) return hip_fail(e, E.who);
  hipLaunchKernelGGL(dev::cg_init_state_blocks_kernel, grid(G.n_seg), dim3(64), 0, S.s, v, S.pre, C.opt->rtol, C.opt->atol);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, E.who);
  auto stop_word = [&] {
    hipLaunchKernelGGL(dev::cg_stop_blocks_kernel, dim3(1), dim3(256), 0, S.s, S.state, G.n_seg, S.stop);
    return hipGetLastError();
  };
  if ((e = stop_word()) != hipSuccess) return hip_fail(e, E.who);   // the first value of the stop word

  dev::ApplyArgs a = S.P.a;
  a.nv = 1;
  a.x = S.p;
  a.y = S.q;
  a.ldx = a.ldy = S.ldw;
  a.partial = S.part_pq;
  a.done_at = nullptr;   // the segments' are in the table's view
  const dev::BlocksArgs dot = G.blocks_args(S, dev::BLOCKS_DOT);
  int k;
  const int rc = iterate(
      E, C.opt, k,
      [&](int k) {
        a.iteration = k;
        const hipError_t e = hdd::abi::launch_apply_blocks<true>(S.P, a, dot, G.total[dev::BLOCKS_DOT], S.s);
        if (e != hipSuccess) return e;
        return with_block(S, [&](auto BS, auto PRE, auto A16) {
          hipLaunchKernelGGL((dev::cg_update_blocks_kernel<BS(), PRE(), A16()>), grid(G.total[dev::BLOCKS_PARTS] + 1), dim3(256), 0, S.s, v, k);
          const hipError_t e = hipGetLastError();
          if (e != hipSuccess) return e;
          hipLaunchKernelGGL(dev::cg_direction_blocks_kernel<PRE()>, grid(G.total[dev::BLOCKS_DIRECTION]), dim3(256), 0, S.s, v, k);
          return hipGetLastError();
        });
      },
      [&](int k, bool& done) {
        hipError_t e = stop_word();
        if (e == hipSuccess) e = fetch(ctx, S, S.stop, 64);
        done = *reinterpret_cast<const int32_t*>(ctx->solve_state_h) <= k;
        return e;
      });
  if (rc) return rc;
  if ((e = fetch(ctx, S, S.state, size_t(G.n_seg) * sizeof(dev::SolveState))) != hipSuccess) return hip_fail(e, E.who);
  return finish(E, ctx, S, k, G.n_seg, C.info,
                [&](int s) { return std::pair<int64_t, int64_t>(G.bounds[s] - G.bounds[0], G.bounds[s + 1] - G.bounds[s]); });
}
}  // namespace

extern "C" const char* hdd_last_solve_kernels(void) { return last_solve_kernels_slot().c_str(); }

extern "C" int64_t hdd_operator_solve_workspace(int64_t rows, int32_t block_size) { return workspace_any(SINGLE, rows, block_size, 1, 1); }

extern "C" int64_t hdd_operator_solve_batched_workspace(int64_t rows, int32_t block_size, int32_t n_rhs)
{
  return workspace_any(BATCHED, rows, block_size, n_rhs, HDD_MAX_VEC);
}

extern "C" int64_t hdd_operator_solve_multi_workspace(int64_t rows, int32_t block_size, int32_t n_rhs)
{
  return workspace_any(MULTI, rows, block_size, n_rhs, HDD_MAX_VEC);
}

extern "C" int64_t hdd_operator_solve_blocks_workspace(int64_t rows, int32_t block_size, int32_t n_blocks)
{
  return workspace_any(BLOCKS, rows, block_size, n_blocks, HDD_MAX_SOLVE_BLOCKS);
}

extern "C" int hdd_operator_solve(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                  int32_t n_comp, const double* theta, const hdd_block_range* range, const double* d_b,
                                  double* d_x, const hdd_solve_options* opt, double* d_work, int64_t n_work,
                                  double* d_history, hdd_solve_info* info, void* stream)
{
  return solve_columns(SINGLE, Call{ctx, mesh, pattern, d_vals, n_comp, theta, 0, range, d_b, 0, d_x, 0, 1, opt, d_work, n_work, d_history, 0, info,
                                    stream, 0, nullptr});
}

extern "C" int hdd_operator_solve_batched(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                          int32_t n_comp, const double* theta, const hdd_block_range* range, const double* d_b,
                                          int64_t ldb, double* d_x, int64_t ldx, int32_t n_rhs, const hdd_solve_options* opt,
                                          double* d_work, int64_t n_work, double* d_history, int64_t ldh, hdd_solve_info* info,
                                          void* stream)
{
  return solve_columns(BATCHED, Call{ctx, mesh, pattern, d_vals, n_comp, theta, 0, range, d_b, ldb, d_x, ldx, n_rhs, opt, d_work, n_work, d_history,
                                     ldh, info, stream, 0, nullptr});
}

// A theta per column: the same affine components at n_rhs parameters.
extern "C" int hdd_operator_solve_multi(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                        int32_t n_comp, const double* theta, int64_t ldt, const hdd_block_range* range,
                                        const double* d_b, int64_t ldb, double* d_x, int64_t ldx, int32_t n_rhs,
                                        const hdd_solve_options* opt, double* d_work, int64_t n_work, double* d_history,
                                        int64_t ldh, hdd_solve_info* info, void* stream)
{
  return solve_columns(MULTI, Call{ctx, mesh, pattern, d_vals, n_comp, theta, ldt, range, d_b, ldb, d_x, ldx, n_rhs, opt, d_work, n_work, d_history,
                                   ldh, info, stream, 0, nullptr});
}

// Every segment of a partition per call.
extern "C" int hdd_operator_solve_blocks(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                         int32_t n_comp, const double* theta, int32_t n_blocks, const int64_t* bounds,
                                         const double* d_b, double* d_x, const hdd_solve_options* opt, double* d_work,
                                         int64_t n_work, double* d_history, int64_t ldh, hdd_solve_info* info, void* stream)
{
  return solve_segments(BLOCKS, Call{ctx, mesh, pattern, d_vals, n_comp, theta, 0, nullptr, d_b, 0, d_x, 0, 1, opt, d_work, n_work, d_history, ldh,
                                     info, stream, n_blocks, bounds});
}
