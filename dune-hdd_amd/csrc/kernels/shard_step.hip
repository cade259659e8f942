// dune-hdd_amd/csrc/kernels/shard_step.hip
//
// One step of the sharded BlockSWIPDG (hdd_block_assemble_sharded; the shard is shard.hip, the communicators
// comm.hip): pack (one kernel, every peer) -> post the exchange (RCCL group send/recv on the communicator's
// transfer stream, or a host transport) -> interior 64-element tiles on the caller's stream while the halo is in
// flight -> stream waits for the receives -> unpack into the ghost columns -> the tiles that touch a ghost.
//
// The entry point validates, builds the halo row layout (HaloArgs), asks csrc/host/shard_plan.hh for the schedule
// (a pure function of the shard's shape, the flags and the communicator kind; the measurements behind every default
// are there), makes sure the streams, events and the fix buffer the plan needs exist, and runs the stages in order.
// A stage looks at the plan, never at the flags.  Last: the watchdog over the stage events.
#include <algorithm>
#include <chrono>
#include <thread>

#include "shard_internal.hh"
#include "shard_plan.hh"

using hdd::set_error;
using namespace hdd::shard;
using hdd::Schedule;
using hdd::StepPlan;

namespace {

// ------------------------------------------------------------------------------------------------
// halo pack / unpack: message of peer p = [rows][count_p] doubles at buf + R * prefix[p]
// ------------------------------------------------------------------------------------------------
struct HaloArgs {
  double* arr[SH_MAX_ARR];             // element-column arrays [rows][ld]
  int32_t row_first[SH_MAX_ARR + 1];   // first halo row of each array
  int32_t n_arrays, n_peers;
  int64_t ld;
  int64_t prefix[SH_MAX_PEERS + 1];    // element prefix over the peers' messages
  int64_t col0[SH_MAX_PEERS];          // unpack: first ghost column of peer p
  const int32_t* idx;                  // pack: concatenated send lists (local element ids)
  double* buf;
};

__device__ __forceinline__ void halo_slot(const HaloArgs& a, int64_t t, int& p, int& arr, int64_t& rr, int64_t& i)
{
  const int R = a.row_first[a.n_arrays];
  p = 0;
  while (p + 1 < a.n_peers && int64_t(R) * a.prefix[p + 1] <= t) ++p;
  const int64_t cnt = a.prefix[p + 1] - a.prefix[p];
  const int64_t loc = t - int64_t(R) * a.prefix[p];
  const int64_t r = loc / cnt;
  i = loc - r * cnt;
  arr = 0;
  while (arr + 1 < a.n_arrays && a.row_first[arr + 1] <= r) ++arr;
  rr = r - a.row_first[arr];
}

__global__ void __launch_bounds__(256) halo_pack_kernel(const HaloArgs a)
{
  const int64_t total = int64_t(a.row_first[a.n_arrays]) * a.prefix[a.n_peers];
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    int p, arr;
    int64_t rr, i;
    halo_slot(a, t, p, arr, rr, i);
    a.buf[t] = a.arr[arr][rr * a.ld + a.idx[a.prefix[p] + i]];
  }
}

__global__ void __launch_bounds__(256) halo_unpack_kernel(const HaloArgs a)
{
  const int64_t total = int64_t(a.row_first[a.n_arrays]) * a.prefix[a.n_peers];
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    int p, arr;
    int64_t rr, i;
    halo_slot(a, t, p, arr, rr, i);
    a.arr[arr][rr * a.ld + a.col0[p] + i] = a.buf[t];
  }
}

hipError_t launch_halo(bool pack, const HaloArgs& a, hipStream_t s)
{
  const int64_t total = int64_t(a.row_first[a.n_arrays]) * a.prefix[a.n_peers];
  if (total == 0) return hipSuccess;
  const unsigned grid = unsigned(std::min<int64_t>((total + 255) / 256, 1024));
  if (pack) hipLaunchKernelGGL(halo_pack_kernel, dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(halo_unpack_kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// one call: its arguments, what the set-up derives from them, what its launches returned
// ------------------------------------------------------------------------------------------------
struct StepCall {
  hdd_ctx* ctx;
  hdd_comm* comm;
  const hdd_scalar_fn* kappa;
  int32_t n_comp;
  const hdd_tensor_fn* tensor;
  const hdd_swipdg_params* params;
  const hdd_csr* pattern;
  double* const* d_vals;
  void* stream;
  hdd_mesh m;
  HaloArgs h;                      // the halo row layout; prefix / idx / buf: the pack's until the loopback unpacks
  bool transfer;                   // not the HDD_SHARD_NO_TRANSFER loopback
  hipStream_t s, ps;               // `stream`; the stream of the exchange (plan.pack_on), the pack and the element pass
  std::vector<double*> fbufs;      // the fix buffer, one slot per component
  int64_t soa_ld;
  int32_t rb, reserve;
  double* loop_buf;                // what the loopback's unpack reads
  bool tiles_done = false;         // the full-range launch went first
  bool fix_unsupported = false;    // no list kernel for these rules: the whole range again after the join
  bool split_unsupported = false;  // no tile-list kernel: everything after the halo
};

// f(ctx, mesh, kappa, n_comp, tensor, params, pattern, rest...): every assembly entry point starts alike
template <class F, class... Rest>
int assemble(F f, const StepCall& c, Rest... rest)
{
  return f(c.ctx, &c.m, c.kappa, c.n_comp, c.tensor, c.params, c.pattern, rest...);
}

int assemble_all(const StepCall& c) { return assemble(hdd_swipdg_assemble, c, c.d_vals, c.stream); }

hipError_t ensure_event(hipEvent_t* ev, unsigned flags)
{
  return *ev ? hipSuccess : hipEventCreateWithFlags(ev, flags);
}

// the host transport ran on the shard's side stream and the fixup runs on `stream`: the ghost columns were written
// on ps, so `stream` needs ev_out (with an off-stream fixup the element pass follows on ps and records it anyway)
bool host_on_side(const StepPlan& p, const StepCall& c)
{
  return c.transfer && p.schedule == Schedule::FixInline && c.comm->kind == hdd_comm::HOST;
}

// 2. halo rows: [coordinates] [tensor] [per-element diffusion factors (each distinct array once)]
int halo_layout(const hdd_shard* sh, uint32_t flags, StepCall& c)
{
  HaloArgs& h = c.h;   // (zero so far)
  h.ld = sh->li.n_local;
  h.n_peers = int32_t(sh->peers.size());
  // (no de-duplication of arrays passed twice: the message layout must depend on the kinds only, which
  // every rank passes alike, never on pointer identity)
  auto add = [&](double* p, int rows) {
    h.arr[h.n_arrays] = p;
    h.row_first[h.n_arrays + 1] = h.row_first[h.n_arrays] + rows;
    ++h.n_arrays;
  };
  if (flags & HDD_SHARD_HALO_GEOMETRY) add(sh->d_coords, sh->gi.dim * sh->gi.nvpe);
  if (c.tensor->kind == HDD_TENSOR_ISO_PER_ELEM || c.tensor->kind == HDD_TENSOR_SYM_PER_ELEM) {
    if (!c.tensor->per_elem) return set_error(HDD_ERR_INVALID, "hdd_block_assemble_sharded: tensor per_elem missing");
    add(const_cast<double*>(c.tensor->per_elem),
        c.tensor->kind == HDD_TENSOR_ISO_PER_ELEM ? 1 : (sh->gi.dim == 3 ? 6 : 3));
  }
  for (int32_t k = 0; k < c.n_comp; ++k)
    if (c.kappa[k].kind == HDD_FN_PER_ELEM) {
      if (!c.kappa[k].per_elem) return set_error(HDD_ERR_INVALID, "hdd_block_assemble_sharded: kappa per_elem missing");
      add(const_cast<double*>(c.kappa[k].per_elem), 1);
    }
  for (int k = 0; k <= h.n_peers; ++k) h.prefix[k] = sh->send_prefix[k];
  h.idx = sh->d_send_idx;
  h.buf = sh->d_sbuf;
  return HDD_OK;
}

// 3. the facts the plan depends on
hdd::StepFacts step_facts(const hdd_shard* sh, uint32_t flags, const StepCall& c)
{
  bool closed_form = true;
  for (int32_t k = 0; k < c.n_comp; ++k)
    closed_form = closed_form && (c.kappa[k].kind == HDD_FN_CONST || c.kappa[k].kind == HDD_FN_PER_ELEM);
#ifdef HDD_ABLATION
  const bool ablation = true;
#else
  const bool ablation = false;
#endif
  const hdd::CommKind kind = !c.comm                          ? hdd::CommKind::None
                             : c.comm->kind == hdd_comm::HOST ? hdd::CommKind::Host
                                                              : hdd::CommKind::Stream;
  return {sh->gi.elem_type, c.h.n_peers, sh->n_in, sh->n_fix, flags, c.transfer, kind, closed_form, ablation};
}

// 4. what the plan needs, created on first use: the side stream and its two events, the watchdog's stage events,
// the fix buffer (first step, or more components: grow; warm up before graph capture)
int ensure_resources(hdd_shard* sh, const StepPlan& p, StepCall& c)
{
  hipError_t e = hipSuccess;
  if (p.side_stream() && !sh->aux) {   // loopback study, host transport (which stages through the host on its stream)
    e = hipStreamCreateWithFlags(&sh->aux, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(e, "hdd_block_assemble_sharded: side stream");
  }
  if (p.side()) {
    e = ensure_event(&sh->ev_in, local_event_flags());
    if (e == hipSuccess) e = ensure_event(&sh->ev_out, local_event_flags());
    if (e != hipSuccess) return hip_fail(e, "hdd_block_assemble_sharded: event");
  }
  c.ps = p.pack_on == hdd::PackOn::Transfer ? c.comm->xfer : p.pack_on == hdd::PackOn::Side ? sh->aux : c.s;
  if (c.transfer && c.comm->kind != hdd_comm::HOST &&
      (ensure_event(&sh->ev_pack, hipEventDisableTiming) != hipSuccess ||
       ensure_event(&sh->ev_xdone, hipEventDisableTiming) != hipSuccess))
    return set_error(HDD_ERR_HIP, "hdd_block_assemble_sharded: stage event");
  c.rb = hdd_fix_rb(sh->gi.elem_type);
  c.soa_ld = (sh->n_fix + 1 + 63) & ~int64_t(63);   // SoA rows start 512-byte aligned
  c.reserve = int32_t(std::min<int64_t>((sh->n_fix + 63) / 64, 256));
  c.loop_buf = sh->d_rbuf;
  if (p.fix_buffer()) {
    const size_t slot = size_t(p.schedule == Schedule::FixSoa ? c.soa_ld : sh->n_fix + 1) * size_t(c.rb);
    const size_t need = slot * size_t(c.n_comp);
    if (need > sh->fixbuf_doubles) {
      if (sh->d_fixbuf) (void)hipFree(sh->d_fixbuf);
      sh->d_fixbuf = nullptr;
      sh->fixbuf_doubles = 0;
      e = hipMalloc(reinterpret_cast<void**>(&sh->d_fixbuf), need * sizeof(double));
      if (e != hipSuccess) return hip_fail(e, "hdd_block_assemble_sharded: fixup buffer");
      sh->fixbuf_doubles = need;
    }
    for (int32_t k = 0; k < c.n_comp; ++k) c.fbufs.push_back(sh->d_fixbuf + size_t(k) * slot);
  }
  return HDD_OK;
}

// after an error behind a successful post: the communicator must not stay posted
int abandon(const StepCall& c, int rc)
{
  if (c.transfer) (void)hdd_comm_wait(c.comm, c.stream);
  return rc;
}

// the loopback study's unpack of its own messages, on `on`
int unpack_loopback(const hdd_shard* sh, StepCall& c, hipStream_t on)
{
  HaloArgs& h = c.h;
  for (int k = 0; k <= h.n_peers; ++k) h.prefix[k] = sh->recv_prefix[k];
  for (int k = 0; k < h.n_peers; ++k) h.col0[k] = sh->recv_col0[k];
  h.idx = nullptr;
  h.buf = c.loop_buf;
  const hipError_t e = launch_halo(false, h, on);
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_block_assemble_sharded: unpack");
}

// ------------------------------------------------------------------------------------------------
// 5. the stages, in the order they are enqueued
// ------------------------------------------------------------------------------------------------

// The side schedules fork here: the Q1 pack on `stream` ahead of the tile launch, then the inputs event the pack
// stream starts from -- recorded before the tile launch, so the halo work does not wait for the tiles.
int stage_fork(hdd_shard* sh, const StepPlan& p, StepCall& c)
{
  hipError_t e = hipSuccess;
  if (p.pack_first) {
    e = launch_halo(true, c.h, c.s);
    if (e != hipSuccess) return hip_fail(e, "hdd_block_assemble_sharded: pack");
  }
  if (p.side()) {
    e = hipEventRecord(sh->ev_in, c.s);
    if (e == hipSuccess) e = hipStreamWaitEvent(c.ps, sh->ev_in, 0);
    if (e != hipSuccess) return hip_fail(e, "hdd_block_assemble_sharded: order pack after inputs");
  }
  return HDD_OK;
}

// The full-range launch first: the SKIP launch of the in-place fixup or the SoA side buffer's reserve launch.
int stage_tiles_first(hdd_shard*, const StepPlan& p, StepCall& c)
{
  if (!p.tiles_first) return HDD_OK;
  const int rc = p.schedule == Schedule::FixSoa ? assemble(hdd_assemble_reserve, c, c.d_vals, c.stream, c.reserve)
                                                : assemble(hdd_assemble_skip_ghost, c, c.d_vals, c.stream, c.reserve);
  if (rc == HDD_OK) c.tiles_done = true;
  return rc == HDD_ERR_UNSUPPORTED ? HDD_OK : rc;   // (unsupported rules: stage_tiles, in round 3's order)
}

// pack the records the peers need (one launch for every peer; Q1 side schedules: done in stage_fork)
int stage_pack(hdd_shard*, const StepPlan& p, StepCall& c)
{
  if (p.pack_first) return HDD_OK;
  const hipError_t e = launch_halo(true, c.h, c.ps);
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_block_assemble_sharded: pack");
}

// Post the exchange.  The receives land straight in the ghost columns: the ghosts of one owner are contiguous
// (recv_col0), so peer k's message is R row messages [row r][count_k], each received into
// arr(r)[row(r) ld + recv_col0[k] ...] -- no receive buffer, no unpack launch.  Sender and receiver list the
// rows in the same order (the layout depends on the kinds only), which is how RCCL / the host transports
// match repeated (peer) messages.
int stage_post(hdd_shard* sh, const StepPlan& p, StepCall& c)
{
  const HaloArgs& h = c.h;
  const int32_t R = h.row_first[h.n_arrays];
  std::vector<int32_t> mp;
  std::vector<const double*> ms;
  std::vector<double*> mr;
  std::vector<int64_t> mn, mrn;
  for (int k = 0; k < h.n_peers; ++k) {
    const int64_t scnt = sh->send_prefix[k + 1] - sh->send_prefix[k];
    const int64_t rcnt = sh->recv_prefix[k + 1] - sh->recv_prefix[k];
    for (int32_t r = 0, a = 0; r < R; ++r) {
      while (a + 1 < h.n_arrays && h.row_first[a + 1] <= r) ++a;
      mp.push_back(sh->peers[size_t(k)]);
      ms.push_back(sh->d_sbuf + int64_t(R) * sh->send_prefix[k] + int64_t(r) * scnt);
      mn.push_back(scnt);
      mr.push_back(h.arr[a] + int64_t(r - h.row_first[a]) * h.ld + sh->recv_col0[k]);
      mrn.push_back(rcnt);
    }
  }
  const bool staged = c.comm->kind != hdd_comm::HOST;   // the watchdog's pack / exchange events
  const int rc = comm_post(c.comm, int32_t(mp.size()), mp.data(), ms.data(), mn.data(), mr.data(), mrn.data(), c.ps,
                           p.direct, staged ? sh->ev_pack : nullptr, staged ? sh->ev_xdone : nullptr);
  if (rc) return rc;
  if (staged) sh->stages |= 3u;
  sh->stage_peers = c.comm->last_peers;
  if (host_on_side(p, c) && hipEventRecord(sh->ev_out, c.ps) != hipSuccess)
    return set_error(HDD_ERR_HIP, "hdd_block_assemble_sharded: host transport event");
  return HDD_OK;
}

// Timing studies: the receive buffers get this rank's own messages (stream-ordered device copies).
// With equal send and receive counts per peer (every halo here: ghost layers are symmetric) the loopback is ONE
// kernel, the unpack reading the send buffer -- as the transfer is: RCCL's group kernel receives straight into
// the ghost columns.  (Round 4 and earlier: a copy per peer + the unpack, i.e. 2-3 kernels for one transfer.)
int stage_loopback(hdd_shard* sh, const StepPlan& p, StepCall& c)
{
  const HaloArgs& h = c.h;
  const int64_t R = h.row_first[h.n_arrays];
  bool same = true;
  for (int k = 0; k < h.n_peers; ++k)
    same = same && sh->send_prefix[k + 1] - sh->send_prefix[k] == sh->recv_prefix[k + 1] - sh->recv_prefix[k];
  if (same) c.loop_buf = sh->d_sbuf;
  for (int k = 0; k < h.n_peers && !same; ++k) {
    const int64_t n =
        R * std::min(sh->send_prefix[k + 1] - sh->send_prefix[k], sh->recv_prefix[k + 1] - sh->recv_prefix[k]);
    if (n > 0 && hipMemcpyAsync(sh->d_rbuf + R * sh->recv_prefix[k], sh->d_sbuf + R * sh->send_prefix[k],
                                size_t(n) * sizeof(double), hipMemcpyDeviceToDevice, c.ps) != hipSuccess)
      return set_error(HDD_ERR_HIP, "hdd_block_assemble_sharded: loopback copy");
  }
  if (p.side() && hipEventRecord(sh->ev_out, c.ps) != hipSuccess)
    return set_error(HDD_ERR_HIP, "hdd_block_assemble_sharded: loopback event");
  return HDD_OK;
}

// Off-stream fixup: on the stream the halo lands on, right after it, the ghost-adjacent elements in place or into
// the side buffer -- concurrent with the assembly, which needs the LDS this pass does without; the loopback study
// unpacks there first.
int stage_element_pass(hdd_shard* sh, const StepPlan& p, StepCall& c)
{
  if (!p.off_stream_fix()) return HDD_OK;
  int rc = c.transfer ? HDD_OK : unpack_loopback(sh, c, c.ps);
  if (rc) return rc;
  rc = p.schedule == Schedule::FixSoa
           ? assemble(hdd_assemble_elements_soa, c, c.fbufs.data(), c.soa_ld, sh->d_fix, sh->n_fix, c.ps)
       : p.schedule == Schedule::FixRowBlocks
           ? assemble(hdd_assemble_elements_buf, c, c.fbufs.data(), sh->d_fix, sh->n_fix, c.ps)
           : assemble(hdd_assemble_elements_inplace, c, c.d_vals, sh->d_fix, sh->n_fix, c.ps);
  if (rc == HDD_ERR_UNSUPPORTED) c.fix_unsupported = true;   // no list kernel for these rules: range again later
  else if (rc) return abandon(c, rc);
  const hipError_t e = hipEventRecord(sh->ev_out, c.ps);
  if (e != hipSuccess) return hip_fail(e, "hdd_block_assemble_sharded: record fixup");
  sh->stages |= 4u;
  return HDD_OK;
}

// The assembly overlaps the transfer.  Side schedules: EVERY tile (one full-size launch at full rate; the row
// blocks of the ghost-adjacent elements read ghost columns the receives are still writing, so the in-place pass's
// launch skips them and the other schedules recompute them).  SplitTiles: the interior tiles only (the kernels that
// take lists: P1 / Q1 persistent policies) -- a second launch of whole boundary tiles later, which on thin strips is
// a large fraction.
int stage_tiles(hdd_shard* sh, const StepPlan& p, StepCall& c)
{
  if (!p.overlap() || c.tiles_done) return HDD_OK;
  const bool split = p.schedule == Schedule::SplitTiles;
  // in-place fixup running: the tiles leave the ghost-adjacent elements' row blocks to it
  const bool skip = p.schedule == Schedule::FixInPlace && !c.fix_unsupported;
  const int rc = split  ? assemble(hdd_swipdg_assemble_tiles, c, c.d_vals, sh->d_tiles_in, sh->n_in, c.stream)
                 : skip ? assemble(hdd_assemble_skip_ghost, c, c.d_vals, c.stream, c.reserve)
                        : assemble_all(c);
  if (rc == HDD_ERR_UNSUPPORTED && split) c.split_unsupported = true;
  else if (rc) return abandon(c, rc);
  return HDD_OK;
}

// `stream` after the receives (transfers receive in place; the loopback study unpacks) and after the element pass
int stage_join(hdd_shard* sh, const StepPlan& p, StepCall& c)
{
  if (c.transfer) {
    const int rc = hdd_comm_wait(c.comm, c.stream);
    if (rc) return rc;
    if (host_on_side(p, c) && hipStreamWaitEvent(c.s, sh->ev_out, 0) != hipSuccess)
      return set_error(HDD_ERR_HIP, "hdd_block_assemble_sharded: wait host transport");
  }
  if (p.off_stream_fix()) {
    const hipError_t e = hipStreamWaitEvent(c.s, sh->ev_out, 0);
    return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_block_assemble_sharded: join fixup");
  }
  if (c.transfer) return HDD_OK;
  if (p.side() && hipStreamWaitEvent(c.s, sh->ev_out, 0) != hipSuccess)
    return set_error(HDD_ERR_HIP, "hdd_block_assemble_sharded: wait loopback");
  return unpack_loopback(sh, c, c.s);
}

// Last: the side buffer's row blocks into place, or the rows that read a ghost (or everything without overlap)
int stage_ghost_rows(hdd_shard* sh, const StepPlan& p, StepCall& c)
{
  if (p.off_stream_fix()) {
    if (c.fix_unsupported) return assemble_all(c);
    if (p.schedule == Schedule::FixSoa)
      return hdd_scatter_fix_q1_soa(c.ctx, &c.m, c.pattern, c.fbufs.data(), c.soa_ld, c.n_comp, sh->d_fix, sh->n_fix,
                                    c.d_vals, c.stream);
    if (p.schedule == Schedule::FixRowBlocks)
      return hdd_scatter_fix(c.ctx, c.pattern, c.rb, c.fbufs.data(), c.n_comp, sh->d_fix, sh->n_fix, c.d_vals,
                             c.stream);
    return HDD_OK;   // in place: the join alone completes the step on `stream`
  }
  if (p.overlap() && !c.split_unsupported) {
    if (p.schedule == Schedule::SplitTiles)
      return assemble(hdd_swipdg_assemble_tiles, c, c.d_vals, sh->d_tiles_bd, sh->n_bd, c.stream);
    const int rc = assemble(hdd_swipdg_assemble_elements, c, c.d_vals, sh->d_fix, sh->n_fix, c.stream);
    if (rc != HDD_ERR_UNSUPPORTED) return rc;   // (no list kernel for these rules: the whole range again)
  }
  return assemble_all(c);
}

}  // namespace

extern "C" int hdd_block_assemble_sharded(hdd_ctx* ctx, hdd_shard* sh, hdd_comm* comm, const hdd_scalar_fn* kappa,
                                          int32_t n_comp, const hdd_tensor_fn* tensor,
                                          const hdd_swipdg_params* params, const hdd_csr* pattern,
                                          double* const* d_vals, uint32_t flags, void* stream)
{
  // 1. validate
  if (!ctx || !sh || !kappa || !tensor || !params || !pattern || !d_vals)
    return set_error(HDD_ERR_INVALID, "hdd_block_assemble_sharded: null argument");
  if (sh->host_only)
    return set_error(HDD_ERR_INVALID, "hdd_block_assemble_sharded: host-only shard (created without a context)");
  if (n_comp < 1 || n_comp > HDD_MAX_COMP)
    return set_error(HDD_ERR_INVALID, "hdd_block_assemble_sharded: need 1 <= n_comp <= HDD_MAX_COMP");
  if (pattern->nnz != sh->nnz || pattern->n_rows != int64_t(sh->gi.nb) * (sh->li.own_end - sh->li.own_begin))
    return set_error(HDD_ERR_INVALID, "hdd_block_assemble_sharded: pattern does not belong to this shard");
  StepCall c{ctx, comm, kappa, n_comp, tensor, params, pattern, d_vals, stream};
  hdd_shard_mesh(sh, &c.m);
  if (flags & HDD_SHARD_HALO_GEOMETRY) {   // ghost geometry arrives through the halo: element-major coords
    c.m.elem_vertices = nullptr;
    c.m.vertex_coords = nullptr;
  }
  c.s = static_cast<hipStream_t>(stream);
  // 2. the halo row layout; without rows or peers the step is one assembly
  int rc = halo_layout(sh, flags, c);
  if (rc) return rc;
  const bool exchange = c.h.n_peers > 0 && !(flags & HDD_SHARD_NO_HALO) && c.h.n_arrays > 0;
  if (!exchange) return assemble_all(c);
  c.transfer = !(flags & HDD_SHARD_NO_TRANSFER);
  if (!comm && c.transfer)
    return set_error(HDD_ERR_INVALID, "hdd_block_assemble_sharded: the shard has halo peers but comm is NULL");
  if (c.h.row_first[c.h.n_arrays] > sh->max_rows)
    return set_error(HDD_ERR_INVALID, "hdd_block_assemble_sharded: too many halo rows");
  const hipError_t e = hipSetDevice(sh->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_block_assemble_sharded: hipSetDevice");
  sh->stages = 0;
  sh->stage_peers.clear();   // a step that times out without a post names no peers, not the previous step's
  sh->marked = false;
  // 3. plan, 4. resources
  const StepPlan p = hdd::plan_step(step_facts(sh, flags, c));
  rc = ensure_resources(sh, p, c);
  if (rc) return rc;
  // 5. the stages
  using Stage = int (*)(hdd_shard*, const StepPlan&, StepCall&);
  const Stage stages[] = {stage_fork,         stage_tiles_first, stage_pack, c.transfer ? stage_post : stage_loopback,
                          stage_element_pass, stage_tiles,       stage_join, stage_ghost_rows};
  for (const Stage stage : stages) {
    rc = stage(sh, p, c);
    if (rc) return rc;
  }
  return HDD_OK;
}

// ------------------------------------------------------------------------------------------------
// watchdog: which stage of the last sharded step has not completed.  A lost peer shows as a step that never
// completes on the device (RCCL waits inside its kernels), so a caller that would block in a device synchronize
// can instead poll these events with a deadline and report the rank and stage before exiting.
// ------------------------------------------------------------------------------------------------
static const char* const stage_names[] = {"complete", "halo pack", "halo exchange (group send/recv)",
                                          "ghost-adjacent element pass", "tile assembly and join"};

extern "C" int hdd_block_step_mark(hdd_shard* sh, void* stream)
{
  if (!sh || sh->host_only) return set_error(HDD_ERR_INVALID, "hdd_block_step_mark: invalid shard");
  hipError_t e = hipSetDevice(sh->device);
  if (e == hipSuccess && !sh->ev_mark) e = hipEventCreateWithFlags(&sh->ev_mark, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(sh->ev_mark, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "hdd_block_step_mark");
  sh->marked = true;
  return HDD_OK;
}

extern "C" int hdd_block_step_query(hdd_shard* sh, int32_t* stage)
{
  if (!sh || !stage || sh->host_only) return set_error(HDD_ERR_INVALID, "hdd_block_step_query: invalid argument");
  const hipEvent_t evs[4] = {(sh->stages & 1u) ? sh->ev_pack : nullptr, (sh->stages & 2u) ? sh->ev_xdone : nullptr,
                             (sh->stages & 4u) ? sh->ev_out : nullptr, sh->marked ? sh->ev_mark : nullptr};
  *stage = HDD_STAGE_COMPLETE;
  for (int i = 0; i < 4; ++i) {
    if (!evs[i]) continue;
    const hipError_t e = hipEventQuery(evs[i]);
    if (e == hipErrorNotReady) {
      *stage = i + 1;
      return HDD_OK;
    }
    if (e != hipSuccess) return hip_fail(e, "hdd_block_step_query");
  }
  return HDD_OK;
}

extern "C" const char* hdd_block_stage_name(int32_t stage)
{
  return stage >= 0 && stage <= HDD_STAGE_ASSEMBLY ? stage_names[stage] : "unknown stage";
}

extern "C" int hdd_block_step_sync(hdd_shard* sh, void* stream, double timeout_s)
{
  int rc = hdd_block_step_mark(sh, stream);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    int32_t st = 0;
    rc = hdd_block_step_query(sh, &st);
    if (rc) return rc;
    if (st == HDD_STAGE_COMPLETE) return HDD_OK;
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (dt > timeout_s) {
      std::string peers;
      for (int32_t p : sh->stage_peers) peers += (peers.empty() ? "" : ", ") + std::to_string(p);
      return set_error(HDD_ERR_TIMEOUT, "rank " + std::to_string(sh->rank) + " of " + std::to_string(sh->nranks) +
                                            ": the sharded step's " + stage_names[st] + " did not complete within " +
                                            std::to_string(timeout_s) + " s (halo peers: " +
                                            (peers.empty() ? "none" : peers) + ")");
    }
    std::this_thread::sleep_for(std::chrono::microseconds(dt < 0.01 ? 20 : 1000));
  }
}
