// dune-hdd_amd/csrc/kernels/comm.hip
//
// The communicators of the sharded step (hdd_comm: RCCL owned / wrapped, host-staged, in-process device transport)
// and the exchange they post: the device hub with its injected stall, hdd_comm_post / _post_direct / _wait.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>

#include "shard_internal.hh"

using hdd::set_error;
using namespace hdd::shard;

// The injected stall: one wave spins (s_sleep between polls) until the host opens the gate or max_ticks of the
// 100 MHz real-time counter have passed -- every launch ends by itself.
__global__ void __launch_bounds__(64) hub_gate_kernel(const uint32_t* gate, uint64_t max_ticks)
{
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (__hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u &&
         __builtin_amdgcn_s_memrealtime() - t0 < max_ticks)
    __builtin_amdgcn_s_sleep(100);
}

static void hub_release(hdd_device_hub* h)
{
  if (!h) return;
  bool last;
  {
    std::lock_guard<std::mutex> lk(h->m);
    last = --h->refs == 0;
  }
  if (last) {
    if (h->gate) (void)hipHostFree(h->gate);
    delete h;
  }
}

extern "C" int hdd_device_hub_create(int32_t nranks, hdd_device_hub** out)
{
  if (!out || nranks < 1) return set_error(HDD_ERR_INVALID, "hdd_device_hub_create: invalid argument");
  auto* h = new hdd_device_hub;
  h->nranks = nranks;
  h->ch.resize(size_t(nranks) * size_t(nranks));
  *out = h;
  return HDD_OK;
}

extern "C" void hdd_device_hub_destroy(hdd_device_hub* hub) { hub_release(hub); }

extern "C" int hdd_device_hub_stall(hdd_device_hub* hub, int32_t rank, double max_seconds)
{
  if (!hub || rank < 0 || rank >= hub->nranks || !(max_seconds > 0.0) || max_seconds > 600.0)
    return set_error(HDD_ERR_INVALID, "hdd_device_hub_stall: invalid argument");
  std::lock_guard<std::mutex> lk(hub->m);
  if (!hub->gate) {
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&hub->gate), 64, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) {
      hub->gate = nullptr;
      return hip_fail(e, "hdd_device_hub_stall: gate word");
    }
  }
  __atomic_store_n(hub->gate, 0u, __ATOMIC_SEQ_CST);
  hub->stall_rank = rank;
  hub->stall_s = max_seconds;
  return HDD_OK;
}

extern "C" int hdd_device_hub_release(hdd_device_hub* hub)
{
  if (!hub) return set_error(HDD_ERR_INVALID, "hdd_device_hub_release: null hub");
  std::lock_guard<std::mutex> lk(hub->m);
  if (hub->gate) __atomic_store_n(hub->gate, 1u, __ATOMIC_SEQ_CST);
  hub->stall_rank = -1;
  return HDD_OK;
}


// ------------------------------------------------------------------------------------------------
// communicators
// ------------------------------------------------------------------------------------------------
static int comm_rccl_streams(hdd_comm* c)
{
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->xfer, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ready, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, local_event_flags());
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_comm: transfer stream / events");
}

extern "C" int hdd_rccl_get_unique_id(void* id)
{
  if (!id) return set_error(HDD_ERR_INVALID, "hdd_rccl_get_unique_id: null id");
  static_assert(sizeof(ncclUniqueId) == HDD_RCCL_ID_BYTES, "ncclUniqueId size");
  const RcclApi& R = rccl();
  if (!R.ok) return set_error(HDD_ERR_UNSUPPORTED, "hdd_rccl_get_unique_id: " + R.err);
  ncclUniqueId u;
  const ncclResult_t r = R.GetUniqueId(&u);
  if (r != ncclSuccess) return nccl_fail(r, "ncclGetUniqueId");
  std::memcpy(id, &u, sizeof(u));
  return HDD_OK;
}

extern "C" int hdd_comm_create_rccl(const void* id, int32_t nranks, int32_t rank, int32_t hip_device, hdd_comm** out)
{
  if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks)
    return set_error(HDD_ERR_INVALID, "hdd_comm_create_rccl: invalid argument");
  const RcclApi& R = rccl();
  if (!R.ok) return set_error(HDD_ERR_UNSUPPORTED, "hdd_comm_create_rccl: " + R.err);
  auto* c = new hdd_comm;
  c->kind = hdd_comm::RCCL_OWNED;
  c->device = hip_device;
  int rc = comm_rccl_streams(c);
  if (rc) {
    hdd_comm_destroy(c);
    return rc;
  }
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  const ncclResult_t r = R.CommInitRank(&c->nccl, nranks, u, rank);
  if (r != ncclSuccess) {
    c->nccl = nullptr;
    hdd_comm_destroy(c);
    return nccl_fail(r, "ncclCommInitRank");
  }
  *out = c;
  return HDD_OK;
}

extern "C" int hdd_comm_wrap_rccl(void* nccl_comm, int32_t hip_device, hdd_comm** out)
{
  if (!nccl_comm || !out) return set_error(HDD_ERR_INVALID, "hdd_comm_wrap_rccl: invalid argument");
  const RcclApi& R = rccl();
  if (!R.ok) return set_error(HDD_ERR_UNSUPPORTED, "hdd_comm_wrap_rccl: " + R.err);
  auto* c = new hdd_comm;
  c->kind = hdd_comm::RCCL_WRAPPED;
  c->device = hip_device;
  c->nccl = static_cast<ncclComm_t>(nccl_comm);
  int rc = comm_rccl_streams(c);
  if (rc) {
    hdd_comm_destroy(c);
    return rc;
  }
  *out = c;
  return HDD_OK;
}

extern "C" int hdd_comm_create_host(hdd_host_exchange_fn fn, void* user, int32_t hip_device, hdd_comm** out)
{
  if (!fn || !out) return set_error(HDD_ERR_INVALID, "hdd_comm_create_host: invalid argument");
  auto* c = new hdd_comm;
  c->kind = hdd_comm::HOST;
  c->device = hip_device;
  c->fn = fn;
  c->user = user;
  *out = c;
  return HDD_OK;
}

extern "C" int hdd_comm_create_device(hdd_device_hub* hub, int32_t rank, int32_t hip_device, hdd_comm** out)
{
  if (!hub || !out || rank < 0 || rank >= hub->nranks)
    return set_error(HDD_ERR_INVALID, "hdd_comm_create_device: invalid argument");
  auto* c = new hdd_comm;
  c->kind = hdd_comm::DEVICE;
  c->device = hip_device;
  c->rank = rank;
  int rc = comm_rccl_streams(c);
  hipError_t e = hipSuccess;
  c->copied.assign(size_t(hub->nranks), nullptr);
  for (auto& ev : c->copied)
    if (rc == HDD_OK && e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (rc == HDD_OK && e != hipSuccess) rc = hip_fail(e, "hdd_comm_create_device: events");
  if (rc) {
    hdd_comm_destroy(c);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(hub->m);
    ++hub->refs;
  }
  c->hub = hub;
  *out = c;
  return HDD_OK;
}

extern "C" void hdd_comm_destroy(hdd_comm* c)
{
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->xfer) (void)hipStreamSynchronize(c->xfer);
  if (c->kind == hdd_comm::RCCL_OWNED && c->nccl && rccl().ok) (void)rccl().CommDestroy(c->nccl);
  if (c->ready) (void)hipEventDestroy(c->ready);
  if (c->done) (void)hipEventDestroy(c->done);
  for (hipEvent_t ev : c->copied)
    if (ev) (void)hipEventDestroy(ev);
  if (c->gated) (void)hipEventDestroy(c->gated);
  if (c->xfer) (void)hipStreamDestroy(c->xfer);
  if (c->pinned) (void)hipHostFree(c->pinned);
  hub_release(c->hub);
  delete c;
}

// DEVICE transport: the group send/recv of one rank.  On the transfer stream (which already waits for the packs
// on `stream`): for every source rank, wait for its packed event, copy its messages into the receive buffers,
// record "copied"; then wait for every destination's "copied" event, so that -- as after ncclGroupEnd -- the
// completion event covers the sends too and the next pack cannot overwrite a send buffer that is still read.
// Host side: publish this rank's sends, then block until each source has published (RCCL blocks on the device
// instead; a thread per rank makes the host rendezvous harmless).  Messages of one directed pair match in order,
// zero-count messages are skipped on both sides (as RCCL does).
static int device_post(hdd_comm* c, int32_t n_peers, const int32_t* peers, const double* const* d_send,
                       const int64_t* send_count, double* const* d_recv, const int64_t* recv_count)
{
  hdd_device_hub& H = *c->hub;
  const int32_t me = c->rank, n = H.nranks;
  std::map<int32_t, std::vector<std::pair<const double*, int64_t>>> out;
  std::map<int32_t, std::vector<std::pair<double*, int64_t>>> in;
  for (int32_t k = 0; k < n_peers; ++k) {
    if (peers[k] < 0 || peers[k] >= n || send_count[k] < 0 || recv_count[k] < 0)
      return set_error(HDD_ERR_INVALID, "hdd_comm_post: peer or count out of range (device transport)");
    if (send_count[k] > 0) out[peers[k]].emplace_back(d_send[k], send_count[k]);
    if (recv_count[k] > 0) in[peers[k]].emplace_back(d_recv[k], recv_count[k]);
  }
  const auto limit = std::chrono::duration<double>(H.timeout_s);
  auto fail = [&](std::unique_lock<std::mutex>& lk, const std::string& msg) {
    if (H.failed.empty()) H.failed = msg;
    lk.unlock();
    H.cv.notify_all();
    return set_error(HDD_ERR_INVALID, "hdd_comm_post (device transport): " + msg);
  };
  hipEvent_t packed_ev = c->ready;   // recorded on the pack stream by the caller; the transfer stream waits for it
  {
    std::lock_guard<std::mutex> lk(H.m);
    if (H.stall_rank == me && H.gate) {   // injected stall: the sends complete only once the gate opens
      if (!c->gated && hipEventCreateWithFlags(&c->gated, hipEventDisableTiming) != hipSuccess) c->gated = nullptr;
      uint32_t* dgate = nullptr;
      hipError_t e = c->gated ? hipHostGetDevicePointer(reinterpret_cast<void**>(&dgate), H.gate, 0) : hipErrorOutOfMemory;
      if (e == hipSuccess) {
        hipLaunchKernelGGL(hub_gate_kernel, dim3(1), dim3(64), 0, c->xfer, dgate, uint64_t(H.stall_s * 1.0e8));
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipEventRecord(c->gated, c->xfer);
      if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: injected stall (device transport)");
      packed_ev = c->gated;
      H.stall_rank = -1;   // one post
    }
  }
  {   // 1. publish
    std::lock_guard<std::mutex> lk(H.m);
    for (auto& [dst, msgs] : out) {
      auto& q = H.ch[size_t(me) * n + dst];
      q.msgs = msgs;
      q.packed = packed_ev;
      ++q.sent;
    }
  }
  H.cv.notify_all();
  // 2. receives: wait for each source's publication, copy on the transfer stream, record copied
  for (auto& [src, msgs] : in) {
    auto& q = H.ch[size_t(src) * n + me];
    std::vector<std::pair<const double*, int64_t>> sent;
    hipEvent_t packed;
    {
      std::unique_lock<std::mutex> lk(H.m);
      if (!H.cv.wait_for(lk, limit, [&] { return q.sent > q.consumed || !H.failed.empty(); }))
        return fail(lk, "rank " + std::to_string(me) + " timed out waiting for rank " + std::to_string(src));
      if (!H.failed.empty()) return set_error(HDD_ERR_INVALID, "hdd_comm_post (device transport): " + H.failed);
      if (q.msgs.size() != msgs.size())
        return fail(lk, "rank " + std::to_string(src) + " sent " + std::to_string(q.msgs.size()) + " messages to rank " +
                            std::to_string(me) + ", which receives " + std::to_string(msgs.size()));
      for (size_t i = 0; i < msgs.size(); ++i)
        if (q.msgs[i].second != msgs[i].second)
          return fail(lk, "message size mismatch between rank " + std::to_string(src) + " and rank " + std::to_string(me));
      sent = q.msgs;
      packed = q.packed;
    }
    hipError_t e = hipStreamWaitEvent(c->xfer, packed, 0);
    for (size_t i = 0; i < msgs.size() && e == hipSuccess; ++i)
      e = hipMemcpyAsync(msgs[i].first, sent[i].first, size_t(msgs[i].second) * sizeof(double), hipMemcpyDefault, c->xfer);
    if (e == hipSuccess) e = hipEventRecord(c->copied[size_t(src)], c->xfer);
    if (e != hipSuccess) {
      std::unique_lock<std::mutex> lk(H.m);
      return fail(lk, std::string("HIP error on rank ") + std::to_string(me) + ": " + hipGetErrorString(e));
    }
    {
      std::lock_guard<std::mutex> lk(H.m);
      q.copied = c->copied[size_t(src)];
      ++q.consumed;
    }
    H.cv.notify_all();
  }
  // 3. sends complete when every destination has copied them
  for (auto& [dst, msgs] : out) {
    auto& q = H.ch[size_t(me) * n + dst];
    hipEvent_t copied;
    {
      std::unique_lock<std::mutex> lk(H.m);
      if (!H.cv.wait_for(lk, limit, [&] { return q.consumed == q.sent || !H.failed.empty(); }))
        return fail(lk, "rank " + std::to_string(me) + " timed out waiting for rank " + std::to_string(dst) + " to receive");
      if (!H.failed.empty()) return set_error(HDD_ERR_INVALID, "hdd_comm_post (device transport): " + H.failed);
      copied = q.copied;
    }
    const hipError_t e = hipStreamWaitEvent(c->xfer, copied, 0);
    if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: wait for the receivers (device transport)");
  }
  return HDD_OK;
}

// the group send/recv of one post, on the transfer stream or (direct) on the caller's
static int rccl_group_sendrecv(hdd_comm* c, int32_t n_peers, const int32_t* peers, const double* const* d_send,
                               const int64_t* send_count, double* const* d_recv, const int64_t* recv_count,
                               hipStream_t stream)
{
  const RcclApi& R = rccl();
  ncclResult_t r = R.GroupStart();
  if (r != ncclSuccess) return nccl_fail(r, "ncclGroupStart");
  for (int32_t k = 0; k < n_peers; ++k) {
    if (send_count[k] > 0) {
      r = R.Send(d_send[k], size_t(send_count[k]), ncclFloat64, peers[k], c->nccl, stream);
      if (r != ncclSuccess) break;
    }
    if (recv_count[k] > 0) {
      r = R.Recv(d_recv[k], size_t(recv_count[k]), ncclFloat64, peers[k], c->nccl, stream);
      if (r != ncclSuccess) break;
    }
  }
  const ncclResult_t r2 = R.GroupEnd();
  if (r != ncclSuccess) return nccl_fail(r, "ncclSend/ncclRecv");
  if (r2 != ncclSuccess) return nccl_fail(r2, "ncclGroupEnd");
  return HDD_OK;
}

// host-staged: device -> pinned host -> fn -> device, all ordered on `stream`
static int host_post(hdd_comm* c, int32_t n_peers, const int32_t* peers, const double* const* d_send,
                     const int64_t* send_count, double* const* d_recv, const int64_t* recv_count, hipStream_t s)
{
  size_t total = 0;
  for (int32_t k = 0; k < n_peers; ++k) {
    if (send_count[k] < 0 || recv_count[k] < 0) return set_error(HDD_ERR_INVALID, "hdd_comm_post: negative count");
    total += size_t(send_count[k]) + size_t(recv_count[k]);
  }
  hipError_t e = hipSuccess;
  if (total > c->pinned_doubles) {
    if (c->pinned) (void)hipHostFree(c->pinned);
    c->pinned = nullptr;
    c->pinned_doubles = 0;
    e = hipHostMalloc(reinterpret_cast<void**>(&c->pinned), std::max<size_t>(total, 1) * sizeof(double), 0);
    if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: pinned staging");
    c->pinned_doubles = total;
  }
  std::vector<const double*> hs(n_peers);
  std::vector<double*> hr(n_peers);
  size_t off = 0;
  for (int32_t k = 0; k < n_peers; ++k) {
    hs[k] = c->pinned + off;
    off += size_t(send_count[k]);
    hr[k] = c->pinned + off;
    off += size_t(recv_count[k]);
    if (send_count[k]) {
      e = hipMemcpyAsync(const_cast<double*>(hs[k]), d_send[k], size_t(send_count[k]) * sizeof(double),
                         hipMemcpyDeviceToHost, s);
      if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: D2H");
    }
  }
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: synchronize");
  const int rc = c->fn(c->user, n_peers, peers, hs.data(), send_count, hr.data(), recv_count);
  if (rc != HDD_OK) return set_error(rc, "hdd_comm_post: host transport failed (status " + std::to_string(rc) + ")");
  for (int32_t k = 0; k < n_peers; ++k)
    if (recv_count[k]) {
      e = hipMemcpyAsync(d_recv[k], hr[k], size_t(recv_count[k]) * sizeof(double), hipMemcpyHostToDevice, s);
      if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: H2D");
    }
  // the staging buffer is reused by the next post: the copies must have left it
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: synchronize");
  c->posted = true;
  return HDD_OK;
}

int hdd::shard::comm_post(hdd_comm* c, int32_t n_peers, const int32_t* peers, const double* const* d_send,
                          const int64_t* send_count, double* const* d_recv, const int64_t* recv_count, void* stream,
                          bool direct, hipEvent_t also_ready, hipEvent_t also_done)
{
  if (!c || n_peers < 0 || (n_peers && (!peers || !d_send || !send_count || !d_recv || !recv_count)))
    return set_error(HDD_ERR_INVALID, "hdd_comm_post: invalid argument");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: hipSetDevice");
  c->last_peers.clear();
  for (int32_t k = 0; k < n_peers; ++k)
    if (std::find(c->last_peers.begin(), c->last_peers.end(), peers[k]) == c->last_peers.end())
      c->last_peers.push_back(peers[k]);
  c->direct = nullptr;
  if (c->kind == hdd_comm::HOST) return host_post(c, n_peers, peers, d_send, send_count, d_recv, recv_count, s);
  direct = direct && c->kind != hdd_comm::DEVICE;   // RCCL only
  const hipStream_t xs = direct ? s : c->xfer;      // where the exchange runs
  e = hipEventRecord(c->ready, s);
  if (e == hipSuccess && also_ready) e = hipEventRecord(also_ready, s);
  if (direct) {
    if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: record ready");
  } else {   // the transfer stream starts after the packs already enqueued on `stream`
    if (e == hipSuccess) e = hipStreamWaitEvent(c->xfer, c->ready, 0);
    if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: order transfer after pack");
  }
  const int rc = c->kind == hdd_comm::DEVICE
                     ? device_post(c, n_peers, peers, d_send, send_count, d_recv, recv_count)
                     : rccl_group_sendrecv(c, n_peers, peers, d_send, send_count, d_recv, recv_count, xs);
  if (rc) return rc;
  e = hipEventRecord(c->done, xs);
  if (e == hipSuccess && also_done) e = hipEventRecord(also_done, xs);
  if (e != hipSuccess) return hip_fail(e, "hdd_comm_post: record completion");
  c->posted = true;
  if (direct) c->direct = s;
  return HDD_OK;
}

extern "C" int hdd_comm_post(hdd_comm* c, int32_t n_peers, const int32_t* peers, const double* const* d_send,
                             const int64_t* send_count, double* const* d_recv, const int64_t* recv_count, void* stream)
{
  return comm_post(c, n_peers, peers, d_send, send_count, d_recv, recv_count, stream, false);
}

extern "C" int hdd_comm_post_direct(hdd_comm* c, int32_t n_peers, const int32_t* peers, const double* const* d_send,
                                    const int64_t* send_count, double* const* d_recv, const int64_t* recv_count,
                                    void* stream)
{
  return comm_post(c, n_peers, peers, d_send, send_count, d_recv, recv_count, stream, true);
}

extern "C" int hdd_comm_wait(hdd_comm* c, void* stream)
{
  if (!c) return set_error(HDD_ERR_INVALID, "hdd_comm_wait: null comm");
  if (!c->posted) return HDD_OK;
  c->posted = false;
  if (c->kind == hdd_comm::HOST) return HDD_OK;   // already ordered on the stream by hdd_comm_post
  if (c->direct && c->direct == static_cast<hipStream_t>(stream)) {   // posted on this very stream
    c->direct = nullptr;
    return HDD_OK;
  }
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = hipStreamWaitEvent(static_cast<hipStream_t>(stream), c->done, 0);
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_comm_wait");
}
