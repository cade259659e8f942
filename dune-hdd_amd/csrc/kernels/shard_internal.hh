// dune-hdd_amd/csrc/kernels/shard_internal.hh -- what the files of the sharded step share: the objects behind the
// opaque handles of hdd.h (hdd_device_hub, hdd_comm: comm.hip; hdd_shard: shard.hip), the run-time RCCL table
// (rccl_api.hip) and comm_post (comm.hip, called by shard_step.hip with its stage events).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "hdd.h"
#include "../host/hdd_internal.hh"

// ------------------------------------------------------------------------------------------------
// in-process device transport (hdd_device_hub): several ranks of one process (one thread each, any devices)
// exchanging device buffers with the stream / event schedule of an RCCL group send/recv.  Per directed pair
// (src, dst) a channel holds the sender's latest publication -- its message list and its "packed" event (the
// send buffers are complete) -- and the receiver's "consumed" event (its copies out of them are complete).
// ------------------------------------------------------------------------------------------------
struct hdd_device_hub {
  struct Channel {
    uint64_t sent = 0, consumed = 0;     // publications by src / publications dst has copied out of
    std::vector<std::pair<const double*, int64_t>> msgs;
    hipEvent_t packed = nullptr;         // src's event after its packs
    hipEvent_t copied = nullptr;         // dst's event after its copies out of publication `consumed`
  };
  int32_t nranks = 0;
  std::mutex m;
  std::condition_variable cv;
  std::vector<Channel> ch;               // [src * nranks + dst]
  std::string failed;                    // first protocol error (every waiting rank returns it)
  int refs = 1;
  double timeout_s = 120.0;
  // error injection (hdd_device_hub_stall): the next post of rank `stall_rank` gates its sends behind a device-side
  // wait for a host word (a peer whose sends never complete, bounded by stall_s), released by hdd_device_hub_release
  int32_t stall_rank = -1;
  double stall_s = 0.0;
  uint32_t* gate = nullptr;              // pinned host word (device-visible): 0 = closed
};

struct hdd_comm {
  enum Kind { RCCL_OWNED, RCCL_WRAPPED, HOST, DEVICE } kind = HOST;
  int device = 0;
  ncclComm_t nccl = nullptr;
  hipStream_t xfer = nullptr;          // transfer stream (RCCL, DEVICE)
  hipEvent_t ready = nullptr, done = nullptr;
  bool posted = false;
  hdd_host_exchange_fn fn = nullptr;
  void* user = nullptr;
  double* pinned = nullptr;            // host staging (HOST)
  size_t pinned_doubles = 0;
  hdd_device_hub* hub = nullptr;       // DEVICE: the hub, this rank, one "copied" event per source rank
  int32_t rank = 0;
  std::vector<hipEvent_t> copied;
  hipEvent_t gated = nullptr;          // DEVICE, injected stall: the sends' event behind the gate
  std::vector<int32_t> last_peers;     // the peers of the last post (watchdog messages)
  hipStream_t direct = nullptr;        // RCCL: the caller's stream the last post ran on directly (serial step)
};

struct hdd_shard {
  int device = 0;
  hdd_local* local = nullptr;
  hdd_grid_info gi{};
  hdd_local_info li{};
  int32_t rank = 0, nranks = 1, s_begin = 0, s_end = 0, degree = 1;
  int64_t nnz = 0;
  std::vector<int64_t> gid;            // host global ids [n_local]
  // device mesh (shard-owned)
  double* d_coords = nullptr;
  int32_t* d_nbrs = nullptr;
  uint32_t* d_finfo = nullptr;
  int64_t* d_gid = nullptr;
  int32_t* d_ev = nullptr;             // vertex-indexed geometry (2d): element -> local vertex ids
  double* d_vxy = nullptr;             //   and the rank-local vertex coordinates (owned + ghost elements')
  // halo
  std::vector<int32_t> peers;
  std::vector<int64_t> send_prefix, recv_prefix, recv_col0;
  int32_t* d_send_idx = nullptr;
  double* d_sbuf = nullptr;
  double* d_rbuf = nullptr;
  int32_t max_rows = 0;
  // tiles
  int32_t* d_tiles_in = nullptr;
  int32_t* d_tiles_bd = nullptr;
  int32_t* d_fix = nullptr;            // owned elements (relative to own_begin) with a ghost face neighbour
  int64_t n_tiles = 0, n_in = 0, n_bd = 0, n_fix = 0;
  int64_t halo_faces = 0;
  // host copies of the plan (hdd_shard_halo_lists / hdd_shard_tile_lists)
  std::vector<int32_t> send_idx, tiles_in, tiles_bd;
  bool host_only = false;          // created without a context: no device arrays
  // side stream of the loopback study (HDD_SHARD_NO_TRANSFER): pack + copies off the assembly stream, as the
  // RCCL path runs them on the transfer stream; created on first use
  hipStream_t aux = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  double* d_fixbuf = nullptr;          // side buffers of the off-stream fixup (n_comp x (n_fix + 1) x fix_rb)
  size_t fixbuf_doubles = 0;
  // watchdog (hdd_block_step_query / _sync): the stages the last step recorded events for, and a marker event
  uint32_t stages = 0;                 // bit 0: pack (ev_pack), 1: exchange (ev_xdone), 2: element pass (ev_out)
  hipEvent_t ev_pack = nullptr, ev_xdone = nullptr;   // recorded beside the communicator's ready / done (comm_post)
  std::vector<int32_t> stage_peers;    // the halo peers of the last step (watchdog messages)
  hipEvent_t ev_mark = nullptr;
  bool marked = false;
};

#pragma GCC visibility push(hidden)   // internal: none of this is an exported symbol
namespace hdd {
namespace shard {

inline int hip_fail(hipError_t e, const char* where)
{
  return set_error(HDD_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

// Events that only order two streams of ONE device (the step's side stream against `stream`, RCCL's transfer
// stream back into `stream`): the data both sides touch stays on that device, so a device-scope release /
// acquire is enough.  A default event's record is a system-scope release -- an L2 write-back of everything the
// previous tile launch left dirty -- which sits between two launches of back-to-back steps (C4 N = 8 one-card
// trace, profiles/r04/q_btb/: 12.5 us of 93 us per step with nothing running).  Events another device waits on
// (the device transport's "packed" = comm->ready, read by peer copies; RCCL may read send buffers from a peer)
// keep the system fence.  HDD_EVENT_SYSTEM_FENCE=1 restores it everywhere (A/B).
inline unsigned local_event_flags()
{
  static const bool sys = getenv("HDD_EVENT_SYSTEM_FENCE") != nullptr;
  return sys ? hipEventDisableTiming : hipEventDisableTiming | hipEventDisableSystemFence;
}

// RCCL, resolved at run time (rccl_api.hip)
struct RcclApi {
  bool ok = false;
  std::string err;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
const RcclApi& rccl();
int nccl_fail(ncclResult_t r, const char* where);

// limits of the halo kernels' argument block (HaloArgs, shard_step.hip): arrays per message, peers per shard
constexpr int SH_MAX_ARR = 16;
constexpr int SH_MAX_PEERS = 64;

// hdd_comm_post / hdd_comm_post_direct (comm.hip).  direct (RCCL only; the serial step): the group send/recv on
// `stream` itself instead of the transfer stream -- nothing overlaps it there, and it saves the two cross-stream hops
// (ready -> transfer stream, done -> `stream`), ~5 us each on the one-card traces; the ready / done
// events are still recorded for the watchdog.
// also_ready / also_done (optional): events of the caller recorded right after the communicator's own ready / done
// events on the same streams -- the sharded step's watchdog stages, owned by the shard, so that a later post on the
// same communicator or its destruction cannot change what the step query reports
int comm_post(hdd_comm* c, int32_t n_peers, const int32_t* peers, const double* const* d_send,
              const int64_t* send_count, double* const* d_recv, const int64_t* recv_count, void* stream, bool direct,
              hipEvent_t also_ready = nullptr, hipEvent_t also_done = nullptr);

}  // namespace shard
}  // namespace hdd
#pragma GCC visibility pop
