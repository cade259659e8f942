// dune-hdd_amd/csrc/kernels/ctx.hh -- the context behind hdd_ctx* (internal; shared by the abi_*.hip files,
// pattern.hip and block_ops.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "hdd.h"
#include "../host/hdd_internal.hh"

#pragma GCC visibility push(hidden)   // internal: none of this is an exported symbol

// A buffer the context keeps between calls and grows on demand (never shrinks): allocation happens only on the first
// call of a size class, so warm a context up once before capturing a call into a hipGraph.  How much is allocated and
// what is waited for before the old buffer is freed differs per buffer, so every call site names both.
struct DeviceScratch {
  enum Slack { EXACT, QUARTER };                              // allocate need, or need + need / 4
  enum SyncBeforeFree { NO_SYNC, SYNC_STREAM, SYNC_DEVICE };  // before an old buffer is freed (stream: reserve's s)
  void* p = nullptr;
  size_t bytes = 0;
  const bool pinned_host;   // pinned host memory instead of device memory

  explicit DeviceScratch(bool pinned_host_ = false) : pinned_host(pinned_host_) {}
  DeviceScratch(const DeviceScratch&) = delete;
  DeviceScratch& operator=(const DeviceScratch&) = delete;
  ~DeviceScratch() { release(); }

  hipError_t reserve(size_t need, Slack slack, SyncBeforeFree sync, hipStream_t s = nullptr)
  {
    if (need <= bytes) return hipSuccess;
    // as the call sites always did: the stream is waited for on a first allocation too and its status ignored;
    // the device only when there is a buffer to free, and a failure ends the call
    if (sync == SYNC_STREAM) (void)hipStreamSynchronize(s);
    if (sync == SYNC_DEVICE && p) {
      const hipError_t e = hipDeviceSynchronize();
      if (e != hipSuccess) return e;
    }
    release();
    const size_t grow = slack == QUARTER ? need + need / 4 : need;
    const hipError_t e = pinned_host ? hipHostMalloc(&p, grow, hipHostMallocDefault) : hipMalloc(&p, grow);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    bytes = grow;
    return hipSuccess;
  }

  void release()
  {
    if (p) (void)(pinned_host ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    bytes = 0;
  }
};

struct hdd_ctx {
  int device = 0;
  DeviceScratch ws;         // device workspace (per-element coefficient records of the p=3 hex kernel)
  // read once at hdd_ctx_create, never per launch
  int n_cu = 256;           // hipDeviceAttributeMultiprocessorCount
  int debug_flags = 0;      // HDD_DEBUG_FLAGS: error injection of the tests; ablation bits (HDD_ABLATION builds only)
  uint32_t variant = 0;     // hdd_ctx_set_variant (ablation build: also HDD_VARIANT): verification variants (0: default)
  int wgcu = 0;             // ablation build, HDD_P1_WGCU: tiles-per-CU sweep override (0: the policy's measured value)
  int q3g_reps = 0;         // ablation build, HDD_Q3G_REPS: workgroups per (XCD, row quad) of the p=3 GEMM kernel
  double* q3g_tab = nullptr;   // p=3 reference matrices [Q3G_K][4096], uploaded on first use
  DeviceScratch scan_ws;       // device-pattern / block-operator scan scratch (kept: no allocation per build)
  DeviceScratch ops_d;         // batched block operators: device descriptor table,
  DeviceScratch ops_h{true};   //   its pinned host staging copy (reused once the last upload has completed)
  hipEvent_t ops_evt = nullptr;
  int64_t* nnz_h = nullptr;    // mapped pinned host word: the device pattern's nnz, written by the elem_ptr kernel
  int64_t* nnz_hd = nullptr;   //   (its device address)
  DeviceScratch rhs_ws;        // 2d RHS boundary-element list (counters zero between calls)
  hipStream_t rhs_stream = nullptr;   // stream of the last split RHS call, and an event behind its face kernel:
  hipEvent_t rhs_evt = nullptr;       //   a call on another stream waits for it (the list is shared state)
  bool rhs_used = false;
  double* apply2_ws = nullptr;   // hdd_operator_apply2's partial sums, allocated with the context (the call allocates nothing)
  // hdd_operator_solve[_batched]: pinned host bytes the device state is read back into -- one 64-byte state per
  // column (HDD_MAX_VEC of them) and 64 bytes of group stop words behind them
  static constexpr size_t SOLVE_STATE_BYTES = (HDD_MAX_VEC + 1) * 64;
  // hdd_operator_solve_blocks reads one state per segment back into the same buffer at the end of a call
  static constexpr size_t SOLVE_BLOCKS_BYTES = size_t(HDD_MAX_SOLVE_BLOCKS) * 64;
  double* solve_state_h = nullptr;   // SOLVE_BLOCKS_BYTES (the larger)
  // hdd_operator_apply_blocks / _solve_blocks: the segment table (64 bytes per segment) is built in pinned host
  // memory; the apply, which has no workspace, keeps its device copy here.  The event is recorded behind the upload:
  // the next call waits for it before it overwrites the host table.
  void* blocks_tab_h = nullptr;
  void* blocks_tab_d = nullptr;
  hipEvent_t blocks_evt = nullptr;

  // the scratch buffers release themselves; what is left are the plain members
  ~hdd_ctx()
  {
    if (q3g_tab) (void)hipFree(q3g_tab);
    if (apply2_ws) (void)hipFree(apply2_ws);
    if (solve_state_h) (void)hipHostFree(solve_state_h);
    if (blocks_tab_h) (void)hipHostFree(blocks_tab_h);
    if (blocks_tab_d) (void)hipFree(blocks_tab_d);
    if (blocks_evt) (void)hipEventDestroy(blocks_evt);
    if (nnz_h) (void)hipHostFree(nnz_h);
    if (rhs_evt) (void)hipEventDestroy(rhs_evt);
    if (ops_evt) (void)hipEventDestroy(ops_evt);
  }
};

// vertex-indexed geometry is read with 32-bit byte offsets (swipdg_elements.hh rsrc32): every [rows][n_local] int32 /
// f64 row offset and every vertex row (at most 3 n_local vertices of 16 B) must stay below 2^32
inline bool vx_offsets_fit(int64_t n_local) { return n_local >= 0 && n_local * 48 < (int64_t(1) << 32); }

inline int hip_fail(hipError_t e, const char* where)
{
  return hdd::set_error(HDD_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

#pragma GCC visibility pop
