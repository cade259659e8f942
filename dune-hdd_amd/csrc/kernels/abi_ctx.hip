// dune-hdd_amd/csrc/kernels/abi_ctx.hip -- C ABI: the context (ctx.hh) and its settings
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "ctx.hh"

using hdd::set_error;

int hdd::ctx_device(const hdd_ctx* ctx) { return ctx ? ctx->device : 0; }

extern "C" int hdd_ctx_create(int hip_device, hdd_ctx** out)
{
  if (!out) return set_error(HDD_ERR_INVALID, "hdd_ctx_create: null out");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return hip_fail(e, "hdd_ctx_create: hipGetDeviceCount");
  if (hip_device < 0 || hip_device >= n) return set_error(HDD_ERR_RANGE, "hdd_ctx_create: no such HIP device");
  e = hipSetDevice(hip_device);
  if (e != hipSuccess) return hip_fail(e, "hdd_ctx_create: hipSetDevice");
  auto* c = new hdd_ctx;
  c->device = hip_device;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, hip_device) == hipSuccess && cus > 0)
    c->n_cu = cus;
  if (const char* df = getenv("HDD_DEBUG_FLAGS")) c->debug_flags = atoi(df);
#ifdef HDD_ABLATION
  // study knobs: only the ablation build reads them from the environment, so an inherited variable cannot change
  // which kernel a release build times; the tests select variants with hdd_ctx_set_variant
  if (const char* v = getenv("HDD_VARIANT")) c->variant = uint32_t(strtoul(v, nullptr, 0));
  if (const char* w = getenv("HDD_P1_WGCU")) c->wgcu = std::max(0, atoi(w));
  if (const char* r = getenv("HDD_Q3G_REPS")) c->q3g_reps = std::max(0, atoi(r));
#endif
  // hdd_operator_apply2 reduces through this buffer and may not allocate: 512 blocks x 64 (i, j) pairs
  e = hipMalloc(reinterpret_cast<void**>(&c->apply2_ws), size_t(512) * HDD_MAX_VEC * HDD_MAX_VEC * sizeof(double));
  if (e != hipSuccess) {
    c->apply2_ws = nullptr;
    delete c;
    return hip_fail(e, "hdd_ctx_create: hipMalloc");
  }
  // hdd_operator_solve / _solve_batched read their states back at every look and may not allocate either
  static_assert(hdd_ctx::SOLVE_BLOCKS_BYTES >= hdd_ctx::SOLVE_STATE_BYTES, "one buffer for both");
  e = hipHostMalloc(reinterpret_cast<void**>(&c->solve_state_h), hdd_ctx::SOLVE_BLOCKS_BYTES, hipHostMallocDefault);
  if (e != hipSuccess) {
    c->solve_state_h = nullptr;
    delete c;
    return hip_fail(e, "hdd_ctx_create: hipHostMalloc");
  }
  // the segment table of hdd_operator_apply_blocks / _solve_blocks
  e = hipHostMalloc(&c->blocks_tab_h, hdd_ctx::SOLVE_BLOCKS_BYTES, hipHostMallocDefault);
  if (e != hipSuccess) c->blocks_tab_h = nullptr;
  if (e == hipSuccess && (e = hipMalloc(&c->blocks_tab_d, hdd_ctx::SOLVE_BLOCKS_BYTES)) != hipSuccess) c->blocks_tab_d = nullptr;
  if (e == hipSuccess && (e = hipEventCreateWithFlags(&c->blocks_evt, hipEventDisableTiming)) != hipSuccess) c->blocks_evt = nullptr;
  if (e != hipSuccess) {
    delete c;
    return hip_fail(e, "hdd_ctx_create: the segment table");
  }
  *out = c;
  return HDD_OK;
}

extern "C" int hdd_ctx_set_debug_flags(hdd_ctx* ctx, int32_t flags)
{
  if (!ctx) return set_error(HDD_ERR_INVALID, "hdd_ctx_set_debug_flags: null context");
  ctx->debug_flags = flags;
  return HDD_OK;
}

extern "C" int hdd_ctx_set_variant(hdd_ctx* ctx, uint32_t variant)
{
  if (!ctx) return set_error(HDD_ERR_INVALID, "hdd_ctx_set_variant: null context");
  ctx->variant = variant;
  return HDD_OK;
}

extern "C" void hdd_ctx_destroy(hdd_ctx* ctx) { delete ctx; }
