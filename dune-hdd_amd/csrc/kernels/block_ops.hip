// dune-hdd_amd/csrc/kernels/block_ops.hip -- C ABI: sub-blocks of an assembled CSR matrix, one at a time
// (hdd_block_operator_*_device, subcsr_* kernels) or batched (hdd_block_operators_*_device, ops_* kernels)
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <string>

#include "ctx.hh"

using hdd::set_error;

// ------------------------------------------------------------------------------------------------
// block operators on the device (BlockSWIPDG::get_local_operator / get_coupling_operator,
// block-swipdg.hh:625-676, 1328-1379): rows [r0, r1) of a sorted CSR pattern restricted to the columns
// [c0, c1).  In the subdomain-major numbering the columns of one subdomain are ONE contiguous sub-range of
// every sorted row, found by two binary searches: count -> scan -> fill, thread per row (rows hold <= 5 (2d)
// or 7 (3d) blocks).  The values need no index map: a second pass copies each row's sub-range.
// ------------------------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ int64_t lower_bound_col(const int32_t* col, int64_t lo, int64_t hi, int64_t v)
{
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    if (int64_t(col[m]) < v) lo = m + 1;
    else hi = m;
  }
  return lo;
}

__global__ void __launch_bounds__(256) subcsr_count_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                           int64_t r0, int64_t n, int64_t c0, int64_t c1,
                                                           int64_t* __restrict__ out_rp)
{
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t a = rp[r0 + i], b = rp[r0 + i + 1];
    const int64_t lo = lower_bound_col(col, a, b, c0);
    out_rp[i + 1] = lower_bound_col(col, lo, b, c1) - lo;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out_rp[0] = 0;
}

__global__ void __launch_bounds__(256) subcsr_fill_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                          int64_t r0, int64_t n, int64_t c0,
                                                          const int64_t* __restrict__ out_rp, int32_t* __restrict__ out_col,
                                                          int64_t* __restrict__ out_src)
{
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t lo = lower_bound_col(col, rp[r0 + i], rp[r0 + i + 1], c0);
    const int64_t k0 = out_rp[i], len = out_rp[i + 1] - k0;
    for (int64_t j = 0; j < len; ++j) {
      out_col[k0 + j] = int32_t(int64_t(col[lo + j]) - c0);
      if (out_src) out_src[k0 + j] = lo + j;
    }
  }
}

struct ValPtrs {
  const double* in[HDD_MAX_COMP];
  double* out[HDD_MAX_COMP];
};

__global__ void __launch_bounds__(256) subcsr_values_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                            int64_t r0, int64_t n, int64_t c0,
                                                            const int64_t* __restrict__ out_rp, ValPtrs v, int nc)
{
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t lo = lower_bound_col(col, rp[r0 + i], rp[r0 + i + 1], c0);
    const int64_t k0 = out_rp[i], len = out_rp[i + 1] - k0;
    for (int c = 0; c < nc; ++c)
      for (int64_t j = 0; j < len; ++j) v.out[c][k0 + j] = v.in[c][lo + j];
  }
}

int subcsr_check(const hdd_csr* p, int64_t r0, int64_t r1, int64_t c0, int64_t c1, const char* who)
{
  if (!p || !p->row_ptr || !p->col) return set_error(HDD_ERR_INVALID, std::string(who) + ": pattern arrays missing");
  if (r0 < 0 || r1 < r0 || r1 > p->n_rows || c0 < 0 || c1 < c0)
    return set_error(HDD_ERR_RANGE, std::string(who) + ": 0 <= row_begin <= row_end <= n_rows, col_begin <= col_end violated");
  if (c1 - c0 > int64_t(INT32_MAX)) return set_error(HDD_ERR_RANGE, std::string(who) + ": column range exceeds int32");
  return HDD_OK;
}

unsigned rows_grid(int64_t n, int n_cu) { return unsigned(std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, int64_t(n_cu) * 16))); }

// ---- batched: n_ops sub-blocks of one pattern in four launches.  The concatenated row-pointer array holds
// a leading slot per operator (count 0) before its row counts, so ONE inclusive scan over all operators leaves
// at operator k's leading slot the number of entries of the operators before it (base) and at its slot j the
// global start of its row j.  Operator k's entries start at noff = the prefix of the EVEN-rounded counts
// (16-byte aligned value arrays: hdd_affine_lincomb takes every operator as it is).
struct OpDesc {
  int64_t r0, c0, c1;   // rows [r0, r0 + rows), columns [c0, c1) of the pattern
  int64_t roff, rows;   // slots [roff, roff + rows + 1) of the concatenated row-pointer array
  int64_t base;         // entries of the operators before k (the scan's value at the leading slot)
  int64_t noff;         // where operator k's entries start in the concatenated outputs (even)
};

__device__ __forceinline__ int op_of_slot(const OpDesc* d, int n_ops, int64_t x)
{
  int lo = 0, hi = n_ops - 1;   // last k with roff_k <= x
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (d[m].roff <= x) lo = m;
    else hi = m - 1;
  }
  return lo;
}

// the sub-range [lo, lo + len) of sorted row [a, b) with columns in [c0, c1): most rows of a coupling operator
// lie wholly outside (first / last column decide, two independent loads), only the rest binary-search
__device__ __forceinline__ void row_range(const int32_t* __restrict__ col, int64_t a, int64_t b, int64_t c0,
                                          int64_t c1, int64_t& lo, int64_t& len)
{
  lo = a;
  len = 0;
  if (a == b) return;
  const int64_t first = col[a], last = col[b - 1];
  if (last < c0 || first >= c1) return;
  if (first >= c0 && last < c1) {
    len = b - a;
    return;
  }
  lo = lower_bound_col(col, a, b, c0);
  len = lower_bound_col(col, lo, b, c1) - lo;
}

__global__ void __launch_bounds__(256) ops_count_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                        const OpDesc* __restrict__ d, int n_ops, int64_t n_slots,
                                                        int64_t* __restrict__ out)
{
  for (int64_t x = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; x < n_slots; x += int64_t(gridDim.x) * blockDim.x) {
    const OpDesc o = d[op_of_slot(d, n_ops, x)];
    const int64_t j = x - o.roff;
    int64_t lo = 0, c = 0;
    if (j > 0) row_range(col, rp[o.r0 + j - 1], rp[o.r0 + j], o.c0, o.c1, lo, c);
    out[x] = c;
  }
}

// one wave: bases and even-rounded offsets of 64 operators per step (loads in parallel, a wave prefix sum)
__global__ void __launch_bounds__(64) ops_base_kernel(const int64_t* __restrict__ scanned, OpDesc* d, int n_ops,
                                                      int64_t* __restrict__ totals)
{
  const int lane = threadIdx.x;
  int64_t carry = 0;
  for (int k0 = 0; k0 < n_ops; k0 += 64) {
    const int k = k0 + lane;
    int64_t b = 0, n = 0;
    if (k < n_ops) {
      b = scanned[d[k].roff];
      n = scanned[d[k].roff + d[k].rows] - b;
    }
    int64_t incl = n + (n & 1);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    const int64_t noff = carry + incl - (n + (n & 1));
    if (k < n_ops) {
      d[k].base = b;
      d[k].noff = noff;
      if (totals) totals[k] = noff;
    }
    carry += __shfl(incl, 63, 64);
  }
  if (totals && lane == 0) totals[n_ops] = carry;
}

// Wave-cooperative copy of the 64 row segments a wave holds (lane l: len[l] entries): the segments' entries
// are numbered through a wave prefix sum and every lane takes entries lane, lane + 64, ...; copy(seg, off)
// handles entry off of segment seg.  Consecutive lanes then write consecutive positions of the
// (operator-contiguous) destination and read runs of the source, instead of 64 lanes each walking its own row
// (64 cache lines per instruction).  Whole waves call it (the slot loops below are wave-uniform).
template <class F>
__device__ __forceinline__ void wave_segments(int len, int* s_end, F&& copy)
{
  const int lane = threadIdx.x & 63;
  int incl = len;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  s_end[lane] = incl;
  const int total = __shfl(incl, 63, 64);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int p = lane; p < total; p += 64) {
    int lo = 0, hi = 63;   // the first segment whose inclusive end exceeds p
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (s_end[m] > p) hi = m;
      else lo = m + 1;
    }
    copy(lo, p - (lo ? s_end[lo - 1] : 0));
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct SegShared {
  int64_t src[4][64], dst[4][64], c0[4][64];
  int end[4][64];
};

// columns (local) / sources at the operators' positions, then the row pointer made operator-relative in place
// (each slot reads only itself: its count is recomputed, the base comes from the descriptor)
__global__ void __launch_bounds__(256) ops_fill_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                       const OpDesc* __restrict__ d, int n_ops, int64_t n_slots,
                                                       int64_t* __restrict__ out_rp, int32_t* __restrict__ out_col,
                                                       int64_t* __restrict__ out_src)
{
  __shared__ SegShared sh;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t xb = int64_t(blockIdx.x) * blockDim.x; xb < n_slots; xb += int64_t(gridDim.x) * blockDim.x) {
    const int64_t x = xb + threadIdx.x;
    int64_t lo = 0, len = 0, dst = 0, c0 = 0;
    if (x < n_slots) {
      const OpDesc o = d[op_of_slot(d, n_ops, x)];
      const int64_t j = x - o.roff;
      const int64_t end = out_rp[x] - o.base;   // operator-relative end of row j - 1
      if (j > 0) row_range(col, rp[o.r0 + j - 1], rp[o.r0 + j], o.c0, o.c1, lo, len);
      dst = o.noff + end - len;
      c0 = o.c0;
      out_rp[x] = end;
    }
    if (out_col || out_src) {
      sh.src[w][lane] = lo;
      sh.dst[w][lane] = dst;
      sh.c0[w][lane] = c0;   // a wave's segments may belong to two operators
      wave_segments(int(len), sh.end[w], [&](int seg, int off) {
        const int64_t si = sh.src[w][seg] + off, di = sh.dst[w][seg] + off;
        if (out_col) out_col[di] = int32_t(int64_t(col[si]) - sh.c0[w][seg]);
        if (out_src) out_src[di] = si;
      });
    }
  }
}

// values: operator k's entries at noff_k + its (relative) row pointer, copied wave-cooperatively
__global__ void __launch_bounds__(256) ops_values_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                         const OpDesc* __restrict__ d, int n_ops, int64_t n_slots,
                                                         const int64_t* __restrict__ out_rp, ValPtrs v, int nc)
{
  __shared__ SegShared sh;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t xb = int64_t(blockIdx.x) * blockDim.x; xb < n_slots; xb += int64_t(gridDim.x) * blockDim.x) {
    const int64_t x = xb + threadIdx.x;
    int64_t lo = 0, len = 0, dst = 0;
    if (x < n_slots) {
      const OpDesc o = d[op_of_slot(d, n_ops, x)];
      const int64_t j = x - o.roff;
      if (j > 0) {
        const int64_t r0 = out_rp[x - 1];
        len = out_rp[x] - r0;
        dst = o.noff + r0;
        if (len) lo = lower_bound_col(col, rp[o.r0 + j - 1], rp[o.r0 + j], o.c0);
      }
    }
    sh.src[w][lane] = lo;
    sh.dst[w][lane] = dst;
    wave_segments(int(len), sh.end[w], [&](int seg, int off) {
      const int64_t si = sh.src[w][seg] + off, di = sh.dst[w][seg] + off;
      for (int c = 0; c < nc; ++c) v.out[c][di] = v.in[c][si];
    });
  }
}
}  // namespace

// descriptor table of a batched call -> ctx->ops_d (stream-ordered upload through the pinned staging copy,
// reused only after the previous upload completed); noff from the host array when given
static int ops_upload(hdd_ctx* ctx, const hdd_csr* p, int32_t n_ops, const hdd_block_range* ops,
                      const int64_t* nnz_off, hipStream_t s, int64_t* n_slots, const char* who)
{
  if (n_ops < 1 || !ops) return set_error(HDD_ERR_INVALID, std::string(who) + ": need n_ops >= 1 ranges");
  const size_t bytes = size_t(n_ops) * sizeof(OpDesc);
  hipError_t e = hipSuccess;
  if (!ctx->ops_evt && (e = hipEventCreateWithFlags(&ctx->ops_evt, hipEventDisableTiming)) != hipSuccess)
    return hip_fail(e, who);
  if ((e = hipEventSynchronize(ctx->ops_evt)) != hipSuccess) return hip_fail(e, who);
  // the last upload has completed (ops_evt above), so the staging copy is free to be rewritten or replaced
  if ((e = ctx->ops_d.reserve(bytes, DeviceScratch::EXACT, DeviceScratch::NO_SYNC)) != hipSuccess) return hip_fail(e, who);
  if ((e = ctx->ops_h.reserve(bytes, DeviceScratch::EXACT, DeviceScratch::NO_SYNC)) != hipSuccess) return hip_fail(e, who);
  auto* h = static_cast<OpDesc*>(ctx->ops_h.p);
  int64_t slots = 0;
  for (int32_t k = 0; k < n_ops; ++k) {
    const hdd_block_range& r = ops[k];
    if (int rc = subcsr_check(p, r.row_begin, r.row_end, r.col_begin, r.col_end, who)) return rc;
    if (nnz_off && (nnz_off[k] & 1))
      return set_error(HDD_ERR_INVALID, std::string(who) + ": nnz_off must be even (16-byte aligned operators)");
    h[k] = OpDesc{r.row_begin, r.col_begin, r.col_end, slots, r.row_end - r.row_begin, 0, nnz_off ? nnz_off[k] : 0};
    slots += r.row_end - r.row_begin + 1;
  }
  if (slots >= int64_t(INT32_MAX))
    return set_error(HDD_ERR_RANGE, std::string(who) + ": sum of (rows + 1) over the operators must fit int32");
  if ((e = hipMemcpyAsync(ctx->ops_d.p, ctx->ops_h.p, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e, who);
  if ((e = hipEventRecord(ctx->ops_evt, s)) != hipSuccess) return hip_fail(e, who);
  *n_slots = slots;
  return HDD_OK;
}

extern "C" int hdd_block_operators_map_device(hdd_ctx* ctx, const hdd_csr* pattern, int32_t n_ops,
                                              const hdd_block_range* ops, int64_t* d_out_row_ptr, int32_t* d_out_col,
                                              int64_t* d_out_src, int64_t* nnz_off, void* stream)
{
  static const char* who = "hdd_block_operators_map_device";
  if (!ctx || !d_out_row_ptr) return set_error(HDD_ERR_INVALID, std::string(who) + ": null argument");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t n = 0;
  if (int rc = ops_upload(ctx, pattern, n_ops, ops, nullptr, s, &n, who)) return rc;
  auto* d = static_cast<OpDesc*>(ctx->ops_d.p);
  const unsigned grid = rows_grid(n, ctx->n_cu);
  hipLaunchKernelGGL(ops_count_kernel, dim3(grid), dim3(256), 0, s, pattern->row_ptr, pattern->col, d, int(n_ops), n,
                     d_out_row_ptr);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, who);
  size_t tmp = 0;
  if ((e = hipcub::DeviceScan::InclusiveSum(nullptr, tmp, d_out_row_ptr, d_out_row_ptr, n, s)) != hipSuccess)
    return hip_fail(e, who);
  // scan scratch + (n_ops + 1) totals, kept in the context
  const size_t need = tmp + size_t(n_ops + 1) * sizeof(int64_t) + 256;
  if ((e = ctx->scan_ws.reserve(need, DeviceScratch::EXACT, DeviceScratch::SYNC_STREAM, s)) != hipSuccess)
    return hip_fail(e, who);
  if ((e = hipcub::DeviceScan::InclusiveSum(ctx->scan_ws.p, tmp, d_out_row_ptr, d_out_row_ptr, n, s)) != hipSuccess)
    return hip_fail(e, who);
  auto* totals = reinterpret_cast<int64_t*>(static_cast<char*>(ctx->scan_ws.p) + ((tmp + 255) & ~size_t(255)));
  hipLaunchKernelGGL(ops_base_kernel, dim3(1), dim3(64), 0, s, d_out_row_ptr, d, int(n_ops),
                     nnz_off ? totals : nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, who);
  hipLaunchKernelGGL(ops_fill_kernel, dim3(grid), dim3(256), 0, s, pattern->row_ptr, pattern->col, d, int(n_ops), n,
                     d_out_row_ptr, d_out_col, d_out_src);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, who);
  if (nnz_off) {
    e = hipMemcpyAsync(nnz_off, totals, size_t(n_ops + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, who);
  }
  return HDD_OK;
}

extern "C" int hdd_block_operators_values_device(hdd_ctx* ctx, const hdd_csr* pattern, int32_t n_ops,
                                                 const hdd_block_range* ops, const int64_t* nnz_off,
                                                 const int64_t* d_out_row_ptr, const double* const* d_vals,
                                                 int32_t n_comp, double* const* d_out, void* stream)
{
  static const char* who = "hdd_block_operators_values_device";
  if (!ctx || !nnz_off || !d_out_row_ptr || !d_vals || !d_out || n_comp < 0 || n_comp > HDD_MAX_COMP)
    return set_error(HDD_ERR_INVALID, std::string(who) + ": invalid argument");
  ValPtrs v{};
  for (int c = 0; c < n_comp; ++c) {
    if (!d_vals[c] || !d_out[c]) return set_error(HDD_ERR_INVALID, std::string(who) + ": null value array");
    v.in[c] = d_vals[c];
    v.out[c] = d_out[c];
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t n = 0;
  if (int rc = ops_upload(ctx, pattern, n_ops, ops, nnz_off, s, &n, who)) return rc;
  if (n_comp == 0) return HDD_OK;
  hipLaunchKernelGGL(ops_values_kernel, dim3(rows_grid(n, ctx->n_cu)), dim3(256), 0, s, pattern->row_ptr, pattern->col,
                     static_cast<const OpDesc*>(ctx->ops_d.p), int(n_ops), n, d_out_row_ptr, v, int(n_comp));
  e = hipGetLastError();
  return e == hipSuccess ? HDD_OK : hip_fail(e, who);
}


extern "C" int hdd_block_operator_map_device(hdd_ctx* ctx, const hdd_csr* pattern, int64_t row_begin, int64_t row_end,
                                             int64_t col_begin, int64_t col_end, int64_t* d_out_row_ptr,
                                             int32_t* d_out_col, int64_t* d_out_src, int64_t* nnz, void* stream)
{
  if (!ctx || !d_out_row_ptr) return set_error(HDD_ERR_INVALID, "hdd_block_operator_map_device: null argument");
  if (int rc = subcsr_check(pattern, row_begin, row_end, col_begin, col_end, "hdd_block_operator_map_device")) return rc;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_block_operator_map_device: hipSetDevice");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = row_end - row_begin;
  const unsigned grid = rows_grid(n, ctx->n_cu);
  hipLaunchKernelGGL(subcsr_count_kernel, dim3(grid), dim3(256), 0, s, pattern->row_ptr, pattern->col, row_begin, n,
                     col_begin, col_end, d_out_row_ptr);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "hdd_block_operator_map_device: count");
  if (n > 0) {
    size_t tmp = 0;
    e = hipcub::DeviceScan::InclusiveSum(nullptr, tmp, d_out_row_ptr + 1, d_out_row_ptr + 1, n, s);
    if (e != hipSuccess) return hip_fail(e, "hdd_block_operator_map_device: scan size");
    // grows once per context (one stream at a time per context)
    e = ctx->scan_ws.reserve(tmp, DeviceScratch::EXACT, DeviceScratch::SYNC_STREAM, s);
    if (e != hipSuccess) return hip_fail(e, "hdd_block_operator_map_device: scratch");
    e = hipcub::DeviceScan::InclusiveSum(ctx->scan_ws.p, tmp, d_out_row_ptr + 1, d_out_row_ptr + 1, n, s);
    if (e != hipSuccess) return hip_fail(e, "hdd_block_operator_map_device: scan");
  }
  if (d_out_col) {
    hipLaunchKernelGGL(subcsr_fill_kernel, dim3(grid), dim3(256), 0, s, pattern->row_ptr, pattern->col, row_begin, n,
                       col_begin, d_out_row_ptr, d_out_col, d_out_src);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "hdd_block_operator_map_device: fill");
  }
  if (nnz) {
    e = hipMemcpyAsync(nnz, d_out_row_ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "hdd_block_operator_map_device: read nnz");
  }
  return HDD_OK;
}

extern "C" int hdd_block_operator_values_device(hdd_ctx* ctx, const hdd_csr* pattern, int64_t row_begin, int64_t row_end,
                                                int64_t col_begin, int64_t col_end, const int64_t* d_out_row_ptr,
                                                const double* const* d_vals, int32_t n_comp, double* const* d_out,
                                                void* stream)
{
  if (!ctx || !d_out_row_ptr || !d_vals || !d_out || n_comp < 0 || n_comp > HDD_MAX_COMP)
    return set_error(HDD_ERR_INVALID, "hdd_block_operator_values_device: invalid argument");
  if (int rc = subcsr_check(pattern, row_begin, row_end, col_begin, col_end, "hdd_block_operator_values_device")) return rc;
  ValPtrs v{};
  for (int c = 0; c < n_comp; ++c) {
    if (!d_vals[c] || !d_out[c]) return set_error(HDD_ERR_INVALID, "hdd_block_operator_values_device: null value array");
    v.in[c] = d_vals[c];
    v.out[c] = d_out[c];
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_block_operator_values_device: hipSetDevice");
  const int64_t n = row_end - row_begin;
  if (n == 0 || n_comp == 0) return HDD_OK;
  hipLaunchKernelGGL(subcsr_values_kernel, dim3(rows_grid(n, ctx->n_cu)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     pattern->row_ptr, pattern->col, row_begin, n, col_begin, d_out_row_ptr, v, int(n_comp));
  e = hipGetLastError();
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_block_operator_values_device: launch");
}
