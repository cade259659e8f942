// dune-hdd_amd/csrc/kernels/abi_vectors.hip -- C ABI: vector kernels around the assembly: the theta-lincomb of affine
// components (AffinelyDecomposedContainer::freeze_parameter, base.hh:338-341), the SoA halo gather / scatter used
// around the RCCL face-halo exchange of a sharded BlockSWIPDG, and the value gather of block-operator extraction.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ctx.hh"

using hdd::set_error;

// ------------------------------------------------------------------------------------------------
// theta-lincomb: out[s][k] = sum_q theta[s][q] v_q[k]; up to LC_T / n_comp samples per launch (128 for the
// affine + 1 component case: the components are read once for all of them), 2 values per lane written as one
// 16-byte non-temporal store per sample.  All samples in one launch: 12.5-12.7 ms for 128 C3 samples against
// 15.2 ms in launches of 32 (scripts/microbench/lincomb_mb.hip, profiles/r02/s3/lincomb_mb.log).
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int LC_T = 256;   // theta values per launch (samples x components): 2 KB of kernel arguments
typedef double lc_dvec2 __attribute__((ext_vector_type(2)));
struct LincombArgs {
  const double* v[HDD_MAX_COMP];
  double theta[LC_T];         // [n_s][n_comp]
  double* out;
  int64_t nnz, stride;
  int32_t n_comp, n_s;
};

__global__ void __launch_bounds__(256) lincomb_kernel(const LincombArgs a)
{
  __shared__ double th[LC_T];
  for (int i = threadIdx.x; i < a.n_s * a.n_comp; i += 256) th[i] = a.theta[i];
  __syncthreads();
  const int64_t n2 = a.nnz >> 1;
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < n2; k += int64_t(gridDim.x) * blockDim.x) {
    double2 v[HDD_MAX_COMP];
#pragma unroll
    for (int c = 0; c < HDD_MAX_COMP; ++c)
      v[c] = c < a.n_comp ? reinterpret_cast<const double2*>(a.v[c])[k] : make_double2(0.0, 0.0);
    for (int s = 0; s < a.n_s; ++s) {
      lc_dvec2 r = {0.0, 0.0};
      const double* ts = th + s * a.n_comp;
#pragma unroll
      for (int c = 0; c < HDD_MAX_COMP; ++c) {
        if (c < a.n_comp) {
          r.x += ts[c] * v[c].x;
          r.y += ts[c] * v[c].y;
        }
      }
      __builtin_nontemporal_store(r, reinterpret_cast<lc_dvec2*>(a.out + s * a.stride) + k);
    }
  }
  if ((a.nnz & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t k = a.nnz - 1;
    for (int s = 0; s < a.n_s; ++s) {
      double r = 0.0;
      for (int c = 0; c < a.n_comp; ++c) r += th[s * a.n_comp + c] * a.v[c][k];
      a.out[s * a.stride + k] = r;
    }
  }
}
}  // namespace

extern "C" int hdd_affine_lincomb(hdd_ctx* ctx, int64_t nnz, const double* const* d_vals, int32_t n_comp,
                                  const double* theta, int32_t n_samples, double* d_out, int64_t out_stride,
                                  void* stream)
{
  if (!ctx || !d_vals || !theta || !d_out) return set_error(HDD_ERR_INVALID, "hdd_affine_lincomb: null argument");
  if (n_comp < 1 || n_comp > HDD_MAX_COMP || n_samples < 0 || nnz < 0 || out_stride < nnz)
    return set_error(HDD_ERR_INVALID, "hdd_affine_lincomb: invalid sizes");
  bool aligned = true;
  for (int c = 0; c < n_comp; ++c) aligned &= d_vals[c] && (reinterpret_cast<uintptr_t>(d_vals[c]) % 16 == 0);
  aligned &= reinterpret_cast<uintptr_t>(d_out) % 16 == 0 && (out_stride % 2 == 0);
  if (!aligned) return set_error(HDD_ERR_INVALID, "hdd_affine_lincomb: arrays must be 16-byte aligned, stride even");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_affine_lincomb: hipSetDevice");
  const int64_t n2 = (nnz + 1) / 2;
  const unsigned grid = unsigned(std::min<int64_t>(std::max<int64_t>((n2 + 255) / 256, 1), 256 * 32));
  const int per_launch = LC_T / n_comp;
  for (int s0 = 0; s0 < n_samples; s0 += per_launch) {
    LincombArgs a{};
    for (int c = 0; c < n_comp; ++c) a.v[c] = d_vals[c];
    a.n_comp = n_comp;
    a.n_s = std::min(per_launch, n_samples - s0);
    for (int s = 0; s < a.n_s; ++s)
      for (int c = 0; c < n_comp; ++c) a.theta[s * n_comp + c] = theta[(s0 + s) * n_comp + c];
    a.out = d_out + int64_t(s0) * out_stride;
    a.nnz = nnz;
    a.stride = out_stride;
    hipLaunchKernelGGL(lincomb_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hdd_affine_lincomb: launch");
  }
  return HDD_OK;
}

// ------------------------------------------------------------------------------------------------
// SoA gather / scatter of element columns (halo records)
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int SOA_MAX = 16;
struct SoaArgs {
  const double* src[SOA_MAX];
  double* dst[SOA_MAX];
  int32_t rows[SOA_MAX];
  int32_t row_first[SOA_MAX + 1];
  int32_t n_arrays;
  int64_t ld, n, offset;
  const int32_t* idx;
  const double* buf_in;
  double* buf_out;
};

__global__ void __launch_bounds__(256) soa_gather_kernel(const SoaArgs a)
{
  const int64_t total = int64_t(a.row_first[a.n_arrays]) * a.n;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = t / a.n, i = t - r * a.n;
    int arr = 0;
    while (arr + 1 < a.n_arrays && a.row_first[arr + 1] <= r) ++arr;
    const int64_t rr = r - a.row_first[arr];
    a.buf_out[t] = a.src[arr][rr * a.ld + a.idx[i]];
  }
}

__global__ void __launch_bounds__(256) soa_scatter_kernel(const SoaArgs a)
{
  const int64_t total = int64_t(a.row_first[a.n_arrays]) * a.n;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = t / a.n, i = t - r * a.n;
    int arr = 0;
    while (arr + 1 < a.n_arrays && a.row_first[arr + 1] <= r) ++arr;
    const int64_t rr = r - a.row_first[arr];
    a.dst[arr][rr * a.ld + a.offset + i] = a.buf_in[t];
  }
}

int soa_args(SoaArgs& a, const int32_t* rows, int32_t n_arrays, int64_t ld, int64_t n)
{
  if (n_arrays < 1 || n_arrays > SOA_MAX || !rows || ld < 0 || n < 0)
    return set_error(HDD_ERR_INVALID, "hdd_soa_*: invalid sizes (1 <= n_arrays <= 16)");
  a.n_arrays = n_arrays;
  a.row_first[0] = 0;
  for (int k = 0; k < n_arrays; ++k) {
    if (rows[k] < 1) return set_error(HDD_ERR_INVALID, "hdd_soa_*: rows must be >= 1");
    a.rows[k] = rows[k];
    a.row_first[k + 1] = a.row_first[k] + rows[k];
  }
  a.ld = ld;
  a.n = n;
  return HDD_OK;
}
}  // namespace

extern "C" int hdd_soa_gather(hdd_ctx* ctx, const double* const* arrays, const int32_t* rows, int32_t n_arrays,
                              int64_t ld, const int32_t* d_idx, int64_t n, double* d_buf, void* stream)
{
  if (!ctx || !arrays || !d_idx || !d_buf) return set_error(HDD_ERR_INVALID, "hdd_soa_gather: null argument");
  SoaArgs a{};
  int rc = soa_args(a, rows, n_arrays, ld, n);
  if (rc) return rc;
  for (int k = 0; k < n_arrays; ++k) a.src[k] = arrays[k];
  a.idx = d_idx;
  a.buf_out = d_buf;
  if (n == 0) return HDD_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_soa_gather: hipSetDevice");
  const int64_t total = int64_t(a.row_first[n_arrays]) * n;
  const unsigned grid = unsigned(std::min<int64_t>((total + 255) / 256, 4096));
  hipLaunchKernelGGL(soa_gather_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  e = hipGetLastError();
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_soa_gather: launch");
}

extern "C" int hdd_soa_scatter(hdd_ctx* ctx, double* const* arrays, const int32_t* rows, int32_t n_arrays, int64_t ld,
                               int64_t dst_offset, int64_t n, const double* d_buf, void* stream)
{
  if (!ctx || !arrays || !d_buf) return set_error(HDD_ERR_INVALID, "hdd_soa_scatter: null argument");
  SoaArgs a{};
  int rc = soa_args(a, rows, n_arrays, ld, n);
  if (rc) return rc;
  for (int k = 0; k < n_arrays; ++k) a.dst[k] = arrays[k];
  a.offset = dst_offset;
  a.buf_in = d_buf;
  if (n == 0) return HDD_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_soa_scatter: hipSetDevice");
  const int64_t total = int64_t(a.row_first[n_arrays]) * n;
  const unsigned grid = unsigned(std::min<int64_t>((total + 255) / 256, 4096));
  hipLaunchKernelGGL(soa_scatter_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  e = hipGetLastError();
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_soa_scatter: launch");
}

// ------------------------------------------------------------------------------------------------
// value gather (block operator extraction)
// ------------------------------------------------------------------------------------------------
namespace {
__global__ void __launch_bounds__(256) gather_values_kernel(const double* v, const int64_t* src, int64_t n, double* out)
{
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < n; k += int64_t(gridDim.x) * blockDim.x)
    __builtin_nontemporal_store(v[src[k]], out + k);
}
}  // namespace

extern "C" int hdd_gather_values(hdd_ctx* ctx, const double* d_vals, const int64_t* d_src, int64_t n, double* d_out,
                                 void* stream)
{
  if (!ctx || !d_vals || !d_src || !d_out || n < 0) return set_error(HDD_ERR_INVALID, "hdd_gather_values: invalid argument");
  if (n == 0) return HDD_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_gather_values: hipSetDevice");
  const unsigned grid = unsigned(std::min<int64_t>((n + 255) / 256, 256 * 16));
  hipLaunchKernelGGL(gather_values_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), d_vals, d_src, n,
                     d_out);
  e = hipGetLastError();
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_gather_values: launch");
}
