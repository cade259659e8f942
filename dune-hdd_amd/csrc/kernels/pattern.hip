// dune-hdd_amd/csrc/kernels/pattern.hip -- the CSR pattern built on the device, for every element type (SURVEY.md
// 8(f)-2; EllipticSWIPDG::pattern, swipdg.hh:169): the kernels, their launchers and the C ABI entry points
// hdd_pattern_elem_ptr_device / hdd_pattern_fill_device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "abi_common.hh"

namespace hdd {
namespace dev {

// ---------------------------------------------------------------------------------------------------
// kernels: counts -> scan (host side) -> fill
// ---------------------------------------------------------------------------------------------------
__global__ void pattern_counts_kernel(const int32_t* __restrict__ nbrs, int32_t nf, int64_t n_local,
                                      int64_t own_begin, int64_t n_own, int64_t nb2, int64_t* __restrict__ counts)
{
  const int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (k >= n_own) return;
  const int64_t e = own_begin + k;
  int blocks = 1;
  for (int f = 0; f < nf; ++f) blocks += nbrs[f * n_local + e] >= 0;
  counts[k] = nb2 * blocks;
}

// one wavefront per element row block: writes nb rows of nb*nblk sorted global columns
__global__ void pattern_fill_kernel(const int32_t* __restrict__ nbrs, int32_t nf, int32_t nb, int64_t n_local,
                                    int64_t own_begin, int64_t n_own, const int64_t* __restrict__ gid,
                                    const int64_t* __restrict__ elem_ptr, int64_t* __restrict__ row_ptr,
                                    int32_t* __restrict__ col)
{
  const int64_t k = blockIdx.x * int64_t(blockDim.x / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= n_own) return;
  const int64_t e = own_begin + k;
  int64_t blk[7];
  int nblk = 0;
  blk[nblk++] = gid ? gid[e] : e;
  for (int f = 0; f < nf; ++f) {
    const int32_t n = nbrs[f * n_local + e];
    if (n >= 0) blk[nblk++] = gid ? gid[n] : n;
  }
  for (int i = 1; i < nblk; ++i)   // insertion sort of <= 7 keys
    for (int j = i; j > 0 && blk[j - 1] > blk[j]; --j) {
      const int64_t t = blk[j]; blk[j] = blk[j - 1]; blk[j - 1] = t;
    }
  const int64_t base = elem_ptr[k];
  const int rl = nb * nblk;   // <= 7 * 64 columns per row
  for (int i = lane; i < nb; i += 64) row_ptr[k * nb + i] = base + int64_t(i) * rl;
  if (k == n_own - 1 && lane == 0) row_ptr[n_own * nb] = base + int64_t(nb) * rl;
  if (nb == 64) {   // Q3: one block row = one wave store, block ids uniform (no division, no indexed array)
    for (int i = 0; i < 64; ++i) {
      int32_t* crow = col + base + int64_t(i) * rl;
#pragma unroll
      for (int b = 0; b < 7; ++b)
        if (b < nblk) crow[b * 64 + lane] = int32_t(blk[b] * 64 + lane);
    }
    return;
  }
  for (int m = lane; m < nb * rl; m += 64) {
    const int c = m % rl;
    col[base + m] = int32_t(blk[c / nb] * nb + (c % nb));
  }
}

// P1 / Q1 (nb = nf = 3 or 4): one wave per 64-element tile, lane = element.  The lane sorts its <= nf + 1
// column blocks in registers, stages its row block of column ids in an LDS image of the tile (offsets from
// ballots, the elem_ptr rule) and the wave streams the tile's contiguous column range out with 16-byte
// stores: no 64-bit divisions, no per-entry block search (the wave-per-element kernel above keeps hexahedra).
__device__ __forceinline__ int lanes_below(uint64_t m)
{
  return int(__builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u)));
}

template <int NB, int NF>
struct PatTile {
  int32_t nb[NF];   // local neighbour ids (< 0: boundary)
  int64_t own;      // global id of the element
};

// Software-pipelined like swipdg_persistent_kernel (gfx950's vmcnt is in order and counts stores): per
// wave a sequence of tiles, memory order [own data of tile t+1][sort + LDS image of t][neighbour global ids
// of t+1][stores of t].  The tile's row_ptr entries are staged in LDS and written with coalesced 8-byte
// stores (a lane's three or four consecutive entries would be 24 / 32 bytes apart); the column range goes
// out as aligned 16-byte non-temporal buffer stores (head / tail ints separately, so no store straddles
// the range); uniform tiles (64 elements with NF interior faces: 16-byte aligned row blocks) are staged with
// 16-byte LDS writes.
template <int NB, int NF>
__global__ void __launch_bounds__(64) pattern_fill_tile_kernel(const int32_t* __restrict__ nbrs, int64_t n_local,
                                                               int64_t own_begin, int64_t n_own,
                                                               const int64_t* __restrict__ gid,
                                                               const int64_t* __restrict__ elem_ptr,
                                                               int64_t* __restrict__ row_ptr, int32_t* __restrict__ col,
                                                               int64_t n_tiles)
{
  constexpr int RB = (NF + 1) * NB * NB;
  constexpr int CH = (64 * RB + 3) / 4;           // 16-byte chunks of a full tile image
  constexpr int CPL = (CH + 63) / 64;             // chunk stores per lane
  __shared__ __attribute__((aligned(16))) int32_t img[64 * RB + 8 + RB];
  __shared__ int64_t rps[64 * NB];
  typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x;
  int64_t t = blockIdx.x;
  if (t >= n_tiles) return;
  const int64_t step = gridDim.x;
  auto load_own = [&](int64_t tt, PatTile<NB, NF>& p) {
    const int64_t k = tt * 64 + lane;
    const int64_t e = own_begin + (k < n_own ? k : tt * 64);
#pragma unroll
    for (int f = 0; f < NF; ++f) p.nb[f] = nbrs[f * n_local + e];
    p.own = gid ? gid[e] : e;
  };
  auto load_keys = [&](const PatTile<NB, NF>& p, int64_t* nk) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int32_t n = p.nb[f];
      nk[f] = n >= 0 ? (gid ? gid[n] : int64_t(n)) : INT64_MAX;
    }
  };
  PatTile<NB, NF> cur;
  int64_t nk[NF];
  load_own(t, cur);
  load_keys(cur, nk);
  for (;;) {
    const bool has_next = t + step < n_tiles;
    const int64_t tn = has_next ? t + step : t;
    PatTile<NB, NF> nxt;
    load_own(tn, nxt);

    const int64_t k0 = t * 64, k = k0 + lane;
    const bool active = k < n_own;
    const int64_t kend = k0 + 64 < n_own ? k0 + 64 : n_own;
    const int nact = int(kend - k0);
    const int64_t base = __builtin_amdgcn_readfirstlane(elem_ptr[k0]);
    const int64_t tend = __builtin_amdgcn_readfirstlane(elem_ptr[kend]);
    int64_t key[NF + 1];
    key[0] = cur.own;
    int nblk = 1;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      key[f + 1] = nk[f];
      nblk += cur.nb[f] >= 0;
    }
#pragma unroll
    for (int i = 0; i < NF; ++i)   // sorting network (bubble, compile-time)
#pragma unroll
      for (int j = 0; j < NF - i; ++j) {
        const int64_t lo = key[j] < key[j + 1] ? key[j] : key[j + 1];
        const int64_t hi = key[j] < key[j + 1] ? key[j + 1] : key[j];
        key[j] = lo;
        key[j + 1] = hi;
      }
    const int64_t al = base & ~int64_t(3);
    const int c = nblk - 1;
    int sum = lanes_below(__ballot(active));
    sum += lanes_below(__ballot(active && (c & 1)));
    sum += 2 * lanes_below(__ballot(active && (c & 2)));
    sum += 4 * lanes_below(__ballot(active && (c & 4)));
    const int off = NB * NB * sum;
    const int rl = NB * nblk;
    if (active) {
#pragma unroll
      for (int i = 0; i < NB; ++i) rps[lane * NB + i] = base + off + i * rl;
    }
    const bool uni = nact == 64 && tend - base == int64_t(64) * RB && base == al;   // wave-uniform
    if (uni) {   // row block of lane = 16-byte aligned at lane * RB: NB rows x (NF + 1) blocks x NB ints
      i32x4* my = reinterpret_cast<i32x4*>(img + lane * RB);
#pragma unroll
      for (int q = 0; q < RB / 4; ++q) {
        i32x4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int m = 4 * q + u, j = m % NB, b = (m / NB) % (NF + 1);
          v[u] = int32_t(key[b] * NB + j);
        }
        my[q] = v;
      }
    } else {
      int32_t* my = active ? img + (base - al) + off : img + 64 * RB + 8;
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int b = 0; b <= NF; ++b)
          if (b < nblk)
#pragma unroll
            for (int j = 0; j < NB; ++j) my[i * rl + b * NB + j] = int32_t(key[b] * NB + j);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    int64_t nk_n[NF];
    load_keys(nxt, nk_n);

    // row_ptr of the tile's rows: contiguous, coalesced
#pragma unroll
    for (int m = 0; m < NB; ++m) {
      const int idx = lane + 64 * m;
      if (idx < nact * NB) row_ptr[k0 * NB + idx] = rps[idx];
    }
    if (k == n_own - 1) row_ptr[n_own * NB] = tend;
    // columns: head ints [base, a0), aligned middle [a0, a1) in 16-byte chunks, tail [a1, tend)
    const int64_t a0 = (base + 3) & ~int64_t(3), a1 = tend & ~int64_t(3);
    if (a0 >= a1) {   // short range (tiny tiles): plain ints
      for (int64_t g = base + lane; g < tend; g += 64) col[g] = img[g - al];
    } else {
      if (lane < a0 - base) col[base + lane] = img[base - al + lane];
      if (lane < tend - a1) col[a1 + lane] = img[a1 - al + lane];
      const int nbytes = int(a1 - a0) * 4;
      __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(col + a0, (short)0, nbytes, 0x00020000);
      const int32_t* src = img + (a0 - al);
#pragma unroll
      for (int u = 0; u < CPL; ++u) {
        const int m = lane + 64 * u;
        const int li = 4 * m < 64 * RB + 4 ? 4 * m : 0;
        const i32x4 v = *reinterpret_cast<const i32x4*>(src + li);
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, m * 16, 0, 2);   // out-of-range chunks dropped
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!has_next) break;
    t = tn;
    cur = nxt;
#pragma unroll
    for (int f = 0; f < NF; ++f) nk[f] = nk_n[f];
  }
}

// elem_ptr in three small launches instead of counts + a general-purpose device scan (which took 40 us of the
// C2 pattern's 200): per-block sums of 2048 elements' counts, one workgroup scanning the block sums, then each
// block re-counts its elements and writes their prefix (the neighbour ids are read twice: 2 x 4 B per face)
constexpr int PE_THREADS = 256, PE_PER = 8, PE_BLOCK = PE_THREADS * PE_PER;   // 8: 2,000 blocks at C2

__device__ __forceinline__ int64_t pe_count(const int32_t* __restrict__ nbrs, int32_t nf, int64_t n_local, int64_t e,
                                            int64_t nb2)
{
  int blocks = 1;
  for (int f = 0; f < nf; ++f) blocks += nbrs[f * n_local + e] >= 0;
  return nb2 * blocks;
}

// block-wide exclusive scan of one value per thread (PE_THREADS threads); returns the block total too
__device__ __forceinline__ int64_t pe_block_scan(int64_t v, int64_t* sh, int64_t& total)
{
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int64_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t u = __shfl_up(incl, off, 64);
    if (lane >= off) incl += u;
  }
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  int64_t before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < PE_THREADS / 64; ++k) {
    before += k < w ? sh[k] : 0;
    total += sh[k];
  }
  __syncthreads();
  return before + incl - v;
}

__global__ void __launch_bounds__(PE_THREADS) pattern_block_sums_kernel(const int32_t* __restrict__ nbrs, int32_t nf,
                                                                        int64_t n_local, int64_t own_begin,
                                                                        int64_t n_own, int64_t nb2,
                                                                        int64_t* __restrict__ sums)
{
  __shared__ int64_t sh[PE_THREADS / 64];
  const int64_t b0 = int64_t(blockIdx.x) * PE_BLOCK + threadIdx.x;   // coalesced: element b0 + i * PE_THREADS
  int64_t v = 0;
#pragma unroll
  for (int i = 0; i < PE_PER; ++i)
    if (b0 + i * PE_THREADS < n_own) v += pe_count(nbrs, nf, n_local, own_begin + b0 + i * PE_THREADS, nb2);
  int64_t total;
  (void)pe_block_scan(v, sh, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: exclusive offsets of the block sums, in place (chunks of PE_THREADS x PE_PER with a carry)
__global__ void __launch_bounds__(PE_THREADS) pattern_sums_scan_kernel(int64_t* __restrict__ sums, int64_t n)
{
  __shared__ int64_t sh[PE_THREADS / 64];
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < n; c0 += PE_BLOCK) {
    const int64_t i0 = c0 + int64_t(threadIdx.x) * PE_PER;
    int64_t v[PE_PER], s = 0;
#pragma unroll
    for (int i = 0; i < PE_PER; ++i) {
      v[i] = i0 + i < n ? sums[i0 + i] : 0;
      s += v[i];
    }
    int64_t total;
    int64_t ex = carry + pe_block_scan(s, sh, total);
#pragma unroll
    for (int i = 0; i < PE_PER; ++i)
      if (i0 + i < n) {
        sums[i0 + i] = ex;
        ex += v[i];
      }
    carry += total;
  }
}

// BASE_SUM: the block's offset is the sum of the preceding blocks' totals, read by every block (L2-resident:
// 2,000 totals at C2, <= 8 loads per thread) -- no scan launch between the two passes; else offs[] holds the
// scanned offsets.  host_nnz (optional, a mapped pinned host word): the total, written by the last element's
// thread, so the caller reads nnz after a stream synchronisation without a copy launch.
template <bool BASE_SUM>
__global__ void __launch_bounds__(PE_THREADS) pattern_elem_ptr_kernel(const int32_t* __restrict__ nbrs, int32_t nf,
                                                                      int64_t n_local, int64_t own_begin,
                                                                      int64_t n_own, int64_t nb2,
                                                                      const int64_t* __restrict__ offs,
                                                                      int64_t* __restrict__ elem_ptr,
                                                                      int64_t* __restrict__ host_nnz)
{
  __shared__ int64_t sh[PE_THREADS / 64];
  __shared__ int64_t cnt[PE_BLOCK];
  int64_t base = 0;
  if constexpr (BASE_SUM) {
    int64_t part[4] = {0, 0, 0, 0};
    const int nb = int(blockIdx.x);
    int i = int(threadIdx.x);
    for (; i + 3 * PE_THREADS < nb; i += 4 * PE_THREADS) {
#pragma unroll
      for (int u = 0; u < 4; ++u) part[u] += offs[i + u * PE_THREADS];
    }
    for (; i < nb; i += PE_THREADS) part[0] += offs[i];
    int64_t tot;
    (void)pe_block_scan((part[0] + part[1]) + (part[2] + part[3]), sh, tot);
    base = tot;
  } else {
    base = offs[blockIdx.x];
  }
  // counts read coalesced (element b0 + i * PE_THREADS), transposed through LDS so that each thread scans
  // PE_PER consecutive elements, prefixes written back coalesced
  const int64_t blk0 = int64_t(blockIdx.x) * PE_BLOCK;
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < PE_PER; ++i) {
    const int64_t k = blk0 + t + i * PE_THREADS;
    cnt[t + i * PE_THREADS] = k < n_own ? pe_count(nbrs, nf, n_local, own_begin + k, nb2) : 0;
  }
  __syncthreads();
  int64_t c[PE_PER], s = 0;
#pragma unroll
  for (int i = 0; i < PE_PER; ++i) {
    c[i] = cnt[t * PE_PER + i];
    s += c[i];
  }
  int64_t total;
  int64_t p = base + pe_block_scan(s, sh, total);   // (its barriers order the cnt reads above)
#pragma unroll
  for (int i = 0; i < PE_PER; ++i) {
    p += c[i];
    cnt[t * PE_PER + i] = p;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PE_PER; ++i) {
    const int64_t k = blk0 + t + i * PE_THREADS;
    if (k < n_own) elem_ptr[k + 1] = cnt[t + i * PE_THREADS];
    if (host_nnz && k == n_own - 1) *host_nnz = cnt[t + i * PE_THREADS];
  }
  if (blockIdx.x == 0 && t == 0) elem_ptr[0] = 0;
}

int64_t pattern_elem_ptr_scratch(int64_t n_own) { return (n_own + PE_BLOCK - 1) / PE_BLOCK; }

hipError_t launch_pattern_elem_ptr(const int32_t* nbrs, int32_t nf, int64_t n_local, int64_t own_begin,
                                   int64_t own_end, int64_t nb2, int64_t* d_elem_ptr, int64_t* d_scratch, hipStream_t s,
                                   int64_t* host_nnz, bool scan_launch)
{
  const int64_t n_own = own_end - own_begin;
  if (n_own <= 0) return hipMemsetAsync(d_elem_ptr, 0, sizeof(int64_t), s);
  const int64_t nblk = pattern_elem_ptr_scratch(n_own);
  hipLaunchKernelGGL(pattern_block_sums_kernel, dim3(unsigned(nblk)), dim3(PE_THREADS), 0, s, nbrs, nf, n_local,
                     own_begin, n_own, nb2, d_scratch);
  // the offsets summed per block up to 32 K blocks (67 M elements: <= 128 L2 loads per thread), else scanned
  if (scan_launch || nblk > 32768) {
    hipLaunchKernelGGL(pattern_sums_scan_kernel, dim3(1), dim3(PE_THREADS), 0, s, d_scratch, nblk);
    hipLaunchKernelGGL(pattern_elem_ptr_kernel<false>, dim3(unsigned(nblk)), dim3(PE_THREADS), 0, s, nbrs, nf,
                       n_local, own_begin, n_own, nb2, d_scratch, d_elem_ptr, host_nnz);
  } else {
    hipLaunchKernelGGL(pattern_elem_ptr_kernel<true>, dim3(unsigned(nblk)), dim3(PE_THREADS), 0, s, nbrs, nf,
                       n_local, own_begin, n_own, nb2, d_scratch, d_elem_ptr, host_nnz);
  }
  return hipGetLastError();
}

hipError_t launch_pattern_counts(const int32_t* nbrs, int32_t nf, int64_t n_local, int64_t own_begin, int64_t own_end,
                                 int64_t nb2, int64_t* d_counts, hipStream_t s)
{
  const int64_t n_own = own_end - own_begin;
  if (n_own <= 0) return hipSuccess;
  hipLaunchKernelGGL(pattern_counts_kernel, dim3(unsigned((n_own + 255) / 256)), dim3(256), 0, s, nbrs, nf, n_local,
                     own_begin, n_own, nb2, d_counts);
  return hipGetLastError();
}

hipError_t launch_pattern_fill(const int32_t* nbrs, int32_t nf, int32_t nb, int64_t n_local, int64_t own_begin,
                               int64_t own_end, const int64_t* gid, const int64_t* elem_ptr, int64_t* row_ptr,
                               int32_t* col, int cus, hipStream_t s)
{
  const int64_t n_own = own_end - own_begin;
  if (n_own <= 0) return hipSuccess;
  if ((nb == 3 && nf == 3) || (nb == 4 && nf == 4)) {
    const int64_t tiles = (n_own + 63) / 64;
    const unsigned grid = unsigned(std::min<int64_t>(tiles, int64_t(cus) * 8));
    if (nb == 3)
      hipLaunchKernelGGL((pattern_fill_tile_kernel<3, 3>), dim3(grid), dim3(64), 0, s, nbrs, n_local, own_begin, n_own,
                         gid, elem_ptr, row_ptr, col, tiles);
    else
      hipLaunchKernelGGL((pattern_fill_tile_kernel<4, 4>), dim3(grid), dim3(64), 0, s, nbrs, n_local, own_begin, n_own,
                         gid, elem_ptr, row_ptr, col, tiles);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(pattern_fill_kernel, dim3(unsigned((n_own + 3) / 4)), dim3(256), 0, s, nbrs, nf, nb, n_local,
                     own_begin, n_own, gid, elem_ptr, row_ptr, col);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hdd

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
using hdd::set_error;
using namespace hdd::abi;

extern "C" int hdd_pattern_elem_ptr_device(hdd_ctx* ctx, const hdd_mesh* m, int32_t nb, int64_t* d_elem_ptr,
                                           int64_t* nnz, void* stream)
{
  static const char* who = "hdd_pattern_elem_ptr_device";
  if (!ctx || !m || !d_elem_ptr || !nnz || nb < 1 || !m->neighbors) return fail(HDD_ERR_INVALID, who, "invalid argument");
  if (int rc = check_elem_type(who, m)) return rc;
  if (int rc = check_own_range(who, m)) return rc;
  const int nf = mesh_faces(m->elem_type);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_pattern_elem_ptr_device: hipSetDevice");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n_own = m->own_end - m->own_begin;
  const size_t tmp_bytes = size_t(hdd::dev::pattern_elem_ptr_scratch(n_own) + 1) * sizeof(int64_t);
  // the context keeps the scratch (one stream at a time per context)
  e = ctx->scan_ws.reserve(tmp_bytes, DeviceScratch::EXACT, DeviceScratch::SYNC_STREAM, s);
  if (e != hipSuccess) return hip_fail(e, "hdd_pattern_elem_ptr_device: scan scratch");
  // nnz reaches the host through a mapped pinned word the elem_ptr kernel writes (no copy launch);
  // HDD_VARIANT_PATTERN_SCAN_COPY: the round-3 scheme (scan launch + device-to-host copy), cross-check
  const bool legacy = (ctx->variant & HDD_VARIANT_PATTERN_SCAN_COPY) != 0;
  if (!legacy && !ctx->nnz_h && n_own > 0) {
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&ctx->nnz_h), sizeof(int64_t), hipHostMallocMapped)) != hipSuccess)
      return hip_fail(e, "hdd_pattern_elem_ptr_device: pinned nnz");
    if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->nnz_hd), ctx->nnz_h, 0)) != hipSuccess) {
      (void)hipHostFree(ctx->nnz_h);
      ctx->nnz_h = nullptr;
      return hip_fail(e, "hdd_pattern_elem_ptr_device: pinned nnz device address");
    }
  }
  const bool mapped = !legacy && n_own > 0;
  e = hdd::dev::launch_pattern_elem_ptr(m->neighbors, nf, m->n_local, m->own_begin, m->own_end, int64_t(nb) * nb,
                                        d_elem_ptr, static_cast<int64_t*>(ctx->scan_ws.p), s,
                                        mapped ? ctx->nnz_hd : nullptr, legacy);
  if (e != hipSuccess) return hip_fail(e, "hdd_pattern_elem_ptr_device: elem_ptr");
  if (!mapped) e = hipMemcpyAsync(nnz, d_elem_ptr + n_own, sizeof(int64_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "hdd_pattern_elem_ptr_device: read nnz");
  if (mapped) *nnz = *static_cast<volatile int64_t*>(ctx->nnz_h);
  return HDD_OK;
}

extern "C" int hdd_pattern_fill_device(hdd_ctx* ctx, const hdd_mesh* m, int32_t nb, const int64_t* d_global_id,
                                       const int64_t* d_elem_ptr, int64_t* d_row_ptr, int32_t* d_col, void* stream)
{
  static const char* who = "hdd_pattern_fill_device";
  if (!ctx || !m || !d_elem_ptr || !d_row_ptr || !d_col || nb < 1 || !m->neighbors)
    return fail(HDD_ERR_INVALID, who, "invalid argument");
  if (int rc = check_elem_type(who, m)) return rc;
  if (int rc = check_own_range(who, m)) return rc;
  const int nf = mesh_faces(m->elem_type);
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_pattern_fill_device: hipSetDevice");
  e = hdd::dev::launch_pattern_fill(m->neighbors, nf, nb, m->n_local, m->own_begin, m->own_end, d_global_id,
                                    d_elem_ptr, d_row_ptr, d_col, ctx->n_cu, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_pattern_fill_device: launch");
}
