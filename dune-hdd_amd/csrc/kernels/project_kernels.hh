// dune-hdd_amd/csrc/kernels/project_kernels.hh -- reduced-basis projection G_q = V^T A_q U of every affine component
// in one pass over the value arrays, and V^T W (hdd_operator_project / hdd_vectors_inner, abi_project.hip).
//
// W = A_q U never goes to memory: a wave forms it for a panel of PROJECT_PANEL = 16 u-vectors on a few rows, re-lays it
// through the LDS into the B operand of v_mfma_f64_16x16x4_f64 and contracts it at once with the same rows of V (the A
// operand, read from memory: in MFMA step s lane l holds V[16 mb + (l & 15)][row (l >> 4) STEPS + s]).  A 16 x 16
// block of G is 8 VGPRs per lane and needs no cross-lane reduction; a wave keeps the HDD_MAX_BASIS / 16 = 4 row blocks
// of its panel (32 VGPRs) over all its rows.  The launch is gridDim.x parts x (n_comp * panels): workgroup (b, q, panel) walks part b's
// rows of component q for u-vectors [16 panel, 16 panel + 16) and leaves its [n_v][16] share at
// partial[b][q][.][16 panel ..]; project_final_kernel adds the parts in order.  So the value arrays are read once per
// panel of 16 u-vectors, V once per panel and component, and the gathers of U come from the cache after the first
// touch of a tile.
//
// project_tile_kernel -- the staging of apply_tile_body (apply_kernels.hh): a wave per 64-element tile, the tile's
//   contiguous value range of ONE component streamed into the swizzled LDS image, the columns derived from
//   mesh->neighbors (a block whose element lies outside the column range is skipped, so the gathers of U need no
//   further range check; sixteen sized buffer resources cost 370 spilled SGPRs).  Lane = element forms IB rows of W
//   per pass (P1: all 3, Q1: 2 of 4 in two passes -- the W buffer of a whole Q1 tile would not fit the 64 KB beside
//   the image), writes them to wb[n][64 IB + 1] (the odd stride keeps the lanes of a write and of a read on different banks), and the
//   wave contracts the 64 IB rows in 16 IB MFMA steps per row block.  LDS per wave: P1 19,456 + 24,704 = 44,160 B,
//   Q1 40,960 + 16,512 = 57,472 B: inside the 64 KB a launch gets without raising the kernel's dynamic-LDS attribute.
// project_csr_kernel -- the structure of apply_csr_body: G = 8 lanes per row, 8 rows at once and 32 per wave pass
//   (eight MFMA steps per row block), or a wave per row, 16 rows per pass (four steps); four waves per workgroup,
//   added in order at the end.  Every n_comp <= HDD_MAX_COMP (the component is a launch index).
// inner_kernel -- V^T W over n entries: both operands straight from memory, 64 rows per wave pass.
//
// Bit-independence: every W entry is one fma chain over its row in the pattern's order, every G entry one MFMA chain
// over the rows in an order that depends on the plan, the row count and gridDim.x alone (gridDim.x in turn on the
// plan and the row count, project_parts).  MFMA positions do not talk to each other, vectors beyond n_v / n_u are
// zeros that are never loaded, so entry (q, i, j) is a function of A_q, v_i, u_j and the range: not of n_v, n_u, the
// other vectors or the position of v_i / u_j in the call.  No atomics.
#pragma once
#include <cstdint>

#include "apply_kernels.hh"

namespace hdd {
namespace dev {

constexpr int PROJECT_PANEL = 16;                     // u-vectors per panel: the N of the MFMA
constexpr int PROJECT_MB = HDD_MAX_BASIS / 16;        // row blocks of G a wave keeps
constexpr int PROJECT_BLOCKS = 512;                   // parts (partial sums per entry) at the most
static_assert(HDD_MAX_BASIS % 16 == 0, "whole MFMA blocks");

typedef double pdbl4 __attribute__((ext_vector_type(4)));

struct ProjectArgs {
  ApplyArgs a;            // the plan; x / ldx: U.  theta, nv, y, partial are not read
  const double* v;        // v[i * ldv + row - row_begin]
  int64_t ldv;
  int32_t n_v, n_u;
  double* partial;        // [gridDim.x][n_comp][n_v][n_u]
};

// G[mb] += V[16 mb + (lane & 15)][off_of(pos)] * wb[(lane & 15) * S + pos] over the 4 STEPS positions of the buffer:
// MFMA step s takes pos = (lane >> 4) STEPS + s, so a lane reads STEPS positions in a row -- of V straight from memory
// (v: the buffer's first row of vector 0), all of a row block's loads in flight before its first MFMA.
// off_of(pos) < 0: no such row (its W entries are zeros); V is not read there, nor for vectors >= n_v.
template <int STEPS, class OffOf>
__device__ __forceinline__ void project_contract(pdbl4 (&G)[PROJECT_MB], const double* wb, int S, const double* v, int64_t ldv, int n_v,
                                                 OffOf&& off_of)
{
  const int lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  double b[STEPS];
  int off[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    b[s] = wb[m * S + kq * STEPS + s];
    off[s] = off_of(kq * STEPS + s);
  }
#pragma unroll
  for (int mb = 0; mb < PROJECT_MB; ++mb) {
    if (mb * 16 >= n_v) break;   // (uniform)
    const bool has = mb * 16 + m < n_v;
    const double* vm = v + int64_t(has ? mb * 16 + m : 0) * ldv;
    double av[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) av[s] = (has && off[s] >= 0) ? vm[off[s]] : 0.0;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) G[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], b[s], G[mb], 0, 0, 0);
  }
}

// entry [r] of lane l's G[mb] is G[16 mb + (l >> 4) + 4 r][l & 15]
__device__ __forceinline__ void project_store(double* out, int n_v, int n_u, int j0, int mb, int r, int lane, double g)
{
  const int i = 16 * mb + (lane >> 4) + 4 * r, j = j0 + (lane & 15);
  if (i < n_v && j < n_u) out[i * n_u + j] = g;
}

template <int NB, int NF>
struct ProjectTile {
  using I = ApplyImage<NB, NF>;
  static constexpr int IB = NB % 3 == 0 ? 3 : 2;      // rows of W per element and pass
  static constexpr int NH = NB / IB;                  // passes
  static constexpr int S = 64 * IB + 1;               // doubles between two u-vectors of the W buffer (odd: banks)
  static constexpr int BYTES = I::BYTES + PROJECT_PANEL * S * 8;
  static_assert(NB % IB == 0 && BYTES <= 64 * 1024, "the dynamic LDS a launch gets without raising the kernel's attribute");
};

template <int NB, int NF>
__global__ void __launch_bounds__(64) project_tile_kernel(const ProjectArgs p, int64_t n_tiles, int n_panels)
{
  using T = ProjectTile<NB, NF>;
  using I = ApplyImage<NB, NF>;
  constexpr int CH = I::CHUNKS, U = I::U, IMG = I::BYTES / 8, IB = T::IB, S = T::S, NV = PROJECT_PANEL;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* wb = lds + IMG;
  const ApplyArgs& a = p.a;
  const int lane = threadIdx.x;
  const int q = int(blockIdx.y) / n_panels, j0 = (int(blockIdx.y) % n_panels) * PROJECT_PANEL;
  const double* vals = a.vals[q];
  pdbl4 G[PROJECT_MB];
#pragma unroll
  for (int mb = 0; mb < PROJECT_MB; ++mb) G[mb] = pdbl4{0.0, 0.0, 0.0, 0.0};
  const TileRange r = tile_range(blockIdx.x, gridDim.x, n_tiles);
  const double* const u0 = a.x + int64_t(j0) * a.ldx;   // the panel's first u-vector
  for (int64_t t = r.t; t < r.t_end; t += r.t_step) {
    const int64_t t0 = a.e_begin + t * 64;
    const int64_t tend = t0 + 64 < a.e_end ? t0 + 64 : a.e_end;
    const bool active = t0 + lane < tend;
    const int64_t e = active ? t0 + lane : t0;
    int nbr[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) nbr[f] = a.nbrs[f * a.n_local + e];
    const int64_t base = apply_uni64(a.elem_ptr[t0 - a.own_begin]);
    const int64_t tile_end = apply_uni64(a.elem_ptr[tend - a.own_begin]);
    const int64_t base_al = base & ~int64_t(1);
    const int tlen_al = int(tile_end - base_al);
    // the previous tile's image and W buffer have been read by every lane
    lds_wave_sync();
    // [stream component q's values of the tile -> LDS image]; chunks beyond the tile read zero (range check)
    {
      const uint32_t vbytes = tile_end > base_al ? uint32_t(tlen_al) * 8u : 0u;
      const __amdgpu_buffer_rsrc_t vr = apply_rsrc(vals + base_al, vbytes);
#pragma unroll 1
      for (int k0 = 0; k0 < CH; k0 += U) {
        if (k0 * 128 >= tlen_al) break;
        dvec2 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = ld128f(vr, uint32_t(lane + 64 * (k0 + u)) * 16u);
#pragma unroll
        for (int u = 0; u < U; ++u) *reinterpret_cast<dvec2*>(lds + apply_swz(2 * (lane + 64 * (k0 + u)))) = v[u];
      }
      // an odd image length: the last value has no whole 16-byte chunk inside the tile's range
      if ((tlen_al & 1) && lane == 0) lds[apply_swz(tlen_al - 1)] = ld64f(vr, uint32_t(tlen_al - 1) * 8u);
    }
    lds_wave_sync();
    // [lane = element: row block from the image, block columns from the neighbours, U gathered per block]
    int nint = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) nint += nbr[f] >= 0;
    const int off = tile_offset<NB>(nint, active) + int(base - base_al);
    int id[NF + 1];
    id[0] = int(e);
#pragma unroll
    for (int f = 0; f < NF; ++f) id[f + 1] = nbr[f] >= 0 ? nbr[f] : 0x7fffffff;
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < NF - i; ++j) {
        const int lo = id[j] < id[j + 1] ? id[j] : id[j + 1], hi = id[j] < id[j + 1] ? id[j + 1] : id[j];
        id[j] = lo;
        id[j + 1] = hi;
      }
    const int rl = NB * (nint + 1);   // row length
#pragma unroll 1
    for (int h = 0; h < T::NH; ++h) {
      double acc[NV][IB];
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int i = 0; i < IB; ++i) acc[v][i] = 0.0;
      if (active) {
#pragma unroll
        for (int b = 0; b <= NF; ++b) {
          if (b > nint || id[b] < a.ce_begin || id[b] >= a.ce_end) continue;   // skipped, not multiplied by zero
          // the block's element lies inside the column range (just checked): plain loads stay inside U's rows
          const double* xb = u0 + (id[b] - a.ce_begin) * NB;
          double xv[NV][NB];
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int j = 0; j < NB; ++j) xv[v][j] = j0 + v < p.n_u ? xb[v * a.ldx + j] : 0.0;
#pragma unroll
          for (int i = 0; i < IB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
              const double m = lds[apply_swz(off + (h * IB + i) * rl + b * NB + j)];
#pragma unroll
              for (int v = 0; v < NV; ++v) acc[v][i] = __builtin_fma(m, xv[v][j], acc[v][i]);
            }
        }
      }
      // the previous pass's W has been read; lanes without an element leave zeros
      lds_wave_sync();
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int i = 0; i < IB; ++i) wb[v * S + lane * IB + i] = acc[v][i];
      lds_wave_sync();
      // position pos of the buffer is row h IB + pos % IB of element t0 + pos / IB
      const int n_el = int(tend - t0);
      project_contract<16 * IB>(G, wb, S, p.v + (t0 - a.e_begin) * NB, p.ldv, p.n_v,
                                [&](int pos) { return pos / IB < n_el ? (pos / IB) * NB + h * IB + pos % IB : -1; });
    }
  }
  double* out = p.partial + (int64_t(blockIdx.x) * a.n_comp + q) * p.n_v * p.n_u;
#pragma unroll
  for (int mb = 0; mb < PROJECT_MB; ++mb)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) project_store(out, p.n_v, p.n_u, j0, mb, rr, lane, G[mb][rr]);
}

// the four waves' blocks in order -> partial[blockIdx.x][q] (red: [4][PROJECT_MB * 4 * 64])
__device__ __forceinline__ void project_block_store(const pdbl4 (&G)[PROJECT_MB], double (*red)[PROJECT_MB * 256], double* out, int n_v, int n_u,
                                                    int j0)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int mb = 0; mb < PROJECT_MB; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(mb * 4 + r) * 64 + lane] = G[mb][r];
  __syncthreads();
  for (int idx = threadIdx.x; idx < PROJECT_MB * 256; idx += 256)
    project_store(out, n_v, n_u, j0, idx / 256, (idx / 64) % 4, idx % 64, ((red[0][idx] + red[1][idx]) + red[2][idx]) + red[3][idx]);
}

// rows of a wave pass of project_csr_kernel<G>
constexpr int project_csr_rows(int G) { return G == 8 ? 32 : 16; }

template <int G>
__global__ void __launch_bounds__(256) project_csr_kernel(const ProjectArgs p, int n_panels)
{
  static_assert(G == 8 || G == 64, "a group of 8 lanes or a wave per row");
  constexpr int RW = project_csr_rows(G), PER = 64 / G, S = RW + 1, NV = PROJECT_PANEL;   // PER: rows at once
  __shared__ double wbuf[4][NV * S];
  __shared__ double red[4][PROJECT_MB * 256];
  const ApplyArgs& a = p.a;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane % G;
  const int q = int(blockIdx.y) / n_panels, j0 = (int(blockIdx.y) % n_panels) * PROJECT_PANEL;
  const double* vals = a.vals[q];
  double* wb = wbuf[wave];
  pdbl4 Gm[PROJECT_MB];
#pragma unroll
  for (int mb = 0; mb < PROJECT_MB; ++mb) Gm[mb] = pdbl4{0.0, 0.0, 0.0, 0.0};
  const int64_t n_rows = a.row_end - a.row_begin;
  const int64_t chunks = (n_rows + RW - 1) / RW;
  for (int64_t ch = int64_t(blockIdx.x) * 4 + wave; ch < chunks; ch += int64_t(gridDim.x) * 4) {   // (wave-uniform)
    const int64_t rb = ch * RW;
    lds_wave_sync();   // the previous pass's W has been read
#pragma unroll 1
    for (int rs = 0; rs < RW / PER; ++rs) {   // PER rows at once, a group of G lanes each
      const int pos = rs * PER + lane / G;
      const int64_t rr = rb + pos;
      double acc[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] = 0.0;
      if (rr < n_rows) {
        int64_t k0 = a.row_ptr[a.row_begin + rr], k1 = a.row_ptr[a.row_begin + rr + 1];
        k0 = k0 < 0 ? 0 : k0;
        k1 = k1 > a.nnz ? a.nnz : k1;
        for (int64_t k = k0 + gl; k < k1; k += G) {
          const int64_t c = a.col[k];
          if (c < a.col_begin || c >= a.col_end) continue;   // skipped, not multiplied by zero
          const double m = vals[k];
          const double* xc = a.x + (c - a.col_begin);
#pragma unroll
          for (int v = 0; v < NV; ++v)
            if (j0 + v < p.n_u) acc[v] = __builtin_fma(m, xc[int64_t(j0 + v) * a.ldx], acc[v]);
        }
      }
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int s = G / 2; s > 0; s >>= 1) acc[v] += __shfl_xor(acc[v], s, G);
      if (gl == 0)
#pragma unroll
        for (int v = 0; v < NV; ++v) wb[v * S + pos] = acc[v];
    }
    lds_wave_sync();
    const int n_here = int(n_rows - rb < RW ? n_rows - rb : RW);
    project_contract<RW / 4>(Gm, wb, S, p.v + rb, p.ldv, p.n_v, [&](int pos) { return pos < n_here ? pos : -1; });
  }
  project_block_store(Gm, red, p.partial + (int64_t(blockIdx.x) * a.n_comp + q) * p.n_v * p.n_u, p.n_v, p.n_u, j0);
}

// partial[blockIdx.x][i][j] = this workgroup's share of v_i . w_j; wave pass: 64 entries (16 in a row per lane and
// vector), 16 MFMA steps per row block
[[maybe_unused]] static __global__ void __launch_bounds__(256) inner_kernel(const double* v, int64_t ldv, int n_v, const double* w, int64_t ldw,
                                                                            int n_w, int64_t n, double* partial)
{
  constexpr int STEPS = 16;
  __shared__ double red[4][PROJECT_MB * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
  const int j0 = int(blockIdx.y) * PROJECT_PANEL;
  pdbl4 G[PROJECT_MB];
#pragma unroll
  for (int mb = 0; mb < PROJECT_MB; ++mb) G[mb] = pdbl4{0.0, 0.0, 0.0, 0.0};
  const bool has_w = j0 + m < n_w;
  const double* wm = w + int64_t(has_w ? j0 + m : 0) * ldw;
  for (int64_t base = (int64_t(blockIdx.x) * 4 + wave) * 64; base < n; base += int64_t(gridDim.x) * 256) {
    const int64_t r0 = base + kq * STEPS;
    double b[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) b[s] = (has_w && r0 + s < n) ? wm[r0 + s] : 0.0;
#pragma unroll
    for (int mb = 0; mb < PROJECT_MB; ++mb) {
      if (mb * 16 >= n_v) break;   // (uniform)
      const bool has = mb * 16 + m < n_v;
      const double* vm = v + int64_t(has ? mb * 16 + m : 0) * ldv;
      double av[STEPS];
#pragma unroll
      for (int s = 0; s < STEPS; ++s) av[s] = (has && r0 + s < n) ? vm[r0 + s] : 0.0;
#pragma unroll
      for (int s = 0; s < STEPS; ++s) G[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], b[s], G[mb], 0, 0, 0);
    }
  }
  project_block_store(G, red, partial + int64_t(blockIdx.x) * n_v * n_w, n_v, n_w, j0);
}

// out[idx] = the parts' partial sums in part order; idx < n_out = n_comp * n_v * n_u
[[maybe_unused]] static __global__ void __launch_bounds__(256) project_final_kernel(const double* partial, int n_parts, int64_t n_out, double* out)
{
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= n_out) return;
  double s = 0.0;
  for (int b = 0; b < n_parts; ++b) s += partial[int64_t(b) * n_out + idx];
  out[idx] = s;
}

}  // namespace dev
}  // namespace hdd
