// dune-hdd_amd/csrc/kernels/apply_kernels.hh -- operator application y = (sum_q theta_q A_q) x on the assembled
// value arrays (hdd_operator_apply / _apply_multi / _apply2, abi_apply.hip; launched by launch_apply, apply_plan.hh).
//
// apply_tile_body -- the assembler run backwards, for 2d P1 / Q1 SWIPDG patterns in local == global numbering.  One
//   wave owns a tile of 64 consecutive elements of the row range (persistent over tiles, the assembler's tile_range
//   XCD sweep).  The tile's row blocks are ONE contiguous CSR value range [elem_ptr[t0], elem_ptr[t0 + 64)): the wave
//   streams it with aligned 16-byte buffer loads (origin base_al = base & ~1, as the assembler's image) into an LDS
//   image (XOR-swizzled against the bank conflicts of row blocks 36 / 80 values apart, apply_swz).  Lane l then takes
//   element t0 + l: its row block starts at the ballot prefix sum of the block counts (tile_offset), its block
//   columns are its own id and its face neighbours' ids sorted ascending -- the ordering hdd_dg_pattern_fill gave the
//   blocks -- so neither col nor row_ptr is read: 8 B per nonzero instead of 12.  Blocks whose element lies outside
//   the column range are skipped (their values are never multiplied).  Every indexed read of x and the value stream
//   go through buffer resources with the true sizes: an index the mesh got wrong reads zero instead of faulting.
//   No pipelining across tiles inside a wave: several waves per CU (8 P1 images, 4 Q1 images fit the LDS) overlap
//   one wave's loads with another's arithmetic, and a wave has up to 20 KB of loads in flight by itself.
//   Two theta modes, which differ in the staging and in the read of a matrix entry only:
//   NC = 0 (apply_tile_kernel): one theta for all vectors, combined on the way into the LDS -- one image whatever
//     n_comp, one LDS read per entry;
//   NC >= 1 (apply_tile_multi_kernel, NC = n_comp): a theta per vector -- image q holds component q's values of the
//     tile in the same layout at lds + q * I::BYTES / 8, and the combination happens at the read: NC LDS reads per
//     entry, then the theta chain per vector.  NC * I::BYTES of LDS per wave: P1 19,456 B per image (NC <= 3:
//     58,368 B, inside the 64 KB a launch gets without raising the kernel's dynamic-LDS attribute), Q1 40,960 B (NC = 1).
// apply_csr_body -- plain CSR on row_ptr / col for everything else; a group of G lanes per row (8 for the short
//   rows of P1 / Q1 / volume patterns, a wave for the hexahedral Q_p rows), shuffle reduction in a fixed order.  One
//   theta (apply_csr_kernel): the matrix entry once per nonzero; a theta per vector (apply_csr_multi_kernel): the
//   n_comp values loaded once, then a chain per vector; every n_comp <= HDD_MAX_COMP.
// A theta per vector (hdd_operator_apply_multi, hdd_operator_solve_multi): y_v = (sum_q theta[v][q] A_q) x_v, the same
//   affine components at several parameters, the value stream read once per group of NV vectors.  Both modes take the
//   matrix entry from apply_entries, the one place where it is written: m = theta[0] a_0, m = fma(theta[q], a_q, m)
//   for q = 1 .. n_comp - 1 in separate statements, then acc = fma(m, x, acc) -- so y_v, and the DOT partial sums on
//   the same grid, are bit for bit those of the single-theta launch on (theta[v], x_v).  Entries of vectors >= nv are
//   copies of vector 0's (never stored).
// apply2_partial_kernel / apply2_final_kernel -- out[i][j] = v_i . w_j in two deterministic stages.
// DOT variants (a square diagonal range: x and y share their numbering) also leave x_v . y_v behind, for the
//   conjugate gradient iteration: every lane adds x_r y_r of its own rows over its tiles / rows in order, the
//   workgroup reduces once at the end (shuffle tree, then the waves in order) and writes
//   partial[v * gridDim.x + blockIdx.x].  Every vector has its own chain and its own tree, those of the NV = 1
//   instantiation: with the same grid, vector v's partial sums are bit for bit those of a one-vector launch on it
//   (the batched solve rests on this).  The instantiations without DOT are unchanged by it (same registers,
//   DESIGN.md 4.6).
// No atomics anywhere: results are bit-identical from call to call.
#pragma once
#include <cstdint>

#include "swipdg_persistent.hh"

namespace hdd {
namespace dev {

constexpr int APPLY_NV = 4;          // vectors per pass of the compile-time multi-vector kernels
constexpr int APPLY2_BLOCKS = 512;   // partial sums per (i, j) pair of apply2 (the context's scratch holds them)
constexpr int APPLY2_PAIRS = HDD_MAX_VEC * HDD_MAX_VEC;

struct ApplyArgs {
  const double* vals[HDD_MAX_COMP];
  double theta[HDD_MAX_COMP];
  int32_t n_comp, nv;                  // nv: vectors of this pass (<= the kernel's NV)
  int64_t nnz;
  const int64_t* row_ptr;              // generic path
  const int32_t* col;
  const int64_t* elem_ptr;             // tile path
  const int32_t* nbrs;
  int64_t n_local, own_begin;
  int64_t e_begin, e_end;              // tile path: local element ids of the row range
  int64_t ce_begin, ce_end;            //            and of the column range
  int64_t row_begin, row_end, col_begin, col_end;
  const double* x;                     // x[v * ldx + col - col_begin]
  int64_t ldx;
  double* y;                           // y[v * ldy + row - row_begin]
  int64_t ldy;
  // DOT variants only (hdd_operator_solve[_batched], solve_kernels.hh): partial[v * gridDim + blockIdx] = this
  // workgroup's share of x_v . y_v, and the iteration's stop word -- the launch returns at once when
  // *done_at <= iteration
  double* partial;
  const int32_t* done_at;
  int32_t iteration;
};

// the arguments of the kernels with a theta per vector
struct ApplyMultiArgs {
  ApplyArgs a;                         // a.theta is not read
  double theta[APPLY_NV][HDD_MAX_COMP];
};

// What one workgroup sees of a launch: its index w() in a grid of nw() workgroups (a Grid), and the ranges and the
// vectors (a View).  A plain launch passes its own blockIdx.x / gridDim.x (LaunchGrid, read where they are used,
// as the kernels always did) and the plan's fields (PlanView); a blocks launch (hdd_operator_apply_blocks /
// _solve_blocks, the end of this file) the virtual index and grid of the workgroup's segment (VirtualGrid) and the
// segment's (SegmentView) ranges, vector offsets, partial sums and stop word.  Every order of summation in the bodies is a function
// of (w, nw) and the ranges alone.
struct LaunchGrid {
  __device__ __forceinline__ uint32_t w() const { return blockIdx.x; }
  __device__ __forceinline__ uint32_t nw() const { return gridDim.x; }
};
struct VirtualGrid {
  uint32_t w_, nw_;
  __device__ __forceinline__ uint32_t w() const { return w_; }
  __device__ __forceinline__ uint32_t nw() const { return nw_; }
};

// the plan's own fields, read where they are used
struct PlanView {
  const ApplyArgs& a;
  __device__ __forceinline__ int64_t e_begin() const { return a.e_begin; }
  __device__ __forceinline__ int64_t e_end() const { return a.e_end; }
  __device__ __forceinline__ int64_t ce_begin() const { return a.ce_begin; }
  __device__ __forceinline__ int64_t ce_end() const { return a.ce_end; }
  __device__ __forceinline__ int64_t row_begin() const { return a.row_begin; }
  __device__ __forceinline__ int64_t row_end() const { return a.row_end; }
  __device__ __forceinline__ int64_t col_begin() const { return a.col_begin; }
  __device__ __forceinline__ int64_t col_end() const { return a.col_end; }
  __device__ __forceinline__ const double* x() const { return a.x; }
  __device__ __forceinline__ double* y() const { return a.y; }
  __device__ __forceinline__ double* partial() const { return a.partial; }
  __device__ __forceinline__ const int32_t* done_at() const { return a.done_at; }
};
__device__ __forceinline__ PlanView apply_view(const ApplyArgs& a) { return PlanView{a}; }

// a segment's
struct SegmentView {
  int64_t e_begin_, e_end_, ce_begin_, ce_end_, row_begin_, row_end_;
  const double* x_;
  double *y_, *partial_;
  const int32_t* done_at_;
  __device__ __forceinline__ int64_t e_begin() const { return e_begin_; }
  __device__ __forceinline__ int64_t e_end() const { return e_end_; }
  __device__ __forceinline__ int64_t ce_begin() const { return ce_begin_; }
  __device__ __forceinline__ int64_t ce_end() const { return ce_end_; }
  __device__ __forceinline__ int64_t row_begin() const { return row_begin_; }
  __device__ __forceinline__ int64_t row_end() const { return row_end_; }
  __device__ __forceinline__ int64_t col_begin() const { return row_begin_; }   // square and diagonal
  __device__ __forceinline__ int64_t col_end() const { return row_end_; }
  __device__ __forceinline__ const double* x() const { return x_; }
  __device__ __forceinline__ double* y() const { return y_; }
  __device__ __forceinline__ double* partial() const { return partial_; }
  __device__ __forceinline__ const int32_t* done_at() const { return done_at_; }
};

// sizes of the tile kernel's LDS image: 16-byte chunks per lane (odd row blocks, P1: the image origin may lie one
// value in front of the tile) and how many of them are loaded back to back
template <int NB, int NF>
struct ApplyImage {
  static constexpr int BB = NB * NB, RB = BB * (NF + 1);
  static constexpr int CHUNKS = (32 * RB + (BB % 2) + 63) / 64;
  static constexpr int U = CHUNKS % 20 == 0 ? 20 : CHUNKS;   // P1: 19 at once; Q1: 40 in two bursts of 20
  static constexpr int BYTES = CHUNKS * 64 * 16;
  static_assert(CHUNKS % U == 0 && U <= 20, "burst length divides the chunk count");
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t apply_rsrc(const double* p, uint32_t nbytes)
{
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(p), (short)0, int(nbytes), 0x00020000);
}

// a wave-uniform 64-bit value (value arrays pass 2^31 entries at the large configurations)
__device__ __forceinline__ int64_t apply_uni64(int64_t v)
{
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(uint64_t(v) >> 32));
  return int64_t((uint64_t(hi) << 32) | lo);
}

// LDS position of image value p.  The lanes read row blocks RB values apart (P1: 36, Q1: 80 -- 8 and 2 distinct
// 8-byte banks per 32 lanes in a plain image): bits 5..8 of the position are XORed onto bits 1..4, which spreads
// the lanes' reads over the 16 bank pairs a 16-byte-aligned pair layout can reach; a 16-byte chunk c moves as a
// whole to c ^ ((c >> 4) & 15), so the staging writes stay aligned and conflict-free.
__device__ __forceinline__ int apply_swz(int p) { return p ^ (((p >> 5) & 15) << 1); }

// One matrix entry at NT thetas: m[t] = sum_q theta[t][q] comp(q), the n components read once.  The statements are
// the contract (the build contracts within an expression only): a product, then one fma per further component.
template <int NT, class Comp>
__device__ __forceinline__ void apply_entries(double (&m)[NT], const double (*theta)[HDD_MAX_COMP], int n, Comp&& comp)
{
  {
    const double w = comp(0);
#pragma unroll
    for (int t = 0; t < NT; ++t) m[t] = theta[t][0] * w;
  }
  for (int q = 1; q < n; ++q) {
    const double w = comp(q);
#pragma unroll
    for (int t = 0; t < NT; ++t) m[t] = __builtin_fma(theta[t][q], w, m[t]);
  }
}

// (sum_q theta_q A_q)[k] of the plan's theta, from the value arrays
__device__ __forceinline__ double apply_entry(const ApplyArgs& a, int64_t k)
{
  double m[1];
  apply_entries<1>(m, &a.theta, a.n_comp, [&](int q) { return a.vals[q][k]; });
  return m[0];
}

// the sum of s over the wave, in every lane (the tree of every DOT variant)
__device__ __forceinline__ double apply_wave_sum(double s)
{
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

// The tile algorithm (header comment).  NC = 0: theta[0] for all vectors; NC >= 1: theta[v] for vector v, NC = n_comp.
template <int NB, int NF, int NV, bool DOT, int NC, class View, class Grid>
__device__ __forceinline__ void apply_tile_body(const ApplyArgs& a, const View& g, const Grid& grid, const double (*theta)[HDD_MAX_COMP], int64_t n_tiles)
{
  using I = ApplyImage<NB, NF>;
  constexpr int CH = I::CHUNKS, U = I::U, IMG = I::BYTES / 8;
  constexpr int NT = NC ? NV : 1;   // thetas
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  [[maybe_unused]] double dot[NV] = {};   // DOT: this lane's x_v . y_v over its elements, in tile order
  if constexpr (DOT)
    if (*g.done_at() <= a.iteration) return;   // (wave-uniform)
  const TileRange r = tile_range(grid.w(), grid.nw(), n_tiles);
  const uint32_t xbytes = uint32_t((g.ce_end() - g.ce_begin()) * NB * 8);
  __amdgpu_buffer_rsrc_t xr[NV];
  [[maybe_unused]] double th[NT][HDD_MAX_COMP];   // NC >= 1: the thetas in registers (entries [.][< NC])
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    xr[v] = apply_rsrc(g.x() + (v < a.nv ? v : 0) * a.ldx, xbytes);
#pragma unroll
    for (int q = 0; q < NC; ++q) th[v][q] = theta[v][q];
  }
  for (int64_t t = r.t; t < r.t_end; t += r.t_step) {
    const int64_t t0 = g.e_begin() + t * 64;
    const int64_t tend = t0 + 64 < g.e_end() ? t0 + 64 : g.e_end();
    const bool active = t0 + lane < tend;
    const int64_t e = active ? t0 + lane : t0;
    int nbr[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) nbr[f] = a.nbrs[f * a.n_local + e];
    const int64_t base = apply_uni64(a.elem_ptr[t0 - a.own_begin]);
    const int64_t tile_end = apply_uni64(a.elem_ptr[tend - a.own_begin]);
    const int64_t base_al = base & ~int64_t(1);
    const int tlen_al = int(tile_end - base_al);   // image length in values, from the aligned origin
    // the previous tile's image has been read by every lane
    lds_wave_sync();
    // [stream the tile's values -> LDS image]; chunks beyond the tile read zero (range check)
    const uint32_t vbytes = tile_end > base_al ? uint32_t(tlen_al) * 8u : 0u;
    if constexpr (NC == 0) {   // the theta combination on the way: one image
#pragma unroll 1
      for (int k0 = 0; k0 < CH; k0 += U) {
        if (k0 * 128 >= tlen_al) break;
        dvec2 v[U];
        {
          const __amdgpu_buffer_rsrc_t vr = apply_rsrc(a.vals[0] + base_al, vbytes);
          const double th0 = theta[0][0];
#pragma unroll
          for (int u = 0; u < U; ++u) v[u] = th0 * ld128f(vr, uint32_t(lane + 64 * (k0 + u)) * 16u);
        }
#pragma unroll 1
        for (int q = 1; q < a.n_comp; ++q) {
          const __amdgpu_buffer_rsrc_t vr = apply_rsrc(a.vals[q] + base_al, vbytes);
          const double thq = theta[0][q];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const dvec2 w = ld128f(vr, uint32_t(lane + 64 * (k0 + u)) * 16u);
            v[u].x = __builtin_fma(thq, w.x, v[u].x);
            v[u].y = __builtin_fma(thq, w.y, v[u].y);
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) *reinterpret_cast<dvec2*>(lds + apply_swz(2 * (lane + 64 * (k0 + u)))) = v[u];
      }
      // an odd image length: the last value has no whole 16-byte chunk inside the tile's range
      if ((tlen_al & 1) && lane == 0) {
        const uint32_t o8 = uint32_t(tlen_al - 1) * 8u;
        double s[1];
        apply_entries<1>(s, theta, a.n_comp, [&](int q) { return ld64f(apply_rsrc(a.vals[q] + base_al, vbytes), o8); });
        lds[apply_swz(tlen_al - 1)] = s[0];
      }
    } else {   // a component at a time -> its image
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const __amdgpu_buffer_rsrc_t vr = apply_rsrc(a.vals[q] + base_al, vbytes);
#pragma unroll 1
        for (int k0 = 0; k0 < CH; k0 += U) {
          if (k0 * 128 >= tlen_al) break;
          dvec2 v[U];
#pragma unroll
          for (int u = 0; u < U; ++u) v[u] = ld128f(vr, uint32_t(lane + 64 * (k0 + u)) * 16u);
#pragma unroll
          for (int u = 0; u < U; ++u) *reinterpret_cast<dvec2*>(lds + q * IMG + apply_swz(2 * (lane + 64 * (k0 + u)))) = v[u];
        }
        if ((tlen_al & 1) && lane == 0) lds[q * IMG + apply_swz(tlen_al - 1)] = ld64f(vr, uint32_t(tlen_al - 1) * 8u);
      }
    }
    lds_wave_sync();
    // [lane = element: row block from the image, block columns from the neighbours, x gathered per block]
    int nint = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) nint += nbr[f] >= 0;
    const int off = tile_offset<NB>(nint, active) + int(base - base_al);
    if (!active) continue;
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
    double acc[NV][NB];
    [[maybe_unused]] double xown[NV][NB] = {};
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[v][i] = 0.0;
#pragma unroll
    for (int b = 0; b <= NF; ++b) {
      if (b > nint || id[b] < g.ce_begin() || id[b] >= g.ce_end()) continue;   // skipped, not multiplied by zero
      const uint32_t xo = uint32_t(id[b] - int(g.ce_begin())) * uint32_t(NB * 8);
      double xv[NV][NB];
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int j = 0; j < NB; ++j) xv[v][j] = v < a.nv ? ld64f(xr[v], xo + 8u * j) : 0.0;
      if constexpr (DOT)   // the element's own block is one of the gathered ones: these are its rows of x
        if (id[b] == int(e))
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int j = 0; j < NB; ++j) xown[v][j] = xv[v][j];
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int p = apply_swz(off + i * rl + b * NB + j);
          // the entry: the combined image's, or per vector from the component images
          [[maybe_unused]] double c[NC ? NC : 1];
          if constexpr (NC == 0) c[0] = lds[p];
#pragma unroll
          for (int q = 0; q < NC; ++q) c[q] = lds[q * IMG + p];
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            double m[1] = {c[0]};
            if constexpr (NC > 0) apply_entries<1>(m, th + v, NC, [&](int q) { return c[q]; });
            acc[v][i] = __builtin_fma(m[0], xv[v][j], acc[v][i]);
          }
        }
    }
    double* yo = g.y() + (e - g.e_begin()) * NB;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (v < a.nv)
#pragma unroll
        for (int i = 0; i < NB; ++i) yo[v * a.ldy + i] = acc[v][i];
    if constexpr (DOT)
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int i = 0; i < NB; ++i) dot[v] = __builtin_fma(xown[v][i], acc[v][i], dot[v]);
  }
  if constexpr (DOT) {   // every lane is back here, whatever its tiles were
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      dot[v] = apply_wave_sum(dot[v]);
      if (lane == 0 && v < a.nv) g.partial()[int64_t(v) * grid.nw() + grid.w()] = dot[v];
    }
  }
}

template <int NB, int NF, int NV, bool DOT = false>
__global__ void __launch_bounds__(64) apply_tile_kernel(const ApplyArgs a, int64_t n_tiles)
{
  apply_tile_body<NB, NF, NV, DOT, 0>(a, apply_view(a), LaunchGrid{}, &a.theta, n_tiles);
}

template <int NB, int NF, int NV, bool DOT, int NC>
__global__ void __launch_bounds__(64) apply_tile_multi_kernel(const ApplyMultiArgs ma, int64_t n_tiles)
{
  static_assert(NV <= APPLY_NV && NC >= 1 && NC <= HDD_MAX_COMP, "theta[APPLY_NV][HDD_MAX_COMP]");
  apply_tile_body<NB, NF, NV, DOT, NC>(ma.a, apply_view(ma.a), LaunchGrid{}, ma.theta, n_tiles);
}

// The CSR algorithm: G lanes per row, 256 / G rows per workgroup pass.  NT = 1: theta[0] for all vectors; NT = NV:
// theta[v] for vector v.
template <int G, int NV, bool DOT, int NT, class View, class Grid>
__device__ __forceinline__ void apply_csr_body(const ApplyArgs& a, const View& g, const Grid& grid, const double (*theta)[HDD_MAX_COMP])
{
  [[maybe_unused]] double dot[NV] = {};   // DOT: the group leaders' x_r y_r over their rows, in row order
  if constexpr (DOT)
    if (*g.done_at() <= a.iteration) return;   // (uniform)
  const int gl = threadIdx.x % G;
  const int64_t n_rows = g.row_end() - g.row_begin();
  const int64_t stride = int64_t(grid.nw()) * (256 / G);
  for (int64_t rr = int64_t(grid.w()) * (256 / G) + threadIdx.x / G; rr < n_rows; rr += stride) {
    int64_t k0 = a.row_ptr[g.row_begin() + rr], k1 = a.row_ptr[g.row_begin() + rr + 1];
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > a.nnz ? a.nnz : k1;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    for (int64_t k = k0 + gl; k < k1; k += G) {
      const int64_t c = a.col[k];
      if (c < g.col_begin() || c >= g.col_end()) continue;   // skipped, not multiplied by zero
      double m[NT];
      apply_entries<NT>(m, theta, a.n_comp, [&](int q) { return a.vals[q][k]; });
      const double* xc = g.x() + (c - g.col_begin());
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (v < a.nv) acc[v] = __builtin_fma(m[NT == 1 ? 0 : v], xc[v * a.ldx], acc[v]);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int s = G / 2; s > 0; s >>= 1) acc[v] += __shfl_xor(acc[v], s, G);
    if (gl == 0)
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (v < a.nv) g.y()[v * a.ldy + rr] = acc[v];
    if constexpr (DOT)
      if (gl == 0)   // square diagonal range: row rr is column rr
#pragma unroll
        for (int v = 0; v < NV; ++v)
          if (v < a.nv) dot[v] = __builtin_fma(g.x()[v * a.ldx + rr], acc[v], dot[v]);
  }
  if constexpr (DOT) {
    __shared__ double red[NV][4];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      dot[v] = apply_wave_sum(dot[v]);
      if ((threadIdx.x & 63) == 0) red[v][threadIdx.x >> 6] = dot[v];
    }
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (v < a.nv) g.partial()[int64_t(v) * grid.nw() + grid.w()] = ((red[v][0] + red[v][1]) + red[v][2]) + red[v][3];
  }
}

template <int G, int NV, bool DOT = false>
__global__ void __launch_bounds__(256) apply_csr_kernel(const ApplyArgs a)
{
  apply_csr_body<G, NV, DOT, 1>(a, apply_view(a), LaunchGrid{}, &a.theta);
}

template <int G, int NV, bool DOT = false>
__global__ void __launch_bounds__(256) apply_csr_multi_kernel(const ApplyMultiArgs ma)
{
  static_assert(NV <= APPLY_NV, "theta[APPLY_NV][HDD_MAX_COMP]");
  apply_csr_body<G, NV, DOT, NV>(ma.a, apply_view(ma.a), LaunchGrid{}, ma.theta);
}

// ---- the block-diagonal part with respect to row segments (hdd_operator_apply_blocks / _solve_blocks) -------------
// One launch serves every segment [row_begin, row_begin + rows) of a partition of a row interval: segment s gets the
// virtual grid grid[kind] it would have in a launch of its own (kind: which launch of the solve, BLOCKS_*), the
// launch has the sum of them as real workgroups, and real workgroup b belongs to the segment s with first[kind] <= b
// < first[kind] + grid[kind], as its virtual workgroup b - first[kind].  The host builds the table (64 bytes per
// segment); a workgroup finds its segment by bisection over first[kind] -- wave-uniform, so scalar loads: twelve
// steps at the most (HDD_MAX_SOLVE_BLOCKS segments), which need no table entry per workgroup and no second copy to
// the device.  (A per-workgroup table was not measured against it.)
enum { BLOCKS_DOT = 0, BLOCKS_PARTS = 1, BLOCKS_DIRECTION = 2, BLOCKS_APPLY = 3, BLOCKS_KINDS = 4 };

struct BlockSegment {
  int64_t row_begin, rows;           // rows = columns of the matrix
  int64_t e_begin, e_end;            // tile path: local element ids of the rows
  int32_t first[BLOCKS_KINDS];       // per kind of launch: the segment's first real workgroup; also the offset of its
  int32_t grid[BLOCKS_KINDS];        //   partial sums of that kind; and its virtual grid
};
static_assert(sizeof(BlockSegment) == 64, "eight doubles of the workspace");

struct BlocksArgs {
  const BlockSegment* seg;
  int32_t n_seg, kind;
  int64_t row0;                      // first row of the interval: segment s of a vector sits at row_begin - row0
  const int32_t* stop;               // DOT: the call's stop word
  const int32_t* done_at;            // DOT: segment s's stop word at done_at[16 s] (its 64-byte SolveState)
};

// the segment of real workgroup b: the last s with first[kind] <= b (the grids are positive: first ascends strictly)
__device__ __forceinline__ int blocks_find(const BlockSegment* seg, int n_seg, int kind, uint32_t b)
{
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (uint32_t(seg[mid].first[kind]) <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// segment s as the bodies see it from real workgroup blockIdx.x: x, y and partial are the interval's
__device__ __forceinline__ VirtualGrid blocks_grid(const BlockSegment& g, int kind)
{
  return VirtualGrid{blockIdx.x - uint32_t(g.first[kind]), uint32_t(g.grid[kind])};
}
__device__ __forceinline__ SegmentView blocks_view(const ApplyArgs& a, const BlocksArgs& B, int s)
{
  const BlockSegment& g = B.seg[s];
  const int64_t o = g.row_begin - B.row0;
  return SegmentView{g.e_begin, g.e_end, g.e_begin - a.own_begin, g.e_end - a.own_begin, g.row_begin, g.row_begin + g.rows,
                     a.x + o, a.y + o, a.partial + g.first[B.kind], B.done_at + 16 * int64_t(s)};
}

// One vector.  DOT: the call's stop word first, then (in the body) the segment's: a workgroup of a segment that is
// done returns at once.
template <int NB, int NF, bool DOT = false>
__global__ void __launch_bounds__(64) apply_tile_blocks_kernel(const ApplyArgs a, const BlocksArgs B)
{
  if constexpr (DOT)
    if (*B.stop <= a.iteration) return;   // (uniform)
  const int s = blocks_find(B.seg, B.n_seg, B.kind, blockIdx.x);
  const SegmentView g = blocks_view(a, B, s);
  apply_tile_body<NB, NF, 1, DOT, 0>(a, g, blocks_grid(B.seg[s], B.kind), &a.theta, (g.e_end() - g.e_begin() + 63) / 64);
}

template <int G, bool DOT = false>
__global__ void __launch_bounds__(256) apply_csr_blocks_kernel(const ApplyArgs a, const BlocksArgs B)
{
  if constexpr (DOT)
    if (*B.stop <= a.iteration) return;   // (uniform)
  const int s = blocks_find(B.seg, B.n_seg, B.kind, blockIdx.x);
  apply_csr_body<G, 1, DOT, 1>(a, blocks_view(a, B, s), blocks_grid(B.seg[s], B.kind), &a.theta);
}

// apply2, stage 1: partial[block][i * HDD_MAX_VEC + j] = sum over the block's rows of v_i[r] w_j[r] (fixed row ->
// thread assignment, shuffle tree, then the four waves in order)
[[maybe_unused]] static __global__ void __launch_bounds__(256) apply2_partial_kernel(const double* v, int64_t ldv, int n_v, const double* w,
                                                             int64_t ldw, int n_u, int64_t n, double* partial)
{
  __shared__ double red[4][APPLY2_PAIRS];
  double acc[HDD_MAX_VEC][HDD_MAX_VEC];
#pragma unroll
  for (int i = 0; i < HDD_MAX_VEC; ++i)
#pragma unroll
    for (int j = 0; j < HDD_MAX_VEC; ++j) acc[i][j] = 0.0;
  for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < n; r += int64_t(gridDim.x) * 256) {
    double vi[HDD_MAX_VEC], wj[HDD_MAX_VEC];
#pragma unroll
    for (int i = 0; i < HDD_MAX_VEC; ++i) vi[i] = i < n_v ? v[i * ldv + r] : 0.0;
#pragma unroll
    for (int j = 0; j < HDD_MAX_VEC; ++j) wj[j] = j < n_u ? w[j * ldw + r] : 0.0;
#pragma unroll
    for (int i = 0; i < HDD_MAX_VEC; ++i)
#pragma unroll
      for (int j = 0; j < HDD_MAX_VEC; ++j) acc[i][j] = __builtin_fma(vi[i], wj[j], acc[i][j]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < HDD_MAX_VEC; ++i)
#pragma unroll
    for (int j = 0; j < HDD_MAX_VEC; ++j) {
      double s = acc[i][j];
      if (i < n_v && j < n_u)   // (uniform)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
      if (lane == 0) red[wave][i * HDD_MAX_VEC + j] = s;
    }
  __syncthreads();
  if (threadIdx.x < APPLY2_PAIRS) {
    const int p = threadIdx.x;
    partial[int64_t(blockIdx.x) * APPLY2_PAIRS + p] = ((red[0][p] + red[1][p]) + red[2][p]) + red[3][p];
  }
}

// stage 2: out[i * n_u + j] = the blocks' partial sums, in block order
[[maybe_unused]] static __global__ void __launch_bounds__(64) apply2_final_kernel(const double* partial, int n_blocks, int n_v, int n_u, double* out)
{
  const int p = threadIdx.x, i = p / HDD_MAX_VEC, j = p % HDD_MAX_VEC;
  if (i >= n_v || j >= n_u) return;
  double s = 0.0;
  for (int b = 0; b < n_blocks; ++b) s += partial[int64_t(b) * APPLY2_PAIRS + p];
  out[i * n_u + j] = s;
}

}  // namespace dev
}  // namespace hdd
