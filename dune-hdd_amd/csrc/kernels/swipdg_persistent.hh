// dune-hdd_amd/csrc/kernels/swipdg_persistent.hh -- the persistent, software-pipelined tile driver of the
// thread-per-element policies (swipdg_persistent_kernel: the pipeline skeleton; its stages -- tile schedule, tile
// layout, image fill, image stores -- are the named functions in front of it) and the two element-list kernels.
//
// gfx950's vmcnt is in order and counts stores: a wave that waits for a load issued after its stores
// also waits for those stores.  So each wave walks a sequence of tiles and orders its memory operations
//   [prefetch own data of tile t+1] [compute tile t -> LDS] [gathers of tile t+1] [stores of tile t]
// The loads of tile t+1 are in flight while tile t computes, the neighbour gathers are issued before the
// store burst, and the stores are branch-free buffer stores (fixed count, out-of-range ones dropped by
// the descriptor's range check), so the next wait can stay counted instead of draining the stores.
//
// LDS image.  Contiguous (element i at its CSR offset inside the tile, streamed with aligned 16-byte reads)
// puts the lanes' row blocks RB doubles apart: for Q1 (RB = 80 = 160 dwords) a ds_write_b64 meets only
// two bank pairs per 32 lanes, a 16-way conflict (80 such writes per tile).  Policies with P::PAD stage
// *uniform* tiles (every element with all NF faces interior: tile length = nact * RB, the bulk of a mesh)
// rotated instead: lane i's value j at lds[i RB + (j + 2 ((i >> 1) & 15)) mod RB] -- 2-way conflicts (the
// floor for a layout that keeps value pairs 16-byte aligned), no padding, so the image is exactly 64 RB
// doubles (40 KB for Q1: 4 tiles per CU instead of 3), and the reader fetches each 16-byte chunk of the
// tile's CSR range with one ds_read_b128.  Other tiles use the contiguous image; for P::PAD policies their
// tail lanes dump into the image's last row block (free: a non-uniform tile with < 64 elements holds at
// most 63 RB - NB^2 values).
#pragma once
#include <cstdint>

#include "swipdg_elements.hh"
#include "swipdg_policy.hh"

// profiling ablations (HDD_DEBUG_FLAGS at run time) exist only in a library built with -DHDD_ABLATION
// (scripts/ablate.py): 1 = skip compute, 2 = drop the value stores, 4 = skip the neighbour gathers; 4194304 = no
// workgroup reserve (read by swipdg_launch.hh, which includes this header).  Every other bit is retired.
#ifdef HDD_ABLATION
#define HDD_ABL(a, bit) (((a).debug_flags & (bit)) != 0)
#else
#define HDD_ABL(a, bit) false
#endif

namespace hdd {
namespace dev {

// offset of this lane's row block inside the tile: NB^2 * sum over the active lanes below of (1 + interior
// faces) -- the pattern's elem_ptr rule -- from ballots + mbcnt instead of a per-element elem_ptr load
template <int NB>
__device__ __forceinline__ int tile_offset(int c, bool active)
{
  auto below = [](uint64_t m) {
    return int(__builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u)));
  };
  int sum = below(__ballot(active));
  sum += below(__ballot(active && (c & 1)));
  sum += 2 * below(__ballot(active && (c & 2)));
  sum += 4 * below(__ballot(active && (c & 4)));
  return NB * NB * sum;
}

// The tile positions [t, t_end) in steps of t_step that workgroup b of G walks.  XCD-aware: hardware block b runs
// on XCD b % 8, and the 8 XCDs sweep contiguous eighths of the tile range.
struct TileRange {
  int64_t t, t_end, t_step;
};
__device__ __forceinline__ TileRange tile_range(int64_t b, int64_t G, int64_t n_tiles)
{
  if (G >= n_tiles) return {b, b + 1, 1};
  const int64_t x = b & 7, w = b >> 3, gx = G >> 3;
  const int64_t s0 = (n_tiles * x) / 8, s1 = (n_tiles * (x + 1)) / 8;
  return {s0 + w, s1, gx};
}

// sizes of a policy's LDS tile image
template <class P>
struct TileImage {
  static constexpr int RB = P::RB;
  static constexpr int IMG = image_blocks<P>() * RB;   // doubles
  static constexpr int STORES = (IMG / 2 + 63) / 64;   // 16-byte stores per lane that cover it
  static constexpr int IMGS = IMG + 2 + RB;   // TWO: doubles per image (+ the alignment slot and the tail lanes' scratch row)
};

// One tile as the stages see it (everything but lane, active and off is wave-uniform)
struct Tile {
  int lane;
  bool active;                       // the lane holds an element of the tile
  int nact;                          // elements of the tile
  int64_t base, tile_end, base_al;   // the tile's CSR value range; base_al: the 16-byte aligned image origin
  int tlen;                          // tile_end - base
  // FULLTILE policies: a tile of 64 elements whose row blocks all have the maximum length (every face interior) --
  // the bulk of a mesh -- has a static image layout (lane l at l RB) and takes the branch-free compute_full
  bool fullt;
  int off;                           // image position of the lane's row block (contiguous image)
  // sharded step (a.skip_ghost): the row blocks of elements with a ghost face neighbour are written by the
  // element pass on the transfer stream, concurrently -- this tile must not store them (mask of those lanes)
  uint64_t gmask;
  bool uni;                          // PAD policies: a uniform tile (rotated image)
};
template <class P, bool SKIP>
__device__ __forceinline__ Tile tile_layout(const AssembleArgs& a, int64_t tile, int lane, int64_t base, int64_t tile_end,
                                            const typename P::Own& own)
{
  Tile T;
  T.lane = lane;
  T.base = base;
  T.tile_end = tile_end;
  const int64_t t0 = a.own_begin + tile * 64;
  T.active = t0 + lane < a.own_end;
  T.base_al = base & ~int64_t(1);
  T.tlen = int(tile_end - base);
  T.fullt = P::FULLTILE && T.tlen == 64 * P::RB;
  if (T.fullt) T.off = lane * P::RB + int(base - T.base_al);
  else T.off = tile_offset<P::NB>(P::n_interior(own), T.active) + int(base - T.base_al);
  T.gmask = 0;
  if constexpr (SKIP) {
    bool g = false;
#pragma unroll
    for (int f = 0; f < P::NF; ++f) g |= own.nbr[f] >= 0 && (own.nbr[f] < a.own_begin || own.nbr[f] >= a.own_end);
    T.gmask = __ballot(T.active && g);
  }
  T.nact = int(a.own_end - t0 < 64 ? a.own_end - t0 : 64);
  T.uni = P::PAD && T.tlen == P::RB * T.nact;
  return T;
}

// Image ranges [rb, re) of a tile's skipped elements (SKIP launches: the lanes of gmask), tile coordinates.  A tile
// holds one or two as a rule -- a strip's row end and the next row's start: the first NR go to scalar registers, any
// further ones are read from their lanes in a (wave-uniform) loop.  bo / be: the lane's own range.
template <int NR>
struct SkipRanges {
  int rb[NR], re[NR];
  uint64_t rest;
  int bo, be;
  __device__ __forceinline__ SkipRanges(uint64_t gmask, int bo_, int be_) : rest(gmask), bo(bo_), be(be_)
  {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      rb[i] = re[i] = 0;
      if (rest) {
        const int l = __builtin_ctzll(rest);
        rest &= rest - 1;
        rb[i] = __builtin_amdgcn_readlane(bo, l);
        re[i] = __builtin_amdgcn_readlane(be, l);
      }
    }
  }
  __device__ __forceinline__ bool contains(int d) const   // image position d inside a skipped element's block
  {
    bool r = false;
#pragma unroll
    for (int i = 0; i < NR; ++i) r |= d >= rb[i] && d < re[i];
    for (uint64_t mm = rest; mm; mm &= mm - 1) {   // more than NR skipped elements
      const int l = __builtin_ctzll(mm);
      r |= d >= __builtin_amdgcn_readlane(bo, l) && d < __builtin_amdgcn_readlane(be, l);
    }
    return r;
  }
};

// rotated-image slot of a uniform tile's CSR value d (what RotImg with rot = 2 ((lane >> 1) & 15) wrote)
template <int RB>
__device__ __forceinline__ int rot_slot(int d)
{
  const int l = d / RB, j = d - l * RB;
  const int q = j + 2 * ((l >> 1) & 15);
  return l * RB + (q < RB ? q : q - RB);
}

// The value stores' cache policy: nt (aux 2).  nt + sc1 (aux 18) measured 0.5350 -> 0.5208 ms in interleaved
// 10-launch loops but +1.0 % in the bench's own 20 / 5 window against the nt library (same box, 3 alternations);
// C2 measured within noise of nt for nt + sc1, sc1 and sc0 + nt (20 interleaved rounds): kept nt
// (profiles/r05/f_aux/).
constexpr int STORE_NT = 2;
__device__ __forceinline__ void store_b128_nt(const dvec2& v, __amdgpu_buffer_rsrc_t rsrc, int voffset, int soffset = 0)
{
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ivec4, v), rsrc, voffset, soffset, STORE_NT);
}
__device__ __forceinline__ void store_b64_nt(double v, __amdgpu_buffer_rsrc_t rsrc, int voffset)
{
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(ivec2, v), rsrc, voffset, 0, STORE_NT);
}
// nbytes of the value array from p on: stores beyond are dropped by the range check
__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_rsrc(double* p, int nbytes)
{
  return __builtin_amdgcn_make_buffer_rsrc(p, (short)0, nbytes, 0x00020000);
}
// the wave's LDS writes become visible to its reads
__device__ __forceinline__ void lds_wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------
// Whole-image stage: [compute tile t -> LDS][gathers t+1][stores t] through an image of 64 row blocks
// ------------------------------------------------------------------------------------------------
// Stores of a tile with skipped elements (T.gmask != 0) from the image img to out; rsrc covers the tile's 16-byte
// aligned interior, nbytes from out + start.  Uniform rotated tiles drop the skipped elements' chunks (element
// blocks are RB doubles apart and RB is even, so no 16-byte chunk straddles two elements); contiguous images test
// each chunk against the skipped elements' ranges.  blk_len: values of the lane's own row block.
template <class P>
__device__ __forceinline__ void store_image_skip(const Tile& T, const double* img, double* out,
                                                 __amdgpu_buffer_rsrc_t rsrc, int64_t start, int nbytes, int blk_len)
{
  constexpr int RB = P::RB, IMG = TileImage<P>::IMG, STORES = TileImage<P>::STORES;
  const int lane = T.lane;
  if (P::PAD && T.uni) {   // (Q1 row blocks are multiples of 16 doubles: base is even, start == base)
    if (!(T.gmask & 1)) out[T.base] = img[rot_slot<RB>(0)];
    if (!((T.gmask >> ((T.tlen - 1) / RB)) & 1)) out[T.tile_end - 1] = img[rot_slot<RB>(T.tlen - 1)];
    const int dmax = T.tlen - 2;
#pragma unroll 1   // (a rolled loop: the unrolled form's 40 offsets cost the main path 90 AGPRs)
    for (int k = 0; k < STORES; ++k) {
      const int d = 2 * (lane + 64 * k);
      const dvec2 v = *reinterpret_cast<const dvec2*>(img + rot_slot<RB>(d <= dmax ? d : 0));
      const int o8 = ((T.gmask >> (d <= dmax ? d / RB : 0)) & 1) ? nbytes : d * 8;
      store_b128_nt(v, rsrc, o8);
    }
  } else if (!T.uni) {
    // contiguous image: each chunk tests its two doubles against the skipped ranges: one 16-byte store when
    // neither is skipped, one 8-byte store when exactly one is
    const SkipRanges<4> skip(T.gmask, T.off, T.off + blk_len);
    const int a0 = int(start - T.base_al);   // image position of the first chunk
    if (!skip.contains(int(T.base - T.base_al))) out[T.base] = img[T.base - T.base_al];
    if (!skip.contains(int(T.tile_end - 1 - T.base_al))) out[T.tile_end - 1] = img[T.tile_end - 1 - T.base_al];
#pragma unroll
    for (int k = 0; k < STORES; ++k) {
      const int idx = 2 * (lane + 64 * k);
      const int li = idx < IMG ? idx : 0;
      const dvec2 v = *reinterpret_cast<const dvec2*>(img + a0 + li);
      // (even blocks, Q1: a chunk's two doubles always share an element)
      const bool s0 = skip.contains(a0 + li), s1 = (P::NB * P::NB) % 2 == 1 ? skip.contains(a0 + li + 1) : s0;
      store_b128_nt(v, rsrc, s0 || s1 ? nbytes : idx * 8);
      if constexpr ((P::NB * P::NB) % 2 == 1) {   // odd blocks (P1): a mixed chunk's unskipped half alone
        const int o8 = s0 == s1 ? nbytes : (s0 ? idx * 8 + 8 : idx * 8);
        store_b64_nt(s0 ? v.y : v.x, rsrc, o8);
      }
    }
  }
}

// Stores of a tile from the image img to out: the head and tail doubles that the 16-byte aligned interior
// [start, start + nbytes) leaves, then STORES 16-byte chunks per lane (those beyond nbytes dropped by rsrc's range)
template <class P, bool SKIP>
__device__ __forceinline__ void store_image(const Tile& T, const double* img, double* out, __amdgpu_buffer_rsrc_t rsrc,
                                            int64_t start, int nbytes, int blk_len)
{
  constexpr int RB = P::RB, IMG = TileImage<P>::IMG, STORES = TileImage<P>::STORES;
  const int lane = T.lane;
  if constexpr (SKIP) {
    if (T.gmask) {
      store_image_skip<P>(T, img, out, rsrc, start, nbytes, blk_len);
      return;
    }
  }
  if (P::PAD && T.uni) {
    const double head = img[rot_slot<RB>(0)];
    const double tail = img[rot_slot<RB>(T.tlen - 1)];
    out[T.base] = head;
    out[T.tile_end - 1] = tail;
    // PAD policies have even row blocks (NB^2 = 16), so a tile's base is even, start == base, and every 16-byte chunk
    // is one aligned LDS pair
    static_assert(!P::PAD || (P::NB * P::NB) % 2 == 0, "rotated image: even row blocks");
    const int dmax = T.tlen - 2;
#pragma unroll
    for (int k = 0; k < STORES; ++k) {
      const int d = 2 * (lane + 64 * k);
      const dvec2 v = *reinterpret_cast<const dvec2*>(img + rot_slot<RB>(d <= dmax ? d : 0));
      store_b128_nt(v, rsrc, d * 8);
    }
  } else {
    const double head = img[T.base - T.base_al];
    const double tail = img[T.tile_end - 1 - T.base_al];
    out[T.base] = head;
    out[T.tile_end - 1] = tail;
    const double* src = img + (start - T.base_al);
#pragma unroll
    for (int k = 0; k < STORES; ++k) {
      const int idx = 2 * (lane + 64 * k);
      const int li = idx < IMG ? idx : 0;
      const dvec2 v = *reinterpret_cast<const dvec2*>(src + li);
      store_b128_nt(v, rsrc, idx * 8);
    }
  }
}

// [compute tile t -> LDS], in two functions.  fill_full_tile: the branch-free compute_full of FULLTILE policies on a
// full tile (false: not taken); fill_image: every other case -- PAD (rotated for uniform tiles) / TWO / FUSED / plain.
// Two functions on purpose: with compute_full and compute behind ONE call boundary (whatever its form: Tile or
// scalars, by value or by reference, forceinline or not) the compiler merges their common head and the C2 kernel
// goes from 188 to 200 VGPRs; one policy call per function leaves it as it was.
template <class P>
__device__ __forceinline__ bool fill_full_tile(const AssembleArgs& a, const Tile& T, int64_t e,
                                               const typename P::Own& own, const typename P::Gat& gat, double* lds)
{
  if constexpr (P::FULLTILE) {
    if (T.fullt && !HDD_ABL(a, 1)) {
      P::compute_full(a, e, own, gat, lds + T.off);
      return true;
    }
  }
  return false;
}
template <class P>
__device__ __forceinline__ void fill_image(const AssembleArgs& a, const Tile& T, int64_t e, const typename P::Own& own,
                                           const typename P::Gat& gat, typename P::Shared& shv, double* lds,
                                           double* scratch)
{
  constexpr int RB = P::RB;
  const bool uni = T.uni, active = T.active;
  const int off = T.off, lane = T.lane;
  if constexpr (P::PAD) {
    const RotImg<RB> img{uni ? lds + lane * RB : (active ? lds + off : scratch),
                         uni ? 2 * ((lane >> 1) & 15) : 0};
    if (!HDD_ABL(a, 1)) P::compute(a, e, own, gat, img);
  } else {
    double* img = active ? lds + off : scratch;
    if constexpr (P::TWO) {   // the shared part once, then both components into their images
      P::prepare(a, own, shv);
      if (!HDD_ABL(a, 1)) P::emit_two(a, e, own, gat, shv, img, img + TileImage<P>::IMGS);
    } else if constexpr (P::FUSED) {   // the shared part once, then component 0 (the others after its stores)
      P::prepare(a, own, shv);
      if (!HDD_ABL(a, 1)) P::emit_component(a, 0, e, own, gat, shv, img);
    } else {
      if (!HDD_ABL(a, 1)) P::compute(a, e, own, gat, img);
    }
  }
}

// [gathers t+1][stores t] of a whole image: the first gather stage of tile t+1 (en, own_n, gat_n), then the stores
// of every component (TWO: the second image; FUSED: the other components are emitted into the same image slots)
template <class P, bool SKIP>
__device__ __forceinline__ void store_whole_images(const AssembleArgs& a, const Tile& T, int64_t e,
                                                   const typename P::Own& own, const typename P::Gat& gat,
                                                   const typename P::Shared& shv, double* lds, double* scratch,
                                                   int64_t en, typename P::Own& own_n, typename P::Gat& gat_n)
{
  const int64_t start = (T.base + 1) & ~int64_t(1);
  const int64_t stop = T.tile_end & ~int64_t(1);
  const int nbytes = stop > start && !HDD_ABL(a, 2) ? int(stop - start) * 8 : 0;
  const int blk_len = P::NB * P::NB * (P::n_interior(own) + 1);
  double* out = a.vals[0];
  const __amdgpu_buffer_rsrc_t rsrc = out_rsrc(out + start, nbytes);
  if (!HDD_ABL(a, 4)) P::load_gat(a, en, own_n, gat_n);
  store_image<P, SKIP>(T, lds, out, rsrc, start, nbytes, blk_len);
  if constexpr (P::TWO) {   // component 1 from the second image
    out = a.vals[1];
    store_image<P, SKIP>(T, lds + TileImage<P>::IMGS, out, out_rsrc(out + start, nbytes), start, nbytes, blk_len);
  } else if constexpr (P::FUSED) {   // the other components: same image slots, their own value arrays
    for (int c = 1; c < a.n_comp; ++c) {
      double* img = T.active ? lds + T.off : scratch;
      if (!HDD_ABL(a, 1)) P::emit_component(a, c, e, own, gat, shv, img);
      lds_wave_sync();
      out = a.vals[c];
      store_image<P, SKIP>(T, lds, out, out_rsrc(out + start, nbytes), start, nbytes, blk_len);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Half images (HALF policies, Q1; the HALF branch of the kernel): the tile's row blocks reach HBM in two halves,
// elements 0-31 and then 32-63, each half's 32 row blocks staged in a 20 KB LDS image and streamed out as one contiguous CSR range
// ([base, base + len0), then [base + len0, tile_end); Q1 row blocks are multiples of 16 values and base is even, so
// both ranges are 16-byte aligned).  20 KB images fit 8 tiles per CU: two waves per SIMD at <= 256 registers.
//
// Every lane computes its element's 80 values ONCE, into registers (all 64 lanes busy), and
// v_permlane32_swap regroups them by half: afterwards V[0..39] hold, in lanes 0-31, rows 0-1 of elements
// 0-31 and, in lanes 32-63, rows 2-3 of elements 0-31 (lane l - 32's); V[40..79] the same for elements 32-63.
// So a half's image takes 40 full-width ds_write_b64, and no element is computed twice (round 4 computed each
// half under a 32-lane exec mask: +57 % VALU instructions for the same output).  The placement of
// a value (row offsets, column offsets, which blocks exist) is computed by the lane that owns the element and
// swapped the same way.
//
// Full uniform tiles (64 elements with four interior faces each: the bulk of a mesh) use a rotated image:
// element m of the half, value (row r, column x) of its row block at
//   m * 80 + 20 ((r + rho_m) & 3) + ((x + rot_m) mod 20),  rot_m = 2 (m & 1), rho_m = (m & 7) >> 1,
// so the 16 lanes of a ds_write_b64 group (elements m and m + 8 share (rot, rho)) hit 8 distinct 8-byte bank
// pairs for every (r, x): 2-way, the floor while value pairs stay 16-byte aligned for the reader (an
// exhaustive search over per-element (row, column) rotations; rotating columns alone mod 20 gives at most 4
// conflict-free elements).  Other tiles (partial, boundary elements) use the contiguous image (CSR order) with
// per-block predicates.  (Sharded SKIP tiles stay on the rotated image: their skipped elements' chunks are dropped
// at the store.)
//
// half_rot_addresses, half_put0 and the policy's emit are the named parts.  The lane's placement and the two-half
// store loop are still written out in the kernel (its HALF branch): behind a function boundary -- a struct with
// members, free functions with the arrays passed by reference, the column and the row part alone -- the placement
// cost the C4 kernel its allocation (223 -> 221 / 222 VGPRs), and the store loop as a function let the compiler put
// half 1's first VALU write into the data registers of half 0's last register-soffset store (the hazard
// tests/test_isa_hazards.py scans for: 12 of 12 SKIP instantiations).  DESIGN.md 4 lists the variants.
// ------------------------------------------------------------------------------------------------

// Rotated half image: the tile-invariant LDS byte addresses of the lane's two row bases (hrow, writer) and of its
// chunks 0..4 (hrd, reader; chunk k + 5 j lies 5120 j bytes further)
template <int RB>
__device__ __forceinline__ void half_rot_addresses(int lane, uint32_t (&hrow)[2], uint32_t (&hrd)[5])
{
  const int m = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i) hrow[i] = uint32_t(m * RB + 20 * ((i + 2 * hi + ((m & 7) >> 1)) & 3)) * 8u;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int c = lane + 64 * k, mc = c / 40, u = c % 40, r = u / 10, x = 2 * (u % 10);
    const int rot2 = 2 * (mc & 1), rho = (mc & 7) >> 1;
    const int w = x + rot2;
    hrd[k] = uint32_t(mc * RB + 20 * ((r + rho) & 3) + (w >= 20 ? w - 20 : w)) * 8u;
  }
}

// Write side of the half-image branch: one 4 x 4 block as the closed forms complete it, rows (0, 1) and (2, 3) swapped
// between the wave's halves, half 0's part straight into the image, half 1's part kept in the registers V1
template <class P>
__device__ __forceinline__ void half_put0(char* ldsb, int b, const double (&blk)[P::NB][P::NB], uint32_t pk0,
                                          const uint32_t (&W0)[P::VR / 4], const uint32_t (&row0)[2],
                                          double (&V1)[P::NV80 / 2])
{
  double lo[2][P::NB];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int c = 0; c < P::NB; ++c) {
      ivec2 x = __builtin_bit_cast(ivec2, blk[i][c]), y = __builtin_bit_cast(ivec2, blk[i + 2][c]);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const auto r = __builtin_amdgcn_permlane32_swap(unsigned(x[d]), unsigned(y[d]), false, false);
        x[d] = int(r[0]);
        y[d] = int(r[1]);
      }
      lo[i][c] = __builtin_bit_cast(double, x);
      V1[i * P::VR + b * P::NB + c] = __builtin_bit_cast(double, y);
    }
  if ((pk0 >> b) & 1u) {
#pragma unroll
    for (int c = 0; c < P::NB; ++c) {
      const uint32_t w = ((W0[(b * P::NB + c) / 4] >> (8 * ((b * P::NB + c) % 4))) & 255u);
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<double*>(ldsb + row0[i] + w) = lo[i][c];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The kernel: the pipeline skeleton.  TL: tiles come from a.tile_list, else 0..n_tiles-1; SKIP: the sharded step's
// full-range launch, which leaves the row blocks of elements with a ghost face neighbour to the concurrent element
// pass (a.skip_ghost)
// ------------------------------------------------------------------------------------------------
template <class P, bool TL, bool SKIP = false>
__global__ void __launch_bounds__(64, P::MINW)
swipdg_persistent_kernel(const AssembleArgs a, int64_t n_tiles)
{
  constexpr int RB = P::RB, IMG = TileImage<P>::IMG;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  const int64_t G = gridDim.x, b = blockIdx.x;
  const TileRange r = tile_range(b, G, n_tiles);
  int64_t t = r.t;
  const int64_t t_end = r.t_end, t_step = r.t_step;
  if (t >= t_end) return;
  double* scratch = P::PAD ? lds + IMG - RB : lds + IMG + 2;
  // Loads whose values must be wave-uniform (tile ids of a tile list, the tiles' CSR bounds elem_ptr[]) are
  // vector loads (the compiler cannot prove elem_ptr unaliased by the value stores, so no s_load); a
  // readfirstlane right after such a load waits for it -- and, vmcnt being in order, for the previous tile's
  // stores issued before it.  So they are issued one tile ahead as raw values and made uniform only in the
  // next iteration, where the wait is a counted one behind the stores.
  // Tile list (interior / halo-boundary split of a sharded assembly): position -> tile.
  auto tile_raw = [&](int64_t pos) -> int64_t {
    if constexpr (TL) return int64_t(a.tile_list[pos]);
    return pos;
  };
  // HALF policies, full uniform tiles: tile-invariant LDS byte addresses of the lane's two row bases (writer) and of
  // its chunks 0..4 (reader; chunk k + 5 j lies 5120 j bytes further)
  [[maybe_unused]] uint32_t hrow[2] = {0u, 0u}, hrd[5] = {0u, 0u, 0u, 0u, 0u};
  if constexpr (P::HALF) half_rot_addresses<RB>(lane, hrow, hrd);
  auto uni64 = [](int64_t v) -> int64_t { return __builtin_amdgcn_readfirstlane(v); };
  auto elem_of_tile = [&](int64_t tile) {
    const int64_t t0 = a.own_begin + tile * 64;
    const int64_t e0 = t0 + lane;
    return e0 < a.own_end ? e0 : t0;
  };
  auto bounds_raw = [&](int64_t tile, int64_t& base_r, int64_t& end_r) {
    const int64_t t0 = a.own_begin + tile * 64;
    const int64_t tend = t0 + 64 < a.own_end ? t0 + 64 : a.own_end;
    base_r = a.elem_ptr[t0 - a.own_begin];
    end_r = a.elem_ptr[tend - a.own_begin];
  };
  auto next = [&](int64_t pos) { return pos + t_step < t_end ? pos + t_step : pos; };
  int64_t tile = uni64(tile_raw(t));
  int64_t e = elem_of_tile(tile);
  typename P::Own own;
  typename P::Gat gat;
  P::load_own(a, e, own);
  P::load_gat(a, e, own, gat);
  P::load_gat2(a, gat);
  int64_t base_r, tile_end_r;
  bounds_raw(tile, base_r, tile_end_r);
  int64_t tile_n_r = tile_raw(next(t));
  // Drain the prologue's loads before entering the loop.  The compiler's wait counts at the loop head are
  // the minimum over the entry paths: entered straight from the prologue, the first tile's vertex rows
  // are followed by only ~7 memory operations, so the first compute of EVERY iteration waited with
  // vmcnt(7) -- i.e. for all but the last two of the previous tile's 20 stores.  With nothing outstanding
  // on entry only the back edge counts, and that wait skips the stores (in-order vmcnt).
  __builtin_amdgcn_s_waitcnt(0);
  for (;;) {
    const bool has_next = t + t_step < t_end;
    const int64_t tn = has_next ? t + t_step : t;
    // own data of the next tile; its id was loaded one iteration ago
    const int64_t tile_n = uni64(tile_n_r);
    const int64_t en = elem_of_tile(tile_n);
    typename P::Own own_n;
    P::load_own(a, en, own_n);
    int64_t base_n_r, tile_end_n_r;
    bounds_raw(tile_n, base_n_r, tile_end_n_r);   // CSR bounds of tile t+1
    const int64_t tile_nn_r = tile_raw(next(tn));
    const int64_t base = uni64(base_r), tile_end = uni64(tile_end_r);   // loaded one iteration ago
    const Tile T = tile_layout<P, SKIP>(a, tile, lane, base, tile_end, own);
    // [compute tile t -> LDS][first gather stage of tile t+1][stores of tile t]
    typename P::Gat gat_n;
    if constexpr (P::HALF) {
      static_assert(P::PAD && !P::FUSED && RB == 80, "half images: the Q1 closed-form policy");
      const int off = T.off, tlen = T.tlen, nact = T.nact;
      const bool active = T.active;
      const uint64_t gmask = T.gmask;
      // (T's fields as locals and T.uni spelled out: with T.uni / T.nact used directly the SKIP instantiations
      // allocate so that a VALU write follows the last register-soffset store into its data registers -- the
      // store-data hazard below; tests/test_isa_hazards.py)
      const bool uni = tlen == RB * nact;
      double* const out = a.vals[0];
      constexpr int STH = IMG / 128;   // 16-byte chunks per lane per half (20)
      constexpr int NH = P::NV80 / 2;  // values per lane per half (40)
      static_assert(STH % 4 == 0, "SKIP tiles store a half in 4 KB windows");
      // (sharded SKIP tiles stay on the rotated image: their skipped elements' chunks are dropped at the store)
      const bool full = uni && nact == 64;   // wave-uniform
      int ps, pf[P::NF];
      P::positions(e, own, ps, pf);
      // column byte offsets of the lane's own element: (x + rot) mod 20 (rotated image) or x (contiguous), x = block
      // position * 4 + column; 8 bits each, four per register
      const int rot2 = full ? 2 * (lane & 1) : 0;
      auto col8 = [&](int x) {
        const int w = x + rot2;
        return uint32_t(w >= P::VR ? w - P::VR : w) * 8u;
      };
      uint32_t W0[P::VR / 4], W1[P::VR / 4];
#pragma unroll
      for (int g = 0; g < P::VR / 4; ++g) {
        uint32_t w = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int q = 4 * g + s, b = q / P::NB, c = q % P::NB;
          const int x = b == 0 ? ps * P::NB + c : pf[b - 1] * P::NB + role_slot<Cube>(own.finfo, b - 1, c);
          w |= col8(x) << (8 * s);
        }
        W0[g] = w;
      }
      // contiguous image: the element block's byte offset in the tile image, the row length in bytes, and which of
      // its blocks exist (bit 0: the element is active, bit 1 + f: face f has a neighbour)
      uint32_t ob0 = uint32_t(off) * 8u, rl0 = uint32_t(P::NB * (P::n_interior(own) + 1)) * 8u, pk0 = active ? 1u : 0u;
#pragma unroll
      for (int f = 0; f < P::NF; ++f) pk0 |= (active && own.nbr[f] >= 0 ? 2u : 0u) << f;
      // the element a lane writes in half h is (lane & 31) + 32 h: after the swaps X0 holds half 0's, X1 half 1's
      auto swap32 = [](uint32_t& x0, uint32_t& x1) {
        const auto r = __builtin_amdgcn_permlane32_swap(x0, x1, false, false);
        x0 = r[0];
        x1 = r[1];
      };
#pragma unroll
      for (int g = 0; g < P::VR / 4; ++g) {
        W1[g] = W0[g];
        swap32(W0[g], W1[g]);
      }
      uint32_t ob1 = ob0, rl1 = rl0, pk1 = pk0;
      swap32(ob0, ob1);
      swap32(rl0, rl1);
      swap32(pk0, pk1);
      const int len0 = full ? 32 * RB : (nact > 32 ? __builtin_amdgcn_readlane(off, 32) : tlen);
      // LDS byte address of the lane's two rows (rows i + 2 (lane >> 5) of its element) in each half's image
      uint32_t row0[2], row1[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t ri = uint32_t(i + 2 * (lane >> 5));
        row0[i] = full ? hrow[i] : ob0 + ri * rl0;
        row1[i] = full ? hrow[i] : ob1 - uint32_t(len0) * 8u + ri * rl1;
      }
      char* const ldsb = reinterpret_cast<char*>(lds);
      auto wcol = [](const uint32_t* Wh, int q) { return (Wh[q / 4] >> (8 * (q % 4))) & 255u; };
      // The values, one 4 x 4 block at a time as the closed forms complete it: rows (0, 1) and (2, 3) swapped
      // between the wave's halves, half 0's part straight into the image, half 1's part kept in registers
      double V1[NH];
      auto put0 = [&](int b, const double (&blk)[P::NB][P::NB]) { half_put0<P>(ldsb, b, blk, pk0, W0, row0, V1); };
      if (!HDD_ABL(a, 1)) P::emit(a, own, gat, put0);
      // sharded step: image ranges of the skipped elements, tile coordinates
      const SkipRanges<4> skip(gmask, off, off + P::NB * P::NB * (P::n_interior(own) + 1));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int hb = h ? len0 : 0, hl = (h ? tlen : len0) - hb;   // wave-uniform
        if (h == 1) {   // half 1's values from registers
#pragma unroll
          for (int b = 0; b < P::NF + 1; ++b) {
            if (!((pk1 >> b) & 1u)) continue;
#pragma unroll
            for (int c = 0; c < P::NB; ++c) {
              const uint32_t w = wcol(W1, b * P::NB + c);
#pragma unroll
              for (int i = 0; i < 2; ++i) *reinterpret_cast<double*>(ldsb + row1[i] + w) = V1[i * P::VR + b * P::NB + c];
            }
          }
        }
        lds_wave_sync();
        if (h == 1 && !HDD_ABL(a, 4)) P::load_gat(a, en, own_n, gat_n);   // first gather stage of tile t+1
        if (hl <= 0) continue;
        const int nb = HDD_ABL(a, 2) ? 0 : hl * 8;
        const __amdgpu_buffer_rsrc_t rh = out_rsrc(out + base + hb, nb);
        const uint32_t gm = SKIP ? uint32_t(gmask >> (32 * h)) : 0u;   // this half's skipped elements
        if (full && !gm) {   // 2560 values: every chunk in range, the lane part of the offset in voffset
#pragma unroll
          for (int k = 0; k < STH; ++k) {
            // lane l's chunk k + 5 j (CSR chunk l + 64 (k + 5 j)) sits at hrd[k] + 5120 j in the rotated image
            const dvec2 v = *reinterpret_cast<const dvec2*>(ldsb + hrd[k % 5] + 5120 * (k / 5));
            // soffset 1024 k: an SGPR, no VALU per store.  hipcc does not pad the hazard of a VALU write to a
            // > 8-byte store's data registers right after a store with a register soffset, and gfx950 then stores
            // a stale first dword (round 5, the SKIP branch below in its first form); nothing but LDS reads follows
            // these stores -- tests/test_isa_hazards.py scans the built library for the pattern.
            store_b128_nt(v, rh, 16 * lane, 1024 * k);
          }
        } else if (full) {   // a sharded SKIP tile: chunk l + 64 k belongs to element (l + 64 k) / 40 of the half (40
          // chunks per 640-byte row block); a skipped element's chunks get a voffset beyond the window and are
          // dropped.  The predicate's VALU follows the stores, so no register soffset here: 4 KB windows, one buffer
          // resource each, the offset inside in voffset + the instruction's immediate.
#pragma unroll
          for (int j = 0; j < STH / 4; ++j) {
            const int nbj = nb - 4096 * j;
            const __amdgpu_buffer_rsrc_t rj = out_rsrc(out + base + hb + 512 * j, nbj > 0 ? nbj : 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int k = 4 * j + q;
              const dvec2 v = *reinterpret_cast<const dvec2*>(ldsb + hrd[k % 5] + 5120 * (k / 5));
              const uint32_t vo = (gm >> ((lane + 64 * k) / 40)) & 1u ? 0x40000000u : 16u * lane;
              store_b128_nt(v, rj, vo + 1024 * q);
            }
          }
        } else {      // the range check drops the chunks beyond the half; skipped elements' chunks go out of range
#pragma unroll
          for (int k = 0; k < STH; ++k) {
            const int d = 2 * (lane + 64 * k);
            const dvec2 v = *reinterpret_cast<const dvec2*>(lds + d);
            const int o8 = SKIP && gmask && skip.contains(hb + d) ? nb : d * 8;
            store_b128_nt(v, rh, o8);
          }
        }
      }
    } else {
      [[maybe_unused]] typename P::Shared shv;
      if (!fill_full_tile<P>(a, T, e, own, gat, lds)) fill_image<P>(a, T, e, own, gat, shv, lds, scratch);
      lds_wave_sync();
      store_whole_images<P, SKIP>(a, T, e, own, gat, shv, lds, scratch, en, own_n, gat_n);
    }
    // second gather stage of tile t+1 (vertex-indexed geometry: the neighbours' off-face vertices by the
    // ids the first stage brought): its wait covers the first stage only, which was issued before the
    // stores of tile t (vmcnt is in order), so it never waits for those stores
    if (!HDD_ABL(a, 4)) P::load_gat2(a, gat_n);   // (ablation 4: no stage-1 ids to follow)
    if (!has_next) break;
    t = tn;
    tile_n_r = tile_nn_r;
    base_r = base_n_r;
    tile_end_r = tile_end_n_r;
    tile = tile_n;
    e = en;
    own = own_n;
    gat = gat_n;
  }
}

// ------------------------------------------------------------------------------------------------
// Element-list pass (a.list_elements): one lane per listed owned element -- the fixup of a sharded step, which
// assembles every tile while the halo is in flight and then recomputes only the elements that read a ghost
// (a few thousand: one lane each, its row block built in the lane's own LDS slot and written by that lane).
// ------------------------------------------------------------------------------------------------
template <class P>
__global__ void __launch_bounds__(64) swipdg_elements_kernel(const AssembleArgs a, int64_t n)
{
  constexpr int RB = P::RB;
  constexpr bool FUSED = P::FUSED;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  double* img = lds + lane * RB;
  for (int64_t i0 = int64_t(blockIdx.x) * 64; i0 < n; i0 += int64_t(gridDim.x) * 64) {
    const int64_t i = i0 + lane;
    const bool act = i < n;
    const int64_t e = a.own_begin + int64_t(a.tile_list[act ? i : i0]);
    typename P::Own own;
    typename P::Gat gat;
    P::load_own(a, e, own);
    P::load_gat(a, e, own, gat);
    P::load_gat2(a, gat);
    const int64_t base = a.elem_ptr[e - a.own_begin];
    const int len = P::NB * P::NB * (P::n_interior(own) + 1);
    [[maybe_unused]] typename P::Shared shv;
    if constexpr (FUSED) P::prepare(a, own, shv);
    const int ncomp = FUSED ? a.n_comp : 1;
    for (int c = 0; c < ncomp; ++c) {
      if constexpr (FUSED) {
        P::emit_component(a, c, e, own, gat, shv, img);
      } else if constexpr (P::PAD) {
        P::compute(a, e, own, gat, RotImg<RB>{img, 0});
      } else {
        P::compute(a, e, own, gat, img);
      }
      double* out = a.vals[c];
      if (act)
        for (int k = 0; k < len; ++k) __builtin_nontemporal_store(img[k], out + base + k);
    }
  }
}

// Element-list pass without LDS, so that it runs on the transfer stream beside a persistent assembly that holds
// the LDS (sharded step, shard_step.hip).  LIST_IN_PLACE: lane i writes the row block of listed element i in
// place (the concurrent assembly runs with a.skip_ghost and leaves those blocks alone; inactive lanes repeat
// lane 0's element); LIST_SIDE_BUFFER: into side buffers a.vals[c] + i RB (slot n: the inactive lanes' dummy), which
// fix_scatter_kernel copies into place after the join (round-3 A/B variant).
template <class P>
__global__ void __launch_bounds__(64) swipdg_elements_buf_kernel(const AssembleArgs a, int64_t n)
{
  constexpr int RB = P::RB;
  constexpr bool FUSED = P::FUSED;
  const int lane = threadIdx.x;
  for (int64_t i0 = int64_t(blockIdx.x) * 64; i0 < n; i0 += int64_t(gridDim.x) * 64) {
    const int64_t i = i0 + lane;
    const bool act = i < n;
    const int64_t e = a.own_begin + int64_t(a.tile_list[act ? i : i0]);
    const int64_t slot = act ? i : n;
    typename P::Own own;
    typename P::Gat gat;
    P::load_own(a, e, own);
    P::load_gat(a, e, own, gat);
    P::load_gat2(a, gat);
    if constexpr (P::EMIT) {
      if (a.list_elements == LIST_SIDE_SOA) {   // value-major side buffer: canonical value k of list entry i at vals[0][k fix_ld + i]
        double* const buf = a.vals[0] + i;
        P::emit(a, own, gat, [&](int b, const double (&blk)[P::NB][P::NB]) {
          if (!act) return;
#pragma unroll
          for (int r = 0; r < P::NB; ++r)
#pragma unroll
            for (int c = 0; c < P::NB; ++c) buf[int64_t(r * P::VR + b * P::NB + c) * a.fix_ld] = blk[r][c];
        });
        continue;
      }
    }
    [[maybe_unused]] typename P::Shared shv;
    if constexpr (FUSED) P::prepare(a, own, shv);
    const int ncomp = FUSED ? a.n_comp : 1;
    const int64_t dst = a.list_elements == LIST_IN_PLACE ?a.elem_ptr[e - a.own_begin] : slot * RB;
    for (int c = 0; c < ncomp; ++c) {
      double* img = a.vals[c] + dst;
      if constexpr (FUSED) P::emit_component(a, c, e, own, gat, shv, img);
      else if constexpr (P::PAD) P::compute(a, e, own, gat, RotImg<RB>{img, 0});
      else P::compute(a, e, own, gat, img);
    }
  }
}

}  // namespace dev
}  // namespace hdd
