// dune-hdd_amd/csrc/host/shard_plan.hh -- the schedule of one sharded step (hdd_block_assemble_sharded,
// csrc/kernels/shard_step.hip) as a value: a pure function of plain facts, host-only (no HIP, no RCCL), so a plain
// C++ compiler builds it and tests/host_asan/asan_host.cpp checks it against the documented truth table.  The two
// run-time fallbacks (HDD_ERR_UNSUPPORTED from a list kernel or from the tile-list kernel) depend on what a launch
// returns and stay in the executor.
#pragma once
#include <cstdint>

#include "hdd.h"

#pragma GCC visibility push(hidden)   // internal: not part of the library's exported symbols
namespace hdd {

enum class Schedule {
  Serial,         // exchange, then everything on `stream`
  SplitTiles,     // interior tiles during the exchange, the tiles with a ghost-adjacent element after it
  FixInline,      // side-stream pack and exchange, every tile beside it, the ghost-adjacent elements on `stream`
                  // after the join (also what a shard without ghost-adjacent elements gets)
  FixInPlace,     // the ghost-adjacent elements on the pack stream, in place, beside a SKIP launch
  FixRowBlocks,   // ... into a row-block side buffer, hdd_scatter_fix after the join
  FixSoa          // ... into a value-major side buffer beside a reserve launch, hdd_scatter_fix_q1_soa after the join
};
enum class PackOn { Stream, Transfer, Side };   // the caller's, the communicator's transfer stream, the shard's own
enum class CommKind { None, Host, Stream };     // no communicator, host-staged, stream-based (RCCL, device transport)

struct StepFacts {
  int32_t elem_type;        // HDD_SIMPLEX / HDD_CUBE / HDD_HEX
  int32_t n_peers;          // halo peers (> 0: a step without an exchange has no plan)
  int64_t n_in;             // interior tiles
  int64_t n_fix;            // owned elements with a ghost face neighbour
  uint32_t flags;           // HDD_SHARD_*
  bool transfer;            // a transfer happens (not the HDD_SHARD_NO_TRANSFER loopback)
  CommKind comm;
  bool kappa_closed_form;   // every diffusion factor HDD_FN_CONST or HDD_FN_PER_ELEM
  bool ablation;            // an HDD_ABLATION build
};

struct StepPlan {
  Schedule schedule = Schedule::Serial;
  PackOn pack_on = PackOn::Stream;
  bool pack_first = false;    // Q1: the pack on `stream` ahead of the tile launch (pack_on still carries the exchange)
  bool tiles_first = false;   // the full-range tile launch is enqueued before the halo work
  bool direct = false;        // comm_post runs on the caller's stream itself

  bool overlap() const { return schedule != Schedule::Serial; }
  bool side() const { return schedule >= Schedule::FixInline; }         // pack and exchange off `stream`
  bool off_stream_fix() const { return schedule >= Schedule::FixInPlace; }
  bool fix_buffer() const { return schedule >= Schedule::FixRowBlocks; }
  bool side_stream() const { return pack_on == PackOn::Side; }          // needs the shard's own stream
};

inline StepPlan plan_step(const StepFacts& f)
{
  const bool p1 = f.elem_type == HDD_SIMPLEX, q1 = f.elem_type == HDD_CUBE;
  const bool fix_flags = (f.flags & (HDD_SHARD_FIX_INLINE | HDD_SHARD_FIX_SCATTER | HDD_SHARD_FIX_INPLACE)) != 0;
  const bool split_flag = (f.flags & HDD_SHARD_SPLIT_TILES) != 0;
  StepPlan p;
  // Default schedule by element type and peer count (one-card step study, profiles/r04/e_reserve/): P1 ranks with
  // two peers split the tiles -- interior tiles during the exchange, the 2 % of tiles with a ghost-adjacent element
  // after it (C2 N = 8 middle rank +0.8 / +4.0 % over one launch, against +10.1 % for the side-buffer fixup and
  // +26.5 % in place, whose row blocks share cache lines with the tiles' stores: P1 blocks are 288 B); every other
  // shard keeps the off-stream element fixup in place (Q1: its split costs +18 %).
  const bool split = split_flag || (!fix_flags && p1 && f.n_peers >= 2 && f.n_in > 0);
  // Round 5, Q1: the serial step by default (pack, exchange, then one half-image launch over every tile).  One-card
  // study on the final kernels (profiles/r05/d_shard/, loopback transfer, back-to-back steps): C4 N = 8 end / middle
  // rank serial +8.5 / +12.3 % over one launch, the overlapped in-place step +16.7 / +20.8 %, the side buffer after
  // the join +13.4 / +18.9 %; N = 2 serial +2.2 / +3.1 %, overlapped +4.3 / +5.0 %.  The kernel trace shows why: the
  // half-image launch holds every wave slot it can (two waves per SIMD, all of the LDS), so the halo kernels beside
  // it wait for the reserved slots (a D2D copy 39 us instead of 5), and each cross-stream join costs ~5 us on the
  // step's critical path.  The overlapped schedules stay selectable (HDD_SHARD_FIX_INPLACE / _FIX_SCATTER / _SPLIT).
  const bool q1_serial = q1 && !fix_flags && !split_flag;
  // (a split without interior tiles has nothing to overlap; HDD_HEX takes no lists)
  if ((f.flags & HDD_SHARD_NO_OVERLAP) || f.elem_type == HDD_HEX || q1_serial || (split && f.n_in == 0)) {
    // direct: RCCL runs straight on `stream` -- nothing overlaps it there, and it saves the two cross-stream hops
    p.direct = true;
    return p;
  }
  if (split) {
    // The split keeps its pack on `stream` before the interior tiles: packing on the side stream beside them measured
    // +10.0 % against +5.3 % (C2 N = 8 middle rank, back-to-back, profiles/r04/o_final/).
    p.schedule = Schedule::SplitTiles;
    return p;
  }
  // The pack and the transfer leave the assembly stream when the assembly overlaps them: the RCCL transfer
  // stream (or, in the loopback study, the shard's side stream) waits for the inputs, packs and sends while
  // `stream` starts the assembly at once -- the pack launch is off the critical path.  (The host transport
  // stages through the host on the stream it is given, so it gets the shard's own.)
  p.pack_on = f.transfer && f.comm == CommKind::Stream ? PackOn::Transfer : PackOn::Side;
  // Q1: the pack runs on `stream` ahead of the tile launch.  Issued on the side stream beside the tile launch it
  // waited for a free wave slot: the half-image SKIP kernel holds 256 VGPRs in each of its two waves per SIMD and
  // all of the LDS, so a kernel beside it gets only the reserved workgroup slots -- the pack took 45 us there
  // against 5 us alone, and the element pass behind it ended after the tiles (one-card kernel trace,
  // profiles/r05/d_shard/).  On `stream` it costs its own few microseconds once, ahead of the launch.
  p.pack_first = q1;
  if ((f.flags & HDD_SHARD_FIX_INLINE) || f.n_fix == 0) {
    p.schedule = Schedule::FixInline;
    return p;
  }
  // Where the fixup writes: in place beside a tile launch that skips those row blocks, or a side buffer + one
  // copy kernel after the join.  Default from the one-card step study (profiles/r03/shard_step/final/, N = 2 and
  // 8): in place, except P1 ranks with two peers (C2 middle ranks: +10 % with the side buffer vs +14 % in place,
  // the P1 tiles' two waves per SIMD leaving the element pass no registers beside them; end ranks +4 % in place
  // vs +8 %); Q1 in place everywhere (+9 % middle / +15 % end rank at N = 8 vs +20 / +13 %)
  //
  // Round 5: Q1 keeps the in-place pass, now beside the half-image kernel's SKIP launch (full SKIP tiles stay on the
  // rotated image and drop the skipped elements' chunks at the store), with the pack ahead of the launch (above).
  // HDD_SHARD_FIX_SCATTER on Q1: the tile launch writes every row block (no SKIP), the ghost-adjacent elements go
  // into a value-major (SoA) side buffer -- each store instruction 64 consecutive doubles -- and one wave per
  // element writes its row block into place after the join (a kernel after the tiles: +18 % at C4 N = 8).
  if ((f.flags & HDD_SHARD_FIX_INPLACE) || !(f.flags & HDD_SHARD_FIX_SCATTER))
    p.schedule = Schedule::FixInPlace;
  // the value-major pass exists for the closed-form Q1 policy only (piecewise-constant kappa: Q1PwcPolicy::emit); a
  // smooth kappa (GenericPolicy) takes the row-block side buffer + hdd_scatter_fix like P1
  else
    p.schedule = q1 && f.kappa_closed_form ? Schedule::FixSoa : Schedule::FixRowBlocks;
  // With the in-place fixup (and the SoA side buffer's reserve launch) the full-range launch is enqueued BEFORE the
  // halo work by default, so it starts at once instead of after the host has issued pack, exchange and element pass
  // (one-card kernel timeline, profiles/r04/n_first/: C4 N = 8 step 113-120 -> 77-79 us when steps do not overlap;
  // back-to-back steps, where the host runs ahead, are unchanged).  It needs nothing the exchange delivers: the row
  // blocks that read a ghost column are the element pass's.  HDD_SHARD_LAUNCH_LAST (ablation builds only; the
  // product library ignores it): round 3's order.
  const bool last = f.ablation && (f.flags & HDD_SHARD_LAUNCH_LAST);
  p.tiles_first = !last && p.schedule != Schedule::FixRowBlocks;
  return p;
}

}  // namespace hdd
#pragma GCC visibility pop
