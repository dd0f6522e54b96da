// The stream kernel's shape rules, its LDS layout and the pass plan of a Sinkhorn grid call, stated once for the kernels
// (sinkhorn_kernels.hpp), the host (pilot_ot_sinkhorn.hip) and the host-only test (tests/sinkhorn_layout_dump.cpp).
// Plain C++17: no HIP include, no HIP call, no pointer.
#pragma once
#include <cstddef>
#include <cstdio>

#include "../../include/pilot_ot.h"

namespace pilot {

constexpr int WAVE = 64, WAVES_PER_WG = 4;
constexpr size_t LDS_BYTES = 160 * 1024;
constexpr int HANDOVER_BUF = 32, HANDOVER_FLUSH = 16;      // per-wave hand-over buffer of the fast kernels (ints), flush level
constexpr int RING_MAX = 16, GREG_MAX = 64;
constexpr int min_of(int a, int b) { return a < b ? a : b; }
#ifndef PILOT_SPLIT_OCC2_MAX_RT
#define PILOT_SPLIT_OCC2_MAX_RT 4
#endif
#ifndef PILOT_SPLIT_OCC2_MAX_RT_TRACK
#define PILOT_SPLIT_OCC2_MAX_RT_TRACK 4      // (K = 80 / 96 at reg 0.01: 160 -> 134 ms, 189 -> 146 ms with one wave and no spills; RT = 4: 32.5 -> 47.5 ms)
#endif
#ifndef PILOT_HALF_OCC2_MAX_RT
#define PILOT_HALF_OCC2_MAX_RT 7             // (fp16-split, piece state: c4 at K = 100 26.85 -> 26.07 ms with two waves and 144 B of spills)
#endif
#ifndef PILOT_HALF_SOLO_MIN_RT
#define PILOT_HALF_SOLO_MIN_RT 1         // (3: duplicates of the fp16-split configuration stay in tiles up to K = 32)
#endif
constexpr int HALF_SOLO_MIN_RT = PILOT_HALF_SOLO_MIN_RT, HALF_OCC4_MAX_RT = 2;
constexpr int SPLIT_OCC2_MAX_RT = PILOT_SPLIT_OCC2_MAX_RT, SPLIT_OCC2_MAX_RT_TRACK = PILOT_SPLIT_OCC2_MAX_RT_TRACK, HALF_OCC2_MAX_RT = PILOT_HALF_OCC2_MAX_RT;

enum { CFG_F32 = 0, CFG_F64 = 1, CFG_S32 = 2, CFG_H32 = 3 };   // CfgF32x16, CfgF64x16, CfgS32x16 (bf16-split products, f32 values), CfgH32x16 (fp16-split)
// The traits of a configuration that the rules below read (sinkhorn_launch.hpp checks them against the kernels' Cfg* structs).
struct CfgShape { int w, nreg; bool split, half; int np, tile, ngrp; };       // w = sizeof(T) / 4
constexpr CfgShape shape_of(int cfg) {
    return cfg == CFG_H32 ? CfgShape{1, 4, true, true, 2, 16, 4}
                          : (cfg == CFG_S32 ? CfgShape{1, 4, true, false, 3, 16, 4} : CfgShape{cfg == CFG_F64 ? 2 : 1, 4, false, false, 0, 16, 4});
}

// ---- register and occupancy rules of the stream kernel: its __launch_bounds__ and the host's launches read the same functions
constexpr int tail_steps(int RT) { return (RT - 1) * 4 + 1; }   // k-steps when only register 0 of the last tile is live
// the operand image is kept in registers when it needs <= 64 VGPRs per lane and the cost is symmetric
constexpr bool operands_in_regs(CfgShape c, int RT, bool sym) { return !c.split && sym && RT * c.nreg * RT * c.w <= GREG_MAX; }
// live panel registers per lane: A, B, U, V, ACC (+ RU, RV when tracking)
constexpr int panel_regs(CfgShape c, int RT, bool sym, bool track, int tv) {
    return (track ? 7 : 5) * RT * c.nreg * c.w + c.nreg * c.w + 56 +
           (tv > 0 ? 24 * c.w : 0) +                         // tail accumulators, broadcast pairs, weights in flight
           (c.split ? 3 * ((RT + 1) / 2) * 4 + 24 : 0) +     // split panel parts + operand parts in flight
           (operands_in_regs(c, RT, sym) ? (RT * c.nreg * RT + 2 * tv * tail_steps(RT)) * c.w : 0);
}
constexpr int min_waves_per_simd(CfgShape c, int RT, bool sym, bool track, int tv) {
    // split variants: two waves per SIMD up to SPLIT_OCC2_MAX_RT row tiles (tracking variants: SPLIT_OCC2_MAX_RT_TRACK), one wave
    // with the whole register file beyond (3 waves per SIMD at RT <= 4: slower)
    // (fp16-split fast kernel at one / two row-tiles: four -- 82 / 116 registers; with the sharded work queue the 634 x 14 cohort runs
    // 0.242 / 0.195 / 0.185 / 0.193 ms at 2 / 3 / 4 / 6 workgroups per CU, K = 16 .. 32 -12 .. -22 %: tools/small_k_occupancy_probe.py)
    if (c.half && !track && RT <= HALF_OCC4_MAX_RT) return 4;
    if (c.split) return RT <= (track ? SPLIT_OCC2_MAX_RT_TRACK : (c.half ? HALF_OCC2_MAX_RT : SPLIT_OCC2_MAX_RT)) ? 2 : 1;
    const int regs = panel_regs(c, RT, sym, track, tv);
    return regs <= 128 ? 4 : (regs <= 168 ? 3 : (regs <= 256 ? 2 : 1));
}
// solo_pairs (64 + ~45 registers of T per lane) rides in the fast launch when the cost is symmetric (PILOT's always is),
// K <= 64, and the launch's register budget holds it without spilling
constexpr bool solo_in_stream(CfgShape c, int RT, bool sym, bool track, int tv) {
    const int mw = min_waves_per_simd(c, RT, sym, track, tv);
    const int budget = mw >= 4 ? 128 : (mw == 3 ? 168 : 256);
    // (round 3 had the fp16-split configuration keep its duplicates in tiles up to K = 32, when a tile's update was shorter
    // than the one-wave-per-pair update; with the straight-line matrix-vector product it is the other way round again:
    // c2 kernel 0.154 -> 0.136 ms, the 1/8 shard of c3 0.253 -> 0.186 ms.  A rule by SHAPE, never by load: the same pair takes
    // the same path in every shard.)
    return !track && sym && RT <= 4 && !(c.half && RT < HALF_SOLO_MIN_RT) && (64 + 45) * c.w <= budget;
}
// ---- LDS of one stream-kernel workgroup, in elements of T ----------------------------------------------------------------
// one form of the operand block: a stationary MFMA A operand in lane order
constexpr int form_elems(CfgShape c, int RT) { return c.split ? c.np * ((RT + 1) / 2) * RT * WAVE * 4 : RT * c.tile * RT * c.tile; }
// finished pairs wait in a wave-private LDS ring for their cost product: per slot the u panel and the v panel (KP values
// each, [tile][group][reg] order) + 4 elements of padding (a lane's 16-byte reads of consecutive slots then fall on
// different banks) that hold POT's plan scale (1, or 1/K^2), the output index and the flags
// (fp16-split configuration: the panels are parked as packed pieces, [part][k-block][lane group] x 16 bytes per column --
// an odd row-tile count rounds up to whole k-blocks)
constexpr int ring_panel_elems(CfgShape c, int RT) { return c.half ? 2 * ((RT + 1) / 2) * c.ngrp * 4 : RT * c.tile; }
constexpr int ring_slot_stride(CfgShape c, int RT) { return 2 * ring_panel_elems(c, RT) + 4; }
// PARKED flush (split configurations, fast kernel, RT <= 4; see ring_flush in sinkhorn_kernels.hpp): a lane parks its U registers,
// or its packed U pieces, in a 16-byte line per row-tile
constexpr bool parked_flush(CfgShape c, int RT, bool track) { return c.split && !track && RT <= 4; }
constexpr int park_lane_elems(CfgShape c, int RT) { return c.half ? 2 * ((RT + 1) / 2) * 4 : RT * c.nreg; }
// tail-row weights (VALU tail rows, tv chains): form 0, and form 1 unless the cost is symmetric
constexpr int tail_weight_elems(CfgShape c, int RT, bool sym, int tv) { return (tv > 0 && !c.split) ? (sym ? 1 : 2) * tv * tail_steps(RT) * WAVE * 2 : 0; }
constexpr int handover_elems(CfgShape c) { return WAVES_PER_WG * HANDOVER_BUF / c.w; }
// The block: [operand images: one or two forms, times two with both exponent bands][first-product table: KP][tail-row weights]
// [rings: one of `ring` slots per wave][park area][hand-over buffers: one per wave, fast kernels only].  (The workgroups that run
// solo_pairs stage none of it: they keep one line of WAVE values per wave at its start.)
struct StreamLayout {
    int table, tail, rings, park, hb, end;           // offsets of the regions; end: behind the last one
    int slot, panel;                                 // a ring slot: [u: panel][v: panel][scale, output index, flags, pad]
    size_t bytes;
};
constexpr StreamLayout stream_layout(CfgShape c, int RT, bool sym, bool track, int tv, int bands, int ring) {
    StreamLayout l{};
    l.table = (sym ? 1 : 2) * form_elems(c, RT) * ((c.split && track && bands == 2) ? 2 : 1);
    l.tail = l.table + RT * c.tile;
    l.rings = l.tail + tail_weight_elems(c, RT, sym, tv);
    l.panel = ring_panel_elems(c, RT); l.slot = ring_slot_stride(c, RT);
    l.park = l.rings + WAVES_PER_WG * ring * l.slot;
    l.hb = l.park + (parked_flush(c, RT, track) ? WAVES_PER_WG * park_lane_elems(c, RT) * WAVE : 0);
    l.end = l.hb + (track ? 0 : handover_elems(c));
    l.bytes = (size_t)l.end * 4 * c.w;
    return l;
}
// Bytes, ring slots and resident workgroups of a launch.  The ring gets as many slots (<= RING_MAX) as fit while `want` workgroups
// stay resident per CU, at least min_ring; else fewer workgroups.  ring == 0: not even one slot per wave fits, and `bytes` is what
// one would need.  `inherited`: bytes a launch reserves beyond its kernel's layout (see plan_grid).
struct StreamLds { size_t bytes; int ring, wgs_per_cu; };
constexpr StreamLds stream_lds(CfgShape c, int RT, bool sym, bool track, int tv, int bands, size_t inherited, int want, int min_ring = 4) {
    const size_t fixed = stream_layout(c, RT, sym, track, tv, bands, 0).bytes + inherited;
    const size_t slots = stream_layout(c, RT, sym, track, tv, bands, 1).bytes + inherited - fixed;     // one slot in every wave's ring
    for (;; --want) {
        const size_t budget = LDS_BYTES / (size_t)want;
        const int ring = budget > fixed ? min_of((int)((budget - fixed) / slots), RING_MAX) : 0;
        if (ring >= min_ring || want == 1) return {fixed + slots * (size_t)(ring < 1 ? 1 : ring), ring, want};
    }
}
// ---- control block of a call (ints, all zero when the call starts): CTRL_INTS counters and queue heads, then the
// order histograms and, from a 128-byte boundary, the ticket counters of the two sharded work queues (see QUEUE_SHARD_MAX_RT and
// order_bucket_kernel in sinkhorn_kernels.hpp).  A plan holds two (pilot_ot_plan::ctrl): an ordinary grid call works on one
// while the setup workgroups of its prep kernel zero the other for the call after it, so no call waits for a memset; the wide
// kernel's call and a call captured into a graph keep a memset and block 0 (see run_grid in pilot_ot_sinkhorn.hip).
constexpr int ORDER_NB = 48;
// the prep kernel computes the order keys in tiles of ORDER_RI selected rows x ORDER_JW columns, one workgroup each
constexpr int ORDER_JW = 128, ORDER_RI = 8;
constexpr long order_tile_count(int N, int n_rows) { return n_rows > 0 ? (long)((N + ORDER_JW - 1) / ORDER_JW) * ((n_rows + ORDER_RI - 1) / ORDER_RI) : 0; }
constexpr int QUEUE_SHARDS = 32, QUEUE_SHARD_STRIDE = 32;
enum : int {
    CTRL_TRACK_LEN = 0,          // length of track_list: the fast launch's hand-overs to the tracking launch
    CTRL_GENERIC_HEAD = 0,       // queue head of a POT-literal call of its own (run_generic without a list)
    CTRL_HEAD_FAST = 1,          // queue heads of the fast launch, the tracking launch and the solo waves
    CTRL_HEAD_TRACK = 2,
    CTRL_HEAD_SOLO = 3,
    CTRL_SPLIT = 4,              // CTRL_SPLIT_INTS ints written by order_scatter_kernel, each the number of leading exact duplicates;
    CTRL_SPLIT_INTS = 4,         //   the solo waves read the last one
    CTRL_SOLO_LEN = CTRL_SPLIT + 3,
    CTRL_FB_LEN = 8,             // length of the f64 fallback list (small reg, or pairs that left the f32 range) and its queue head
    CTRL_FB_HEAD = 9,
    CTRL_NAN_LEN = 10,           // length of the NaN list (pairs re-solved by the POT-literal kernel) and its queue head
    CTRL_NAN_HEAD = 11,
    CTRL_UNEQUAL = 12,           // set by the prep kernel when the rows of P do not all carry the same mass
    CTRL_INTS = 16,
    CTRL_ORDER_HIST = CTRL_INTS,                                              // 2 * ORDER_NB: histogram + scatter cursors
    CTRL_SHARDS_AT = (CTRL_ORDER_HIST + 2 * ORDER_NB + 31) / 32 * 32,         // QUEUE_SHARDS counters of the fast launch
    CTRL_SHARDS_TRACK_AT = CTRL_SHARDS_AT + QUEUE_SHARDS * QUEUE_SHARD_STRIDE,  // ... and of the tracking launch
    CTRL_BLOCK_INTS = CTRL_SHARDS_TRACK_AT + QUEUE_SHARDS * QUEUE_SHARD_STRIDE,
    CTRL_NONE = -1,              // (in a pass plan: no such slot, the kernel gets a null pointer)
};
// Bits of the PILOT_OT_DEBUG test switch (experiments and tests of the Sinkhorn grid call; tools/ and tests set the numbers)
enum : int {
    DBG_NATURAL_ORDER = 2,        // no longest-first work order, only the duplicates are told apart
    DBG_WGS_SHIFT = 4,            // bits 4..6: resident workgroups per CU of the fast launch (0: its own occupancy)
    DBG_NO_TAIL_ROWS = 256,       // the last row-tile on the MFMA path (no VALU tail-row variant)
    DBG_NO_SOLO = 512,            // exact duplicates in the tiles, no one-wave-per-pair path in the fast launch
    DBG_NO_NAN_PASS = 1024,       // no POT-literal pass for the pairs that end in NaN
    DBG_NO_SOLO_F64 = 2048,       // the f64 fallback pass on 16-pair tiles, not one wave per pair
    DBG_NO_REDO64 = 4096,         // single-band pairs that leave the f32 range go to the POT-literal pass, not the f64 one
    DBG_NO_TRACK_ALL = 8192,      // the fast pass runs first beyond max(M)/reg = 24 too
};
// The test switches that act inside the launch sequence of a Sinkhorn grid call: read once per call (pilot_ot_sinkhorn_grid_dev)
// and part of the graph-replay key, so a changed switch is captured anew, never replayed from the old sequence
struct SinkhornSwitches {
    int debug;          // PILOT_OT_DEBUG (DBG_* bits)
    int no_quad;        // PILOT_OT_NO_QUAD set: 112 < K <= 128 on the one-wave kernel
    int generic_wgs;    // PILOT_OT_GENERIC_WGS: fewer workgroups for the POT-literal kernel (0: unset)
    bool operator==(const SinkhornSwitches &o) const { return debug == o.debug && no_quad == o.no_quad && generic_wgs == o.generic_wgs; }
};

// ---- the passes of a grid call.  112 < K <= 128, symmetric cost: the fast pass of the fp16-split configuration runs four waves per tile (quad_kernels.hpp)
constexpr int QUAD_MIN_K = 113, QUAD_MAX_K = 128;
constexpr bool quad_covers(int K, bool sym) { return sym && K >= QUAD_MIN_K && K <= QUAD_MAX_K; }
// workgroups of a launch of WAVES_PER_WG tiles each: per_cu resident per CU, no more than the tiles fill
constexpr int clamp_wgs(int n_cu, int per_cu, int tiles) { return min_of(n_cu * per_cu, (tiles + WAVES_PER_WG - 1) / WAVES_PER_WG); }
enum PairList { LIST_ORDER, LIST_TRACK, LIST_FB };     // the plan's order_list, its track_list, the second half of its nan_list
struct PassPlan {
    bool run = false, track = false, quad = false, solo_f64 = false;           // tau-tracking; four waves per tile; one wave per pair (f64 pass)
    int cfg = 0, tv = 0, live1 = 0;       // the kernel variant: tv > 0 the VALU tail rows (plain configurations), live1 the split ones' K mod 16 in 1..4
    int bands = 1;                        // 2: the Gibbs kernel in two exponent bands (small reg)
    size_t inherited = 0;                 // bytes the launch reserves beyond its kernel's layout
    StreamLds lds = {};
    int wgs = 0, solo_blocks = 0;         // workgroups, of which the leading solo_blocks run solo_pairs
    PairList list = LIST_ORDER;           // the work list; control slots of its length (CTRL_NONE: every pair of the call), its queue head and
    int len_slot = CTRL_NONE, head_slot = CTRL_NONE, shards_at = CTRL_NONE;     //   the first ticket counter of its sharded queue (CTRL_NONE: one head)
};
struct GridPasses {
    int rc = PILOT_OT_OK;         // or PILOT_OT_ENOTSUP with msg: a pass this shape launches does not fit LDS (whatever n_rows)
    char msg[160] = "";
    int mode = 0, write_tail = 0, ob = 0;     // launch_prep's mode, write_tail and n_blocks
    PassPlan fast, track, f64;    // (the f32 passes append to f64.list what the f64 pass solves again)
};
// What a grid call launches.  cfg: the configuration of the fast pass; CFG_H32 (fp16-split) tracks on the bf16-split kernel.
// mixed (cfg == CFG_S32 only): small reg under PILOT_OT_PREC_AUTO -- every pair is first iterated in f32 (two-band tracking kernel); pairs whose
// plan may touch Gibbs entries outside the f32-safe range, or that went NaN, are collected (ring_flush) and solved again by the f64 tracking kernel.
inline GridPasses plan_grid(int cfg, int N, int K, int n_rows, bool sym, bool mixed, double max_cost_over_reg, int n_cu, const SinkhornSwitches &sw) {
    GridPasses g;
    const CfgShape fast = shape_of(cfg);
    const bool half = fast.half, split = fast.split;
    const int TILE = 16, RT = (K + TILE - 1) / TILE, n_tail = K - (RT - 1) * TILE, debug = sw.debug;
    // split: skip the dead registers of the last tile (beyond 4 row-tiles those variants run out of registers and spill
    // 600-980 B per lane; the plain variants do not, and measure the same there)
    const int live1 = (split && RT >= 2 && RT <= 4 && n_tail <= 4) ? 1 : 0;
    // K mod 16 in 1..4: the (at most four) cell types of the last row-tile are computed on the VALU (tail_rows)
    // (RT = 8 variants spill: left on the MFMA path; so is a shape without room for the weights next to a ring of four)
    int tv = (!split && RT >= 2 && RT <= 7 && n_tail <= 4 && !(debug & DBG_NO_TAIL_ROWS)) ? (n_tail <= 2 ? 1 : 2) : 0;
    if (tv && stream_layout(fast, RT, sym, false, tv, 1, 4).bytes > LDS_BYTES) tv = 0;
    // Between the fp16-split range and the two-band path (12 < max(M)/reg <= 60) a few pairs per matrix leave the f32 range in
    // the single-band kernels (a scaling jumps past the fp16 domain within one update; products underflow at reg <= 0.025).
    // They used to go to the POT-literal kernel with the other NaN pairs -- one workgroup per pair, 12.5 us per update: 3 to 13
    // pairs cost 12 ms of a 30 ms call at reg 0.025 .. 0.0175.  They are collected like the small-reg path collects its
    // hand-over and solved again by the f64 tracking kernel (symmetric cost, K <= 64: one wave per pair, 1.1 us per update).
    const bool redo64 = !mixed && split && max_cost_over_reg > 12.0 && !(debug & DBG_NO_REDO64);
    // From max(M)/reg = 24 on nearly every pair tau-absorbs (c3: 28 % at 20, 94 % at 25) and the fast pass only hands its pairs
    // over after a few dozen wasted updates (3.7 of 11.6 ms at reg 0.04): every pair goes to the tracking kernel at once, as
    // in the two-band path.
    const bool track_all = mixed || (split && !half && max_cost_over_reg > 24.0 && !(debug & DBG_NO_TRACK_ALL));
    // exact duplicates (a == b): one wave per pair in the leading workgroups of the fast launch (symmetric cost, K <= 64)
    // ... while the grid is small.  A wave that iterates ONE pair has the shorter update (K = 50: 0.57 us against 0.77 us for a lone
    // 16-pair wave), which is what a launch with fewer tiles than wave slots waits for (c2; the row shards of a multi-device call);
    // on a full device the 600 diagonal pairs of c3 (165 updates on average, up to 301) on 600 waves of their own are a tail instead:
    // main kernel 0.617 -> 0.584 ms with the duplicates in the tiles (tools/solo_probe.py; crossover between 5 600 and 7 500 tiles at 2 048
    // wave slots).  The rule reads the FULL grid (N x N), not the rows of this call: a row shard and the full grid send the same pair
    // down the same path, so their bits agree.
    // (the shape rules read the configuration as its fast pass is instantiated: the split variants with live1 as their TV)
    const int tv_fast = split ? live1 : tv;
    const long full_tiles = ((long)N * N + TILE - 1) / TILE, wave_slots = (long)n_cu * min_waves_per_simd(fast, RT, sym, false, tv_fast) * WAVES_PER_WG;
    const bool solo = solo_in_stream(fast, RT, sym, false, tv_fast) && !(debug & DBG_NO_SOLO) && !track_all && full_tiles < 3 * wave_slots;
    const int n_pairs = n_rows * N, tiles = (n_pairs + TILE - 1) / TILE;
    // first pass: throughput kernel (pairs that would tau-absorb are handed to the second pass)
    PassPlan &f = g.fast, &t = g.track, &d = g.f64;
    f.run = !track_all; f.cfg = cfg; f.tv = tv; f.live1 = live1; f.quad = half && quad_covers(K, sym) && !sw.no_quad;  f.head_slot = CTRL_HEAD_FAST; f.shards_at = CTRL_SHARDS_AT;
    // second pass: pairs in which POT would tau-absorb (track_all: EVERY pair, longest first), with the absorption iterations tracked.
    // The split configurations track on the bf16-split kernel; larger tracking variants spill with the tail rows.
    // (its result need not match the fast kernels' bits: a pair is always solved by one of them)
    t.run = t.track = true; t.cfg = split ? (int)CFG_S32 : cfg; t.tv = RT <= 4 ? tv : 0; t.live1 = live1; t.bands = mixed ? 2 : 1;
    t.head_slot = CTRL_HEAD_TRACK; t.shards_at = CTRL_SHARDS_TRACK_AT; if (!track_all) { t.list = LIST_TRACK; t.len_slot = CTRL_TRACK_LEN; }
    const CfgShape tracking = shape_of(t.cfg);
    // inherited: the tracking launch keeps the fast pass's hand-over buffers, which it never fills, and its tail-weight bytes, which
    // it reads only with the same tv; both decide its ring and its resident workgroups
    t.inherited = ((size_t)handover_elems(tracking) + tail_weight_elems(tracking, RT, sym, tv) - tail_weight_elems(tracking, RT, sym, t.tv)) * 4 * tracking.w;
    // third pass: the collected pairs in f64 (operand images and proportions rebuilt for f64 in the same buffers -- the f32 passes are complete in
    // stream order; no ordering, the list is short: tens of pairs, and every one runs long, so one wave per pair where solo_pairs covers the shape)
    d.run = mixed || redo64; d.track = true; d.cfg = CFG_F64; d.solo_f64 = sym && K <= 64 && !(debug & DBG_NO_SOLO_F64);
    d.list = mixed ? LIST_TRACK : LIST_FB; d.len_slot = CTRL_FB_LEN; d.head_slot = CTRL_FB_HEAD;
    g.rc = PILOT_OT_ENOTSUP;      // (until every pass is found to fit)
    t.lds = stream_lds(tracking, RT, sym, true, t.tv, t.bands, t.inherited, min_waves_per_simd(tracking, RT, sym, true, split ? live1 : t.tv));
    if (!t.lds.ring) { snprintf(g.msg, sizeof g.msg, "K=%d with a %ssymmetric cost needs %zu B of LDS (> %zu) in this precision", K, sym ? "" : "non-", t.lds.bytes, LDS_BYTES); return g; }
    if (f.run && !f.quad) {
        int want = min_waves_per_simd(fast, RT, sym, false, tv_fast);
        // (K <= 4: a third of the pairs tau-absorb and are handed over, and the hand-over's atomics and list stores are what more resident
        // waves contend for -- K = 3 / 4 at N = 600: 0.60 / 0.64 ms at two workgroups per CU, 0.69 / 0.72 at four; from K = 5 on four win)
        if (half && K <= 4 && want > 2) want = 2;
        if ((debug >> DBG_WGS_SHIFT) & 7) want = (debug >> DBG_WGS_SHIFT) & 7;      // experiment: resident workgroups per CU
        f.lds = stream_lds(fast, RT, sym, false, tv, 1, 0, want);
        if (!f.lds.ring) { snprintf(g.msg, sizeof g.msg, "K=%d: operand images + ring + park area exceed LDS", K); return g; }
    }
    if (d.run && !d.solo_f64) {
        d.lds = stream_lds(shape_of(CFG_F64), RT, sym, true, 0, 1, 0, min_waves_per_simd(shape_of(CFG_F64), RT, sym, true, 0));
        if (!d.lds.ring) { snprintf(g.msg, sizeof g.msg, "K=%d: the f64 fallback needs %zu B of LDS", K, d.lds.bytes); return g; }
    }
    g.rc = PILOT_OT_OK;
    if (n_rows == 0) { f.run = t.run = d.run = false; return g; }
    // longest-first work order (see order_bucket_kernel)
    g.ob = min_of((n_pairs + 1023) / 1024, n_cu);
    g.mode = (solo ? 2 : 0) | ((debug & DBG_NATURAL_ORDER) ? 4 : 0);   // bit 1: solo duplicates, bit 2: natural order (experiment)
    g.write_tail = (tv ? 1 : 0) | 2 | (mixed ? 4 : 0);
    if (solo) f.solo_blocks = min_of((n_rows + WAVES_PER_WG - 1) / WAVES_PER_WG, n_cu);     // the diagonal; more duplicates queue up
    // (quad: one tile per workgroup, two workgroups per CU)
    f.wgs = f.quad ? min_of(2 * n_cu, tiles) : clamp_wgs(n_cu, f.lds.wgs_per_cu, tiles) + f.solo_blocks;
    t.wgs = clamp_wgs(n_cu, t.lds.wgs_per_cu, tiles);
    d.wgs = d.solo_f64 ? 64 : clamp_wgs(n_cu, d.lds.wgs_per_cu, tiles);
    return g;
}

}  // namespace pilot
