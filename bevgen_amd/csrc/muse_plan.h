// How a Route M forward (muse.cpp) launches its projections, as pure functions of (shape, switches, which workspaces exist): no HIP runtime call, no environment read,
// no heap.  Exercised on the CPU (tests/test_muse_plan_cpu.py through tests/host/muse_plan_dump.cpp); the driver that executes the decisions is muse.cpp.
#pragma once
#include "gemm_plan.h"

namespace bevgen {

// Route M's A/B switches, one environment variable each (muse_switches() in muse.cpp fills the struct; the table is in DESIGN.md).  ln_fold and ln_merge are read per
// forward - the tests switch them inside one process - the other four once per process.
struct MuseSwitches {
    int ln_fold = 1;       // $BEVGEN_LN_FOLD: 0 | 1 | 2, muse_fold_level
    int ln_merge = -1;     // $BEVGEN_LN_MERGE: -1 unset (by batch size), 0 = kernel, 1 = tile, muse_tile_merge
    int qkv_merge = 1;     // $BEVGEN_QKV_MERGE: 0 never, 3 only up to 3072 token rows, muse_qkv_merged
    int qkv_wm4 = 1;       // $BEVGEN_QKV_WM4: 0 = the merged q|k|v projection does not pin 256-row blocks, muse_proj_plan
    int ksplit = 0;        // $BEVGEN_KSPLIT: > 0 pins the k slices of the narrow projections, pick_ksplit
    int attn_ksplit = 0;   // $BEVGEN_ATTN_KSPLIT: > 0 pins the key ranges of the self-attention, pick_attn_ksplit
};

// LayerNorm folded across the GEMMs around it (GemmArgs::ln_*; needs the fold constants of bevgen_finalize: split-precision mode with fp32 weights).
//   0  the LayerNorm kernels of rounds 1-5 everywhere
//   1  (default) the feed-forward's INNER LayerNorm (over F = 2730 columns, the widest pass: 3.3 % of the sixteen-scene step) disappears: the GEGLU epilogue writes raw
//      planes + per-32-column row sums INSTEAD of its fp32 result (no extra bytes), a one-thread-per-row kernel merges the sums (8 bytes read per 32 elements), the
//      down-projection multiplies by W4 o gamma and applies rstd (acc - mean cs)
//   2  all four LayerNorms of a layer (the residual-stream projections then write planes + sums BESIDES their fp32 row)
// Measured, same box, scenes/s at 16 / 2 / 1 scenes per call (profiles/r06_ab_ln_fold.txt): level 0 10.29 / 7.88 / 6.04, level 1 **10.53 / 7.98 / 6.06**, level 2 10.10 / 7.85 /
// 5.95 - the extra plane stores of the residual-stream epilogues cost more than the LayerNorm passes they replace (round 3 found the same with another design), at
// every batch size; level 2 stays as a tested switch.  $BEVGEN_LN_FOLD pins the level (A/B runs, tests).
// (Round 3 built a first LayerNorm fold - producers wrote (row x gamma) planes + per-group (mean, M2), a merge kernel per LayerNorm - token-exact and SLOWER, 10.12 ->
// 9.86 scenes/s, profiles/r03_ab_ln_fold.txt; removed in round 4.  Round 6's form has no merge launch - the consumer adds the group sums itself, in the shadow of its
// first DMA - no gamma in the producer (it sits in W o gamma), and the inner LayerNorm's producer writes planes INSTEAD of its fp32 result.)
inline int muse_fold_level(const MuseSwitches& sw, bool has_fold_constants) { return has_fold_constants ? std::max(0, std::min(sw.ln_fold, 2)) : 0; }

// Who merges a folded LayerNorm's group sums: up to two scenes every workgroup of the consuming projection runs ONE tile and merges its rows itself (no launch between
// producer and consumer: at one scene a 9 us kernel + its ramp per LayerNorm); above that one finalize kernel per LayerNorm feeds all tiles ($BEVGEN_LN_MERGE = kernel | tile)
inline bool muse_tile_merge(const MuseSwitches& sw, long rows) { return sw.ln_merge >= 0 ? sw.ln_merge == 1 : rows <= 3072; }

// to_q and to_kv of the self-attention read the same LayerNorm planes (muse_net:126-132): ONE projection over the concatenated weight, query / key / value preparation in
// its epilogue ($BEVGEN_QKV_MERGE=0: the two launches of rounds 2-4, for A/B runs)
// Measured, round 5 (profiles/r05_ab_qkv_merge*.txt): one scene 161.9 -> 160.4 ms, sixteen scenes 10.31 -> 10.21 scenes/s - merged only on the low-latency path then.
// Round 6, after the staged row-major epilogues and with the row-split rest choosing its own block shape (profiles/r06_ab_qkv_merge.txt, same box, ms per step
// separate -> merged): three scenes 387.0 -> 373.5 (+3.6 %), four 443.7 -> 437.2, six 614.0 -> 607.1, eight 771.0 -> 768.7, twelve 1122.0 -> 1108.7 (+1.2 %),
// sixteen 1424.0 -> 1422.2: merged at every batch size.  $BEVGEN_QKV_MERGE = 0 never, 3 only up to 3072 token rows (the round-5 rule; A/B runs)
inline bool muse_qkv_merged(const MuseSwitches& sw, long rows) { return sw.qkv_merge != 0 && (sw.qkv_merge != 3 || rows <= 3072); }

// Low-latency path (one or two scenes per call, scripts/interactive_editing.py:273-277): a [rows, D] x [D, D] projection is only cdiv(rows, 128) * D / 128 tiles -
// 96 workgroups at one six-view scene, on 256 CUs.  Its k range is cut into slices until the grid covers the chip; the slices' partial tiles are added in a fixed
// order (tokens stay identical run to run, and identical to the unsplit path up to fp32 summation order - checked against the B = 16 path in the tests).
// How many slices (measured at one six-view scene, rows = 1536, tools/gemm_small_probe.py + profiles/r03_gemm_small_*.txt): with the eight-wave small-problem block of
// gemm_split_glds.hip a [1536, 1024] x [1024, K] projection costs 7.6 us of fixed time (dispatch, pipeline fill from cold operands, store tail) + 0.43 us per k-tile
// on 96 CUs.  A second slice halves the loop but adds a 6.4 us reduce launch and gives up the fused epilogues (q preparation): a wash at K = 1024 (21.4 vs 20.9 us),
// a clear gain for a long k loop (K = 5504: 82 -> 51 us).  So: two slices from K = 2048 up, none below - and none where the 128-row grid covers at most half of the CUs:
// there the launcher's 64-row blocks double the grid without a reduce launch (one-scene down-projection, K = 2752: 37.9 + 7.1 -> 40 us; step 169.9 -> 167.9 ms).  (Round-3 history: with the four-wave
// block - 12 us + 0.62 us per k-tile - two slices everywhere were the optimum, step 257 -> 241 ms.)  $BEVGEN_KSPLIT pins the slices (A/B runs, tests).
constexpr int kMuseKsplitMax = 6;   // the split-K workspace (kpart) holds this many slices of [rows, D]
inline int pick_ksplit(long rows, int N, int K, int ksplit_switch) {
    if ((long)cdiv(rows, 256) * cdiv(N, 128) >= 256) return 1;          // the 256-row tiling already fills the chip
    const long tiles = (long)cdiv(rows, 128) * cdiv(N, 128);
    if (tiles >= 160) return 1;
    int s = (K >= 2048 && tiles > 128) ? 2 : 1;   // (<= 128 tiles: the launcher's 64-row blocks already double the grid, without a reduce: 45 -> 40 us at K = 2752)
    if (ksplit_switch > 0) s = std::min(kMuseKsplitMax, ksplit_switch);
    while (s > 1 && K / 32 < 2 * s) --s;
    return s;
}
// does a call of `rows` token rows carve the split-K workspace?  (its two narrow projection shapes: K = D and K = Fpad)
inline bool muse_needs_kpart(long rows, int D, int Fpad, const MuseSwitches& sw) { return std::max(pick_ksplit(rows, D, D, sw.ksplit), pick_ksplit(rows, D, Fpad, sw.ksplit)) > 1; }

// Key ranges of the self-attention (same low-latency path): one scene is cdiv(1536, 256) * 16 heads = 96 workgroups on 256 CUs, each walking all 49 key tiles;
// with the keys cut in two, 192 workgroups walk half of them and a combine kernel merges the pairs.  Only when the ranges stay long (>= 8 tiles each) and the
// grid leaves at least half of the CUs idle.  $BEVGEN_ATTN_KSPLIT pins it (A/B runs, tests).
inline int pick_attn_ksplit(long blocks, int ntiles, int attn_ksplit_switch) {
    if (attn_ksplit_switch > 0) return std::max(1, std::min(std::min(attn_ksplit_switch, 8), ntiles));
    if (blocks * 2 > 256) return 1;
    const int ks = std::min(std::min(4, (int)(256 / blocks)), ntiles / 8);
    return std::max(ks, 1);
}

// batches up to this many token rows carry a stream-K workspace in split-precision mode, whatever $BEVGEN_GEMM_SK says (glds_sk_pays decides per projection)
constexpr long kMuseSkMaxRows = 8192;

// The LDS-DMA projections of the split path and how each is launched.  "stream-K asked": the launch carries the stream-K workspace and a new epoch IF the call has such
// a workspace - but the ask alone already suppresses split-K.  (The launcher takes the stream-K form only with $BEVGEN_GEMM_SK set: gemm_plan.h.)
//
//   projection                                | stream-K asked when                | split-K when                                                          | otherwise
//   PROJ_OUT    to_out x 2, down-projection   | glds_sk_pays(M, N)                 | kpart exists, N <= 1024, no fold role (producer or consumer), stream-K | fused epilogue, one launch
//                                             |                                    | not asked: ksplit = pick_ksplit                                       |
//   PROJ_Q      q (self un-merged, cross)     | glds_sk_pays(B Nq, H 64)           | no fold role, stream-K not asked, kpart exists, H 64 <= 1024,          | EPI_MUSE_Q
//                                             |                                    | pick_ksplit > 1: UN-FUSED projection into qraw with split-K (and no    |
//                                             |                                    | stream-K), then launch_muse_q_prep_split                              |
//   PROJ_KV     k|v, q|k|v                    | glds_sk_pays(rows, N)              | never                                                                 | fused epilogue; force_wm = 4 when merged and $BEVGEN_QKV_WM4
//   PROJ_GEGLU  GEGLU up-projection           | glds_sk_pays(rows, 2 Fpad)         | never                                                                 | EPI_GEGLU (+ fold roles)
//   PROJ_UP     up-projection without the     | never                              | never                                                                 | plain
//               GEGLU weight order            |                                    |                                                                       |
//
// (a folded projection keeps its epilogue: the split-K reduce kernel has none of it; stream-K keeps the fused epilogue and needs no reduce launch)
enum MuseProj { PROJ_OUT = 0, PROJ_Q = 1, PROJ_KV = 2, PROJ_GEGLU = 3, PROJ_UP = 4 };
struct MuseProjIn {
    MuseProj kind = PROJ_UP;
    long M = 0; int N = 0, K = 0;
    bool fold_role = false;    // the launch is producer or consumer of a folded LayerNorm
    bool merged = false;       // PROJ_KV: the q|k|v form
    bool has_kpart = false;    // the call carved a split-K workspace (muse_needs_kpart)
    bool has_sk_ws = false;    // the call carved a stream-K workspace
};
struct MuseProjPlan {
    bool sk_asked = false;     // (suppresses split-K with or without a workspace)
    bool sk = false;           // the launch carries the stream-K workspace and advances its epoch
    bool kpart = false;        // the launch is handed the split-K workspace, with `ksplit` slices (1 = the launcher's single-slice forms)
    int ksplit = 1;
    bool q_unfused = false;    // PROJ_Q: plain projection into qraw + launch_muse_q_prep_split
    int force_wm = 0;          // one scene: 144 blocks of 256 x 128 (one per CU, the staged row-major epilogue) against 288 of 128 x 128 sharing CUs in pairs on a two-stage ring
};                             // (one scene 158.9 -> 153.8 ms, profiles/r06_ab_b1_qkv_wm4.txt; $BEVGEN_QKV_WM4 = 0: A/B runs)
inline MuseProjPlan muse_proj_plan(const MuseProjIn& in, const MuseSwitches& sw, const GldsSwitches& gsw) {
    MuseProjPlan p;
    if (in.kind == PROJ_UP) return p;
    p.sk_asked = glds_sk_pays(gsw, in.M, in.N);
    p.sk = p.sk_asked && in.has_sk_ws;
    const bool may_split = in.has_kpart && in.N <= 1024 && !in.fold_role && !p.sk_asked;
    if (in.kind == PROJ_OUT && may_split) {
        p.kpart = true;
        p.ksplit = pick_ksplit(in.M, in.N, in.K, sw.ksplit);
    }
    if (in.kind == PROJ_Q && may_split && pick_ksplit(in.M, in.N, in.K, sw.ksplit) > 1) {
        p.q_unfused = p.kpart = true;
        p.ksplit = pick_ksplit(in.M, in.N, in.K, sw.ksplit);
    }
    if (in.kind == PROJ_KV && in.merged && sw.qkv_wm4) p.force_wm = 4;
    return p;
}

}  // namespace bevgen
