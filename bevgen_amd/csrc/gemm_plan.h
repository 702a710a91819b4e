// Launch plan of the LDS-DMA GEMM (gemm_split_glds.hip): which instantiation runs a problem, on which grid, with how much LDS - as a pure function of
// (GemmArgs, switches, CU count).  No HIP runtime call, no environment read, no heap: the function runs once per GEMM / convolution launch and is exercised on the CPU
// (tests/test_gemm_plan_cpu.py through tests/host/gemm_plan_dump.cpp).  The kernels and the driver that executes a plan are in gemm_split_glds.hip.
#pragma once
#include "common.h"
#include "kernels.h"
#include "profiler.h"
#include <algorithm>

namespace bevgen {

// the 'same' defaults of a 3x3 convolution (GemmArgs: 0 / -1 = derive): stride 1, pad 1, stored input = output size, or half of it behind a fused 2x upsample
inline GemmArgs conv_defaults(const GemmArgs& g0) {
    GemmArgs g = g0;
    if (g.mode == MODE_CONV3) {
        if (g.conv_stride == 0) g.conv_stride = 1;
        if (g.conv_pad < 0) g.conv_pad = 1;
        if (g.conv_hin == 0) g.conv_hin = g.conv_up ? g.conv_h / 2 : g.conv_h;
        if (g.conv_win == 0) g.conv_win = g.conv_up ? g.conv_w / 2 : g.conv_w;
    }
    return g;
}

// The launcher's A/B switches, one environment variable each (glds_switches() in gemm_split_glds.hip reads them once per process; the table is in DESIGN.md)
struct GldsSwitches { int sk = 0, rpf = 1, rme = 1, band = 0, wm = 0, top_wm = 4, rowsplit = 1, bot_wm = 0, stages = 0, conv_thin = 1, half8 = 1, conv_fast = 1; };
// names one instantiation: gemm_split_glds_kernel<MODE, WM, S, W16, KS, TI, TJ>, or with sk gemm_split_glds_sk_kernel<WM, S, W16>
struct GldsVariant { int mode, wm, s; bool w16, ks; int ti, tj; bool sk; };
// g: as the kernel receives it (g.M = END row of this launch, g.m_base its first); reduce_after: split-K, launch_splitk_reduce follows
struct GldsLaunch { GemmArgs g; GldsVariant v; dim3 grid; int threads; size_t lds; int prof_kind; double work; bool reduce_after; };
struct GldsPlan { int n; GldsLaunch l[2]; };   // 2 = a row-split problem

// THE list of instantiations, X(MODE, WM, S, W16, KS, TI, TJ, SK): the stream-K kernel x W16, then 13 tuples x W16.  The kernel table, the per-device LDS opt-in and the
// launch (gemm_split_glds.hip) all expand this one list; a plan that names a tuple outside it is refused.
#define BG_GLDS_VARIANTS(X)                                                                                                                           \
    X(MODE_PLAIN, 4, 3, false, false, 2, 2, true) X(MODE_PLAIN, 4, 3, true, false, 2, 2, true)                                                        \
    X(MODE_PLAIN, 2, 2, false, false, 2, 2, false) X(MODE_CONV3, 2, 2, false, false, 2, 2, false) X(MODE_CONV3S, 2, 2, false, false, 2, 2, false)     \
    X(MODE_PLAIN, 4, 3, false, false, 2, 2, false) X(MODE_CONV3, 4, 3, false, false, 2, 2, false) X(MODE_CONV3S, 4, 3, false, false, 2, 2, false)     \
    X(MODE_PLAIN, 2, 2, true, false, 2, 2, false) X(MODE_CONV3, 2, 2, true, false, 2, 2, false) X(MODE_CONV3S, 2, 2, true, false, 2, 2, false)        \
    X(MODE_PLAIN, 4, 3, true, false, 2, 2, false) X(MODE_CONV3, 4, 3, true, false, 2, 2, false) X(MODE_CONV3S, 4, 3, true, false, 2, 2, false)        \
    X(MODE_PLAIN, 2, 2, false, true, 2, 2, false) X(MODE_PLAIN, 2, 2, true, true, 2, 2, false)                                                        \
    X(MODE_PLAIN, 2, 4, false, false, 1, 2, false) X(MODE_PLAIN, 2, 4, true, false, 1, 2, false)                                                      \
    X(MODE_PLAIN, 2, 4, false, true, 1, 2, false) X(MODE_PLAIN, 2, 4, true, true, 1, 2, false)                                                        \
    X(MODE_CONV3, 2, 4, false, false, 1, 2, false) X(MODE_CONV3S, 2, 4, false, false, 1, 2, false)                                                    \
    X(MODE_CONV3, 2, 4, true, false, 1, 2, false) X(MODE_CONV3S, 2, 4, true, false, 1, 2, false)                                                      \
    X(MODE_PLAIN, 1, 4, false, false, 1, 2, false) X(MODE_PLAIN, 1, 4, true, false, 1, 2, false)                                                      \
    X(MODE_PLAIN, 1, 4, false, false, 1, 1, false) X(MODE_PLAIN, 1, 4, true, false, 1, 1, false)
#define BG_GLDS_TUPLE(...) GldsVariant{__VA_ARGS__},
constexpr GldsVariant kGldsVariants[] = {BG_GLDS_VARIANTS(BG_GLDS_TUPLE)};
#undef BG_GLDS_TUPLE
constexpr int kGldsVariantCount = (int)(sizeof(kGldsVariants) / sizeof(kGldsVariants[0]));
inline int glds_variant_index(const GldsVariant& v) {   // -1: not an instantiation
    for (int i = 0; i < kGldsVariantCount; ++i) {
        const GldsVariant& t = kGldsVariants[i];
        if (t.mode == v.mode && t.wm == v.wm && t.s == v.s && t.w16 == v.w16 && t.ks == v.ks && t.ti == v.ti && t.tj == v.tj && t.sk == v.sk) return i;
    }
    return -1;
}

// Quantities the kernels fix, each written once (gemm_split_glds.hip asserts that the tile constants are its own)
constexpr int kGldsBN = 128, kGldsBK = 32;   // block columns, k-tile
constexpr size_t kGldsLdsSlots = 4096, kGldsLdsSums = 2048, kGldsLdsMerge = 8192;   // LayerNorm (mean, rstd) slots | prefetch sink; prefetch | group sums; the block merge's fp64 partial sums
constexpr int glds_threads(const GldsVariant& v) { return v.wm * 512 / (v.ti * v.tj); }   // the kernels' __launch_bounds__
constexpr size_t glds_ring_bytes(const GldsVariant& v) { return (size_t)v.s * (v.wm * 64 + kGldsBN) * 2 * kGldsBK * 2; }   // S stages of (block rows + 128) lines of (32 hi | 32 lo) halves
// the dynamic-LDS maximum a variant is opted in to, once per device: the ring plus every extra for the plain mode (the stream-K kernel: the slots only), the ring alone for the convolutions
constexpr size_t glds_lds_max(const GldsVariant& v) {
    return glds_ring_bytes(v) + (v.sk ? kGldsLdsSlots : v.mode == MODE_PLAIN ? kGldsLdsSlots + kGldsLdsSums + kGldsLdsMerge : 0);
}

// Does the stream-K form pay?  T tiles of 256 x 128 cost ceil(T / 256) rounds of the chip; the form removes the empty part of the last round (and the second launch of a
// row-split problem) at the price of one partial-tile exchange per workgroup (~3 us) - worth it when at least 15 % of the rounds would be empty and every workgroup still
// gets a few k-tiles.  One scene (rows 1536): q|k|v 144 tiles (44 % empty), the 1024-wide projections 48 (81 %), the up-projection 258 (50 % of two rounds); two scenes:
// 288 / 96 / 516; sixteen scenes: 2304 = 9 rounds exactly, 768 = 3, 4128 = 16.1 (its row-split form stays).
inline bool glds_sk_pays(const GldsSwitches& sw, long rows, int N) {
    if (!sw.sk) return false;   // (default off: see glds_plan_range)
    const long T = (long)cdiv(rows, 256) * cdiv(N, kGldsBN), rounds = (T + 255) / 256;
    const double empty = 1.0 - (double)T / (double)(rounds * 256);
    // ... and only while a tile is shared by two or three workgroups (T >= 128): with fewer tiles every tile's last workgroup merges five or more 128 KiB partials while
    // the others idle - measured slower than the 64-row blocks of the data-parallel launch at every such shape (profiles/r06_ab_gemm_sk_ops.txt)
    return T >= 128 && empty >= 0.15;
}

// One row range [g.m_base, g.M) of a problem -> its launch.  Where the range should be cut in two (row split), *cut receives the cut row and the result is not used.
inline GldsLaunch glds_plan_range(const GemmArgs& g_in, const GldsSwitches& sw, int cus, bool (*xcd_ok)(), int* cut) {
    GldsLaunch L{};
    GemmArgs& g = L.g;
    const auto emit = [&L](const GldsVariant& v, dim3 grid, size_t lds, int prof_kind, double work) {
        L.v = v; L.grid = grid; L.threads = glds_threads(v); L.lds = lds; L.prof_kind = prof_kind; L.work = work; L.reduce_after = L.g.ksplit > 1;
    };
    g = conv_defaults(g_in);
    if (g.mode == MODE_CONV3) {
        BG_REQUIRE(g.conv_cin % kGldsBK == 0 && g.K == 9 * g.conv_cin, "conv3x3: Cin=%d must be a multiple of 32", g.conv_cin);
        const long a_bytes = (long)(g.M / (g.conv_h * g.conv_w)) * g.conv_hin * g.conv_win * g.conv_cin * 4;
        BG_REQUIRE(a_bytes < 0xFFFFFF00L, "conv3x3 (LDS-DMA): the activation planes (%ld bytes) must stay below 4 GiB per launch", a_bytes);
        g.a_bytes = (int)(unsigned)a_bytes;
    }
    BG_REQUIRE(g.A_hi && g.A_lo && g.B_hi && g.B_lo, "gemm_split_glds: both operands must be pre-split");
    g.row_major_epi = sw.rme != 0;
    g.r_prefetch = sw.rpf && g.mode == MODE_PLAIN && g.R && (g.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(g.R) & 15) == 0 && (long)g.M * g.ldr * 4 < 0x7FFFFFFFL && g.N >= 64;
    if (g.gn_part)
        BG_REQUIRE(g.mode == MODE_CONV3 && g.epi == 0 && g.ksplit <= 1 && g.M % 256 == 0 && g.m_base == 0 && g.N % kGldsBN == 0 && g.ldc == g.N && (g.ldc & 3) == 0 &&
                       (!g.R || (g.ldr & 3) == 0) && (reinterpret_cast<uintptr_t>(g.C) & 15) == 0 && (!g.R || (reinterpret_cast<uintptr_t>(g.R) & 15) == 0) && !g.bias_m,
                   "gemm_split_glds: GroupNorm partials need whole 256 x 128 tiles of a convolution with the plain epilogue (M=%d N=%d)", g.M, g.N);
    BG_REQUIRE(g.K % kGldsBK == 0 && g.lda % kGldsBK == 0 && g.ldb % kGldsBK == 0, "gemm_split_glds: K, lda, ldb must be multiples of 32 (K=%d lda=%d ldb=%d)", g.K, g.lda, g.ldb);
    BG_REQUIRE(g.batch == 1, "gemm_split_glds: batched form not provided");
    if (g.epi == EPI_MUSE_KV)
        BG_REQUIRE(g.mode == MODE_PLAIN && g.N == 2 * g.epi_heads * 64 && g.epi_hi && g.epi_lo && g.epi_hi2 && g.epi_lo2 && g.epi_aux && g.epi_scale && g.epi_rows > 0 &&
                       g.epi_ld >= g.epi_rows + 1 && !g.R && !g.bias_n && !g.bias_m && g.act == ACT_NONE && (g.no_row_split || g.M % g.epi_rows == 0),
                   "gemm_split_glds: bad fused k/v-preparation arguments");
    if (g.epi == EPI_GEGLU)
        BG_REQUIRE(g.mode == MODE_PLAIN && g.N % kGldsBN == 0 && (g.ldc % 4 == 0 && g.ldc >= g.N / 2) && !g.R && !g.bias_n && !g.bias_m && g.act == ACT_NONE,
                   "gemm_split_glds: bad fused GEGLU arguments (N=%d ldc=%d)", g.N, g.ldc);
    if (g.epi == EPI_MUSE_QKV)
        BG_REQUIRE(g.mode == MODE_PLAIN && g.N == 3 * g.epi_heads * 64 && g.epi_hi && g.epi_lo && g.epi_hi2 && g.epi_lo2 && g.epi_aux && g.epi_scale && g.epi_qh && g.epi_ql &&
                       g.epi_qscale && g.epi_rows > 0 && g.epi_ld >= g.epi_rows + 1 && !g.R && !g.bias_n && !g.bias_m && g.act == ACT_NONE &&
                       (g.no_row_split || g.M % g.epi_rows == 0) && g.ksplit <= 1,
                   "gemm_split_glds: bad fused q/k/v-preparation arguments");
    if (g.epi == EPI_MUSE_Q)
        BG_REQUIRE(g.mode == MODE_PLAIN && g.N % 64 == 0 && g.epi_hi && g.epi_lo && g.epi_scale && g.epi_rows > 0 && g.epi_heads * 64 == g.N && !g.R && !g.bias_n && !g.bias_m,
                   "gemm_split_glds: bad fused q-preparation arguments");
    if (g.ln_in_stats || g.ln_in_gsums)
        BG_REQUIRE(g.mode == MODE_PLAIN && g.ln_in_cs && g.N % 4 == 0 && g.ksplit <= 1 && !(g.ln_in_stats && g.ln_in_gsums) &&
                       (!g.ln_in_gsums || (g.ln_in_groups > 0 && g.ln_in_count > 0 && g.ln_rows >= g.M)),
                   "gemm_split_glds: bad folded-LayerNorm consumer arguments (N=%d ksplit=%d groups=%d)", g.N, g.ksplit, g.ln_in_groups);
    if (g.ln_out_planes)
        BG_REQUIRE(g.mode == MODE_PLAIN && g.ln_out_stats && g.ln_rows >= g.M && g.ln_out_ld % 32 == 0 && g.ksplit <= 1 &&
                       (g.epi == EPI_GEGLU ? g.ln_out_ld * 2 >= g.N : (g.epi == 0 && g.ln_out_ld >= g.N && g.N % 32 == 0 && (g.ldc & 3) == 0 && (!g.R || (g.ldr & 3) == 0) &&
                                                                        (reinterpret_cast<uintptr_t>(g.C) & 15) == 0 && (!g.R || (reinterpret_cast<uintptr_t>(g.R) & 15) == 0))),
                   "gemm_split_glds: bad folded-LayerNorm producer arguments (ld=%d N=%d epi=%d)", g.ln_out_ld, g.N, g.epi);
    // ---- stream-K route (the caller provided a workspace: Route M's projections): problems whose 256 x 128 tiles would leave much of their last round of the chip empty
    // DEFAULT OFF: measured slower than the launcher's other choices at every Route-M shape of one, two and four scenes (profiles/r06_ab_gemm_sk_ops.txt: +4 .. +27 us per
    // projection; one scene 163.8 -> 168.5 ms with the routing rule below, 214 ms with every projection): a partial 256 x 128 tile is 128 KiB to publish and to read back,
    // every segment refills the three-stage ring, and the workgroup that holds a tile's last k range merges while its peers idle - together more than the empty part of
    // the last round they remove.  $BEVGEN_GEMM_SK=1 routes by glds_sk_pays, 2 takes the form whenever a workspace is given (the operator tests force it per call).
    // (xcd_ok launches a probe kernel on its first use per device: it is asked last, only when every other precondition holds)
    // (a single-product launch never takes it: the stream-K kernel has no single-product instantiation)
    if (g.sk_ws && (sw.sk || g.sk_force) && !g.a_hi_only && g.mode == MODE_PLAIN && g.ksplit <= 1 && g.m_base == 0 && !g.no_row_split && !g.bias_m && !g.ln_in_gsums && xcd_ok() &&
        (sw.sk == 2 || g.sk_force || glds_sk_pays(sw, g.M, g.N))) {
        g.sk_tiles = cdiv(g.M, 256) * cdiv(g.N, kGldsBN);
        const long units = (long)g.sk_tiles * (g.K / kGldsBK);
        const int G = (int)std::max<long>(8, std::min<long>(std::min(cus, 256), units / 2)) & ~7;   // (a multiple of 8: whole tiles per XCD; >= two k-tiles per workgroup; 256 slots)
        g.tile_band = 0;
        const GldsVariant v{MODE_PLAIN, 4, 3, g.b_lo_zero, false, 2, 2, true};
        emit(v, dim3(G), glds_lds_max(v), PROF_GEMM_SMALL, 2.0 * g.M * (double)g.N * g.K);
        return L;
    }
    g.tile_band = 4;   // band height of the XCD-aware tile order (measured optimum for 256 x 128 tiles)
    if (sw.band > 0) g.tile_band = sw.band;   // A/B switch (tools/ab.sh m env BEVGEN_GEMM_BAND=2,4,8)
    // 256-row tiles (8 waves, 3 stages, one block per CU) unless the problem is too small to give every CU one of them; then 128-row tiles
    // with 2 stages (64 KiB) so that two independent 4-wave blocks share a CU
    const int rows = g.M - g.m_base;   // (g.M is the END row of this launch, g.m_base its first)
    const int wm = (sw.wm == 2 || sw.wm == 4) ? sw.wm : (g.force_wm == 4 && sw.top_wm == 4) ? 4 : ((long)cdiv(rows, 256) * cdiv(g.N, kGldsBN) >= 256 ? 4 : 2);
    // Tile quantisation: T tiles of 256 x 128 on 256 CUs cost ceil(T / 256) rounds - the up-projection of sixteen scenes is 4128 tiles = 16.1 rounds and pays 17, of one
    // scene 258 tiles and pays 2, a [12288, 1024] projection of the three-camera shape 384 tiles and pays 2.  When the last round would hold at most 128 tiles, the launch
    // is cut at a row-tile boundary: the first part fills whole rounds, the rest (<= 128 tiles' worth of rows) runs as 128-row blocks, one short round of its own
    // (about 0.45 of a full one).  Same kernels, same per-row arithmetic: results are bit-identical to the single launch.  $BEVGEN_GEMM_ROWSPLIT=0 turns it off (A/B runs)
    if (sw.rowsplit && !g.no_row_split && wm == 4 && g.mode == MODE_PLAIN && g.ksplit <= 1) {
        const long gx = cdiv(g.N, kGldsBN), gy = cdiv(rows, 256), T = gx * gy;
        const long full = T / 256;                       // whole rounds
        const long gy_top = full * 256 / gx;             // row tiles that fit them
        const long rest = (gy - gy_top) * gx;            // tiles left for the last round
        if (T % 256 != 0 && full >= 1 && gy_top >= 1 && gy_top < gy && rest <= 128) {
            *cut = g.m_base + (int)gy_top * 256;         // end row of the first part
            return L;
        }
    }
    // ... unless even those leave CUs without a second block (a batch of one or two scenes): then nothing shares the CU, and the block becomes eight waves with
    // 32x64 patches on a four-stage ring (three k-tiles in flight instead of one; the kernel's TI note).  Measured on the Route M step (tools/ab_env_m.sh): one scene
    // 236 -> 199 ms, two scenes 303 -> 270 ms; at three and four scenes (288 / 384 blocks: two four-wave blocks per CU) the eight-wave block is 2-3 % slower.
    // $BEVGEN_GEMM_STAGES = 2 | 8 | 16 pins the small-problem shape for A/B runs and tests (2: four waves, two stages; 8: eight waves, four stages; 16: 64-row blocks)
    const bool lone = (g.mode == MODE_PLAIN || sw.conv_thin) && (long)cdiv(g.N, kGldsBN) * cdiv(rows, 128) * g.ksplit <= 256;
    // ... and when even the 128-row blocks cover at most half of the CUs (a [1536, 1024] projection: 96), 64-row blocks of four waves (32x64 patches, four stages): twice
    // the blocks, a shorter k-tile each (16 = that shape): 21.4 -> 18.4 us at K = 1024, one-scene step 195.7 -> 187.4 ms on the same box (profiles/r03_ab_b1_half_rows.txt)
    const bool half_rows = lone && g.mode == MODE_PLAIN && g.ksplit == 1 && (long)cdiv(g.N, kGldsBN) * cdiv(rows, 128) <= 128;
    int shape = lone ? (half_rows ? 16 : 8) : 2;
    if (g.mode == MODE_PLAIN && (sw.stages == 2 || sw.stages == 8 || (sw.stages == 16 && g.ksplit == 1))) shape = sw.stages;
    const int stages = wm == 4 ? 3 : (shape == 2 ? 2 : 4);
    const bool thin = wm == 2 && shape == 8, half = wm == 2 && shape == 16;
    // ... and with the plain epilogue (bias / activation / residual: the fused ones need 64-column wave patches) the 64-row block runs on eight waves of 32x32 patches
    const bool half8 = half && sw.half8 && g.epi == 0;
    const int tbm = half ? 64 : wm * 64;
    BG_REQUIRE(g.ksplit >= 1 && (g.ksplit == 1 || (g.kpart && g.epi == 0 && g.mode == MODE_PLAIN && wm == 2 && !half && g.K / kGldsBK >= 2 * g.ksplit && !g.bias_m)),
               "gemm_split_glds: split-K needs a workspace, the plain epilogue, the 128-row tile and >= 2 k-tiles per slice (ksplit=%d K=%d)", g.ksplit, g.K);
    const bool conv = g.mode == MODE_CONV3;
    // stride 1, padding 1, no fused upsample: the variant with wave-uniform tap displacements (MODE_CONV3S; $BEVGEN_CONV_FAST=0 keeps the general one, for A/B runs)
    const bool convs = conv && sw.conv_fast && !g.conv_general && !g.conv_up && g.conv_stride == 1 && g.conv_pad == 1 && g.conv_hin == g.conv_h && g.conv_win == g.conv_w;
    // the block shape as a template tuple: tbm / 64 row groups, 32-row wave patches on the eight-wave small-problem blocks, 32-column ones on the half8 block
    const GldsVariant v{convs ? MODE_CONV3S : conv ? MODE_CONV3 : MODE_PLAIN, tbm / 64, stages, g.b_lo_zero, g.ksplit > 1, (thin || half) ? 1 : 2, half8 ? 1 : 2, false};
    emit(v, dim3(cdiv(g.N, kGldsBN), cdiv(rows, tbm), g.ksplit),
         glds_ring_bytes(v) + ((g.ln_in_stats || g.ln_in_gsums || g.r_prefetch) ? kGldsLdsSlots : 0) + ((g.r_prefetch || g.ln_in_gsums) ? kGldsLdsSums : 0) + (g.ln_in_gsums ? kGldsLdsMerge : 0),
         conv ? PROF_CONV3 : (wm == 4 ? PROF_GEMM : PROF_GEMM_SMALL), 2.0 * rows * (double)g.N * g.K);
    return L;
}

// The whole problem: one launch, or the two of a row-split problem.  xcd_ok = the device's placement probe (xcd_placement_verified), asked only by a launch that meets
// every other stream-K precondition.
inline GldsPlan plan_gemm_split_glds(const GemmArgs& g, const GldsSwitches& sw, int cus, bool (*xcd_ok)()) {
    GldsPlan p;
    int cut = 0, none = 0;
    p.n = 1;
    p.l[0] = glds_plan_range(g, sw, cus, xcd_ok, &cut);
    if (!cut) return p;
    GemmArgs top = g, bot = g;
    top.no_row_split = bot.no_row_split = true;
    top.force_wm = 4;                            // the part that was sized to fill whole rounds of 256-row blocks keeps them
    top.M = bot.m_base = cut;
    // ... and the rest picks its block by its OWN size even when the caller pinned 256-row blocks for the whole problem (q | k | v of two scenes: 288 tiles = 240 +
    // 48; the 48 as 256-row blocks kept 48 CUs busy for 33.5 us, as 192 blocks of 64 rows ~18 us; profiles/r06_ab_rowsplit_bot.txt).  $BEVGEN_ROWSPLIT_BOT_WM=4: as before
    if (sw.bot_wm != 4) bot.force_wm = 0;
    // (the rest on a side stream BESIDE a first part that leaves CUs idle - one scene: 215 blocks on 256 CUs - was measured and rejected: the fork / join events cost
    // more than the overlap buys, one scene 162.9 -> 173.4 ms, sixteen scenes 10.34 -> 10.30 scenes/s; profiles/r05_ab_rowsplit_side_*.txt)
    p.n = 2;
    p.l[0] = glds_plan_range(top, sw, cus, xcd_ok, &none);
    p.l[1] = glds_plan_range(bot, sw, cus, xcd_ok, &none);
    return p;
}

}  // namespace bevgen
