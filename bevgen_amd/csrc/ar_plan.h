// The shape of a Route A decode step (ar.cpp), as pure functions of (batch, model, configuration, switches, state of the fused MLP launch): no HIP runtime call, no
// environment read, no heap.  Exercised on the CPU (tests/test_ar_plan_cpu.py through tests/host/ar_plan_dump.cpp).  The shape predicates of the decode kernels live here
// too, with the constants they use: decode_fused.hip and attention.hip take them from this header (through kernels.h), so kernel, launcher and plan share one definition.
#pragma once
#include <algorithm>
#include "../../include/bevgen_hip.h"
#include "common.h"

namespace bevgen {

// Route A's A/B switches, one environment variable each (ar_switches() in ar.cpp fills the struct; the table is in DESIGN.md).  ln2_fold and mlp_fuse are read once per
// process, pick_tail at every call (its value counts per bevgen_ar_sample).
struct ArSwitches {
    int ln2_fold = 1;    // $BEVGEN_LN2_FOLD: 0 = ln2 in front of the MLP up-projection in its direct form (and no fused MLP launch, which has the folded form only)
    int pick_tail = 1;   // $BEVGEN_PICK_TAIL: 0 = the token's store and the new row's embedding are launches of their own, not the pick launch's tail
    int mlp_fuse = 1;    // $BEVGEN_MLP_FUSE: 0 = never the fused MLP launch (mlp_fused_supported answers false)
};

// ---------------------------------------------------------------- shape predicates of the decode kernels
constexpr int SF_WAVES = 8;             // waves of skinny_fused_kernel / ar_mlp_fused_kernel
constexpr int AF_WAVES = 16;            // waves of the fused decode attention kernels
constexpr int ROWSRC_MAX_SPLITS = 8;    // (4 K slices of the MLP-down launch; 8 XCD planes of the fused MLP launch)
constexpr int ROWSRC_RS_SPLITS = 4;     // the row-source form of skinny_fused_kernel (decode_path = split) keeps its register budget: at most 4 partials
constexpr int MLP_FUSED_PLANES = 8;     // partial planes of the fused MLP launch, one per XCD

inline int skinny_fused_ksplit(int N, int K) {
    // the K slice of one workgroup is at most 1024 (A tile in LDS, W slice in registers); beyond that, split until the grid covers the chip
    int s = 1;
    while (K / s > 1024 || (s < ROWSRC_RS_SPLITS && cdiv(N, 16) * s < 192 && (K / (s * 2)) % (SF_WAVES * 16) == 0 && K / (s * 2) >= 256)) s *= 2;
    return s;
}
inline bool skinny_fused_supported(int M, int N, int K, bool ln) {
    if (M < 1 || M > 64 || K % 4 != 0) return false;
    const int s = ln ? 1 : skinny_fused_ksplit(N, K);
    if (K % s != 0 || s > ROWSRC_RS_SPLITS) return false;   // the consumer's row source adds at most ROWSRC_RS_SPLITS partials
    const int kw = K / s;
    return kw <= 1024 && kw % (SF_WAVES * 16) == 0;
}
// fp16 and int8 weight images (one lane map): the K slice of a workgroup must be a multiple of 32 per wave
inline bool skinny_fused_f16_ok(int N, int K, bool ln) {
    const int s = ln ? 1 : skinny_fused_ksplit(N, K);
    return K % s == 0 && (K / s) % (SF_WAVES * 32) == 0;
}
inline bool ar_attn_fused_supported(int B, int G, int D, int H) { return D == H * 64 && D % 4 == 0 && D <= 1024 && (G == 1 || G == 2 || G == 4) && B % G == 0; }
inline size_t ar_attn_fused_lds_bytes(int G, int D, int Lpad) {
    return ((size_t)Lpad + (size_t)G * D + (size_t)G * 192 + (size_t)AF_WAVES * (G + 1) * 66 + (size_t)AF_WAVES * G) * sizeof(float) + ((size_t)Lpad / 16 + 2 + 8) * sizeof(uint16_t) +
           1024;   // (+ 1 KiB of slack)
}
inline int decode_attention_splits(int B, int H, int n_max) {
    // B*H >= 192 workgroups already cover the chip: one 16-wave workgroup per (sequence, head), direct epilogue.
    // Fewer than that: split the context over workgroups (at least 256 keys per split) and merge in a second kernel.
    if ((long)B * H >= 192) return 1;
    int S = 1;
    while ((long)B * H * S < 1024 && n_max / (S * 2) >= 256) S *= 2;
    return S;
}
// the fused MLP launch (ar_mlp_fused_kernel), shape half: row chunks of 16, at most 64 rows; the K slices per wave - 128 of D, 64 of the XCD's D / 2 - are written out for
// D = 1024.  Device half: one workgroup per CU (every workgroup of an XCD must be resident at once, workgroup i on XCD i % 8) and a verified XCD placement
inline bool mlp_fused_shape_ok(int M, int D) { return M >= 1 && M <= 64 && D == 1024; }
inline bool mlp_fused_cus_ok(int cus, int D) { return cus >= 4 * D / 16; }

// ---------------------------------------------------------------- the decode plan
constexpr int kArAutoSplitMaxSeqs = 4;   // decode_path = auto: the split layer up to this many sequences (layout groups) per call; bevgen_finalize packs its QKV image by the same bound

struct ArPlanIn {
    int B = 0;                              // sequences of the call
    int G = 1;                              // sequences per layout group: the state's G (ar_prefill: its samples_per_layout candidate, ar_prefill_group)
    int D = 0, H = 0, K = 0, L = 0, V = 0;  // model: width, heads, condition rows, sequence length, vocabulary (head rows)
    int decode_path = BEVGEN_DECODE_FUSED;  // as configured (BEVGEN_DECODE_*)
    int w_f16 = 0;                          // decode_weight_dtype, the storage kind of the packed images: 0 fp32, 1 fp16 (BEVGEN_W_F16), 2 int8 codes + row scales (BEVGEN_W_I8:
                                            // the int8 image keeps the fp16 image's lane map, so every rule below that asks `w_f16` holds for both)
    int chains = 0;                         // as configured ($BEVGEN_DECODE_CHAINS through the Python host)
    bool trace = false;                     // the phase-timestamp buffer is attached
    bool mlpf_ready = false;                // the context holds the fused MLP launch's barrier words and no launch of it has failed (mlpf_sync && !mlpf_disabled)
    bool mlpf_device_ok = false;            // mlp_fused_cus_ok and XCD placement verified, asked once per context at bevgen_finalize
};
struct ArStepPlan {
    int path = BEVGEN_DECODE_FUSED;         // the effective path: auto resolved
    bool fused = false;                     // the three/four-launch layer of decode_fused.hip; false = the per-operator step
    bool split = false;                     // fused, in its split form (LayerNorm + QKV projection kernel, attention-only kernel)
    int chains = 1, Bc = 0;                 // independent sequence groups on streams of their own, sequences of each
    bool mlp_fused = false;                 // both MLP projections in one launch
    bool ln2_fold = true;                   // two-launch MLP: ln2 folded into the up-projection
    int down_ksplit = 1;                    // K slices of the MLP down-projection
    int attn_ksplit = 1;                    // split layer: ranges of the key walk of one (sequence, head); 1 = one workgroup walks it
    bool pick_embeds = false;               // ar_sample: the pick launch also stores the token and writes the new row's embedding
    bool needs_split_qkv_image = false;     // the path is the split one: its packed QKV operand image must exist (ctx_pack_split_qkv)
};

inline bool ar_split_supported(const ArPlanIn& in) {
    return skinny_fused_supported(in.B, 3 * in.D, in.D, true) && (!in.w_f16 || skinny_fused_f16_ok(3 * in.D, in.D, true));
}
inline bool ar_mlp_fused_ok(const ArPlanIn& in, const ArSwitches& sw, int M) { return sw.mlp_fuse && mlp_fused_shape_ok(M, in.D) && in.mlpf_device_ok; }

// BEVGEN_DECODE_AUTO: the split layer for up to four sequences (layout groups) per call, else the fused one.  Same box, config 4, fp32, full decodes, ms per step
// split / fused: B = 1 0.99 / 1.28, B = 2 1.04 / 1.24, B = 3 1.14 / 1.22, B = 4 1.17 / 1.21, B = 6 1.27 / 1.21, B = 8 1.34 / 1.24, B = 16 1.47 / 1.42.  With 16-64
// workgroups per layer the fused kernel's per-head GEMV cannot pull the 12.6 MB of q/k/v weights fast enough and a workgroup's 1.2 MB K/V range streams at one CU's
// rate; the projection kernel spreads the weights over 192 workgroups and the attention-only kernel cuts each key walk into up to four ranges.
// Round 5, with both MLP projections in one launch (ar_mlp_fused_kernel, fused path only), same box, full decodes, ms per step fused / split (profiles/r05_auto_threshold.txt):
// fp16 cache + fp16 weights B = 1 0.710 / 0.829, 2 0.715 / 0.855, 4 0.727 / 0.940, 8 0.737 / 1.014 - the fused layer wins at EVERY batch size; fp32 storage
// B = 1 1.116 / 0.919, 2 1.091 / 0.945, 3 1.094 / 1.044, 4 1.094 / 1.072, 6 1.095 / 1.186: the split layer up to four sequences, as before.
inline int ar_effective_path(const ArPlanIn& in, const ArSwitches& sw) {
    if (in.decode_path != BEVGEN_DECODE_AUTO) return in.decode_path;
    if (in.w_f16 && in.G <= 1 && in.mlpf_ready && ar_mlp_fused_ok(in, sw, in.B)) return BEVGEN_DECODE_FUSED;
    return (in.B / std::max(in.G, 1) <= kArAutoSplitMaxSeqs && ar_split_supported(in)) ? BEVGEN_DECODE_SPLIT : BEVGEN_DECODE_FUSED;
}
// does the step run the layer of decode_fused.hip?  Otherwise the per-operator step (one kernel per operator, any shape)
inline bool ar_fused(const ArPlanIn& in, const ArSwitches& sw) {
    const int path = ar_effective_path(in, sw);
    if (path != BEVGEN_DECODE_FUSED && path != BEVGEN_DECODE_SPLIT) return false;
    const int B = in.B, G = in.G, D = in.D;
    if (path == BEVGEN_DECODE_SPLIT && !ar_split_supported(in)) return false;
    if (G > 1 && in.K % 16 != 0) return false;   // the shared condition prefix must end on a 16-key chunk boundary (the per-operator path replicates it instead)
    return ar_attn_fused_supported(B, G, D, in.H) && skinny_fused_supported(B, 4 * D, D, true) && skinny_fused_supported(B, D, 4 * D, false) &&
           skinny_fused_supported(B, in.V, D, true) && ar_attn_fused_lds_bytes(G, D, (int)round_up(in.L, 4)) <= 64 * 1024 &&
           (!in.w_f16 || (skinny_fused_f16_ok(4 * D, D, true) && skinny_fused_f16_ok(D, 4 * D, false) && skinny_fused_f16_ok(in.V, D, true)));
}
// ar_prefill, samples_per_layout = S: the S sequences of a layout share a workgroup (and the group's first cache slot) only on the fused paths; otherwise G = 1
inline int ar_prefill_group(ArPlanIn in, const ArSwitches& sw, int S) {
    in.G = S;
    return ar_fused(in, sw) ? S : 1;
}

// Number of independent sequence groups ("chains") the fused step is cut into.  A decode step is a chain of ~75 short, strictly dependent kernels; each one pays its ramp,
// one cold weight burst and its tail alone (the weight-streaming projections reach ~2 TB/s while they run, the chip idles in between).  Sequences are independent, so
// the batch is cut into chains enqueued on separate streams: the hardware then always has another chain's kernel to run - a projection's 16.8 MB weight burst under the
// other chain's K/V stream.  The price: every chain streams the layer's projection weights (50 MB / layer with fp32 storage) itself; the second read of a matrix
// follows the first within a layer and is served by the memory-side cache.  (A persistent single-launch layer was measured instead and rejected: a grid-wide
// exchange between phases costs 7.9 us on this 8-XCD part, profiles/r03_xchg_probe.txt - more than a kernel boundary.)
inline int ar_decode_chains(const ArPlanIn& in) {
    int n = in.chains;
    if (n <= 0) n = 1;   // measured (profiles/r03_chain_probe.txt, B = 16): 1 chain 1.41 ms/step, 2 chains 1.60, 4 chains 1.96 - the option stays for experiments
    n = std::min(n, 4);
    while (n > 1 && ((in.B / in.G) % n != 0 || (in.B / in.G) / n < 1)) --n;
    if (in.trace) n = 1;   // the phase-timestamp buffers are indexed by workgroup of ONE launch per kind
    return n;
}

inline ArStepPlan ar_step_plan(const ArPlanIn& in, const ArSwitches& sw) {
    ArStepPlan p;
    p.path = ar_effective_path(in, sw);
    p.needs_split_qkv_image = p.path == BEVGEN_DECODE_SPLIT;
    p.fused = ar_fused(in, sw);
    p.split = p.fused && p.path == BEVGEN_DECODE_SPLIT;
    p.chains = p.fused ? ar_decode_chains(in) : 1;
    p.Bc = in.B / p.chains;
    p.ln2_fold = sw.ln2_fold != 0;
    p.down_ksplit = skinny_fused_ksplit(in.D, 4 * in.D);
    // Both MLP projections of a layer in one launch (ar_mlp_fused_kernel): the fused three-launch layer, one chain, at most 64 rows (row chunks of 16), ln2 folded, a device
    // whose CUs hold the whole grid at once.  Otherwise the two skinny launches.
    p.mlp_fused = p.fused && !p.split && p.chains == 1 && p.ln2_fold && in.mlpf_ready && p.down_ksplit > 1 && ar_mlp_fused_ok(in, sw, p.Bc);
    // split layer, one or two sequences: 16-32 workgroups cannot pull a 1.2 MB K/V range each at the chip's rate - split the key walk over more of them (the partial
    // states live in the per-operator path's workspace, sized for decode_attention_splits(B, H, L): at least this many)
    if (p.split && in.G == 1 && p.Bc * in.H < 128) p.attn_ksplit = std::max(1, std::min(std::min(4, 128 / (p.Bc * in.H)), decode_attention_splits(in.B, in.H, in.L)));
    p.pick_embeds = p.fused && p.chains == 1 && sw.pick_tail != 0;
    return p;
}

// ar_sample captures one step and replays it as a hipGraph: only when there is something to replay, the caller does not want every step's logits, the profiler is off
// and the context allows graphs; otherwise every step is enqueued eagerly
inline bool ar_use_graph(int steps, bool wants_step_logits, bool profiling, bool graphs_disabled) { return steps > 2 && !wants_step_logits && !profiling && !graphs_disabled; }

}  // namespace bevgen
