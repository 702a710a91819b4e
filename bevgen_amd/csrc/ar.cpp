// Route A: autoregressive sparse-causal transformer with camera bias, run as prefill + KV-cache decode.
//   GPT.forward                      transformer/mingpt_sparse.py:319-391
//   Block.forward                    :240-253   (x = ln1(x); x = x + attn(x); x = x + mlp(ln2(x)) - residual from ln1(x), no out-proj)
//   CustomSparseSelfAttention        :185-212   + SparseSelfAttention.forward transformer/sparse_self_attention.py:103-177
//   Net2NetTransformer.sample        stage2/cond_transformer_multi_view.py:154-227
//
// The reference re-runs the whole L-token forward for every generated token (ar_lm:198).  Image rows are causal in decode
// order and condition rows only see condition columns (mask_generator.py:148, 202-206), so the logits of step s depend only on
// rows <= K-1+s: we compute the K condition rows once (prefill), keep K/V of every layer, and per step push exactly one new
// row through the stack (validity verified against the reference).
#include <atomic>
#include <mutex>
#include "model.h"
#include "profiler.h"

namespace bevgen {

// Decode steps that contain a launch whose workgroups wait for each other (ar_mlp_fused_kernel: every workgroup of an XCD must be resident at once) must not interleave
// with another such stream of launches on the same device: two half-resident grids could starve each other until the bounded spin gives up.  One context is one stream
// of strictly ordered launches; the decode calls of ALL Route-A contexts of the process are chained on the device by one event per device (a call's launches wait until
// the previous call's have drained) and on the host by a mutex held while a call enqueues: one uncontended lock, one stream wait and one event record per call - taken
// unconditionally (a "more than one context alive" fast path would race with a context created while another one is decoding).  Another PROCESS on the same GPU is not
// covered: there the bounded spin times out, the launch poisons itself (later launches return at once), the status word reports it and the context falls back to the
// two-launch form (Ctx::check_status).
namespace {
std::mutex g_spin_mu;
hipEvent_t g_spin_ev[64] = {};
struct SpinSerial {
    std::unique_lock<std::mutex> lk;
    hipEvent_t ev = nullptr;
    hipStream_t q = nullptr;
    SpinSerial(const Ctx& c, hipStream_t stream) {
        if (!c.mlpf_sync || c.mlpf_disabled) return;
        lk = std::unique_lock<std::mutex>(g_spin_mu);
        hipEvent_t& e = g_spin_ev[c.device >= 0 && c.device < 64 ? c.device : 0];
        if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev = e; q = stream;
        HIP_CHECK(hipStreamWaitEvent(q, ev, 0));   // (never recorded yet: a no-op)
    }
    void rebind(hipStream_t stream) { if (ev) { HIP_CHECK(hipStreamWaitEvent(stream, ev, 0)); q = stream; } }
    ~SpinSerial() { if (ev) (void)hipEventRecord(ev, q); }
};
}  // namespace

// $BEVGEN_LN2_FOLD and $BEVGEN_MLP_FUSE once per process, $BEVGEN_PICK_TAIL at every call (ar_plan.h)
ArSwitches ar_switches() {
    const auto env = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    static const ArSwitches once = [&] {
        ArSwitches s;
        s.ln2_fold = env("BEVGEN_LN2_FOLD", 1);
        s.mlp_fuse = env("BEVGEN_MLP_FUSE", 1);
        return s;
    }();
    ArSwitches s = once;
    s.pick_tail = env("BEVGEN_PICK_TAIL", 1);
    return s;
}

namespace {

GemmArgs gemm_args(const float* A, int lda, const float* W, int ldb, const float* bias, float* C, int ldc, int M, int N, int K, int act, const float* R, int ldr) {
    GemmArgs g;
    g.A = A; g.B = W; g.C = C; g.R = R; g.bias_n = bias;
    g.M = M; g.N = N; g.K = K;
    g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.ldr = ldr; g.act = act;
    return g;
}
void gemm(const float* A, int lda, const float* W, int ldb, const float* bias, float* C, int ldc, int M, int N, int K, int act, const float* R, int ldr, hipStream_t s) {
    launch_gemm(gemm_args(A, lda, W, ldb, bias, C, ldc, M, N, K, act, R, ldr), s);
}

int cache_dtype(const Ctx& c) { return c.cfg.kv_cache_dtype == BEVGEN_KV_F16 ? 1 : c.cfg.kv_cache_dtype == BEVGEN_KV_I8 ? 2 : 0; }
// The KV cache of one layer, K or V: [B, H, L, 64] elements; the int8 mode appends its [B, H, L] fp32 row scales (bevgen_hip.h).  Every size, stride and offset of the cache
// goes through these three.
size_t cache_layer_bytes(const Ctx& c, int B) {
    const size_t rows = (size_t)B * c.H * c.L;
    switch (cache_dtype(c)) { case 1: return rows * 128; case 2: return rows * kKvI8RowBytes; default: return rows * 256; }
}
size_t cache_slot_bytes(const Ctx& c, int b0) { return (size_t)b0 * c.H * c.L * 64 * (cache_dtype(c) == 0 ? 4 : cache_dtype(c) == 1 ? 2 : 1); }   // slot b0's first element inside a layer
// int8: bytes from slot b0's codes to slot b0's scales, in a layer of B slots (the kernels' sc_off; unused otherwise)
long cache_scale_off(const Ctx& c, int B, int b0) { return (long)c.H * c.L * (64L * B - 60L * b0); }
int replicate_elem_bytes(const Ctx& c) { return cache_dtype(c) == 0 ? 4 : cache_dtype(c) == 1 ? 2 : 1; }

struct StepWs {
    float *x, *xn, *qkv, *x2, *h, *m1, *dec_ws, *gemm_ws, *logits;
    float *x2b, *part;   // fused path: second x2 buffer (layers alternate), split-K partials of the MLP down-projection
    int64_t* tok;
    int splits;
};

// The plan of a decode step (ar_plan.h) for B sequences in groups of G, from the context as it is NOW: every entry point computes it once and hands it down -
// mlpf_disabled may change between calls (Ctx::check_status), so a plan is never kept across calls.
ArPlanIn plan_in(const Ctx& c, int B, int G) {
    ArPlanIn in;
    in.B = B; in.G = G;
    in.D = c.D; in.H = c.H; in.K = c.K; in.L = c.L; in.V = c.V;
    in.decode_path = c.cfg.decode_path; in.w_f16 = c.cfg.decode_weight_dtype; in.chains = c.cfg.decode_chains; in.trace = c.trace != nullptr;
    in.mlpf_ready = c.mlpf_sync && !c.mlpf_disabled; in.mlpf_device_ok = c.mlpf_device_ok;
    return in;
}
ArStepPlan step_plan(const Ctx& c, int B, int G) { return ar_step_plan(plan_in(c, B, G), ar_switches()); }

size_t part_floats(const Ctx& c, int B) { return (size_t)std::max(skinny_fused_ksplit(c.D, 4 * c.D), MLP_FUSED_PLANES) * B * c.D; }

// The decode-step buffers: a layout function (arena.h), fixed at the start of the per-call arena so that a captured graph keeps seeing the same addresses.  ar_prefill and
// ar_forward start their layouts with it; ar_logits, ar_decode_step and ar_sample re-carve it alone after a reset() WITHOUT reserving: they rely on that reservation.
StepWs step_ws(const Ctx& c, Arena& a, int B) {
    StepWs w;
    const int D = c.D;
    w.x = a.get<float>((size_t)B * D);
    w.xn = a.get<float>((size_t)B * D);
    w.qkv = a.get<float>((size_t)B * 3 * D);
    w.x2 = a.get<float>((size_t)B * D);
    w.h = a.get<float>((size_t)B * D);
    w.m1 = a.get<float>((size_t)B * 4 * D);
    w.splits = decode_attention_splits(B, c.H, c.L);
    w.dec_ws = reinterpret_cast<float*>(a.alloc(decode_attention_ws_bytes(B, c.H, w.splits)));
    size_t gw = std::max(std::max(gemm_skinny_ws_bytes(B, 3 * D, D), gemm_skinny_ws_bytes(B, 4 * D, D)),
                         std::max(gemm_skinny_ws_bytes(B, D, 4 * D), gemm_skinny_ws_bytes(B, c.V, D)));
    w.gemm_ws = reinterpret_cast<float*>(a.alloc(gw));
    w.logits = a.get<float>((size_t)B * c.V);
    w.tok = a.get<int64_t>((size_t)B);
    w.x2b = a.get<float>((size_t)B * D);
    w.part = a.get<float>(part_floats(c, B));
    return w;
}

void small_gemm(const float* A, int lda, const float* W, int ldb, const float* bias, float* C, int ldc, int M, int N, int K, int act, const float* R, int ldr,
                float* ws, hipStream_t s) {
    const GemmArgs g = gemm_args(A, lda, W, ldb, bias, C, ldc, M, N, K, act, R, ldr);
    if (M <= 64) launch_gemm_skinny_ws(g, ws, s);
    else launch_gemm(g, s);
}

// Flash attention over whole sequences: Q [B, H, Nq, 64], K / V [B, H, Lk, 64] (the first Nk_pad rows of a head are read), masked bias [H or 1][Nq][Nk_pad] and the
// key-tile lists built from it.  The caller adds the residual and the output with its layout.
AttnArgs attn_args(const float* Q, const float* K, const float* V, int Lk, const float* bias, const uint16_t* tiles, bool per_head, int B, int H, int Nq, int Nk_pad) {
    AttnArgs a{};
    a.Q = Q; a.K = K; a.V = V; a.bias = bias;
    a.B = B; a.H = H; a.Nq = Nq; a.Nk_pad = Nk_pad;
    a.q_bstride = (long)H * Nq * 64; a.q_hstride = (long)Nq * 64;
    a.kv_bstride = (long)H * Lk * 64; a.kv_hstride = (long)Lk * 64;
    a.ldbias = Nk_pad; a.bias_head_stride = per_head ? (long)Nq * Nk_pad : 0; a.scale = 0.125f;
    a.tiles = tiles; a.tiles_head_stride = per_head ? (long)cdiv(Nq, 128) * (Nk_pad / 32 + 1) : 0; a.tiles_ld = Nk_pad / 32 + 1;
    return a;
}

// masked bias of layer i over its first R rows and keys, and the key tiles of every query block that hold a present block
void build_layer_bias(Ctx& c, int i, float* bias, uint16_t* tiles, int R, int Rpad, hipStream_t s) {
    launch_build_masked_bias(c.attn_bias, c.vis_of_layer(i), bias, c.keep_heads, R, R, Rpad, c.L, 0.125f, s);
    launch_build_attn_tiles(bias, (long)R * Rpad, Rpad, c.keep_heads, R, Rpad, tiles, s);
}

// One transformer layer over whole sequences from row 0 (Block.forward, mingpt_sparse.py:240-253), as ar_prefill and ar_forward run it; what differs between them:
struct PrefixRows {
    int nseq, R, Rpad;                      // sequences, rows of each, the rows padded to the attention's key tile
    float *x, *xn, *x2, *h, *qkv, *m1, *Q;  // x [nseq R, D]: the residual stream, in and out; the others scratch of the same rows
    float *k, *v; int Lk;                   // fp32 K / V that the attention reads, [nseq, H, Lk, 64]
    void *kcache, *vcache;                  // these sequences' slots of the layer's cache - null when k / v ARE those slots (ar_prefill with an fp32 cache)
    const float* bias; uint16_t* tiles;     // masked bias [keep_heads][R][Rpad] and its tile lists
    float* layer_bias;                      // non-null: bias and tiles of THIS layer are built here, behind the scatters (ar_prefill with per-layer layouts)
};
void prefix_layer(Ctx& c, int i, const PrefixRows& p, hipStream_t s, long sc_off = 0) {
    const ArLayer& l = c.ar[i];
    const int D = c.D, H = c.H, rows = p.nseq * p.R;
    launch_layernorm(p.x, D, l.ln1_w, l.ln1_b, p.xn, D, rows, D, 1e-5f, s);
    gemm(p.xn, D, l.wqkv, D, l.bqkv, p.qkv, 3 * D, rows, 3 * D, D, ACT_NONE, nullptr, 0, s);
    launch_ar_qkv_scatter(p.qkv, p.Q, p.k, p.v, 0, p.nseq, H, p.R, 0, p.Lk, s);                                                    // what this pass's attention reads
    if (p.kcache) launch_ar_qkv_scatter(p.qkv, nullptr, p.kcache, p.vcache, cache_dtype(c), p.nseq, H, p.R, 0, c.L, s, sc_off);   // the persistent rows [0, R) the decode steps read
    if (p.layer_bias) build_layer_bias(c, i, p.layer_bias, p.tiles, p.R, p.Rpad, s);
    AttnArgs a = attn_args(p.Q, p.k, p.v, p.Lk, p.layer_bias ? p.layer_bias : p.bias, p.tiles, c.keep_heads > 1, p.nseq, H, p.R, p.Rpad);
    a.R = p.xn; a.O = p.x2; a.o_bstride = (long)p.R * D; a.o_qstride = D; a.o_hstride = 64;
    launch_attention(a, s);  // x2 = ln1(x) + attn
    launch_layernorm(p.x2, D, l.ln2_w, l.ln2_b, p.h, D, rows, D, 1e-5f, s);
    gemm(p.h, D, l.mlp0_w, D, l.mlp0_b, p.m1, 4 * D, rows, 4 * D, D, ACT_GELU, nullptr, 0, s);
    gemm(p.m1, 4 * D, l.mlp2_w, 4 * D, l.mlp2_b, p.x, D, rows, D, 4 * D, ACT_NONE, p.x2, D, s);
}

// Camera embeddings of all B sequences (state of the decode steps), then the condition rows of the first sequence of every group of S into x [B / S, K, D]; S > 1:
// cg / eg take contiguous [B / S, ...] copies of those sequences' ids and camera embeddings
void embed_condition(Ctx& c, const int64_t* cond, const float* I_inv, const float* E_inv, int B, int S, int64_t* cg, float* eg, float* x, hipStream_t s) {
    const auto& g = c.cfg;
    auto& st = c.ars;
    const int D = c.D, K = c.K, G = B / S;
    if (g.image_embed)
        launch_camera_embed(I_inv, E_inv, c.image_plane, c.pf("img_embed.weight"), c.pf("cam_embed.weight"), st.img_embed, st.c_embed, B, g.num_cams, c.T, D, s);
    const float* c_embed = st.c_embed;
    if (S > 1) {
        HIP_CHECK(hipMemcpy2DAsync(cg, (size_t)K * 8, cond, (size_t)S * K * 8, (size_t)K * 8, G, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpy2DAsync(eg, (size_t)g.num_cams * D * 4, st.c_embed, (size_t)S * g.num_cams * D * 4, (size_t)g.num_cams * D * 4, G, hipMemcpyDeviceToDevice, s));
        cond = cg; c_embed = eg;
    }
    const bool bev = g.bev_embed;
    launch_cond_embed(cond, c.pf("cond_tok_emb.weight"), c.pf("cond_pos_emb"), bev ? c.pf("bev_grid") : nullptr, bev ? c.pf("bev_embed.weight") : nullptr,
                      bev ? c.pf("bev_embed.bias") : nullptr, bev ? c.pf("bev_cam_pos_emb") : nullptr, c_embed, x, G, g.num_cams, K, D, g.cond_vocab_size, s);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ operator seam
void sparse_self_attention_op(Ctx& c, const float* q, const float* k, const float* v, const int64_t* layout, const float* mask, const float* add, int B, int H,
                              int L, int block, float* out, hipStream_t s) {
    BG_REQUIRE(L % block == 0, "Sequence Length, %d, needs to be dividable by Block size %d!", L, block);  // ssa:54-57
    const int Lpad = (int)round_up(L, 32);
    const int nb = L / block;
    const bool pad = Lpad != L;
    struct { uint8_t *allowed, *lay; uint16_t *chunks, *tiles; float *bias, *kpad, *vpad; } w;
    c.arena.carve([&](Arena& a) {
        w.allowed = a.get<uint8_t>((size_t)L * L);
        w.lay = a.get<uint8_t>((size_t)H * nb * nb);
        w.chunks = a.get<uint16_t>((size_t)H * nb * (cdiv(L, 16) + 1));
        w.bias = a.get<float>((size_t)H * L * Lpad);
        w.tiles = a.get<uint16_t>(attn_tiles_elems(H, L, Lpad));
        w.kpad = pad ? a.get<float>((size_t)B * H * Lpad * 64) : nullptr;
        w.vpad = pad ? a.get<float>((size_t)B * H * Lpad * 64) : nullptr;
    });
    SparseVis vis;
    launch_build_allowed(mask, w.allowed, (long)L * L, s);
    launch_build_layout(layout, w.lay, w.chunks, H, nb, block, L, (int)cdiv(L, 16) + 1, s);
    vis.allowed = w.allowed; vis.ldallowed = L;
    vis.lay = w.lay; vis.lay_head_stride = (long)nb * nb; vis.nb = nb; vis.blk = block;
    float* bias = w.bias;
    launch_build_masked_bias(add, vis, bias, H, L, L, Lpad, L, 0.125f, s);
    // only the key tiles in which some row of a query block sees a key are loaded and multiplied (the reference computes the nonzero layout blocks only, ssa:63-85)
    uint16_t* tiles = w.tiles;
    launch_build_attn_tiles(bias, (long)L * Lpad, Lpad, H, L, Lpad, tiles, s);
    const float *kp = k, *vp = v;
    if (pad) {
        float *kpad = w.kpad, *vpad = w.vpad;
        HIP_CHECK(hipMemsetAsync(kpad, 0, (size_t)B * H * Lpad * 64 * sizeof(float), s));
        HIP_CHECK(hipMemsetAsync(vpad, 0, (size_t)B * H * Lpad * 64 * sizeof(float), s));
        HIP_CHECK(hipMemcpy2DAsync(kpad, (size_t)Lpad * 256, k, (size_t)L * 256, (size_t)L * 256, (size_t)B * H, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpy2DAsync(vpad, (size_t)Lpad * 256, v, (size_t)L * 256, (size_t)L * 256, (size_t)B * H, hipMemcpyDeviceToDevice, s));
        kp = kpad; vp = vpad;
    }
    AttnArgs a = attn_args(q, kp, vp, Lpad, bias, tiles, true, B, H, L, Lpad);
    a.O = out; a.o_bstride = (long)H * L * 64; a.o_qstride = 64; a.o_hstride = (long)L * 64;  // [B,H,L,64] like the reference op
    launch_attention(a, s);
}

// persistent per-batch state of a decode (K/V cache of every layer, geometric embeddings, newest hidden row, device step counter): zeroed cache, step 0
static void ar_state_setup(Ctx& c, int B, hipStream_t s) {
    const auto& g = c.cfg;
    const int D = c.D, L = c.L;
    auto& st = c.ars;
    BG_REQUIRE(cache_dtype(c) != 2 || L % 4 == 0, "kv_cache = i8: the sequence length %d must be a multiple of 4 (16-byte aligned layers)", L);
    const size_t cache_b = (size_t)g.num_layers * cache_layer_bytes(c, B);
    st.B = B;
    st.step = 0;
    c.persist.carve([&](Arena& a) {
        st.kcache = a.alloc(cache_b);
        st.vcache = a.alloc(cache_b);
        st.img_embed = g.image_embed ? a.get<float>((size_t)B * g.num_cams * c.T * D) : nullptr;
        st.c_embed = a.get<float>((size_t)B * g.num_cams * D);
        st.hidden = a.get<float>((size_t)B * D);
        st.d_step = a.get<int>(1);
    });
    HIP_CHECK(hipMemsetAsync(st.kcache, 0, cache_b, s));
    HIP_CHECK(hipMemsetAsync(st.vcache, 0, cache_b, s));
    HIP_CHECK(hipMemsetAsync(st.d_step, 0, sizeof(int), s));
}

// ------------------------------------------------------------------------------------------------ prefill
// samples_per_layout = S > 1 (BASELINE config 5): consecutive groups of S sequences share their condition (BEV ids and cameras), so the condition
// prefix is pushed through the stack once per LAYOUT (B / S sequences) and its K/V rows are then replicated into the S cache slots of the group.
void ar_prefill(Ctx& c, const int64_t* cond, const float* I_inv, const float* E_inv, int B, hipStream_t s, int samples_per_layout) {
    const auto& g = c.cfg;
    BG_REQUIRE(g.route == BEVGEN_ROUTE_AR, "context was not created for the autoregressive route");
    BG_REQUIRE(B >= 1, "batch must be positive");
    const int S = samples_per_layout < 1 ? 1 : samples_per_layout;
    BG_REQUIRE(B % S == 0, "batch %d is not a multiple of samples_per_layout %d", B, S);
    const int G = B / S;   // layouts = sequences actually prefilled
    const int D = c.D, H = c.H, K = c.K, L = c.L;
    auto& st = c.ars;
    // decode_path = auto: the split layer's QKV operand image is packed by the first batch that will run it (S sequences per workgroup only on the fused paths)
    const ArSwitches sw = ar_switches();
    const int group = ar_prefill_group(plan_in(c, B, 1), sw, S);
    if (ar_step_plan(plan_in(c, B, group), sw).needs_split_qkv_image) ctx_pack_split_qkv(c, s);
    ar_state_setup(c, B, s);

    // workspace: the decode-step buffers first (stable addresses), then the prefill activations
    const size_t rows = (size_t)G * K;
    const int kvd = cache_dtype(c);   // fp16 cache: the prefill attention reads exact fp32 K/V from a scratch pair
    const size_t layer_bias = c.prefill_bias ? 0 : (size_t)c.keep_heads * K * c.Kpad;   // per-layer layouts: this layer's masked bias is built on the fly
    float *x, *xn, *x2, *h, *qkv, *m1, *Q, *lbias, *eg, *tk, *tv, *hid;
    uint16_t* ltiles;   // key tiles of the condition rows that hold a present block (rebuilt per layer when layouts differ)
    int64_t* cg;
    c.arena.carve([&](Arena& a) {
        (void)step_ws(c, a, B);
        x = a.get<float>(rows * D);
        xn = a.get<float>(rows * D);
        x2 = a.get<float>(rows * D);
        h = a.get<float>(rows * D);
        qkv = a.get<float>(rows * 3 * D);
        m1 = a.get<float>(rows * 4 * D);
        Q = a.get<float>((size_t)G * H * K * 64);
        lbias = c.prefill_bias ? nullptr : a.get<float>(layer_bias);
        ltiles = a.get<uint16_t>(attn_tiles_elems(c.keep_heads, K, c.Kpad));
        cg = S > 1 ? a.get<int64_t>((size_t)G * K) : nullptr;   // first sequence of every group -> contiguous [G, ...] inputs of the prefill
        eg = S > 1 ? a.get<float>((size_t)G * g.num_cams * D) : nullptr;
        tk = kvd ? a.get<float>((size_t)G * H * c.Kpad * 64) : nullptr;
        tv = kvd ? a.get<float>((size_t)G * H * c.Kpad * 64) : nullptr;
        hid = S > 1 ? a.get<float>((size_t)G * D) : nullptr;   // the groups' last condition rows, fanned out into st.hidden at the end
    });
    if (c.prefill_bias) launch_build_attn_tiles(c.prefill_bias, (long)K * c.Kpad, c.Kpad, c.keep_heads, K, c.Kpad, ltiles, s);

    embed_condition(c, cond, I_inv, E_inv, B, S, cg, eg, x, s);
    if (kvd) {
        HIP_CHECK(hipMemsetAsync(tk, 0, (size_t)G * H * c.Kpad * 64 * sizeof(float), s));   // pad rows K..Kpad stay zero
        HIP_CHECK(hipMemsetAsync(tv, 0, (size_t)G * H * c.Kpad * 64 * sizeof(float), s));
    }
    const size_t layer_bytes_p = cache_layer_bytes(c, B);
    BG_REQUIRE(c.Kpad <= L, "condition length padded to %d exceeds the cache length %d", c.Kpad, L);
    PrefixRows p{G, K, c.Kpad, x, xn, x2, h, qkv, m1, Q, tk, tv, c.Kpad, nullptr, nullptr, c.prefill_bias, ltiles, lbias};
    for (int i = 0; i < g.num_layers; ++i) {   // all G K rows at once, into cache slots [0, G) for now
        char* kcb = reinterpret_cast<char*>(st.kcache) + i * layer_bytes_p;
        char* vcb = reinterpret_cast<char*>(st.vcache) + i * layer_bytes_p;
        if (kvd) { p.kcache = kcb; p.vcache = vcb; }                                                               // the fp16 image the decode steps read
        else { p.k = reinterpret_cast<float*>(kcb); p.v = reinterpret_cast<float*>(vcb); p.Lk = L; }   // the attention reads the cache itself
        prefix_layer(c, i, p, s, cache_scale_off(c, B, 0));   // (G of the layer's B slots are written)
    }
    st.G = 1;
    if (S == 1) {
        launch_gather_rows(x, st.hidden, B, K - 1, K, D, s);
        return;
    }
    if (group == S) {
        // the fused decode kernel reads the K prefix rows of a group from the group's FIRST cache slot: move slot g -> slot g*S, highest group first
        // (a destination never holds a source that is still needed); the other slots of the group keep only their private rows >= K
        st.G = S;
        for (int gi = G - 1; gi >= 1; --gi)
            launch_replicate_prefix(st.kcache, st.vcache, g.num_layers, B, H, L, K, gi, gi * S, 1, replicate_elem_bytes(c), s);
    } else {
        // per-operator path: fan the shared prefix out into every slot of the group
        for (int gi = G - 1; gi >= 0; --gi)
            launch_replicate_prefix(st.kcache, st.vcache, g.num_layers, B, H, L, K, gi, gi * S, S, replicate_elem_bytes(c), s);
    }
    launch_gather_rows(x, hid, G, K - 1, K, D, s);
    for (int j = 0; j < S; ++j)
        HIP_CHECK(hipMemcpy2DAsync(st.hidden + (size_t)j * D, (size_t)S * D * 4, hid, (size_t)D * 4, (size_t)D * 4, G, hipMemcpyDeviceToDevice, s));
}

// ln_f + head on the newest rows (mingpt_sparse.py:386-387)
static void head_logits(Ctx& c, StepWs& w, const ArStepPlan& plan, int B, float* logits, hipStream_t s) {
    auto& st = c.ars;
    if (plan.fused) {
        SkinnyFusedArgs g;
        g.A = st.hidden; g.lda = c.D;
        g.ln_w = c.pf("ln_f.weight"); g.ln_b = c.pf("ln_f.bias"); g.eps = 1e-5f;
        g.Wp = c.head_wp; g.w_f16 = c.cfg.decode_weight_dtype; g.w_scale = c.head_sc;
        g.C = logits; g.ldc = c.V;
        g.M = B; g.N = c.V; g.K = c.D; g.ksplit = 1;
        launch_skinny_fused(g, s);
        return;
    }
    launch_layernorm(st.hidden, c.D, c.pf("ln_f.weight"), c.pf("ln_f.bias"), w.xn, c.D, B, c.D, 1e-5f, s);
    small_gemm(w.xn, c.D, c.pf("head.weight"), c.D, nullptr, logits, c.V, B, c.V, c.D, ACT_NONE, nullptr, 0, w.gemm_ws, s);
}

void ar_logits(Ctx& c, float* logits, hipStream_t s) {
    auto& st = c.ars;
    BG_REQUIRE(st.B > 0, "bevgen_ar_prefill must be called first");
    c.arena.reset();
    StepWs w = step_ws(c, c.arena, st.B);
    head_logits(c, w, step_plan(c, st.B, st.G), st.B, logits, s);
}

// One chain = the sequences [r0, r0 + Bc) through all layers.  Fused form of the step (decode_fused.hip): per layer {ln1 + qkv + attention, ln2 + MLP up + GELU,
// MLP down split over K}; the down-projection's partial sums, bias and residual are folded into the next consumer's row fetch (RowSrc), the last layer's into
// the hidden-state write.
static void decode_chain_launch(Ctx& c, StepWs& w, const ArStepPlan& plan, const int64_t* tok, int r0, int* counter, hipStream_t s) {
    const auto& g = c.cfg;
    auto& st = c.ars;
    const int D = c.D, H = c.H, B = st.B, Bc = plan.Bc, L = c.L;
    float* x = w.x + (size_t)r0 * D;
    if (!(st.pick_embeds && tok == w.tok && r0 == 0 && Bc == B))   // (ar_sample's pick launch already wrote the new rows' embeddings)
    launch_ar_step_embed(tok + r0, c.pf("x_tok_emb.weight"), st.img_embed ? st.img_embed + (size_t)r0 * g.num_cams * c.T * D : nullptr, c.pf("x_pos_emb"), c.fwd_idx,
                         st.d_step, x, Bc, g.num_cams, c.T, D, g.vocab_size + 1, s);
    const size_t layer_bytes = cache_layer_bytes(c, B);
    const size_t chain_off = cache_slot_bytes(c, r0);         // this chain's first cache slot inside a layer
    const int ks = plan.down_ksplit;
    const int wf16 = g.decode_weight_dtype;   // storage kind of the images: 0 fp32, 1 fp16, 2 int8 (+ the layers' row scales)
    float* part = w.part + (size_t)ks * r0 * D;               // [ks][Bc][D] per chain, chains back to back
    float* m1 = w.m1 + (size_t)r0 * 4 * D;
    float* qkv = w.qkv + (size_t)r0 * 3 * D;
    float* xn = w.xn + (size_t)r0 * D;
    RowSrc src;
    src.base = x; src.ld = D;
    for (int i = 0; i < g.num_layers; ++i) {
        const ArLayer& l = c.ar[i];
        float* x2 = ((i & 1) ? w.x2b : w.x2) + (size_t)r0 * D;
        ArAttnFusedArgs a;
        if (plan.split) {   // LayerNorm + QKV projection of the chain's rows in one MFMA kernel (the weight is read once), ln1(x) kept for the residual
            SkinnyFusedArgs pq;
            pq.a_src = &src;
            pq.ln_w = l.ln1_w; pq.ln_b = l.ln1_b; pq.eps = 1e-5f;
            pq.Wp = l.wqkv_wp; pq.w_f16 = wf16; pq.w_scale = l.wqkv_sc; pq.bias = l.bqkv;
            pq.C = qkv; pq.ldc = 3 * D;
            pq.xn_out = xn; pq.ldxn = D;
            pq.M = Bc; pq.N = 3 * D; pq.K = D; pq.ksplit = 1;
            launch_skinny_fused(pq, s);
            a.qkv = qkv; a.xn = xn;
            if (plan.attn_ksplit > 1) { a.ksplit = plan.attn_ksplit; a.kws = w.dec_ws + (size_t)r0 * H * w.splits * 66; }   // (per chain: its sequences' slots of the per-operator path's workspace)
        } else {
            a.x = src;
            a.ln_w = l.ln1_w; a.ln_b = l.ln1_b; a.eps = 1e-5f;
            a.wqkv = l.wqkv; a.bqkv = l.bqkv; a.wqkv_h = l.wqkv_h; a.wqkv_sc = l.wqkv_sc;
            a.ln_cs = l.ln1_cs; a.ln_ds = l.ln1_ds;
        }
        a.kcache = reinterpret_cast<char*>(st.kcache) + i * layer_bytes + chain_off;
        a.vcache = reinterpret_cast<char*>(st.vcache) + i * layer_bytes + chain_off;
        a.kv_dtype = cache_dtype(c); a.sc_off = cache_scale_off(c, B, r0);
        a.bias = c.attn_bias; a.ldbias = L;
        a.vis = c.vis_of_layer(i);
        a.out = x2; a.ldo = D;
        a.B = Bc; a.G = st.G; a.H = H; a.D = D; a.Lmax = L;
        a.n = c.K + 1; a.d_n = st.d_step; a.n_hint = st.step;
        a.prefix = c.K; a.scale = 0.125f;
        a.trace = c.trace;
        launch_ar_attn_fused(a, s);
        if (plan.mlp_fused) {   // ln2 + MLP up + GELU + MLP down in one launch: 8 partial planes (one per XCD) for the next consumer's row fetch
            MlpFusedArgs mf;
            mf.A = x2; mf.lda = D;
            mf.ln_w = l.ln2_w; mf.ln_cs = l.mlp0_cs; mf.ln_ds = l.mlp0_ds; mf.eps = 1e-5f;
            mf.Wup = l.mlp0_wp; mf.Wdn = l.mlp2_wp; mf.w_f16 = wf16; mf.Wup_sc = l.mlp0_sc; mf.Wdn_sc = l.mlp2_sc;
            mf.hidden = m1; mf.C = part;
            mf.sync = c.mlpf_sync; mf.err = c.status_dev;
            mf.M = Bc; mf.D = D;
            mf.trace = c.trace ? c.trace + 4096 * 8 : nullptr;
            launch_ar_mlp_fused(mf, s);
            src = RowSrc{};
            src.base = x2; src.ld = D; src.partial = part; src.ns = MLP_FUSED_PLANES; src.pstride = (long)Bc * D; src.pld = D; src.bias = l.mlp2_b;
            continue;
        }
        SkinnyFusedArgs up;
        up.A = x2; up.lda = D;
        up.ln_w = l.ln2_w; up.ln_b = l.ln2_b; up.eps = 1e-5f;
        up.Wp = l.mlp0_wp; up.w_f16 = wf16; up.w_scale = l.mlp0_sc; up.bias = l.mlp0_b;
        // ln2 folded into the product (skinny_fused_kernel<.., FD>).  Same-box A/B, ms per decode step, folded vs direct: fp16 cache + fp16 weights 0.989-0.994 vs
        // 0.992-0.998, fp16 cache + fp32 weights 1.137-1.151 vs 1.154-1.163, fp32 both 1.447-1.454 vs 1.466-1.482 (profiles/r04_ab_ln2_fold.txt).  $BEVGEN_LN2_FOLD=0: direct form
        if (plan.ln2_fold) { up.ln_cs = l.mlp0_cs; up.ln_ds = l.mlp0_ds; }
        up.C = m1; up.ldc = 4 * D;
        up.M = Bc; up.N = 4 * D; up.K = D; up.ksplit = 1; up.act = ACT_GELU;
        up.trace = c.trace ? c.trace + 4096 * 8 : nullptr;
        launch_skinny_fused(up, s);
        SkinnyFusedArgs dn;
        dn.A = m1; dn.lda = 4 * D;
        dn.Wp = l.mlp2_wp; dn.w_f16 = wf16; dn.w_scale = l.mlp2_sc;
        dn.M = Bc; dn.N = D; dn.K = 4 * D; dn.ksplit = ks;
        dn.trace = c.trace ? c.trace + 2 * 4096 * 8 : nullptr;
        if (ks > 1) {
            dn.C = part;
            src = RowSrc{};
            src.base = x2; src.ld = D; src.partial = part; src.ns = ks; src.pstride = (long)Bc * D; src.pld = D; src.bias = l.mlp2_b;
        } else {   // narrow models: the whole K fits one workgroup; bias here, residual through the row source
            float* hrow = w.h + (size_t)r0 * D;
            dn.C = hrow; dn.ldc = D; dn.bias = l.mlp2_b;
            src = RowSrc{};
            src.base = x2; src.ld = D; src.partial = hrow; src.ns = 1; src.pstride = 0; src.pld = D;
        }
        launch_skinny_fused(dn, s);
    }
    launch_rowsrc_materialize(src, st.hidden + (size_t)r0 * D, Bc, D, counter, s);   // hidden state of the chain's new rows (+ the step counter when this is the only chain)
}

static void decode_step_launch_fused(Ctx& c, StepWs& w, const ArStepPlan& plan, const int64_t* tok, hipStream_t s) {
    auto& st = c.ars;
    const int nch = plan.chains, Bc = plan.Bc;
    if (nch == 1) {
        decode_chain_launch(c, w, plan, tok, 0, st.d_step, s);
        return;
    }
    // fork: chains 1.. on side streams behind everything already enqueued on s; join before the step counter moves (every kernel of the step reads it)
    while ((int)c.chain_streams.size() < nch - 1) {
        hipStream_t q;
        hipEvent_t e;
        HIP_CHECK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c.chain_streams.push_back(q);
        c.chain_join.push_back(e);
    }
    if (!c.chain_fork) HIP_CHECK(hipEventCreateWithFlags(&c.chain_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(c.chain_fork, s));
    for (int k = 1; k < nch; ++k) {
        hipStream_t q = c.chain_streams[k - 1];
        HIP_CHECK(hipStreamWaitEvent(q, c.chain_fork, 0));
        decode_chain_launch(c, w, plan, tok, k * Bc, nullptr, q);
        HIP_CHECK(hipEventRecord(c.chain_join[k - 1], q));
    }
    decode_chain_launch(c, w, plan, tok, 0, nullptr, s);
    for (int k = 1; k < nch; ++k) HIP_CHECK(hipStreamWaitEvent(s, c.chain_join[k - 1], 0));
    launch_increment(st.d_step, s);
}

// one new row through all layers; position / bias row / cache slot are derived from the device-side step counter
static void decode_step_launch(Ctx& c, StepWs& w, const ArStepPlan& plan, const int64_t* tok, hipStream_t s) {
    const auto& g = c.cfg;
    auto& st = c.ars;
    if (plan.fused) {
        decode_step_launch_fused(c, w, plan, tok, s);
        return;
    }
    const int D = c.D, H = c.H, B = st.B, L = c.L;
    launch_ar_step_embed(tok, c.pf("x_tok_emb.weight"), st.img_embed, c.pf("x_pos_emb"), c.fwd_idx, st.d_step, w.x, B, g.num_cams, c.T, D, g.vocab_size + 1, s);
    const size_t layer_bytes = cache_layer_bytes(c, B);
    const float* xin = w.x;
    for (int i = 0; i < g.num_layers; ++i) {
        const ArLayer& l = c.ar[i];
        char* kc = reinterpret_cast<char*>(st.kcache) + i * layer_bytes;
        char* vc = reinterpret_cast<char*>(st.vcache) + i * layer_bytes;
        launch_layernorm(xin, D, l.ln1_w, l.ln1_b, w.xn, D, B, D, 1e-5f, s);
        small_gemm(w.xn, D, l.wqkv, D, l.bqkv, w.qkv, 3 * D, B, 3 * D, D, ACT_NONE, nullptr, 0, w.gemm_ws, s);
        DecodeAttnArgs a;
        a.q = w.qkv; a.ldq = 3 * D;
        a.append_k = w.qkv + D; a.append_v = w.qkv + 2 * D;  // the new row (sequence position K + step) is appended inside the attention kernel
        a.kcache = kc; a.vcache = vc;
        a.bias = c.attn_bias; a.ldbias = L;
        a.vis = c.vis_of_layer(i);
        a.R = w.xn; a.ldr = D; a.O = w.x2; a.ldo = D;
        a.B = B; a.H = H; a.n = c.K + 1; a.d_n = st.d_step; a.n_hint = st.step; a.Lmax = L;
        a.scale = 0.125f; a.kv_dtype = cache_dtype(c);
        launch_decode_attention_ws(a, w.dec_ws, w.splits, s);
        launch_layernorm(w.x2, D, l.ln2_w, l.ln2_b, w.h, D, B, D, 1e-5f, s);
        small_gemm(w.h, D, l.mlp0_w, D, l.mlp0_b, w.m1, 4 * D, B, 4 * D, D, ACT_GELU, nullptr, 0, w.gemm_ws, s);
        small_gemm(w.m1, 4 * D, l.mlp2_w, 4 * D, l.mlp2_b, w.x, D, B, D, 4 * D, ACT_NONE, w.x2, D, w.gemm_ws, s);
        xin = w.x;
    }
    HIP_CHECK(hipMemcpyAsync(st.hidden, w.x, (size_t)B * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    launch_increment(st.d_step, s);
}

void ar_decode_step(Ctx& c, const int64_t* tok, hipStream_t s) {
    auto& st = c.ars;
    BG_REQUIRE(st.B > 0, "bevgen_ar_prefill must be called first");
    BG_REQUIRE(st.step < c.N, "all %d image tokens have already been decoded", c.N);
    c.arena.reset();
    StepWs w = step_ws(c, c.arena, st.B);
    st.pick_embeds = false;   // the caller's tokens: embed them here
    SpinSerial serial(c, s);
    decode_step_launch(c, w, step_plan(c, st.B, st.G), tok, s);
    st.step += 1;
}

void ar_sample(Ctx& c, const int64_t* cond, const float* I_inv, const float* E_inv, int B, int steps, int top_k, float temperature, int greedy,
               const float* noise_u, int samples_per_layout, const int64_t* forced, int64_t* out, float* step_logits, hipStream_t s) {
    BG_REQUIRE(steps >= 1 && steps <= c.N, "steps=%d out of range [1,%d]", steps, c.N);
    BG_REQUIRE(greedy || noise_u, "stochastic sampling needs explicit uniform noise d_noise_u [steps, B]");
    ar_prefill(c, cond, I_inv, E_inv, B, s, samples_per_layout);
    auto& st = c.ars;
    c.step_events_used = 0;   // bevgen_ar_step_times describes THIS call: a call that takes the eager path below reports no steps
    c.arena.reset();
    StepWs w = step_ws(c, c.arena, B);
    const ArStepPlan plan = step_plan(c, B, st.G);
    launch_fill_i64(out, (long)B * c.N, c.cfg.vocab_size, s);  // x = vocab_size everywhere (ar_lm:157)

    // one decode iteration: logits of the newest row -> token -> (optionally) push the token through the stack.
    // Every position-dependent quantity (decode-order index, cache slot, bias row, context length, noise row) is read from the device-side
    // step counter, so the launch sequence is identical for every step and can be captured once and replayed as a hipGraph.
    // (the token's store into `out` and - fused path, one chain - the new row's embedding ride in the pick launch: two launches per step less)
    ArPickTail tail;
    tail.out_all = out; tail.fwd_idx = c.fwd_idx; tail.N = c.N;
    st.pick_embeds = plan.pick_embeds;
    if (st.pick_embeds) {
        tail.tok_emb = c.pf("x_tok_emb.weight"); tail.img_embed = st.img_embed; tail.pos_emb = c.pf("x_pos_emb"); tail.x = w.x;
        tail.C = c.cfg.num_cams; tail.T = c.T; tail.D = c.D; tail.vocab_rows = c.cfg.vocab_size + 1;
    }
    auto head_and_pick = [&](float* lg, hipStream_t q) {
        head_logits(c, w, plan, B, lg, q);
        launch_ar_pick(lg, c.V, greedy ? nullptr : noise_u, st.d_step, forced, w.tok, B, c.V, top_k, temperature, q, &tail);
    };

    const bool use_graph = ar_use_graph(steps, step_logits != nullptr, prof_enabled(), c.disable_graphs);
    SpinSerial serial(c, s);
    if (!use_graph) {
        for (int step = 0; step < steps; ++step) {
            head_and_pick(step_logits ? step_logits + (size_t)step * B * c.V : w.logits, s);
            if (step + 1 < steps) {
                decode_step_launch(c, w, plan, w.tok, s);
                st.step += 1;
            }
        }
        return;
    }

    // graph path: capture {head, pick, store, one full decode step} on a library-owned stream (the caller's stream may be the legacy
    // default stream, which cannot be captured), replay it steps-1 times, finish with one eager head+pick.
    if (!c.graph_stream) {
        HIP_CHECK(hipStreamCreateWithFlags(&c.graph_stream, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&c.graph_ev_in, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&c.graph_ev_out, hipEventDisableTiming));
    }
    hipStream_t q = c.graph_stream;
    HIP_CHECK(hipEventRecord(c.graph_ev_in, s));
    HIP_CHECK(hipStreamWaitEvent(q, c.graph_ev_in, 0));
    serial.q = s;   // (the call's last launches rejoin the caller's stream below: the chain event is recorded there)
    Ctx::GraphKey key;
    key.B = B; key.G = st.G; key.fused = plan.fused; key.split = plan.split; key.chains = plan.chains; key.mlp_fused = plan.mlp_fused; key.top_k = top_k; key.greedy = greedy; key.kv = cache_dtype(c); key.temperature = temperature;
    key.noise = greedy ? nullptr : noise_u; key.forced = forced; key.out = out; key.arena = c.arena.base; key.persist = c.persist.base; key.trace = c.trace;
    if (!c.graph_exec || !(c.graph_key == key)) {
        if (c.graph_exec) c.retire_graph(c.graph_exec, c.graph);
        c.graph_exec = nullptr; c.graph = nullptr;
        hipGraph_t graph = nullptr;
        HIP_CHECK(hipStreamBeginCapture(q, hipStreamCaptureModeThreadLocal));
        try {
            head_and_pick(w.logits, q);
            decode_step_launch(c, w, plan, w.tok, q);
        } catch (...) {
            (void)hipStreamEndCapture(q, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            throw;
        }
        HIP_CHECK(hipStreamEndCapture(q, &graph));
        HIP_CHECK(hipGraphInstantiate(&c.graph_exec, graph, nullptr, nullptr, 0));
        c.graph = graph;
        c.graph_key = key;
    }
    auto stamp = [&]() {
        if (!c.time_steps) return;
        if (c.step_events_used == (int)c.step_events.size()) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            c.step_events.push_back(e);
        }
        HIP_CHECK(hipEventRecord(c.step_events[c.step_events_used++], q));
    };
    stamp();
    for (int step = 0; step + 1 < steps; ++step) {
        HIP_CHECK(hipGraphLaunch(c.graph_exec, q));
        stamp();
    }
    st.step += steps - 1;
    head_and_pick(w.logits, q);
    HIP_CHECK(hipEventRecord(c.graph_ev_out, q));
    HIP_CHECK(hipStreamWaitEvent(s, c.graph_ev_out, 0));
}

// ------------------------------------------------------------------------------------------------ one-pass teacher-forced forward + token scoring
// GPT.forward over the K condition rows AND the first n image rows in decode order (gpt:319-391; shared_step's cross-entropy ar_lm:277-349) as ONE batched pass:
// the prefill's layer loop over R = K + n rows per sequence instead of n single-row decode steps.  Input row K + s embeds ids[b, fwd_idx[s]]; logits row s comes from
// hidden row K - 1 + s.  The mask is causal in decode order, so no computed row sees the pad rows K + N .. L, which are never computed.  The context is left as after
// ar_prefill + n ar_decode_step calls with the same tokens: cache rows [0, R) of every layer, hidden = row R - 1, step counters = n.
//
// Workspace rule.  The layer loop is the outer one, so that the masked bias and the key-tile lists of a layer (keep_heads x R x Rpad floats: 359 MB at config 4 with
// per-head layouts, the largest single item) are built once per LAYER (once per CALL when the layers share a layout) and never per group; the residual stream x of all B
// sequences therefore lives across layers (B x R x D floats).  Everything else of a layer - ln rows, q|k|v, the MLP hidden rows, Q and the fp32 K/V image the flash
// kernel reads: 13 D floats per row - is allocated for one GROUP of Bg = max(1, min(B, 4096 / R)) sequences and reused by the groups in turn: at most 4096 rows, or one
// sequence (2368 rows at config 4), whatever B is.  The head runs in chunks of at most 2048 rows of one sequence.
void ar_forward(Ctx& c, const int64_t* cond, const float* I_inv, const float* E_inv, int B, const int64_t* ids, int n, float* logits, const int64_t* target,
                const float* weight, float* nll, float* loss, hipStream_t s) {
    const auto& g = c.cfg;
    BG_REQUIRE(g.route == BEVGEN_ROUTE_AR, "context was not created for the autoregressive route");
    BG_REQUIRE(B >= 1, "batch must be positive");
    BG_REQUIRE(n >= 1 && n <= c.N, "ar_forward: n_steps=%d out of range [1,%d]", n, c.N);
    const int D = c.D, H = c.H, K = c.K, L = c.L, V = c.V;
    const int R = K + n, Rpad = (int)round_up(R, 32);
    BG_REQUIRE(R <= L, "ar_forward: %d condition + %d image rows exceed the sequence length %d", K, n, L);
    auto& st = c.ars;
    if (step_plan(c, B, 1).needs_split_qkv_image) ctx_pack_split_qkv(c, s);   // decode steps may follow
    ar_state_setup(c, B, s);
    st.G = 1;
    st.pick_embeds = false;

    const int Bg = std::max(1, std::min(B, 4096 / R));
    const size_t rows_g = (size_t)Bg * R;
    const int CH = std::min(n, 2048);   // head chunk (rows of one sequence)
    const int Hk = c.keep_heads;
    const size_t kv_g = (size_t)Bg * H * Rpad * 64;
    float *x, *cx, *xn, *x2, *h, *qkv, *m1, *Q, *tk, *tv, *bias, *hn, *ltile, *wnll;
    uint16_t* tiles;
    c.arena.carve([&](Arena& a) {
        (void)step_ws(c, a, B);   // the decode-step buffers keep their addresses at the start of the arena
        x = a.get<float>((size_t)B * R * D);
        cx = a.get<float>((size_t)B * K * D);
        xn = a.get<float>(rows_g * D);
        x2 = a.get<float>(rows_g * D);
        h = a.get<float>(rows_g * D);
        qkv = a.get<float>(rows_g * 3 * D);
        m1 = a.get<float>(rows_g * 4 * D);
        Q = a.get<float>((size_t)Bg * H * R * 64);
        tk = a.get<float>(kv_g);   // exact fp32 K / V of the group's rows, padded to the attention's key tile (rows R .. Rpad stay zero)
        tv = a.get<float>(kv_g);
        bias = a.get<float>((size_t)Hk * R * Rpad);
        tiles = a.get<uint16_t>(attn_tiles_elems(Hk, R, Rpad));
        hn = a.get<float>((size_t)CH * D);
        ltile = logits ? nullptr : a.get<float>((size_t)CH * V);
        wnll = a.get<float>((size_t)B * n);
    });
    HIP_CHECK(hipMemsetAsync(tk, 0, kv_g * sizeof(float), s));
    HIP_CHECK(hipMemsetAsync(tv, 0, kv_g * sizeof(float), s));

    // ---- embeddings: condition rows [0, K), image rows [K, R) in decode order
    embed_condition(c, cond, I_inv, E_inv, B, 1, nullptr, nullptr, cx, s);
    HIP_CHECK(hipMemcpy2DAsync(x, (size_t)R * D * 4, cx, (size_t)K * D * 4, (size_t)K * D * 4, B, hipMemcpyDeviceToDevice, s));
    launch_ar_seq_embed(ids, c.pf("x_tok_emb.weight"), st.img_embed, c.pf("x_pos_emb"), c.fwd_idx, x, B, n, R, K, c.N, D, g.vocab_size + 1, s);

    // ---- layers
    const size_t layer_bytes = cache_layer_bytes(c, B);
    PrefixRows p{0, R, Rpad, nullptr, xn, x2, h, qkv, m1, Q, tk, tv, Rpad, nullptr, nullptr, bias, tiles, nullptr};
    for (int i = 0; i < g.num_layers; ++i) {
        if (i == 0 || c.keep_layers > 1) build_layer_bias(c, i, bias, tiles, R, Rpad, s);   // shared layout (density 1): one bias image and one set of tile lists per call
        for (int b0 = 0; b0 < B; b0 += Bg) {
            p.nseq = std::min(Bg, B - b0);
            p.x = x + (size_t)b0 * R * D;
            p.kcache = reinterpret_cast<char*>(st.kcache) + i * layer_bytes + cache_slot_bytes(c, b0);   // (fp32, fp16 or int8 codes)
            p.vcache = reinterpret_cast<char*>(st.vcache) + i * layer_bytes + cache_slot_bytes(c, b0);
            prefix_layer(c, i, p, s, cache_scale_off(c, B, b0));
        }
    }

    // ---- state hand-over: as after n decode steps
    launch_gather_rows(x, st.hidden, B, R - 1, R, D, s);
    launch_set_i32(st.d_step, n, s);
    st.step = n;

    // ---- ln_f + head + scoring, per sequence in row chunks: logits row s <- hidden row K - 1 + s.  The SAME chunking whether or not the caller wants the logits (then the
    // head GEMM writes straight into d_logits, else into a tile that the row kernel consumes at once): nll / loss are bit-identical between the two forms
    for (int b = 0; b < B; ++b)
        for (int s0 = 0; s0 < n; s0 += CH) {
            const int rows = std::min(CH, n - s0);
            float* lg = logits ? logits + ((size_t)b * n + s0) * V : ltile;
            launch_layernorm(x + ((size_t)b * R + K - 1 + s0) * D, D, c.pf("ln_f.weight"), c.pf("ln_f.bias"), hn, D, rows, D, 1e-5f, s);
            gemm(hn, D, c.pf("head.weight"), D, nullptr, lg, V, rows, V, D, ACT_NONE, nullptr, 0, s);
            launch_ar_score_rows(lg, V, target, weight, c.fwd_idx, b, s0, rows, c.N, V, nll ? nll + (size_t)b * n + s0 : nullptr, wnll + (size_t)b * n + s0, s);
        }
    if (loss) launch_mean_fixed_order(wnll, (long)B * n, loss, s);
}

// durations of the graph replays of the most recent bevgen_ar_sample (one decode step each), in milliseconds; synchronises the library stream
int ar_step_times(Ctx& c, float* out_ms, int cap) {
    if (c.step_events_used < 2) return 0;
    HIP_CHECK(hipEventSynchronize(c.step_events[c.step_events_used - 1]));
    const int n = std::min(cap, c.step_events_used - 1);
    for (int i = 0; i < n; ++i) HIP_CHECK(hipEventElapsedTime(&out_ms[i], c.step_events[i], c.step_events[i + 1]));
    return n;
}
}  // namespace bevgen
