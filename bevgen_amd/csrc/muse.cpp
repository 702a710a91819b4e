// Route M: MaskGit bidirectional decoder.
//   TransformerMultiView.forward      stage2/muse_maskgit_pytorch.py:283-371
//   TransformerBlocks / Attention     :171-202 / :90-169        FeedForward :78-88
//   MaskGit.generate                  :511-627                   SelfCritic  :388-396
//
// What is hoisted out of the 18-iteration loop (all of it is arithmetic the reference repeats identically 72 times per call):
//   * geometric image embedding + condition (BEV) embedding          (depend only on cameras / cond ids)
//   * cross-attention K/V of every layer (to_kv(context) + l2norm)    (context is never updated)
//   * the attention-bias matrices                                     (built once in bevgen_finalize)
// and what is dropped: the classifier-free-guidance "null" forwards (bit-identical to the conditional ones in eval mode,
// muse_net:352) and the critic forward after the last iteration (its scores are never read).  Opt-in guidance (MaskgitSampling::cond_scale != 1) adds a REAL null pass
// per iteration - context_mask all false - in which a layer's cross-attention block is the constant row c.null_rows[i] (muse_blocks, null_condition).
//
// A forward (muse_blocks) is the token embedding, the layers in ONE of two precisions - muse_blocks_f32, the exact-fp32 path, or muse_blocks_split, the f16x3 path on
// (hi, lo) f16 planes - and the final LayerNorm.  Every LDS-DMA projection of the split path ends in project(), which executes the decision of muse_plan.h.
#include "model.h"
#include "muse_plan.h"

namespace bevgen {

namespace {

struct MuseWs {
    int B = 0;
    int S = 1;   // samples per BEV layout: consecutive groups of S scenes share their condition, whose cross-attention K / V exist once per layout
    bool generate = false;   // the call also needs logits and scores
    bool loss = false;       // MaskGit.forward's losses: logits, the masked ids / mask / counts and one value per token row
    bool guided = false;     // generate with classifier-free guidance: a second logits buffer for the null-condition pass

    long rows = 0;
    float *img = nullptr, *c_embed = nullptr, *context = nullptr;
    int64_t* cond_g = nullptr; float* c_embed_g = nullptr;   // S > 1: the first scene of every group as contiguous [G, ...] inputs of the condition side
    std::vector<float*> crossK, crossV;
    float *logits = nullptr, *scores = nullptr;   // generate only (logits: loss too)
    float* logits_null = nullptr;                 // guided generate only
    int64_t* loss_x = nullptr; uint8_t* loss_mask = nullptr; int* loss_n = nullptr; float* loss_rows = nullptr;   // loss only: x [rows], mask [rows], n [B * cams], nll / bce [rows]
    float *x = nullptr, *xn = nullptr, *qraw = nullptr, *kvraw = nullptr, *Q = nullptr, *Ks = nullptr, *Vs = nullptr, *att = nullptr, *h = nullptr, *g = nullptr;
    size_t kvS = 0, kvC = 0;   // elements of one self- / cross-attention K (or V) buffer: B (or B / S) x H x Nk_pad x 64
    float* attn_ws = nullptr; int attn_ks = 1;   // key-split self-attention of the low-latency path (pick_attn_ksplit): partial rows of the key ranges
    float* kpart = nullptr;   // split-K partial tiles of the narrow (N = D) projections when the batch is too small to fill the chip (low-latency path)
    float *stats_d = nullptr, *stats_f = nullptr;   // folded LayerNorms: per-(32 columns, row) (sum, sum of squares) of the residual rows [D / 32][rows][2] / of the GEGLU rows [Fpad / 32][rows][2]
    float* rowstat = nullptr;                       // ... merged to (mean, rstd) per row [rows][2] by launch_ln_stats_finalize
    void* sk_ws = nullptr;                          // stream-K workspace of the projections (small batches; flags zeroed in muse_prepare), null = never stream-K
    unsigned sk_epoch = 0;                          // bumped per projection launch that carries the workspace
    // the tensors a forward and the sampling loop need by name, looked up once per call (muse_prepare)
    const float *token_emb = nullptr, *pos_emb = nullptr, *norm_g = nullptr, *to_logits = nullptr, *critic_w = nullptr, *critic_b = nullptr;
};

// The switches of muse_plan.h from the environment: ln_fold and ln_merge per call of this function (the tests switch them inside one process), the other four once per process
MuseSwitches muse_switches() {
    static const MuseSwitches once = [] {
        const auto env = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        MuseSwitches s;
        s.qkv_merge = env("BEVGEN_QKV_MERGE", 1);
        s.qkv_wm4 = env("BEVGEN_QKV_WM4", 1);
        s.ksplit = env("BEVGEN_KSPLIT", 0);
        s.attn_ksplit = env("BEVGEN_ATTN_KSPLIT", 0);
        return s;
    }();
    MuseSwitches s = once;
    const char *fold = getenv("BEVGEN_LN_FOLD"), *merge = getenv("BEVGEN_LN_MERGE");
    s.ln_fold = fold ? atoi(fold) : 1;
    s.ln_merge = merge ? (merge[0] == 't' ? 1 : 0) : -1;
    return s;
}

// a buffer that holds the (hi, lo) f16 planes of n elements back to back (same bytes as the fp32 buffer of n elements it replaces): Q, K, V^T of both attentions
struct Planes { _Float16 *hi, *lo; };
Planes planes_of(float* buf, size_t n) { _Float16* hi = reinterpret_cast<_Float16*>(buf); return {hi, hi + n}; }

struct In { const float* p = nullptr; int ld = 0; };   // a row-major fp32 matrix and its row stride
struct Out { float* p = nullptr; int ld = 0; };

// C[M, N] = A[M, K] W[N, K]^T (+ R): what every GEMM of Route M starts from (A: gemm() / on_planes()).  A single-product context (BEVGEN_PRECISION_F16X1) says so here,
// on every launch - the fp32-A ones (cross to_kv, to_logits) included
GemmArgs gemm_args(const Ctx& c, In W, Out C, int M, int N, int K, In R = {}) {
    GemmArgs g;
    g.B = W.p; g.C = C.p; g.R = R.p;
    g.M = M; g.N = N; g.K = K;
    g.ldb = W.ld; g.ldc = C.ld; g.ldr = R.ld;
    g.a_hi_only = c.single_product;
    return g;
}
void gemm(In A, GemmArgs g, hipStream_t s) {
    g.A = A.p; g.lda = A.ld;
    launch_gemm(g, s);
}
// same with A given as interleaved (hi, lo) f16 planes [M][lda/32][2][32] (split-precision mode: the producer kernel wrote them)
GemmArgs on_planes(const void* planes, int lda, GemmArgs g) {
    g.A_hi = reinterpret_cast<const uint16_t*>(planes); g.A_lo = g.A_hi + 32;
    g.lda = lda;
    return g;
}

// folded-LayerNorm roles of a projection (GemmArgs::ln_*): `in` = it consumes raw planes + the statistics of `in_groups` 32-column groups over `in_count` real columns
// (B must then be the W o gamma matrix, cs its row sums); `out_planes` = it produces raw planes + statistics of its own output rows
struct LnFold {
    const float* in_stats = nullptr; const float* in_cs = nullptr;   // consumer: per-row (mean, rstd) [rows][2] and the column sums of W o gamma
    const float* in_gsums = nullptr; int in_groups = 0, in_count = 0; // ... or (small batches) the producer's group sums, merged by the consuming workgroups themselves
    void* out_planes = nullptr; float* out_stats = nullptr; int out_ld = 0;
};
void set_fold(GemmArgs& g, const LnFold* f) {
    if (!f) return;
    g.ln_in_stats = f->in_stats; g.ln_in_cs = f->in_cs;
    g.ln_in_gsums = f->in_gsums; g.ln_in_groups = f->in_groups; g.ln_in_count = f->in_count;
    g.ln_out_planes = f->out_planes; g.ln_out_stats = f->out_stats; g.ln_out_ld = f->out_ld;
    g.ln_rows = g.M;
}

// One forward of the split path: what its three sub-layer functions share
struct Fwd {
    const Ctx& c;
    MuseWs& w;
    hipStream_t s;
    int rows, B, N;
    MuseSwitches sw;
    int fold;          // muse_fold_level
    bool tile_merge;   // muse_tile_merge: the consuming workgroups merge a LayerNorm's group sums themselves
    // fold == 2: the residual-stream projections (to_out of both attention modules, the feed-forward's down-projection) write, besides the fp32 row, the raw planes of the
    // row into w.xn and its statistics into w.stats_d: the next projection multiplies them by W o gamma.  `x_planes_ready`: w.xn / w.stats_d hold the current w.x
    bool x_planes_ready = false;
    LnFold prod_x;     // producer role of a residual-stream projection
};

// consumer role behind a folded LayerNorm over `count` real columns in `groups` 32-column groups (launches the merge kernel unless the consumer's tiles merge)
LnFold consumer(const Fwd& f, const float* gsums, int groups, int count, const float* cs) {
    LnFold r;
    r.in_cs = cs;
    if (f.tile_merge) { r.in_gsums = gsums; r.in_groups = groups; r.in_count = count; }
    else { launch_ln_stats_finalize(gsums, f.w.rowstat, f.rows, groups, count, 1e-5f, f.s); r.in_stats = f.w.rowstat; }
    return r;
}

// THE launch of an LDS-DMA projection of the split path: `g` with its operands and fused epilogue as the table's last column wants them, the rest by muse_proj_plan
void project(Fwd& f, MuseProj kind, GemmArgs g, const LnFold* fold = nullptr, bool merged = false) {
    MuseWs& w = f.w;
    MuseProjIn in;
    in.kind = kind; in.M = g.M; in.N = g.N; in.K = g.K;
    in.fold_role = fold != nullptr; in.merged = merged;
    in.has_kpart = w.kpart != nullptr; in.has_sk_ws = w.sk_ws != nullptr;   // (qraw, the un-fused q projection's output, is part of every workspace)
    const MuseProjPlan p = muse_proj_plan(in, f.sw, glds_switches());
    if (p.q_unfused) {   // small batch: the projection split over K into qraw, then the query preparation as its own (tiny) kernel
        GemmArgs r = on_planes(g.A_hi, g.lda, gemm_args(f.c, {g.B, g.ldb}, {w.qraw, g.N}, g.M, g.N, g.K));
        r.ksplit = p.ksplit; r.kpart = w.kpart;
        launch_gemm(r, f.s);
        launch_muse_q_prep_split(w.qraw, g.epi_scale, g.epi_hi, g.epi_lo, g.M / g.epi_rows, g.epi_heads, g.epi_rows, g.epi_post, f.s);
        return;
    }
    if (p.kpart) { g.ksplit = p.ksplit; g.kpart = w.kpart; }
    set_fold(g, fold);
    if (p.sk) { g.sk_ws = w.sk_ws; g.sk_epoch = ++w.sk_epoch; }
    g.force_wm = p.force_wm;
    launch_gemm(g, f.s);
}

// to_q over the LayerNorm planes in w.xn with the query preparation (l2norm, q_scale, hi/lo split, head-major layout) fused into the GEMM epilogue
GemmArgs q_args(const Fwd& f, const float* W, const float* q_scale) {
    const int D = f.c.D, H = f.c.H;
    const Planes Q = planes_of(f.w.Q, (size_t)f.rows * D);
    GemmArgs g = on_planes(f.w.xn, D, gemm_args(f.c, {W, D}, {nullptr, H * 64}, f.B * f.N, H * 64, D));
    g.epi = EPI_MUSE_Q; g.epi_scale = q_scale; g.epi_hi = Q.hi; g.epi_lo = Q.lo; g.epi_rows = f.N; g.epi_heads = H;
    g.epi_post = 8.0f * kLog2e;   // sim = 8 q.k (muse_net:150) in the base-2 domain of the split attention kernel
    return g;
}

// the split attention kernel over the prepared Q planes; output as the planes of the [rows, D] matrix the to_out projection reads
AttnSplitArgs attn_args(const Fwd& f, Planes K, Planes VT, int Nk_pad) {
    const Planes Q = planes_of(f.w.Q, (size_t)f.rows * f.c.D);
    AttnSplitArgs sa{};
    sa.Qh = Q.hi; sa.Ql = Q.lo; sa.Kh = K.hi; sa.Kl = K.lo; sa.VTh = VT.hi; sa.VTl = VT.lo;
    sa.O = f.w.att; sa.B = f.B; sa.H = f.c.H; sa.Nq = f.N; sa.Nk_pad = Nk_pad;
    sa.bias_head_stride = 0; sa.scale = 8.0f * kLog2e;
    sa.o_bstride = (long)f.N * f.c.D; sa.o_qstride = f.c.D; sa.o_hstride = 64;
    sa.Op = reinterpret_cast<_Float16*>(f.w.att);
    return sa;
}

// x += to_out(attention(LayerNorm(x))) over the tokens themselves.  Every GEMM input is produced directly as (hi, lo) f16 planes (same bytes as the fp32 buffer they replace)
void self_attention_split(Fwd& f, const MuseLayer& l) {
    const Ctx& c = f.c;
    MuseWs& w = f.w;
    const int D = c.D, rows = f.rows;
    const bool f0 = f.fold == 2 && f.x_planes_ready;   // (layer 0 reads the embedding: no projection produced it - its first LayerNorm stays a kernel)
    LnFold cons_x;   // consumer role behind a LayerNorm over the D residual columns
    if (!f0) launch_layernorm_planes(w.x, D, l.norm_g[0], nullptr, w.xn, D, rows, D, 1e-5f, f.s);
    else cons_x = consumer(f, w.stats_d, D / 32, D, nullptr);
    const bool merged = l.to_qkv_self && muse_qkv_merged(f.sw, rows);
    if (!merged) {
        cons_x.in_cs = l.fold_q_self_cs;
        project(f, PROJ_Q, q_args(f, f0 ? l.fold_q_self : l.to_q[0], l.q_scale[0]), f0 ? &cons_x : nullptr);
    }
    // to_kv (merged: q | k | v) with the key / value preparation in its epilogue: k planes [B, H, NkS_pad, 64], v planes transposed [B, H, 64, NkS_pad]
    const Planes K = planes_of(w.Ks, w.kvS), VT = planes_of(w.Vs, w.kvS);
    const float* W = merged ? (f0 ? l.fold_qkv : l.to_qkv_self) : (f0 ? l.fold_kv_self : l.to_kv[0]);
    const int Nkv = (merged ? 3 : 2) * D;
    GemmArgs gk = on_planes(w.xn, D, gemm_args(c, {W, D}, {nullptr, Nkv}, rows, Nkv, D));
    gk.epi = merged ? EPI_MUSE_QKV : EPI_MUSE_KV;
    gk.epi_scale = l.k_scale[0]; gk.epi_hi = K.hi; gk.epi_lo = K.lo; gk.epi_hi2 = VT.hi; gk.epi_lo2 = VT.lo;
    gk.epi_aux = l.null_self; gk.epi_rows = f.N; gk.epi_heads = c.H; gk.epi_ld = c.NkS_pad;
    if (merged) {
        const Planes Q = planes_of(w.Q, (size_t)rows * D);
        gk.epi_qh = Q.hi; gk.epi_ql = Q.lo; gk.epi_qscale = l.q_scale[0];
        gk.epi_post = 8.0f * kLog2e;   // sim = 8 q.k (muse_net:150) in the base-2 domain of the split attention kernel
    }
    cons_x.in_cs = merged ? l.fold_qkv_cs : l.fold_kv_self_cs;
    project(f, PROJ_KV, gk, f0 ? &cons_x : nullptr, merged);
    AttnSplitArgs sa = attn_args(f, K, VT, c.NkS_pad);
    sa.bias = c.bias_self; sa.bias_pk = c.bias_self_pk; sa.ldbias = c.ldS;
    sa.ksplit = w.attn_ks; sa.kws = w.attn_ws;
    launch_attention_split(sa, f.s);
    project(f, PROJ_OUT, on_planes(w.att, D, gemm_args(c, {l.to_out[0], D}, {w.x, D}, rows, D, D, {w.x, D})), f.fold == 2 ? &f.prod_x : nullptr);   // x = to_out(att) + x
}

// x += to_out(attention(LayerNorm(x))) over layer i's keys / values of the condition (muse_prepare)
void cross_attention_split(Fwd& f, const MuseLayer& l, int i) {
    const Ctx& c = f.c;
    MuseWs& w = f.w;
    const int D = c.D, rows = f.rows;
    LnFold cons_x;
    if (f.fold != 2) launch_layernorm_planes(w.x, D, l.norm_g[1], nullptr, w.xn, D, rows, D, 1e-5f, f.s);
    else cons_x = consumer(f, w.stats_d, D / 32, D, l.fold_q_cross_cs);
    project(f, PROJ_Q, q_args(f, f.fold == 2 ? l.fold_q_cross : l.to_q[1], l.q_scale[1]), f.fold == 2 ? &cons_x : nullptr);
    AttnSplitArgs sa = attn_args(f, planes_of(w.crossK[i], w.kvC), planes_of(w.crossV[i], w.kvC), c.NkC_pad);   // (the cross-attention's 9 key tiles stay one range)
    sa.bias = c.bias_cross; sa.bias_pk = c.bias_cross_pk; sa.ldbias = c.ldC;
    sa.kv_group = w.S;   // the samples of a layout read the layout's cross-attention K / V
    launch_attention_split(sa, f.s);
    project(f, PROJ_OUT, on_planes(w.att, D, gemm_args(c, {l.to_out[1], D}, {w.x, D}, rows, D, D, {w.x, D})), f.fold == 2 ? &f.prod_x : nullptr);
}

// x += W4 LayerNorm(GEGLU(W1 LayerNorm(x))) (muse_net:78-88); `last`: no layer follows.  `null_row` (null-condition pass, fold <= 1): x += null_row first, in the
// launch of the first LayerNorm - the whole cross-attention block of that pass
void feed_forward_split(Fwd& f, const MuseLayer& l, bool last, const float* null_row = nullptr) {
    const Ctx& c = f.c;
    MuseWs& w = f.w;
    const int D = c.D, rows = f.rows, fold = f.fold;
    if (null_row) launch_add_row_layernorm(w.x, D, null_row, l.ff_g0, w.xn, D, rows, D, 1e-5f, true, f.s);
    else if (fold != 2) launch_layernorm_planes(w.x, D, l.ff_g0, nullptr, w.xn, D, rows, D, 1e-5f, f.s);
    if (l.ff_w1_geglu) {
        // GEGLU in the up-projection's epilogue: h = gate * gelu(x) as [rows, Fpad] (pad columns exactly 0), then the LayerNorm half on its own - or (fold >= 1)
        // folded away: the epilogue writes the raw planes of h and its row statistics, the down-projection multiplies by W4 o gamma
        GemmArgs ge = on_planes(w.xn, D, gemm_args(c, {fold == 2 ? l.fold_w1 : l.ff_w1_geglu, D}, {w.h, c.Fpad}, rows, 2 * c.Fpad, D));
        ge.epi = EPI_GEGLU;
        LnFold fg;
        if (fold == 2) fg = consumer(f, w.stats_d, D / 32, D, l.fold_w1_cs);
        if (fold >= 1) { fg.out_planes = w.g; fg.out_stats = w.stats_f; fg.out_ld = c.Fpad; }
        project(f, PROJ_GEGLU, ge, fold >= 1 ? &fg : nullptr);
        if (fold == 0) launch_layernorm_planes(w.h, c.Fpad, l.ff_g3, nullptr, w.g, c.Fpad, rows, c.F, 1e-5f, f.s);
    } else {
        project(f, PROJ_UP, on_planes(w.xn, D, gemm_args(c, {l.ff_w1, D}, {w.h, 2 * c.F}, rows, 2 * c.F, D)));
        launch_geglu_layernorm_planes(w.h, 2 * c.F, l.ff_g3, w.g, c.Fpad, rows, c.F, 1e-5f, f.s);
    }
    LnFold fd;   // the down-projection: consumer of the inner LayerNorm (fold >= 1), producer for the next layer's first LayerNorm (fold == 2, not behind the last layer)
    if (fold >= 1 && l.ff_w1_geglu) fd = consumer(f, w.stats_f, c.Fpad / 32, c.F, l.fold_w4_cs);
    const bool prod_next = fold == 2 && !last;
    if (prod_next) { fd.out_planes = w.xn; fd.out_stats = w.stats_d; fd.out_ld = D; }
    const bool cons = fd.in_stats || fd.in_gsums, any = cons || fd.out_planes;
    project(f, PROJ_OUT, on_planes(w.g, c.Fpad, gemm_args(c, {cons ? l.fold_w4 : l.ff_w4_padded, c.Fpad}, {w.x, D}, rows, D, c.Fpad, {w.x, D})), any ? &fd : nullptr);
    f.x_planes_ready = prod_next;
}

// the layers in split precision (f16x3; f16x1 and weights = f16 are this path with other weight planes)
void muse_blocks_split(const Ctx& c, MuseWs& w, hipStream_t s, bool null_condition) {
    Fwd f{c, w, s, (int)w.rows, w.B, c.N, muse_switches()};
    f.fold = muse_fold_level(f.sw, !c.muse.empty() && c.muse[0].fold_w4);
    // (the null-condition pass adds a row to x between the self-attention's output projection and the feed-forward's first LayerNorm: planes and statistics that
    // projection would produce at fold level 2 describe the row before the add, so that pass runs at level <= 1)
    if (null_condition) f.fold = std::min(f.fold, 1);
    f.tile_merge = muse_tile_merge(f.sw, f.rows);
    f.prod_x.out_planes = w.xn; f.prod_x.out_stats = w.stats_d; f.prod_x.out_ld = c.D;
    const int layers = c.cfg.num_layers;
    for (int i = 0; i < layers; ++i) {
        const MuseLayer& l = c.muse[i];
        self_attention_split(f, l);
        if (!null_condition) cross_attention_split(f, l, i);
        feed_forward_split(f, l, i + 1 == layers, null_condition ? c.null_rows + (size_t)i * c.D : nullptr);
    }
}

// the layers in exact fp32: sixteen launches per layer (null-condition pass: eleven - the cross-attention block and the LayerNorm behind it are one launch)
void muse_blocks_f32(const Ctx& c, MuseWs& w, hipStream_t s, bool null_condition) {
    const int D = c.D, H = c.H, B = w.B, N = c.N, F = c.F, Fpad = c.Fpad, rows = (int)w.rows;
    AttnArgs self{};
    self.Q = w.Q; self.K = w.Ks; self.V = w.Vs; self.bias = c.bias_self; self.R = nullptr; self.O = w.att;
    self.B = B; self.H = H; self.Nq = N; self.Nk_pad = c.NkS_pad;
    self.q_bstride = (long)H * N * 64; self.q_hstride = (long)N * 64;
    self.kv_bstride = (long)H * c.NkS_pad * 64; self.kv_hstride = (long)c.NkS_pad * 64;
    self.ldbias = c.ldS; self.bias_head_stride = 0; self.scale = 8.0f;
    self.o_bstride = (long)N * D; self.o_qstride = D; self.o_hstride = 64;
    AttnArgs cross = self;
    cross.bias = c.bias_cross; cross.Nk_pad = c.NkC_pad; cross.ldbias = c.ldC;
    cross.kv_bstride = (long)H * c.NkC_pad * 64; cross.kv_hstride = (long)c.NkC_pad * 64;
    cross.kv_group = w.S;   // the samples of a layout read the layout's cross-attention K / V
    for (int i = 0; i < c.cfg.num_layers; ++i) {
        const MuseLayer& l = c.muse[i];
        // ---- self attention
        launch_layernorm(w.x, D, l.norm_g[0], nullptr, w.xn, D, rows, D, 1e-5f, s);
        gemm({w.xn, D}, gemm_args(c, {l.to_q[0], D}, {w.qraw, D}, rows, D, D), s);
        gemm({w.xn, D}, gemm_args(c, {l.to_kv[0], D}, {w.kvraw, 2 * D}, rows, 2 * D, D), s);
        launch_muse_q_prep(w.qraw, l.q_scale[0], w.Q, B, H, N, s);
        launch_muse_kv_prep(w.kvraw, l.null_kv[0], l.k_scale[0], w.Ks, w.Vs, B, H, N, c.NkS_pad, s);
        launch_attention(self, s);
        gemm({w.att, D}, gemm_args(c, {l.to_out[0], D}, {w.x, D}, rows, D, D, {w.x, D}), s);   // x = to_out(att) + x
        if (null_condition) {
            // ---- cross attention over no visible key (x += r_i) and the feed-forward's first LayerNorm
            launch_add_row_layernorm(w.x, D, c.null_rows + (size_t)i * D, l.ff_g0, w.xn, D, rows, D, 1e-5f, false, s);
        } else {
            // ---- cross attention
            launch_layernorm(w.x, D, l.norm_g[1], nullptr, w.xn, D, rows, D, 1e-5f, s);
            gemm({w.xn, D}, gemm_args(c, {l.to_q[1], D}, {w.qraw, D}, rows, D, D), s);
            launch_muse_q_prep(w.qraw, l.q_scale[1], w.Q, B, H, N, s);
            cross.K = w.crossK[i]; cross.V = w.crossV[i];
            launch_attention(cross, s);
            gemm({w.att, D}, gemm_args(c, {l.to_out[1], D}, {w.x, D}, rows, D, D, {w.x, D}), s);
            // ---- feed forward
            launch_layernorm(w.x, D, l.ff_g0, nullptr, w.xn, D, rows, D, 1e-5f, s);
        }
        gemm({w.xn, D}, gemm_args(c, {l.ff_w1, D}, {w.h, 2 * F}, rows, 2 * F, D), s);
        launch_geglu_layernorm(w.h, 2 * F, l.ff_g3, w.g, Fpad, rows, F, 1e-5f, s);
        gemm({w.g, Fpad}, gemm_args(c, {l.ff_w4_padded, Fpad}, {w.x, D}, rows, D, Fpad, {w.x, D}), s);
    }
}

// The workspace of a Route M call (w.B, w.S, w.rows and w.generate set): the one description of it, run twice by Arena::carve (the rule is in arena.h)
void muse_layout(const Ctx& c, MuseWs& w, Arena& a) {
    const auto& g = c.cfg;
    const MuseSwitches sw = muse_switches();
    const int D = c.D, H = c.H, B = w.B, G = B / w.S;
    w.img = g.image_embed ? a.get<float>((size_t)w.rows * D) : nullptr;
    w.c_embed = g.image_embed ? a.get<float>((size_t)B * g.num_cams * D) : nullptr;
    w.context = a.get<float>((size_t)G * c.K * D);
    w.x = a.get<float>((size_t)w.rows * D);
    w.xn = a.get<float>((size_t)w.rows * D);
    w.qraw = a.get<float>((size_t)w.rows * D);
    w.att = a.get<float>((size_t)w.rows * D);
    w.kvraw = a.get<float>((size_t)std::max<long>(w.rows, (long)B * c.K) * 2 * D);
    w.Q = a.get<float>((size_t)w.rows * D);
    w.kvS = (size_t)B * H * c.NkS_pad * 64;
    w.Ks = a.get<float>(w.kvS);
    w.Vs = a.get<float>(w.kvS);
    w.h = a.get<float>((size_t)w.rows * 2 * c.F);
    w.g = a.get<float>((size_t)w.rows * c.Fpad);
    w.kpart = muse_needs_kpart(w.rows, D, c.Fpad, sw) ? a.get<float>((size_t)kMuseKsplitMax * w.rows * D) : nullptr;
    w.attn_ks = pick_attn_ksplit((long)cdiv(c.N, 256) * H * B, c.NkS_pad / 32, sw.attn_ksplit);
    w.attn_ws = w.attn_ks > 1 ? a.get<float>((size_t)attn_split_ws_floats(B, H, c.N, w.attn_ks)) : nullptr;
    w.stats_d = a.get<float>((size_t)w.rows * 2 * (D / 32));
    w.stats_f = a.get<float>((size_t)w.rows * 2 * (c.Fpad / 32));
    w.rowstat = a.get<float>((size_t)w.rows * 2);
    w.sk_ws = w.rows <= kMuseSkMaxRows && g.precision == BEVGEN_PRECISION_F16X3 ? a.alloc(gemm_sk_ws_bytes()) : nullptr;
    w.cond_g = w.S > 1 ? a.get<int64_t>((size_t)G * c.K) : nullptr;
    w.c_embed_g = w.S > 1 && g.image_embed ? a.get<float>((size_t)G * g.num_cams * D) : nullptr;
    w.kvC = (size_t)G * H * c.NkC_pad * 64;
    w.crossK.resize(g.num_layers);
    w.crossV.resize(g.num_layers);
    for (int i = 0; i < g.num_layers; ++i) {
        w.crossK[i] = a.get<float>(w.kvC);
        w.crossV[i] = a.get<float>(w.kvC);
    }
    w.logits = w.generate || w.loss ? a.get<float>((size_t)w.rows * c.V) : nullptr;
    w.logits_null = w.guided ? a.get<float>((size_t)w.rows * c.V) : nullptr;
    w.scores = w.generate ? a.get<float>((size_t)w.rows) : nullptr;
    w.loss_x = w.loss ? a.get<int64_t>((size_t)w.rows) : nullptr;
    w.loss_mask = w.loss ? a.get<uint8_t>((size_t)w.rows) : nullptr;
    w.loss_n = w.loss ? a.get<int>((size_t)B * g.num_cams) : nullptr;
    w.loss_rows = w.loss ? a.get<float>((size_t)w.rows) : nullptr;
}

// per-batch constants: the workspace, the tensors used by name, embeddings + cross-attention K/V
void muse_prepare(Ctx& c, MuseWs& w, const MuseBatch& in, bool generate, hipStream_t s, bool loss = false, bool guided = false) {
    const auto& g = c.cfg;
    const std::string p = "transformer.";
    const int B = in.B, S = in.samples_per_layout < 1 ? 1 : in.samples_per_layout;
    BG_REQUIRE(B % S == 0, "batch %d is not a multiple of samples_per_layout %d", B, S);
    const int G = B / S;   // BEV layouts: the condition side (context embedding, cross-attention K / V of every layer) is built once per layout
    w.S = S;
    w.B = B;
    w.generate = generate;
    w.loss = loss;
    w.guided = guided;
    w.rows = (long)B * c.N;
    c.arena.carve([&](Arena& a) { muse_layout(c, w, a); });
    w.token_emb = c.pf(p + "token_emb.weight"); w.pos_emb = c.pf(p + "pos_emb.weight");
    w.norm_g = c.pf(p + "transformer_blocks.norm.gamma"); w.to_logits = c.pf(p + "to_logits.weight");
    if (c.find("token_critic.to_pred.weight")) { w.critic_w = c.pf("token_critic.to_pred.weight"); w.critic_b = c.pf("token_critic.to_pred.bias"); }
    const int D = c.D, H = c.H;
    if (w.sk_ws) {
        HIP_CHECK(hipMemsetAsync(w.sk_ws, 0, 1024 * sizeof(unsigned), s));   // the flag words: a flag equal to a launch's epoch means "published in this launch"
        w.sk_epoch = 0;
    }
    HIP_CHECK(hipMemsetAsync(w.Ks, 0, w.kvS * sizeof(float), s));  // rows beyond the real keys stay zero
    HIP_CHECK(hipMemsetAsync(w.Vs, 0, w.kvS * sizeof(float), s));

    if (g.image_embed)
        launch_camera_embed(in.I_inv, in.E_inv, c.image_plane, c.pf(p + "img_embed.weight"), c.pf(p + "cam_embed.weight"), w.img, w.c_embed, B, g.num_cams, c.T, D, s);
    const int64_t* cond_g = in.cond;
    const float* c_embed_g = w.c_embed;
    if (S > 1) {   // the first scene of every group -> contiguous [G, ...] inputs of the condition side
        HIP_CHECK(hipMemcpy2DAsync(w.cond_g, (size_t)c.K * 8, in.cond, (size_t)S * c.K * 8, (size_t)c.K * 8, G, hipMemcpyDeviceToDevice, s));
        cond_g = w.cond_g;
        if (w.c_embed) {
            HIP_CHECK(hipMemcpy2DAsync(w.c_embed_g, (size_t)g.num_cams * D * 4, w.c_embed, (size_t)S * g.num_cams * D * 4, (size_t)g.num_cams * D * 4, G, hipMemcpyDeviceToDevice, s));
            c_embed_g = w.c_embed_g;
        }
    }
    launch_cond_embed(cond_g, c.pf(p + "cond_token_emb.weight"), c.pf(p + "cond_pos_emb.weight"), g.bev_embed ? c.pf(p + "bev_grid") : nullptr,
                      g.bev_embed ? c.pf(p + "bev_embed.weight") : nullptr, g.bev_embed ? c.pf(p + "bev_embed.bias") : nullptr,
                      g.bev_embed ? c.pf(p + "bev_cam_pos_emb") : nullptr, c_embed_g, w.context, G, g.num_cams, c.K, D, g.cond_vocab_size, s);

    // cross-attention keys/values: to_kv(context) (context is NOT layer-normed, muse_net:128-132), null kv prepended, k l2-normalised
    for (int i = 0; i < g.num_layers; ++i) {
        HIP_CHECK(hipMemsetAsync(w.crossK[i], 0, w.kvC * sizeof(float), s));
        HIP_CHECK(hipMemsetAsync(w.crossV[i], 0, w.kvC * sizeof(float), s));
        const MuseLayer& l = c.muse[i];
        gemm({w.context, D}, gemm_args(c, {l.to_kv[1], D}, {w.kvraw, 2 * D}, G * c.K, 2 * D, D), s);
        if (c.cfg.precision == BEVGEN_PRECISION_F16X3) {
            const Planes K = planes_of(w.crossK[i], w.kvC), VT = planes_of(w.crossV[i], w.kvC);
            launch_muse_kv_prep_split(w.kvraw, l.null_kv[1], l.k_scale[1], K.hi, K.lo, VT.hi, VT.lo, G, H, c.K, c.NkC_pad, s);
        } else {
            launch_muse_kv_prep(w.kvraw, l.null_kv[1], l.k_scale[1], w.crossK[i], w.crossV[i], G, H, c.K, c.NkC_pad, s);
        }
    }
}

// one transformer pass over the current ids: leaves LayerNorm(x) (= `embed`, muse_net:202) in w.xn.  The two precisions share the token embedding and the final LayerNorm.
// null_condition: the pass with context_mask = False for every scene (muse_net:158-166, 352-356: what a dropped condition is) - each layer's cross-attention block is
// x += c.null_rows[i], fused into the feed-forward's first LayerNorm (launch_add_row_layernorm); everything else is the same launches
void muse_blocks(const Ctx& c, MuseWs& w, const int64_t* ids, hipStream_t s, bool null_condition = false) {
    const int D = c.D, rows = (int)w.rows;
    launch_token_embed(ids, w.token_emb, w.img, w.pos_emb, w.x, w.B, c.N, D, c.cfg.vocab_size + 1, s);
    if (c.cfg.precision == BEVGEN_PRECISION_F16X3) muse_blocks_split(c, w, s, null_condition);
    else muse_blocks_f32(c, w, s, null_condition);
    launch_layernorm(w.x, D, w.norm_g, nullptr, w.xn, D, rows, D, 1e-5f, s);
}

}  // namespace

void muse_forward(Ctx& c, const MuseBatch& in, const int64_t* ids, float* logits, float* embed, hipStream_t s, bool null_condition) {
    BG_REQUIRE(c.cfg.route == BEVGEN_ROUTE_MASKGIT, "context was not created for the MaskGit route");
    BG_REQUIRE(in.B >= 1, "batch must be positive");
    MuseWs w;
    muse_prepare(c, w, in, false, s);
    muse_blocks(c, w, ids, s, null_condition);
    const int rows = (int)w.rows;
    if (embed) HIP_CHECK(hipMemcpyAsync(embed, w.xn, (size_t)rows * c.D * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (logits) gemm({w.xn, c.D}, gemm_args(c, {w.to_logits, c.D}, {logits, c.V}, rows, c.V, c.D), s);
}

void maskgit_generate(Ctx& c, const MuseBatch& in, const MaskgitSampling& sp, int64_t* out, hipStream_t s) {
    const int timesteps = sp.timesteps, score_mode = sp.score_mode;
    BG_REQUIRE(c.cfg.route == BEVGEN_ROUTE_MASKGIT, "context was not created for the MaskGit route");
    BG_REQUIRE(in.B >= 1 && timesteps >= 1 && sp.sched, "bad generate arguments");
    BG_REQUIRE(score_mode != 0 || c.find("token_critic.to_pred.weight"), "maskgit_generate: the context holds no token critic (token_critic.to_pred.*): use score_mode 1 / 2");
    BG_REQUIRE(score_mode >= 0 && score_mode <= 2, "score_mode %d: 0 token critic, 1 softmax confidence, 2 softmax confidence with re-masking of earlier tokens", score_mode);
    const bool guided = sp.cond_scale != 1.f;   // (scale 1 is the conditional logits: the launches of an unguided call)
    MuseWs w;
    muse_prepare(c, w, in, true, s, false, guided);
    const int rows = (int)w.rows;            // B*C*T token rows
    const int seqs = in.B * c.cfg.num_cams;  // rows of the [B*C, T] id matrix
    const int T = c.T, V = c.V, D = c.D;
    float *logits = w.logits, *scores = w.scores;
    const int64_t mask_id = c.cfg.vocab_size;
    int64_t* ids = out;  // generation happens in the caller's output buffer
    launch_fill_i64(ids, rows, mask_id, s);
    launch_fill(scores, rows, 0.f, s);
    for (int step = 0; step < timesteps; ++step) {
        const int steps_until_x0 = timesteps - 1 - step;
        const double frac = (double)steps_until_x0 / (double)timesteps;
        launch_remask(ids, scores, sp.init_ids, seqs, T, sp.sched[step], mask_id, s);
        muse_blocks(c, w, ids, s);
        gemm({w.xn, D}, gemm_args(c, {w.to_logits, D}, {logits, V}, rows, V, D), s);
        if (guided) {   // the null-condition pass over the same ids; from here on `logits` holds null + (cond - null) * cond_scale (top-k filter, pick and confidence scores)
            muse_blocks(c, w, ids, s, true);
            gemm({w.xn, D}, gemm_args(c, {w.to_logits, D}, {w.logits_null, V}, rows, V, D), s);
            launch_cfg_combine(logits, V, w.logits_null, V, rows, V, sp.cond_scale, s);
        }
        // score_mode 1 / 2 (force_not_use_token_critic, muse_net:611-622): the scores come out of the pick itself (1 - softmax(logits)[pred]) and the critic forward
        // is not run at all - 18 transformer forwards per call instead of 35
        launch_maskgit_pick(ids, logits, V, sp.gumbel_u ? sp.gumbel_u + (size_t)step * rows * V : nullptr, rows, V, sp.topk_k, (float)((double)sp.temperature * frac), mask_id, s,
                            sp.noise_seed, (unsigned)step, score_mode ? scores : nullptr, score_mode);
        if (score_mode == 0 && step + 1 < timesteps) {  // the critic scores only select what the NEXT iteration re-masks (guided too: the critic reads the conditional embed, muse_net:394-396)
            muse_blocks(c, w, ids, s);
            launch_critic_scores(w.xn, D, w.critic_w, w.critic_b, sp.critic_u ? sp.critic_u + (size_t)step * rows : nullptr, sp.critic_noise_scale, (float)frac, scores, rows, D, s,
                                 sp.noise_seed, (unsigned)step);
        }
    }
}

// MaskGit.forward in eval mode (muse_net:629-729): mask, forward, masked cross-entropy; with the self critic the gumbel pick at the masked positions, a second forward
// (embed only: the head is not run) and the critic's BCE.  Every reduction is a fixed-order double sum: two calls give the same bits.
void maskgit_loss(Ctx& c, const MuseBatch& in, const int64_t* ids, const MaskgitLoss& lp, hipStream_t s) {
    BG_REQUIRE(c.cfg.route == BEVGEN_ROUTE_MASKGIT, "context was not created for the MaskGit route");
    BG_REQUIRE(in.B >= 1 && ids && lp.h_num_masked && lp.out, "bad maskgit_loss arguments");
    BG_REQUIRE(lp.perm_u || lp.noise_seed, "maskgit_loss: neither d_perm_u nor a noise_seed: a mask needs randomness");
    BG_REQUIRE(!lp.with_critic || lp.gumbel_u || lp.noise_seed, "maskgit_loss: the critic input is a gumbel sample: neither d_gumbel_u nor a noise_seed");
    BG_REQUIRE(!lp.with_critic || c.find("token_critic.to_pred.weight"), "maskgit_loss: the context holds no token critic (token_critic.to_pred.*): call with with_critic = 0");
    const int seqs = in.B * c.cfg.num_cams, T = c.T, V = c.V, D = c.D;
    long masked = 0;
    for (int r = 0; r < seqs; ++r) {
        BG_REQUIRE(lp.h_num_masked[r] >= 1 && lp.h_num_masked[r] <= T, "maskgit_loss: h_num_masked[%d]=%d outside [1, %d]", r, lp.h_num_masked[r], T);
        masked += lp.h_num_masked[r];
    }
    MuseWs w;
    muse_prepare(c, w, in, false, s, true);
    const long rows = w.rows;
    const int64_t mask_id = c.cfg.vocab_size;
    HIP_CHECK(hipMemcpyAsync(w.loss_n, lp.h_num_masked, (size_t)seqs * sizeof(int), hipMemcpyHostToDevice, s));   // (a few hundred bytes of pageable memory: the runtime copies them to its staging buffer before the call returns)
    launch_maskgit_train_mask(ids, lp.perm_u, w.loss_n, w.loss_x, w.loss_mask, seqs, T, mask_id, lp.noise_seed, s);
    if (lp.mask_out) HIP_CHECK(hipMemcpyAsync(lp.mask_out, w.loss_mask, (size_t)rows, hipMemcpyDeviceToDevice, s));
    if (lp.x_out) HIP_CHECK(hipMemcpyAsync(lp.x_out, w.loss_x, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    muse_blocks(c, w, w.loss_x, s);
    gemm({w.xn, D}, gemm_args(c, {w.to_logits, D}, {w.logits, V}, (int)rows, V, D), s);
    launch_maskgit_ce_rows(w.logits, V, ids, w.loss_mask, w.loss_rows, rows, V, s);
    launch_mean_fixed_order(w.loss_rows, rows, lp.out + 1, s, masked);
    if (lp.with_critic) {
        // gumbel_sample over all V logits (no top-k, muse_net:713) replaces exactly the masked positions of x: critic_input = where(mask, sampled, x) (:718)
        launch_maskgit_pick(w.loss_x, w.logits, V, lp.gumbel_u, (int)rows, V, V, lp.temperature, mask_id, s, lp.noise_seed, 0u, nullptr, 0);
        if (lp.critic_input_out) HIP_CHECK(hipMemcpyAsync(lp.critic_input_out, w.loss_x, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        muse_blocks(c, w, w.loss_x, s);
        launch_critic_bce_rows(w.xn, D, w.critic_w, w.critic_b, ids, w.loss_x, w.loss_rows, rows, D, s);
        launch_mean_fixed_order(w.loss_rows, rows, lp.out + 2, s);
    }
    launch_maskgit_loss_combine(lp.out, lp.critic_loss_weight, lp.with_critic, s);
}

}  // namespace bevgen
