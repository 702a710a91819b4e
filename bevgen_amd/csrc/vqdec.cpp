// Stage-1 VQGAN decode:  ids -> codebook rows -> post_quant_conv -> Decoder -> (denormalise)
//   VectorQuantizer2.get_codebook_entry   stage1/quantize.py:314-329
//   VQModel.decode                        stage1/vqgan.py:118-121
//   Decoder.forward                       stage1/model.py:506-537   ResnetBlock :117-137, AttnBlock :168-192, Upsample :49-53
//   util.denormalize_tensor               bev_utils/util.py:97-118
//
// Activations are NHWC so that every convolution is an implicit GEMM with K = (tap, channel) contiguous:
//   3x3 conv  -> gemm.hip MODE_CONV3 (im2col gather in the A-tile loader, nearest-2x upsample fused into the gather)
//   1x1 conv  -> plain GEMM over pixels
//   AttnBlock -> four 1x1 GEMMs + batched Q K^T / softmax / P V GEMMs (single head of width C, 256 tokens)
// GroupNorm(32)+swish is a stats pass + an elementwise pass; residual adds ride in the GEMM epilogues.
#include "model.h"

namespace bevgen {

namespace {

const std::string kPrefix = "first_stage_model.";

ConvW load_conv(Ctx& c, const std::string& name, int k) {
    const DevTensor& w = c.need(kPrefix + name + ".weight");
    BG_REQUIRE(w.shape.size() == 4 && w.shape[2] == k && w.shape[3] == k, "conv '%s' is not a %dx%d kernel", name.c_str(), k, k);
    ConvW cw;
    cw.cout = (int)w.shape[0];
    cw.cin = (int)w.shape[1];
    cw.k = k;
    cw.b = c.pf(kPrefix + name + ".bias");
    cw.w = reinterpret_cast<float*>(c.own(w.bytes));
    launch_relayout_conv_weight(w.f(), cw.w, cw.cout, cw.cin, k, k, 0);
    c.split_weight(cw.w, (long)cw.cout * cw.cin * k * k);
    return cw;
}

ResBlockW load_res(Ctx& c, const std::string& p) {
    ResBlockW r;
    r.n1w = c.pf(kPrefix + p + "norm1.weight"); r.n1b = c.pf(kPrefix + p + "norm1.bias");
    r.n2w = c.pf(kPrefix + p + "norm2.weight"); r.n2b = c.pf(kPrefix + p + "norm2.bias");
    r.c1 = load_conv(c, p + "conv1", 3);
    r.c2 = load_conv(c, p + "conv2", 3);
    r.cin = r.c1.cin; r.cout = r.c1.cout;
    r.has_nin = c.find(kPrefix + p + "nin_shortcut.weight") != nullptr;
    if (r.has_nin) r.nin = load_conv(c, p + "nin_shortcut", 1);
    BG_REQUIRE(r.has_nin == (r.cin != r.cout), "resnet block '%s': shortcut/channels mismatch", p.c_str());
    return r;
}

AttnBlockW load_attn(Ctx& c, const std::string& p) {
    AttnBlockW a;
    a.nw = c.pf(kPrefix + p + "norm.weight"); a.nb = c.pf(kPrefix + p + "norm.bias");
    a.q = load_conv(c, p + "q", 1); a.k = load_conv(c, p + "k", 1); a.v = load_conv(c, p + "v", 1); a.proj = load_conv(c, p + "proj_out", 1);
    a.c = a.q.cin;
    return a;
}

struct Act { float* p; int n, h, w, c; long elems() const { return (long)n * h * w * c; } };

// GroupNorm statistics of a tensor as partial sums out of the epilogue of the convolution that produced it (GemmArgs::gn_part): `of` names the tensor they describe.
// Every writer of an activation buffer goes through note_write() so that a stale association can never be used.
struct GnPart { float* buf = nullptr; const float* of = nullptr; };
static void note_write(GnPart* gp, const float* y) { if (gp && gp->of == y) gp->of = nullptr; }

static bool gn_epilogue() {
    static const int gn_epi = getenv("BEVGEN_GN_EPILOGUE") ? atoi(getenv("BEVGEN_GN_EPILOGUE")) : 1;   // (0: always the statistics pass, for A/B runs)
    return gn_epi != 0;
}

// planes: x.p holds the interleaved (hi, lo) f16 plane image of the activation (written by gn(..., planes = true)) instead of fp32
void conv3(const Act& x, const ConvW& w, float* y, const float* residual, int up, hipStream_t s, bool planes = false, GnPart* gp = nullptr) {
    GemmArgs g;
    note_write(gp, y);
    const int oh = up ? x.h * 2 : x.h, ow = up ? x.w * 2 : x.w;
    g.mode = MODE_CONV3;
    if (planes) { g.A_hi = reinterpret_cast<const uint16_t*>(x.p); g.A_lo = g.A_hi + 32; }
    else g.A = x.p;
    g.B = w.w; g.C = y; g.R = residual; g.bias_n = w.b;
    g.M = x.n * oh * ow; g.N = w.cout; g.K = 9 * w.cin;
    g.lda = w.cin; g.ldb = 9 * w.cin; g.ldc = w.cout; g.ldr = w.cout;
    g.conv_h = oh; g.conv_w = ow; g.conv_cin = w.cin; g.conv_up = up;
    // the LDS-DMA kernel (plane input) also leaves the GroupNorm partial sums of its output where the shape allows: the consumer's statistics pass disappears
    if (gn_epilogue() && gp && gp->buf && planes && groupnorm_partials_supported(oh * ow, w.cout)) { g.gn_part = gp->buf; gp->of = y; }
    launch_gemm(g, s);
}

void conv1(const float* x, long rows, const ConvW& w, float* y, const float* residual, hipStream_t s, GnPart* gp = nullptr) {
    note_write(gp, y);
    GemmArgs g;
    g.A = x; g.B = w.w; g.C = y; g.R = residual; g.bias_n = w.b;
    g.M = (int)rows; g.N = w.cout; g.K = w.cin;
    g.lda = w.cin; g.ldb = w.cin; g.ldc = w.cout; g.ldr = w.cout;
    launch_gemm(g, s);
}

// Range-safe mode (cfg.vq_range, split precision): the sites where an UN-normalised activation becomes an f16 operand take a per-tensor exponent from the next slot
// (kernels.h launch_range_*).  Decoder: conv_in (reads post_quant_conv's output), every nin_shortcut and every upsample convolution (both read the residual stream).
// Encoder: conv_in (reads the caller's image), every nin_shortcut and every downsample convolution (residual stream), quant_conv (reads conv_out's output).
// Everything else on the path reads a GroupNorm output or softmax-weighted values of one, or runs on the exact-fp32 kernel (the batched attention products, the
// quantizer's codebook products); the codebook and the weights are parameters, refused as before.
// pre_of: the tensor whose exponent a fused pass has already left in the next slot (range_next_slot): the site that reads it takes the slot without a pass of its own.
struct RangeSites { int* exps = nullptr; unsigned* amax = nullptr; int used = 0, cap = 0; const float* pre_of = nullptr; };

struct DecWs {
    float *a, *b, *t;   // ping-pong activations + temp (each max_act floats)
    float* stats;       // [n*32*2]
    void* gn_ws;
    float *q, *k, *vT, *S;
    float *o, *zq, *img, *dots, *zz;   // third rotating activation buffer; latents; decode: pixel staging / encode: codebook products and row norms
    GnPart part;        // epilogue partials of the most recent convolution output (buf: groupnorm_part_floats of the widest level, or null)
    RangeSites* range = nullptr;   // non-null: range-safe mode
};

const int* range_exponent(DecWs& ws, const Act& x, hipStream_t s) {
    RangeSites& r = *ws.range;
    BG_REQUIRE(r.used < r.cap, "vq: more range-safe sites than counted (%d)", r.cap);
    BG_REQUIRE(!r.pre_of || r.pre_of == x.p, "vq: the next range-safe slot was prepared for another tensor");
    if (r.pre_of) r.pre_of = nullptr;
    else launch_range_exponent(x.p, x.elems(), r.amax + r.used, r.exps + r.used, s);
    return r.exps + r.used++;
}

// the slot the NEXT site takes, for a pass that writes that site's operand `of` and leaves its exponent on the way (launch_*_amax)
struct NextSlot { unsigned* amax; int* e; };
NextSlot range_next_slot(DecWs& ws, const float* of) {
    RangeSites& r = *ws.range;
    BG_REQUIRE(r.used < r.cap && !r.pre_of, "vq: more range-safe sites than counted (%d)", r.cap);
    r.pre_of = of;
    return NextSlot{r.amax + r.used, r.exps + r.used};
}

// the encoder's two fused passes (0: their unfused pairs, for A/B runs)
static bool enc_fuse() {
    static const int fuse = getenv("BEVGEN_VQ_ENC_FUSE") ? atoi(getenv("BEVGEN_VQ_ENC_FUSE")) : 1;
    return fuse != 0;
}

// range-safe form of a convolution that reads the un-normalised fp32 tensor x itself: x 2^-e into `tmp` (x's size), W x' without the bias, then y = 2^e y + b.
// k = 1: 1x1, k = 3: 3x3 (up: fused nearest-2x upsample; down: the encoder's Downsample, conv3_down).  y_feeds_site: y is the next site's operand - the last pass also
// leaves that site's exponent (range_next_slot)
void conv3_down(const Act& x, const ConvW& w, float* y, hipStream_t s);
void conv_ranged(const Act& x, const ConvW& w, int k, int up, float* tmp, float* y, DecWs& ws, hipStream_t s, int down = 0, bool y_feeds_site = false) {
    const int* e = range_exponent(ws, x, s);
    note_write(&ws.part, tmp);
    launch_range_scale(x.p, tmp, x.elems(), e, s);
    ConvW wb = w;
    wb.b = nullptr;
    const long rows = down ? (long)x.n * (x.h / 2) * (x.w / 2) : (long)x.n * x.h * x.w * (up ? 4 : 1);
    if (k == 1) conv1(tmp, rows, wb, y, nullptr, s, &ws.part);
    else if (down) { note_write(&ws.part, y); conv3_down(Act{tmp, x.n, x.h, x.w, x.c}, wb, y, s); }
    else conv3(Act{tmp, x.n, x.h, x.w, x.c}, wb, y, nullptr, up, s, false, &ws.part);
    if (y_feeds_site && enc_fuse()) {
        const NextSlot nx = range_next_slot(ws, y);
        launch_range_unscale_amax(y, w.b, rows, w.cout, e, nx.amax, nx.e, s);
    } else {
        launch_range_unscale(y, w.b, nullptr, rows, w.cout, e, nullptr, s);
    }
}

// statistics of x: from the producing convolution's epilogue partials when they describe exactly this tensor, else the pass over the tensor
void gn_stats(const Act& x, DecWs& ws, hipStream_t s) {
    if (ws.part.of == x.p && ws.part.buf) launch_groupnorm_stats_from_partials(ws.part.buf, ws.stats, x.n, x.h * x.w, x.c, 1e-6f, s);
    else launch_groupnorm_stats(x.p, ws.stats, ws.gn_ws, x.n, x.h * x.w, x.c, 1e-6f, s);
}

void gn(const Act& x, const float* w, const float* b, float* y, int swish, DecWs& ws, hipStream_t s, bool planes = false) {
    gn_stats(x, ws, s);
    note_write(&ws.part, y);
    if (planes) launch_groupnorm_apply_planes(x.p, ws.stats, w, b, y, x.n, x.h * x.w, x.c, swish, s);
    else launch_groupnorm_apply(x.p, ws.stats, w, b, y, x.n, x.h * x.w, x.c, swish, s);
}

// x (in ws.a-or-b) -> out buffer `y`; uses ws.t and the other ping-pong buffer as scratch
void resblock(const ResBlockW& r, Act& x, float* y, float* scratch, DecWs& ws, hipStream_t s, bool planes) {
    // h = conv1(swish(norm1(x)));  split-precision mode: the normalised activation is written directly as the (hi, lo) planes the convolution reads
    gn(x, r.n1w, r.n1b, ws.t, 1, ws, s, planes);
    Act t{ws.t, x.n, x.h, x.w, r.cin};
    conv3(t, r.c1, scratch, nullptr, 0, s, planes, &ws.part);
    Act h1{scratch, x.n, x.h, x.w, r.cout};
    gn(h1, r.n2w, r.n2b, ws.t, 1, ws, s, planes);
    Act t2{ws.t, x.n, x.h, x.w, r.cout};
    const float* shortcut = x.p;
    if (r.has_nin) {  // x = nin_shortcut(x)  (1x1), written over h1 (no longer needed after norm2)
        if (ws.range) conv_ranged(x, r.nin, 1, 0, y, scratch, ws, s);   // (y is free until conv2 writes it)
        else conv1(x.p, (long)x.n * x.h * x.w, r.nin, scratch, nullptr, s, &ws.part);
        shortcut = scratch;
    }
    conv3(t2, r.c2, y, shortcut, 0, s, planes, &ws.part);  // y = x + conv2(...); its epilogue also leaves the statistics the next block's norm1 needs
    x = Act{y, x.n, x.h, x.w, r.cout};
}

void attnblock(const AttnBlockW& a, Act& x, float* y, DecWs& ws, hipStream_t s) {
    const int hw = x.h * x.w, C = a.c, n = x.n;
    const int hwp = (int)round_up(hw, 32);   // key dimension padded to the GEMM's k granularity (non-square latents: 14 x 25 = 350 -> 352); pad keys carry P = 0, v = 0
    const long rows = (long)n * hw;
    gn(x, a.nw, a.nb, ws.t, 0, ws, s);
    conv1(ws.t, rows, a.q, ws.q, nullptr, s);
    conv1(ws.t, rows, a.k, ws.k, nullptr, s);
    if (hwp != hw) HIP_CHECK(hipMemsetAsync(ws.vT, 0, (size_t)n * C * hwp * sizeof(float), s));
    {   // vT[img] [C, hw] = Wv [C,C] * h_img^T + bias (per row)
        GemmArgs g;
        g.A = a.v.w; g.B = ws.t; g.C = ws.vT; g.bias_m = a.v.b;
        g.M = C; g.N = hw; g.K = C; g.lda = C; g.ldb = C; g.ldc = hwp;
        g.batch = n; g.strideA = 0; g.strideB = (long)hw * C; g.strideC = (long)C * hwp;
        launch_gemm(g, s);
    }
    {   // S[img] [hw, hw] = q k^T
        GemmArgs g;
        g.A = ws.q; g.B = ws.k; g.C = ws.S;
        g.M = hw; g.N = hw; g.K = C; g.lda = C; g.ldb = C; g.ldc = hwp;
        g.batch = n; g.strideA = (long)hw * C; g.strideB = (long)hw * C; g.strideC = (long)hw * hwp;
        launch_gemm(g, s);
    }
    launch_row_softmax(ws.S, (int)rows, hw, 1.0f / sqrtf((float)C), s, hwp);  // w_ * int(c)**-0.5, softmax over keys
    {   // O[img] [hw, C] = P [hw,hw] * v [hw, C]  (B operand = vT [C, hw])
        GemmArgs g;
        g.A = ws.S; g.B = ws.vT; g.C = ws.q;  // reuse q as the output buffer
        g.M = hw; g.N = C; g.K = hwp; g.lda = hwp; g.ldb = hwp; g.ldc = C;
        g.batch = n; g.strideA = (long)hw * hwp; g.strideB = (long)C * hwp; g.strideC = (long)hw * C;
        launch_gemm(g, s);
    }
    conv1(ws.q, rows, a.proj, y, x.p, s, &ws.part);  // x + proj_out(h)
    x = Act{y, n, x.h, x.w, C};
}

// Downsample (stage1/model.py:56-75): F.pad(x, (0,1,0,1)) + 3x3 convolution, stride 2, padding 0; x.h and x.w even.  The bottom / right zero padding is the gather's bounds test.
void conv3_down(const Act& x, const ConvW& w, float* y, hipStream_t s) {
    GemmArgs ga;
    ga.mode = MODE_CONV3;
    ga.A = x.p; ga.B = w.w; ga.C = y; ga.bias_n = w.b;
    ga.M = x.n * (x.h / 2) * (x.w / 2); ga.N = w.cout; ga.K = 9 * w.cin;
    ga.lda = w.cin; ga.ldb = 9 * w.cin; ga.ldc = w.cout;
    ga.conv_h = x.h / 2; ga.conv_w = x.w / 2; ga.conv_cin = w.cin; ga.conv_up = 0;
    ga.conv_hin = x.h; ga.conv_win = x.w; ga.conv_stride = 2; ga.conv_pad = 0;
    launch_gemm(ga, s);
}

// VectorQuantizer2.forward (stage1/quantize.py:271-312): ids = argmin_j (|z|^2 + |e_j|^2) - 2 z.e_j, exact fp32 products (the codebook is never split); ee = |e_j|^2
void quantize(const float* z, const float* codebook, const float* ee, float* zz, float* dots, int64_t* ids, long rows, int n_e, int D, hipStream_t s) {
    launch_row_sqnorm(z, zz, rows, D, s);
    GemmArgs gd;
    gd.A = z; gd.B = codebook; gd.C = dots;
    gd.M = (int)rows; gd.N = n_e; gd.K = D; gd.lda = D; gd.ldb = D; gd.ldc = n_e;
    launch_gemm(gd, s);
    launch_vq_argmin(dots, zz, ee, ids, rows, n_e, s);
}

// Decoder.forward's last operators (norm_out, swish, conv_out) + denormalise + NCHW / uint8 store: one kernel, or (fused = false, or a shape it does not take) three.
// out_mode as in vq_decode; mean / stdv are read for out_mode != 0 only; img: [n, h w, cout] scratch of the three-kernel form
void out_tail(const Act& x, const float* nw, const float* nb, const ConvW& co, const float* mean, const float* stdv, int out_mode, bool fused, void* out, float* img, DecWs& ws,
              bool planes, hipStream_t s) {
    const int denorm = out_mode != 0;
    float* of = out_mode == 2 ? nullptr : reinterpret_cast<float*>(out);
    uint8_t* o8 = out_mode == 2 ? reinterpret_cast<uint8_t*>(out) : nullptr;
    if (fused && vq_out_conv_supported(x.c, co.cout)) {   // norm_out + swish + conv_out + denormalise + layout in one kernel
        gn_stats(x, ws, s);
        launch_vq_out_conv(x.p, ws.stats, nw, nb, co.w, co.b, denorm ? mean : nullptr, denorm ? stdv : nullptr, denorm ? 1 : 0, of, o8, x.n, x.h, x.w, x.c, co.cout, s);
        return;
    }
    gn(x, nw, nb, ws.t, 1, ws, s, planes);
    Act t{ws.t, x.n, x.h, x.w, x.c};
    conv3(t, co, img, nullptr, 0, s, planes);  // [n, h w, cout]
    launch_nhwc_to_nchw(img, of, x.n, x.h * x.w, co.cout, co.cout, denorm ? mean : nullptr, denorm ? stdv : nullptr, denorm ? 1 : 0, s, o8);
}

}  // namespace

static void vq_enc_finalize(Ctx& c);

void vq_finalize(Ctx& c) {
    const auto& g = c.cfg;
    BG_REQUIRE(g.vq_num_levels >= 1 && g.vq_num_levels <= 8, "vq_num_levels out of range");
    const DevTensor& cb = c.need(kPrefix + "quantize.embedding.weight");
    BG_REQUIRE(cb.shape.size() == 2 && cb.shape[0] == g.vq_n_embed && cb.shape[1] == g.vq_embed_dim, "codebook must be [n_embed, embed_dim]");
    c.codebook = cb.f();
    c.has_vq = c.find(kPrefix + "decoder.conv_in.weight") != nullptr;
    c.has_vq_enc = c.find(kPrefix + "encoder.conv_in.weight") != nullptr;
    BG_REQUIRE(c.has_vq || c.has_vq_enc, "VQGAN context: neither decoder.* nor encoder.* tensors were loaded");
    if (c.has_vq_enc) vq_enc_finalize(c);
    if (!c.has_vq) return;
    c.post_quant = load_conv(c, "post_quant_conv", 1);
    c.conv_in = load_conv(c, "decoder.conv_in", 3);
    c.mid1 = load_res(c, "decoder.mid.block_1.");
    c.mid_attn = load_attn(c, "decoder.mid.attn_1.");
    c.mid2 = load_res(c, "decoder.mid.block_2.");
    c.up.clear();
    c.up.resize(g.vq_num_levels);
    int res = g.vq_resolution >> (g.vq_num_levels - 1);
    for (int lvl = g.vq_num_levels - 1; lvl >= 0; --lvl) {
        UpLevelW& u = c.up[lvl];
        for (int b = 0; b < g.vq_num_res_blocks + 1; ++b) {
            const std::string p = "decoder.up." + std::to_string(lvl) + ".";
            u.blocks.push_back(load_res(c, p + "block." + std::to_string(b) + "."));
            if (res == g.vq_attn_resolution) u.attns.push_back(load_attn(c, p + "attn." + std::to_string(b) + "."));
        }
        u.has_up = lvl != 0;
        if (u.has_up) {
            u.up = load_conv(c, "decoder.up." + std::to_string(lvl) + ".upsample.conv", 3);
            res *= 2;
        }
    }
    c.norm_out_w = c.pf(kPrefix + "decoder.norm_out.weight");
    c.norm_out_b = c.pf(kPrefix + "decoder.norm_out.bias");
    c.conv_out = load_conv(c, "decoder.conv_out", 3);
    const float mean[3] = {0.4265f, 0.4489f, 0.4769f}, stdv[3] = {0.2053f, 0.2206f, 0.2578f};
    c.denorm_mean = reinterpret_cast<float*>(c.own(sizeof mean));
    c.denorm_std = reinterpret_cast<float*>(c.own(sizeof stdv));
    HIP_CHECK(hipMemcpy(c.denorm_mean, mean, sizeof mean, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(c.denorm_std, stdv, sizeof stdv, hipMemcpyHostToDevice));
}

// The decoder is fully convolutional (stage1/model.py:506-537): the latent grid is lat_h x lat_w (cam_latent_res, e.g. 16 x 16 or nuScenes' 14 x 25), the output
// (lat_h << (levels-1)) x (lat_w << (levels-1)); which levels carry AttnBlocks is decided by ddconfig.resolution alone (curr_res == attn_resolutions, :466-480).
// out_mode: 0 = raw fp32, 1 = denormalised fp32 in [0,1], 2 = denormalised uint8 round(x*255) (`out` then points to uint8).
void vq_decode(Ctx& c, const int64_t* ids, const float* latents_nchw, int n_total, int lat_h, int lat_w, int out_mode, void* out, hipStream_t s) {
    BG_REQUIRE(c.has_vq, "this context holds no VQGAN decoder weights (decoder.* tensors were not loaded)");
    const auto& g = c.cfg;
    const bool planes = g.precision == BEVGEN_PRECISION_F16X3;   // split-precision mode: GroupNorm writes (hi, lo) planes, convolutions read them by LDS-DMA
    BG_REQUIRE(lat_h >= 1 && lat_w >= 1, "vq_decode: latent grid %d x %d", lat_h, lat_w);
    const int denorm = out_mode != 0;
    const long lat_hw = (long)lat_h * lat_w;
    const int RH = lat_h << (g.vq_num_levels - 1), RW = lat_w << (g.vq_num_levels - 1);
    BG_REQUIRE(!denorm || g.vq_out_ch == 3, "denormalize needs 3 output channels");
    // widest activation per image: max over levels of h*w * channels; most attention tokens over the levels that carry AttnBlocks
    long per_img = 0, attn_hw = lat_hw;
    int max_c = 0;
    {
        long hw = lat_hw;
        for (int lvl = g.vq_num_levels - 1; lvl >= 0; --lvl) {
            const int ch = g.vq_ch * g.vq_ch_mult[lvl];
            const int ch_in = lvl == g.vq_num_levels - 1 ? ch : g.vq_ch * g.vq_ch_mult[lvl + 1];
            per_img = std::max<long>(per_img, hw * std::max(ch, ch_in));
            max_c = std::max(max_c, std::max(ch, ch_in));
            if (!c.up[lvl].attns.empty()) attn_hw = std::max(attn_hw, hw);
            if (lvl != 0) hw *= 4;
        }
    }
    const long attn_hwp = round_up(attn_hw, 32);
    // images per pass: the 16 x 16 stages only fill the chip (256 x 128 tiles on 256 CUs) from ~48 images; 148 -> 128 ms per 96 images vs 16, arena ~10 GB.  (Round 5: smaller
    // passes whose full-resolution tensors would fit the 256 MB memory-side cache between conv -> statistics -> apply -> conv are slower throughout: 6 / 12 / 24 images per
    // pass 11.96 / 9.14 / 7.96 ms per scene against 7.47, profiles/r05_ab_vq.txt)
    const int chunk_max = 48;
    const int attn_c = max_c;
    const int chunk = std::min(n_total, chunk_max);
    // the workspace of a pass over n images (a layout function, arena.h): metered for the largest pass, carved per pass
    auto layout = [&](Arena& a, DecWs& ws, int n) {
        if (planes) ws.part.buf = a.get<float>((size_t)per_img * n / 64 + 64);   // GroupNorm partials of one tensor: (pixels / 32) x (channels / 4) x 2
        ws.a = a.get<float>((size_t)per_img * n);
        ws.b = a.get<float>((size_t)per_img * n);
        ws.t = a.get<float>((size_t)per_img * n);
        ws.stats = a.get<float>((size_t)n * 64);
        ws.gn_ws = a.alloc(groupnorm_ws_bytes(n, RH * RW));
        ws.q = a.get<float>((size_t)n * attn_hwp * attn_c);
        ws.k = a.get<float>((size_t)n * attn_hwp * attn_c);
        ws.vT = a.get<float>((size_t)n * attn_hwp * attn_c);
        ws.S = a.get<float>((size_t)n * attn_hwp * attn_hwp);
        ws.zq = a.get<float>((size_t)n * lat_hw * g.vq_embed_dim);
        ws.img = a.get<float>((size_t)n * RH * RW * 4);
        ws.o = a.get<float>((size_t)per_img * n);
    };
    c.arena.reserve(Arena::measure([&](Arena& a) { DecWs ws; layout(a, ws, chunk); }));
    RangeSites sites;
    c.vq_range_used = 0;
    if (planes && g.vq_range) {
        int per_pass = 1;   // conv_in
        auto count = [&](const ResBlockW& r) { per_pass += r.has_nin ? 1 : 0; };
        count(c.mid1); count(c.mid2);
        for (const UpLevelW& u : c.up) {
            for (const ResBlockW& r : u.blocks) count(r);
            per_pass += u.has_up ? 1 : 0;
        }
        sites.cap = per_pass * cdiv(n_total, chunk);
        c.vq_range_slots.reserve((size_t)sites.cap * 8);
        sites.exps = reinterpret_cast<int*>(c.vq_range_slots.base);
        sites.amax = reinterpret_cast<unsigned*>(sites.exps + sites.cap);
        HIP_CHECK(hipMemsetAsync(sites.exps, 0, (size_t)sites.cap * 8, s));
    }
    for (int i0 = 0; i0 < n_total; i0 += chunk) {
        const int n = std::min(chunk, n_total - i0);
        c.arena.reset();
        DecWs ws;
        if (sites.cap) ws.range = &sites;
        layout(c.arena, ws, n);
        float *zq = ws.zq, *img = ws.img;

        const long lrows = (long)n * lat_hw;
        if (ids) launch_codebook_gather(ids + (long)i0 * lat_hw, c.codebook, zq, (int)lrows, g.vq_embed_dim, g.vq_n_embed, s);
        else launch_nchw_to_nhwc(latents_nchw + (long)i0 * g.vq_embed_dim * lat_hw, zq, n, (int)lat_hw, g.vq_embed_dim, s);
        conv1(zq, lrows, c.post_quant, ws.t, nullptr, s);                       // post_quant_conv
        Act x{ws.t, n, lat_h, lat_w, g.vq_z_channels};
        if (ws.range) conv_ranged(x, c.conv_in, 3, 0, ws.b, ws.a, ws, s);
        else conv3(x, c.conv_in, ws.a, nullptr, 0, s, false, &ws.part);          // conv_in
        x = Act{ws.a, n, lat_h, lat_w, c.conv_in.cout};
        // three rotating activation buffers (input / scratch / output of a block) + ws.t for the normalised tensor
        float* o = ws.o;
        auto res_step = [&](const ResBlockW& r) {
            // buffers: x.p in {a,b,o}; pick scratch and y as the two others
            float* bufs[3] = {ws.a, ws.b, o};
            float* scratch = nullptr; float* y = nullptr;
            for (float* b : bufs) { if (b != x.p) { if (!scratch) scratch = b; else y = b; } }
            resblock(r, x, y, scratch, ws, s, planes);
        };
        auto attn_step = [&](const AttnBlockW& ab) {
            float* bufs[3] = {ws.a, ws.b, o};
            float* y = nullptr;
            for (float* b : bufs) if (b != x.p) { y = b; break; }
            attnblock(ab, x, y, ws, s);
        };
        res_step(c.mid1);
        attn_step(c.mid_attn);
        res_step(c.mid2);
        for (int lvl = g.vq_num_levels - 1; lvl >= 0; --lvl) {
            const UpLevelW& u = c.up[lvl];
            for (size_t b = 0; b < u.blocks.size(); ++b) {
                res_step(u.blocks[b]);
                if (!u.attns.empty()) attn_step(u.attns[b]);
            }
            if (u.has_up) {  // nearest 2x + 3x3 conv, fused
                float* bufs[3] = {ws.a, ws.b, o};
                float* y = nullptr;
                for (float* b : bufs) if (b != x.p) { y = b; break; }
                // The upsample convolution reads the block output directly (no GroupNorm in front of it, s1model:49-53): in split-precision mode the tensor is first
                // re-laid out as (hi, lo) planes (one elementwise pass over the SMALL pre-upsample tensor) so that the 4x larger convolution runs on the LDS-DMA kernel
                // instead of the register-staged one ($BEVGEN_VQ_UP_PLANES=0: as in rounds 2-4)
                static const int up_planes = getenv("BEVGEN_VQ_UP_PLANES") ? atoi(getenv("BEVGEN_VQ_UP_PLANES")) : 1;
                const int q4 = x.c >> 2;
                if (planes && up_planes && (q4 & (q4 - 1)) == 0 && x.c % 32 == 0) {
                    note_write(&ws.part, ws.t);
                    Act xp{ws.t, x.n, x.h, x.w, x.c};
                    if (ws.range) {
                        // x 2^-e as planes, the convolution without its bias and without the epilogue statistics (they would describe the unscaled sums), then
                        // y = 2^e y + b in one pass that also leaves those statistics where the epilogue would have
                        const int* e = range_exponent(ws, x, s);
                        launch_range_split(x.p, ws.t, (long)x.n * x.h * x.w, x.c, e, s);
                        ConvW wb = u.up;
                        wb.b = nullptr;
                        conv3(xp, wb, y, nullptr, 1, s, true, nullptr);
                        note_write(&ws.part, y);
                        const bool part = gn_epilogue() && ws.part.buf && groupnorm_partials_supported(4 * x.h * x.w, u.up.cout);
                        launch_range_unscale(y, u.up.b, nullptr, 4L * x.n * x.h * x.w, u.up.cout, e, part ? ws.part.buf : nullptr, s);
                        if (part) ws.part.of = y;
                    } else {
                        launch_to_planes(x.p, ws.t, x.n, x.h * x.w, x.c, s);
                        conv3(xp, u.up, y, nullptr, 1, s, true, &ws.part);
                    }
                } else if (ws.range) {
                    conv_ranged(x, u.up, 3, 1, ws.t, y, ws, s);
                } else {
                    conv3(x, u.up, y, nullptr, 1, s, false, &ws.part);
                }
                x = Act{y, x.n, x.h * 2, x.w * 2, u.up.cout};
            }
        }
        const long o_off = (long)i0 * g.vq_out_ch * RH * RW;
        static const bool tail_off = getenv("BEVGEN_VQ_TAIL") && atoi(getenv("BEVGEN_VQ_TAIL")) == 0;   // (A/B switch: 0 = the three-kernel tail)
        void* o_ptr = out_mode == 2 ? static_cast<void*>(reinterpret_cast<uint8_t*>(out) + o_off) : static_cast<void*>(reinterpret_cast<float*>(out) + o_off);
        out_tail(x, c.norm_out_w, c.norm_out_b, c.conv_out, c.denorm_mean, c.denorm_std, out_mode, !tail_off, o_ptr, img, ws, planes, s);
    }
    c.vq_range_used = sites.used;
}

// exponents of the most recent decode / encode call (host array); synchronises
int vq_range_exponents(Ctx& c, int32_t* out, int cap) {
    HIP_CHECK(hipDeviceSynchronize());
    const int n = std::min(c.vq_range_used, cap);
    if (n > 0) HIP_CHECK(hipMemcpy(out, c.vq_range_slots.base, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return c.vq_range_used;
}

// =====================================================================================================
// Encoder + quantizer: the step BEFORE the sampling path (encode_to_c / encode_to_z, muse_lm:142-155)
//   Encoder.forward        stage1/model.py:405-433   (Downsample :56-75: zero pad (0,1,0,1) then 3x3 stride-2 conv)
//   VQModel.encode         stage1/vqgan.py:84-116    (geometric_embedding=False in the released configs)
//   VectorQuantizer2.forward  stage1/quantize.py:271-312
// =====================================================================================================
static ConvW load_conv_in_padded(Ctx& c, const std::string& name, int cin_pad) {
    const DevTensor& w = c.need(kPrefix + name + ".weight");
    BG_REQUIRE(w.shape.size() == 4 && w.shape[2] == 3 && w.shape[3] == 3, "conv '%s' is not a 3x3 kernel", name.c_str());
    ConvW cw;
    cw.cout = (int)w.shape[0];
    cw.cin = cin_pad;
    cw.k = 3;
    cw.b = c.pf(kPrefix + name + ".bias");
    cw.w = reinterpret_cast<float*>(c.own((size_t)cw.cout * 9 * cin_pad * sizeof(float)));
    launch_relayout_conv_weight_pad(w.f(), cw.w, cw.cout, (int)w.shape[1], cin_pad, 3, 3, 0);
    c.split_weight(cw.w, (long)cw.cout * 9 * cin_pad);
    return cw;
}

static void vq_enc_finalize(Ctx& c) {
    const auto& g = c.cfg;
    BG_REQUIRE(g.vq_in_channels >= 1, "vq_in_channels must be set for the encoder");
    c.enc_cin_pad = (int)round_up(g.vq_in_channels, 32);
    c.enc_conv_in = load_conv_in_padded(c, "encoder.conv_in", c.enc_cin_pad);
    c.down.clear();
    c.down.resize(g.vq_num_levels);
    int res = g.vq_resolution;
    for (int lvl = 0; lvl < g.vq_num_levels; ++lvl) {
        DownLevelW& d = c.down[lvl];
        const std::string p = "encoder.down." + std::to_string(lvl) + ".";
        for (int b = 0; b < g.vq_num_res_blocks; ++b) {
            d.blocks.push_back(load_res(c, p + "block." + std::to_string(b) + "."));
            if (res == g.vq_attn_resolution) d.attns.push_back(load_attn(c, p + "attn." + std::to_string(b) + "."));
        }
        d.has_down = lvl != g.vq_num_levels - 1;
        if (d.has_down) {
            d.down = load_conv(c, p + "downsample.conv", 3);
            res /= 2;
        }
    }
    c.enc_mid1 = load_res(c, "encoder.mid.block_1.");
    c.enc_mid_attn = load_attn(c, "encoder.mid.attn_1.");
    c.enc_mid2 = load_res(c, "encoder.mid.block_2.");
    c.enc_norm_out_w = c.pf(kPrefix + "encoder.norm_out.weight");
    c.enc_norm_out_b = c.pf(kPrefix + "encoder.norm_out.bias");
    c.enc_conv_out = load_conv(c, "encoder.conv_out", 3);
    c.quant_conv = load_conv(c, "quant_conv", 1);
    BG_REQUIRE(c.enc_conv_out.cout == g.vq_z_channels && c.quant_conv.cout == g.vq_embed_dim, "encoder output channels do not match z_channels / embed_dim (double_z must be False)");
    c.codebook_sqnorm = reinterpret_cast<float*>(c.own((size_t)g.vq_n_embed * sizeof(float)));
    launch_row_sqnorm(c.codebook, c.codebook_sqnorm, g.vq_n_embed, g.vq_embed_dim, 0);
}

// x [n, in_channels, RH, RW] with RH, RW multiples of 2^(levels-1) (fully convolutional: 256 x 256 or nuScenes' 224 x 400) -> ids [n, (RH >> (levels-1)) * (RW >> (levels-1))]
void vq_encode(Ctx& c, const float* x_nchw, int n_total, int RH, int RW, int64_t* ids, hipStream_t s) {
    BG_REQUIRE(c.has_vq_enc, "this context holds no VQGAN encoder weights (encoder.* tensors were not loaded)");
    const auto& g = c.cfg;
    const bool planes = g.precision == BEVGEN_PRECISION_F16X3;   // split-precision mode: GroupNorm writes (hi, lo) planes, convolutions read them by LDS-DMA
    const int f = 1 << (g.vq_num_levels - 1);
    BG_REQUIRE(RH >= f && RW >= f && RH % f == 0 && RW % f == 0, "vq_encode: image %d x %d is not a multiple of the downsampling factor %d", RH, RW, f);
    const int lat_h = RH / f, lat_w = RW / f;
    const long lat_hw = (long)lat_h * lat_w;
    long per_img = (long)RH * RW * std::max(c.enc_cin_pad, g.vq_ch), attn_hw = lat_hw;
    int max_c = g.vq_ch;
    {
        long hw = (long)RH * RW;
        for (int lvl = 0; lvl < g.vq_num_levels; ++lvl) {
            const int ch = g.vq_ch * g.vq_ch_mult[lvl];
            per_img = std::max<long>(per_img, hw * ch);
            max_c = std::max(max_c, ch);
            if (!c.down[lvl].attns.empty()) attn_hw = std::max(attn_hw, hw);
            if (lvl != g.vq_num_levels - 1) hw /= 4;
        }
    }
    const int chunk = std::min(n_total, 48);
    const long attn_hwp = round_up(attn_hw, 32);
    // the workspace of a pass over n images (a layout function, arena.h): metered for the largest pass, carved per pass
    auto layout = [&](Arena& a, DecWs& ws, int n) {
        ws.a = a.get<float>((size_t)per_img * n);
        ws.b = a.get<float>((size_t)per_img * n);
        ws.t = a.get<float>((size_t)per_img * n);
        ws.o = a.get<float>((size_t)per_img * n);
        ws.stats = a.get<float>((size_t)n * 64);
        ws.gn_ws = a.alloc(groupnorm_ws_bytes(n, RH * RW));
        ws.q = a.get<float>((size_t)n * attn_hwp * max_c);
        ws.k = a.get<float>((size_t)n * attn_hwp * max_c);
        ws.vT = a.get<float>((size_t)n * attn_hwp * max_c);
        ws.S = a.get<float>((size_t)n * attn_hwp * attn_hwp);
        ws.dots = a.get<float>((size_t)n * lat_hw * g.vq_n_embed);
        ws.zq = a.get<float>((size_t)n * lat_hw * g.vq_embed_dim);
        ws.zz = a.get<float>((size_t)n * lat_hw);
    };
    c.arena.reserve(Arena::measure([&](Arena& a) { DecWs ws; layout(a, ws, chunk); }));
    RangeSites sites;
    c.vq_range_used = 0;
    if (planes && g.vq_range) {
        int per_pass = 2;   // conv_in, quant_conv
        auto count = [&](const ResBlockW& r) { per_pass += r.has_nin ? 1 : 0; };
        for (const DownLevelW& d : c.down) {
            for (const ResBlockW& r : d.blocks) count(r);
            per_pass += d.has_down ? 1 : 0;
        }
        count(c.enc_mid1); count(c.enc_mid2);
        sites.cap = per_pass * cdiv(n_total, chunk);
        c.vq_range_slots.reserve((size_t)sites.cap * 8);
        sites.exps = reinterpret_cast<int*>(c.vq_range_slots.base);
        sites.amax = reinterpret_cast<unsigned*>(sites.exps + sites.cap);
        HIP_CHECK(hipMemsetAsync(sites.exps, 0, (size_t)sites.cap * 8, s));
    }
    for (int i0 = 0; i0 < n_total; i0 += chunk) {
        const int n = std::min(chunk, n_total - i0);
        c.arena.reset();
        DecWs ws;
        if (sites.cap) ws.range = &sites;
        layout(c.arena, ws, n);
        const long lrows = (long)n * lat_hw;
        float *o = ws.o, *dots = ws.dots, *zq = ws.zq, *zz = ws.zz;

        const float* x_in = x_nchw + (long)i0 * g.vq_in_channels * RH * RW;
        Act x{ws.t, n, RH, RW, c.enc_cin_pad};
        if (ws.range) {   // the layout change also leaves the image's exponent: conv_in's site needs no pass of its own over the padded tensor
            if (enc_fuse()) {
                const NextSlot nx = range_next_slot(ws, ws.t);
                launch_nchw_to_nhwc_pad_amax(x_in, ws.t, n, RH * RW, g.vq_in_channels, c.enc_cin_pad, nx.amax, nx.e, s);
            } else {
                launch_nchw_to_nhwc_pad(x_in, ws.t, n, RH * RW, g.vq_in_channels, c.enc_cin_pad, s);
            }
            conv_ranged(x, c.enc_conv_in, 3, 0, ws.b, ws.a, ws, s);
        } else {
            launch_nchw_to_nhwc_pad(x_in, ws.t, n, RH * RW, g.vq_in_channels, c.enc_cin_pad, s);
            conv3(x, c.enc_conv_in, ws.a, nullptr, 0, s);
        }
        x = Act{ws.a, n, RH, RW, c.enc_conv_in.cout};
        auto pick2 = [&](float*& scratch, float*& y) {
            float* bufs[3] = {ws.a, ws.b, o};
            scratch = nullptr; y = nullptr;
            for (float* b : bufs) { if (b != x.p) { if (!scratch) scratch = b; else y = b; } }
        };
        auto res_step = [&](const ResBlockW& r) { float *sc, *y; pick2(sc, y); resblock(r, x, y, sc, ws, s, planes); };
        auto attn_step = [&](const AttnBlockW& ab) { float *sc, *y; pick2(sc, y); attnblock(ab, x, y, ws, s); };
        for (int lvl = 0; lvl < g.vq_num_levels; ++lvl) {
            const DownLevelW& d = c.down[lvl];
            for (size_t b = 0; b < d.blocks.size(); ++b) {
                res_step(d.blocks[b]);
                if (!d.attns.empty()) attn_step(d.attns[b]);
            }
            if (d.has_down) {  // F.pad(x, (0,1,0,1)) + conv 3x3 stride 2 padding 0
                float *sc, *y; pick2(sc, y);
                // (its output is the next level's residual stream: where that level opens with a nin_shortcut, that site's operand)
                const bool feeds_nin = !c.down[lvl + 1].blocks.empty() && c.down[lvl + 1].blocks[0].has_nin;
                if (ws.range) conv_ranged(x, d.down, 3, 0, sc, y, ws, s, 1, feeds_nin);
                else conv3_down(x, d.down, y, s);
                x = Act{y, x.n, x.h / 2, x.w / 2, d.down.cout};
            }
        }
        res_step(c.enc_mid1);
        attn_step(c.enc_mid_attn);
        res_step(c.enc_mid2);
        gn(x, c.enc_norm_out_w, c.enc_norm_out_b, ws.t, 1, ws, s, planes);
        Act t{ws.t, x.n, x.h, x.w, x.c};
        float *sc, *y; pick2(sc, y);
        conv3(t, c.enc_conv_out, y, nullptr, 0, s, planes);                     // [n, lat*lat, z_channels]
        if (ws.range) conv_ranged(Act{y, x.n, x.h, x.w, g.vq_z_channels}, c.quant_conv, 1, 0, sc, zq, ws, s);
        else conv1(y, lrows, c.quant_conv, zq, nullptr, s);             // quant_conv (1x1)
        quantize(zq, c.codebook, c.codebook_sqnorm, zz, dots, ids + (long)i0 * lat_hw, lrows, g.vq_n_embed, g.vq_embed_dim, s);
    }
    c.vq_range_used = sites.used;
}

// =====================================================================================================
// Operator entries (bevgen_op_* in api.cpp): the pieces above on caller-supplied device tensors, at shapes of their own.  They forward to the launchers / helpers the model
// path uses and add no arithmetic.  Weights arrive as the checkpoint stores them ([Cout][Cin][kh][kw]) and are prepared the way load_conv prepares them, into the arena.
// =====================================================================================================
namespace {

// The weights of one operator call: re-laid out into the arena and, in split-precision mode, registered as split weights FOR THE DURATION OF THE CALL (the registry is
// keyed by pointer and the arena hands the same addresses to the next call: a registration that outlived the call would serve stale planes).
struct OpWeights {
    Ctx& c;
    hipStream_t s;
    std::vector<const float*> keys;
    OpWeights(Ctx& c_, hipStream_t s_) : c(c_), s(s_) {}
    ~OpWeights() { for (const float* k : keys) c.split.erase(k); }
    struct Buf { float* w; void* planes; };
    // the layout half of conv(): the re-laid-out weight and, in split-precision mode, its planes
    static Buf take(const Ctx& c, Arena& a, int cout, int cin, int k) {
        const size_t n = (size_t)cout * cin * k * k;
        Buf b;
        b.w = a.get<float>(n);
        b.planes = c.cfg.precision == BEVGEN_PRECISION_F16X3 ? a.alloc(n * 4) : nullptr;
        return b;
    }
    ConvW conv(Buf buf, const float* w_oihw, const float* b, int cout, int cin, int k) {
        ConvW cw;
        cw.cout = cout; cw.cin = cin; cw.k = k; cw.b = b;
        const long n = (long)cout * cin * k * k;
        cw.w = buf.w;
        launch_relayout_conv_weight(w_oihw, cw.w, cout, cin, k, k, s);
        if (c.cfg.precision == BEVGEN_PRECISION_F16X3) {
            void* planes = buf.planes;
            const bool w16 = c.cfg.weight_dtype == BEVGEN_W_F16;
            if (w16) launch_round_to_f16(cw.w, nullptr, n, s);
            launch_split_weight(cw.w, planes, n, s);
            c.split[cw.w] = SplitPlanes{reinterpret_cast<const uint16_t*>(planes), reinterpret_cast<const uint16_t*>(planes) + 32, w16};
            keys.push_back(cw.w);
        }
        return cw;
    }
};

}  // namespace

void vq_op_conv3x3_down(Ctx& c, const float* x, const float* w, const float* bias, float* y, int n, int H, int W, int Cin, int Cout, hipStream_t s) {
    BG_REQUIRE(n >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && Cin >= 32 && Cin % 32 == 0 && Cout >= 1,
               "op_conv3x3_down: needs even H, W and Cin %% 32 == 0 (H=%d W=%d Cin=%d)", H, W, Cin);
    OpWeights::Buf wb;
    c.arena.carve([&](Arena& a) { wb = OpWeights::take(c, a, Cout, Cin, 3); });
    OpWeights ow(c, s);
    const ConvW cw = ow.conv(wb, w, bias, Cout, Cin, 3);
    conv3_down(Act{const_cast<float*>(x), n, H, W, Cin}, cw, y, s);
}

// one range-safe site as vq_decode / vq_encode run it (conv_ranged); kind 0: 1x1, 1: 3x3, 2: the Downsample.  kind 2 ends in the fused pass (y_feeds_site) as a
// downsample in front of a nin_shortcut does; the exponent that pass leaves for y stays in the arena.
void vq_op_conv_ranged(Ctx& c, const float* x, const float* w, const float* bias, int kind, float* y, int32_t* d_exp, int n, int H, int W, int Cin, int Cout, hipStream_t s) {
    BG_REQUIRE(c.cfg.precision == BEVGEN_PRECISION_F16X3, "op_conv_ranged: the range-safe sites belong to the split-precision mode (precision = f16x3)");
    BG_REQUIRE(kind >= 0 && kind <= 2, "op_conv_ranged: kind %d (0 = 1x1, 1 = 3x3, 2 = downsample)", kind);
    BG_REQUIRE(n >= 1 && H >= 1 && W >= 1 && Cin >= 32 && Cin % 32 == 0 && Cout >= 4 && Cout % 4 == 0, "op_conv_ranged: needs Cin %% 32 == 0 and Cout %% 4 == 0 (Cin=%d Cout=%d)", Cin, Cout);
    BG_REQUIRE(kind != 2 || (H % 2 == 0 && W % 2 == 0), "op_conv_ranged: the downsample needs even H, W (H=%d W=%d)", H, W);
    BG_REQUIRE(x != y, "op_conv_ranged: the output must not alias the input");
    const int k = kind == 0 ? 1 : 3;
    OpWeights::Buf wb;
    float* tmp;
    RangeSites sites;
    sites.cap = 2;
    c.arena.carve([&](Arena& a) {
        wb = OpWeights::take(c, a, Cout, Cin, k);
        tmp = a.get<float>((size_t)n * H * W * Cin);
        sites.exps = a.get<int>(2 * sites.cap);
    });
    sites.amax = reinterpret_cast<unsigned*>(sites.exps + sites.cap);
    HIP_CHECK(hipMemsetAsync(sites.exps, 0, (size_t)sites.cap * 8, s));
    OpWeights ow(c, s);
    const ConvW cw = ow.conv(wb, w, bias, Cout, Cin, k);
    DecWs ws{};
    ws.range = &sites;
    conv_ranged(Act{const_cast<float*>(x), n, H, W, Cin}, cw, k, 0, tmp, y, ws, s, kind == 2, kind == 2);
    HIP_CHECK(hipMemcpyAsync(d_exp, sites.exps, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
}

void vq_op_attn_block(Ctx& c, const float* x, const float* norm_w, const float* norm_b, const float* wq, const float* bq, const float* wk, const float* bk, const float* wv,
                      const float* bv, const float* wp, const float* bp, float* y, int n, int h, int w, int C, hipStream_t s) {
    BG_REQUIRE(n >= 1 && h >= 1 && w >= 1 && C >= 32 && C % 32 == 0 && C <= 1024, "op_vq_attn_block: C=%d must be a multiple of 32 (at most 1024)", C);
    BG_REQUIRE(x != y, "op_vq_attn_block: the output must not alias the input (the residual is read by the last GEMM)");
    const long hw = (long)h * w, hwp = round_up(hw, 32);
    const size_t f = sizeof(float);
    const size_t qb = (size_t)n * hwp * C * f, sb = (size_t)n * hwp * hwp * f;
    OpWeights::Buf wb[4];
    DecWs ws{};
    c.arena.carve([&](Arena& ar) {
        for (OpWeights::Buf& b : wb) b = OpWeights::take(c, ar, C, C, 1);
        ws.t = ar.get<float>((size_t)n * hw * C);
        ws.stats = ar.get<float>((size_t)n * 64);
        ws.gn_ws = ar.alloc(groupnorm_ws_bytes(n, (int)hw));
        ws.q = ar.get<float>(qb / f);
        ws.k = ar.get<float>(qb / f);
        ws.vT = ar.get<float>(qb / f);
        ws.S = ar.get<float>(sb / f);
    });
    OpWeights ow(c, s);
    AttnBlockW a;
    a.nw = norm_w; a.nb = norm_b; a.c = C;
    a.q = ow.conv(wb[0], wq, bq, C, C, 1); a.k = ow.conv(wb[1], wk, bk, C, C, 1); a.v = ow.conv(wb[2], wv, bv, C, C, 1); a.proj = ow.conv(wb[3], wp, bp, C, C, 1);
    // the model's workspace holds whatever the previous kernels left there: NaN bit patterns here, so that a pad column that is read without having been written shows
    HIP_CHECK(hipMemsetAsync(ws.q, 0xFF, qb, s));
    HIP_CHECK(hipMemsetAsync(ws.k, 0xFF, qb, s));
    HIP_CHECK(hipMemsetAsync(ws.vT, 0xFF, qb, s));
    HIP_CHECK(hipMemsetAsync(ws.S, 0xFF, sb, s));
    Act xa{const_cast<float*>(x), n, h, w, C};
    attnblock(a, xa, y, ws, s);
}

void vq_op_out_tail(Ctx& c, const float* x, const float* norm_w, const float* norm_b, const float* w, const float* bias, const float* mean, const float* stdv, int out_mode,
                    int three_kernels, void* out, int n, int H, int W, int C, hipStream_t s) {
    const int cout = 3;
    BG_REQUIRE(n >= 1 && H >= 1 && W >= 1 && C >= 32 && C % 32 == 0 && C <= 1024, "op_vq_out_tail: C=%d must be a multiple of 32 (at most 1024)", C);
    BG_REQUIRE(out_mode >= 0 && out_mode <= 2 && (out_mode == 0 || (mean && stdv)), "op_vq_out_tail: out_mode 0 / 1 / 2; 1 and 2 need mean and std");
    const bool planes = c.cfg.precision == BEVGEN_PRECISION_F16X3;
    const long hw = (long)H * W;
    OpWeights::Buf wb;
    DecWs ws{};
    c.arena.carve([&](Arena& a) {
        wb = OpWeights::take(c, a, cout, C, 3);
        ws.t = a.get<float>((size_t)n * hw * C);
        ws.stats = a.get<float>((size_t)n * 64);
        ws.gn_ws = a.alloc(groupnorm_ws_bytes(n, (int)hw));
        ws.img = a.get<float>((size_t)n * hw * 4);
    });
    OpWeights ow(c, s);
    const ConvW co = ow.conv(wb, w, bias, cout, C, 3);
    out_tail(Act{const_cast<float*>(x), n, H, W, C}, norm_w, norm_b, co, mean, stdv, out_mode, three_kernels == 0, out, ws.img, ws, planes, s);
}

void vq_op_quantize(Ctx& c, const float* z, const float* codebook, int64_t* ids, float* zz_out, float* ee_out, long rows, int n_e, int D, hipStream_t s) {
    BG_REQUIRE(rows >= 1 && rows <= 0x7FFFFFFFL && n_e >= 1 && D >= 32 && D % 32 == 0, "op_vq_quantize: needs D %% 32 == 0 (rows=%ld n_e=%d D=%d)", rows, n_e, D);
    float *dots, *zz, *ee;
    c.arena.carve([&](Arena& a) {
        dots = a.get<float>((size_t)rows * n_e);
        zz = a.get<float>((size_t)rows);
        ee = a.get<float>((size_t)n_e);
    });
    launch_row_sqnorm(codebook, ee, n_e, D, s);   // (the model: once, at finalize)
    quantize(z, codebook, ee, zz, dots, ids, rows, n_e, D, s);
    if (zz_out) HIP_CHECK(hipMemcpyAsync(zz_out, zz, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (ee_out) HIP_CHECK(hipMemcpyAsync(ee_out, ee, (size_t)n_e * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void vq_op_conv3x3_gn_stats(Ctx& c, const float* x, const float* w, const float* bias, int range_route, float* y, float* part, float* stats, int n, int H, int W, int Cin,
                            int Cout, hipStream_t s) {
    BG_REQUIRE(c.cfg.precision == BEVGEN_PRECISION_F16X3, "op_conv3x3_gn_stats: the convolution epilogue that leaves GroupNorm partials belongs to the split-precision mode (precision = f16x3)");
    BG_REQUIRE(gn_epilogue(), "op_conv3x3_gn_stats: the epilogue statistics are switched off (BEVGEN_GN_EPILOGUE=0)");
    const int hw = H * W, q4 = Cin >> 2;
    BG_REQUIRE(n >= 1 && H >= 1 && W >= 1 && Cin >= 32 && Cin % 32 == 0 && (q4 & (q4 - 1)) == 0 && bias, "op_conv3x3_gn_stats: needs a bias and Cin / 4 a power of two >= 8 (Cin=%d)", Cin);
    BG_REQUIRE(groupnorm_partials_supported(hw, Cout), "groupnorm from partials: unsupported shape hw=%d C=%d", hw, Cout);
    OpWeights::Buf wbuf;
    float* planes;
    int* e;
    c.arena.carve([&](Arena& a) {
        wbuf = OpWeights::take(c, a, Cout, Cin, 3);
        planes = a.get<float>((size_t)n * hw * Cin);
        e = range_route ? a.get<int>(1) : nullptr;
    });
    OpWeights ow(c, s);
    ConvW cw = ow.conv(wbuf, w, bias, Cout, Cin, 3);
    Act xp{planes, n, H, W, Cin};
    if (range_route) {   // the upsample site of the range-safe mode without the upsample, exponent 0: planes, the convolution without its bias, then bias + statistics in one pass
        HIP_CHECK(hipMemsetAsync(e, 0, sizeof(int), s));
        launch_range_split(x, planes, (long)n * hw, Cin, e, s);
        ConvW wb = cw;
        wb.b = nullptr;
        conv3(xp, wb, y, nullptr, 0, s, true, nullptr);
        launch_range_unscale(y, cw.b, nullptr, (long)n * hw, Cout, e, part, s);
    } else {
        launch_to_planes(x, planes, n, hw, Cin, s);
        GnPart gp;
        gp.buf = part;
        conv3(xp, cw, y, nullptr, 0, s, true, &gp);
        BG_REQUIRE(gp.of == y, "op_conv3x3_gn_stats: the convolution did not leave partials");
    }
    launch_groupnorm_stats_from_partials(part, stats, n, hw, Cout, 1e-6f, s);
}

}  // namespace bevgen
