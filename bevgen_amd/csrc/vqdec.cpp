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
//
// Structure: vq_plan.h holds what is pure (sizes, pass cut, site count, upsample form); `Pass` below holds one pass over up to 48 images - its buffers, the current
// activation and every launch that writes one; vq_decode / vq_encode are the list of steps.
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

// the plan's shape (vq_plan.h) of one direction, from the configuration and, level by level, from the loaded weights
VqShape shape_of(const bevgen_cfg& g, bool encoder, int cin_pad, const ResBlockW& mid1, const ResBlockW& mid2) {
    VqShape sh;
    sh.encoder = encoder;
    sh.levels = g.vq_num_levels; sh.ch = g.vq_ch; sh.cin_pad = cin_pad;
    for (int l = 0; l < sh.levels; ++l) sh.ch_mult[l] = g.vq_ch_mult[l];
    sh.mid_nin = (mid1.has_nin ? 1 : 0) + (mid2.has_nin ? 1 : 0);
    return sh;
}
void shape_level(VqShape& sh, int lvl, const std::vector<ResBlockW>& blocks, bool attn, bool resample) {
    for (const ResBlockW& r : blocks) sh.nin[lvl] += r.has_nin ? 1 : 0;
    sh.first_nin[lvl] = !blocks.empty() && blocks[0].has_nin;
    sh.attn[lvl] = attn;
    sh.resample[lvl] = resample;
}

// the four A/B switches of this file, read once per process
const VqSwitches& vq_switches() {
    static const VqSwitches sw = [] {
        const auto on = [](const char* name) { const char* v = getenv(name); return !v || atoi(v) != 0; };   // unset = on
        VqSwitches r;
        r.gn_epilogue = on("BEVGEN_GN_EPILOGUE");
        r.enc_fuse = on("BEVGEN_VQ_ENC_FUSE");
        r.up_planes = on("BEVGEN_VQ_UP_PLANES");
        r.tail = on("BEVGEN_VQ_TAIL");
        return r;
    }();
    return sw;
}

// planes: p holds the interleaved (hi, lo) f16 plane image of the activation (written by Pass::gn / Pass::to_planes) instead of fp32
struct Act { float* p; int n, h, w, c; bool planes = false; long elems() const { return (long)n * h * w * c; } };

// GroupNorm statistics of a tensor as partial sums out of the epilogue of the convolution that produced it (GemmArgs::gn_part): `of` names the tensor they describe.
// Every writer of an activation buffer is a method of Pass and goes through note_write() so that a stale association can never be used.
struct GnPart { float* buf = nullptr; const float* of = nullptr; };
void note_write(GnPart& gp, const float* y) { if (gp.of == y) gp.of = nullptr; }

// Range-safe mode (cfg.vq_range, split precision): the sites where an UN-normalised activation becomes an f16 operand take a per-tensor exponent from the next slot
// (kernels.h launch_range_*).  Decoder: conv_in (reads post_quant_conv's output), every nin_shortcut and every upsample convolution (both read the residual stream).
// Encoder: conv_in (reads the caller's image), every nin_shortcut and every downsample convolution (residual stream), quant_conv (reads conv_out's output).
// Everything else on the path reads a GroupNorm output or softmax-weighted values of one, or runs on the exact-fp32 kernel (the batched attention products, the
// quantizer's codebook products); the codebook and the weights are parameters, refused as before.
// cap is vq_sites_per_pass x passes (vq_plan.h) and a decode / encode call must use exactly that many (sites_done).
// pre_of: the tensor whose exponent a fused pass has already left in the next slot (next_slot): the site that reads it takes the slot without a pass of its own.
struct RangeSites { int* exps = nullptr; unsigned* amax = nullptr; int used = 0, cap = 0; const float* pre_of = nullptr; };

// the slots of a decode / encode call of `cap` sites (0: not the range-safe mode), zeroed
RangeSites sites_reserve(Ctx& c, int cap, hipStream_t s) {
    RangeSites r;
    c.vq_range_used = 0;
    if (cap == 0) return r;
    r.cap = cap;
    c.vq_range_slots.reserve((size_t)cap * 8);
    r.exps = reinterpret_cast<int*>(c.vq_range_slots.base);
    r.amax = reinterpret_cast<unsigned*>(r.exps + cap);
    HIP_CHECK(hipMemsetAsync(r.exps, 0, (size_t)cap * 8, s));
    return r;
}
void sites_done(Ctx& c, const RangeSites& r) {
    BG_REQUIRE(r.used == r.cap, "vq: the passes ran %d range-safe sites, the plan counted %d", r.used, r.cap);
    c.vq_range_used = r.used;
}

// a 3x3 convolution of x as an implicit GEMM: 'same' (stride 1, padding 1), behind a fused nearest-2x upsample, or the encoder's Downsample (stage1/model.py:56-75:
// F.pad(x, (0,1,0,1)) + stride 2, padding 0; x.h and x.w even; the bottom / right zero padding is the gather's bounds test).  The caller adds C and R.
enum ConvGeom { CONV_SAME, CONV_UP2, CONV_DOWN2 };
GemmArgs conv3_args(const Act& x, const ConvW& w, ConvGeom geom) {
    GemmArgs g;
    const int oh = geom == CONV_UP2 ? x.h * 2 : geom == CONV_DOWN2 ? x.h / 2 : x.h, ow = geom == CONV_UP2 ? x.w * 2 : geom == CONV_DOWN2 ? x.w / 2 : x.w;
    g.mode = MODE_CONV3;
    if (x.planes) { g.A_hi = reinterpret_cast<const uint16_t*>(x.p); g.A_lo = g.A_hi + 32; }
    else g.A = x.p;
    g.B = w.w; g.bias_n = w.b;
    g.M = x.n * oh * ow; g.N = w.cout; g.K = 9 * w.cin;
    g.lda = w.cin; g.ldb = 9 * w.cin; g.ldc = w.cout; g.ldr = w.cout;
    g.conv_h = oh; g.conv_w = ow; g.conv_cin = w.cin; g.conv_up = geom == CONV_UP2;
    if (geom == CONV_DOWN2) { g.conv_hin = x.h; g.conv_win = x.w; g.conv_stride = 2; g.conv_pad = 0; }
    return g;
}

// One range-safe site: x 2^-e into `tmp` (x's size), W x' without the bias, then y = 2^e y + b.
struct RangedOpts {
    int k = 3;                    // 1: a 1x1 convolution (geom unused)
    ConvGeom geom = CONV_SAME;
    bool plane_operand = false;   // x 2^-e is written as the (hi, lo) plane image and the convolution runs on the LDS-DMA kernel, instead of fp32
    bool leave_partials = false;  // the last pass also leaves the GroupNorm partials of y where the convolution's epilogue would have (it cannot: they would describe the unscaled sums)
    bool y_feeds_site = false;    // y is the next site's operand: the last pass also leaves that site's exponent (next_slot)
    const int* e = nullptr;       // the exponent, where the caller has one; null: the next slot (range_exponent)
};

// the decoder's last step: out_mode as in vq_decode; mean / stdv are read for out_mode != 0 only; img: [n, h w, max(4, cout)] scratch of the three-kernel form
struct TailOut { void* out; int out_mode; const float *mean, *stdv; float* img; bool fused; };

// the geometric embedding of a pass (launch_vq_geo_embed): the matrices of the pass's images, the latent plane and the two weights [z_channels, 4]
struct GeoEmbed { const float *I_inv, *E_inv, *plane, *wimg, *wcam; };

// One pass over n images: the carved buffers, the current activation and every launch that writes an activation buffer.
struct Pass {
    hipStream_t s = nullptr;
    // three rotating activation buffers (input / scratch / output of a block) + t for the normalised tensor (each per_img x n floats)
    float *a = nullptr, *b = nullptr, *o = nullptr, *t = nullptr;
    float* stats = nullptr;   // [n*32*2]
    void* gn_ws = nullptr;
    float *q = nullptr, *k = nullptr, *vT = nullptr, *S = nullptr;
    float* zq = nullptr;      // latents [n, lat_h lat_w, embed_dim]
    Act x{};                  // the current activation: in a, b or o
    GnPart part;              // epilogue partials of the most recent convolution output (buf: groupnorm_part_floats of the widest level, or null)
    RangeSites* range = nullptr;   // non-null: range-safe mode
    bool planes = false;      // split-precision mode: GroupNorm writes (hi, lo) planes, convolutions read them by LDS-DMA
    bool encoder = false;

    // ---- the rotation: the buffers that are not x
    struct Two { float *first, *second; };
    Two others() const {
        float* r[2] = {nullptr, nullptr};
        int i = 0;
        for (float* buf : {a, b, o}) if (buf != x.p && i < 2) r[i++] = buf;
        return Two{r[0], r[1]};
    }
    float* other() const { return others().first; }

    // ---- range-safe slots
    const int* range_exponent(const Act& in) {
        RangeSites& r = *range;
        BG_REQUIRE(r.used < r.cap, "vq: more range-safe sites than counted (%d)", r.cap);
        BG_REQUIRE(!r.pre_of || r.pre_of == in.p, "vq: the next range-safe slot was prepared for another tensor");
        if (r.pre_of) r.pre_of = nullptr;
        else launch_range_exponent(in.p, in.elems(), r.amax + r.used, r.exps + r.used, s);
        return r.exps + r.used++;
    }
    // the slot the NEXT site takes, for a pass that writes that site's operand `of` and leaves its exponent on the way (launch_*_amax)
    struct NextSlot { unsigned* amax; int* e; };
    NextSlot next_slot(const float* of) {
        RangeSites& r = *range;
        BG_REQUIRE(r.used < r.cap && !r.pre_of, "vq: more range-safe sites than counted (%d)", r.cap);
        r.pre_of = of;
        return NextSlot{r.amax + r.used, r.exps + r.used};
    }

    // ---- writers: every launch into a, b, o or t
    void conv1(const float* in, long rows, const ConvW& w, float* y, const float* residual) {
        note_write(part, y);
        GemmArgs g;
        g.A = in; g.B = w.w; g.C = y; g.R = residual; g.bias_n = w.b;
        g.M = (int)rows; g.N = w.cout; g.K = w.cin;
        g.lda = w.cin; g.ldb = w.cin; g.ldc = w.cout; g.ldr = w.cout;
        launch_gemm(g, s);
    }
    // stats: the LDS-DMA kernel (plane input) also leaves the GroupNorm partial sums of its output where the shape allows: the consumer's statistics pass disappears
    void conv3(const Act& in, const ConvW& w, float* y, ConvGeom geom, const float* residual = nullptr, bool stats = true) {
        note_write(part, y);
        GemmArgs g = conv3_args(in, w, geom);
        g.C = y; g.R = residual;
        if (stats && vq_switches().gn_epilogue && part.buf && in.planes && groupnorm_partials_supported(g.conv_h * g.conv_w, w.cout)) { g.gn_part = part.buf; part.of = y; }
        launch_gemm(g, s);
    }
    // statistics of `in`: from the producing convolution's epilogue partials when they describe exactly this tensor, else the pass over the tensor
    void gn_stats(const Act& in) {
        if (part.of == in.p && part.buf) launch_groupnorm_stats_from_partials(part.buf, stats, in.n, in.h * in.w, in.c, 1e-6f, s);
        else launch_groupnorm_stats(in.p, stats, gn_ws, in.n, in.h * in.w, in.c, 1e-6f, s);
    }
    Act gn(const Act& in, const float* w, const float* b_, float* y, int swish, bool as_planes) {
        gn_stats(in);
        note_write(part, y);
        if (as_planes) launch_groupnorm_apply_planes(in.p, stats, w, b_, y, in.n, in.h * in.w, in.c, swish, s);
        else launch_groupnorm_apply(in.p, stats, w, b_, y, in.n, in.h * in.w, in.c, swish, s);
        return Act{y, in.n, in.h, in.w, in.c, as_planes};
    }
    // `in` (x 2^-e with an exponent) as the (hi, lo) plane image
    Act to_planes(const Act& in, float* y, const int* e) {
        note_write(part, y);
        if (e) launch_range_split(in.p, y, (long)in.n * in.h * in.w, in.c, e, s);
        else launch_to_planes(in.p, y, in.n, in.h * in.w, in.c, s);
        return Act{y, in.n, in.h, in.w, in.c, true};
    }
    Act scale(const Act& in, float* y, const int* e) {
        note_write(part, y);
        launch_range_scale(in.p, y, in.elems(), e, s);
        return Act{y, in.n, in.h, in.w, in.c};
    }
    // y = 2^e y + b over y [n, hw, w.cout]
    void unscale(float* y, const ConvW& w, int n, int hw, const int* e, const RangedOpts& o_) {
        note_write(part, y);
        const long rows = (long)n * hw;
        if (o_.y_feeds_site && vq_switches().enc_fuse) {
            const NextSlot nx = next_slot(y);
            launch_range_unscale_amax(y, w.b, rows, w.cout, e, nx.amax, nx.e, s);
            return;
        }
        const bool leave = o_.leave_partials && vq_switches().gn_epilogue && part.buf && groupnorm_partials_supported(hw, w.cout);
        launch_range_unscale(y, w.b, nullptr, rows, w.cout, e, leave ? part.buf : nullptr, s);
        if (leave) part.of = y;
    }
    // the encoder's image, NCHW -> NHWC with the channels padded, into t; range-safe mode: the layout change also leaves the image's exponent, so that conv_in's site needs
    // no pass of its own over the padded tensor
    Act load_image(const float* x_nchw, int n, int h, int w, int cin, int cin_pad) {
        note_write(part, t);
        if (range && vq_switches().enc_fuse) {
            const NextSlot nx = next_slot(t);
            launch_nchw_to_nhwc_pad_amax(x_nchw, t, n, h * w, cin, cin_pad, nx.amax, nx.e, s);
        } else {
            launch_nchw_to_nhwc_pad(x_nchw, t, n, h * w, cin, cin_pad, s);
        }
        return Act{t, n, h, w, cin_pad};
    }

    // ---- the range-safe site (RangedOpts)
    void ranged(const Act& in, const ConvW& w, float* tmp, float* y, const RangedOpts& o_) {
        const int* e = o_.e ? o_.e : range_exponent(in);
        const Act xs = o_.plane_operand ? to_planes(in, tmp, e) : scale(in, tmp, e);
        ConvW wb = w;
        wb.b = nullptr;
        const int hw = o_.k == 1 || o_.geom == CONV_SAME ? in.h * in.w : o_.geom == CONV_UP2 ? 4 * in.h * in.w : (in.h / 2) * (in.w / 2);
        if (o_.k == 1) conv1(tmp, (long)in.n * hw, wb, y, nullptr);
        else conv3(xs, wb, y, o_.geom, nullptr, false);
        unscale(y, w, in.n, hw, e, o_);
    }

    // ---- steps: x -> the step's output
    void conv_in(const Act& in, const ConvW& w) {   // `in` is in t
        if (range) ranged(in, w, b, a, RangedOpts{});
        else conv3(in, w, a, CONV_SAME);
        x = Act{a, in.n, in.h, in.w, w.cout};
    }
    void res(const ResBlockW& r) {
        const Two free = others();
        float *scratch = free.first, *y = free.second;
        // h = conv1(swish(norm1(x)));  split-precision mode: the normalised activation is written directly as the (hi, lo) planes the convolution reads
        conv3(gn(x, r.n1w, r.n1b, t, 1, planes), r.c1, scratch, CONV_SAME);
        const Act t2 = gn(Act{scratch, x.n, x.h, x.w, r.cout}, r.n2w, r.n2b, t, 1, planes);
        const float* shortcut = x.p;
        if (r.has_nin) {  // x = nin_shortcut(x)  (1x1), written over h1 (no longer needed after norm2)
            RangedOpts one;
            one.k = 1;
            if (range) ranged(x, r.nin, y, scratch, one);   // (y is free until conv2 writes it)
            else conv1(x.p, (long)x.n * x.h * x.w, r.nin, scratch, nullptr);
            shortcut = scratch;
        }
        conv3(t2, r.c2, y, CONV_SAME, shortcut);  // y = x + conv2(...); its epilogue also leaves the statistics the next block's norm1 needs
        x = Act{y, x.n, x.h, x.w, r.cout};
    }
    void attn(const AttnBlockW& ab) {
        float* y = encoder ? others().second : other();   // (the two directions have always rotated differently here)
        const int hw = x.h * x.w, C = ab.c, n = x.n;
        const int hwp = (int)round_up(hw, 32);   // key dimension padded to the GEMM's k granularity (non-square latents: 14 x 25 = 350 -> 352); pad keys carry P = 0, v = 0
        const long rows = (long)n * hw;
        gn(x, ab.nw, ab.nb, t, 0, false);
        conv1(t, rows, ab.q, q, nullptr);
        conv1(t, rows, ab.k, k, nullptr);
        if (hwp != hw) HIP_CHECK(hipMemsetAsync(vT, 0, (size_t)n * C * hwp * sizeof(float), s));
        {   // vT[img] [C, hw] = Wv [C,C] * h_img^T + bias (per row)
            GemmArgs g;
            g.A = ab.v.w; g.B = t; g.C = vT; g.bias_m = ab.v.b;
            g.M = C; g.N = hw; g.K = C; g.lda = C; g.ldb = C; g.ldc = hwp;
            g.batch = n; g.strideA = 0; g.strideB = (long)hw * C; g.strideC = (long)C * hwp;
            launch_gemm(g, s);
        }
        {   // S[img] [hw, hw] = q k^T
            GemmArgs g;
            g.A = q; g.B = k; g.C = S;
            g.M = hw; g.N = hw; g.K = C; g.lda = C; g.ldb = C; g.ldc = hwp;
            g.batch = n; g.strideA = (long)hw * C; g.strideB = (long)hw * C; g.strideC = (long)hw * hwp;
            launch_gemm(g, s);
        }
        launch_row_softmax(S, (int)rows, hw, 1.0f / sqrtf((float)C), s, hwp);  // w_ * int(c)**-0.5, softmax over keys
        {   // O[img] [hw, C] = P [hw,hw] * v [hw, C]  (B operand = vT [C, hw])
            GemmArgs g;
            g.A = S; g.B = vT; g.C = q;  // reuse q as the output buffer
            g.M = hw; g.N = C; g.K = hwp; g.lda = hwp; g.ldb = hwp; g.ldc = C;
            g.batch = n; g.strideA = (long)hw * hwp; g.strideB = (long)C * hwp; g.strideC = (long)hw * C;
            launch_gemm(g, s);
        }
        conv1(q, rows, ab.proj, y, x.p);  // x + proj_out(h)
        x = Act{y, n, x.h, x.w, C};
    }
    // Upsample: nearest 2x + 3x3 conv, fused (the three forms: vq_plan.h)
    void up(const ConvW& w) {
        float* y = other();
        RangedOpts ro;
        ro.geom = CONV_UP2;
        switch (vq_up_form(x.c, planes, range != nullptr, vq_switches())) {
        case VQ_UP_PLANES:
            ro.plane_operand = ro.leave_partials = true;
            if (range) ranged(x, w, t, y, ro);
            else conv3(to_planes(x, t, nullptr), w, y, CONV_UP2);
            break;
        case VQ_UP_RANGED_F32: ranged(x, w, t, y, ro); break;
        case VQ_UP_PLAIN: conv3(x, w, y, CONV_UP2); break;
        }
        x = Act{y, x.n, x.h * 2, x.w * 2, w.cout};
    }
    // Downsample; feeds_site: the output is the operand of the next level's nin_shortcut (vq_feeds_nin)
    void down(const ConvW& w, bool feeds_site) {
        const Two free = others();
        RangedOpts ro;
        ro.geom = CONV_DOWN2;
        ro.y_feeds_site = feeds_site;
        if (range) ranged(x, w, free.first, free.second, ro);
        else conv3(x, w, free.second, CONV_DOWN2);
        x = Act{free.second, x.n, x.h / 2, x.w / 2, w.cout};
    }
    // Decoder.forward's last operators (norm_out, swish, conv_out) + denormalise + NCHW / uint8 store: one kernel, or (TailOut::fused = false, or a shape it does not take) three
    void tail(const float* nw, const float* nb, const ConvW& co, const TailOut& to) {
        const int denorm = to.out_mode != 0;
        const float *mean = denorm ? to.mean : nullptr, *stdv = denorm ? to.stdv : nullptr;
        float* of = to.out_mode == 2 ? nullptr : reinterpret_cast<float*>(to.out);
        uint8_t* o8 = to.out_mode == 2 ? reinterpret_cast<uint8_t*>(to.out) : nullptr;
        if (to.fused && vq_out_conv_supported(x.c, co.cout)) {   // norm_out + swish + conv_out + denormalise + layout in one kernel
            gn_stats(x);
            launch_vq_out_conv(x.p, stats, nw, nb, co.w, co.b, mean, stdv, denorm, of, o8, x.n, x.h, x.w, x.c, co.cout, s);
            return;
        }
        conv3(gn(x, nw, nb, t, 1, planes), co, to.img, CONV_SAME, nullptr, false);  // [n, h w, cout]
        launch_nhwc_to_nchw(to.img, of, x.n, x.h * x.w, co.cout, co.cout, mean, stdv, denorm, s, o8);
    }
    // Encoder.forward's last operators and quant_conv (1x1): x -> zq [n, lat_h lat_w, embed_dim]
    // geo: the camera-ray embedding is added to conv_out's output in place, in front of quant_conv and of its range-safe site (whose exponent is therefore that of the sum)
    void to_latents(const float* nw, const float* nb, const ConvW& conv_out, const ConvW& quant_conv, const GeoEmbed* geo) {
        const Two free = others();
        conv3(gn(x, nw, nb, t, 1, planes), conv_out, free.second, CONV_SAME, nullptr, false);   // [n, lat_h lat_w, z_channels]
        if (geo) {
            note_write(part, free.second);
            launch_vq_geo_embed(free.second, geo->I_inv, geo->E_inv, geo->plane, geo->wimg, geo->wcam, x.n, x.h * x.w, conv_out.cout, s);
        }
        RangedOpts one;
        one.k = 1;
        if (range) ranged(Act{free.second, x.n, x.h, x.w, conv_out.cout}, quant_conv, free.first, zq, one);
        else conv1(free.second, (long)x.n * x.h * x.w, quant_conv, zq, nullptr);
    }
};

// The workspace of a pass over n images (layout functions, arena.h): metered for the largest pass, carved per pass.  Allocation order and sizes are part of the measured
// arena bytes and stay as they are.
struct DecBufs { float* img = nullptr; };                    // pixel staging of the three-kernel tail [n, RH RW, max(4, out_ch)]: its convolution writes ldc = out_ch
inline size_t tail_staging_floats(long pixels, int cout) { return (size_t)pixels * (size_t)std::max(4, cout); }   // (4 for every out_ch <= 4: the measured arena bytes of the camera decoder)
struct EncBufs { float *dots = nullptr, *zz = nullptr; };   // codebook products [n lat_h lat_w, n_embed] and row norms of the quantizer

DecBufs dec_layout(Arena& a, Pass& p, const VqSizes& z, int embed_dim, int out_ch, int n) {
    DecBufs d;
    if (p.planes) p.part.buf = a.get<float>((size_t)z.per_img * n / 64 + 64);   // GroupNorm partials of one tensor: (pixels / 32) x (channels / 4) x 2
    p.a = a.get<float>((size_t)z.per_img * n);
    p.b = a.get<float>((size_t)z.per_img * n);
    p.t = a.get<float>((size_t)z.per_img * n);
    p.stats = a.get<float>((size_t)n * 64);
    p.gn_ws = a.alloc(groupnorm_ws_bytes(n, z.RH * z.RW));
    p.q = a.get<float>((size_t)n * z.attn_hwp * z.max_c);
    p.k = a.get<float>((size_t)n * z.attn_hwp * z.max_c);
    p.vT = a.get<float>((size_t)n * z.attn_hwp * z.max_c);
    p.S = a.get<float>((size_t)n * z.attn_hwp * z.attn_hwp);
    p.zq = a.get<float>((size_t)n * z.lat_h * z.lat_w * embed_dim);
    d.img = a.get<float>(tail_staging_floats((long)n * z.RH * z.RW, out_ch));
    p.o = a.get<float>((size_t)z.per_img * n);
    return d;
}

// The encoder allocates NO partials buffer (p.part.buf stays null), so its convolutions never leave epilogue statistics and every GroupNorm runs the statistics pass:
// an asymmetry with the decoder that is measured behaviour, kept as it is.
EncBufs enc_layout(Arena& a, Pass& p, const VqSizes& z, int embed_dim, int n_embed, int n) {
    EncBufs e;
    const size_t lrows = (size_t)n * z.lat_h * z.lat_w;
    p.a = a.get<float>((size_t)z.per_img * n);
    p.b = a.get<float>((size_t)z.per_img * n);
    p.t = a.get<float>((size_t)z.per_img * n);
    p.o = a.get<float>((size_t)z.per_img * n);
    p.stats = a.get<float>((size_t)n * 64);
    p.gn_ws = a.alloc(groupnorm_ws_bytes(n, z.RH * z.RW));
    p.q = a.get<float>((size_t)n * z.attn_hwp * z.max_c);
    p.k = a.get<float>((size_t)n * z.attn_hwp * z.max_c);
    p.vT = a.get<float>((size_t)n * z.attn_hwp * z.max_c);
    p.S = a.get<float>((size_t)n * z.attn_hwp * z.attn_hwp);
    e.dots = a.get<float>(lrows * n_embed);
    p.zq = a.get<float>(lrows * embed_dim);
    e.zz = a.get<float>(lrows);
    return e;
}

// VectorQuantizer2.forward (stage1/quantize.py:271-312): ids = argmin_j (|z|^2 + |e_j|^2) - 2 z.e_j, exact fp32 products (the codebook is never split); ee = |e_j|^2
struct Codebook { const float *e, *ee; int n_e, D; };
void quantize(const float* z, long rows, const Codebook& cb, float* zz, float* dots, int64_t* ids, hipStream_t s) {
    launch_row_sqnorm(z, zz, rows, cb.D, s);
    GemmArgs gd;
    gd.A = z; gd.B = cb.e; gd.C = dots;
    gd.M = (int)rows; gd.N = cb.n_e; gd.K = cb.D; gd.lda = cb.D; gd.ldb = cb.D; gd.ldc = cb.n_e;
    launch_gemm(gd, s);
    launch_vq_argmin(dots, zz, cb.ee, ids, rows, cb.n_e, s);
}

ConvW load_conv_in_padded(Ctx& c, const std::string& name, int cin_pad) {
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

// Encoder + quantizer weights (vq_encode below)
void vq_enc_finalize(Ctx& c) {
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
    // img_embed / cam_embed of VQModel(geometric_embedding=True): 1x1 convolutions [z_channels, 4, 1, 1] without a bias, read as [z_channels, 4]
    const DevTensor *wi = c.find(kPrefix + "img_embed.weight"), *wc = c.find(kPrefix + "cam_embed.weight");
    BG_REQUIRE((wi != nullptr) == (wc != nullptr), "geometric embedding: img_embed.weight and cam_embed.weight come together ('%s' is missing)", wi ? "cam_embed.weight" : "img_embed.weight");
    c.has_vq_geo = wi != nullptr;
    if (c.has_vq_geo) {
        for (const DevTensor* w : {wi, wc})
            BG_REQUIRE(w->shape.size() == 4 && w->shape[0] == g.vq_z_channels && w->shape[1] == 4 && w->shape[2] == 1 && w->shape[3] == 1,
                       "geometric embedding: img_embed.weight / cam_embed.weight must be [z_channels = %d, 4, 1, 1] (cam_emd_dim == z_channels)", g.vq_z_channels);
        c.vq_geo_wimg = wi->f();
        c.vq_geo_wcam = wc->f();
    }
    c.vq_enc_shape = shape_of(g, true, c.enc_cin_pad, c.enc_mid1, c.enc_mid2);
    for (int lvl = 0; lvl < g.vq_num_levels; ++lvl) shape_level(c.vq_enc_shape, lvl, c.down[lvl].blocks, !c.down[lvl].attns.empty(), c.down[lvl].has_down);
}

}  // namespace

void vq_finalize(Ctx& c) {
    const auto& g = c.cfg;
    BG_REQUIRE(g.vq_num_levels >= 1 && g.vq_num_levels <= kVqMaxLevels, "vq_num_levels out of range");
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
    c.vq_dec_shape = shape_of(g, false, 0, c.mid1, c.mid2);
    for (int lvl = 0; lvl < g.vq_num_levels; ++lvl) shape_level(c.vq_dec_shape, lvl, c.up[lvl].blocks, !c.up[lvl].attns.empty(), c.up[lvl].has_up);
}

// The decoder on a latent grid of lat_h x lat_w (sizes: vq_scan).
// out_mode: 0 = raw fp32, 1 = denormalised fp32 in [0,1], 2 = denormalised uint8 round(x*255) (`out` then points to uint8).
void vq_decode(Ctx& c, const int64_t* ids, const float* latents_nchw, int n_total, int lat_h, int lat_w, int out_mode, void* out, hipStream_t s) {
    BG_REQUIRE(c.has_vq, "this context holds no VQGAN decoder weights (decoder.* tensors were not loaded)");
    const auto& g = c.cfg;
    BG_REQUIRE(lat_h >= 1 && lat_w >= 1, "vq_decode: latent grid %d x %d", lat_h, lat_w);
    BG_REQUIRE(out_mode == 0 || g.vq_out_ch == 3, "denormalize needs 3 output channels");
    BG_REQUIRE(c.conv_out.cout == g.vq_out_ch, "vq_decode: decoder.conv_out has %d output channels, the configuration says out_ch = %d", c.conv_out.cout, g.vq_out_ch);
    Pass proto;
    proto.s = s;
    proto.planes = g.precision == BEVGEN_PRECISION_F16X3;
    const VqSizes z = vq_scan(c.vq_dec_shape, lat_h, lat_w);
    const VqPasses cut = vq_pass_cut(n_total);
    const long lat_hw = (long)lat_h * lat_w;
    c.arena.reserve(Arena::measure([&](Arena& a) { Pass p = proto; dec_layout(a, p, z, g.vq_embed_dim, c.conv_out.cout, cut.chunk); }));
    RangeSites sites = sites_reserve(c, proto.planes && g.vq_range ? vq_sites_per_pass(c.vq_dec_shape) * cut.passes : 0, s);
    if (sites.cap) proto.range = &sites;
    for (int i0 = 0; i0 < n_total; i0 += cut.chunk) {
        const int n = std::min(cut.chunk, n_total - i0);
        c.arena.reset();
        Pass p = proto;
        const DecBufs d = dec_layout(c.arena, p, z, g.vq_embed_dim, c.conv_out.cout, n);
        if (ids) launch_codebook_gather(ids + (long)i0 * lat_hw, c.codebook, p.zq, (int)(n * lat_hw), g.vq_embed_dim, g.vq_n_embed, s);
        else launch_nchw_to_nhwc(latents_nchw + (long)i0 * g.vq_embed_dim * lat_hw, p.zq, n, (int)lat_hw, g.vq_embed_dim, s);
        p.conv1(p.zq, n * lat_hw, c.post_quant, p.t, nullptr);                       // post_quant_conv
        p.conv_in(Act{p.t, n, lat_h, lat_w, g.vq_z_channels}, c.conv_in);
        p.res(c.mid1);
        p.attn(c.mid_attn);
        p.res(c.mid2);
        for (int lvl = g.vq_num_levels - 1; lvl >= 0; --lvl) {
            const UpLevelW& u = c.up[lvl];
            for (size_t b = 0; b < u.blocks.size(); ++b) {
                p.res(u.blocks[b]);
                if (!u.attns.empty()) p.attn(u.attns[b]);
            }
            if (u.has_up) p.up(u.up);
        }
        const long o_off = (long)i0 * g.vq_out_ch * z.RH * z.RW;
        void* o_ptr = out_mode == 2 ? static_cast<void*>(reinterpret_cast<uint8_t*>(out) + o_off) : static_cast<void*>(reinterpret_cast<float*>(out) + o_off);
        p.tail(c.norm_out_w, c.norm_out_b, c.conv_out, TailOut{o_ptr, out_mode, c.denorm_mean, c.denorm_std, d.img, vq_switches().tail});
    }
    sites_done(c, sites);
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
// x [n, in_channels, RH, RW] with RH, RW multiples of 2^(levels-1) (fully convolutional: 256 x 256 or nuScenes' 224 x 400) -> ids [n, (RH >> (levels-1)) * (RW >> (levels-1))]
// ex: per-image geometry (a context with img_embed / cam_embed needs it, one without refuses it), row_err [n, lat_h lat_w] and the codebook loss over all rows of the call
void vq_encode(Ctx& c, const float* x_nchw, int n_total, int RH, int RW, int64_t* ids, const VqEncodeExtras& ex, hipStream_t s) {
    BG_REQUIRE(c.has_vq_enc, "this context holds no VQGAN encoder weights (encoder.* tensors were not loaded)");
    const bool geo = ex.I_inv || ex.E_inv || ex.plane;
    BG_REQUIRE(!geo || (ex.I_inv && ex.E_inv && ex.plane), "vq_encode: the geometry is I_inv, E_inv and the image plane together");
    BG_REQUIRE(!c.has_vq_geo || geo, "vq_encode: this VQGAN has a geometric embedding (img_embed / cam_embed): the call needs I_inv, E_inv and the image plane");
    BG_REQUIRE(c.has_vq_geo || !geo, "vq_encode: geometry was passed, but this VQGAN has no geometric embedding (img_embed.weight / cam_embed.weight were not loaded)");
    BG_REQUIRE(!ex.loss || ex.row_err, "vq_encode: the loss is taken over row_err, which the caller provides");
    const auto& g = c.cfg;
    const int f = 1 << (g.vq_num_levels - 1);
    BG_REQUIRE(RH >= f && RW >= f && RH % f == 0 && RW % f == 0, "vq_encode: image %d x %d is not a multiple of the downsampling factor %d", RH, RW, f);
    Pass proto;
    proto.s = s;
    proto.planes = g.precision == BEVGEN_PRECISION_F16X3;
    proto.encoder = true;
    const VqSizes z = vq_scan(c.vq_enc_shape, RH, RW);
    const VqPasses cut = vq_pass_cut(n_total);
    const long lat_hw = (long)z.lat_h * z.lat_w;
    c.arena.reserve(Arena::measure([&](Arena& a) { Pass p = proto; enc_layout(a, p, z, g.vq_embed_dim, g.vq_n_embed, cut.chunk); }));
    RangeSites sites = sites_reserve(c, proto.planes && g.vq_range ? vq_sites_per_pass(c.vq_enc_shape) * cut.passes : 0, s);
    if (sites.cap) proto.range = &sites;
    for (int i0 = 0; i0 < n_total; i0 += cut.chunk) {
        const int n = std::min(cut.chunk, n_total - i0);
        c.arena.reset();
        Pass p = proto;
        const EncBufs e = enc_layout(c.arena, p, z, g.vq_embed_dim, g.vq_n_embed, n);
        p.conv_in(p.load_image(x_nchw + (long)i0 * g.vq_in_channels * RH * RW, n, RH, RW, g.vq_in_channels, c.enc_cin_pad), c.enc_conv_in);
        for (int lvl = 0; lvl < g.vq_num_levels; ++lvl) {
            const DownLevelW& d = c.down[lvl];
            for (size_t b = 0; b < d.blocks.size(); ++b) {
                p.res(d.blocks[b]);
                if (!d.attns.empty()) p.attn(d.attns[b]);
            }
            if (d.has_down) p.down(d.down, vq_feeds_nin(c.vq_enc_shape, lvl));
        }
        p.res(c.enc_mid1);
        p.attn(c.enc_mid_attn);
        p.res(c.enc_mid2);
        const GeoEmbed ge{geo ? ex.I_inv + (long)i0 * 9 : nullptr, geo ? ex.E_inv + (long)i0 * 16 : nullptr, ex.plane, c.vq_geo_wimg, c.vq_geo_wcam};
        p.to_latents(c.enc_norm_out_w, c.enc_norm_out_b, c.enc_conv_out, c.quant_conv, geo ? &ge : nullptr);
        quantize(p.zq, n * lat_hw, Codebook{c.codebook, c.codebook_sqnorm, g.vq_n_embed, g.vq_embed_dim}, e.zz, e.dots, ids + (long)i0 * lat_hw, s);
        if (ex.row_err) launch_vq_row_err(p.zq, c.codebook, ids + (long)i0 * lat_hw, ex.row_err + (long)i0 * lat_hw, n * lat_hw, g.vq_n_embed, g.vq_embed_dim, s);
    }
    sites_done(c, sites);
    if (ex.loss) launch_vq_loss(ex.row_err, (long)n_total * lat_hw, g.vq_embed_dim, ex.beta, ex.loss, s);   // once, over all rows of all passes
}

// =====================================================================================================
// Operator entries (bevgen_op_* in api.cpp): the pieces above on caller-supplied device tensors, at shapes of their own.  They forward to the launchers / Pass methods the
// model path uses and add no arithmetic.  Weights arrive as the checkpoint stores them ([Cout][Cin][kh][kw]) and are prepared the way load_conv prepares them, into the arena.
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

// an operator's pass: the caller's input is the current activation
Pass op_pass(const Ctx& c, hipStream_t s, const float* x, int n, int h, int w, int C) {
    Pass p;
    p.s = s;
    p.planes = c.cfg.precision == BEVGEN_PRECISION_F16X3;
    p.x = Act{const_cast<float*>(x), n, h, w, C};
    return p;
}

}  // namespace

void vq_op_conv3x3_down(Ctx& c, const float* x, const float* w, const float* bias, float* y, int n, int H, int W, int Cin, int Cout, hipStream_t s) {
    BG_REQUIRE(n >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && Cin >= 32 && Cin % 32 == 0 && Cout >= 1,
               "op_conv3x3_down: needs even H, W and Cin %% 32 == 0 (H=%d W=%d Cin=%d)", H, W, Cin);
    OpWeights::Buf wb;
    c.arena.carve([&](Arena& a) { wb = OpWeights::take(c, a, Cout, Cin, 3); });
    OpWeights ow(c, s);
    const ConvW cw = ow.conv(wb, w, bias, Cout, Cin, 3);
    Pass p = op_pass(c, s, x, n, H, W, Cin);
    p.conv3(p.x, cw, y, CONV_DOWN2);
}

// one range-safe site as vq_decode / vq_encode run it (Pass::ranged); kind 0: 1x1, 1: 3x3, 2: the Downsample.  kind 2 ends in the fused pass (y_feeds_site) as a
// downsample in front of a nin_shortcut does; the exponent that pass leaves for y stays in the arena.  Two slots, of which kinds 0 and 1 use one.
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
    Pass p = op_pass(c, s, x, n, H, W, Cin);
    p.range = &sites;
    RangedOpts ro;
    ro.k = k;
    if (kind == 2) { ro.geom = CONV_DOWN2; ro.y_feeds_site = true; }
    p.ranged(p.x, cw, tmp, y, ro);
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
    Pass p = op_pass(c, s, x, n, h, w, C);
    p.a = y;   // the rotation's one free buffer: the caller's output
    c.arena.carve([&](Arena& ar) {
        for (OpWeights::Buf& b : wb) b = OpWeights::take(c, ar, C, C, 1);
        p.t = ar.get<float>((size_t)n * hw * C);
        p.stats = ar.get<float>((size_t)n * 64);
        p.gn_ws = ar.alloc(groupnorm_ws_bytes(n, (int)hw));
        p.q = ar.get<float>(qb / f);
        p.k = ar.get<float>(qb / f);
        p.vT = ar.get<float>(qb / f);
        p.S = ar.get<float>(sb / f);
    });
    OpWeights ow(c, s);
    AttnBlockW a;
    a.nw = norm_w; a.nb = norm_b; a.c = C;
    a.q = ow.conv(wb[0], wq, bq, C, C, 1); a.k = ow.conv(wb[1], wk, bk, C, C, 1); a.v = ow.conv(wb[2], wv, bv, C, C, 1); a.proj = ow.conv(wb[3], wp, bp, C, C, 1);
    // the model's workspace holds whatever the previous kernels left there: NaN bit patterns here, so that a pad column that is read without having been written shows
    HIP_CHECK(hipMemsetAsync(p.q, 0xFF, qb, s));
    HIP_CHECK(hipMemsetAsync(p.k, 0xFF, qb, s));
    HIP_CHECK(hipMemsetAsync(p.vT, 0xFF, qb, s));
    HIP_CHECK(hipMemsetAsync(p.S, 0xFF, sb, s));
    p.attn(a);
}

void vq_op_out_tail(Ctx& c, const float* x, const float* norm_w, const float* norm_b, const float* w, const float* bias, const float* mean, const float* stdv, int out_mode,
                    int three_kernels, void* out, int n, int H, int W, int C, int cout, hipStream_t s) {
    BG_REQUIRE(cout >= 1 && cout <= 64, "op_vq_out_tail: cout=%d (1 .. 64)", cout);
    BG_REQUIRE(out_mode == 0 || cout == 3, "op_vq_out_tail: denormalize needs 3 output channels (cout=%d)", cout);
    BG_REQUIRE(n >= 1 && H >= 1 && W >= 1 && C >= 32 && C % 32 == 0 && C <= 1024, "op_vq_out_tail: C=%d must be a multiple of 32 (at most 1024)", C);
    BG_REQUIRE(out_mode >= 0 && out_mode <= 2 && (out_mode == 0 || (mean && stdv)), "op_vq_out_tail: out_mode 0 / 1 / 2; 1 and 2 need mean and std");
    const long hw = (long)H * W;
    OpWeights::Buf wb;
    Pass p = op_pass(c, s, x, n, H, W, C);
    float* img;
    c.arena.carve([&](Arena& a) {
        wb = OpWeights::take(c, a, cout, C, 3);
        p.t = a.get<float>((size_t)n * hw * C);
        p.stats = a.get<float>((size_t)n * 64);
        p.gn_ws = a.alloc(groupnorm_ws_bytes(n, (int)hw));
        img = a.get<float>(tail_staging_floats(n * hw, cout));
    });
    OpWeights ow(c, s);
    const ConvW co = ow.conv(wb, w, bias, cout, C, 3);
    p.tail(norm_w, norm_b, co, TailOut{out, out_mode, mean, stdv, img, three_kernels == 0});
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
    quantize(z, rows, Codebook{codebook, ee, n_e, D}, zz, dots, ids, s);
    if (zz_out) HIP_CHECK(hipMemcpyAsync(zz_out, zz, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (ee_out) HIP_CHECK(hipMemcpyAsync(ee_out, ee, (size_t)n_e * sizeof(float), hipMemcpyDeviceToDevice, s));
}

void vq_op_quant_error(const float* z, const float* codebook, const int64_t* ids, float beta, float* row_err, float* loss, long rows, int n_e, int D, hipStream_t s) {
    BG_REQUIRE(rows >= 1 && rows <= 0x7FFFFFFFL && n_e >= 1 && D >= 32 && D % 32 == 0, "op_vq_quant_error: needs D %% 32 == 0 (rows=%ld n_e=%d D=%d)", rows, n_e, D);
    launch_vq_row_err(z, codebook, ids, row_err, rows, n_e, D, s);
    if (loss) launch_vq_loss(row_err, rows, D, beta, loss, s);
}

void vq_op_conv3x3_gn_stats(Ctx& c, const float* x, const float* w, const float* bias, int range_route, float* y, float* part, float* stats, int n, int H, int W, int Cin,
                            int Cout, hipStream_t s) {
    BG_REQUIRE(c.cfg.precision == BEVGEN_PRECISION_F16X3, "op_conv3x3_gn_stats: the convolution epilogue that leaves GroupNorm partials belongs to the split-precision mode (precision = f16x3)");
    BG_REQUIRE(vq_switches().gn_epilogue, "op_conv3x3_gn_stats: the epilogue statistics are switched off (BEVGEN_GN_EPILOGUE=0)");
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
    const ConvW cw = ow.conv(wbuf, w, bias, Cout, Cin, 3);
    Pass p = op_pass(c, s, x, n, H, W, Cin);
    p.part.buf = part;
    if (range_route) {   // the upsample site of the range-safe mode without the upsample, with a zeroed exponent: planes, the convolution without its bias, then bias + statistics in one pass
        HIP_CHECK(hipMemsetAsync(e, 0, sizeof(int), s));
        RangedOpts ro;
        ro.plane_operand = ro.leave_partials = true;
        ro.e = e;
        p.ranged(p.x, cw, planes, y, ro);
    } else {
        p.conv3(p.to_planes(p.x, planes, nullptr), cw, y, CONV_SAME);
    }
    BG_REQUIRE(p.part.of == y, "op_conv3x3_gn_stats: the convolution did not leave partials");
    launch_groupnorm_stats_from_partials(part, stats, n, hw, Cout, 1e-6f, s);
}

}  // namespace bevgen
