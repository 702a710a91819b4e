// LPIPS (VGG16) host driver: the prepared-weight image, the workspace and the launch sequence of bevgen_lpips (kernels: lpips_kernels.hip; convolutions: launch_gemm, MODE_CONV3
// with the ACT_RELU epilogue).  Image pairs run in chunks of lpips_chunk(H, W, precision): a and b of a chunk are ONE batch of 2 m images, so every convolution is one
// launch per chunk, and the workspace does not depend on n beyond the first chunk.
//
// Both memory images (prepared weights, workspace) are caller-owned and are carved by ONE layout function each, run on a metering Arena for the size and on the caller's
// block for the pointers (arena.h, the workspace rule).
//
// Split-precision contexts: conv1_1 reads the planes the preparation kernel wrote, a convolution behind a pool the planes the pool wrote, and a convolution behind another
// convolution the planes of launch_to_planes (the existing splitter) over the fp32 ReLU output - which the taps need in fp32 anyway.
#include <algorithm>

#include "../../include/bevgen_hip.h"
#include "arena.h"
#include "common.h"
#include "kernels.h"

namespace bevgen {

namespace {

constexpr int kLayers = 13, kTaps = 5;
constexpr int kCin[kLayers] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int kCout[kLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr bool kPoolBefore[kLayers] = {false, false, true, false, true, false, false, true, false, false, true, false, false};
constexpr int kTapAfter[kLayers] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};   // relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
constexpr int kTapC[kTaps] = {64, 128, 256, 512, 512};
inline int cin_pad(int l) { return std::max(kCin[l], 32); }

bool precision_ok(int precision) { return precision == BEVGEN_PRECISION_FP32 || precision == BEVGEN_PRECISION_F16X3 || precision == BEVGEN_PRECISION_F16X1; }
bool shape_ok(int n, int H, int W) { return n >= 1 && H >= 16 && W >= 16 && (long)H * W <= (1L << 21); }

struct Prepared {
    float* w[kLayers];        // [Cout][3][3][Cin_pad]
    uint16_t* wp[kLayers];    // the (hi, lo) planes of w (split precision only)
    float* b[kLayers];
    float* lin[kTaps];
    float* ss;                // shift 0 .. 2, scale 4 .. 6
};
void prepared_layout(Arena& ar, bool split, Prepared& p) {
    for (int l = 0; l < kLayers; ++l) {
        const size_t elems = (size_t)kCout[l] * 9 * cin_pad(l);
        p.w[l] = ar.get<float>(elems);
        p.wp[l] = split ? ar.get<uint16_t>(2 * elems) : nullptr;
        p.b[l] = ar.get<float>(kCout[l]);
    }
    for (int k = 0; k < kTaps; ++k) p.lin[k] = ar.get<float>(kTapC[k]);
    p.ss = ar.get<float>(8);
}

struct Work {
    float *x0, *x1;     // two activation buffers, each the largest tensor: 2 m H W 64 floats
    void* planes;       // the operand plane image of the convolution about to run (split precision only), the same bytes
    double* partial;    // m x the most workgroups a tap launches per image
    double* layers;     // [m, 5]
};
void work_layout(Arena& ar, bool split, int m, int H, int W, Work& k) {
    const size_t act = (size_t)2 * m * H * W * 64;
    k.x0 = ar.get<float>(act);
    k.x1 = ar.get<float>(act);
    k.planes = split ? ar.alloc(act * sizeof(float)) : nullptr;
    int blocks = 1, h = H, w = W;
    for (int t = 0; t < kTaps; ++t) {
        blocks = std::max(blocks, lpips_tap_blocks(h * w, kTapC[t]));
        h /= 2, w /= 2;
    }
    k.partial = ar.get<double>((size_t)m * blocks);
    k.layers = ar.get<double>((size_t)m * kTaps);
}

// the caller's block as an arena (never grown or released)
Arena over(void* base, size_t bytes) {
    Arena ar;
    ar.base = static_cast<char*>(base);
    ar.cap = bytes;
    return ar;
}

}  // namespace

int lpips_chunk(int H, int W, int precision) {
    (void)precision;   // (both arithmetic modes hold two fp32 activations per pair; the plane image of the split modes is budgeted in lpips_workspace_bytes)
    return (int)std::max<long>(1, std::min<long>((1L << 18) / ((long)H * W), 64));   // four pairs of 256 x 256 per pass
}

long lpips_prepared_bytes(int precision) {
    if (!precision_ok(precision)) return -1;
    Prepared p;
    return (long)Arena::measure([&](Arena& ar) { prepared_layout(ar, precision != BEVGEN_PRECISION_FP32, p); });
}

long lpips_workspace_bytes(int n, int H, int W, int precision) {
    if (!precision_ok(precision) || !shape_ok(n, H, W)) return -1;
    Work k;
    const int m = std::min(n, lpips_chunk(H, W, precision));
    return (long)Arena::measure([&](Arena& ar) { work_layout(ar, precision != BEVGEN_PRECISION_FP32, m, H, W, k); });
}

void lpips_prepare(bool split, const float* const* w_oihw, const float* const* bias, const float* const* lin, const float* shift, const float* scale, void* prepared,
                   hipStream_t s) {
    BG_REQUIRE(w_oihw && bias && lin && shift && scale && prepared, "lpips_prepare: null argument");
    BG_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0, "lpips_prepare: d_prepared must be 256-byte aligned");
    for (int l = 0; l < kLayers; ++l) BG_REQUIRE(w_oihw[l] && bias[l], "lpips_prepare: convolution %d has no weight or bias", l);
    for (int k = 0; k < kTaps; ++k) BG_REQUIRE(lin[k], "lpips_prepare: lin%d is missing", k);
    Prepared p;
    Arena ar = over(prepared, (size_t)lpips_prepared_bytes(split ? BEVGEN_PRECISION_F16X3 : BEVGEN_PRECISION_FP32));
    prepared_layout(ar, split, p);
    for (int l = 0; l < kLayers; ++l) {
        launch_conv_weight_relayout(w_oihw[l], p.w[l], kCout[l], kCin[l], cin_pad(l), s);
        if (split) launch_split_weight(p.w[l], p.wp[l], (long)kCout[l] * 9 * cin_pad(l), s);
        HIP_CHECK(hipMemcpyAsync(p.b[l], bias[l], sizeof(float) * kCout[l], hipMemcpyDeviceToDevice, s));
    }
    for (int k = 0; k < kTaps; ++k) HIP_CHECK(hipMemcpyAsync(p.lin[k], lin[k], sizeof(float) * kTapC[k], hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemsetAsync(p.ss, 0, sizeof(float) * 8, s));
    HIP_CHECK(hipMemcpyAsync(p.ss, shift, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(p.ss + 4, scale, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
}

void lpips_run(bool split, const void* prepared, const void* a, const void* b, int dtype, int n, int H, int W, int normalize, double* out, double* layers, void* work,
               hipStream_t s) {
    BG_REQUIRE(prepared && a && b && out && work, "lpips: null argument");
    BG_REQUIRE(dtype == BEVGEN_DTYPE_F32 || dtype == BEVGEN_DTYPE_U8, "lpips: images of dtype %d (needs fp32 or uint8)", dtype);
    BG_REQUIRE(shape_ok(n, H, W), "lpips: images [%d, 3, %d, %d] (needs n >= 1, H and W >= 16 so that relu5_3 has a pixel, H W <= 2^21)", n, H, W);
    BG_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0 && (reinterpret_cast<uintptr_t>(work) & 255) == 0, "lpips: d_prepared and d_work must be 256-byte aligned");
    const int precision = split ? BEVGEN_PRECISION_F16X3 : BEVGEN_PRECISION_FP32;
    const int chunk = std::min(n, lpips_chunk(H, W, precision));
    Prepared p;
    Arena pa = over(const_cast<void*>(prepared), (size_t)lpips_prepared_bytes(precision));
    prepared_layout(pa, split, p);
    Work k;
    Arena wa = over(work, (size_t)lpips_workspace_bytes(n, H, W, precision));
    work_layout(wa, split, chunk, H, W, k);
    const size_t image_bytes = (size_t)3 * H * W * (dtype == BEVGEN_DTYPE_U8 ? 1 : 4);

    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        double* lay = layers ? layers + (long)i0 * kTaps : k.layers;
        float *cur = k.x0, *nxt = k.x1;
        int h = H, w = W, c = 32;
        launch_lpips_prep(static_cast<const char*>(a) + i0 * image_bytes, static_cast<const char*>(b) + i0 * image_bytes, dtype, m, H * W, normalize, p.ss, split ? nullptr : cur,
                          split ? k.planes : nullptr, s);
        for (int l = 0; l < kLayers; ++l) {
            if (kPoolBefore[l]) {   // cur = the tap tensor: pooled into the next convolution's operand
                launch_maxpool2x2(cur, split ? nullptr : nxt, split ? k.planes : nullptr, 2 * m, h, w, c, s);
                h /= 2, w /= 2;
                if (!split) std::swap(cur, nxt);
            } else if (split && l > 0) {
                launch_to_planes(cur, k.planes, 2 * m, h * w, c, s);
            }
            GemmArgs g;
            g.mode = MODE_CONV3;
            if (split) {
                g.A_hi = static_cast<const uint16_t*>(k.planes); g.A_lo = g.A_hi + 32;
                g.B_hi = p.wp[l]; g.B_lo = p.wp[l] + 32;
            } else {
                g.A = cur;
                g.acc_flush = true;   // (K up to 4608: the single fp32 accumulation chain is too long for the deep taps, gemm.hip)
            }
            g.B = p.w[l]; g.bias_n = p.b[l]; g.C = nxt; g.act = ACT_RELU;
            g.M = 2 * m * h * w; g.N = kCout[l]; g.K = 9 * c;
            g.lda = c; g.ldb = 9 * c; g.ldc = kCout[l]; g.ldr = kCout[l];
            g.conv_h = h; g.conv_w = w; g.conv_cin = c;
            launch_gemm(g, s);
            std::swap(cur, nxt);
            c = kCout[l];
            const int t = kTapAfter[l];
            if (t >= 0) launch_lpips_tap(cur, cur + (long)m * h * w * c, p.lin[t], m, h * w, c, k.partial, lay + t, kTaps, s);
        }
        launch_lpips_total(lay, out + i0, m, s);
    }
}

}  // namespace bevgen
