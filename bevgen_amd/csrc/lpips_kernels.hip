// Kernels of LPIPS with the VGG16 feature stack (the reference's modules/losses/lpips.py:41-54, 57-64, 116-122; scripts/metrics_eval.py:117,122 "PSIM/LPIPS"), around the
// thirteen 3x3 convolutions, which are the library's implicit-GEMM kernels with the ACT_RELU epilogue (gemm.hip, gemm_split_glds.hip):
//   lpips_prep_kernel      a, b NCHW (fp32 / uint8) -> one NHWC batch of 2 m images, 32 channels (3 real), (2 x - 1,) (x - shift) / scale; fp32 and / or (hi, lo) planes
//   maxpool2x2_kernel      MaxPool2d(2, 2), NHWC, float4 along C; fp32 and / or the (hi, lo) plane image the next LDS-DMA convolution reads (the tap tensor is read once)
//   lpips_tap_kernel       the distance of one tap: both feature tensors read once, one double per workgroup; lpips_tap_finish_kernel adds an image's partials in a fixed order
// Everything here is fp32 per element with double sums in a fixed order and no atomics: two calls give the same bits, and image i's value does not depend on the batch.
#include <algorithm>

#include "../../include/bevgen_hip.h"
#include "common.h"
#include "kernels.h"

namespace bevgen {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float load01(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float load01(const uint8_t* p, long i) { return __fdiv_rn((float)p[i], 255.f); }

dim3 stream_grid(long items) { return dim3((unsigned)std::max<long>(1, std::min<long>((items + kThreads - 1) / kThreads, 8192))); }

// ------------------------------------------------------------------------------------------------ input preparation
// one thread per (pixel of the 2 m images, channel quad of the 8): quad 0 holds the three scaled channels and a zero, quads 1 .. 7 are the zero padding of conv1_1's operand
template <typename T>
__global__ __launch_bounds__(kThreads) void lpips_prep_kernel(const T* __restrict__ a, const T* __restrict__ b, int m, int hw, int normalize, const float* __restrict__ ss,
                                                              float4* __restrict__ y, _Float16* __restrict__ planes, unsigned* __restrict__ status) {
    const long total = (long)2 * m * hw * 8;
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
        const int q = (int)(i & 7);
        const long pix = i >> 3;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q == 0) {
            const long img = pix / hw;
            const long p = pix - img * hw;
            const T* src = img < m ? a + img * 3 * hw : b + (img - m) * 3 * hw;
            float c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float x = load01(src, (long)k * hw + p);
                if (normalize) x = __fsub_rn(__fmul_rn(2.f, x), 1.f);
                c[k] = __fdiv_rn(__fsub_rn(x, ss[k]), ss[4 + k]);
            }
            v = make_float4(c[0], c[1], c[2], 0.f);
        }
        if (y) y[i] = v;
        if (planes) store_planes4(planes + pix * 64, q * 4, v, bad);
    }
    if (bad) status_raise(status, BG_ST_F16_RANGE);
}

// ------------------------------------------------------------------------------------------------ 2x2 max-pool
// max that keeps a NaN (torch's max_pool2d)
__device__ __forceinline__ float pool_max(float a, float b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ float4 pool_max4(float4 a, float4 b) { return make_float4(pool_max(a.x, b.x), pool_max(a.y, b.y), pool_max(a.z, b.z), pool_max(a.w, b.w)); }

// one thread per (output pixel, channel quad); rows 2 oy, 2 oy + 1 <= H - 1 and columns 2 ox, 2 ox + 1 <= W - 1 for every oy < H / 2, ox < W / 2
__global__ __launch_bounds__(kThreads) void maxpool2x2_kernel(const float4* __restrict__ x, float4* __restrict__ y, _Float16* __restrict__ planes, long total, int H, int W,
                                                              int OH, int OW, int q4, unsigned* __restrict__ status) {
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
        const long op = i / q4;
        const int cq = (int)(i - op * q4);
        const int ox = (int)(op % OW);
        const long t = op / OW;
        const int oy = (int)(t % OH);
        const long img = t / OH;
        const long base = ((img * H + 2 * oy) * W + 2 * ox) * q4 + cq;
        const long down = (long)W * q4;
        const float4 v = pool_max4(pool_max4(x[base], x[base + q4]), pool_max4(x[base + down], x[base + down + q4]));
        if (y) y[i] = v;
        // (v 1 + 0 like launch_range_split at exponent 0 and launch_to_planes: the same bits, the sign of a zero included)
        if (planes) store_planes4(planes + op * 8 * q4, cq * 4, make_float4(fmaf(v.x, 1.f, 0.f), fmaf(v.y, 1.f, 0.f), fmaf(v.z, 1.f, 0.f), fmaf(v.w, 1.f, 0.f)), bad);
    }
    if (bad) status_raise(status, BG_ST_F16_RANGE);
}

// ------------------------------------------------------------------------------------------------ tap distance
// A pixel's C channels sit on a group of LG = C / 4 lanes (C = 512: 64 lanes, two float4 each), so a wave holds 64 / LG pixels and every load instruction of a wave is one
// contiguous kilobyte.  Sums over the group: DPP row operations for 16 lanes, then v_permlane16_swap / v_permlane32_swap (common.h) - a butterfly, every lane ends with the
// same bits.  All 64 lanes stay active through the reductions: a pixel past the image's last reads the last pixel again and is left out of the sum.
//
// LPIPS_TAP_K = 20: the fp32 roundings the test bound K 2^-24 sum_c w_c 2 |d| (|fa^| + |fb^|), d = fa^ - fb^, allows per normalised value (tests/lpips_ref.py TAP_K).
//   on f^: a term of sum_c f^2 passes its fused square-and-add, at most 7 more additions inside the lane (8 channels at C = 512) and 6 butterfly steps - 14 roundings on
//          the sum, so 7 on its root - then the root itself, the + 1e-10 and the division: 10.  An error of 10 u |f^| on both values moves d^2 by 10 u 2 |d| (|fa^| + |fb^|).
//   behind it: the subtraction, d d, w (d d) and at most 7 + 6 additions of the channel sum are 16 roundings relative to non-negative terms w d^2, and
//          d^2 <= |d| (|fa^| + |fb^|) = half the bound's term: they count as 8 more.  18, stated as 20 (second-order terms; the double sums are 2^-53 each).
[[maybe_unused]] constexpr int LPIPS_TAP_K = 20;

template <int LG>
__device__ __forceinline__ float group_sum(float v) {
    v = row16_sum(v);
    if (LG >= 32) v += xor16(v);
    if (LG >= 64) v += xor32(v);
    return v;
}

template <int C>
__global__ __launch_bounds__(kThreads) void lpips_tap_kernel(const float* __restrict__ fa, const float* __restrict__ fb, const float* __restrict__ w, int pix, int G,
                                                             double* __restrict__ partial) {
    constexpr int V = C == 512 ? 2 : 1;       // float4 per lane and image
    constexpr int LG = C / (4 * V);           // lanes per pixel: 16, 32, 64, 64
    constexpr int PW = 64 / LG;               // pixels per wave
    constexpr int PB = 4 * PW;                // pixels per workgroup and iteration
    __shared__ double sh[PB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / LG, l = lane % LG;
    const long image = blockIdx.x / G;
    const int blk = (int)(blockIdx.x - image * G);
    const float4* pa = reinterpret_cast<const float4*>(fa + image * (long)pix * C);
    const float4* pb = reinterpret_cast<const float4*>(fb + image * (long)pix * C);
    float4 wv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) wv[v] = reinterpret_cast<const float4*>(w)[l + v * LG];

    double acc = 0.0;
    for (int p0 = blk * PB; p0 < pix; p0 += G * PB) {   // (the same trip count for every thread of the workgroup)
        const int p = p0 + wave * PW + grp;
        const bool valid = p < pix;
        const long row = (long)min(p, pix - 1) * (C / 4);
        float4 x[V], y[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            x[v] = pa[row + l + v * LG];
            y[v] = pb[row + l + v * LG];
        }
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            sa = fmaf(x[v].x, x[v].x, sa); sa = fmaf(x[v].y, x[v].y, sa); sa = fmaf(x[v].z, x[v].z, sa); sa = fmaf(x[v].w, x[v].w, sa);
            sb = fmaf(y[v].x, y[v].x, sb); sb = fmaf(y[v].y, y[v].y, sb); sb = fmaf(y[v].z, y[v].z, sb); sb = fmaf(y[v].w, y[v].w, sb);
        }
        sa = group_sum<LG>(sa);
        sb = group_sum<LG>(sb);
        const float na = __fadd_rn(__fsqrt_rn(sa), 1e-10f), nb = __fadd_rn(__fsqrt_rn(sb), 1e-10f);
        float t = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float xs[4] = {x[v].x, x[v].y, x[v].z, x[v].w}, ys[4] = {y[v].x, y[v].y, y[v].z, y[v].w}, ws[4] = {wv[v].x, wv[v].y, wv[v].z, wv[v].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = __fsub_rn(__fdiv_rn(xs[e], na), __fdiv_rn(ys[e], nb));
                t = __fadd_rn(t, __fmul_rn(ws[e], __fmul_rn(d, d)));
            }
        }
        t = group_sum<LG>(t);
        if (valid) acc += (double)t;
    }
    if (l == 0) sh[wave * PW + grp] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < PB; ++i) s += sh[i];
        partial[blockIdx.x] = s;
    }
}

// out[i * stride] = (image i's G partials) / pix, one wave per image: lane t adds partials t, t + 64, ... in index order, then a binary tree over the 64 lane sums
__global__ __launch_bounds__(64) void lpips_tap_finish_kernel(const double* __restrict__ partial, int G, int pix, double* __restrict__ out, int stride) {
    __shared__ double sh[64];
    const int i = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int g = t; g < G; g += 64) s += partial[(long)i * G + g];
    sh[t] = s;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) out[(long)i * stride] = sh[0] / (double)pix;
}

__global__ void lpips_total_kernel(const double* __restrict__ layers, double* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* d = layers + (long)i * 5;
    out[i] = (((d[0] + d[1]) + d[2]) + d[3]) + d[4];
}

__global__ __launch_bounds__(kThreads) void conv_weight_relayout_kernel(const float* __restrict__ w, float* __restrict__ o, long total, int Cin, int Cin_pad) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long)gridDim.x * kThreads) {
        const int ci = (int)(i % Cin_pad);
        const long r = i / Cin_pad;
        const int tap = (int)(r % 9);
        const long co = r / 9;
        o[i] = ci < Cin ? w[(co * Cin + ci) * 9 + tap] : 0.f;
    }
}

template <int C>
void tap_launch(const float* fa, const float* fb, const float* w, int n, int pix, int G, double* partial, hipStream_t s) {
    hipLaunchKernelGGL(lpips_tap_kernel<C>, dim3((unsigned)((long)n * G)), dim3(kThreads), 0, s, fa, fb, w, pix, G, partial);
    LAUNCH_CHECK();
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host side
void launch_lpips_prep(const void* a, const void* b, int dtype, int m, int hw, int normalize, const float* shift_scale, float* y, void* planes, hipStream_t s) {
    BG_REQUIRE(dtype == BEVGEN_DTYPE_F32 || dtype == BEVGEN_DTYPE_U8, "lpips: images of dtype %d (needs fp32 or uint8)", dtype);
    BG_REQUIRE(a && b && shift_scale && (y || planes) && m >= 1 && hw >= 1, "lpips_prep: bad arguments");
    const dim3 grid = stream_grid((long)2 * m * hw * 8);
    if (dtype == BEVGEN_DTYPE_F32)
        hipLaunchKernelGGL(lpips_prep_kernel<float>, grid, dim3(kThreads), 0, s, static_cast<const float*>(a), static_cast<const float*>(b), m, hw, normalize, shift_scale,
                           reinterpret_cast<float4*>(y), reinterpret_cast<_Float16*>(planes), status_current());
    else
        hipLaunchKernelGGL(lpips_prep_kernel<uint8_t>, grid, dim3(kThreads), 0, s, static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), m, hw, normalize, shift_scale,
                           reinterpret_cast<float4*>(y), reinterpret_cast<_Float16*>(planes), status_current());
    LAUNCH_CHECK();
}

void launch_maxpool2x2(const float* x, float* y, void* planes, int n, int H, int W, int C, hipStream_t s) {
    BG_REQUIRE(x && (y || planes) && n >= 1 && H >= 2 && W >= 2 && C >= 32 && C % 32 == 0, "maxpool2x2: [%d, %d, %d, %d] (needs H, W >= 2 and C a multiple of 32)", n, H, W, C);
    const int OH = H / 2, OW = W / 2;
    const long total = (long)n * OH * OW * (C / 4);
    hipLaunchKernelGGL(maxpool2x2_kernel, stream_grid(total), dim3(kThreads), 0, s, reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y),
                       reinterpret_cast<_Float16*>(planes), total, H, W, OH, OW, C / 4, status_current());
    LAUNCH_CHECK();
}

// workgroups per image: one per 64 wave-loads of pixels, at most 256 - a function of the tap's own shape alone
int lpips_tap_blocks(int pix, int C) {
    const int pb = C == 64 ? 16 : C == 128 ? 8 : 4;
    return (int)std::max<long>(1, std::min<long>(((long)pix + 4L * pb - 1) / (4L * pb), 256));
}

void launch_lpips_tap(const float* fa, const float* fb, const float* w, int n, int pix, int C, double* partial, double* out, int out_stride, hipStream_t s) {
    BG_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, "lpips_tap: C=%d (the VGG16 taps have 64, 128, 256 or 512 channels)", C);
    BG_REQUIRE(fa && fb && w && partial && out && n >= 1 && pix >= 1 && out_stride >= 1 && (long)n * 256 <= 0x7FFFFFFFL, "lpips_tap: bad arguments (n=%d pixels=%d)", n, pix);
    const int G = lpips_tap_blocks(pix, C);
    switch (C) {
        case 64: tap_launch<64>(fa, fb, w, n, pix, G, partial, s); break;
        case 128: tap_launch<128>(fa, fb, w, n, pix, G, partial, s); break;
        case 256: tap_launch<256>(fa, fb, w, n, pix, G, partial, s); break;
        default: tap_launch<512>(fa, fb, w, n, pix, G, partial, s); break;
    }
    hipLaunchKernelGGL(lpips_tap_finish_kernel, dim3(n), dim3(64), 0, s, partial, G, pix, out, out_stride);
    LAUNCH_CHECK();
}

void launch_lpips_total(const double* layers, double* out, int n, hipStream_t s) {
    hipLaunchKernelGGL(lpips_total_kernel, dim3(cdiv(n, 64)), dim3(64), 0, s, layers, out, n);
    LAUNCH_CHECK();
}

void launch_conv_weight_relayout(const float* w_oihw, float* w_ohwi, int Cout, int Cin, int Cin_pad, hipStream_t s) {
    BG_REQUIRE(w_oihw && w_ohwi && Cout >= 1 && Cin >= 1 && Cin <= Cin_pad, "conv_weight_relayout: bad arguments");
    const long total = (long)Cout * 9 * Cin_pad;
    hipLaunchKernelGGL(conv_weight_relayout_kernel, stream_grid(total), dim3(kThreads), 0, s, w_oihw, w_ohwi, total, Cin, Cin_pad);
    LAUNCH_CHECK();
}

}  // namespace bevgen
