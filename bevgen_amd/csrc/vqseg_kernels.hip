// Kernels of the stage-1 BEV segmentation model (VQSegmentationModel, stage1/vqgan.py:216-261) beside its encoder / decoder:
//   BCELoss / BCELossWithQuant    losses/segmentation.py:7,17    F.binary_cross_entropy_with_logits(prediction, target), mean reduction (+ codebook_weight * qloss)
//   to_rgb                        stage1/vqgan.py:207-212        F.conv2d(x, colorize [3, C, 1, 1]) then (x - x.min()) / (x.max() - x.min()) over the WHOLE tensor,
//                                 stage1/vqgan.py:253-256        on the reconstruction preceded by torch.round(torch.sigmoid(.))
// fp32 arithmetic in every precision mode; no LDS beyond the reductions.
//
// Three numerical statements (the tests rest on them):
//   1. threshold is `x > 0`.  That is round(sigmoid(x)) with ties to even everywhere except 0 < x <~ 6e-8, where fp32 sigmoid rounds to exactly 0.5 and the reference
//      rounds that to 0 (on the CPU, torch.round(torch.sigmoid(1e-9)) = 0): round(sigmoid(.)) of a logit near 0 is a step, no bound in the logit's error carries across it.
//   2. the min-max normalisation is global: ONE extreme that moves rescales every pixel of every image of the call.  min and max do not depend on the order they are
//      taken in, so the result is bit-reproducible although it goes through atomics.
//   3. the reference decodes z + (z_q - z) (its straight-through estimator), the library decodes z_q: at most an ulp of z apart in front of the decoder.
#include "common.h"
#include "kernels.h"

namespace bevgen {

// ------------------------------------------------------------------------------------------------ binary cross entropy with logits, mean
// l(x, t) = max(x, 0) - x t + log1p(exp(-|x|)) per element in fp32 (no overflow at any x: the exponent's argument is <= 0; soft targets allowed; NaN propagates through
// x t).  The sum is taken in double in a FIXED order, so two calls give the same bits: with G = gridDim.x (a function of count alone), element i goes to thread i % 256 of
// block (i / 256) % G, which adds its elements in index order; a binary tree over the block's 256 sums gives partial[block]; then ONE block adds the G partials (thread t:
// t, t + 256, ... in index order, then the same tree), multiplies by 1 / count in double and rounds to float once.
__device__ __forceinline__ double block_tree_sum(double acc, double* sh) {
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(256) void bce_logits_fixed_order_kernel(const float* __restrict__ x, const float* __restrict__ t, long n, double* __restrict__ partial) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float xi = x[i];
        const float l = __fadd_rn(__fsub_rn(fmaxf(xi, 0.f), __fmul_rn(xi, t[i])), log1pf(expf(-fabsf(xi))));
        acc += (double)l;
    }
    const double s = block_tree_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[0] = bce; with qloss: out[1] = bce + codebook_weight * qloss as torch evaluates it in fp32 (the product rounded, then the sum)
__global__ __launch_bounds__(256) void bce_logits_finish_kernel(const double* __restrict__ partial, int G, double inv_count, const float* __restrict__ qloss, float codebook_weight,
                                                                float* __restrict__ out) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < G; i += 256) acc += partial[i];
    const double s = block_tree_sum(acc, sh);
    if (threadIdx.x == 0) {
        const float bce = (float)(s * inv_count);
        out[0] = bce;
        if (qloss) out[1] = __fadd_rn(bce, __fmul_rn(codebook_weight, qloss[0]));
    }
}

int bce_logits_blocks(long count) { return (int)std::max<long>(1, std::min<long>((count + 1023) / 1024, 1024)); }

void launch_bce_logits(const float* logits, const float* target, long count, const float* qloss, float codebook_weight, double* partial, float* out, hipStream_t s) {
    BG_REQUIRE(count >= 1, "bce_logits: count=%ld", count);
    const int G = bce_logits_blocks(count);
    hipLaunchKernelGGL(bce_logits_fixed_order_kernel, dim3(G), dim3(256), 0, s, logits, target, count, partial);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(bce_logits_finish_kernel, dim3(1), dim3(256), 0, s, partial, G, 1.0 / (double)count, qloss, codebook_weight, out);
    LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------ to_rgb
// fp32 bits as unsigned integers that order like the floats (-0 below +0); a NaN becomes the largest word for the max and the smallest for the min, both of which decode
// to a NaN again: one NaN makes every pixel NaN, as x.min() / x.max() do in the reference.
__device__ __forceinline__ unsigned ord_encode(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_decode(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }

// x [n, C, hw] -> y [n, 3, hw] = sum_c colorize[k][c] v_c in channel order (fmaf), v = x or its threshold; thread = pixel (loads and stores of a wave are contiguous in
// every channel plane), the 3 C weights are wave-uniform; minmax[0] = min, [1] = max of y in the ordered encoding (one atomic pair per wave).
__global__ __launch_bounds__(256) void seg_colorize_kernel(const float* __restrict__ x, const float* __restrict__ colorize, int threshold, float* __restrict__ y, long pixels,
                                                           int hw, int C, unsigned* __restrict__ minmax) {
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (long)gridDim.x * blockDim.x) {
        const long n = i / hw;
        const int p = (int)(i - n * hw);
        const float* xp = x + n * C * hw + p;
        float acc[3] = {0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            float v = xp[(long)c * hw];
            if (threshold) v = v > 0.f ? 1.f : (v <= 0.f ? 0.f : v);   // (a NaN stays a NaN)
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = fmaf(colorize[k * C + c], v, acc[k]);
        }
        float* yp = y + n * 3 * hw + p;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            yp[(long)k * hw] = acc[k];
            const bool nan = acc[k] != acc[k];
            const unsigned e = ord_encode(acc[k]);
            lo = min(lo, nan ? 0u : e);
            hi = max(hi, nan ? 0xFFFFFFFFu : e);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o, 64));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(minmax, lo);
        atomicMax(minmax + 1, hi);
    }
}

// in place y = (y - min) / (max - min): IEEE fp32 subtractions and a true division; max == min divides 0 by 0 as the reference does
__global__ __launch_bounds__(256) void seg_minmax_normalize_kernel(float* __restrict__ y, long total, const unsigned* __restrict__ minmax) {
    const float lo = ord_decode(minmax[0]), hi = ord_decode(minmax[1]);
    const float den = __fsub_rn(hi, lo);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) y[i] = __fdiv_rn(__fsub_rn(y[i], lo), den);
}

void launch_seg_colorize(const float* x, const float* colorize, int threshold, float* rgb, int n, int C, int H, int W, unsigned* minmax, hipStream_t s) {
    BG_REQUIRE(n >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= 32, "seg_colorize: C=%d (1 .. 32)", C);
    const long hw = (long)H * W, pixels = (long)n * hw;
    BG_REQUIRE(hw <= 0x7FFFFFFFL && pixels * 32 <= 0x7FFFFFFFFFFFL, "seg_colorize: %ld pixels", pixels);
    HIP_CHECK(hipMemsetAsync(minmax, 0xFF, sizeof(unsigned), s));
    HIP_CHECK(hipMemsetAsync(minmax + 1, 0x00, sizeof(unsigned), s));
    hipLaunchKernelGGL(seg_colorize_kernel, dim3((unsigned)std::min<long>((pixels + 255) / 256, 4096)), dim3(256), 0, s, x, colorize, threshold, rgb, pixels, (int)hw, C, minmax);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_minmax_normalize_kernel, dim3((unsigned)std::min<long>((3 * pixels + 255) / 256, 8192)), dim3(256), 0, s, rgb, 3 * pixels, minmax);
    LAUNCH_CHECK();
}

}  // namespace bevgen
