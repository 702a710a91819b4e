// Small VQGAN-decode helpers: codebook lookup (VectorQuantizer2.get_codebook_entry, stage1/quantize.py:314-329) and the final
// layout change NHWC -> NCHW fused with util.denormalize_tensor (bev_utils/util.py:97-118: x*std+mean per channel, clamp [0,1]).
#include "common.h"
#include "kernels.h"

namespace bevgen {

__global__ __launch_bounds__(256) void codebook_gather_kernel(const int64_t* __restrict__ ids, const float* __restrict__ codebook, float* __restrict__ out,
                                                              long rows, int dim4, int n_embed) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < rows * dim4; i += (long)gridDim.x * blockDim.x) {
        const long r = i / dim4;
        const int c = (int)(i - r * dim4);
        long id = ids[r];
        id = id < 0 ? 0 : (id >= n_embed ? n_embed - 1 : id);
        reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(codebook)[id * dim4 + c];
    }
}

void launch_codebook_gather(const int64_t* ids, const float* codebook, float* out, int rows, int dim, int n_embed, hipStream_t s) {
    BG_REQUIRE(dim % 4 == 0, "codebook_gather: embed dim must be a multiple of 4");
    const long total = (long)rows * (dim / 4);
    hipLaunchKernelGGL(codebook_gather_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, s, ids, codebook, out, (long)rows, dim / 4, n_embed);
    LAUNCH_CHECK();
}

// x [n, hw, ldc] (first C channels used) -> y [n, C, hw]
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int hw, int C, int ldc,
                                                           const float* __restrict__ mean, const float* __restrict__ stdv, int clamp01, uint8_t* __restrict__ y8,
                                                           unsigned* __restrict__ status) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int p = (int)(i % hw);
        const long nc = i / hw;
        const int c = (int)(nc % C);
        const long n = nc / C;
        float v = x[(n * hw + p) * ldc + c];
        if (nonfinite(v)) status_raise(status, BG_ST_NONFINITE_PIXELS);   // (the clamp below would turn a NaN into a valid-looking pixel)
        if (mean) v = v * stdv[c] + mean[c];
        if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
        if (y8) y8[i] = (uint8_t)fminf(fmaxf(rintf(v * 255.0f), 0.f), 255.f);   // round(x*255) (half to even, like torch.round), the storage format of the images
        else y[i] = v;
    }
}

void launch_nhwc_to_nchw(const float* x, float* y, int n, int hw, int C, int ldc, const float* mean, const float* stdv, int clamp01, hipStream_t s, uint8_t* y8) {
    const long total = (long)n * C * hw;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((int)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, s, x, y, total, hw, C, ldc, mean, stdv, clamp01, y8, status_current());
    LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------ decoder tail in one kernel
// Decoder.forward's last three operators (stage1/model.py:532-536: norm_out -> nonlinearity -> conv_out) + denormalize_tensor (bev_utils/util.py:97-118) + the NHWC -> NCHW
// (/ uint8) write: GroupNorm-apply + swish on the way INTO LDS, a direct 3x3 convolution 128 -> 3 on the vector ALUs, per-channel x std + mean, clamp, store.
// As an implicit GEMM the 3-channel convolution filled 3 of the 128 columns of an MFMA tile (1.8-3.7 ms per 48-image pass, + 1.2 ms for the GroupNorm-apply pass that wrote
// the 1.6 GB plane image it read); each output pixel is 1152 MACs x 3 channels over data that is read once: bandwidth work.
// One workgroup = 16 x 16 output pixels of one image; the 18 x 18 halo tile goes through LDS in chunks of 32 channels (pixel stride 36 floats: ds_read_b128 of 16 consecutive
// pixels is bank-conflict free), zero outside the image (the convolution pads the ACTIVATED tensor); thread = pixel, 3 accumulators; weights are wave-uniform (scalar loads).
constexpr int OC_T = 16, OC_HALO = OC_T + 2, OC_CC = 32, OC_PS = 36;
template <int COUT>
__global__ __launch_bounds__(256) void vq_out_conv_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ wgt, const float* __restrict__ bias, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                          int clamp01, float* __restrict__ y, uint8_t* __restrict__ y8, int H, int W, int C, unsigned* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) float tile[OC_HALO * OC_HALO * OC_PS];
    const int tid = threadIdx.x, px = tid & 15, py = tid >> 4;
    const int x0 = blockIdx.x * OC_T, y0 = blockIdx.y * OC_T, n = blockIdx.z;
    const int cpg = C / 32;   // GroupNorm(32 groups)
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = 0.f;
    for (int c0 = 0; c0 < C; c0 += OC_CC) {
        // ---- halo tile of this channel chunk, normalised + activated: one float4 (4 channels of one pixel) per thread and pass
        for (int i = tid; i < OC_HALO * OC_HALO * (OC_CC / 4); i += 256) {
            const int q = i & (OC_CC / 4 - 1), p = i / (OC_CC / 4);
            const int hy = p / OC_HALO, hx = p - hy * OC_HALO;
            const int gy = y0 + hy - 1, gx = x0 + hx - 1;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const int c = c0 + 4 * q;
                const float4 v = *reinterpret_cast<const float4*>(x + (((long)n * H + gy) * W + gx) * C + c);
                const float in[4] = {v.x, v.y, v.z, v.w};
                float r[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float* st = stats + ((long)n * 32 + (c + k) / cpg) * 2;
                    const float t = (in[k] - st[0]) * st[1] * gamma[c + k] + beta[c + k];
                    r[k] = t / (1.f + expf(-t));
                }
                o = make_float4(r[0], r[1], r[2], r[3]);
            }
            *reinterpret_cast<float4*>(&tile[p * OC_PS + 4 * q]) = o;
        }
        __syncthreads();
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float* tp = &tile[((py + dy) * OC_HALO + px + dx) * OC_PS];
                const float* wp = wgt + (long)(dy * 3 + dx) * C + c0;   // [Cout][kh][kw][Cin]
#pragma unroll
                for (int c = 0; c < OC_CC; c += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(tp + c);
#pragma unroll
                    for (int co = 0; co < COUT; ++co) {
                        const float* w = wp + (long)co * 9 * C + c;
                        acc[co] = fmaf(v.x, w[0], acc[co]);
                        acc[co] = fmaf(v.y, w[1], acc[co]);
                        acc[co] = fmaf(v.z, w[2], acc[co]);
                        acc[co] = fmaf(v.w, w[3], acc[co]);
                    }
                }
            }
        __syncthreads();
    }
    const int oy = y0 + py, ox = x0 + px;
    if (oy < H && ox < W) {
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            float v = acc[co] + (bias ? bias[co] : 0.f);
            if (nonfinite(v)) status_raise(status, BG_ST_NONFINITE_PIXELS);   // (the clamp below would turn a NaN into a valid-looking pixel)
            if (mean) v = v * stdv[co] + mean[co];
            if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
            const long o = (((long)n * COUT + co) * H + oy) * W + ox;
            if (y8) y8[o] = (uint8_t)fminf(fmaxf(rintf(v * 255.0f), 0.f), 255.f);   // round(x*255), half to even like torch.round
            else y[o] = v;
        }
    }
}

// COUT is a template argument (the accumulators live in registers, the weight addresses are wave-uniform): 3 = the camera decoder, 7 = the BEV segmentation decoder
// (stage_1_bev.yaml: out_ch 7).  Compiler's resource report: <3> 57 VGPRs, <7> 81 VGPRs, both 3 waves / SIMD (the 46.6 KB tile is the limit), no scratch and no
// VGPR spill; <7> parks 73 SGPRs (its 7 x 9 wave-uniform weight rows) in VGPR lanes, <3> 3.  Any other count takes the three-kernel tail.
bool vq_out_conv_supported(int C, int cout) { return (cout == 3 || cout == 7) && C % 32 == 0 && C >= 32; }

void launch_vq_out_conv(const float* x, const float* stats, const float* gamma, const float* beta, const float* wgt, const float* bias, const float* mean, const float* stdv, int clamp01,
                        float* y, uint8_t* y8, int n, int H, int W, int C, int cout, hipStream_t s) {
    BG_REQUIRE(vq_out_conv_supported(C, cout), "vq_out_conv: C=%d cout=%d", C, cout);
    if (cout == 3)
        hipLaunchKernelGGL((vq_out_conv_kernel<3>), dim3(cdiv(W, OC_T), cdiv(H, OC_T), n), dim3(256), 0, s, x, stats, gamma, beta, wgt, bias, mean, stdv, clamp01, y, y8, H, W, C, status_current());
    else
        hipLaunchKernelGGL((vq_out_conv_kernel<7>), dim3(cdiv(W, OC_T), cdiv(H, OC_T), n), dim3(256), 0, s, x, stats, gamma, beta, wgt, bias, mean, stdv, clamp01, y, y8, H, W, C, status_current());
    LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------ range-safe split precision (precision = 'f16x3r')
// The decoder's UN-normalised residual stream becomes an f16 operand in front of a few convolutions (upsample, nin_shortcut, conv_in).  A convolution is linear in its
// input, so W x + b = 2^e (W (x 2^-e)) + b for any e; with e a per-tensor power of two both scalings are exact in every bit the (hi, lo) split keeps:
//   range_absmax_kernel    max |x| of the tensor (one atomic max per wave on a zeroed word); NaN / inf raise BG_ST_F16_RANGE as the plane writers do and stay out of the max
//   range_exponent_kernel  e = 0 where max |x| < 32768, else the smallest e with max |x| 2^-e < 32768 - ONE int in device memory, never read by the host on the decode path
//   range_split_kernel     x 2^-e as (hi, lo) planes (the LDS-DMA convolution's operand) / range_scale_kernel: x 2^-e as fp32 (the register-staged kernel splits it itself)
//   range_unscale_kernel   y = 2^e y + b[c] (+ residual) over the convolution's bias-free output; fmaf(1, y, b) rounds like the epilogue's y + b: e = 0 reproduces precision =
//                          'f16x3' bit for bit.  Its second form also leaves the GroupNorm partial sums the skipped epilogue would have left (GemmArgs::gn_part), same layout,
//                          same order of additions.
__global__ __launch_bounds__(256) void range_absmax_kernel(const float4* __restrict__ x, long n4, unsigned* __restrict__ amax, unsigned* __restrict__ status) {
    float m = 0.f;
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 v = x[i];
        const float in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (nonfinite(in[k])) bad = 1;
            else m = fmaxf(m, fabsf(in[k]));
        }
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(amax, __float_as_uint(m));   // (bit patterns of non-negative finite floats order like the floats)
    if (bad) status_raise(status, BG_ST_F16_RANGE);
}

__global__ void range_exponent_kernel(const unsigned* __restrict__ amax, int* __restrict__ e_out) {
    const int k = (int)(*amax >> 23) - 127;   // max |x| in [2^k, 2^(k+1)) (finite by construction: k <= 127)
    *e_out = min(max(k - 14, 0), 113);        // 2^(k+1-e) <= 2^15; 2^-113 and 2^113 are normal floats
}

__device__ __forceinline__ float range_pow2(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }

__global__ __launch_bounds__(256) void range_split_kernel(const float4* __restrict__ x, _Float16* __restrict__ planes, long n4, int q4, const int* __restrict__ e,
                                                          unsigned* __restrict__ status) {
    const float sc = range_pow2(-*e);
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const long pix = i / q4;
        const int cq = (int)(i - pix * q4);
        const float4 v = x[i];
        // (x sc + 0 like launch_to_planes' x 1 + 0: the same bits at e = 0, the sign of a zero included)
        store_planes4(planes + pix * 8 * q4, cq * 4, make_float4(fmaf(v.x, sc, 0.f), fmaf(v.y, sc, 0.f), fmaf(v.z, sc, 0.f), fmaf(v.w, sc, 0.f)), bad);
    }
    if (bad) status_raise(status, BG_ST_F16_RANGE);
}

__global__ __launch_bounds__(256) void range_scale_kernel(const float4* __restrict__ x, float4* __restrict__ y, long n4, const int* __restrict__ e) {
    const float sc = range_pow2(-*e);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 v = x[i];
        y[i] = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
    }
}

__device__ __forceinline__ float4 range_unscale4(float4 v, float up, float4 b, const float4* __restrict__ R, long i) {
    float4 o = make_float4(fmaf(up, v.x, b.x), fmaf(up, v.y, b.y), fmaf(up, v.z, b.z), fmaf(up, v.w, b.w));
    if (R) { const float4 r = R[i]; o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w; }
    return o;
}

__global__ __launch_bounds__(256) void range_unscale_kernel(float4* __restrict__ y, const float* __restrict__ bias, const float4* __restrict__ R, long n4, int q4,
                                                            const int* __restrict__ e) {
    const float up = range_pow2(*e);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int cq = (int)(i % q4);
        const float4 b = bias ? reinterpret_cast<const float4*>(bias)[cq] : make_float4(0.f, 0.f, 0.f, 0.f);
        y[i] = range_unscale4(y[i], up, b, R, i);
    }
}

// One workgroup = 32 rows (pixels); lane = (row, one of two neighbouring channel quads), exactly the epilogue's assignment (gemm_split_glds.hip: r = lane & 31, h = lane >> 5),
// the four waves share the 128-byte lines of an iteration.  rows % 32 == 0 and C % 32 == 0 (launcher): every lane is active in the DPP sums.
__global__ __launch_bounds__(256) void range_unscale_gn_kernel(float* __restrict__ y, const float* __restrict__ bias, int C, const int* __restrict__ e, float* __restrict__ gn_part) {
    const float up = range_pow2(*e);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const long m = (long)blockIdx.x * 32 + r;
    for (int o = wave; o < (C >> 3); o += 4) {
        const int n = 8 * o + 4 * h;
        float4* p = reinterpret_cast<float4*>(y + m * C + n);
        const float4 t = range_unscale4(*p, up, *reinterpret_cast<const float4*>(bias + n), nullptr, 0);
        *p = t;
        const float v[4] = {t.x, t.y, t.z, t.w};
        float s4 = (v[0] + v[1]) + (v[2] + v[3]);
        float q4 = fmaf(v[0], v[0], v[1] * v[1]) + fmaf(v[2], v[2], v[3] * v[3]);
        s4 = row16_sum(s4); q4 = row16_sum(q4);
        s4 += xor16(s4); q4 += xor16(q4);
        if (r == 0) *reinterpret_cast<float2*>(gn_part + ((m >> 5) * (C >> 2) + (n >> 2)) * 2) = make_float2(s4, q4);
    }
}

// The encoder's fused forms (vq_encode, range-safe mode): a pass that writes a tensor which the NEXT site reads as its operand also leaves that tensor's absmax, so the
// next site's range_absmax_kernel pass disappears.  Both write exactly the bits of their unfused kernels and treat NaN / inf as range_absmax_kernel does.
__device__ __forceinline__ void range_amax_finish(float m, unsigned bad, unsigned* __restrict__ amax, unsigned* __restrict__ status) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(amax, __float_as_uint(m));
    if (bad) status_raise(status, BG_ST_F16_RANGE);
}

__device__ __forceinline__ void range_amax4(float4 t, float& m, unsigned& bad) {
    const float v[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (nonfinite(v[k])) bad = 1;
        else m = fmaxf(m, fabsf(v[k]));
    }
}

// range_unscale_kernel (no residual) + the absmax of what it writes
__global__ __launch_bounds__(256) void range_unscale_amax_kernel(float4* __restrict__ y, const float* __restrict__ bias, long n4, int q4, const int* __restrict__ e,
                                                                 unsigned* __restrict__ amax, unsigned* __restrict__ status) {
    const float up = range_pow2(*e);
    float m = 0.f;
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int cq = (int)(i % q4);
        const float4 b = bias ? reinterpret_cast<const float4*>(bias)[cq] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 t = range_unscale4(y[i], up, b, nullptr, 0);
        y[i] = t;
        range_amax4(t, m, bad);
    }
    range_amax_finish(m, bad, amax, status);
}

// x [n, C, hw] -> y [n, hw, Cpad] (channels >= C are zero: launch_nchw_to_nhwc_pad's output) + the absmax of x; one thread per channel quad of a pixel
__global__ __launch_bounds__(256) void nchw_to_nhwc_pad_amax_kernel(const float* __restrict__ x, float4* __restrict__ y, long n4, int hw, int C, int q4,
                                                                    unsigned* __restrict__ amax, unsigned* __restrict__ status) {
    float m = 0.f;
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % q4) * 4;
        const long np = i / q4;
        const int p = (int)(np % hw);
        const long n = np / hw;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = c0 + k < C ? x[(n * C + c0 + k) * hw + p] : 0.f;
        const float4 t = make_float4(v[0], v[1], v[2], v[3]);
        y[i] = t;
        range_amax4(t, m, bad);
    }
    range_amax_finish(m, bad, amax, status);
}

static dim3 range_grid(long n4) { return dim3((unsigned)std::max<long>(1, std::min<long>((n4 + 255) / 256, 8192))); }

void launch_range_unscale_amax(float* y, const float* bias, long rows, int C, const int* e, unsigned* amax_next, int* e_next, hipStream_t s) {
    BG_REQUIRE(C % 4 == 0 && rows > 0, "range_unscale: C=%d must be a multiple of 4", C);
    const long n4 = rows * (C / 4);
    hipLaunchKernelGGL(range_unscale_amax_kernel, range_grid(n4), dim3(256), 0, s, reinterpret_cast<float4*>(y), bias, n4, C / 4, e, amax_next, status_current());
    LAUNCH_CHECK();
    hipLaunchKernelGGL(range_exponent_kernel, dim3(1), dim3(1), 0, s, amax_next, e_next);
    LAUNCH_CHECK();
}

void launch_nchw_to_nhwc_pad_amax(const float* x, float* y, int n, int hw, int C, int Cpad, unsigned* amax, int* e, hipStream_t s) {
    BG_REQUIRE(Cpad % 4 == 0 && C >= 1 && C <= Cpad && n >= 1 && hw >= 1, "nchw_to_nhwc_pad: C=%d Cpad=%d (Cpad must be a multiple of 4)", C, Cpad);
    const long n4 = (long)n * hw * (Cpad / 4);
    hipLaunchKernelGGL(nchw_to_nhwc_pad_amax_kernel, range_grid(n4), dim3(256), 0, s, x, reinterpret_cast<float4*>(y), n4, hw, C, Cpad / 4, amax, status_current());
    LAUNCH_CHECK();
    hipLaunchKernelGGL(range_exponent_kernel, dim3(1), dim3(1), 0, s, amax, e);
    LAUNCH_CHECK();
}

void launch_range_exponent(const float* x, long elems, unsigned* amax, int* e, hipStream_t s) {
    BG_REQUIRE(elems > 0 && elems % 4 == 0, "range_exponent: element count %ld must be a positive multiple of 4", elems);
    hipLaunchKernelGGL(range_absmax_kernel, range_grid(elems / 4), dim3(256), 0, s, reinterpret_cast<const float4*>(x), elems / 4, amax, status_current());
    LAUNCH_CHECK();
    hipLaunchKernelGGL(range_exponent_kernel, dim3(1), dim3(1), 0, s, amax, e);
    LAUNCH_CHECK();
}

void launch_range_split(const float* x, void* planes, long pixels, int C, const int* e, hipStream_t s) {
    BG_REQUIRE(C % 32 == 0 && pixels > 0, "range_split: C=%d must be a multiple of 32", C);
    const long n4 = pixels * (C / 4);
    hipLaunchKernelGGL(range_split_kernel, range_grid(n4), dim3(256), 0, s, reinterpret_cast<const float4*>(x), reinterpret_cast<_Float16*>(planes), n4, C / 4, e, status_current());
    LAUNCH_CHECK();
}

void launch_range_scale(const float* x, float* y, long elems, const int* e, hipStream_t s) {
    BG_REQUIRE(elems > 0 && elems % 4 == 0, "range_scale: element count %ld must be a positive multiple of 4", elems);
    hipLaunchKernelGGL(range_scale_kernel, range_grid(elems / 4), dim3(256), 0, s, reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), elems / 4, e);
    LAUNCH_CHECK();
}

void launch_range_unscale(float* y, const float* bias, const float* residual, long rows, int C, const int* e, float* gn_part, hipStream_t s) {
    BG_REQUIRE(C % 4 == 0 && rows > 0, "range_unscale: C=%d must be a multiple of 4", C);
    if (gn_part) {
        BG_REQUIRE(rows % 32 == 0 && C % 32 == 0 && bias && !residual && rows / 32 <= 0x7FFFFFFFL, "range_unscale: GroupNorm partials need rows %% 32 == 0, C %% 32 == 0 and a bias (rows=%ld C=%d)", rows, C);
        hipLaunchKernelGGL(range_unscale_gn_kernel, dim3((unsigned)(rows / 32)), dim3(256), 0, s, y, bias, C, e, gn_part);
    } else {
        const long n4 = rows * (C / 4);
        hipLaunchKernelGGL(range_unscale_kernel, range_grid(n4), dim3(256), 0, s, reinterpret_cast<float4*>(y), bias, reinterpret_cast<const float4*>(residual), n4, C / 4, e);
    }
    LAUNCH_CHECK();
}

// x [n, C, hw] -> y [n, hw, C]
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int hw, int C) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long np = i / C;
        const int p = (int)(np % hw);
        const long n = np / hw;
        y[i] = x[(n * C + c) * hw + p];
    }
}

void launch_nchw_to_nhwc(const float* x, float* y, int n, int hw, int C, hipStream_t s) {
    const long total = (long)n * C * hw;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((int)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, s, x, y, total, hw, C);
    LAUNCH_CHECK();
}

}  // namespace bevgen
