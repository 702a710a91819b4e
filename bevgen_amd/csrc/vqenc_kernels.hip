// Kernels of the VQGAN *encode* side (the step before the sampling path: BEV segmentation -> condition token ids, images -> z ids):
//   VectorQuantizer2.forward   stage1/quantize.py:271-312   argmin_j ( |z|^2 + |e_j|^2 - 2 z.e_j )
//   input layout change NCHW -> NHWC with the channel axis zero-padded to a multiple of 32 (implicit-GEMM convolutions need Cin % 32 == 0)
#include "common.h"
#include "kernels.h"

namespace bevgen {

// x [n, C, hw] -> y [n, hw, Cpad] (channels >= C are zero)
__global__ __launch_bounds__(256) void nchw_to_nhwc_pad_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int hw, int C, int Cpad) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const long np = i / Cpad;
        const int p = (int)(np % hw);
        const long n = np / hw;
        y[i] = c < C ? x[(n * C + c) * hw + p] : 0.f;
    }
}
void launch_nchw_to_nhwc_pad(const float* x, float* y, int n, int hw, int C, int Cpad, hipStream_t s) {
    const long total = (long)n * hw * Cpad;
    hipLaunchKernelGGL(nchw_to_nhwc_pad_kernel, dim3((int)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, s, x, y, total, hw, C, Cpad);
    LAUNCH_CHECK();
}

// conv weight [Cout][Cin][kh][kw] -> [Cout][kh][kw][CinPad] (zero padded)
__global__ void relayout_conv_weight_pad_kernel(const float* __restrict__ w, float* __restrict__ o, int cout, int cin, int cin_pad, int kh, int kw) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)cout * cin_pad * kh * kw;
    if (i >= total) return;
    const int ci = (int)(i % cin_pad);
    long t = i / cin_pad;
    const int x = (int)(t % kw); t /= kw;
    const int y = (int)(t % kh);
    const int co = (int)(t / kh);
    o[i] = ci < cin ? w[(((long)co * cin + ci) * kh + y) * kw + x] : 0.f;
}
void launch_relayout_conv_weight_pad(const float* w, float* o, int cout, int cin, int cin_pad, int kh, int kw, hipStream_t s) {
    hipLaunchKernelGGL(relayout_conv_weight_pad_kernel, dim3(cdiv((long)cout * cin_pad * kh * kw, 256)), dim3(256), 0, s, w, o, cout, cin, cin_pad, kh, kw);
    LAUNCH_CHECK();
}

// out[row] = sum_k x[row,k]^2   (one wave per row)
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ x, float* __restrict__ out, long rows, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float s = 0.f;
    for (int i = lane; i < D; i += 64) { const float v = x[row * D + i]; s = fmaf(v, v, s); }
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}
void launch_row_sqnorm(const float* x, float* out, long rows, int D, hipStream_t s) {
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((int)((rows + 3) / 4)), dim3(256), 0, s, x, out, rows, D);
    LAUNCH_CHECK();
}

// ids[row] = argmin_j (zz[row] + ee[j]) - 2 * dots[row, j]; ties -> lowest index (torch.argmin).  A NaN distance never wins.  A row without any finite distance (NaN / inf
// in the image, an overflow in the encoder: `d < best` is false for NaN and for inf < inf) has no minimum: BG_ST_NONFINITE_LATENTS is raised and the in-range id 0 written.
__global__ __launch_bounds__(256) void vq_argmin_kernel(const float* __restrict__ dots, const float* __restrict__ zz, const float* __restrict__ ee, int64_t* __restrict__ ids,
                                                        long rows, int n_e, unsigned* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float z2 = zz[row];
    float best = INFINITY;
    int bidx = 0x7fffffff;
    for (int j = lane; j < n_e; j += 64) {
        const float d = (z2 + ee[j]) - 2.f * dots[row * n_e + j];
        if (d < best) { best = d; bidx = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (ob < best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if (lane == 0) {
        const bool none = bidx == 0x7fffffff;
        if (none) status_raise(status, BG_ST_NONFINITE_LATENTS);
        ids[row] = none ? 0 : bidx;
    }
}
void launch_vq_argmin(const float* dots, const float* zz, const float* ee, int64_t* ids, long rows, int n_e, hipStream_t s) {
    hipLaunchKernelGGL(vq_argmin_kernel, dim3((int)((rows + 3) / 4)), dim3(256), 0, s, dots, zz, ee, ids, rows, n_e, status_current());
    LAUNCH_CHECK();
}

// VQModel.encode's geometric embedding (stage1/vqgan.py:87-112), added in place to the encoder output h [n, T, D] (NHWC): for image i and latent pixel t
//   c4 = E_inv[i][:, 3];  d = E_inv[i] [I_inv[i] plane[:, t]; 1];  e[o] = Wimg[o,:].d - Wcam[o,:].c4;  h[i,t,:] += e / (|e| + 1e-7)
// The arithmetic of camera_embed_kernel (embed.hip), four-term products as ((a+b)+c)+d.  One wave per latent pixel, four pixels per block: no LDS, no barrier; lane l
// keeps channels l, l + 64, ... (NV of them, those >= D idle: D = 32 leaves half a wave without work) in registers between the sum of squares and the add, so h is read
// and written once.  The wave index goes through readfirstlane, which makes pixel, image and with them the loads of the matrices and the plane scalar.
template <int NV>
__global__ __launch_bounds__(256) void vq_geo_embed_kernel(float* __restrict__ h, const float* __restrict__ I_inv, const float* __restrict__ E_inv,
                                                           const float* __restrict__ plane, const float* __restrict__ Wimg, const float* __restrict__ Wcam, long pixels,
                                                           int T, int D) {
    const int lane = threadIdx.x & 63;
    const long pix = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pix >= pixels) return;   // the tail block
    const long i = (unsigned)pix / (unsigned)T;   // (pixels fits an int: the launcher checks it)
    const int t = (int)(pix - i * T);
    const float* Ii = I_inv + i * 9;
    const float* Ei = E_inv + i * 16;
    const float c4[4] = {Ei[3], Ei[7], Ei[11], Ei[15]};
    const float px = plane[t], py = plane[T + t], pz = plane[2 * T + t];
    float camv[4];
#pragma unroll
    for (int r = 0; r < 3; ++r) camv[r] = (Ii[3 * r] * px + Ii[3 * r + 1] * py) + Ii[3 * r + 2] * pz;
    camv[3] = 1.f;
    float d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = ((Ei[4 * r] * camv[0] + Ei[4 * r + 1] * camv[1]) + Ei[4 * r + 2] * camv[2]) + Ei[4 * r + 3] * camv[3];
    float e[NV];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int o = lane + 64 * k;
        e[k] = 0.f;
        if (o < D) {
            const float* wi = Wimg + o * 4;
            const float* wc = Wcam + o * 4;
            const float de = ((wi[0] * d[0] + wi[1] * d[1]) + wi[2] * d[2]) + wi[3] * d[3];
            const float ce = ((wc[0] * c4[0] + wc[1] * c4[1]) + wc[2] * c4[2]) + wc[3] * c4[3];
            e[k] = de - ce;
            ss = fmaf(e[k], e[k], ss);
        }
    }
    const float nrm = sqrtf(wave_sum(ss)) + 1e-7f;
    float* row = h + pix * D;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int o = lane + 64 * k;
        if (o < D) row[o] += e[k] / nrm;
    }
}
void launch_vq_geo_embed(float* h, const float* I_inv, const float* E_inv, const float* plane, const float* Wimg, const float* Wcam, int n, int T, int D, hipStream_t s) {
    BG_REQUIRE(n >= 1 && T >= 1 && D >= 32 && D % 32 == 0 && D <= 1024, "vq_geo_embed: D=%d must be a multiple of 32 (at most 1024)", D);
    const long pixels = (long)n * T;
    BG_REQUIRE(pixels <= 0x7FFFFFFFL, "vq_geo_embed: %ld latent pixels", pixels);
    const dim3 grid((int)((pixels + 3) / 4)), block(256);
    const int nv = (D + 63) / 64;
    if (nv <= 1) hipLaunchKernelGGL(vq_geo_embed_kernel<1>, grid, block, 0, s, h, I_inv, E_inv, plane, Wimg, Wcam, pixels, T, D);
    else if (nv <= 2) hipLaunchKernelGGL(vq_geo_embed_kernel<2>, grid, block, 0, s, h, I_inv, E_inv, plane, Wimg, Wcam, pixels, T, D);
    else if (nv <= 4) hipLaunchKernelGGL(vq_geo_embed_kernel<4>, grid, block, 0, s, h, I_inv, E_inv, plane, Wimg, Wcam, pixels, T, D);
    else if (nv <= 8) hipLaunchKernelGGL(vq_geo_embed_kernel<8>, grid, block, 0, s, h, I_inv, E_inv, plane, Wimg, Wcam, pixels, T, D);
    else hipLaunchKernelGGL(vq_geo_embed_kernel<16>, grid, block, 0, s, h, I_inv, E_inv, plane, Wimg, Wcam, pixels, T, D);
    LAUNCH_CHECK();
}

// row_err[r] = sum_c (codebook[ids[r]][c] - z[r][c])^2 as direct fp32 differences (|z|^2 - 2 z.e + |e|^2 cancels); one wave per row.  NaN / inf in z propagate into the
// row's error (the arg-min has already raised BG_ST_NONFINITE_LATENTS for such a row); the id is clamped into the codebook.
__global__ __launch_bounds__(256) void vq_row_err_kernel(const float* __restrict__ z, const float* __restrict__ codebook, const int64_t* __restrict__ ids,
                                                         float* __restrict__ row_err, long rows, int n_e, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    long id = ids[row];
    id = id < 0 ? 0 : (id >= n_e ? n_e - 1 : id);
    float s = 0.f;
    for (int i = lane; i < D; i += 64) { const float v = codebook[id * D + i] - z[row * D + i]; s = fmaf(v, v, s); }
    s = wave_sum(s);
    if (lane == 0) row_err[row] = s;
}
void launch_vq_row_err(const float* z, const float* codebook, const int64_t* ids, float* row_err, long rows, int n_e, int D, hipStream_t s) {
    hipLaunchKernelGGL(vq_row_err_kernel, dim3((int)((rows + 3) / 4)), dim3(256), 0, s, z, codebook, ids, row_err, rows, n_e, D);
    LAUNCH_CHECK();
}

// out[0] = scale * sum(x) in a FIXED order, the pattern of mean_fixed_order_kernel (sampler.hip): thread t adds elements t, t + 256, ... in double, then a binary tree over
// the 256 partial sums; two calls give the same bits.  The codebook loss: scale = (1 + beta) / (rows D), which is the forward value of both the legacy and the corrected
// formula (stage1/quantize.py:290-295).  One workgroup.
__global__ __launch_bounds__(256) void vq_loss_fixed_order_kernel(const float* __restrict__ x, long n, double scale, float* __restrict__ out) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) acc += (double)x[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(sh[0] * scale);
}
void launch_vq_loss(const float* row_err, long rows, int D, float beta, float* loss, hipStream_t s) {
    const double scale = (1.0 + (double)beta) / ((double)rows * (double)D);
    hipLaunchKernelGGL(vq_loss_fixed_order_kernel, dim3(1), dim3(256), 0, s, row_err, rows, scale, loss);
    LAUNCH_CHECK();
}

}  // namespace bevgen
