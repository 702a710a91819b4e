// Image-level evaluation metrics on planes that are already on the device (the step scripts/metrics_eval.py:115-132 of the reference takes after `generate`):
//   image_sqerr   per image sum((a - b)^2) and the running min / max of the target b: the states of PeakSignalNoiseRatio(data_range=None)
//   ssim          per image sum of the SSIM map over the VALID Gaussian windows: the state of StructuralSimilarityIndexMeasure(data_range=R)
// Images are [n, C, H, W], contiguous, fp32 (nominally in [0, 1]) or uint8 (v / 255, one IEEE division).  fp32 / fp64 arithmetic in every precision mode.
//
// Reductions run in a FIXED order and use no floating atomics: a workgroup's threads add their elements in index order in double, a binary tree over the 256 thread sums
// gives one partial per workgroup, and a second kernel adds each image's partials (thread t: t, t + 256, ... in index order, then the same tree).  The number of partials
// of an image is a function of its own shape alone, so image i's result does not depend on what else is in the batch, and two calls give the same bits.
//
// Cancellation (the folded LayerNorm statistics): E_w[x^2] - mu^2 in fp32 loses everything below 2^-24 mu^2, and SSIM adds c2 = 9e-4 to exactly that difference.
// On a bright, almost flat pair the plain formula is off by 1e-3 per pixel.  The second moments here are therefore taken about a per-tile shift s (the target's pixel in
// the middle of the tile's halo): both images are stored in LDS as x - s, the products are formed from those, and s is added back to the two means only.  Variances and
// the covariance do not depend on s; |x - s| is the local contrast, not the level.
#include <cmath>

#include "../../include/bevgen_hip.h"
#include "common.h"
#include "kernels.h"

namespace bevgen {

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 32;          // output columns of an SSIM tile
constexpr int kMaxKernel = 33;      // largest Gaussian window (halo tile 64 wide)

__device__ __forceinline__ float load01(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float load01(const uint8_t* p, long i) { return __fdiv_rn((float)p[i], 255.f); }

// min / max that keep a NaN once they have seen one (torch.min / torch.max)
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a) ? a : ((b != b || b < a) ? b : a); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }

__device__ __forceinline__ double tree_sum_256(double acc, double* sh) {
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------------------------------------ squared error
// n G workgroups: workgroup g of image i (blockIdx.x = i G + g) adds elements g 256 + t, (g + G) 256 + t, ... of that image.  fp32: d = a - b and d d are one fp32 operation each, the sum is double.
// uint8: (a - b)^2 as integers in a 64-bit counter, exact; the counters (< 2^53) then go through the double tree without a rounding.
__device__ __forceinline__ void sq_accumulate(const float* a, const float* b, long i, double& acc, unsigned long long&, float& lo, float& hi) {
    const float y = b[i];
    const float d = __fsub_rn(a[i], y);
    acc += (double)__fmul_rn(d, d);
    lo = nan_min(lo, y);
    hi = nan_max(hi, y);
}
__device__ __forceinline__ void sq_accumulate(const uint8_t* a, const uint8_t* b, long i, double&, unsigned long long& iacc, float& lo, float& hi) {
    const int y = b[i];
    const int d = (int)a[i] - y;
    iacc += (unsigned long long)(d * d);
    const float yf = __fdiv_rn((float)y, 255.f);
    lo = fminf(lo, yf);
    hi = fmaxf(hi, yf);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void image_sqerr_kernel(const T* __restrict__ a, const T* __restrict__ b, long count, int G, double* __restrict__ partial,
                                                               float* __restrict__ part_minmax) {
    __shared__ double sh[kThreads];
    __shared__ float shlo[kThreads], shhi[kThreads];
    const long image = blockIdx.x / G;
    const int blk = (int)(blockIdx.x - image * G);
    const long base = image * count;
    double acc = 0.0;
    unsigned long long iacc = 0ull;
    float lo = INFINITY, hi = -INFINITY;
    for (long i = (long)blk * kThreads + threadIdx.x; i < count; i += (long)G * kThreads) sq_accumulate(a + base, b + base, i, acc, iacc, lo, hi);
    const double s = tree_sum_256(acc + (double)iacc, sh);
    shlo[threadIdx.x] = lo;
    shhi[threadIdx.x] = hi;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            shlo[threadIdx.x] = nan_min(shlo[threadIdx.x], shlo[threadIdx.x + o]);
            shhi[threadIdx.x] = nan_max(shhi[threadIdx.x], shhi[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long p = blockIdx.x;
        partial[p] = s;
        part_minmax[2 * p] = shlo[0];
        part_minmax[2 * p + 1] = shhi[0];
    }
}

// out[i] = sum of image i's `per_image` partials (one workgroup per image).  part_minmax non-null: workgroup 0 also merges all gridDim.x * per_image (min, max) pairs
// INTO minmax[0 .. 1] (min and max do not depend on the order they are taken in).
__global__ __launch_bounds__(kThreads) void metrics_finish_kernel(const double* __restrict__ partial, long per_image, double* __restrict__ out,
                                                                  const float* __restrict__ part_minmax, float* __restrict__ minmax) {
    __shared__ double sh[kThreads];
    __shared__ float shlo[kThreads], shhi[kThreads];
    const double* p = partial + (long)blockIdx.x * per_image;
    double acc = 0.0;
    for (long i = threadIdx.x; i < per_image; i += kThreads) acc += p[i];
    const double s = tree_sum_256(acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
    if (part_minmax && blockIdx.x == 0) {
        const long total = (long)gridDim.x * per_image;
        float lo = INFINITY, hi = -INFINITY;
        for (long i = threadIdx.x; i < total; i += kThreads) {
            lo = nan_min(lo, part_minmax[2 * i]);
            hi = nan_max(hi, part_minmax[2 * i + 1]);
        }
        shlo[threadIdx.x] = lo;
        shhi[threadIdx.x] = hi;
        __syncthreads();
        for (int o = kThreads / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                shlo[threadIdx.x] = nan_min(shlo[threadIdx.x], shlo[threadIdx.x + o]);
                shhi[threadIdx.x] = nan_max(shhi[threadIdx.x], shhi[threadIdx.x + o]);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            minmax[0] = nan_min(minmax[0], shlo[0]);
            minmax[1] = nan_max(minmax[1], shhi[0]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ SSIM
struct SsimArgs {
    int H, W, OH, OW;        // plane and map (H - k + 1, W - k + 1) sizes
    int k, TH;               // window size; output rows of a tile (32, or 16 from k = 23 on so that the LDS stays below 64 KB)
    int tiles_x, tiles_y;
    float c1, c2;
    float g[kMaxKernel + 3];   // normalised 1-D Gaussian
};

inline int ssim_tile_rows(int k) { return k <= 21 ? 32 : 16; }
inline size_t ssim_lds_bytes(int k) {
    const int EH = ssim_tile_rows(k) + k - 1, EW = kTileW + k - 1;
    return sizeof(double) * kThreads + sizeof(float) * ((size_t)2 * EH * EW + (size_t)5 * EH * kTileW + kMaxKernel + 3);
}

// One workgroup per (plane, TH x 32 tile of the map).  LDS: the two (TH + k - 1) x (32 + k - 1) halo tiles as x - s, y - s (coalesced row loads; outside the plane: 0,
// which only reaches windows that are masked out), the horizontal pass of the five moments (x, y, xx, yy, xy) over every halo row (five [EH][32] planes; k = 11: 27 KB),
// the 1-D weights, 256 doubles for the tree.  Every LDS access of both passes has the 32 lanes of a half wave on 32 consecutive floats: no bank conflicts.
// Vertical pass, the SSIM expression (no clamp), the thread's pixels added in double in index order, then the tree: one double per tile.
template <typename T>
__global__ __launch_bounds__(kThreads) void ssim_tile_kernel(const T* __restrict__ a, const T* __restrict__ b, SsimArgs p, double* __restrict__ partial,
                                                             float* __restrict__ map) {
    extern __shared__ double ssim_lds[];
    const int k = p.k, TH = p.TH, EH = TH + k - 1, EW = kTileW + k - 1;
    double* red = ssim_lds;
    float* A = reinterpret_cast<float*>(ssim_lds + kThreads);
    float* B = A + EH * EW;
    float* Hm = B + EH * EW;                 // [5][EH][32]
    float* g = Hm + 5 * EH * kTileW;
    const int t = threadIdx.x;

    const long bid = blockIdx.x;
    const int tx = (int)(bid % p.tiles_x), ty = (int)((bid / p.tiles_x) % p.tiles_y);
    const long plane = bid / ((long)p.tiles_x * p.tiles_y);
    const int y0 = ty * TH, x0 = tx * kTileW;
    const T* pa = a + plane * p.H * (long)p.W;
    const T* pb = b + plane * p.H * (long)p.W;

    if (t < k) g[t] = p.g[t];
    const float s = load01(pb, (long)min(y0 + EH / 2, p.H - 1) * p.W + min(x0 + EW / 2, p.W - 1));
    for (int i = t; i < EH * EW; i += kThreads) {
        const int r = i / EW, c = i - r * EW;
        const int gy = y0 + r, gx = x0 + c;
        float va = 0.f, vb = 0.f;
        if (gy < p.H && gx < p.W) {
            const long o = (long)gy * p.W + gx;
            va = __fsub_rn(load01(pa, o), s);
            vb = __fsub_rn(load01(pb, o), s);
        }
        A[i] = va;
        B[i] = vb;
    }
    __syncthreads();

    const int plane_sz = EH * kTileW;
    for (int i = t; i < plane_sz; i += kThreads) {
        const int r = i >> 5, c = i & 31;
        const float* ra = A + r * EW + c;
        const float* rb = B + r * EW + c;
        float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
        for (int j = 0; j < k; ++j) {
            const float w = g[j], x = ra[j], y = rb[j];
            const float wx = w * x, wy = w * y;
            sx += wx;
            sy += wy;
            sxx = fmaf(wx, x, sxx);
            syy = fmaf(wy, y, syy);
            sxy = fmaf(wx, y, sxy);
        }
        Hm[i] = sx;
        Hm[plane_sz + i] = sy;
        Hm[2 * plane_sz + i] = sxx;
        Hm[3 * plane_sz + i] = syy;
        Hm[4 * plane_sz + i] = sxy;
    }
    __syncthreads();

    double acc = 0.0;
    for (int i = t; i < TH * kTileW; i += kThreads) {
        const int oy = i >> 5, ox = i & 31;
        const float* h = Hm + oy * kTileW + ox;
        float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
        for (int j = 0; j < k; ++j) {
            const float w = g[j];
            const float* hj = h + j * kTileW;
            mx = fmaf(w, hj[0], mx);
            my = fmaf(w, hj[plane_sz], my);
            exx = fmaf(w, hj[2 * plane_sz], exx);
            eyy = fmaf(w, hj[3 * plane_sz], eyy);
            exy = fmaf(w, hj[4 * plane_sz], exy);
        }
        const int gy = y0 + oy, gx = x0 + ox;
        if (gy < p.OH && gx < p.OW) {
            const float vxx = exx - mx * mx, vyy = eyy - my * my, vxy = exy - mx * my;   // about s: the shift cancels in all three
            const float ux = mx + s, uy = my + s;
            const float num = (2.f * ux * uy + p.c1) * (2.f * vxy + p.c2);
            const float den = (ux * ux + uy * uy + p.c1) * (vxx + vyy + p.c2);
            const float v = num / den;
            if (map) map[(plane * p.OH + gy) * (long)p.OW + gx] = v;
            acc += (double)v;
        }
    }
    const double sum = tree_sum_256(acc, red);
    if (t == 0) partial[bid] = sum;
}

template <typename T>
void ssim_launch(const void* a, const void* b, const SsimArgs& p, long blocks, double* partial, float* map, hipStream_t s) {
    hipLaunchKernelGGL(ssim_tile_kernel<T>, dim3((unsigned)blocks), dim3(kThreads), ssim_lds_bytes(p.k), s, static_cast<const T*>(a), static_cast<const T*>(b), p, partial, map);
    LAUNCH_CHECK();
}

bool metrics_shape_ok(int dtype, int n, int C, int H, int W) {
    if (dtype != BEVGEN_DTYPE_F32 && dtype != BEVGEN_DTYPE_U8) return false;
    if (n < 1 || C < 1 || H < 1 || W < 1) return false;
    return (long)C * H * W <= 0x7FFFFFFFL && (long)n * C <= (1L << 23);   // (n G workgroups and n C tiles_y tiles_x tiles stay below 2^31)
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host side
int image_sqerr_blocks(long count) { return (int)std::max<long>(1, std::min<long>((count + 2047) / 2048, 128)); }

long image_sqerr_workspace_bytes(int n, int C, int H, int W) {
    if (!metrics_shape_ok(BEVGEN_DTYPE_F32, n, C, H, W)) return -1;
    const long parts = (long)n * image_sqerr_blocks((long)C * H * W);
    return parts * (long)(sizeof(double) + 2 * sizeof(float));
}

long ssim_tiles_per_image(int C, int H, int W, int k) {
    const int OH = H - k + 1, OW = W - k + 1;
    return (long)C * cdiv(OH, ssim_tile_rows(k)) * cdiv(OW, kTileW);
}

long ssim_workspace_bytes(int n, int C, int H, int W, int k) {
    if (!metrics_shape_ok(BEVGEN_DTYPE_F32, n, C, H, W) || k < 1 || k > kMaxKernel || k % 2 == 0 || H < k || W < k) return -1;
    const long parts = (long)n * ssim_tiles_per_image(C, H, W, k);
    return parts > 0x7FFFFFFFL ? -1 : parts * (long)sizeof(double);
}

void launch_image_sqerr(const void* a, const void* b, int dtype, int n, int C, int H, int W, double* sse, float* minmax, void* work, hipStream_t s) {
    BG_REQUIRE(metrics_shape_ok(dtype, n, C, H, W), "image_sqerr: images [%d, %d, %d, %d] of dtype %d (needs a non-empty fp32 or uint8 batch)", n, C, H, W, dtype);
    const long count = (long)C * H * W;
    const int G = image_sqerr_blocks(count);
    double* partial = static_cast<double*>(work);
    float* part_minmax = reinterpret_cast<float*>(partial + (long)n * G);
    if (dtype == BEVGEN_DTYPE_F32)
        hipLaunchKernelGGL(image_sqerr_kernel<float>, dim3((unsigned)((long)n * G)), dim3(kThreads), 0, s, static_cast<const float*>(a), static_cast<const float*>(b), count, G, partial,
                           part_minmax);
    else
        hipLaunchKernelGGL(image_sqerr_kernel<uint8_t>, dim3((unsigned)((long)n * G)), dim3(kThreads), 0, s, static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), count, G, partial,
                           part_minmax);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(n), dim3(kThreads), 0, s, partial, (long)G, sse, part_minmax, minmax);
    LAUNCH_CHECK();
}

void launch_ssim(const void* a, const void* b, int dtype, int n, int C, int H, int W, int k, double sigma, double data_range, double k1, double k2, double* sums, float* map,
                 void* work, hipStream_t s) {
    BG_REQUIRE(metrics_shape_ok(dtype, n, C, H, W), "ssim: images [%d, %d, %d, %d] of dtype %d (needs a non-empty fp32 or uint8 batch)", n, C, H, W, dtype);
    BG_REQUIRE(k >= 1 && k <= kMaxKernel && k % 2 == 1, "ssim: kernel_size %d (odd, 1 .. %d)", k, kMaxKernel);
    BG_REQUIRE(H >= k && W >= k, "ssim: a %d x %d plane has no valid %d x %d window", H, W, k, k);
    BG_REQUIRE(sigma > 0.0 && data_range > 0.0, "ssim: sigma %g, data_range %g (both > 0)", sigma, data_range);
    SsimArgs p{};
    p.H = H, p.W = W, p.OH = H - k + 1, p.OW = W - k + 1, p.k = k, p.TH = ssim_tile_rows(k);
    p.tiles_x = cdiv(p.OW, kTileW), p.tiles_y = cdiv(p.OH, p.TH);
    p.c1 = (float)((k1 * data_range) * (k1 * data_range)), p.c2 = (float)((k2 * data_range) * (k2 * data_range));
    double gd[kMaxKernel], gs = 0.0;
    for (int j = 0; j < k; ++j) {
        const double d = (double)j - 0.5 * (k - 1);
        gd[j] = std::exp(-0.5 * (d / sigma) * (d / sigma));
        gs += gd[j];
    }
    for (int j = 0; j < k; ++j) p.g[j] = (float)(gd[j] / gs);
    const long per_image = ssim_tiles_per_image(C, H, W, k), blocks = (long)n * per_image;
    BG_REQUIRE(blocks <= 0x7FFFFFFFL && n <= 0x7FFFFFFF, "ssim: %ld tiles in one call", blocks);
    double* partial = static_cast<double*>(work);
    if (dtype == BEVGEN_DTYPE_F32)
        ssim_launch<float>(a, b, p, blocks, partial, map, s);
    else
        ssim_launch<uint8_t>(a, b, p, blocks, partial, map, s);
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(n), dim3(kThreads), 0, s, partial, per_image, sums, (const float*)nullptr, (float*)nullptr);
    LAUNCH_CHECK();
}

}  // namespace bevgen
