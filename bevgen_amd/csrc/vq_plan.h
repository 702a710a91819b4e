// The pure part of the VQGAN host driver (vqdec.cpp): activation sizes, the pass cut, the range-safe sites of a pass and the form of the upsample convolution, as plain
// functions of a small shape struct.  No HIP header, no environment read, no heap.  Exercised on the CPU (tests/test_vq_plan_cpu.py through tests/host/vq_plan_dump.cpp);
// vq_finalize / vq_enc_finalize fill the shape from the loaded weights, vq_decode / vq_encode execute what the plan says.
#pragma once
#include <algorithm>

namespace bevgen {

constexpr int kVqMaxLevels = 8;   // bevgen_cfg::vq_ch_mult

// What the plan needs to know of one direction of the loaded model.  Level 0 is the full resolution in both directions; the decoder walks levels - 1 .. 0, the encoder 0 .. levels - 1.
struct VqShape {
    bool encoder = false;
    int levels = 0, ch = 0;
    int ch_mult[kVqMaxLevels] = {};
    bool attn[kVqMaxLevels] = {};        // the level's blocks are followed by AttnBlocks
    int nin[kVqMaxLevels] = {};          // blocks of the level with a nin_shortcut
    bool first_nin[kVqMaxLevels] = {};   // the level's first block is one of them (it then reads the resampled tensor of the level before)
    bool resample[kVqMaxLevels] = {};    // the level ends in an Upsample (decoder) / a Downsample (encoder)
    int mid_nin = 0;                     // the same count over mid.block_1 and mid.block_2
    int cin_pad = 0;                     // encoder: the image's channels padded to the GEMM's k granularity
};

// The switches of the VQGAN path, one environment variable each, all for A/B runs; vq_switches() in vqdec.cpp reads them once per process.
struct VqSwitches {
    bool gn_epilogue = true;   // $BEVGEN_GN_EPILOGUE: 0 = always the statistics pass over the tensor, never the producing convolution's epilogue partials
    bool enc_fuse = true;      // $BEVGEN_VQ_ENC_FUSE: 0 = the unfused pairs of the encoder's two fused passes (layout change + absmax, unscale + absmax)
    bool up_planes = true;     // $BEVGEN_VQ_UP_PLANES: 0 = the upsample convolution reads fp32 on the register-staged kernel, as in rounds 2-4
    bool tail = true;          // $BEVGEN_VQ_TAIL: 0 = the three-kernel tail (norm_out + swish, conv_out, denormalise + layout)
};

struct VqSizes {
    long per_img = 0;                // floats of the widest activation of one image
    int max_c = 0;                   // widest channel count
    long attn_hw = 0, attn_hwp = 0;  // most attention tokens per image, and padded to the GEMM's k granularity (14 x 25 = 350 -> 352)
    int lat_h = 0, lat_w = 0;        // latent grid
    int RH = 0, RW = 0;              // image
};

// Both networks are fully convolutional (stage1/model.py:405-433, :506-537).  Decoder: (h, w) is the latent grid (cam_latent_res, e.g. 16 x 16 or nuScenes' 14 x 25), the image
// (h << (levels-1)) x (w << (levels-1)).  Encoder: (h, w) is the image, multiples of 2^(levels-1) (256 x 256, 224 x 400).  Which levels carry AttnBlocks is decided by
// ddconfig.resolution alone (curr_res == attn_resolutions, :466-480), so VqShape::attn comes from the loaded weights, not from (h, w).
inline VqSizes vq_scan(const VqShape& sh, int h, int w) {
    VqSizes z;
    const int top = sh.levels - 1;
    if (sh.encoder) { z.RH = h; z.RW = w; z.lat_h = h >> top; z.lat_w = w >> top; }
    else { z.lat_h = h; z.lat_w = w; z.RH = h << top; z.RW = w << top; }
    const long lat_hw = (long)z.lat_h * z.lat_w;
    z.attn_hw = lat_hw;   // the mid AttnBlock
    // widest activation per image: max over levels of h*w * channels; most attention tokens over the levels that carry AttnBlocks
    if (sh.encoder) {
        z.per_img = (long)h * w * std::max(sh.cin_pad, sh.ch);   // the padded image and conv_in's output
        z.max_c = sh.ch;
        long hw = (long)h * w;
        for (int lvl = 0; lvl < sh.levels; ++lvl) {
            const int ch = sh.ch * sh.ch_mult[lvl];
            z.per_img = std::max(z.per_img, hw * ch);
            z.max_c = std::max(z.max_c, ch);
            if (sh.attn[lvl]) z.attn_hw = std::max(z.attn_hw, hw);
            if (lvl != top) hw /= 4;
        }
    } else {
        long hw = lat_hw;
        for (int lvl = top; lvl >= 0; --lvl) {
            const int ch = sh.ch * sh.ch_mult[lvl];
            const int ch_in = lvl == top ? ch : sh.ch * sh.ch_mult[lvl + 1];
            z.per_img = std::max(z.per_img, hw * std::max(ch, ch_in));
            z.max_c = std::max(z.max_c, std::max(ch, ch_in));
            if (sh.attn[lvl]) z.attn_hw = std::max(z.attn_hw, hw);
            if (lvl != 0) hw *= 4;
        }
    }
    z.attn_hwp = (z.attn_hw + 31) / 32 * 32;
    return z;
}

// Images per pass: the 16 x 16 stages only fill the chip (256 x 128 tiles on 256 CUs) from ~48 images; 148 -> 128 ms per 96 images vs 16, arena ~10 GB.  (Round 5: smaller
// passes whose full-resolution tensors would fit the 256 MB memory-side cache between conv -> statistics -> apply -> conv are slower throughout: 6 / 12 / 24 images per
// pass 11.96 / 9.14 / 7.96 ms per scene against 7.47, profiles/r05_ab_vq.txt)
constexpr int kVqChunkMax = 48;
struct VqPasses { int chunk = 0, passes = 0; };   // every pass takes `chunk` images, the last one the rest
inline VqPasses vq_pass_cut(int n_total) {
    VqPasses p;
    p.chunk = std::min(n_total, kVqChunkMax);
    p.passes = p.chunk > 0 ? (n_total + p.chunk - 1) / p.chunk : 0;
    return p;
}

// Range-safe sites of one pass (vqdec.cpp RangeSites): decoder conv_in, every nin_shortcut, every upsample; encoder conv_in, quant_conv, every nin_shortcut, every downsample
inline int vq_sites_per_pass(const VqShape& sh) {
    int n = (sh.encoder ? 2 : 1) + sh.mid_nin;
    for (int lvl = 0; lvl < sh.levels; ++lvl) n += sh.nin[lvl] + (sh.resample[lvl] ? 1 : 0);
    return n;
}
// encoder: the downsample of `lvl` writes the next level's residual stream; where that level opens with a nin_shortcut, the downsample's output is that site's operand
inline bool vq_feeds_nin(const VqShape& sh, int lvl) { return sh.encoder && sh.resample[lvl] && lvl + 1 < sh.levels && sh.first_nin[lvl + 1]; }

// The upsample convolution reads the block output directly (no GroupNorm in front of it, stage1/model.py:49-53).  In split-precision mode (`planes`) the tensor is first re-laid
// out as (hi, lo) planes - one elementwise pass over the SMALL pre-upsample tensor - so that the 4x larger convolution runs on the LDS-DMA kernel instead of the
// register-staged one; the re-layout takes C / 4 a power of two and C % 32 == 0.  Where it does not apply, the range-safe mode takes its fp32 form of the site.
enum VqUpForm { VQ_UP_PLANES = 0, VQ_UP_RANGED_F32 = 1, VQ_UP_PLAIN = 2 };
inline VqUpForm vq_up_form(int C, bool planes, bool range, const VqSwitches& sw) {
    const int q4 = C >> 2;
    if (planes && sw.up_planes && (q4 & (q4 - 1)) == 0 && C % 32 == 0) return VQ_UP_PLANES;
    return planes && range ? VQ_UP_RANGED_F32 : VQ_UP_PLAIN;
}

}  // namespace bevgen
