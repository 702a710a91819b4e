/* libbevgen_hip - C ABI of the MI355X-native BEVGen stage-2 sampling path (gfx950 / ROCm).
 *
 * The reference (alexanderswerdlow/BEVGen) is pure Python: it has NO FFI for this path; its "plugin" mechanism is
 * Hydra `_target_` instantiation of Python classes (configs/experiment/muse_stage_two_multi_view.yaml:17,26,31,41;
 * configs/model/stage_2.yaml:1,7,9,36,59).  The drop-in is therefore two layers:
 *   - Python classes with the reference's constructor/forward signatures (package bevgen_amd), and
 *   - this C ABI underneath them, which is what a maintainer binds (ctypes stub in INTEGRATION.md).
 * Each entry point below names the reference function whose arithmetic it replaces (paths under
 * multi_view_generation/, line numbers as in the surveyed tree).
 *
 * Conventions
 *   - every function returns 0 on success, a negative code on failure; bevgen_last_error(ctx) gives the message
 *   - the CALLER owns every buffer passed in; `const T* d_*` / `T* d_*` are DEVICE pointers (e.g. torch tensor
 *     data_ptr()), `h_*` are HOST pointers; the library owns weights, KV cache and workspace inside the context
 *   - `stream` is a hipStream_t (0 = default stream); calls are asynchronous on it unless stated otherwise,
 *     the library performs no hidden host synchronisation on the sampling path.  One documented exception: a Route-A context created with decode_path = AUTO
 *     and max_batch > 4 that is nevertheless called with <= 4 sequences packs the split decode layer's q/k/v operand image on that FIRST such call
 *     (one device allocation per layer, ~300 MB at BASELINE config 4 in fp32, and one stream synchronisation, once per context); every other
 *     configuration (max_batch 0 or <= 4, decode_path = SPLIT) takes it at bevgen_finalize
 *   - one context per (device, model); a context is not thread-safe, different contexts may be used from different host threads concurrently
 *   - int64 token ids, fp32 everything else (the arithmetic type is a context property: BEVGEN_PRECISION_*)
 */
#ifndef BEVGEN_HIP_H
#define BEVGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEVGEN_ABI_VERSION 10   /* 10 (additive, same version and struct): classifier-free guidance of Route M - bevgen_maskgit_generate_guided, bevgen_muse_forward_ex, bevgen_op_add_row_layernorm, bevgen_op_cfg_combine; a library without them is told apart by the missing symbols.  10 (additive, same version and struct): bevgen_vq_encode_ex, bevgen_op_vq_geo_embed, bevgen_op_vq_quant_error; a library without them is told apart by the missing symbols.  10: bevgen_cfg.vq_range covers bevgen_vq_encode (bevgen_vq_range_exponents reports the most recent decode OR encode call), bevgen_op_conv_ranged.  9: operator entries of the VQGAN building blocks (bevgen_op_conv3x3_down, _vq_attn_block, _vq_out_tail, _vq_quantize, _conv3x3_gn_stats), BEVGEN_STATUS_NONFINITE_LATENTS.  8: bevgen_cfg.vq_range (taken out of reserved[]: the struct size is unchanged), bevgen_vq_range_exponents, bevgen_op_range_split.  7: operator entries of the token samplers (bevgen_op_remask, _maskgit_pick, _critic_scores, _ar_pick, _ar_score_rows, _mean_fixed_order).  6: device status word (bevgen_synchronize, bevgen_status, BEVGEN_ERR_NUMERIC, BEVGEN_STATUS_*).  5: bevgen_op_mlp_fused; a context without max_batch <= 4 packs the split decode layer lazily (see Conventions).  4: 4: BEVGEN_PROFILE_KINDS 5 -> 6 (bevgen_profile_end writes 18 doubles), bevgen_cfg.decode_chains, decode_path values 2 / 3 */

enum { BEVGEN_ROUTE_MASKGIT = 0, BEVGEN_ROUTE_AR = 1 };
/* FP32  : every product and accumulation in exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32) - bit-exact greedy tokens vs the CPU reference.
 * F16X3 : large GEMMs / convolutions as 3 f16 MFMAs per k-step on (hi, lo*2^-11) splits of the fp32 operands: ~2^-22 relative error per product,
 *         fp32 accumulation, up to 5x the fp32 MFMA rate.  Everything else (attention, norms, samplers, decode-step GEMMs) stays fp32.
 * F16X1 : "single product", an opt-in trade of accuracy for matrix instructions on Route M.  The context is an F16X3 context in everything (VQGAN, Route A, attention,
 *         range policy: |v| >= 65520 raises BEVGEN_STATUS_F16_RANGE) except that every Route M projection that multiplies pre-split operands - to_q, to_kv, the merged
 *         self-attention q|k|v, to_out, both feed-forward matrices, to_logits, their split-K forms, and whatever Route M sends through the on-the-fly-split kernel -
 *         computes f16(A) f16(W)^T with fp32 accumulation: ONE MFMA per product.  bevgen_finalize rounds those matrices to f16 in place whatever weight_dtype says and
 *         builds no LayerNorm fold constants (as under BEVGEN_W_F16); the VQGAN's convolutions keep following weight_dtype.  Epilogues (bias, GELU, residual, the q /
 *         q|k|v / k|v preparation, GEGLU) and the plane writers are unchanged; the attention kernel keeps its three products (its loop is bound by the softmax phase, not
 *         by the matrix phase).  The mode reaches a launch only from bevgen_muse_forward, bevgen_maskgit_generate and bevgen_maskgit_generate_ex.  Activations are
 *         rounded to 11 significant bits on every call, where the reference's bf16 autocast keeps 8.  (A value of this enum and not a word of bevgen_cfg.reserved[]: a
 *         library that does not know the mode refuses the context instead of running it with three products.) */
enum { BEVGEN_PRECISION_FP32 = 0, BEVGEN_PRECISION_BF16 = 1 /* reserved */, BEVGEN_PRECISION_F16X3 = 2, BEVGEN_PRECISION_F16X1 = 3 };
/* KV-cache storage of Route A.  BEVGEN_KV_I8 (opt-in, lossy): per layer, K and V each are [B, H, Lmax, 64] int8 codes followed immediately by [B, H, Lmax] fp32 row scales
 * - 68 B H Lmax bytes, the scale plane at byte offset 64 B H Lmax.  Quantiser of one 64-element row r (one head's k or v of one token), IEEE fp32 throughout:
 * amax = max |r_i|; amax < 1e-30: codes 0, scale 0; else scale = amax / 127, code_i = clamp(rint(r_i * (127 / amax)), -127, 127) (round to nearest even); the value read
 * back is code_i * scale.  Every finite row is representable (no range refusal); a NaN / inf in a row raises BEVGEN_STATUS_KV_NONFINITE. */
enum { BEVGEN_KV_F32 = 0, BEVGEN_KV_F16 = 1, BEVGEN_KV_I8 = 2 };
enum { BEVGEN_DECODE_FUSED = 0, BEVGEN_DECODE_PER_OP = 1, BEVGEN_DECODE_SPLIT = 2, BEVGEN_DECODE_AUTO = 3 };
/* BEVGEN_W_I8 (decode_weight_dtype only): int8 codes with one fp32 scale per output row of a projection matrix W [N, K] - the quantiser of the int8 KV cache above applied
 * to the row W[n, :] (amax over the row; amax < 1e-30: codes 0, scale 0; scale = amax / 127, code = clamp(rint(w * (127 / amax)), -127, 127), value = code * scale). */
enum { BEVGEN_W_F32 = 0, BEVGEN_W_F16 = 1, BEVGEN_W_I8 = 2 };
enum { BEVGEN_DTYPE_F32 = 0, BEVGEN_DTYPE_I64 = 1, BEVGEN_DTYPE_U8 = 2, BEVGEN_DTYPE_F64 = 3 };

enum {
    BEVGEN_OK = 0,
    BEVGEN_ERR_INVALID = -1,   /* bad argument / missing tensor / unsupported size */
    BEVGEN_ERR_HIP = -2,       /* a HIP runtime call failed */
    BEVGEN_ERR_STATE = -3,     /* call order violated (e.g. generate before finalize) */
    BEVGEN_ERR_INTERNAL = -4,
    BEVGEN_ERR_NUMERIC = -5    /* a kernel flagged a non-finite logit / pixel or an operand outside the f16 range of the chosen precision (device status word, below):
                                  the results of the call that raised it are invalid */
};

/* Device status word.  The reference asserts on the HOST, every decode step, that the transformer's inputs and logits are finite
 * (transformer/mingpt_sparse.py:383,388; stage2/cond_transformer_multi_view.py:202).  This library never synchronises on the sampling path; instead the kernels
 * that touch the values anyway OR a bit into one host-visible word per context (mapped host memory) and the host reads it
 *   - in bevgen_synchronize (after waiting for the stream: the call a caller makes before it trusts / copies the results),
 *   - at the entry of EVERY later entry point on the context (no synchronisation: an error raised by an earlier asynchronous call is reported by the next call at the latest),
 *   - in bevgen_finalize (weights outside the f16 range of the chosen precision) and, as a message on stderr, in bevgen_destroy.
 * A raised word is returned as BEVGEN_ERR_NUMERIC (bits 4, 8, 16, 32, 64) or BEVGEN_ERR_INTERNAL (bits 1, 2) and then cleared.
 * Policy for precision = F16X3 / fp16 storage modes: an operand whose f16 image would be inf / NaN (|v| >= 65520) is an ERROR, not rescaled - the split keeps fp32-class
 * mantissas but f16's exponent range, where the reference's bf16 / fp32 arithmetic has 8 exponent bits; such a checkpoint must run with BEVGEN_PRECISION_FP32.
 * One opt-in exception, stage 1 only: with bevgen_cfg.vq_range = 1 the un-normalised activation tensors of the decoder and the encoder that become f16 operands (decoder: in
 * front of the upsample convolutions, the nin_shortcut convolutions and conv_in; encoder: the image in front of conv_in, the residual stream in front of the nin_shortcut
 * and downsample convolutions, conv_out's output in front of quant_conv) are rescaled by a per-tensor power of two chosen on the device (exact in every bit the split
 * keeps), so BEVGEN_STATUS_F16_RANGE is then raised by stage 1 only for NaN / inf activations and for a codebook entry outside the range.  Weights outside the range are
 * refused by bevgen_finalize in either setting; the transformer routes ignore vq_range. */
enum {
    BEVGEN_STATUS_MLP_BARRIER = 1,        /* fused MLP launch of the decode step: an XCD-local barrier timed out (the GPU was shared); the context falls back to two launches */
    BEVGEN_STATUS_MLP_PLACEMENT = 2,      /* ...: a workgroup was not placed on the XCD its index implies */
    BEVGEN_STATUS_NONFINITE_LOGITS = 4,   /* a sampler read a NaN / inf logit or critic score */
    BEVGEN_STATUS_F16_RANGE = 8,          /* a value written as an f16 operand (hi / lo planes, fp16 KV cache, fp16 decode activations, fp16 weights) was NaN or |v| >= 65520 */
    BEVGEN_STATUS_NONFINITE_PIXELS = 16,  /* the VQGAN decoder produced a NaN / inf pixel */
    BEVGEN_STATUS_NONFINITE_LATENTS = 32, /* the VQGAN quantizer met a latent row without a finite distance to any codebook entry (NaN / inf in the image or an overflow in the
                                             encoder): that row's token id is written as 0 */
    BEVGEN_STATUS_KV_NONFINITE = 64       /* a key / value row written into the int8 KV cache (BEVGEN_KV_I8) held a NaN / inf */
};

/* Sizes of the stage-2 transformer (mirror of GPTConfig, modules/transformer/mingpt_sparse.py:26-102) and of the
 * stage-1 VQGAN decoder (ddconfig, configs/model/stage_2.yaml:45-55).  Zero-initialise, then fill. */
typedef struct bevgen_cfg {
    int32_t abi_version;     /* = BEVGEN_ABI_VERSION */
    int32_t route;           /* BEVGEN_ROUTE_* */
    int32_t precision;       /* BEVGEN_PRECISION_* (arithmetic of projections / KV-cache storage) */
    int32_t num_layers, num_heads, dim, vocab_size, cond_vocab_size;
    int32_t num_cams, cam_latent_h, cam_latent_w;      /* T = h*w tokens per camera, N = C*T */
    int32_t num_cond_tokens;                           /* K (BEV latent cells) */
    int32_t seq_len;                                   /* L = gpt_block_size */
    int32_t sparse_block_size;                         /* blk; L % blk == 0 */
    int32_t image_embed, bev_embed, camera_bias;       /* feature flags */
    int32_t ff_inner;                                  /* Route M: int(dim*4*2/3); 0 for Route A */
    int32_t max_batch;                                 /* upper bound on scenes (Route M) / sequences (Route A) per call */
    /* stage-1 decoder; vq_ch == 0 -> no VQGAN in this context */
    int32_t vq_ch, vq_num_res_blocks, vq_z_channels, vq_embed_dim, vq_n_embed, vq_resolution, vq_out_ch;
    int32_t vq_num_levels;
    int32_t vq_ch_mult[8];
    int32_t vq_attn_resolution;                        /* spatial size at which AttnBlocks are inserted (16) */
    int32_t vq_in_channels;                            /* encoder input channels (3 images / 7 Argoverse BEV classes); 0 = decoder only */
    int32_t kv_cache_dtype;                            /* Route A KV-cache storage: BEVGEN_KV_F32 (default, bit-exact tokens) or BEVGEN_KV_F16 (fp16 storage,
                                                          fp32 accumulate: half the decode-attention HBM traffic; tokens no longer guaranteed identical) or
                                                          BEVGEN_KV_I8 (int8 codes + one fp32 scale per (token, head) row, fp32 accumulate: 68 bytes per row; lossy) */
    int32_t decode_path;                               /* Route A decode step: BEVGEN_DECODE_FUSED (default: three launches per layer, decode_fused.hip) or
                                                          BEVGEN_DECODE_PER_OP (one kernel per operator: the round-1 path, kept as the A/B reference) or
                                                          BEVGEN_DECODE_SPLIT (four launches per layer: LayerNorm + QKV projection of the whole batch as one MFMA kernel that
                                                          reads the weight once, then the decode-attention kernel proper = the K/V stream and nothing else) or
                                                          BEVGEN_DECODE_AUTO (what the Python host asks for: SPLIT, with the key walk of every (sequence, head) cut into up to
                                                          four ranges, for up to four sequences / layout groups per call - the interactive single-scene caller, where 16-64
                                                          workgroups per layer cannot pull weights and K/V fast enough: 0.92 vs 1.12 ms/step at B = 1 - else FUSED; with
                                                          decode_weight_dtype = BEVGEN_W_F16 FUSED at every batch size: its single MLP launch makes it the faster form, 0.71 vs 0.83) */
    int32_t decode_weight_dtype;                       /* Route A projection weights (q/k/v, MLP, head): BEVGEN_W_F32 (default) or BEVGEN_W_F16: bevgen_finalize rounds them to
                                                          fp16-representable values (prefill and decode then use the same model: the reference's Route A runs fp16,
                                                          sparse_self_attention.py:127) and the decode step streams the 2-byte copies: half the weight traffic; or
                                                          BEVGEN_W_I8: bevgen_finalize replaces them by code * scale (int8 codes, one fp32 scale per output row; the
                                                          fused q | k | v matrix row by row, i.e. per row of each [D, D] matrix) - prefill, bevgen_ar_forward and decode
                                                          run that one model - and the decode step streams the 1-byte codes, with the row scale applied to the fp32
                                                          accumulator.  Both need a fused-like decode_path and dim % 256 == 0; BEVGEN_W_I8 excludes weight_dtype =
                                                          BEVGEN_W_F16 (dequantised values are not fp16-representable) */
    int32_t weight_dtype;                              /* every matrix that feeds a split-precision GEMM / convolution (needs BEVGEN_PRECISION_F16X3): BEVGEN_W_F32
                                                          (default: hi + lo f16 planes, three MFMAs per product, fp32-class results on the fp32 weights) or BEVGEN_W_F16:
                                                          bevgen_finalize rounds those matrices to f16 once (the reference's own GPU runs cast them to bf16 / fp16 on
                                                          every call: muse bf16 autocast, sparse_self_attention.py:127) - activations keep their hi + lo planes, a
                                                          product is two MFMAs, and the results are fp32-class results OF THE ROUNDED MODEL.  Route A: together with
                                                          decode_weight_dtype = BEVGEN_W_F16 only */
    int32_t decode_chains;                             /* Route A fused decode step: the batch is cut into this many independent sequence groups ("chains") whose
                                                          layer kernels are enqueued on separate HIP streams (one fork / join per step inside the captured graph), so
                                                          that one chain's weight-streaming projections run under another chain's K/V stream instead of every short
                                                          dependent kernel paying its ramp alone.  0 = the library's choice for the batch, 1 = a single chain */
    int32_t vq_range;                                  /* stage 1 (decoder and encoder) with BEVGEN_PRECISION_F16X3: 0 (default) = an un-normalised activation outside the f16 operand range
                                                          is refused (BEVGEN_STATUS_F16_RANGE); 1 = "range-safe": per call and per site, a device-side absmax of the tensor, an
                                                          exponent e (0 where absmax < 32768, else the smallest e with absmax 2^-e < 32768), the operand split as x 2^-e and the
                                                          convolution's result formed as 2^e (W x') + bias (+ residual).  No host synchronisation; e = 0 everywhere gives the bits
                                                          of vq_range = 0.  Ignored with BEVGEN_PRECISION_FP32 */
    int32_t reserved[9];
} bevgen_cfg;

typedef struct bevgen_ctx bevgen_ctx;

/* ---------------------------------------------------------------------------------------------------------------
 * lifecycle                                                                                                       */
int bevgen_create(const bevgen_cfg* cfg, int device, bevgen_ctx** out);
void bevgen_destroy(bevgen_ctx* ctx);
const char* bevgen_last_error(const bevgen_ctx* ctx);   /* ctx may be NULL: error of the last failed bevgen_create */
int bevgen_abi_version(void);
/* Wait for `stream` (and the library's own decode stream) and report what the kernels of the calls enqueued so far flagged: 0, or BEVGEN_ERR_NUMERIC / BEVGEN_ERR_INTERNAL
 * with the details in bevgen_last_error.  This is where the reference's per-step `assert isfinite` lands (see "Device status word" above). */
int bevgen_synchronize(bevgen_ctx* ctx, void* stream);
/* The raw status word (BEVGEN_STATUS_* bits) as the host sees it right now: no synchronisation, nothing cleared. */
int bevgen_status(bevgen_ctx* ctx, unsigned* word);

/* Upload one tensor (synchronous H2D copy).  `name` is the reference state_dict key
 * (utils/general.py:119-160 loader semantics: names listed in bevgen_amd/weights.py), with the prefixes
 *   "transformer." / "token_critic."  Route M MaskGit keys   (stage2/muse_maskgit_pytorch.py:204-261, 388-392)
 *   ""                                Route A GPT keys        (transformer/mingpt_sparse.py:267-308)
 *   "first_stage_model."              stage-1 VQModel keys    (stage1/vqgan.py:31-80)
 * or one of the static tables (built on the host exactly as in the reference, bevgen_amd/tables.py):
 *   "table.forward_shuffle_idx" i64[N]   CustomPermuter          transformer/permuter.py:33-88
 *   "table.attention_mask"      f32[L,L] allowed_pattern[0]      transformer/mask_generator.py:202-206
 *   "table.layout"              i64[H,L/blk,L/blk]               transformer/mask_generator.py:217-228
 *   "table.prob_matrix"         f32[L,L] camera-bias prior       transformer/mask_generator.py:172-190
 *   "table.image_plane"         f32[3,T] pixel plane             transformer/mingpt_sparse.py:288-294
 * Unknown names are stored and ignored (strict=False). */
int bevgen_load_tensor(bevgen_ctx* ctx, const char* name, const void* h_data, int dtype, int ndim, const int64_t* shape);

/* Convenience wrapper: the four tables at once (any pointer may be NULL to skip it). */
int bevgen_set_tables(bevgen_ctx* ctx, const int64_t* h_forward_shuffle_idx, const float* h_attention_mask,
                      const int64_t* h_layout, const float* h_prob_matrix, const float* h_image_plane);

/* Validate that every tensor the route needs is present and build the derived device data (fused QKV weights,
 * attention-bias matrices = tril-scatter(camera_bias_emb) + prob_matrix as in mingpt_sparse.py:375-380 /
 * muse_maskgit_pytorch.py:343-348, visibility masks, re-laid-out conv kernels).  Must precede any compute call. */
int bevgen_finalize(bevgen_ctx* ctx);

/* ---------------------------------------------------------------------------------------------------------------
 * Route M - MaskGit                                                                                               */

/* TransformerMultiView.forward in eval mode (stage2/muse_maskgit_pytorch.py:283-371):
 *   d_ids [B*C, T] (mask id = vocab_size), d_cond_ids [B, K], d_I_inv [B,C,3,3], d_E_inv [B,C,4,4]
 *   -> d_logits [B*C, T, V] and/or d_embed [B*C, T, D] (either may be NULL). */
int bevgen_muse_forward(bevgen_ctx* ctx, const int64_t* d_ids, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv,
                        int B, float* d_logits, float* d_embed, void* stream);
/* The same with null_condition != 0: the forward with context_mask = False for every scene (:158-166) - what the reference computes in .train() mode with
 * cond_drop_prob = 1 (:352-354), the "null" forward of classifier-free guidance.  No layout token is visible to the cross-attention, whose softmax then puts weight exactly 1
 * on the learned null key (exp(-finfo.max - finite) is 0 in fp32): layer i's cross-attention block adds r_i = to_out_i vec(null_v_i) to every row, a [D] vector that
 * bevgen_finalize computes once (fp64 accumulation, from the to_out matrix the context's mode multiplies by).  Self-attention, feed-forward, the final LayerNorm and
 * to_logits are bevgen_muse_forward's.  null_condition == 0 is bevgen_muse_forward. */
int bevgen_muse_forward_ex(bevgen_ctx* ctx, const int64_t* d_ids, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv,
                           int B, float* d_logits, float* d_embed, int null_condition, void* stream);

/* MaskGit.generate with the self token critic (stage2/muse_maskgit_pytorch.py:511-627).
 *   h_mask_schedule[timesteps]  tokens re-masked at each iteration, max(int(cos(pi/2 t) T), 1) (:566-567) - host-computed
 *   topk_k                      ceil((1 - topk_filter_thres) * V) (:453-454)
 *   d_gumbel_u [timesteps, B*C, T, V], d_critic_u [timesteps, B*C, T]  explicit U[0,1) noise replacing :430-431/:446-448,
 *                               NULL = deterministic setting (gumbel noise 0, critic uniform 0.5)
 *   noise_seed                  used when the explicit tensors are NULL: != 0 -> the samplers draw their uniforms in registers (Philox4x32-10 keyed by
 *                               (noise_seed, iteration, element): stream 0 = gumbel [rows*V], stream 1 = critic [rows]; bevgen_op_philox_uniform writes the
 *                               same numbers out) - stochastic sampling without 1.8 GB of noise tensors; 0 -> the deterministic setting
 *   d_init_ids [B*C, T] or NULL (partial decoding, :543-544, 573-574)
 *   -> d_out_ids [B*C, T]
 * The classifier-free-guidance "null" forwards of the reference (:272-276, 394-396) are bit-identical to the conditional
 * ones in eval mode and are not executed; the critic forward after the last iteration (result unused) is skipped.  Guidance with a real null-condition forward is
 * bevgen_maskgit_generate_guided (below). */
int bevgen_maskgit_generate(bevgen_ctx* ctx, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv, int B,
                            int timesteps, const int32_t* h_mask_schedule, float temperature, int topk_k, float critic_noise_scale,
                            const float* d_gumbel_u, const float* d_critic_u, const int64_t* d_init_ids, int64_t* d_out_ids,
                            unsigned long long noise_seed, void* stream);

/* The remaining branches of MaskGit.generate (stage2/muse_maskgit_pytorch.py:511-627) and BASELINE config 5's sample sharing:
 *   score_mode 0  the token critic (above);
 *              1  force_not_use_token_critic = True (:611-619): scores = 1 - softmax(logits)[pred], -1e5 at positions that were not masked in the iteration;
 *                 no critic forward is run (18 transformer forwards per call instead of 35); d_critic_u / critic_noise_scale are not used;
 *              2  ... with can_remask_prev_masked = True (:620-622): the same scores at EVERY position (the prediction is drawn everywhere)
 *   samples_per_layout S > 1: consecutive groups of S scenes share their BEV layout and cameras (all B = layouts * S rows of d_cond_ids / matrices are
 *                 passed; the flag enables the reuse): the condition embedding and the cross-attention K / V of every layer are built once per
 *                 LAYOUT and read by the S samples of the group. */
int bevgen_maskgit_generate_ex(bevgen_ctx* ctx, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv, int B,
                               int timesteps, const int32_t* h_mask_schedule, float temperature, int topk_k, float critic_noise_scale,
                               const float* d_gumbel_u, const float* d_critic_u, const int64_t* d_init_ids, int64_t* d_out_ids,
                               unsigned long long noise_seed, int score_mode, int samples_per_layout, void* stream);

/* bevgen_maskgit_generate_ex with classifier-free guidance (opt-in; departs from the reference's eval-mode behaviour, whose null forward equals the conditional one):
 * every iteration also runs the null-condition pass of bevgen_muse_forward_ex over the same ids and the logits the iteration uses - top-k filter, gumbel pick and the
 * 1 - softmax(logits)[pred] scores of score_mode 1 / 2 - are null + (cond - null) * cond_scale, evaluated in fp32 as three separately rounded operations (sub, mul, add).
 * The token critic reads the CONDITIONAL embed (SelfCritic.forward_with_cond_scale, :272, 394-396): its forward is the one of the unguided call.  Per iteration:
 * conditional forward + null pass (+ critic forward).  cond_scale == 1 runs exactly the launches of bevgen_maskgit_generate_ex. */
int bevgen_maskgit_generate_guided(bevgen_ctx* ctx, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv, int B,
                                   int timesteps, const int32_t* h_mask_schedule, float temperature, int topk_k, float critic_noise_scale,
                                   const float* d_gumbel_u, const float* d_critic_u, const int64_t* d_init_ids, int64_t* d_out_ids,
                                   unsigned long long noise_seed, int score_mode, int samples_per_layout, float cond_scale, void* stream);

/* MaskGit.forward in eval mode (stage2/muse_maskgit_pytorch.py:629-729; no condition drop, no self conditioning): the validation losses.
 *   d_ids [B*C, T]              the ground-truth token ids
 *   h_num_masked[B*C]           tokens masked per row, clamp(round(T cos(pi/2 t)), min = 1) (:660-662) - host-computed with the reference's own fp32 operations, in [1, T]
 *   d_perm_u [B*C, T] or NULL   the uniforms whose argsort is the reference's batch_randperm (:665): position i of a row is masked iff the index of the row's i-th smallest
 *                               uniform is below the row's count; equal uniforms rank by index (one of the orders an unstable argsort may return)
 *   d_gumbel_u [B*C, T, V] or NULL   uniforms of gumbel_sample (:713, no top-k); read with with_critic only
 *   noise_seed                  used where an explicit tensor is NULL: d_perm_u = Philox stream 2 (element = plain index), d_gumbel_u = stream 0 (the layout of
 *                               bevgen_maskgit_generate), both at iteration 0 and reproducible through bevgen_op_philox_uniform.  0 with a NULL tensor is refused.
 *   temperature                 sample_temperature (the reference's default is Python's random())
 *   with_critic                 0: the masked cross-entropy alone, d_out = {ce, ce, 0}; else d_out = {ce + critic_loss_weight * bce, ce, bce} (:729), which needs
 *                               token_critic.to_pred.* in the context
 *   d_mask_out [B*C, T] u8, d_x_out, d_critic_input_out [B*C, T] i64, each or NULL: the mask, the masked ids and where(mask, sampled, x) (:718; with_critic only)
 * ce = mean over the masked positions of logsumexp(logits) - logits[id]; bce = mean over all positions of BCE-with-logits(to_pred(embed(critic_input)), id != critic_input).
 * Both are fixed-order double sums rounded to float once: two calls give the same bits.  The two transformer forwards are bevgen_muse_forward's, in the context's precision. */
int bevgen_maskgit_loss(bevgen_ctx* ctx, const int64_t* d_ids, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv, int B,
                        const int32_t* h_num_masked, const float* d_perm_u, const float* d_gumbel_u, float temperature, unsigned long long noise_seed,
                        int with_critic, float critic_loss_weight, float* d_out /* [3] */, uint8_t* d_mask_out, int64_t* d_x_out, int64_t* d_critic_input_out,
                        void* stream);
/* The three kernels of bevgen_maskgit_loss, one entry each (sampler.hip).
 * maskgit_train_mask: d_mask [rows, T] = argsort(u) < d_num_masked[row] with u = d_perm_u, else Philox stream 2 of `seed`; d_x = mask_id where masked, else d_ids.  T <= 13107. */
int bevgen_op_maskgit_train_mask(bevgen_ctx* ctx, const int64_t* d_ids, const float* d_perm_u /* or NULL */, const int32_t* d_num_masked, int rows, int T, int64_t mask_id,
                                 unsigned long long seed, int64_t* d_x, uint8_t* d_mask, void* stream);
/* masked_ce: d_nll[p] = logsumexp(d_logits[p, :V]) - d_logits[p, d_ids[p]] where d_mask[p], 0 elsewhere (an id outside [0, V): NaN); V <= 1024, ldl >= V.  Non-finite logits of a
 * masked position raise BEVGEN_STATUS_NONFINITE_LOGITS.  d_out non-NULL: d_out[0] = sum(d_nll) / denom in a fixed order. */
int bevgen_op_masked_ce(bevgen_ctx* ctx, const float* d_logits, int ldl, const int64_t* d_ids, const uint8_t* d_mask, long rows, int V, long denom, float* d_nll,
                        float* d_out /* or NULL */, void* stream);
/* critic_bce: z = d_embed[p, :D] . d_w + d_b[0], y = (d_ids[p] != d_critic_input[p]), d_loss_rows[p] = max(z, 0) - z y + log1p(exp(-|z|)); D % 4 == 0, lde % 4 == 0, d_embed
 * and d_w 16-byte aligned.  d_out non-NULL: d_out[0] = the mean over the rows in a fixed order. */
int bevgen_op_critic_bce(bevgen_ctx* ctx, const float* d_embed, int lde, const float* d_w, const float* d_b, const int64_t* d_ids, const int64_t* d_critic_input, long rows,
                         int D, float* d_loss_rows, float* d_out /* or NULL */, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Route A - autoregressive sparse-causal transformer with camera bias (prefill + KV-cache decode)                 */

/* Operator seam: SparseSelfAttention.forward(query, key, value, attn_mask, add_mask)
 * (transformer/sparse_self_attention.py:103-177): q,k,v,out [B,H,L,64] fp32, layout i64 [H,L/blk,L/blk],
 * attn_mask f32 [L,L] ('mul' mode: 0 = masked), add_mask f32 [L,L] or NULL.  Dense restatement of the DeepSpeed
 * sdd/softmax/dsd pipeline: out = softmax(dh^-0.5 (q k^T + add_mask) + M) v.  Stateless (ctx only carries errors/workspace). */
int bevgen_sparse_self_attention(bevgen_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, const int64_t* d_layout,
                                 const float* d_attn_mask, const float* d_add_mask, int B, int H, int L, int block, float* d_out, void* stream);

/* GPT.forward over the K condition rows (transformer/mingpt_sparse.py:319-391 restricted to rows 0..K-1): fills the KV cache
 * of all layers for B sequences and leaves the hidden state of row K-1 ready for bevgen_ar_logits. */
int bevgen_ar_prefill(bevgen_ctx* ctx, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv, int B, void* stream);

/* ln_f + head on the newest row (mingpt_sparse.py:386-387): d_logits [B, V] = logits of decode step `n_decoded`. */
int bevgen_ar_logits(bevgen_ctx* ctx, float* d_logits, void* stream);

/* Feed the token chosen at the current step (stage2/cond_transformer_multi_view.py:219) and advance one position:
 * embedding of the token at its (camera, latent cell) + one pass over all layers against the KV cache. */
int bevgen_ar_decode_step(bevgen_ctx* ctx, const int64_t* d_token, void* stream);

/* Teacher-forced GPT.forward (transformer/mingpt_sparse.py:319-391) over the K condition rows and the first n_steps image rows in decode order, as ONE batched pass,
 * plus shared_step's token cross-entropy (stage2/cond_transformer_multi_view.py:277-349), asynchronous on `stream`:
 *   d_ids    [B, C*T] int64 camera-major, as GPT.forward receives them: input row K + s is the embedding of d_ids[b, forward_shuffle_idx[s]]; an id equal to
 *            vocab_size is the pad embedding (gpt:328-329 substitutes it for the camera-major last token when sampling = False - the caller does that)
 *   n_steps  1 .. C*T; pad rows K + C*T .. seq_len are never computed (the mask is causal in decode order: no computed row sees them)
 *   d_logits [B, n_steps, V] in DECODE order, or NULL: row s comes from hidden row K - 1 + s and predicts decode position s.  With NULL the logits are produced and
 *            consumed in row chunks and never exist as one buffer
 *   d_target [B, C*T] int64 camera-major or NULL (then d_weight, d_nll and d_loss must be NULL); a target outside [0, V) gives a NaN nll
 *   d_weight [B, C*T] float camera-major or NULL (= 1)
 *   d_nll    [B, n_steps] float in decode order or NULL: logsumexp(logits[b, s, :]) - logits[b, s, d_target[b, forward_shuffle_idx[s]]] (unweighted)
 *   d_loss   1 float or NULL: sum(w * nll) / (B * n_steps), reduced in a fixed order in double precision - two identical calls give the same bits
 * A NaN / inf logit raises BEVGEN_STATUS_NONFINITE_LOGITS as the samplers do.  Precision / weight modes are those of bevgen_ar_prefill.  Afterwards the context is
 * exactly as after bevgen_ar_prefill followed by n_steps calls of bevgen_ar_decode_step with the same tokens (K/V cache rows [0, K + n_steps) in the context's cache
 * dtype, newest hidden row, step counter): bevgen_ar_logits / bevgen_ar_decode_step may follow.  There is no samples_per_layout form of this call: every sequence
 * is scored on its own. */
int bevgen_ar_forward(bevgen_ctx* ctx, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv, int B, const int64_t* d_ids, int n_steps,
                      float* d_logits, const int64_t* d_target, const float* d_weight, float* d_nll, float* d_loss, void* stream);

/* Net2NetTransformer.sample (stage2/cond_transformer_multi_view.py:154-227) with prefill + KV cache:
 *   top_k <= 0 disables the filter; greedy != 0 -> arg-max (sample=False), else inverse-CDF draw with d_noise_u [steps, B];
 *   samples_per_layout: consecutive groups of sequences share cond ids/cameras (B = layouts * samples_per_layout rows are
 *   passed explicitly; the flag only enables prefix reuse);  -> d_out_ids [B, C, T] (camera-major, like the reference's x) */
int bevgen_ar_sample(bevgen_ctx* ctx, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv, int B, int steps,
                     int top_k, float temperature, int greedy, const float* d_noise_u, int samples_per_layout,
                     int64_t* d_out_ids, float* d_step_logits /* [steps,B,V] or NULL */, void* stream);

/* Same with partial decoding (cond_transformer_multi_view.py:161-165, 181-182: the tokens of the cameras in `partial_decoding_idx` are taken from the
 * encoded ground-truth images and their positions are skipped by the sampling loop): d_forced_ids [steps, B] int64 in DECODE order, entry >= 0 = the
 * token to emit at that step (it is still pushed through the stack so that later positions attend to it), < 0 = draw the token.  NULL = bevgen_ar_sample. */
int bevgen_ar_sample_forced(bevgen_ctx* ctx, const int64_t* d_cond_ids, const float* d_I_inv, const float* d_E_inv, int B, int steps,
                            int top_k, float temperature, int greedy, const float* d_noise_u, int samples_per_layout,
                            const int64_t* d_forced_ids, int64_t* d_out_ids, float* d_step_logits, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * stage-1 VQGAN decode                                                                                            */

/* decode_to_img (stage2/cond_transformer_multi_view_muse.py:157-164): get_codebook_entry (stage1/quantize.py:314-329) ->
 * post_quant_conv + Decoder (stage1/vqgan.py:118-121, stage1/model.py:506-537) [-> util.denormalize_tensor, bev_utils/util.py:97-118].
 * The decoder is fully convolutional: the latent grid is lat_h x lat_w = cam_latent_res (16 x 16 for 256 x 256 images, 14 x 25 for nuScenes 224 x 400;
 * 0, 0 = the square grid of ddconfig.resolution), the image (lat_h << (levels-1)) x (lat_w << (levels-1)).
 *   out_mode BEVGEN_VQ_OUT_RAW      d_out fp32 [n, out_ch, H, W], the decoder output
 *            BEVGEN_VQ_OUT_DENORM   d_out fp32 [n, 3, H, W] in [0,1]  (x*std + mean, clamped)
 *            BEVGEN_VQ_OUT_U8       d_out uint8 [n, 3, H, W] = round(255 * denormalised): the storage / wire format of the generated images
 *   d_ids [n, lat_h*lat_w]. */
enum { BEVGEN_VQ_OUT_RAW = 0, BEVGEN_VQ_OUT_DENORM = 1, BEVGEN_VQ_OUT_U8 = 2 };
int bevgen_vq_decode(bevgen_ctx* ctx, const int64_t* d_ids, int n, int lat_h, int lat_w, int out_mode, void* d_out, void* stream);

/* VQModel.encode (stage1/vqgan.py:84-116 with geometric_embedding=False): Encoder (stage1/model.py:405-433) -> quant_conv ->
 * VectorQuantizer2.forward arg-min (stage1/quantize.py:271-312).  d_x [n, in_channels, H, W] fp32 (NCHW, as get_input produces it,
 * muse_lm:166-179; H, W multiples of 2^(levels-1); 0, 0 = ddconfig.resolution squared) -> d_ids [n, (H >> (levels-1)) * (W >> (levels-1))] int64.
 * This is encode_to_c (BEV segmentation -> condition tokens) and encode_to_z (muse_lm:142-155). */
int bevgen_vq_encode(bevgen_ctx* ctx, const float* d_x, int n, int H, int W, int64_t* d_ids, void* stream);

/* bevgen_vq_encode with the two things a stage-1 checkpoint is judged by (bevgen_vq_encode forwards here with NULLs):
 *  - the geometric embedding of a camera VQGAN (stage1/vqgan.py:87-112, geometric_embedding=True): a context loaded with img_embed.weight and cam_embed.weight
 *    ([z_channels, 4, 1, 1], no bias; exactly one of the two, or another shape, fails bevgen_finalize) adds normalize(Wimg d - Wcam c) (d = E_inv [I_inv pix; 1],
 *    c = E_inv[:, 3], norm + 1e-7) to the encoder output in front of quant_conv (and of quant_conv's range-safe site, whose exponent is chosen from the sum).
 *    d_I_inv [n, 3, 3], d_E_inv [n, 4, 4] per image, d_plane [3, h*w] (x = linspace(0,1,w) image_width, y = linspace(0,1,h) image_height, 1).  Such a context REQUIRES
 *    the three pointers and a context without the two weights REFUSES them (BEVGEN_ERR_INVALID): the embedding is never skipped silently.
 *  - the quantizer's error: d_row_err [n, h*w] (or NULL) = |codebook[id] - z|^2 per latent row as direct fp32 differences, and d_loss (one float, or NULL; needs
 *    d_row_err, which belongs to the caller because the workspace is reset per pass of 48 images) = (1 + beta) / (n h w embed_dim) * sum(row_err), the forward value
 *    of VectorQuantizer2's loss in both its legacy and corrected form (stage1/quantize.py:290-295), accumulated in double in a fixed order once over all rows of the call
 *    (bit-reproducible).  NaN / inf latents propagate into row_err and the loss; BEVGEN_STATUS_NONFINITE_LATENTS is raised by the arg-min as before. */
int bevgen_vq_encode_ex(bevgen_ctx* ctx, const float* d_x, int n, int H, int W, const float* d_I_inv /* or NULL */, const float* d_E_inv /* or NULL */,
                        const float* d_plane /* or NULL */, float beta, int64_t* d_ids, float* d_row_err /* or NULL */, float* d_loss /* or NULL */, void* stream);

/* VQModel.decode(quant) (stage1/vqgan.py:118-121) for already looked-up latents: d_zq [n, embed_dim, lat_h, lat_w] (NCHW, like the reference). */
int bevgen_vq_decode_latents(bevgen_ctx* ctx, const float* d_zq, int n, int lat_h, int lat_w, int out_mode, void* d_out, void* stream);

/* vq_range = 1: the exponents the most recent bevgen_vq_decode / bevgen_vq_decode_latents / bevgen_vq_encode call on this context chose, in site order (per pass of up to
 * 48 images; decode: conv_in, then every nin_shortcut and upsample convolution in execution order; encode: conv_in, then every nin_shortcut and downsample convolution in
 * execution order, then quant_conv), written to the HOST array h_out[cap]; *count = their number (may exceed cap; 0 with vq_range = 0 or before the first call).
 * Synchronises the device. */
int bevgen_vq_range_exponents(bevgen_ctx* ctx, int32_t* h_out, int cap, int* count);

/* ---------------------------------------------------------------------------------------------------------------
 * Operator-level entry points (parity tests and roofline measurements call the kernels through these)             */
int bevgen_op_gemm(bevgen_ctx* ctx, const float* d_a, const float* d_w, const float* d_bias, const float* d_residual, float* d_c,
                   int M, int N, int K, int act_gelu, int skinny, void* stream);            /* C = A W^T (+bias)(gelu)(+res); skinny: 0 tiled fp32, 1 M <= 64, 2-4 split-precision
                                                                                               kernels (tests / probes), 5 = 3 with the k range split over three slices, 6 = 3 in its stream-K form;
                                                                                               single-product (BEVGEN_PRECISION_F16X1) forms, w's low plane ignored: 7 = 4 computing
                                                                                               f16(A) f16(W)^T, 8 = 7 with the k range in three slices, 9 = 2 single-product */
/* Route M's projections with their fused epilogues (gemm_split_glds.hip EPI_MUSE_Q / _KV / _QKV), operands built the way bevgen_finalize and muse.cpp build them
 * (f16x3 contexts).  kind 0 = to_q, 1 = to_kv, 2 = q | k | v over d_a [B T, K] and d_w [64 H (kind + 1), K]; d_ln_gamma non-NULL: the A planes come from the LayerNorm
 * kernel (gamma only) instead of a plain split of d_a.  Outputs are caller-owned f16 planes, never cleared here: Qh / Ql [B, H, T, 64] (kind 0, 2), Kh / Kl [B, H, ld, 64]
 * with key row 1 + token and the prepared null key at row 0, VTh / VTl [B, H, 64, ld] (kind 1, 2; ld >= T + 1).  block: 0 = the launcher's choice, 4 = 256-row blocks.
 * weights: 0 = the split planes of d_w, 1 = d_w rounded to f16 (two products), 2 = additionally the single-product form.  form 0 = the fused epilogue; 1 (kind 0, 1) =
 * un-fused as the small-batch path runs it: the plain projection (k range in `ksplit` slices, added in slice order) and the preparation kernel - which also zero-fills
 * the value columns (T, ld).  Unsupported arguments return BEVGEN_ERR_INVALID without a launch. */
int bevgen_op_muse_qkv(bevgen_ctx* ctx, int kind, const float* d_a, const float* d_w, const float* d_ln_gamma /* or NULL */, const float* d_q_scale, const float* d_k_scale,
                       const float* d_null_kv /* [2, H, 64] */, int B, int T, int H, int K, int ld, float post, int block, int weights, int form, int ksplit, void* d_qh, void* d_ql,
                       void* d_kh, void* d_kl, void* d_vth, void* d_vtl, void* stream);
/* Route M's feed-forward behind its first LayerNorm: y [M, Dout] = LN_gamma3(gate * gelu(a)) W4^T + residual with (a | gate) = x W1^T, Fpad = round_up(F, 64), x [M, D],
 * w1 [2 F, D], w4 [Dout, F]; D % 32 == 0, Dout % 32 == 0.  level 0: GEGLU epilogue to fp32 d_h [M, Fpad], the LayerNorm kernel, the plain down-projection; 1: the
 * up-projection writes the raw planes d_g_planes [M][Fpad / 32][hi 32 | lo 32] and the group sums d_g_sums [Fpad / 32][M][2] instead, the down-projection consumes them
 * (W4 o gamma3); 2: the down-projection also writes the planes d_y_planes [M][Dout / 32][64] and sums d_y_sums [Dout / 32][M][2] of its own output rows.  merge 0: the
 * statistics kernel ((mean, rstd) in d_rowstat [M][2]), 1: the consuming tiles merge the group sums.  block as above, on both projections.  Every output may be NULL
 * (scratch is used); none is cleared; a level never writes the outputs of another level. */
int bevgen_op_muse_ff(bevgen_ctx* ctx, const float* d_x, const float* d_w1, const float* d_gamma3, const float* d_w4, const float* d_residual, int M, int D, int F, int Dout,
                      int level, int merge, int block, float* d_h, void* d_g_planes, float* d_g_sums, float* d_rowstat, void* d_y_planes, float* d_y_sums, float* d_y,
                      void* stream);
/* LayerNorm (gamma, optional beta; eps 1e-5) of d_x [rows, ldx] over D columns written as the interleaved plane image d_planes [rows][ldy / 32][hi 32 | lo 32] (columns
 * [D, ldy) zero); geglu != 0: d_x is [rows, 2 D] = (a | gate), row stride ldx, and the rows normalised are gate * gelu(a) (no beta). */
int bevgen_op_layernorm_planes(bevgen_ctx* ctx, const float* d_x, int ldx, const float* d_gamma, const float* d_beta /* or NULL */, void* d_planes, int ldy, int rows, int D,
                               int geglu, void* stream);
/* The null-condition pass's stand-in for a cross-attention block and the LayerNorm behind it: d_x[row, 0:D] += d_r[0:D] (written back), then LayerNorm (gamma, eps 1e-5) of
 * the updated row into d_y - fp32 rows [rows, ldy] (planes == 0) or the plane image of bevgen_op_layernorm_planes (planes != 0, ldy % 32 == 0); columns [D, ldy) zero.
 * The bits of an fp32 add followed by bevgen_op_layernorm / bevgen_op_layernorm_planes.  D % 4 == 0, 16-byte aligned pointers. */
int bevgen_op_add_row_layernorm(bevgen_ctx* ctx, float* d_x, int ldx, const float* d_r, const float* d_gamma, void* d_y, int ldy, int rows, int D, int planes, void* stream);
/* Classifier-free guidance on logits: d_cond[row, 0:V] = d_null + (d_cond - d_null) * cond_scale in place (fp32 sub, mul, add, each rounded once); row strides ldc / ldn,
 * columns [V, ldc) untouched. */
int bevgen_op_cfg_combine(bevgen_ctx* ctx, float* d_cond, int ldc, const float* d_null, int ldn, long rows, int V, float cond_scale, void* stream);
/* Decode-step projection (decode_fused.hip): C = act(LayerNorm?(A) W^T + bias) for M <= 64 rows; d_ln_w NULL = no LayerNorm; ksplit > 1 (no LayerNorm, no bias / act):
 * d_c receives the split-K partial sums [ksplit, M, N] that the consumer adds; ksplit 0 = the library's choice for (N, K), returned through *ksplit_out if non-NULL;
 * ksplit -1 (LayerNorm with beta and bias): one K slice, the LayerNorm folded into the product the way the decode step launches ln2 + MLP-up.
 * On a context created with decode_weight_dtype = BEVGEN_W_I8 the operator quantises d_w and runs the int8 image (the result is that of the dequantised matrix). */
int bevgen_op_ln_gemm(bevgen_ctx* ctx, const float* d_a, const float* d_ln_w, const float* d_ln_b, float eps, const float* d_w, const float* d_bias, float* d_c,
                      int M, int N, int K, int act_gelu, int ksplit, int* ksplit_out, void* stream);
/* The row quantiser of BEVGEN_W_I8 alone: d_w [N, K] fp32 -> d_codes [N, K] int8 row-major, d_scales [N], and (d_dequant non-NULL) the values code * scale [N, K]. */
int bevgen_op_quantize_rows_i8(bevgen_ctx* ctx, const float* d_w, int N, int K, void* d_codes, float* d_scales, float* d_dequant /* or NULL */, void* stream);
/* Both MLP projections of a Route-A decode layer in one launch (decode_fused.hip ar_mlp_fused_kernel; Block.forward's mlp(ln2(x)), transformer/mingpt_sparse.py:232-253):
 * d_out [M, D] = Linear2(GELU(Linear1(LayerNorm(d_x)))) WITHOUT the residual, M <= 64, D = 1024; w_f16 = 1: the matrices are rounded to fp16 first (decode_weights = f16);
 * w_f16 = 2: quantised to int8 codes with row scales (decode_weights = i8: the result is that of the dequantised matrices).
 * Returns BEVGEN_ERR_INVALID where the launch is not supported (shape, or a device with fewer CUs than its 4 D / 16 workgroups). */
int bevgen_op_mlp_fused(bevgen_ctx* ctx, const float* d_x, const float* d_ln_w, const float* d_ln_b, float eps, const float* d_w1 /*[4D, D]*/, const float* d_b1,
                        const float* d_w2 /*[D, 4D]*/, const float* d_b2, int w_f16, float* d_out, int M, int D, void* stream);
/* d_out[i] = the uniform the MaskGit samplers draw for element i of noise stream `stream_id` (0 gumbel, 1 critic) at iteration `iter` under `seed`. */
int bevgen_op_philox_uniform(bevgen_ctx* ctx, unsigned long long seed, unsigned iter, unsigned stream_id, int V /* vocabulary size: row layout of stream 0 */, long n,
                             float* d_out, void* stream);
/* Token samplers and scorers (sampler.hip), one entry per kernel; every pointer marked "or NULL" stays optional.  Non-finite logits / scores raise BEVGEN_STATUS_NONFINITE_LOGITS.
 * remask: the n_mask highest scores of each row of d_ids [rows, T] (ties: lower index first) become mask_id, then d_init_ids entries != mask_id are re-imposed; T <= 16384. */
int bevgen_op_remask(bevgen_ctx* ctx, int64_t* d_ids, const float* d_scores, const int64_t* d_init_ids /* or NULL */, int rows, int T, int n_mask, int64_t mask_id, void* stream);
/* maskgit_pick: d_ids [rows] == mask_id are replaced by argmax(topk_k(logits) / max(temperature, 1e-10) + gumbel(u)); u = d_gumbel_u [rows, V], else Philox(seed, iter) when
 * seed != 0, else none (plain arg-max, lowest index on ties).  V <= 1024, 1 <= k.  conf_mode 1 / 2: d_conf_scores [rows] = 1 - softmax(logits)[pred] at masked positions
 * (-1e5 elsewhere) / at every position. */
int bevgen_op_maskgit_pick(bevgen_ctx* ctx, int64_t* d_ids, const float* d_logits, int ldl, const float* d_gumbel_u /* or NULL */, int rows, int V, int k, float temperature,
                           int64_t mask_id, unsigned long long seed, unsigned iter, float* d_conf_scores /* or NULL */, int conf_mode, void* stream);
/* critic_scores: d_scores[r] = d_embed[r, :D] . d_w + d_b[0] + ((u[r] - 0.5) * noise_scale) * frac; u = d_u, else Philox stream 1 of (seed, iter) when seed != 0, else 0.5.
 * D % 4 == 0, lde % 4 == 0, d_embed and d_w 16-byte aligned. */
int bevgen_op_critic_scores(bevgen_ctx* ctx, const float* d_embed, int lde, const float* d_w, const float* d_b, const float* d_u /* or NULL */, float noise_scale, float frac,
                            unsigned long long seed, unsigned iter, float* d_scores, int rows, int D, void* stream);
/* ar_pick: d_out[r] = token of row r of d_logits [rows, ldl]: logits / temperature, top_k (0 = off, ties kept), arg-max (d_u NULL) or inverse-CDF draw with
 * d_u [steps, rows]; d_step (device int, or NULL = step 0) selects the row of d_u / d_forced [steps, rows] (entries >= 0 are emitted verbatim).  Optional tail (d_out_all
 * non-NULL; needs d_step): d_out_all[r, d_fwd_idx[step]] = token, and with d_x non-NULL d_x[r, :D] = (d_tok_emb[min(token, vocab_rows - 1)] + d_img_embed[r, fwd_idx[step]])
 * + d_pos_emb[fwd_idx[step]] with d_img_embed [rows, C * T, D] or NULL; D % 4 == 0. */
int bevgen_op_ar_pick(bevgen_ctx* ctx, const float* d_logits, int ldl, const float* d_u /* or NULL */, const int* d_step /* or NULL */, const int64_t* d_forced /* or NULL */,
                      int64_t* d_out, int rows, int V, int top_k, float temperature, int64_t* d_out_all /* or NULL */, const int64_t* d_fwd_idx, int N, const float* d_tok_emb,
                      const float* d_img_embed /* or NULL */, const float* d_pos_emb, float* d_x /* or NULL */, int C, int T, int D, int vocab_rows, void* stream);
/* ar_score_rows: rows [s0, s0 + rows) in decode order of sequence b: d_nll[r] (or NULL) = logsumexp(d_logits[r, :V]) - d_logits[r, t], t = d_target[b, d_fwd_idx[s0 + r]]
 * (outside [0, V): NaN), d_wnll[r] = d_weight[b, d_fwd_idx[s0 + r]] (NULL = 1) * nll; d_target NULL: only the finiteness check of the rows. */
int bevgen_op_ar_score_rows(bevgen_ctx* ctx, const float* d_logits, int ldl, const int64_t* d_target /* [B, N] or NULL */, const float* d_weight /* or NULL */,
                            const int64_t* d_fwd_idx, int b, int s0, int rows, int N, int V, float* d_nll /* or NULL */, float* d_wnll, void* stream);
/* d_out[0] = sum(d_x[0..n)) / n, accumulated in double in a fixed order: two calls give the same bits. */
int bevgen_op_mean_fixed_order(bevgen_ctx* ctx, const float* d_x, long n, float* d_out, void* stream);
int bevgen_op_layernorm(bevgen_ctx* ctx, const float* d_x, const float* d_gamma, const float* d_beta, float* d_y, int rows, int D, float eps, void* stream);
int bevgen_op_geglu_layernorm(bevgen_ctx* ctx, const float* d_h, const float* d_gamma, float* d_y, int rows, int F, int ldy, void* stream);
int bevgen_op_attention(bevgen_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, const float* d_bias, int ldbias,
                        int B, int H, int Nq, int Nk_pad, float scale, float* d_out, void* stream);   /* q [B,H,Nq,64], k/v [B,H,Nk_pad,64] */
/* The same with the key tiles of the split-precision kernel cut into `key_splits` ranges (1..8; needs Nk_pad / 32 >= key_splits) merged by a combine kernel - the form
 * the Route M model path picks for its self-attention at one scene per call (muse.cpp pick_attn_ksplit); fp32-precision contexts ignore key_splits. */
int bevgen_op_attention_ex(bevgen_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, const float* d_bias, int ldbias,
                           int B, int H, int Nq, int Nk_pad, float scale, int key_splits, float* d_out, void* stream);
/* Route M's split-precision attention kernel (attention_split.hip) launched the way muse.cpp launches it (attn_args, self_attention_split / cross_attention_split) on
 * caller-owned f16 planes - what bevgen_op_muse_qkv writes: Qh / Ql [B, H, Nq, 64] with the score scale (x log2 e) folded in, Kh / Kl [B / kv_group, H, Nk_pad, 64],
 * VTh / VTl [B / kv_group, H, 64, Nk_pad]; batch element b reads K / V slot b / kv_group (kv_group >= 1 divides B).  d_bias [Nq, ldbias] (or NULL; ldbias % 4 == 0,
 * ldbias >= Nk_pad) is the matrix the context hands to the kernel's bias packer: in the base-2 domain (already multiplied by log2 e), -1e30 = hidden, every column the
 * kernel must not see (from the last key on) hidden; it is not rescaled here, only packed into scratch.  Rows / columns of K / V^T behind the last visible key may hold
 * any finite values.  key_splits 1..8 and <= Nk_pad / 32: the key tiles in that many ranges and the combine kernel.  Exactly one output: d_out fp32 [B, Nq, 64 H], or
 * d_out_planes, the f16 image [B Nq][64 H / 32][hi 32 | lo 32] the to_out projection reads - (hi, lo) of the same fp32 values, bit for bit; an output value outside the
 * f16 range raises BEVGEN_STATUS_F16_RANGE in the plane form.  Nothing is cleared or pre-filled; every pointer 16-byte aligned.  f16x3 contexts only; unsupported
 * arguments return BEVGEN_ERR_INVALID without a launch. */
int bevgen_op_muse_attention(bevgen_ctx* ctx, const void* d_qh, const void* d_ql, const void* d_kh, const void* d_kl, const void* d_vth, const void* d_vtl,
                             const float* d_bias /* or NULL */, int ldbias, int B, int H, int Nq, int Nk_pad, int kv_group, int key_splits, float* d_out /* or NULL */,
                             void* d_out_planes /* or NULL */, void* stream);
int bevgen_op_decode_attention(bevgen_ctx* ctx, const float* d_q, const void* d_kcache, const void* d_vcache, int kv_dtype,
                               const float* d_bias, int ldbias, const uint8_t* d_keep, int ldkeep, long keep_head_stride,
                               int B, int H, int n, int Lmax, float scale, float* d_out, void* stream);
/* Attention half of one Route A decode layer as the fused path runs it (decode_fused.hip ar_attn_fused_kernel; Block.forward mingpt_sparse.py:240-253 +
 * SparseSelfAttention.forward sparse_self_attention.py:150-176) for ONE new row per sequence:
 *   row = d_x[b] (+ d_rbias + sum of the ns split-K partials d_partial [ns, B, D]) -> xn = ln1(row) -> q | k | v = Wqkv xn + bqkv (fused [3D, D]) ->
 *   k, v written to cache row n-1 -> softmax(dh^-0.5 (q k^T + d_bias[n-1, :]) + mask) v over keys 0..n-1 -> d_out[b] = xn + attention.
 * Visibility as the reference defines it: d_attn_mask [L, L] fp32 (0 = hidden) AND d_layout int64 [H, L/block, L/block] (0 = block absent, never read);
 * either may be NULL.  G > 1: consecutive groups of G sequences share their first `prefix` keys, read from the group's first cache slot.
 * kv_dtype 0 fp32 / 1 fp16 cache [B, H, Lmax, 64]; w_f16 = 1: the projection weights are rounded to fp16 and streamed as 2-byte values;
 * w_f16 = 2: quantised to int8 codes with one scale per row (BEVGEN_W_I8) and streamed as 1-byte values.
 * split = 0: the fused kernel as the sampling path launches it (G = 1: leading K/V steps of the key walk staged in LDS by LDS-DMA); split = -1: without staged pieces.
 * split > 0: the BEVGEN_DECODE_SPLIT form of the same computation (LayerNorm + QKV projection kernel, then the attention-only kernel); split = k > 1: with the
 * key walk of every (sequence, head) cut into k ranges on k workgroups and merged by the combine kernel (what one- and two-sequence calls run; G = 1). */
int bevgen_op_ar_attn_fused(bevgen_ctx* ctx, const float* d_x, const float* d_partial, int ns, const float* d_rbias, const float* d_ln_w, const float* d_ln_b,
                            const float* d_wqkv, const float* d_bqkv, int w_f16, void* d_kcache, void* d_vcache, int kv_dtype, const float* d_bias, int ldbias,
                            const float* d_attn_mask, const int64_t* d_layout, int block, int B, int G, int H, int n, int Lmax, int prefix, int split, float* d_out, void* stream);
/* upsample2x: bit 0 = nearest-2x upsample of the input fused into the gather; bit 1 = run the LDS-DMA kernel on (hi, lo) operand planes split inside the call (Cin % 32 == 0;
 * the decoder reaches that kernel with planes its GroupNorm wrote); bit 2 (with bit 1) = its general variant also where the stride-1 variant applies. */
int bevgen_op_conv3x3(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_w_ohwi, const float* d_bias, const float* d_residual,
                      float* d_y_nhwc, int n, int H, int W, int Cin, int Cout, int upsample2x, void* stream);
int bevgen_op_groupnorm(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_gamma, const float* d_beta, float* d_y, int n, int hw, int C,
                        int swish, void* stream);
/* The range-safe operand preparation on its own (vq_range = 1): d_x [n, hw, C] fp32 (C % 32 == 0) -> d_exp[0] = e (the rule at bevgen_cfg.vq_range) and
 * d_planes = the interleaved (hi, lo) f16 plane image [n * hw][C / 32][2][32] of x 2^-e (x = (hi + lo 2^-11) 2^e).  NaN / inf in d_x raise BEVGEN_STATUS_F16_RANGE. */
int bevgen_op_range_split(bevgen_ctx* ctx, const float* d_x, int n, int hw, int C, void* d_planes, int32_t* d_exp, void* stream);
/* Building blocks of the stage-1 VQGAN at shapes of their own (vqdec.cpp; the model reaches them only through bevgen_vq_encode / bevgen_vq_decode).  Activations are NHWC fp32,
 * convolution weights arrive as the checkpoint stores them ([Cout][Cin][kh][kw]) and are re-laid out (and, with precision = F16X3, split) inside the call.
 * conv3x3_down: the encoder's Downsample, F.pad(x, (0,1,0,1)) + 3x3 convolution with stride 2 and padding 0: d_y [n, H/2, W/2, Cout]; H, W even, Cin % 32 == 0. */
int bevgen_op_conv3x3_down(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_w_oihw, const float* d_bias /* or NULL */, float* d_y_nhwc, int n, int H, int W, int Cin,
                           int Cout, void* stream);
/* vq_attn_block: AttnBlock.forward (stage1/model.py:168-192): d_y = x + proj_out(softmax(q k^T C^-0.5) v) with q, k, v = 1x1 convolutions [C][C] of GroupNorm(x); C % 32 == 0;
 * d_y must not alias d_x. */
int bevgen_op_vq_attn_block(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_norm_w, const float* d_norm_b, const float* d_wq, const float* d_bq, const float* d_wk,
                            const float* d_bk, const float* d_wv, const float* d_bv, const float* d_wp, const float* d_bp, float* d_y_nhwc, int n, int h, int w, int C, void* stream);
/* vq_out_tail: the decoder's last operators, conv_out(swish(norm_out(x))) with d_w [3][C][3][3], then out_mode 0: raw fp32 NCHW [n, 3, H, W]; 1: x std + mean clamped to [0, 1];
 * 2: round(255 x) of that as uint8 (d_out then points to uint8).  three_kernels = 0: the fused kernel; 1: GroupNorm-apply, implicit-GEMM convolution and layout kernel.
 * A NaN / inf pixel raises BEVGEN_STATUS_NONFINITE_PIXELS. */
int bevgen_op_vq_out_tail(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_norm_w, const float* d_norm_b, const float* d_w_oihw, const float* d_bias /* or NULL */,
                          const float* d_mean /* [3], or NULL with out_mode 0 */, const float* d_std, int out_mode, int three_kernels, void* d_out, int n, int H, int W, int C,
                          void* stream);
/* vq_out_tail_ex: vq_out_tail with `cout` output channels (d_w [cout][C][3][3], d_bias [cout], d_out [n, cout, H, W]); bevgen_op_vq_out_tail is this with cout = 3.
 * cout 3 and 7 (the BEV segmentation decoder, out_ch 7) have the fused kernel, any other count runs the three-kernel form whatever three_kernels says; the pixel staging
 * of that form is max(4, cout) floats per pixel.  out_mode 1 / 2 need cout == 3. */
int bevgen_op_vq_out_tail_ex(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_norm_w, const float* d_norm_b, const float* d_w_oihw, const float* d_bias /* or NULL */,
                             const float* d_mean /* [3], or NULL with out_mode 0 */, const float* d_std, int out_mode, int three_kernels, void* d_out, int n, int H, int W, int C,
                             int cout, void* stream);
/* bce_logits: F.binary_cross_entropy_with_logits(logits, target) with mean reduction (losses/segmentation.py:7,17): per element max(x, 0) - x t + log1p(exp(-|x|)) in fp32
 * (|x| up to 1e4 and beyond without overflow, soft targets allowed, NaN propagates), summed in double in a fixed order (two calls give the same bits), times 1 / count in
 * double, rounded to float once -> d_out[0].  d_qloss non-NULL: also d_out[1] = d_out[0] + codebook_weight * d_qloss[0] in fp32, the product rounded and then the sum, as
 * torch evaluates BCELossWithQuant's `bce_loss + self.codebook_weight*qloss`; d_qloss NULL leaves d_out[1] untouched.  fp32 in every precision mode. */
int bevgen_op_bce_logits(bevgen_ctx* ctx, const float* d_logits, const float* d_target, long count, const float* d_qloss /* or NULL */, float codebook_weight,
                         float* d_out /* [2]: bce, total */, void* stream);
/* seg_colorize: VQModel.to_rgb's random projection (stage1/vqgan.py:207-212): d_rgb [n, 3, H, W] = (y - min y) / (max y - min y) with y_k = sum_c d_colorize[k][c] v_c in
 * channel order (fmaf), d_x [n, C, H, W] (NCHW), C <= 32; d_rgb must not alias d_x.  threshold = 0: v = x.  threshold = 1: v = (x > 0 ? 1 : 0), which stands for the
 * reference's torch.round(torch.sigmoid(x)) (vqgan:253-256): the two agree (ties to even) everywhere except 0 < x <~ 6e-8, where fp32 sigmoid rounds to 0.5 and the
 * reference therefore gives 0 (on the CPU, torch.round(torch.sigmoid(1e-9)) = 0).  round(sigmoid(.)) of a logit near 0 is a step: no bound on the logit carries over.
 * min and max are taken over the WHOLE tensor (all n images), on the device, through an order-preserving integer encoding and atomicMin / atomicMax: one moved extreme
 * rescales every pixel, the order of the atomics does not matter, so the result is bit-reproducible.  IEEE fp32 subtraction and a true division; max == min gives 0 / 0
 * as in the reference; a NaN makes every pixel NaN.  (The reference's model decodes z + (z_q - z), this library z_q: at most an ulp of z apart in front of the decoder.) */
int bevgen_op_seg_colorize(bevgen_ctx* ctx, const float* d_x, const float* d_colorize /* [3, C] */, int threshold, float* d_rgb, int n, int C, int H, int W, void* stream);
/* Image metrics on planes that are already on the device (the PSNR / SSIM step of scripts/metrics_eval.py:115-132).  d_a, d_b [n, C, H, W], contiguous, of ONE dtype:
 * BEVGEN_DTYPE_F32 (values nominally in [0, 1]) or BEVGEN_DTYPE_U8 (0 .. 255, meaning v / 255).  fp32 / fp64 kernels in every precision mode, on any context.  Sums are
 * taken in double in a fixed order without floating atomics: two calls give the same bits and image i's result does not depend on the rest of the batch.  A NaN pixel
 * gives a NaN for its image only and raises no status bit.  d_work: bevgen_metrics_workspace_bytes(op, ...) bytes of caller memory (8-byte aligned), not kept between calls.
 * Refused with BEVGEN_ERR_INVALID before any launch: another dtype, an empty batch, C H W >= 2^31, and for ssim an even kernel_size, kernel_size > 33, H or W < kernel_size.
 * image_sqerr: d_sse[i] = sum over image i of (a - b)^2 - fp32: the difference and the square one fp32 operation each, the sum in double; uint8: the exact integer sum of
 * (a - b)^2 in units of 1 / 255^2 - and d_minmax[0] = min(d_minmax[0], min b), d_minmax[1] = max(d_minmax[1], max b) (uint8: of v / 255): the caller initialises d_minmax to
 * (+inf, -inf) once and every call merges into it, which is what PeakSignalNoiseRatio(data_range=None) tracks. */
int bevgen_op_image_sqerr(bevgen_ctx* ctx, const void* d_a, const void* d_b, int dtype, int n, int C, int H, int W, double* d_sse /* [n] */, float* d_minmax /* [2] */,
                          void* d_work, void* stream);
/* ssim: d_sums[i] = sum over the map [C, H - k + 1, W - k + 1] of image i of ((2 mx my + c1)(2 sxy + c2)) / ((mx^2 + my^2 + c1)(sxx + syy + c2)), c1 = (k1 R)^2, c2 = (k2 R)^2,
 * no clamp; the moments are taken with the normalised Gaussian window g g^T, g_j = exp(-d_j^2 / 2 sigma^2), over the VALID windows only (equal to reflect-padding by
 * (k - 1) / 2, filtering and cropping the pad).  fp32 per pixel; the second moments are accumulated about a per-tile shift (the target's pixel in the middle of the tile's
 * halo), which is added back to the means only: E[x^2] - mu^2 then cancels on the local contrast, not on the level.  d_map (or NULL): the fp32 map [n, C, H-k+1, W-k+1]. */
int bevgen_op_ssim(bevgen_ctx* ctx, const void* d_a, const void* d_b, int dtype, int n, int C, int H, int W, int kernel_size, double sigma, double data_range, double k1,
                   double k2, double* d_sums /* [n] */, float* d_map /* or NULL */, void* d_work, void* stream);
/* LPIPS with the VGG16 feature stack (the reference's modules/losses/lpips.py:41-54, 57-64, 116-122; the "PSIM/LPIPS" line of scripts/metrics_eval.py), eval mode.
 *   x' = (x - shift) / scale per channel (after 2 x - 1 with normalize != 0), fp32, one operation each; uint8 pixels are v / 255 (one fp32 division)
 *   VGG16 features[0:30]: thirteen 3x3 convolutions (stride 1, zero padding 1) with bias and ReLU, MaxPool2d(2, 2) (odd sizes floor) in front of convolutions 2, 4, 7, 10;
 *   taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (64, 128, 256, 512, 512 channels)
 *   d_k = mean_{h,w} sum_c lin_k[c] (fa^ - fb^)^2, f^ = f / (sqrt(sum_c f^2) + 1e-10): fp32 per element in that order, the spatial sum in double in a fixed order, no
 *   atomics (two calls give the same bits; image i's value does not depend on the batch); LPIPS = (((d_0 + d_1) + d_2) + d_3) + d_4 per image pair.
 * A context of precision FP32 runs the convolutions on the exact-fp32 kernel, every other precision on the three-product f16 kernel ((hi, lo) operand planes: a NaN or
 * |v| >= 65520 activation or weight raises BEVGEN_STATUS_F16_RANGE).  Parity with the `lpips` / torchmetrics packages is unpinned (neither is part of the reference tree);
 * torchmetrics' host-side range check of the inputs is not reproduced.
 * bevgen_lpips_prepare: the thirteen weights d_w[l] [Cout][Cin][3][3] and biases d_bias[l] [Cout] (h_w, h_bias: HOST arrays of 13 device pointers, in network order),
 * h_lin: 5 device pointers to the non-negative lin vectors [C_k], d_shift / d_scale [3] -> d_prepared (bevgen_lpips_prepared_bytes(precision) bytes of caller memory,
 * 256-byte aligned): weights re-laid to [Cout][3][3][Cin] (the first layer's Cin padded to 32 with zeros) and, on a split-precision context, their (hi, lo) planes.  Once per
 * checkpoint; d_prepared belongs to the precision of the context that wrote it.
 * bevgen_lpips: d_a, d_b [n, 3, H, W] contiguous, of ONE dtype (BEVGEN_DTYPE_F32 or _U8) -> d_out [n] and, with d_layers non-NULL, the five d_k per pair [n, 5].  Pairs run
 * in chunks whose size depends on (H, W, precision) only, a and b of a chunk as one batch.  d_work: bevgen_lpips_workspace_bytes(n, H, W, precision) bytes, 256-byte aligned,
 * not kept between calls.  Refused with BEVGEN_ERR_INVALID before any launch: H or W < 16 (relu5_3 would have no pixel), n < 1, H W > 2^21, another dtype. */
int bevgen_lpips_prepare(bevgen_ctx* ctx, const float* const* h_w, const float* const* h_bias, const float* const* h_lin, const float* d_shift, const float* d_scale,
                         void* d_prepared, void* stream);
int bevgen_lpips(bevgen_ctx* ctx, const void* d_prepared, const void* d_a, const void* d_b, int dtype, int n, int H, int W, int normalize, double* d_out /* [n] */,
                 double* d_layers /* [n, 5] or NULL */, void* d_work, void* stream);
/* Its building blocks on caller tensors.  conv3x3_act: bevgen_op_conv3x3 with an activation in the epilogue, act 0 = none, 1 = ReLU: max(0, acc + bias) (+ residual), a NaN
 * stays; no separate pass over the tensor.
 * maxpool2x2: d_x [n, H, W, C] NHWC -> d_y [n, H / 2, W / 2, C] (MaxPool2d(2, 2): odd sizes floor, a NaN stays) and, with d_planes non-NULL, the (hi, lo) f16 plane image
 * [n (H / 2) (W / 2)][C / 32][2][32] of the pooled tensor in the same pass, bit for bit what bevgen_op_range_split writes for it at exponent 0 (out-of-range values raise
 * BEVGEN_STATUS_F16_RANGE).  C % 32 == 0; H, W >= 2.
 * lpips_tap: d_out[i] = d_k of the feature pair d_fa[i], d_fb[i] [pixels, C] with the weights d_w [C]; C = 64, 128, 256 or 512. */
int bevgen_op_conv3x3_act(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_w_ohwi, const float* d_bias, const float* d_residual,
                          float* d_y_nhwc, int n, int H, int W, int Cin, int Cout, int upsample2x, int act, void* stream);
int bevgen_op_maxpool2x2(bevgen_ctx* ctx, const float* d_x_nhwc, float* d_y_nhwc, void* d_planes /* or NULL */, int n, int H, int W, int C, void* stream);
int bevgen_op_lpips_tap(bevgen_ctx* ctx, const float* d_fa, const float* d_fb, const float* d_w, int n, int pixels, int C, double* d_out /* [n] */, void* stream);
/* vq_quantize: VectorQuantizer2.forward's arg-min, d_ids[r] = argmin_j (|z_r|^2 + |e_j|^2) - 2 z_r . e_j with the lowest index on ties; d_z [rows, D], d_codebook [n_e, D],
 * D % 32 == 0; d_zz [rows] / d_ee [n_e] (or NULL) receive the squared norms.  A row without a finite distance gets id 0 and raises BEVGEN_STATUS_NONFINITE_LATENTS. */
int bevgen_op_vq_quantize(bevgen_ctx* ctx, const float* d_z, const float* d_codebook, int64_t* d_ids, float* d_zz /* or NULL */, float* d_ee /* or NULL */, long rows, int n_e,
                          int D, void* stream);
/* vq_geo_embed: the geometric embedding of bevgen_vq_encode_ex on a caller tensor, in place: d_h [n, T, D] += normalize(Wimg d - Wcam c) per latent pixel; d_I_inv [n, 3, 3],
 * d_E_inv [n, 4, 4], d_plane [3, T], d_wimg / d_wcam [D, 4]; D % 32 == 0, D <= 1024.  fp32 in every precision mode.  One wave per pixel: h is read and written once. */
int bevgen_op_vq_geo_embed(bevgen_ctx* ctx, float* d_h, const float* d_I_inv, const float* d_E_inv, const float* d_plane, const float* d_wimg, const float* d_wcam, int n, int T,
                           int D, void* stream);
/* vq_quant_error: d_row_err[r] = sum_c (d_codebook[d_ids[r]][c] - d_z[r][c])^2 (direct fp32 differences, ids clamped into [0, n_e)) and, with d_loss non-NULL,
 * d_loss[0] = (1 + beta) / (rows D) * sum(row_err) in double, fixed order.  D % 32 == 0.  Reads z once and the gathered codebook rows.  A NaN in z gives a NaN row_err
 * of that row only. */
int bevgen_op_vq_quant_error(bevgen_ctx* ctx, const float* d_z, const float* d_codebook, const int64_t* d_ids, float beta, float* d_row_err, float* d_loss /* or NULL */,
                             long rows, int n_e, int D, void* stream);
/* conv3x3_gn_stats (precision = F16X3 contexts): the LDS-DMA 3x3 convolution (stride 1, padding 1) on (hi, lo) planes of d_x whose epilogue leaves the GroupNorm(32) partial sums
 * of its output, d_part [n H W / 32][Cout / 4][2] fp32 (sum, sum of squares), and the statistics made of them, d_stats [n, 32, 2] = (mean, rstd) at eps 1e-6.
 * range_route != 0: the form of the range-safe mode instead (convolution without the bias, then the bias + statistics pass at exponent 0).  H W % 256 == 0 and
 * Cout % 128 == 0, else BEVGEN_ERR_INVALID. */
int bevgen_op_conv3x3_gn_stats(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_w_oihw, const float* d_bias, int range_route, float* d_y_nhwc, float* d_part, float* d_stats,
                               int n, int H, int W, int Cin, int Cout, void* stream);
/* conv_ranged (precision = F16X3 contexts, else BEVGEN_ERR_INVALID): ONE site of the range-safe mode exactly as bevgen_vq_decode / bevgen_vq_encode run it, whatever the
 * context's vq_range: device-side absmax of d_x and exponent e (the rule at bevgen_cfg.vq_range) -> d_exp[0], the convolution of x 2^-e without its bias, then
 * y = 2^e y + bias.  kind 0: 1x1; 1: 3x3, stride 1, padding 1; 2: the encoder's Downsample (zero pad bottom / right, 3x3, stride 2; H and W even, d_y [n, H/2, W/2, Cout],
 * and its last pass is the fused one that also takes the absmax of d_y).  Cin % 32 == 0, Cout % 4 == 0; d_bias is required; d_y must not alias d_x.  NaN / inf in d_x
 * raise BEVGEN_STATUS_F16_RANGE. */
int bevgen_op_conv_ranged(bevgen_ctx* ctx, const float* d_x_nhwc, const float* d_w_oihw, const float* d_bias, int kind, float* d_y_nhwc, int32_t* d_exp, int n, int H, int W,
                          int Cin, int Cout, void* stream);
/* The kernels in front of and around the layer stacks (embed.hip, tables.hip, the tile-list path of attention.hip), each through the launcher the model calls, with
 * operands laid out as muse.cpp / ar.cpp / context.cpp lay them out.  No entry clears or pre-fills a caller buffer.
 * camera_embed: d_img [B, C, T, D] = normalize(Wimg d - Wcam c) with d = E_inv [I_inv pix; 1], c = E_inv[..., 3] (norm + 1e-7), d_c_embed [B, C, D] = Wcam c;
 * d_I_inv [B, C, 3, 3], d_E_inv [B, C, 4, 4], d_plane [3, T], d_wimg / d_wcam [D, 4]. */
int bevgen_op_camera_embed(bevgen_ctx* ctx, const float* d_I_inv, const float* d_E_inv, const float* d_plane, const float* d_wimg, const float* d_wcam, float* d_img,
                           float* d_c_embed, int B, int C, int T, int D, void* stream);
/* cond_embed: d_out [B, K, D] = (d_cond_tok[clamp(id, 0, cond_vocab - 1)] + (bev_embed(grid) - sum_c (d_bev_cam_pos[c, k] + d_c_embed[b, c]))) + d_cond_pos[k]; the
 * middle term only with d_bev_grid [>= 2, K] non-NULL (then d_wbev [D, 2], d_bbev [D], d_bev_cam_pos [C, K, D], d_c_embed [B, C, D] are required). */
int bevgen_op_cond_embed(bevgen_ctx* ctx, const int64_t* d_cond_ids, const float* d_cond_tok, const float* d_cond_pos, const float* d_bev_grid /* or NULL */,
                         const float* d_wbev, const float* d_bbev, const float* d_bev_cam_pos, const float* d_c_embed, float* d_out, int B, int C, int K, int D,
                         int cond_vocab, void* stream);
/* token_rows: one row (table[clamp(id, 0, vocab_rows - 1)] + d_img row) + d_pos row per token (d_img NULL: no geometric term); D % 4 == 0 for kinds 0 and 2.
 *   kind 0 token_embed:   d_ids [B, N], d_img [B, N, D], d_pos [N, D] -> d_out [B, N, D]
 *   kind 1 ar_step_embed: d_ids [B] (this step's tokens), d_img [B, C T, D], j = d_fwd_idx[*d_step] -> d_out [B, D]
 *   kind 2 ar_seq_embed:  d_ids [B, N] camera-major, d_img [B, N, D], j = d_fwd_idx[s] -> d_out[b, row0 + s] of [B, rows_per_seq, D] for s < n_steps
 *   kind 3 gather_rows:   d_out [B, D] = d_table[b, row0] of [B, rows_per_seq, D]
 *   kind 4 store_tokens:  d_out (int64 [B, N]) [b, d_fwd_idx[*d_step]] = d_ids[b] */
int bevgen_op_token_rows(bevgen_ctx* ctx, int kind, const int64_t* d_ids, const float* d_table, const float* d_img /* or NULL */, const float* d_pos,
                         const int64_t* d_fwd_idx, const int* d_step, void* d_out, int B, int N, int D, int vocab_rows, int C, int T, int n_steps, int rows_per_seq, int row0,
                         void* stream);
/* The fp32 Route M q / k / v preparation: d_q [B, H, Nq, 64] = l2norm(8 d_qraw [B Nq, 64 H]) o d_q_scale (d_qraw NULL: skipped); d_k / d_v [B, H, Nk_pad, 64] rows
 * [0, Nk] = (null key / value of d_null_kv [2, H, 64], then d_kvraw [B Nk, (k | v) 64 H]), keys l2-normalised o d_k_scale (d_kvraw NULL: skipped). */
int bevgen_op_muse_qkv_prep_f32(bevgen_ctx* ctx, const float* d_qraw /* or NULL */, const float* d_kvraw /* or NULL */, const float* d_null_kv, const float* d_q_scale,
                                const float* d_k_scale, float* d_q, float* d_k, float* d_v, int B, int H, int Nq, int Nk, int Nk_pad, void* stream);
/* Route A's KV-cache writers on a cache [B, H, Lmax, 64] (kv_dtype 0 fp32 / 1 fp16; fp16 values outside the range raise BEVGEN_STATUS_F16_RANGE; 2 int8: the
 * BEVGEN_KV_I8 layout of B slots, [layers] of them back to back for replicate_prefix, which copies both planes; NaN / inf rows raise BEVGEN_STATUS_KV_NONFINITE).
 * bevgen_op_decode_attention and bevgen_op_ar_attn_fused take the same three storage types.
 *   kind 0 scatter: rows [pos0, pos0 + n) of every (b, h) from d_qkv [B n, (q | k | v) 64 H]; d_q [B, H, n, 64] (or NULL) receives the queries
 *   kind 1 append:  n = 1, row *d_pos + pos0 (d_pos a device int)
 *   kind 2 replicate_prefix: cache [layers, B, H, Lmax, 64]: the first `rows` rows of sequence slot `src` are copied to slots [dst0, dst0 + count) of every layer and head */
int bevgen_op_kv_cache_write(bevgen_ctx* ctx, int kind, const float* d_qkv, float* d_q /* or NULL */, void* d_kcache, void* d_vcache, int kv_dtype, int B, int H, int n,
                             int pos0, const int* d_pos, int Lmax, int layers, int rows, int src, int dst0, int count, void* stream);
/* The tables bevgen_finalize and the Route A prefill build (tables.hip, attention.hip), written into caller buffers.
 *   kind 0 attn_bias:   d_out0 [L, L] = tril_scatter(d_in0 [L (L + 1) / 2] or NULL) + (d_in1 [L, L] or NULL)
 *   kind 1 muse_bias:   d_in0 = attn_bias [L, L], rows = N, cols = K -> d_out0 [N, ld0] = (0 | attn_bias[K + q, K ..] | -1e30), d_out1 [N, ld1] = (0 | attn_bias[K + q, .. K) | -1e30)
 *   kind 2 allowed:     d_out0 (uint8 [rows cols]) = d_in0 (fp32) != 0
 *   kind 3 layout:      d_in0 int64 [heads, L / blk, L / blk] -> d_out0 uint8 of the same shape, d_out1 uint16 [heads, L / blk, ld1] = (count, ascending ids of the 16-key
 *                       chunks that overlap a present block); ld1 >= ceil(L / 16) + 1; slots behind the count are not written
 *   kind 4 masked_bias: d_out0 [heads, rows, ld1] = visible(h, r, c) ? scale d_in0[r, c] (row stride ld0; NULL: 0) : -1e30, columns >= cols -1e30; visible = element mask
 *                       d_in1 (uint8 [L, L], head stride hs0; NULL: all) AND block layout d_in2 (uint8 [., L / blk, L / blk], head stride hs1; NULL: all)
 *   kind 5 attn_tiles:  d_in0 = masked bias (row stride ld0, head stride hs0), rows = Nq, cols = Nk_pad -> d_out0 uint16 [heads, ceil(Nq / 128), Nk_pad / 32 + 1] =
 *                       (count, ascending ids of the 32-key tiles in which a row of the 128-row block has a value above 0.5 * -1e30) */
int bevgen_op_attn_tables(bevgen_ctx* ctx, int kind, const void* d_in0, const void* d_in1, const void* d_in2, void* d_out0, void* d_out1, int heads, int L, int rows, int cols,
                          int blk, int ld0, int ld1, long hs0, long hs1, float scale, void* stream);
/* The flash-attention kernel in the form Route A's prefill and bevgen_sparse_self_attention run it: d_bias [H, Nq, ldbias] a masked bias per head, use_tiles != 0: the
 * tile lists built from it inside the call (launch_build_attn_tiles), d_k / d_v [B / kv_group, H, Nk_pad, 64], d_residual (or NULL) added in the output's layout,
 * out_layout 0: d_out [B, Nq, 64 H], 1: [B, H, Nq, 64].  Every query row must see a key in a listed tile. */
int bevgen_op_attention_tiles(bevgen_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, const float* d_bias, int ldbias, const float* d_residual /* or NULL */,
                              int B, int H, int Nq, int Nk_pad, float scale, int kv_group, int use_tiles, int out_layout, float* d_out, void* stream);

/* Per-kernel timing support for bench.py's roofline leg: number of workgroup splits the decode-attention kernel uses. */
int bevgen_decode_attention_splits(int B, int H, int n);
/* Bytes of workspace bevgen_op_image_sqerr (op 0; kernel_size ignored) / bevgen_op_ssim (op 1) need for these shapes: a pure function, no context.  -1: the call would be refused. */
long bevgen_metrics_workspace_bytes(int op, int n, int C, int H, int W, int kernel_size);
/* Bytes of the prepared-weight image of bevgen_lpips_prepare and of bevgen_lpips' workspace, for a context of BEVGEN_PRECISION_* `precision`: pure functions, no context,
 * computed by the layout code that carves the two blocks.  -1: an unknown precision / a call that would be refused.  The workspace does not grow with n beyond one chunk. */
long bevgen_lpips_prepared_bytes(int precision);
long bevgen_lpips_workspace_bytes(int n, int H, int W, int precision);

/* HIP-event timing of the hot kernels on their launch stream.  Between begin and end every launch of
 *   0 gemm (fp32 MFMA)   1 conv3x3 (implicit GEMM)   2 flash attention   3 decode attention   4 skinny GEMM
 *   5 small-problem launches of the split-precision GEMM (128- / 64-row blocks, the short last part of a row-split launch; kind 0 is then one kernel)
 * is bracketed by an event pair; end synchronises the device and writes out[kind*3 + {0,1,2}] =
 * {launches, total milliseconds, total algorithmic work (FLOP for 0-2 and 5, bytes for 3-4)} for the 6 kinds (18 doubles). */
#define BEVGEN_PROFILE_KINDS 6
int bevgen_profile_begin(bevgen_ctx* ctx);
int bevgen_profile_end(bevgen_ctx* ctx, double* out);

/* Per-step latency of bevgen_ar_sample: with timing enabled the library records one HIP event after every replay of the captured decode step;
 * bevgen_ar_step_times writes the durations (ms) of the most recent call's steps to the HOST array h_out_ms[cap] and their number to *count (synchronises). */
int bevgen_ar_step_timing(bevgen_ctx* ctx, int enable);
int bevgen_ar_step_times(bevgen_ctx* ctx, float* h_out_ms, int cap, int* count);

/* Diagnostics: phase timestamps of the fused Route A decode kernels.  d_buf = device buffer of 3 * 4096 * 8 int64 (kinds: 0 ln1+qkv+attention,
 * 1 ln2+MLP-up, 2 MLP-down; [workgroup][8] 100 MHz device timestamps at the phase boundaries of the most recent launch), NULL = off. */
int bevgen_set_trace_buffer(bevgen_ctx* ctx, void* d_buf);

#ifdef __cplusplus
}
#endif
#endif /* BEVGEN_HIP_H */
