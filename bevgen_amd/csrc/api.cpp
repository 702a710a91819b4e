// extern "C" surface of libbevgen_hip (declared in include/bevgen_hip.h): argument validation, exception -> error-code
// translation.  No torch types cross this boundary: raw pointers, sizes and a hipStream_t.
#include <memory>

#include "model.h"
#include "profiler.h"

using namespace bevgen;

struct bevgen_ctx : public Ctx {};

static thread_local std::string g_create_error;

template <class F>
static int guarded(bevgen_ctx* ctx, F&& f, bool check_first = true) {
    try {
        if (!ctx) return BEVGEN_ERR_INVALID;
        HIP_CHECK(hipSetDevice(ctx->device));
        split_registry_set(ctx->cfg.precision == BEVGEN_PRECISION_F16X3 ? &ctx->split : nullptr);
        struct CurrentProf {   // this context's profiler and status word receive the launch records / flags of this call (restored on every exit path)
            Profiler* old;
            unsigned* old_st;
            CurrentProf(Profiler* p, unsigned* st) : old(prof_set_current(p)), old_st(status_set_current(st)) {}
            ~CurrentProf() { prof_set_current(old); status_set_current(old_st); }
        } cur(&ctx->prof, ctx->status_dev);
        // a flag raised by a kernel of an EARLIER (asynchronous) call: the host-visible word is read without synchronising, the error belongs to that call
        if (check_first) ctx->check_status("raised by an earlier call on this context");
        f();
        return BEVGEN_OK;
    } catch (const Error& e) {
        if (ctx) ctx->last_error = e.what();
        return e.code;
    } catch (const std::exception& e) {
        if (ctx) ctx->last_error = e.what();
        return BEVGEN_ERR_INTERNAL;
    }
}

static void need_final(bevgen_ctx* c) {
    if (!c->finalized) fail(BEVGEN_ERR_STATE, "bevgen_finalize must be called after loading tensors and before compute calls");
}

extern "C" {

int bevgen_abi_version(void) { return BEVGEN_ABI_VERSION; }

int bevgen_create(const bevgen_cfg* cfg, int device, bevgen_ctx** out) {
    try {
        BG_REQUIRE(cfg && out, "bevgen_create: null argument");
        BG_REQUIRE(cfg->abi_version == BEVGEN_ABI_VERSION, "bevgen_create: ABI version %d, library is %d", cfg->abi_version, BEVGEN_ABI_VERSION);
        BG_REQUIRE(cfg->route == BEVGEN_ROUTE_MASKGIT || cfg->route == BEVGEN_ROUTE_AR, "bevgen_create: unknown route %d", cfg->route);
        BG_REQUIRE(cfg->kv_cache_dtype == BEVGEN_KV_F32 || cfg->kv_cache_dtype == BEVGEN_KV_F16 || cfg->kv_cache_dtype == BEVGEN_KV_I8, "bevgen_create: kv_cache_dtype must be BEVGEN_KV_F32, BEVGEN_KV_F16 or BEVGEN_KV_I8");
        const bool f16x1 = cfg->precision == BEVGEN_PRECISION_F16X1;
        BG_REQUIRE(cfg->precision == BEVGEN_PRECISION_FP32 || cfg->precision == BEVGEN_PRECISION_F16X3 || f16x1,
                   "bevgen_create: precision must be BEVGEN_PRECISION_FP32, BEVGEN_PRECISION_F16X3 or BEVGEN_PRECISION_F16X1");
        BG_REQUIRE(cfg->weight_dtype == BEVGEN_W_F32 || (cfg->weight_dtype == BEVGEN_W_F16 && (cfg->precision == BEVGEN_PRECISION_F16X3 || f16x1)),
                   "bevgen_create: weight_dtype must be BEVGEN_W_F32, or BEVGEN_W_F16 together with BEVGEN_PRECISION_F16X3 / _F16X1");
        BG_REQUIRE(cfg->decode_weight_dtype == BEVGEN_W_F32 || cfg->decode_weight_dtype == BEVGEN_W_F16 || cfg->decode_weight_dtype == BEVGEN_W_I8,
                   "bevgen_create: decode_weight_dtype must be BEVGEN_W_F32, BEVGEN_W_F16 or BEVGEN_W_I8, got %d", cfg->decode_weight_dtype);
        BG_REQUIRE(cfg->vq_range == 0 || cfg->vq_range == 1, "bevgen_create: vq_range must be 0 (refuse) or 1 (rescale), got %d", cfg->vq_range);
        int ndev = 0;
        HIP_CHECK(hipGetDeviceCount(&ndev));
        BG_REQUIRE(device >= 0 && device < ndev, "bevgen_create: device %d not present (%d visible)", device, ndev);
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, device));
        BG_REQUIRE(std::string(prop.gcnArchName).rfind("gfx950", 0) == 0, "bevgen_create: device %d is %s; this library is built for gfx950 (MI355X) only", device,
                   prop.gcnArchName);
        HIP_CHECK(hipSetDevice(device));
        std::unique_ptr<bevgen_ctx> c(new bevgen_ctx());
        c->cfg = *cfg;
        if (f16x1) {   // an F16X3 context in everything but the Route M projections (bevgen_hip.h): every `precision == F16X3` test of the library holds for it
            c->cfg.precision = BEVGEN_PRECISION_F16X3;
            c->single_product = true;
        }
        c->device = device;
        // the device status word: mapped host memory, so that the host reads it without a copy or a synchronisation (common.h BG_ST_*)
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&c->status_host), 64, hipHostMallocMapped));
        *c->status_host = 0;
        HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->status_dev), c->status_host, 0));
        *out = c.release();
        return BEVGEN_OK;
    } catch (const Error& e) {
        g_create_error = e.what();
        return e.code;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        return BEVGEN_ERR_INTERNAL;
    }
}

void bevgen_destroy(bevgen_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    if (ctx->status_host && *ctx->status_host)   // nobody asked (no bevgen_synchronize, no later call): the last resort is to say it here
        fprintf(stderr, "libbevgen_hip: context destroyed with device status word %u pending (BEVGEN_STATUS_* in bevgen_hip.h): results of its last calls were invalid\n",
                *ctx->status_host);
    delete ctx;
}

const char* bevgen_last_error(const bevgen_ctx* ctx) { return ctx ? ctx->last_error.c_str() : g_create_error.c_str(); }

int bevgen_synchronize(bevgen_ctx* ctx, void* stream) {
    return guarded(ctx, [&] {
        HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        if (ctx->graph_stream) HIP_CHECK(hipStreamSynchronize(ctx->graph_stream));   // (joined into `stream` by an event at the end of bevgen_ar_sample; belt and braces)
        ctx->check_status("bevgen_synchronize");
    }, false);
}

int bevgen_status(bevgen_ctx* ctx, unsigned* word) {
    if (!ctx || !word) return BEVGEN_ERR_INVALID;
    *word = ctx->status_host ? __atomic_load_n(ctx->status_host, __ATOMIC_ACQUIRE) : 0u;
    return BEVGEN_OK;
}

int bevgen_load_tensor(bevgen_ctx* ctx, const char* name, const void* h, int dtype, int ndim, const int64_t* shape) {
    return guarded(ctx, [&] { ctx_load_tensor(*ctx, name, h, dtype, ndim, shape); });
}

int bevgen_set_tables(bevgen_ctx* ctx, const int64_t* fwd, const float* mask, const int64_t* layout, const float* prob, const float* plane) {
    return guarded(ctx, [&] {
        const auto& g = ctx->cfg;
        const int64_t T = (int64_t)g.cam_latent_h * g.cam_latent_w, N = T * g.num_cams, L = g.seq_len, nb = L / g.sparse_block_size;
        if (fwd) { const int64_t s[1] = {N}; ctx_load_tensor(*ctx, "table.forward_shuffle_idx", fwd, BEVGEN_DTYPE_I64, 1, s); }
        if (mask) { const int64_t s[2] = {L, L}; ctx_load_tensor(*ctx, "table.attention_mask", mask, BEVGEN_DTYPE_F32, 2, s); }
        if (layout) { const int64_t s[3] = {g.num_heads, nb, nb}; ctx_load_tensor(*ctx, "table.layout", layout, BEVGEN_DTYPE_I64, 3, s); }
        if (prob) { const int64_t s[2] = {L, L}; ctx_load_tensor(*ctx, "table.prob_matrix", prob, BEVGEN_DTYPE_F32, 2, s); }
        if (plane) { const int64_t s[2] = {3, T}; ctx_load_tensor(*ctx, "table.image_plane", plane, BEVGEN_DTYPE_F32, 2, s); }
    });
}

int bevgen_finalize(bevgen_ctx* ctx) {
    return guarded(ctx, [&] { ctx_finalize(*ctx); });
}

int bevgen_muse_forward(bevgen_ctx* ctx, const int64_t* ids, const int64_t* cond, const float* I_inv, const float* E_inv, int B, float* logits, float* embed, void* stream) {
    return bevgen_muse_forward_ex(ctx, ids, cond, I_inv, E_inv, B, logits, embed, 0, stream);
}

int bevgen_muse_forward_ex(bevgen_ctx* ctx, const int64_t* ids, const int64_t* cond, const float* I_inv, const float* E_inv, int B, float* logits, float* embed,
                           int null_condition, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(ids && cond && I_inv && E_inv, "muse_forward: null input");
        BG_REQUIRE(B >= 1 && (ctx->cfg.max_batch <= 0 || B <= ctx->cfg.max_batch), "muse_forward: batch %d exceeds max_batch %d", B, ctx->cfg.max_batch);
        muse_forward(*ctx, MuseBatch{cond, I_inv, E_inv, B}, ids, logits, embed, (hipStream_t)stream, null_condition != 0);
    });
}

int bevgen_maskgit_generate(bevgen_ctx* ctx, const int64_t* cond, const float* I_inv, const float* E_inv, int B, int timesteps, const int32_t* sched, float temperature,
                            int topk_k, float critic_noise_scale, const float* gumbel_u, const float* critic_u, const int64_t* init_ids, int64_t* out,
                            unsigned long long noise_seed, void* stream) {
    return bevgen_maskgit_generate_ex(ctx, cond, I_inv, E_inv, B, timesteps, sched, temperature, topk_k, critic_noise_scale, gumbel_u, critic_u, init_ids, out, noise_seed, 0, 1, stream);
}

int bevgen_maskgit_generate_ex(bevgen_ctx* ctx, const int64_t* cond, const float* I_inv, const float* E_inv, int B, int timesteps, const int32_t* sched, float temperature,
                               int topk_k, float critic_noise_scale, const float* gumbel_u, const float* critic_u, const int64_t* init_ids, int64_t* out,
                               unsigned long long noise_seed, int score_mode, int samples_per_layout, void* stream) {
    return bevgen_maskgit_generate_guided(ctx, cond, I_inv, E_inv, B, timesteps, sched, temperature, topk_k, critic_noise_scale, gumbel_u, critic_u, init_ids, out, noise_seed,
                                          score_mode, samples_per_layout, 1.f, stream);
}

int bevgen_maskgit_generate_guided(bevgen_ctx* ctx, const int64_t* cond, const float* I_inv, const float* E_inv, int B, int timesteps, const int32_t* sched, float temperature,
                                   int topk_k, float critic_noise_scale, const float* gumbel_u, const float* critic_u, const int64_t* init_ids, int64_t* out,
                                   unsigned long long noise_seed, int score_mode, int samples_per_layout, float cond_scale, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(cond_scale == cond_scale && cond_scale - cond_scale == 0.f, "maskgit_generate: cond_scale must be finite");
        need_final(ctx);
        BG_REQUIRE(cond && I_inv && E_inv && out && sched, "maskgit_generate: null argument");
        BG_REQUIRE(B >= 1 && (ctx->cfg.max_batch <= 0 || B <= ctx->cfg.max_batch), "maskgit_generate: batch %d exceeds max_batch %d", B, ctx->cfg.max_batch);
        BG_REQUIRE(topk_k >= 1 && topk_k <= ctx->cfg.vocab_size, "maskgit_generate: topk_k=%d out of range", topk_k);
        for (int i = 0; i < timesteps; ++i)
            BG_REQUIRE(sched[i] >= 1 && sched[i] <= ctx->cfg.cam_latent_h * ctx->cfg.cam_latent_w, "maskgit_generate: mask_schedule[%d]=%d out of range", i, sched[i]);
        BG_REQUIRE(samples_per_layout >= 1 && B % samples_per_layout == 0, "maskgit_generate: batch %d is not a multiple of samples_per_layout %d", B, samples_per_layout);
        const MaskgitSampling sp{timesteps, sched, temperature, topk_k, critic_noise_scale, gumbel_u, critic_u, init_ids, noise_seed, score_mode, cond_scale};
        maskgit_generate(*ctx, MuseBatch{cond, I_inv, E_inv, B, samples_per_layout}, sp, out, (hipStream_t)stream);
    });
}

int bevgen_maskgit_loss(bevgen_ctx* ctx, const int64_t* ids, const int64_t* cond, const float* I_inv, const float* E_inv, int B, const int32_t* h_num_masked,
                        const float* perm_u, const float* gumbel_u, float temperature, unsigned long long noise_seed, int with_critic, float critic_loss_weight, float* out,
                        uint8_t* mask_out, int64_t* x_out, int64_t* critic_input_out, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(ids && cond && I_inv && E_inv && h_num_masked && out, "maskgit_loss: null argument");
        BG_REQUIRE(B >= 1 && (ctx->cfg.max_batch <= 0 || B <= ctx->cfg.max_batch), "maskgit_loss: batch %d exceeds max_batch %d", B, ctx->cfg.max_batch);
        const MaskgitLoss lp{h_num_masked, perm_u, gumbel_u, temperature, noise_seed, with_critic != 0, critic_loss_weight, out, mask_out, x_out, critic_input_out};
        maskgit_loss(*ctx, MuseBatch{cond, I_inv, E_inv, B}, ids, lp, (hipStream_t)stream);
    });
}

int bevgen_op_maskgit_train_mask(bevgen_ctx* ctx, const int64_t* ids, const float* perm_u, const int32_t* num_masked, int rows, int T, int64_t mask_id,
                                 unsigned long long seed, int64_t* x, uint8_t* mask, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(ids && num_masked && x && mask && rows >= 1 && T >= 1, "op_maskgit_train_mask: bad arguments");
        launch_maskgit_train_mask(ids, perm_u, num_masked, x, mask, rows, T, mask_id, seed, (hipStream_t)stream);
    });
}

int bevgen_op_masked_ce(bevgen_ctx* ctx, const float* logits, int ldl, const int64_t* ids, const uint8_t* mask, long rows, int V, long denom, float* nll, float* out,
                        void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(logits && ids && mask && nll && rows >= 1 && V >= 1 && ldl >= V && (!out || denom >= 1), "op_masked_ce: bad arguments");
        launch_maskgit_ce_rows(logits, ldl, ids, mask, nll, rows, V, (hipStream_t)stream);
        if (out) launch_mean_fixed_order(nll, rows, out, (hipStream_t)stream, denom);
    });
}

int bevgen_op_critic_bce(bevgen_ctx* ctx, const float* embed, int lde, const float* w, const float* b, const int64_t* ids, const int64_t* critic_input, long rows, int D,
                         float* loss_rows, float* out, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(embed && w && b && ids && critic_input && loss_rows && rows >= 1 && D >= 1 && lde >= D, "op_critic_bce: bad arguments");
        launch_critic_bce_rows(embed, lde, w, b, ids, critic_input, loss_rows, rows, D, (hipStream_t)stream);
        if (out) launch_mean_fixed_order(loss_rows, rows, out, (hipStream_t)stream);
    });
}

int bevgen_op_philox_uniform(bevgen_ctx* ctx, unsigned long long seed, unsigned iter, unsigned stream_id, int V, long n, float* out, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(out && n >= 0, "op_philox_uniform: bad arguments");
        launch_philox_fill(out, n, seed, iter, stream_id, V, (hipStream_t)stream);
    });
}

int bevgen_sparse_self_attention(bevgen_ctx* ctx, const float* q, const float* k, const float* v, const int64_t* layout, const float* mask, const float* add, int B,
                                 int H, int L, int block, float* out, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(q && k && v && layout && mask && out, "sparse_self_attention: null argument");
        BG_REQUIRE(B >= 1 && H >= 1 && L >= 1 && block >= 1, "sparse_self_attention: bad sizes");
        sparse_self_attention_op(*ctx, q, k, v, layout, mask, add, B, H, L, block, out, (hipStream_t)stream);
    });
}

int bevgen_ar_prefill(bevgen_ctx* ctx, const int64_t* cond, const float* I_inv, const float* E_inv, int B, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(cond && I_inv && E_inv, "ar_prefill: null input");
        ar_prefill(*ctx, cond, I_inv, E_inv, B, (hipStream_t)stream);
    });
}

int bevgen_ar_logits(bevgen_ctx* ctx, float* logits, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(logits, "ar_logits: null output");
        ar_logits(*ctx, logits, (hipStream_t)stream);
    });
}

int bevgen_ar_decode_step(bevgen_ctx* ctx, const int64_t* tok, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(tok, "ar_decode_step: null token pointer");
        ar_decode_step(*ctx, tok, (hipStream_t)stream);
    });
}

int bevgen_ar_forward(bevgen_ctx* ctx, const int64_t* cond, const float* I_inv, const float* E_inv, int B, const int64_t* ids, int n_steps, float* logits,
                      const int64_t* target, const float* weight, float* nll, float* loss, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(cond && I_inv && E_inv && ids, "ar_forward: null input");
        BG_REQUIRE(B >= 1 && (ctx->cfg.max_batch <= 0 || B <= ctx->cfg.max_batch), "ar_forward: batch %d exceeds max_batch %d", B, ctx->cfg.max_batch);
        BG_REQUIRE(target || (!nll && !loss && !weight), "ar_forward: d_nll / d_loss / d_weight need d_target");
        ar_forward(*ctx, cond, I_inv, E_inv, B, ids, n_steps, logits, target, weight, nll, loss, (hipStream_t)stream);
    });
}

int bevgen_ar_sample(bevgen_ctx* ctx, const int64_t* cond,const float* I_inv, const float* E_inv, int B, int steps, int top_k, float temperature, int greedy,
                     const float* noise_u, int samples_per_layout, int64_t* out, float* step_logits, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(cond && I_inv && E_inv && out, "ar_sample: null argument");
        BG_REQUIRE(temperature > 0.f, "ar_sample: temperature must be positive");
        ar_sample(*ctx, cond, I_inv, E_inv, B, steps, top_k, temperature, greedy, noise_u, samples_per_layout, nullptr, out, step_logits, (hipStream_t)stream);
    });
}

int bevgen_ar_sample_forced(bevgen_ctx* ctx, const int64_t* cond, const float* I_inv, const float* E_inv, int B, int steps, int top_k, float temperature, int greedy,
                            const float* noise_u, int samples_per_layout, const int64_t* forced, int64_t* out, float* step_logits, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(cond && I_inv && E_inv && out, "ar_sample_forced: null argument");
        BG_REQUIRE(temperature > 0.f, "ar_sample_forced: temperature must be positive");
        ar_sample(*ctx, cond, I_inv, E_inv, B, steps, top_k, temperature, greedy, noise_u, samples_per_layout, forced, out, step_logits, (hipStream_t)stream);
    });
}

static void vq_default_grid(const bevgen_ctx* ctx, int& h, int& w) {   // 0 x 0 = the square grid of ddconfig.resolution
    if (h <= 0 || w <= 0) h = w = ctx->cfg.vq_resolution >> (ctx->cfg.vq_num_levels - 1);
}

int bevgen_vq_decode(bevgen_ctx* ctx, const int64_t* ids, int n, int lat_h, int lat_w, int out_mode, void* out, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(ids && out && n >= 1 && out_mode >= 0 && out_mode <= 2, "vq_decode: bad arguments");
        vq_default_grid(ctx, lat_h, lat_w);
        vq_decode(*ctx, ids, nullptr, n, lat_h, lat_w, out_mode, out, (hipStream_t)stream);
    });
}

int bevgen_vq_encode(bevgen_ctx* ctx, const float* x, int n, int H, int W, int64_t* ids, void* stream) {
    return bevgen_vq_encode_ex(ctx, x, n, H, W, nullptr, nullptr, nullptr, 0.25f, ids, nullptr, nullptr, stream);
}

int bevgen_vq_encode_ex(bevgen_ctx* ctx, const float* x, int n, int H, int W, const float* I_inv, const float* E_inv, const float* plane, float beta, int64_t* ids,
                        float* row_err, float* loss, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(x && ids && n >= 1, "vq_encode: bad arguments");
        if (H <= 0 || W <= 0) H = W = ctx->cfg.vq_resolution;
        VqEncodeExtras ex;
        ex.I_inv = I_inv; ex.E_inv = E_inv; ex.plane = plane;
        ex.beta = beta; ex.row_err = row_err; ex.loss = loss;
        vq_encode(*ctx, x, n, H, W, ids, ex, (hipStream_t)stream);
    });
}

int bevgen_vq_decode_latents(bevgen_ctx* ctx, const float* zq, int n, int lat_h, int lat_w, int out_mode, void* out, void* stream) {
    return guarded(ctx, [&] {
        need_final(ctx);
        BG_REQUIRE(zq && out && n >= 1 && out_mode >= 0 && out_mode <= 2, "vq_decode_latents: bad arguments");
        vq_default_grid(ctx, lat_h, lat_w);
        vq_decode(*ctx, nullptr, zq, n, lat_h, lat_w, out_mode, out, (hipStream_t)stream);
    });
}

int bevgen_vq_range_exponents(bevgen_ctx* ctx, int32_t* h_out, int cap, int* count) {
    return guarded(ctx, [&] {
        BG_REQUIRE(count && cap >= 0 && (h_out || cap == 0), "vq_range_exponents: bad arguments");
        *count = vq_range_exponents(*ctx, h_out, cap);
    });
}

int bevgen_op_gemm(bevgen_ctx* ctx, const float* a, const float* w, const float* bias, const float* residual, float* c, int M, int N, int K, int act_gelu, int skinny,
                   void* stream) {
    const int skinny_in = skinny;
    return guarded(ctx, [&] {
        GemmArgs g;
        g.A = a; g.B = w; g.C = c; g.R = residual; g.bias_n = bias;
        g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.ldr = N;
        g.act = act_gelu ? ACT_GELU : ACT_NONE;
        if (skinny == 5 || skinny == 6) skinny = 3;   // 5 = mode 3 with the k range split over three slices (the low-latency path of small batches); needs M small enough for
        const bool ksplit3 = skinny_in == 5 || skinny_in == 8;   // 128-row tiles.  6 = mode 3 in its stream-K form (gemm_split_glds_sk_kernel), whatever the shape
        const bool stream_k = skinny_in == 6;
        // 7 - 9 = the single-product forms (BEVGEN_PRECISION_F16X1): 7 = mode 4 computing f16(a) f16(w)^T, 8 = 7 with the k range in three slices, 9 = mode 2
        // (gemm_split_kernel) single-product.  w's low plane is ignored whatever w holds
        const bool single = skinny_in >= 7 && skinny_in <= 9;
        if (skinny == 7 || skinny == 8) skinny = 4;
        if (skinny == 9) skinny = 2;
        if (skinny == 4 || skinny == 3 || skinny == 2) {  // split-precision paths with on-the-fly operand splits (tests / roofline probes): 3 = LDS-DMA kernel, 4 = the same for
                                                          // an f16-representable w (two MFMAs per product: the weights='f16' mode's kernel)
            uint16_t *bp, *ap;
            ctx->arena.carve([&](Arena& ar) {
                bp = ar.get<uint16_t>((size_t)N * K * 2);
                ap = skinny >= 3 ? ar.get<uint16_t>((size_t)M * K * 2) : nullptr;
                g.kpart = skinny >= 3 && ksplit3 ? ar.get<float>((size_t)3 * M * N) : nullptr;
                g.sk_ws = skinny >= 3 && stream_k ? ar.alloc(gemm_sk_ws_bytes()) : nullptr;
            });
            launch_split_weight(w, bp, (long)N * K, (hipStream_t)stream);
            g.B_hi = bp; g.B_lo = bp + 32;
            g.a_hi_only = single;
            g.b_lo_zero = single;
            if (skinny >= 3) {
                g.b_lo_zero = skinny == 4;
                launch_split_weight(a, ap, (long)M * K, (hipStream_t)stream);
                g.A_hi = ap; g.A_lo = ap + 32;
                if (ksplit3) g.ksplit = 3;
                if (stream_k) {
                    HIP_CHECK(hipMemsetAsync(g.sk_ws, 0, 1024 * sizeof(unsigned), (hipStream_t)stream));
                    g.sk_epoch = 1; g.sk_force = true;
                }
                launch_gemm_split_glds(g, (hipStream_t)stream);
            } else {
                launch_gemm_split(g, (hipStream_t)stream);
            }
        } else if (skinny) {   // split-K workspace from this context's arena (one per context / device)
            float* ws;
            ctx->arena.carve([&](Arena& ar) { ws = reinterpret_cast<float*>(ar.alloc(gemm_skinny_ws_bytes(M, N, K))); });
            launch_gemm_skinny_ws(g, ws, (hipStream_t)stream);
        }
        else launch_gemm(g, (hipStream_t)stream);
    });
}

int bevgen_op_muse_qkv(bevgen_ctx* ctx, int kind, const float* a, const float* w, const float* ln_gamma, const float* q_scale, const float* k_scale, const float* null_kv, int B,
                       int T, int H, int K, int ld, float post, int block, int weights, int form, int ksplit, void* qh, void* ql, void* kh, void* kl, void* vth, void* vtl,
                       void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        const bool has_q = kind == 0 || kind == 2, has_kv = kind == 1 || kind == 2;
        BG_REQUIRE(ctx->cfg.precision == BEVGEN_PRECISION_F16X3, "op_muse_qkv: needs a split-precision (f16x3) context");
        BG_REQUIRE(kind >= 0 && kind <= 2 && a && w && B >= 1 && T >= 1 && H >= 1 && K >= 32 && K % 32 == 0 && (long)B * T * K < (1L << 30) && 192L * H * K < (1L << 30),
                   "op_muse_qkv: bad arguments (the plane images are addressed with 32-bit byte offsets)");
        BG_REQUIRE((!has_q || (q_scale && qh && ql)) && (!has_kv || (k_scale && null_kv && kh && kl && vth && vtl && ld >= T + 1)),
                   "op_muse_qkv: kind %d needs its scales, its output planes and ld >= T + 1 (ld=%d T=%d)", kind, ld, T);
        BG_REQUIRE((block == 0 || block == 4) && weights >= 0 && weights <= 2 && (form == 0 || (form == 1 && kind != 2)) && ksplit >= 1 && ksplit <= 8 && (form == 1 || ksplit == 1),
                   "op_muse_qkv: block 0 | 4, weights 0..2, form 0 | 1 (1: kind 0 or 1), ksplit 1..8 (form 1 only)");
        const int M = B * T, HD = H * 64, N = HD * (kind + 1);
        uint16_t *ap, *bp;
        float *wr, *raw, *kpart;
        void* aux;
        ctx->arena.carve([&](Arena& ar) {
            ap = ar.get<uint16_t>((size_t)M * K * 2);
            bp = ar.get<uint16_t>((size_t)N * K * 2);
            wr = weights ? ar.get<float>((size_t)N * K) : nullptr;   // round_to_f16 rounds in place: a copy of the caller's matrix
            aux = has_kv ? ar.alloc((size_t)4 * HD * sizeof(_Float16)) : nullptr;
            raw = form == 1 ? ar.get<float>((size_t)M * N) : nullptr;
            kpart = form == 1 && ksplit > 1 ? ar.get<float>((size_t)ksplit * M * N) : nullptr;
        });
        if (ln_gamma) launch_layernorm_planes(a, K, ln_gamma, nullptr, ap, K, M, K, 1e-5f, s);
        else launch_split_weight(a, ap, (long)M * K, s);
        const float* wu = w;
        if (weights) {
            HIP_CHECK(hipMemcpyAsync(wr, w, (size_t)N * K * sizeof(float), hipMemcpyDeviceToDevice, s));
            launch_round_to_f16(wr, nullptr, (long)N * K, s);
            wu = wr;
        }
        launch_split_weight(wu, bp, (long)N * K, s);
        if (has_kv) launch_muse_null_kv_prep(null_kv, k_scale, aux, H, s);
        GemmArgs g;
        g.A_hi = ap; g.A_lo = ap + 32; g.B = wu; g.B_hi = bp; g.B_lo = bp + 32;
        g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N;
        g.b_lo_zero = weights >= 1; g.a_hi_only = weights == 2;
        g.force_wm = block;
        if (form == 1) {   // muse.cpp project(): the projection into the raw matrix, then the preparation kernel
            g.C = raw; g.ksplit = ksplit; g.kpart = kpart;
            launch_gemm_split_glds(g, s);
            if (kind == 0) launch_muse_q_prep_split(raw, q_scale, qh, ql, B, H, T, post, s);
            else launch_muse_kv_prep_split(raw, null_kv, k_scale, kh, kl, vth, vtl, B, H, T, ld, s);
            return;
        }
        g.epi = kind == 0 ? EPI_MUSE_Q : kind == 1 ? EPI_MUSE_KV : EPI_MUSE_QKV;
        g.epi_rows = T; g.epi_heads = H;
        if (kind == 0) { g.epi_scale = q_scale; g.epi_hi = qh; g.epi_lo = ql; g.epi_post = post; }
        else {
            g.epi_scale = k_scale; g.epi_hi = kh; g.epi_lo = kl; g.epi_hi2 = vth; g.epi_lo2 = vtl; g.epi_aux = aux; g.epi_ld = ld;
            if (kind == 2) { g.epi_qh = qh; g.epi_ql = ql; g.epi_qscale = q_scale; g.epi_post = post; }
        }
        launch_gemm_split_glds(g, s);
    });
}

int bevgen_op_muse_ff(bevgen_ctx* ctx, const float* x, const float* w1, const float* gamma3, const float* w4, const float* residual, int M, int D, int F, int Dout, int level,
                      int merge, int block, float* h_out, void* g_planes, float* g_sums, float* rowstat_out, void* y_planes, float* y_sums, float* y_out, void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        BG_REQUIRE(ctx->cfg.precision == BEVGEN_PRECISION_F16X3, "op_muse_ff: needs a split-precision (f16x3) context");
        BG_REQUIRE(x && w1 && gamma3 && w4 && residual && M >= 1 && D >= 32 && D % 32 == 0 && F >= 1 && F <= 3072 && Dout >= 32 && Dout % 32 == 0 && (long)M * std::max(D, F + 64) < (1L << 30) &&
                       (long)Dout * (F + 64) < (1L << 30) && (long)M * Dout < (1L << 29),
                   "op_muse_ff: bad arguments (the plane images are addressed with 32-bit byte offsets)");
        BG_REQUIRE(level >= 0 && level <= 2 && (merge == 0 || merge == 1) && (block == 0 || block == 4), "op_muse_ff: level 0..2, merge 0 | 1, block 0 | 4");
        BG_REQUIRE(reinterpret_cast<uintptr_t>(residual) % 16 == 0 && reinterpret_cast<uintptr_t>(y_out) % 16 == 0 && reinterpret_cast<uintptr_t>(h_out) % 16 == 0,
                   "op_muse_ff: residual, y and h must be 16-byte aligned");
        const int Fpad = (int)round_up(F, 64), GF = Fpad / 32, GD = Dout / 32;
        uint16_t *xp, *w1p, *w4p;
        float *w1o, *w4pad, *w4g, *cs, *h, *gs, *rs, *ys, *y;
        void *gp, *yp;
        ctx->arena.carve([&](Arena& ar) {
            xp = ar.get<uint16_t>((size_t)M * D * 2);
            w1o = ar.get<float>((size_t)2 * Fpad * D);
            w1p = ar.get<uint16_t>((size_t)2 * Fpad * D * 2);
            w4pad = ar.get<float>((size_t)Dout * Fpad);
            w4g = level >= 1 ? ar.get<float>((size_t)Dout * Fpad) : nullptr;
            cs = level >= 1 ? ar.get<float>((size_t)Dout) : nullptr;
            w4p = ar.get<uint16_t>((size_t)Dout * Fpad * 2);
            h = level == 0 && !h_out ? ar.get<float>((size_t)M * Fpad) : h_out;
            gp = level == 0 || !g_planes ? ar.alloc((size_t)M * Fpad * 4) : g_planes;   // (level 0: the NORMALISED planes - not the image the caller's buffer is for)
            gs = level >= 1 && !g_sums ? ar.get<float>((size_t)GF * M * 2) : g_sums;
            rs = level >= 1 && merge == 0 && !rowstat_out ? ar.get<float>((size_t)M * 2) : rowstat_out;
            yp = level == 2 && !y_planes ? ar.alloc((size_t)M * Dout * 4) : y_planes;
            ys = level == 2 && !y_sums ? ar.get<float>((size_t)GD * M * 2) : y_sums;
            y = !y_out ? ar.get<float>((size_t)M * Dout) : y_out;
        });
        // operands as bevgen_finalize prepares them: the GEGLU row order of W1, W4 zero-padded to Fpad columns, and (folded forms) W4 o gamma3 with its row sums
        launch_split_weight(x, xp, (long)M * D, s);
        launch_geglu_weight_order(w1, w1o, F, Fpad, D, s);
        launch_split_weight(w1o, w1p, 2L * Fpad * D, s);
        launch_pad_rows(w4, F, w4pad, Fpad, Dout, F, s);
        if (level >= 1) launch_ln_fold_weight(w4pad, gamma3, w4g, cs, Dout, Fpad, F, s);
        const float* w4u = level >= 1 ? w4g : w4pad;
        launch_split_weight(w4u, w4p, (long)Dout * Fpad, s);
        // up-projection with GEGLU in its epilogue (muse.cpp feed_forward_split)
        GemmArgs ge;
        ge.A_hi = xp; ge.A_lo = xp + 32; ge.B = w1o; ge.B_hi = w1p; ge.B_lo = w1p + 32;
        ge.M = M; ge.N = 2 * Fpad; ge.K = D; ge.lda = D; ge.ldb = D; ge.ldc = Fpad;
        ge.C = h; ge.epi = EPI_GEGLU; ge.force_wm = block;
        if (level >= 1) { ge.ln_out_planes = gp; ge.ln_out_stats = gs; ge.ln_out_ld = Fpad; ge.ln_rows = M; }
        launch_gemm_split_glds(ge, s);
        if (level == 0) launch_layernorm_planes(h, Fpad, gamma3, nullptr, gp, Fpad, M, F, 1e-5f, s);
        // down-projection + residual
        GemmArgs gd;
        gd.A_hi = reinterpret_cast<const uint16_t*>(gp); gd.A_lo = gd.A_hi + 32; gd.B = w4u; gd.B_hi = w4p; gd.B_lo = w4p + 32;
        gd.M = M; gd.N = Dout; gd.K = Fpad; gd.lda = Fpad; gd.ldb = Fpad; gd.ldc = Dout; gd.ldr = Dout;
        gd.C = y; gd.R = residual; gd.force_wm = block;
        if (level >= 1) {
            gd.ln_in_cs = cs; gd.ln_rows = M;
            if (merge == 0) { launch_ln_stats_finalize(gs, rs, M, GF, F, 1e-5f, s); gd.ln_in_stats = rs; }
            else { gd.ln_in_gsums = gs; gd.ln_in_groups = GF; gd.ln_in_count = F; }
        }
        if (level == 2) { gd.ln_out_planes = yp; gd.ln_out_stats = ys; gd.ln_out_ld = Dout; gd.ln_rows = M; }
        launch_gemm_split_glds(gd, s);
    });
}

int bevgen_op_layernorm_planes(bevgen_ctx* ctx, const float* x, int ldx, const float* gamma, const float* beta, void* planes, int ldy, int rows, int D, int geglu, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && gamma && planes && rows >= 1 && D >= 1 && ldy >= D && ldy % 32 == 0, "op_layernorm_planes: bad arguments");
        if (geglu) {
            BG_REQUIRE(!beta && ldx >= 2 * D, "op_layernorm_planes: the GEGLU form has no beta and reads rows of 2 D columns (ldx=%d D=%d)", ldx, D);
            launch_geglu_layernorm_planes(x, ldx, gamma, planes, ldy, rows, D, 1e-5f, (hipStream_t)stream);
        } else {
            BG_REQUIRE(ldx >= D, "op_layernorm_planes: ldx=%d < D=%d", ldx, D);
            launch_layernorm_planes(x, ldx, gamma, beta, planes, ldy, rows, D, 1e-5f, (hipStream_t)stream);
        }
    });
}

int bevgen_op_ln_gemm(bevgen_ctx* ctx, const float* a, const float* ln_w, const float* ln_b, float eps, const float* w, const float* bias, float* c, int M, int N, int K,
                      int act_gelu, int ksplit, int* ksplit_out, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(skinny_fused_supported(M, N, K, ln_w != nullptr), "op_ln_gemm: unsupported shape M=%d N=%d K=%d", M, N, K);
        SkinnyFusedArgs g;
        g.A = a; g.lda = K; g.ln_w = ln_w; g.ln_b = ln_b; g.eps = eps;
        // a context created with decode_weight_dtype = i8 runs the operator on the int8 image of `w` (the model that mode defines: code * scale per row); the
        // fold constants below then come from the dequantised matrix, as bevgen_finalize takes them
        const bool wi8 = ctx->cfg.decode_weight_dtype == BEVGEN_W_I8;
        float *wp, *cs, *ds, *sc, *wdq;
        ctx->arena.carve([&](Arena& ar) {
            wp = wi8 ? reinterpret_cast<float*>(ar.alloc(skinny_packed_bytes_i8(N, K))) : ar.get<float>(skinny_packed_floats(N, K));
            cs = ksplit == -1 ? ar.get<float>((size_t)N) : nullptr;
            ds = ksplit == -1 ? ar.get<float>((size_t)N) : nullptr;
            sc = wi8 ? ar.get<float>((size_t)N) : nullptr;
            wdq = wi8 && ksplit == -1 ? ar.get<float>((size_t)N * K) : nullptr;
        });
        if (wi8) {
            const int kw = K / (ksplit > 0 ? ksplit : (ln_w ? 1 : skinny_fused_ksplit(N, K)));
            BG_REQUIRE(kw % (SF_WAVES * 32) == 0, "op_ln_gemm: int8 weights need a K slice that is a multiple of %d (K=%d)", SF_WAVES * 32, K);
            launch_pack_skinny_weight_i8(w, wp, sc, N, K, (hipStream_t)stream);
            if (wdq) { launch_quantize_rows_i8(w, N, K, nullptr, nullptr, wdq, (hipStream_t)stream); w = wdq; }
            g.w_f16 = 2; g.w_scale = sc;
        } else {
            launch_pack_skinny_weight(w, wp, N, K, (hipStream_t)stream);
        }
        g.Wp = wp; g.bias = bias; g.C = c; g.ldc = N;
        g.M = M; g.N = N; g.K = K; g.act = act_gelu ? ACT_GELU : ACT_NONE;
        g.ksplit = ksplit > 0 ? ksplit : (ln_w ? 1 : skinny_fused_ksplit(N, K));
        if (ksplit == -1) {   // the form the decode step launches for ln2 + MLP-up: LayerNorm folded into the product, row constants from launch_ar_ln_fold
            BG_REQUIRE(ln_w && ln_b && bias, "op_ln_gemm: ksplit = -1 (folded LayerNorm) needs gamma, beta and a bias");
            launch_ar_ln_fold(w, bias, ln_w, ln_b, cs, ds, N, K, (hipStream_t)stream);
            g.ln_cs = cs; g.ln_ds = ds;
        }
        if (ksplit_out) *ksplit_out = g.ksplit;
        g.trace = ctx->trace ? ctx->trace + 4096 * 8 : nullptr;
        launch_skinny_fused(g, (hipStream_t)stream);
    });
}

int bevgen_op_quantize_rows_i8(bevgen_ctx* ctx, const float* w, int N, int K, void* codes, float* scales, float* dequant, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(w && N >= 1 && K >= 1 && codes && scales, "op_quantize_rows_i8: bad arguments");
        launch_quantize_rows_i8(w, N, K, codes, scales, dequant, (hipStream_t)stream);
    });
}

int bevgen_op_mlp_fused(bevgen_ctx* ctx, const float* x, const float* ln_w, const float* ln_b, float eps, const float* w1, const float* b1, const float* w2, const float* b2,
                        int w_f16, float* out, int M, int D, void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        BG_REQUIRE(x && ln_w && ln_b && w1 && b1 && w2 && b2 && out, "op_mlp_fused: missing operand");
        BG_REQUIRE(w_f16 >= 0 && w_f16 <= 2, "op_mlp_fused: w_f16 = %d (0 fp32, 1 fp16, 2 int8 weights)", w_f16);
        BG_REQUIRE(mlp_fused_supported(M, D, w_f16 != 0), "op_mlp_fused: unsupported shape M=%d D=%d (or a device with fewer CUs than workgroups / BEVGEN_MLP_FUSE=0)", M, D);
        const size_t eb = w_f16 == 2 ? 1 : w_f16 ? sizeof(_Float16) : sizeof(float);   // (skinny_packed_bytes_i8 == skinny_packed_floats: one byte per element)
        void *w1p, *w2p;
        float *cs, *ds, *hidden, *part, *zero, *w1r, *w2r, *sc1, *sc2;
        unsigned* sync;
        ctx->arena.carve([&](Arena& ar) {
            w1p = ar.alloc(skinny_packed_floats(4 * D, D) * eb);
            w2p = ar.alloc(skinny_packed_floats(D, 4 * D) * eb);
            cs = ar.get<float>((size_t)4 * D);
            ds = ar.get<float>((size_t)4 * D);
            hidden = ar.get<float>((size_t)M * 4 * D);
            part = ar.get<float>((size_t)MLP_FUSED_PLANES * M * D);
            zero = ar.get<float>((size_t)M * D);
            sync = ar.get<unsigned>(mlp_fused_sync_words());
            w1r = w_f16 ? ar.get<float>((size_t)4 * D * D) : nullptr;
            w2r = w_f16 == 1 ? ar.get<float>((size_t)4 * D * D) : nullptr;
            sc1 = w_f16 == 2 ? ar.get<float>((size_t)4 * D) : nullptr;
            sc2 = w_f16 == 2 ? ar.get<float>((size_t)D) : nullptr;
        });
        const float *w1u = w1, *w2u = w2;
        if (w_f16 == 2) {   // the model decode_weights = i8 defines: code * scale per row (the row constants of the folded ln2 from the dequantised up matrix)
            launch_pack_skinny_weight_i8(w1, w1p, sc1, 4 * D, D, s);
            launch_pack_skinny_weight_i8(w2, w2p, sc2, D, 4 * D, s);
            launch_quantize_rows_i8(w1, 4 * D, D, nullptr, nullptr, w1r, s);
            w1u = w1r;
        } else if (w_f16) {   // the model decode_weights = f16 defines: matrices rounded to fp16-representable values (row constants from the rounded matrix, as bevgen_finalize does)
            HIP_CHECK(hipMemcpyAsync(w1r, w1, (size_t)4 * D * D * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(w2r, w2, (size_t)4 * D * D * sizeof(float), hipMemcpyDeviceToDevice, s));
            launch_round_to_f16(w1r, nullptr, (long)4 * D * D, s);
            launch_round_to_f16(w2r, nullptr, (long)4 * D * D, s);
            w1u = w1r; w2u = w2r;
            launch_pack_skinny_weight_f16(w1u, w1p, 4 * D, D, s);
            launch_pack_skinny_weight_f16(w2u, w2p, D, 4 * D, s);
        } else {
            launch_pack_skinny_weight(w1u, reinterpret_cast<float*>(w1p), 4 * D, D, s);
            launch_pack_skinny_weight(w2u, reinterpret_cast<float*>(w2p), D, 4 * D, s);
        }
        launch_ar_ln_fold(w1u, b1, ln_w, ln_b, cs, ds, 4 * D, D, s);
        HIP_CHECK(hipMemsetAsync(zero, 0, (size_t)M * D * sizeof(float), s));
        HIP_CHECK(hipMemsetAsync(sync, 0, mlp_fused_sync_words() * sizeof(unsigned), s));
        MlpFusedArgs g;
        g.A = x; g.lda = D; g.ln_w = ln_w; g.ln_cs = cs; g.ln_ds = ds; g.eps = eps;
        g.Wup = reinterpret_cast<const float*>(w1p); g.Wdn = reinterpret_cast<const float*>(w2p); g.w_f16 = w_f16; g.Wup_sc = sc1; g.Wdn_sc = sc2;
        g.hidden = hidden; g.C = part; g.sync = sync; g.err = ctx->status_dev; g.M = M; g.D = D;
        g.trace = ctx->trace ? ctx->trace + 4096 * 8 : nullptr;
        // (twice: the second launch runs on the barrier state the first one left behind - the self-cleaning property the hipGraph replay of the decode step relies on)
        launch_ar_mlp_fused(g, s);
        launch_ar_mlp_fused(g, s);
        RowSrc r;
        r.base = zero; r.ld = D; r.partial = part; r.ns = MLP_FUSED_PLANES; r.pstride = (long)M * D; r.pld = D; r.bias = b2;
        launch_rowsrc_materialize(r, out, M, D, nullptr, s);
        HIP_CHECK(hipStreamSynchronize(s));
        ctx->check_status("op_mlp_fused");
    });
}

int bevgen_op_remask(bevgen_ctx* ctx, int64_t* ids, const float* scores, const int64_t* init_ids, int rows, int T, int n_mask, int64_t mask_id, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(ids && scores && rows >= 1 && T >= 1, "op_remask: bad arguments");
        launch_remask(ids, scores, init_ids, rows, T, n_mask, mask_id, (hipStream_t)stream);
    });
}

int bevgen_op_maskgit_pick(bevgen_ctx* ctx, int64_t* ids, const float* logits, int ldl, const float* gumbel_u, int rows, int V, int k, float temperature, int64_t mask_id,
                           unsigned long long seed, unsigned iter, float* conf_scores, int conf_mode, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(ids && logits && rows >= 1 && V >= 1 && ldl >= V, "op_maskgit_pick: bad arguments");
        launch_maskgit_pick(ids, logits, ldl, gumbel_u, rows, V, k, temperature, mask_id, (hipStream_t)stream, seed, iter, conf_scores, conf_mode);
    });
}

int bevgen_op_critic_scores(bevgen_ctx* ctx, const float* embed, int lde, const float* w, const float* b, const float* u, float noise_scale, float frac,
                            unsigned long long seed, unsigned iter, float* scores, int rows, int D, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(embed && w && b && scores && rows >= 1 && D >= 1 && lde >= D, "op_critic_scores: bad arguments");
        launch_critic_scores(embed, lde, w, b, u, noise_scale, frac, scores, rows, D, (hipStream_t)stream, seed, iter);
    });
}

int bevgen_op_ar_pick(bevgen_ctx* ctx, const float* logits, int ldl, const float* u, const int* d_step, const int64_t* forced, int64_t* out, int rows, int V, int top_k,
                      float temperature, int64_t* out_all, const int64_t* fwd_idx, int N, const float* tok_emb, const float* img_embed, const float* pos_emb, float* x, int C, int T,
                      int D, int vocab_rows, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(logits && out && rows >= 1 && V >= 1 && ldl >= V, "op_ar_pick: bad arguments");
        BG_REQUIRE(!out_all || (fwd_idx && N >= 1), "op_ar_pick: out_all needs fwd_idx and N");
        BG_REQUIRE(!x || (out_all && tok_emb && pos_emb && vocab_rows >= 1 && D >= 1), "op_ar_pick: x needs out_all, tok_emb, pos_emb and vocab_rows");
        ArPickTail tail;
        tail.out_all = out_all; tail.fwd_idx = fwd_idx; tail.N = N;
        tail.tok_emb = tok_emb; tail.img_embed = img_embed; tail.pos_emb = pos_emb; tail.x = x;
        tail.C = C; tail.T = T; tail.D = D; tail.vocab_rows = vocab_rows;
        launch_ar_pick(logits, ldl, u, d_step, forced, out, rows, V, top_k, temperature, (hipStream_t)stream, out_all ? &tail : nullptr);
    });
}

int bevgen_op_ar_score_rows(bevgen_ctx* ctx, const float* logits, int ldl, const int64_t* target, const float* weight, const int64_t* fwd_idx, int b, int s0, int rows, int N,
                            int V, float* nll, float* wnll, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(logits && V >= 1 && ldl >= V && b >= 0 && (!target || fwd_idx), "op_ar_score_rows: bad arguments");
        launch_ar_score_rows(logits, ldl, target, weight, fwd_idx, b, s0, rows, N, V, nll, wnll, (hipStream_t)stream);
    });
}

int bevgen_op_mean_fixed_order(bevgen_ctx* ctx, const float* x, long n, float* out, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && out && n >= 1, "op_mean_fixed_order: bad arguments");
        launch_mean_fixed_order(x, n, out, (hipStream_t)stream);
    });
}

int bevgen_op_layernorm(bevgen_ctx* ctx, const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, void* stream) {
    return guarded(ctx, [&] { launch_layernorm(x, D, gamma, beta, y, D, rows, D, eps, (hipStream_t)stream); });
}

int bevgen_op_add_row_layernorm(bevgen_ctx* ctx, float* x, int ldx, const float* r, const float* gamma, void* y, int ldy, int rows, int D, int planes, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && r && gamma && y && rows >= 1 && D >= 1, "op_add_row_layernorm: bad arguments");
        launch_add_row_layernorm(x, ldx, r, gamma, y, ldy, rows, D, 1e-5f, planes != 0, (hipStream_t)stream);
    });
}

int bevgen_op_cfg_combine(bevgen_ctx* ctx, float* cond, int ldc, const float* null_logits, int ldn, long rows, int V, float cond_scale, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(cond && null_logits && rows >= 1 && V >= 1, "op_cfg_combine: bad arguments");
        launch_cfg_combine(cond, ldc, null_logits, ldn, rows, V, cond_scale, (hipStream_t)stream);
    });
}

int bevgen_op_geglu_layernorm(bevgen_ctx* ctx, const float* h, const float* gamma, float* y, int rows, int F, int ldy, void* stream) {
    return guarded(ctx, [&] { launch_geglu_layernorm(h, 2 * F, gamma, y, ldy, rows, F, 1e-5f, (hipStream_t)stream); });
}

int bevgen_op_attention(bevgen_ctx* ctx, const float* q, const float* k, const float* v, const float* bias, int ldbias, int B, int H, int Nq, int Nk_pad, float scale,
                        float* out, void* stream) {
    return bevgen_op_attention_ex(ctx, q, k, v, bias, ldbias, B, H, Nq, Nk_pad, scale, 1, out, stream);
}

int bevgen_op_attention_ex(bevgen_ctx* ctx, const float* q, const float* k, const float* v, const float* bias, int ldbias, int B, int H, int Nq, int Nk_pad, float scale,
                           int key_splits, float* out, void* stream) {
    return guarded(ctx, [&] {
        if (ctx->cfg.precision == BEVGEN_PRECISION_F16X3) {
            // the split-precision flash-attention kernel of Route M on caller-supplied fp32 operands: operand images and the packed bias are built here
            BG_REQUIRE(Nk_pad % 32 == 0 && (bias == nullptr || (ldbias % 4 == 0 && ldbias >= Nk_pad)), "op_attention (split precision): Nk_pad %% 32, bias row stride %% 4 and >= Nk_pad");
            hipStream_t s = (hipStream_t)stream;
            const size_t nq = (size_t)B * H * Nq * 64, nk = (size_t)B * H * Nk_pad * 64;
            const size_t bpk = bias ? (size_t)attn_bias_packed_floats(Nq, Nk_pad) : 0, braw = bias ? (size_t)Nq * ldbias : 0;
            BG_REQUIRE(key_splits >= 1 && key_splits <= 8 && Nk_pad / 32 >= key_splits, "op_attention: key_splits=%d out of range for Nk_pad=%d", key_splits, Nk_pad);
            const size_t kws = key_splits > 1 ? (size_t)attn_split_ws_floats(B, H, Nq, key_splits) : 0;
            _Float16 *Qp, *Kp, *Vp;
            float *b2, *pk;
            AttnSplitArgs sa{};
            ctx->arena.carve([&](Arena& ar) {
                Qp = ar.get<_Float16>(nq * 2);
                Kp = ar.get<_Float16>(nk * 2);
                Vp = ar.get<_Float16>(nk * 2);
                b2 = bias ? ar.get<float>(braw) : nullptr;
                pk = bias ? ar.get<float>(bpk) : nullptr;
                sa.kws = key_splits > 1 ? ar.get<float>(kws) : nullptr;
            });
            launch_attn_split_operands(q, k, v, Qp, Qp + nq, Kp, Kp + nk, Vp, Vp + nk, B, H, Nq, Nk_pad, scale * kLog2e, s);
            sa.Qh = Qp; sa.Ql = Qp + nq; sa.Kh = Kp; sa.Kl = Kp + nk; sa.VTh = Vp; sa.VTl = Vp + nk;
            if (bias) {
                HIP_CHECK(hipMemcpyAsync(b2, bias, braw * 4, hipMemcpyDeviceToDevice, s));
                launch_scale(b2, (long)braw, kLog2e, s);
                launch_pack_attn_bias(b2, ldbias, Nq, Nk_pad, pk, s);
                sa.bias = b2; sa.bias_pk = pk; sa.ldbias = ldbias;
            }
            sa.bias_head_stride = 0;
            if (key_splits > 1) sa.ksplit = key_splits;
            sa.O = out; sa.Op = nullptr; sa.B = B; sa.H = H; sa.Nq = Nq; sa.Nk_pad = Nk_pad; sa.scale = scale * kLog2e;
            sa.o_bstride = (long)Nq * H * 64; sa.o_qstride = (long)H * 64; sa.o_hstride = 64;
            launch_attention_split(sa, s);
            return;
        }
        AttnArgs a{};
        a.Q = q; a.K = k; a.V = v; a.bias = bias; a.R = nullptr; a.O = out;
        a.B = B; a.H = H; a.Nq = Nq; a.Nk_pad = Nk_pad;
        a.q_bstride = (long)H * Nq * 64; a.q_hstride = (long)Nq * 64;
        a.kv_bstride = (long)H * Nk_pad * 64; a.kv_hstride = (long)Nk_pad * 64;
        a.ldbias = ldbias; a.bias_head_stride = 0; a.scale = scale;
        a.o_bstride = (long)Nq * H * 64; a.o_qstride = (long)H * 64; a.o_hstride = 64;
        launch_attention(a, (hipStream_t)stream);
    });
}

int bevgen_op_muse_attention(bevgen_ctx* ctx, const void* qh, const void* ql, const void* kh, const void* kl, const void* vth, const void* vtl, const float* bias, int ldbias,
                             int B, int H, int Nq, int Nk_pad, int kv_group, int key_splits, float* out, void* out_planes, void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
        BG_REQUIRE(ctx->cfg.precision == BEVGEN_PRECISION_F16X3, "op_muse_attention: needs a split-precision (f16x3) context");
        BG_REQUIRE(qh && ql && kh && kl && vth && vtl && B >= 1 && H >= 1 && Nq >= 1 && Nk_pad >= 32 && Nk_pad % 32 == 0 && (long)B * H * std::max(Nq, Nk_pad) * 64 < (1L << 30),
                   "op_muse_attention: bad arguments (planes Qh / Ql [B,H,Nq,64], Kh / Kl [B/kv_group,H,Nk_pad,64], VTh / VTl [B/kv_group,H,64,Nk_pad], Nk_pad %% 32)");
        BG_REQUIRE(al16(qh) && al16(ql) && al16(kh) && al16(kl) && al16(vth) && al16(vtl) && al16(bias) && al16(out) && al16(out_planes), "op_muse_attention: every pointer must be 16-byte aligned");
        BG_REQUIRE(bias == nullptr || (ldbias % 4 == 0 && ldbias >= Nk_pad), "op_muse_attention: bias row stride %d must be a multiple of 4 and >= Nk_pad = %d", ldbias, Nk_pad);
        BG_REQUIRE(kv_group >= 1 && B % kv_group == 0, "op_muse_attention: batch %d is not a multiple of kv_group %d", B, kv_group);
        BG_REQUIRE(key_splits >= 1 && key_splits <= 8 && key_splits <= Nk_pad / 32, "op_muse_attention: key_splits=%d out of range (1..8, at most Nk_pad / 32 = %d)", key_splits, Nk_pad / 32);
        BG_REQUIRE((out != nullptr) != (out_planes != nullptr), "op_muse_attention: exactly one of d_out and d_out_planes must be given");
        float* pk;
        AttnSplitArgs sa{};
        ctx->arena.carve([&](Arena& ar) {
            pk = bias ? ar.get<float>((size_t)attn_bias_packed_floats(Nq, Nk_pad)) : nullptr;
            sa.kws = key_splits > 1 ? ar.get<float>((size_t)attn_split_ws_floats(B, H, Nq, key_splits)) : nullptr;
        });
        if (bias) launch_pack_attn_bias(bias, ldbias, Nq, Nk_pad, pk, s);
        // (muse.cpp attn_args, self_attention_split / cross_attention_split)
        sa.Qh = reinterpret_cast<const _Float16*>(qh); sa.Ql = reinterpret_cast<const _Float16*>(ql);
        sa.Kh = reinterpret_cast<const _Float16*>(kh); sa.Kl = reinterpret_cast<const _Float16*>(kl);
        sa.VTh = reinterpret_cast<const _Float16*>(vth); sa.VTl = reinterpret_cast<const _Float16*>(vtl);
        sa.bias = bias; sa.bias_pk = pk; sa.ldbias = ldbias; sa.bias_head_stride = 0;
        sa.O = out; sa.Op = reinterpret_cast<_Float16*>(out_planes);
        sa.B = B; sa.H = H; sa.Nq = Nq; sa.Nk_pad = Nk_pad; sa.scale = 8.0f * kLog2e;
        sa.o_bstride = (long)Nq * H * 64; sa.o_qstride = (long)H * 64; sa.o_hstride = 64;
        sa.kv_group = kv_group;
        sa.ksplit = key_splits;
        launch_attention_split(sa, s);
    });
}

int bevgen_op_decode_attention(bevgen_ctx* ctx, const float* q, const void* kc, const void* vc, int kv_dtype, const float* bias, int ldbias, const uint8_t* keep,
                               int ldkeep, long keep_head_stride, int B, int H, int n, int Lmax, float scale, float* out, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(kv_dtype >= 0 && kv_dtype <= 2, "op_decode_attention: kv_dtype %d", kv_dtype);
        DecodeAttnArgs a;
        a.q = q; a.ldq = H * 64; a.kcache = kc; a.vcache = vc; a.kv_dtype = kv_dtype;
        a.bias = bias; a.ldbias = ldbias;
        a.vis.allowed = keep; a.vis.ldallowed = ldkeep; a.vis.allowed_head_stride = keep_head_stride;   // a dense per-head plane is an element mask with a head stride
        a.O = out; a.ldo = H * 64; a.B = B; a.H = H; a.n = n; a.Lmax = Lmax; a.scale = scale;
        const int S = decode_attention_splits(a.B, a.H, a.n);
        float* ws;
        ctx->arena.carve([&](Arena& ar) { ws = reinterpret_cast<float*>(ar.alloc(decode_attention_ws_bytes(a.B, a.H, S))); });
        launch_decode_attention_ws(a, ws, S, (hipStream_t)stream);
    });
}

int bevgen_op_ar_attn_fused(bevgen_ctx* ctx, const float* x, const float* partial, int ns, const float* rbias, const float* ln_w, const float* ln_b, const float* wqkv,
                            const float* bqkv, int w_f16, void* kc, void* vc, int kv_dtype, const float* bias, int ldbias, const float* attn_mask, const int64_t* layout,
                            int block, int B, int G, int H, int n, int Lmax, int prefix, int split, float* out, void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        const int D = H * 64, L = Lmax;
        BG_REQUIRE(x && ln_w && ln_b && wqkv && bqkv && kc && vc && out && n >= 1 && n <= Lmax && kv_dtype >= 0 && kv_dtype <= 2, "op_ar_attn_fused: bad arguments");
        BG_REQUIRE(w_f16 >= 0 && w_f16 <= 2, "op_ar_attn_fused: w_f16 = %d (0 fp32, 1 fp16, 2 int8 weights)", w_f16);
        BG_REQUIRE(ar_attn_fused_supported(B, G, D, H), "op_ar_attn_fused: unsupported shape B=%d G=%d D=%d H=%d", B, G, D, H);
        BG_REQUIRE(!layout || (block >= 1 && L % block == 0), "op_ar_attn_fused: Lmax %d is not a multiple of the block size %d", L, block);
        const int nb = layout ? L / block : 0, cld = (int)cdiv(L, 16) + 1;
        ArAttnFusedArgs a;
        if (split == -1) { a.stage_cap = 0; split = 0; }                       // the fused kernel without K/V pieces staged in LDS
        void* h;
        float *tmp, *cs, *ds, *wp, *qkv, *xn, *sc;
        uint8_t *al, *lay;
        uint16_t* ch;
        ctx->arena.carve([&](Arena& ar) {
            h = w_f16 ? ar.alloc((size_t)3 * D * D * 2) : nullptr;   // (int8: the codes take half of it)
            sc = w_f16 == 2 ? ar.get<float>((size_t)3 * D) : nullptr;
            tmp = w_f16 ? ar.get<float>((size_t)3 * D * D) : nullptr;   // round_to_f16 rounds in place: work on a copy of the caller's matrix (arena: no allocation, no sync)
            cs = ar.get<float>((size_t)3 * D);   // row constants of the folded ln1
            ds = ar.get<float>((size_t)3 * D);
            al = attn_mask ? ar.get<uint8_t>((size_t)L * L) : nullptr;
            lay = layout ? ar.get<uint8_t>((size_t)H * nb * nb) : nullptr;
            ch = layout ? ar.get<uint16_t>((size_t)H * nb * cld) : nullptr;
            wp = split ? ar.get<float>(skinny_packed_floats(3 * D, D)) : nullptr;
            qkv = split ? ar.get<float>((size_t)B * 3 * D) : nullptr;
            xn = split ? ar.get<float>((size_t)B * D) : nullptr;
            a.kws = split > 1 ? ar.get<float>((size_t)B * H * split * 66) : nullptr;   // split = k > 1: the partial states of the k key ranges
        });
        a.x.base = x; a.x.ld = D;
        if (partial && ns > 0) { a.x.partial = partial; a.x.ns = ns; a.x.pstride = (long)B * D; a.x.pld = D; }
        a.x.bias = rbias;
        a.ln_w = ln_w; a.ln_b = ln_b; a.wqkv = wqkv; a.bqkv = bqkv;
        const float* w_rounded = nullptr;
        if (w_f16 == 2) {   // codes, scales and the dequantised matrix (fold constants) in one pass over the caller's matrix
            launch_quantize_rows_i8(wqkv, 3 * D, D, h, sc, tmp, s);
            a.wqkv_h = h; a.wqkv_sc = sc;
            w_rounded = tmp;
        } else if (w_f16) {
            HIP_CHECK(hipMemcpyAsync(tmp, wqkv, (size_t)3 * D * D * 4, hipMemcpyDeviceToDevice, s));
            launch_round_to_f16(tmp, h, 3L * D * D, s);
            a.wqkv_h = h;
            w_rounded = tmp;
        }
        // row constants of the folded ln1, on the matrix the kernel multiplies by (the fp16-rounded one with w_f16)
        launch_ar_ln_fold(w_f16 ? w_rounded : wqkv, bqkv, ln_w, ln_b, cs, ds, 3 * D, D, s);
        a.ln_cs = cs; a.ln_ds = ds;
        a.kcache = kc; a.vcache = vc; a.kv_dtype = kv_dtype;
        a.bias = bias; a.ldbias = ldbias;
        if (attn_mask) {
            launch_build_allowed(attn_mask, al, (long)L * L, s);
            a.vis.allowed = al; a.vis.ldallowed = L;
        }
        if (layout) {
            launch_build_layout(layout, lay, ch, H, nb, block, L, cld, s);
            a.vis.lay = lay; a.vis.lay_head_stride = (long)nb * nb; a.vis.nb = nb; a.vis.blk = block;
            a.vis.chunks = ch; a.vis.chunks_head_stride = (long)nb * cld; a.vis.chunks_ld = cld;
        }
        a.out = out; a.ldo = D;
        a.B = B; a.G = G; a.H = H; a.D = D; a.Lmax = Lmax; a.n = n; a.prefix = prefix; a.scale = 0.125f;
        a.trace = ctx->trace;
        if (split) {
            BG_REQUIRE(skinny_fused_supported(B, 3 * D, D, true) && (!w_f16 || skinny_fused_f16_ok(3 * D, D, true)), "op_ar_attn_fused: the split form does not support B=%d D=%d", B, D);
            if (w_f16 == 2) launch_pack_skinny_weight_i8(wqkv, wp, sc, 3 * D, D, s);   // (the same scales again)
            else if (w_f16) launch_pack_skinny_weight_f16(wqkv, wp, 3 * D, D, s);   // rounds to fp16 while packing
            else launch_pack_skinny_weight(wqkv, wp, 3 * D, D, s);
            SkinnyFusedArgs pq;
            const RowSrc src = a.x;
            pq.a_src = &src;
            pq.ln_w = ln_w; pq.ln_b = ln_b; pq.Wp = wp; pq.w_f16 = w_f16; pq.w_scale = sc; pq.bias = bqkv;
            pq.C = qkv; pq.ldc = 3 * D; pq.xn_out = xn; pq.ldxn = D;
            pq.M = B; pq.N = 3 * D; pq.K = D; pq.ksplit = 1;
            launch_skinny_fused(pq, s);
            a.qkv = qkv; a.xn = xn;
            if (split > 1) {   // split = k > 1: the attention-only kernel with its key walk cut into k ranges (one sequence per workgroup)
                BG_REQUIRE(G == 1, "op_ar_attn_fused: a key split needs G = 1");
                a.ksplit = split;
            }
        }
        launch_ar_attn_fused(a, s);
    });
}

static int op_conv3x3_act(bevgen_ctx* ctx, const float* x, const float* w, const float* bias, const float* residual, float* y, int n, int H, int W, int Cin, int Cout,
                          int up, int act, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(act == 0 || act == 1, "op_conv3x3_act: act %d (0 = none, 1 = ReLU)", act);
        GemmArgs g;
        g.act = act ? ACT_RELU : ACT_NONE;
        const int flags = up;   // bit 0: nearest-2x upsample fused into the gather; bit 1: the LDS-DMA kernel on operand planes split here (tests / probes: the model hands it
        up &= 1;                // planes its GroupNorm wrote); bit 2 (with bit 1): the general convolution variant also where the stride-1 one (MODE_CONV3S) applies
        const int oh = up ? 2 * H : H, ow = up ? 2 * W : W;
        g.mode = MODE_CONV3;
        g.A = x; g.B = w; g.C = y; g.R = residual; g.bias_n = bias;
        g.M = n * oh * ow; g.N = Cout; g.K = 9 * Cin; g.lda = Cin; g.ldb = 9 * Cin; g.ldc = Cout; g.ldr = Cout;
        g.conv_h = oh; g.conv_w = ow; g.conv_cin = Cin; g.conv_up = up;
        if (flags & 2) {
            BG_REQUIRE(Cin % 32 == 0, "op_conv3x3: the LDS-DMA kernel needs Cin %% 32 == 0 (Cin=%d)", Cin);
            const size_t xb = (size_t)n * H * W * Cin * 4, wb = (size_t)Cout * 9 * Cin * 4;
            uint16_t *ap, *bp;
            ctx->arena.carve([&](Arena& ar) {
                ap = reinterpret_cast<uint16_t*>(ar.alloc(xb));
                bp = reinterpret_cast<uint16_t*>(ar.alloc(wb));
            });
            launch_split_weight(x, ap, (long)n * H * W * Cin, (hipStream_t)stream);
            launch_split_weight(w, bp, (long)Cout * 9 * Cin, (hipStream_t)stream);
            g.A = nullptr; g.A_hi = ap; g.A_lo = ap + 32; g.B_hi = bp; g.B_lo = bp + 32;
            g.conv_general = (flags & 4) != 0;
        }
        launch_gemm(g, (hipStream_t)stream);
    });
}

int bevgen_op_conv3x3(bevgen_ctx* ctx, const float* x, const float* w, const float* bias, const float* residual, float* y, int n, int H, int W, int Cin, int Cout,
                      int up, void* stream) {
    return op_conv3x3_act(ctx, x, w, bias, residual, y, n, H, W, Cin, Cout, up, 0, stream);
}

int bevgen_op_conv3x3_act(bevgen_ctx* ctx, const float* x, const float* w, const float* bias, const float* residual, float* y, int n, int H, int W, int Cin, int Cout,
                          int up, int act, void* stream) {
    return op_conv3x3_act(ctx, x, w, bias, residual, y, n, H, W, Cin, Cout, up, act, stream);
}

int bevgen_op_maxpool2x2(bevgen_ctx* ctx, const float* x, float* y, void* planes, int n, int H, int W, int C, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && y, "op_maxpool2x2: null argument");
        launch_maxpool2x2(x, y, planes, n, H, W, C, (hipStream_t)stream);
    });
}

int bevgen_op_lpips_tap(bevgen_ctx* ctx, const float* fa, const float* fb, const float* w, int n, int pixels, int C, double* out, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(fa && fb && w && out && n >= 1 && pixels >= 1, "op_lpips_tap: bad arguments");
        BG_REQUIRE(C == 64 || C == 128 || C == 256 || C == 512, "op_lpips_tap: C=%d (the VGG16 taps have 64, 128, 256 or 512 channels)", C);
        double* partial;
        ctx->arena.carve([&](Arena& ar) { partial = ar.get<double>((size_t)n * lpips_tap_blocks(pixels, C)); });
        launch_lpips_tap(fa, fb, w, n, pixels, C, partial, out, 1, (hipStream_t)stream);
    });
}

int bevgen_lpips_prepare(bevgen_ctx* ctx, const float* const* w, const float* const* bias, const float* const* lin, const float* shift, const float* scale, void* prepared,
                         void* stream) {
    return guarded(ctx, [&] { lpips_prepare(ctx->cfg.precision != BEVGEN_PRECISION_FP32, w, bias, lin, shift, scale, prepared, (hipStream_t)stream); });
}

int bevgen_lpips(bevgen_ctx* ctx, const void* prepared, const void* a, const void* b, int dtype, int n, int H, int W, int normalize, double* out, double* layers, void* work,
                 void* stream) {
    return guarded(ctx, [&] { lpips_run(ctx->cfg.precision != BEVGEN_PRECISION_FP32, prepared, a, b, dtype, n, H, W, normalize, out, layers, work, (hipStream_t)stream); });
}

int bevgen_op_groupnorm(bevgen_ctx* ctx, const float* x, const float* gamma, const float* beta, float* y, int n, int hw, int C, int swish, void* stream) {
    return guarded(ctx, [&] {
        float* stats;
        void* ws;
        ctx->arena.carve([&](Arena& ar) {
            stats = ar.get<float>((size_t)n * 64);
            ws = ar.alloc(groupnorm_ws_bytes(n, hw));
        });
        launch_groupnorm_stats(x, stats, ws, n, hw, C, 1e-6f, (hipStream_t)stream);
        launch_groupnorm_apply(x, stats, gamma, beta, y, n, hw, C, swish, (hipStream_t)stream);
    });
}

int bevgen_op_range_split(bevgen_ctx* ctx, const float* x, int n, int hw, int C, void* planes, int32_t* d_exp, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && planes && d_exp && n >= 1 && hw >= 1 && C >= 32 && C % 32 == 0, "op_range_split: bad arguments (C must be a multiple of 32)");
        hipStream_t s = (hipStream_t)stream;
        unsigned* amax;
        ctx->arena.carve([&](Arena& ar) { amax = ar.get<unsigned>(1); });
        HIP_CHECK(hipMemsetAsync(amax, 0, sizeof(unsigned), s));
        launch_range_exponent(x, (long)n * hw * C, amax, d_exp, s);
        launch_range_split(x, planes, (long)n * hw, C, d_exp, s);
    });
}

int bevgen_op_conv3x3_down(bevgen_ctx* ctx, const float* x, const float* w, const float* bias, float* y, int n, int H, int W, int Cin, int Cout, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && w && y, "op_conv3x3_down: null argument");
        vq_op_conv3x3_down(*ctx, x, w, bias, y, n, H, W, Cin, Cout, (hipStream_t)stream);
    });
}

int bevgen_op_vq_attn_block(bevgen_ctx* ctx, const float* x, const float* norm_w, const float* norm_b, const float* wq, const float* bq, const float* wk, const float* bk,
                            const float* wv, const float* bv, const float* wp, const float* bp, float* y, int n, int h, int w, int C, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && norm_w && norm_b && wq && bq && wk && bk && wv && bv && wp && bp && y, "op_vq_attn_block: null argument");
        vq_op_attn_block(*ctx, x, norm_w, norm_b, wq, bq, wk, bk, wv, bv, wp, bp, y, n, h, w, C, (hipStream_t)stream);
    });
}

int bevgen_op_vq_out_tail(bevgen_ctx* ctx, const float* x, const float* norm_w, const float* norm_b, const float* w, const float* bias, const float* mean, const float* stdv,
                          int out_mode, int three_kernels, void* out, int n, int H, int W, int C, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && norm_w && norm_b && w && out, "op_vq_out_tail: null argument");
        vq_op_out_tail(*ctx, x, norm_w, norm_b, w, bias, mean, stdv, out_mode, three_kernels, out, n, H, W, C, 3, (hipStream_t)stream);
    });
}

int bevgen_op_vq_out_tail_ex(bevgen_ctx* ctx, const float* x, const float* norm_w, const float* norm_b, const float* w, const float* bias, const float* mean, const float* stdv,
                             int out_mode, int three_kernels, void* out, int n, int H, int W, int C, int cout, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && norm_w && norm_b && w && out, "op_vq_out_tail: null argument");
        vq_op_out_tail(*ctx, x, norm_w, norm_b, w, bias, mean, stdv, out_mode, three_kernels, out, n, H, W, C, cout, (hipStream_t)stream);
    });
}

int bevgen_op_bce_logits(bevgen_ctx* ctx, const float* logits, const float* target, long count, const float* qloss, float codebook_weight, float* out, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(logits && target && out && count >= 1, "op_bce_logits: bad arguments");
        double* partial;
        ctx->arena.carve([&](Arena& ar) { partial = ar.get<double>((size_t)bce_logits_blocks(count)); });
        launch_bce_logits(logits, target, count, qloss, codebook_weight, partial, out, (hipStream_t)stream);
    });
}

int bevgen_op_seg_colorize(bevgen_ctx* ctx, const float* x, const float* colorize, int threshold, float* rgb, int n, int C, int H, int W, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && colorize && rgb && x != rgb, "op_seg_colorize: null argument (or the output aliases the input)");
        unsigned* minmax;
        ctx->arena.carve([&](Arena& ar) { minmax = ar.get<unsigned>(2); });
        launch_seg_colorize(x, colorize, threshold, rgb, n, C, H, W, minmax, (hipStream_t)stream);
    });
}

int bevgen_op_image_sqerr(bevgen_ctx* ctx, const void* a, const void* b, int dtype, int n, int C, int H, int W, double* sse, float* minmax, void* work, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(a && b && sse && minmax && work, "op_image_sqerr: null argument");
        launch_image_sqerr(a, b, dtype, n, C, H, W, sse, minmax, work, (hipStream_t)stream);
    });
}

int bevgen_op_ssim(bevgen_ctx* ctx, const void* a, const void* b, int dtype, int n, int C, int H, int W, int kernel_size, double sigma, double data_range, double k1, double k2,
                   double* sums, float* map, void* work, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(a && b && sums && work, "op_ssim: null argument");
        launch_ssim(a, b, dtype, n, C, H, W, kernel_size, sigma, data_range, k1, k2, sums, map, work, (hipStream_t)stream);
    });
}

int bevgen_op_vq_quantize(bevgen_ctx* ctx, const float* z, const float* codebook, int64_t* ids, float* zz, float* ee, long rows, int n_e, int D, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(z && codebook && ids, "op_vq_quantize: null argument");
        vq_op_quantize(*ctx, z, codebook, ids, zz, ee, rows, n_e, D, (hipStream_t)stream);
    });
}

int bevgen_op_vq_geo_embed(bevgen_ctx* ctx, float* h, const float* I_inv, const float* E_inv, const float* plane, const float* wimg, const float* wcam, int n, int T, int D,
                           void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(h && I_inv && E_inv && plane && wimg && wcam, "op_vq_geo_embed: null argument");
        launch_vq_geo_embed(h, I_inv, E_inv, plane, wimg, wcam, n, T, D, (hipStream_t)stream);
    });
}

int bevgen_op_vq_quant_error(bevgen_ctx* ctx, const float* z, const float* codebook, const int64_t* ids, float beta, float* row_err, float* loss, long rows, int n_e, int D,
                             void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(z && codebook && ids && row_err, "op_vq_quant_error: null argument");
        vq_op_quant_error(z, codebook, ids, beta, row_err, loss, rows, n_e, D, (hipStream_t)stream);
    });
}

int bevgen_op_conv3x3_gn_stats(bevgen_ctx* ctx, const float* x, const float* w, const float* bias, int range_route, float* y, float* part, float* stats, int n, int H, int W,
                               int Cin, int Cout, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && w && y && part && stats, "op_conv3x3_gn_stats: null argument");
        vq_op_conv3x3_gn_stats(*ctx, x, w, bias, range_route, y, part, stats, n, H, W, Cin, Cout, (hipStream_t)stream);
    });
}

int bevgen_op_conv_ranged(bevgen_ctx* ctx, const float* x, const float* w, const float* bias, int kind, float* y, int32_t* d_exp, int n, int H, int W, int Cin, int Cout,
                          void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(x && w && bias && y && d_exp, "op_conv_ranged: null argument");
        vq_op_conv_ranged(*ctx, x, w, bias, kind, y, d_exp, n, H, W, Cin, Cout, (hipStream_t)stream);
    });
}

// ---- the kernels around the layer stacks: each entry is the model's launcher on caller buffers (nothing is cleared, nothing staged)
int bevgen_op_camera_embed(bevgen_ctx* ctx, const float* I_inv, const float* E_inv, const float* plane, const float* wimg, const float* wcam, float* img, float* c_embed, int B,
                           int C, int T, int D, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(I_inv && E_inv && plane && wimg && wcam && img && c_embed && B >= 1 && C >= 1 && T >= 1 && D >= 1, "op_camera_embed: bad arguments");
        launch_camera_embed(I_inv, E_inv, plane, wimg, wcam, img, c_embed, B, C, T, D, (hipStream_t)stream);
    });
}

int bevgen_op_cond_embed(bevgen_ctx* ctx, const int64_t* cond_ids, const float* cond_tok, const float* cond_pos, const float* bev_grid, const float* wbev, const float* bbev,
                         const float* bev_cam_pos, const float* c_embed, float* out, int B, int C, int K, int D, int cond_vocab, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(cond_ids && cond_tok && cond_pos && out && B >= 1 && C >= 0 && K >= 1 && D >= 1 && cond_vocab >= 1, "op_cond_embed: bad arguments");
        BG_REQUIRE(!bev_grid || (wbev && bbev && bev_cam_pos && c_embed), "op_cond_embed: the grid form needs bev_embed's weight and bias, bev_cam_pos_emb and c_embed");
        launch_cond_embed(cond_ids, cond_tok, cond_pos, bev_grid, wbev, bbev, bev_cam_pos, c_embed, out, B, C, K, D, cond_vocab, (hipStream_t)stream);
    });
}

int bevgen_op_token_rows(bevgen_ctx* ctx, int kind, const int64_t* ids, const float* table, const float* img, const float* pos, const int64_t* fwd_idx, const int* d_step,
                         void* out, int B, int N, int D, int vocab_rows, int C, int T, int n_steps, int rows_per_seq, int row0, void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        BG_REQUIRE(kind >= 0 && kind <= 4 && out && B >= 1, "op_token_rows: bad arguments");
        float* x = reinterpret_cast<float*>(out);
        if (kind == 0) {
            BG_REQUIRE(ids && table && pos && N >= 1 && D >= 1 && vocab_rows >= 1, "op_token_rows (token_embed): bad arguments");
            launch_token_embed(ids, table, img, pos, x, B, N, D, vocab_rows, s);
        } else if (kind == 1) {
            BG_REQUIRE(ids && table && pos && fwd_idx && d_step && D >= 1 && vocab_rows >= 1 && C >= 1 && T >= 1, "op_token_rows (ar_step_embed): bad arguments");
            launch_ar_step_embed(ids, table, img, pos, fwd_idx, d_step, x, B, C, T, D, vocab_rows, s);
        } else if (kind == 2) {
            BG_REQUIRE(ids && table && pos && fwd_idx && N >= 1 && D >= 1 && vocab_rows >= 1 && row0 >= 0, "op_token_rows (ar_seq_embed): bad arguments");
            launch_ar_seq_embed(ids, table, img, pos, fwd_idx, x, B, n_steps, rows_per_seq, row0, N, D, vocab_rows, s);
        } else if (kind == 3) {
            BG_REQUIRE(table && D >= 1 && row0 >= 0 && row0 < rows_per_seq, "op_token_rows (gather_rows): bad arguments");
            launch_gather_rows(table, x, B, row0, rows_per_seq, D, s);
        } else {
            BG_REQUIRE(ids && fwd_idx && d_step && N >= 1, "op_token_rows (store_tokens): bad arguments");
            launch_store_tokens(ids, fwd_idx, d_step, reinterpret_cast<int64_t*>(out), B, N, s);
        }
    });
}

int bevgen_op_muse_qkv_prep_f32(bevgen_ctx* ctx, const float* qraw, const float* kvraw, const float* null_kv, const float* q_scale, const float* k_scale, float* q, float* k,
                                float* v, int B, int H, int Nq, int Nk, int Nk_pad, void* stream) {
    return guarded(ctx, [&] {
        BG_REQUIRE(B >= 1 && H >= 1 && (qraw || kvraw), "op_muse_qkv_prep_f32: bad arguments");
        BG_REQUIRE(!qraw || (q_scale && q && Nq >= 1), "op_muse_qkv_prep_f32: the query form needs q_scale and d_q");
        BG_REQUIRE(!kvraw || (null_kv && k_scale && k && v && Nk >= 1 && Nk_pad >= Nk + 1), "op_muse_qkv_prep_f32: the key / value form needs null_kv, k_scale, d_k, d_v and Nk_pad >= Nk + 1");
        if (qraw) launch_muse_q_prep(qraw, q_scale, q, B, H, Nq, (hipStream_t)stream);
        if (kvraw) launch_muse_kv_prep(kvraw, null_kv, k_scale, k, v, B, H, Nk, Nk_pad, (hipStream_t)stream);
    });
}

int bevgen_op_kv_cache_write(bevgen_ctx* ctx, int kind, const float* qkv, float* q, void* kc, void* vc, int kv_dtype, int B, int H, int n, int pos0, const int* d_pos, int Lmax,
                             int layers, int rows, int src, int dst0, int count, void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        BG_REQUIRE(kind >= 0 && kind <= 2 && kc && vc && kv_dtype >= 0 && kv_dtype <= 2 && B >= 1 && H >= 1 && Lmax >= 1, "op_kv_cache_write: bad arguments");
        if (kind == 0) {
            BG_REQUIRE(qkv && n >= 1 && pos0 >= 0 && pos0 + n <= Lmax, "op_kv_cache_write (scatter): rows [%d, %d) do not fit Lmax = %d", pos0, pos0 + n, Lmax);
            launch_ar_qkv_scatter(qkv, q, kc, vc, kv_dtype, B, H, n, pos0, Lmax, s);
        } else if (kind == 1) {
            BG_REQUIRE(qkv && d_pos && pos0 >= 0 && pos0 < Lmax, "op_kv_cache_write (append): bad arguments");
            launch_ar_kv_append(qkv, kc, vc, kv_dtype, B, H, pos0, d_pos, Lmax, s);
        } else {
            BG_REQUIRE(layers >= 1 && rows >= 0 && rows <= Lmax && src >= 0 && src < B && dst0 >= 0 && count >= 0 && dst0 + count <= B,
                       "op_kv_cache_write (replicate_prefix): slots [%d, %d) / source %d / %d rows do not fit B = %d, Lmax = %d", dst0, dst0 + count, src, rows, B, Lmax);
            launch_replicate_prefix(kc, vc, layers, B, H, Lmax, rows, src, dst0, count, kv_dtype == 0 ? 4 : kv_dtype == 1 ? 2 : 1, s);
        }
    });
}

int bevgen_op_attn_tables(bevgen_ctx* ctx, int kind, const void* in0, const void* in1, const void* in2, void* out0, void* out1, int heads, int L, int rows, int cols, int blk,
                          int ld0, int ld1, long hs0, long hs1, float scale, void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        const float* f0 = reinterpret_cast<const float*>(in0);
        BG_REQUIRE(kind >= 0 && kind <= 5 && out0, "op_attn_tables: bad arguments");
        if (kind == 0) {
            BG_REQUIRE(L >= 1, "op_attn_tables (attn_bias): bad arguments");
            launch_build_attn_bias(f0, reinterpret_cast<const float*>(in1), reinterpret_cast<float*>(out0), L, s);
        } else if (kind == 1) {
            BG_REQUIRE(in0 && out1 && rows >= 1 && cols >= 1 && L >= rows + cols && ld0 >= 1 && ld1 >= 1, "op_attn_tables (muse_bias): bad arguments");
            launch_build_muse_bias(f0, L, cols, rows, reinterpret_cast<float*>(out0), ld0, reinterpret_cast<float*>(out1), ld1, s);
        } else if (kind == 2) {
            BG_REQUIRE(in0 && rows >= 1 && cols >= 1, "op_attn_tables (allowed): bad arguments");
            launch_build_allowed(f0, reinterpret_cast<uint8_t*>(out0), (long)rows * cols, s);
        } else if (kind == 3) {
            BG_REQUIRE(in0 && out1 && heads >= 1 && blk >= 1 && L >= 1 && L % blk == 0 && ld1 >= (L + 15) / 16 + 1, "op_attn_tables (layout): bad arguments");
            launch_build_layout(reinterpret_cast<const int64_t*>(in0), reinterpret_cast<uint8_t*>(out0), reinterpret_cast<uint16_t*>(out1), heads, L / blk, blk, L, ld1, s);
        } else if (kind == 4) {
            BG_REQUIRE(heads >= 1 && rows >= 1 && cols >= 1 && ld1 >= cols && (!in0 || ld0 >= cols), "op_attn_tables (masked_bias): bad arguments");
            BG_REQUIRE(!in1 || (L >= rows && L >= cols), "op_attn_tables (masked_bias): the element mask is [L, L]");
            BG_REQUIRE(!in2 || (blk >= 1 && L % blk == 0 && L >= rows && L >= cols), "op_attn_tables (masked_bias): the block layout covers L = %d keys in blocks of %d", L, blk);
            SparseVis v;
            if (in1) { v.allowed = reinterpret_cast<const uint8_t*>(in1); v.ldallowed = L; v.allowed_head_stride = hs0; }
            if (in2) { v.lay = reinterpret_cast<const uint8_t*>(in2); v.lay_head_stride = hs1; v.nb = L / blk; v.blk = blk; }
            launch_build_masked_bias(f0, v, reinterpret_cast<float*>(out0), heads, rows, cols, ld1, ld0, scale, s);
        } else {
            BG_REQUIRE(in0 && heads >= 1 && rows >= 1 && cols >= 32 && cols % 32 == 0 && ld0 >= cols, "op_attn_tables (attn_tiles): bad arguments");
            launch_build_attn_tiles(f0, hs0, ld0, heads, rows, cols, reinterpret_cast<uint16_t*>(out0), s);
        }
    });
}

int bevgen_op_attention_tiles(bevgen_ctx* ctx, const float* q, const float* k, const float* v, const float* bias, int ldbias, const float* residual, int B, int H, int Nq,
                              int Nk_pad, float scale, int kv_group, int use_tiles, int out_layout, float* out, void* stream) {
    return guarded(ctx, [&] {
        hipStream_t s = (hipStream_t)stream;
        BG_REQUIRE(q && k && v && bias && out && B >= 1 && H >= 1 && Nq >= 1, "op_attention_tiles: null argument");
        BG_REQUIRE(Nk_pad >= 32 && Nk_pad % 32 == 0 && ldbias >= Nk_pad && ldbias % 4 == 0, "op_attention_tiles: Nk_pad %% 32, bias row stride %% 4 and >= Nk_pad");
        BG_REQUIRE(kv_group >= 1 && B % kv_group == 0, "op_attention_tiles: batch %d is not a multiple of kv_group %d", B, kv_group);
        BG_REQUIRE(out_layout == 0 || out_layout == 1, "op_attention_tiles: out_layout 0 = [B, Nq, 64 H], 1 = [B, H, Nq, 64]");
        AttnArgs a{};
        a.Q = q; a.K = k; a.V = v; a.bias = bias; a.R = residual; a.O = out;
        a.B = B; a.H = H; a.Nq = Nq; a.Nk_pad = Nk_pad;
        a.q_bstride = (long)H * Nq * 64; a.q_hstride = (long)Nq * 64;
        a.kv_bstride = (long)H * Nk_pad * 64; a.kv_hstride = (long)Nk_pad * 64;
        a.ldbias = ldbias; a.bias_head_stride = (long)Nq * ldbias; a.scale = scale;
        a.kv_group = kv_group;
        if (out_layout == 0) { a.o_bstride = (long)Nq * H * 64; a.o_qstride = (long)H * 64; a.o_hstride = 64; }
        else { a.o_bstride = (long)H * Nq * 64; a.o_qstride = 64; a.o_hstride = (long)Nq * 64; }
        if (use_tiles) {
            uint16_t* tiles;
            ctx->arena.carve([&](Arena& ar) { tiles = ar.get<uint16_t>(attn_tiles_elems(H, Nq, Nk_pad)); });
            launch_build_attn_tiles(bias, a.bias_head_stride, ldbias, H, Nq, Nk_pad, tiles, s);
            a.tiles = tiles; a.tiles_head_stride = (long)cdiv(Nq, 128) * (Nk_pad / 32 + 1); a.tiles_ld = Nk_pad / 32 + 1;
        }
        launch_attention(a, s);
    });
}

int bevgen_decode_attention_splits(int B, int H, int n) { return decode_attention_splits(B, H, n); }

long bevgen_lpips_prepared_bytes(int precision) { return lpips_prepared_bytes(precision); }
long bevgen_lpips_workspace_bytes(int n, int H, int W, int precision) { return lpips_workspace_bytes(n, H, W, precision); }

long bevgen_metrics_workspace_bytes(int op, int n, int C, int H, int W, int kernel_size) {
    return op == 0 ? image_sqerr_workspace_bytes(n, C, H, W) : op == 1 ? ssim_workspace_bytes(n, C, H, W, kernel_size) : -1;
}

int bevgen_profile_begin(bevgen_ctx* ctx) {
    return guarded(ctx, [&] { ctx->prof.begin(); });
}

int bevgen_profile_end(bevgen_ctx* ctx, double* out) {
    return guarded(ctx, [&] {
        BG_REQUIRE(out, "profile_end: null output");
        ctx->prof.end(out);
    });
}

int bevgen_ar_step_timing(bevgen_ctx* ctx, int enable) {
    return guarded(ctx, [&] { ctx->time_steps = enable != 0; });
}

int bevgen_ar_step_times(bevgen_ctx* ctx, float* h_out_ms, int cap, int* count) {
    return guarded(ctx, [&] {
        BG_REQUIRE(h_out_ms && count && cap >= 0, "ar_step_times: bad arguments");
        *count = ar_step_times(*ctx, h_out_ms, cap);
    });
}

int bevgen_set_trace_buffer(bevgen_ctx* ctx, void* d_buf) {
    return guarded(ctx, [&] { ctx->trace = reinterpret_cast<long long*>(d_buf); });
}

}  // extern "C"
