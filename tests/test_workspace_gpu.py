"""Workspace arena across calls: a sequence of calls on ONE long-lived context - the arena grows, is reused without growing, shrinks its layout and regrows, and every
conditional allocation (samples_per_layout copies, generate's logits / scores, the fp32 K/V scratch, ar_forward's logits tile, the decoder's plane partials) comes and goes -
must give, call by call, bit-identical results to the same call on a fresh context, whose arena is sized by that call alone."""
import pytest
import torch

from oracle import cases

pytestmark = pytest.mark.gpu


def _cpu(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [None if t is None else t.cpu() for t in out]


def _check_sequence(make_ctx, steps):
    """steps: name -> callable(ctx) returning tensors.  All on one context first, then each on a context of its own."""
    ctx = make_ctx()
    shared = {name: _cpu(fn(ctx)) for name, fn in steps.items()}
    ctx.close()
    for name, fn in steps.items():
        ctx = make_ctx()
        fresh = _cpu(fn(ctx))
        ctx.close()
        assert len(fresh) == len(shared[name])
        for i, (a, b) in enumerate(zip(shared[name], fresh)):
            assert (a is None) == (b is None), (name, i)
            assert a is None or torch.equal(a, b), f"{name}, result {i}: {(a != b).sum().item()} of {a.numel()} elements differ between the long-lived and a fresh context"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_route_m_call_sequence_equals_fresh_contexts(precision):
    from bevgen_amd import synthetic
    from bevgen_amd.runtime import Context

    case = cases.CASES["m_tiny_rays"]
    cfg = case.make_cfg()
    sd = cases.maskgit_state_dict(cfg, case.weight_seed)
    T, V, ts = cfg.num_cam_tokens, cfg.vocab_size, case.timesteps

    def make_ctx():
        ctx = Context(cfg, route="maskgit", precision=precision)
        ctx.load_state_dict(sd)
        ctx.set_tables()
        ctx.finalize()
        return ctx

    def generate(scenes, seed, S=1):
        bt = synthetic.make_batch(cfg, scenes // S, seed=seed)
        bt = {k: v.repeat_interleave(S, dim=0) for k, v in bt.items()}
        rows = scenes * cfg.num_cams
        gu, cu = synthetic.uniform_noise((ts, rows, T, V), seed, 0), synthetic.uniform_noise((ts, rows, T), seed, 1)
        return lambda ctx: ctx.maskgit_generate(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], timesteps=ts, gumbel_u=gu, critic_u=cu, samples_per_layout=S)

    def forward(scenes, seed):
        bt = synthetic.make_batch(cfg, scenes, seed=seed)
        ids = torch.randint(0, V + 1, (scenes * cfg.num_cams, T), generator=torch.Generator().manual_seed(seed))
        return lambda ctx: ctx.muse_forward(ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])

    _check_sequence(make_ctx, {"1 generate, 1 scene": generate(1, 41), "2 generate, 4 scenes, 2 per layout": generate(4, 42, S=2), "3 forward, 2 scenes": forward(2, 43),
                               "4 generate, 1 scene again": generate(1, 44)})


@pytest.mark.parametrize("path", ["fused", "per_op"])
def test_route_a_call_sequence_equals_fresh_contexts(path):
    from bevgen_amd import presets, synthetic
    from bevgen_amd.runtime import Context

    cfg = presets.route_a(3, num_layers=2, dim=256, heads=4, vocab=64, cam_res=(64, 64), cam_latent_res=(4, 4), bev_latent_res=(4, 4), block=16, window_len=8)
    sd = cases.gpt_state_dict(cfg, 1234)
    N, V = cfg.num_img_tokens, cfg.vocab_size

    def make_ctx():
        ctx = Context(cfg, route="ar", decode_path=path)
        ctx.load_state_dict(sd)
        ctx.set_tables()
        ctx.finalize()
        return ctx

    def sample(B, seed, S=1):
        bt = synthetic.make_batch(cfg, B // S, seed=seed)
        bt = {k: v.repeat_interleave(S, dim=0) for k, v in bt.items()}
        noise = synthetic.uniform_noise((N, B), seed, 2)
        return lambda ctx: ctx.ar_sample(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], greedy=False, top_k=8, noise_u=noise, samples_per_layout=S)

    def forward(B, seed):
        bt = synthetic.make_batch(cfg, B, seed=seed)
        ids = torch.randint(0, V, (B, N), generator=torch.Generator().manual_seed(seed))
        return lambda ctx: ctx.ar_forward(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], ids, target=ids, want_logits=False)

    def stepwise(B, seed):
        bt = synthetic.make_batch(cfg, B, seed=seed)
        tok = torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(seed))

        def run(ctx):
            ctx.ar_prefill(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])
            l0 = ctx.ar_logits()
            ctx.ar_decode_step(tok)
            return l0, ctx.ar_logits(check=True)

        return run

    _check_sequence(make_ctx, {"1 sample, B = 2": sample(2, 51), "2 forward, B = 3, no logits": forward(3, 52), "3 sample, B = 6, 2 per layout": sample(6, 53, S=2),
                               "4 prefill + logits + step + logits, B = 2": stepwise(2, 54), "5 sample, B = 2": sample(2, 55)})


def test_vq_call_sequence_equals_fresh_contexts():
    from bevgen_amd.runtime import Context

    v = cases.VQ_TINY
    sd = cases.vq_state_dict(v["dd"], v["n_embed"], v["embed_dim"], v["seed"], with_encoder=True)
    dd = v["dd"]
    lat = dd["resolution"] // 2 ** (len(dd["ch_mult"]) - 1)

    def make_ctx():
        ctx = Context(None, vq_ddconfig=dd, vq_n_embed=v["n_embed"], vq_embed_dim=v["embed_dim"])
        ctx.load_state_dict(sd, prefix="first_stage_model.")
        ctx.finalize()
        return ctx

    def decode(n, seed):
        ids = torch.randint(0, v["n_embed"], (n, lat * lat), generator=torch.Generator().manual_seed(seed))
        return lambda ctx: ctx.vq_decode(ids, denormalize=True)

    def encode(n, seed):
        x = torch.randn(n, dd["in_channels"], dd["resolution"], dd["resolution"], generator=torch.Generator().manual_seed(seed))
        return lambda ctx: ctx.vq_encode(x)

    _check_sequence(make_ctx, {"1 decode, 1 image": decode(1, 61), "2 decode, 3 images": decode(3, 62), "3 encode, 2 images": encode(2, 63), "4 decode, 1 image again": decode(1, 64)})
