"""Classifier-free guidance of Route M on the GPU against the float64 restatement (tests/cfg_ref.py): the null-condition forward, guided generate token for token,
guidance off = today's tokens, the drop-in boundary, and the opt-in rounded modes."""
import pytest
import torch

import cfg_ref as G
from oracle import cases, restate as R
from test_models_gpu import _assert_flips_only_at_near_ties, _flip_report, _round_gemm_weights_route_m

pytestmark = pytest.mark.gpu

# tests/test_models_gpu.py holds the conditional forward of m_tiny_rays to `rel(...) < 1e-4` (test_route_m_tiny: fp32; test_route_m_split_precision_mode: f16x3), and
# tests/test_status_gpu.py holds m_fold (test_route_m_folded_layernorm_levels_reproduce_the_reference_tokens) and m_tiny_heavy
# (test_route_m_heavy_tailed_weights_tokens_bit_exact) to the same 1e-4 in both modes: of the largest |value| of the tensor
FORWARD_BOUND = 1e-4
SCALE, TS = G.SCALE, G.TIMESTEPS


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def make_ctx(cfg, sd, **kw):
    from bevgen_amd.runtime import Context

    ctx = Context(cfg, route="maskgit", **kw)
    ctx.load_state_dict(sd)
    ctx.set_tables()
    ctx.finalize()
    return ctx


def gen(ctx, bt, noise, **kw):
    nz = {} if noise is None else dict(gumbel_u=noise["gumbel_u"], critic_u=noise["critic_u"])
    return ctx.maskgit_generate(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], timesteps=TS, topk_filter_thres=0.9, **nz, **kw).cpu()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["m_tiny_rays", "m_fold", "m_tiny_heavy"])
def test_null_forward(name, precision):
    """Logits and embed of the null-condition forward versus the restatement's literal masked form, at the bound the conditional forward of the same case and mode is
    held to (FORWARD_BOUND above)."""
    case, cfg, sd, bt = G.fixture(name)
    ids = G.random_ids(case, cfg)
    lr, er = G.muse_forward_null(sd, cfg, ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads)
    ctx = make_ctx(cfg, sd, precision=precision)
    lg, eg = ctx.muse_forward(ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], null_condition=True)
    lc, _ = ctx.muse_forward(ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])
    assert ctx.status() == 0
    ctx.close()
    el, ee = rel(lg.cpu().double(), lr), rel(eg.cpu().double(), er)
    print(f"null forward {name} {precision}: logits {el:.2e} embed {ee:.2e}")
    assert el < FORWARD_BOUND and ee < FORWARD_BOUND
    assert rel(lc.cpu().double(), lr) > 0.1, "the conditional forward is another function"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", G.D_CASES)
def test_guided_generate_reproduces_the_restatement(name, precision):
    """Guided generate (scale 3, 6 timesteps, topk_filter_thres 0.9) equals maskgit_generate_guided token for token on the (case, noise) pairs of
    tests/test_cfg_ref_cpu.py's condition (d): with the token critic on all of them, with use_token_critic=False on cfg_ref.FP32_AGREES_WITHOUT_CRITIC.  The other pairs
    without the critic are dropped from THIS test: there the restatement's own fp32 evaluation does not return its fp64 ids (the comment at that constant says why), so
    a free run has nothing to be equal to; test_guided_confidence_branch_iteration_by_iteration checks every pair of that branch, those included, iteration by iteration.
    Why exact here: every pick of these runs is decided by a relative margin >= 1e-4 (asserted there).  The guided logits amplify a logit error (|s| + |s - 1|) =
    5-fold at s = 3; tests/test_models_gpu.py ASSERTS 1e-4 for the forward (FORWARD_BOUND), which alone would not cover the margin - what covers it is the error these two
    modes have, fp32 round-off class (its docstrings quote 2e-5 for f16x3; test_null_forward prints the figure): five times 2e-6 is a tenth of the margin."""
    case, cfg, sd, bt = G.fixture(name)
    ctx = make_ctx(cfg, sd, precision=precision)
    for tag in G.D_NOISES:
        noise = G.noise_of(case, cfg, tag)
        for critic in (True, False):
            if not critic and name not in G.FP32_AGREES_WITHOUT_CRITIC:
                continue
            want, _ = G.guided_run(name, tag, critic)
            got = gen(ctx, bt, noise, cond_scale=SCALE, use_token_critic=critic)
            assert torch.equal(got, want), f"{tag} critic={critic}: " + _flip_report(got, want)
    assert ctx.status() == 0
    ctx.close()


ULP = 2.0 ** -24


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("remask", [False, True], ids=["score_mode1", "score_mode2"])
@pytest.mark.parametrize("name", G.D_CASES)
def test_guided_confidence_branch_iteration_by_iteration(name, remask, precision):
    """The branch without the token critic (score_mode 1, and 2 = can_remask_prev_masked) under guidance, on every (case, noise) pair, teacher-forced on the fp64
    restatement's trace: per iteration the masked ids go through the conditional forward, the null forward, cfg_combine and the pick kernel with confidence scores.
      * the picks equal the restatement's exactly (their margins are >= 1e-4: condition (d));
      * every confidence score is within 8 x 2^-24 + 4 e s of the fp64 score s, e = the observed logit error of the row: 1 - p has slope <= 2 (1 - p) in the logits
        (doubled for safety), and p itself carries a few fp32 roundings.  score_mode 2 scores a prediction at positions that are not picked: they are compared where that
        prediction is decided by the same margin, and -1e5 is exact at the unpicked positions of score_mode 1;
      * the re-masking kernel, given these scores and the next iteration's count, masks every position whose fp64 score clears the first excluded score by twice the
        tolerance and none that falls short of the last included score by as much: the sets differ only among scores tied within the tolerance."""
    case, cfg, sd, bt = G.fixture(name)
    ctx = make_ctx(cfg, sd, precision=precision)
    rows, T, V, mask_id = case.batch * cfg.num_cams, cfg.num_cam_tokens, cfg.vocab_size, cfg.vocab_size
    sched = R.mask_schedule(TS, T)
    mode = 2 if remask else 1
    for tag in G.D_NOISES:
        noise = G.noise_of(case, cfg, tag)
        _, trace = G.guided_run(name, tag, False, remask=remask)
        worst = 0.0
        for step, t in enumerate(trace):
            x_in = torch.where(t["picked"], torch.full_like(t["ids"], mask_id), t["ids"])
            lc, _ = ctx.muse_forward(x_in, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], want_embed=False)
            ln, _ = ctx.muse_forward(x_in, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], want_embed=False, null_condition=True)
            ours = ctx.op_cfg_combine(lc.reshape(-1, V), ln.reshape(-1, V), SCALE)
            ids = x_in.reshape(-1).cuda().clone()
            conf = torch.full((rows * T,), 7.0, dtype=torch.float32, device="cuda")
            gu = None if noise is None else noise["gumbel_u"][step].reshape(-1, V).cuda().contiguous()
            ctx.op_maskgit_pick(ids, ours, V, mask_id=mask_id, topk_filter_thres=0.9, temperature=t["temp"], gumbel_u=gu, conf_scores=conf, conf_mode=mode)
            assert torch.equal(ids.cpu().reshape(rows, T), t["ids"]), f"{tag} iteration {step}: " + _flip_report(ids.cpu().reshape(rows, T), t["ids"])
            err = (ours.cpu().double().reshape(rows, T, V) - t["logits"]).abs().amax(-1)
            s64, got = t["scores"], conf.cpu().double().reshape(rows, T)
            tol = 8 * ULP + 4 * err * s64.abs()
            if remask:
                decided = t["picked"] | (G.row_margins(t["y"]) >= G.MARGIN)
            else:
                decided = t["picked"]
                assert torch.equal(got[~t["picked"]], s64[~t["picked"]]) and (s64[~t["picked"]] == -1e5).all()
            over = ((got - s64).abs() / tol)[decided]
            worst = max(worst, float(over.max()))
            assert (over <= 1).all(), f"{tag} iteration {step}: a confidence score is {float(over.max()):.2f} tolerances from the fp64 score"
            if step + 1 == len(trace):
                continue
            n = sched[step + 1]
            masked = ctx.op_remask(t["ids"].cuda().clone(), conf.reshape(rows, T), n, mask_id).cpu() == mask_id
            assert (masked.sum(-1) == n).all()
            for r in range(rows):
                if remask and not decided[r].all():
                    continue   # (score_mode 2: a row with an undecided prediction has no fp64 score to order by)
                srt = s64[r].sort(descending=True).values
                slack = 2 * float(tol[r][decided[r]].max())   # (score_mode 1: the unpicked positions hold -1e5 exactly)
                clearly_in = s64[r] > (srt[n] + slack if n < T else -float("inf"))
                clearly_out = s64[r] < srt[n - 1] - slack
                assert masked[r][clearly_in].all() and not masked[r][clearly_out].any(), f"{tag} iteration {step} row {r}: re-masked set differs beyond ties"
        print(f"confidence branch {name} {precision} score_mode {mode} {tag}: worst score error {worst:.2f} of its tolerance")
    assert ctx.status() == 0
    ctx.close()


def test_null_pass_under_fold_level_2(monkeypatch):
    """BEVGEN_LN_FOLD=2: the conditional pass folds all four LayerNorms of a layer, the null pass runs its layers at level 1 (the planes a level-2 output projection
    leaves describe the row before the add).  m_fold, the smallest shape on which the fold engages: null forward at FORWARD_BOUND, guided tokens exact."""
    monkeypatch.setenv("BEVGEN_LN_FOLD", "2")
    case, cfg, sd, bt = G.fixture("m_fold")
    ids = G.random_ids(case, cfg)
    lr, er = G.muse_forward_null(sd, cfg, ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads)
    ctx = make_ctx(cfg, sd, precision="f16x3")
    lg, eg = ctx.muse_forward(ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], null_condition=True)
    assert rel(lg.cpu().double(), lr) < FORWARD_BOUND and rel(eg.cpu().double(), er) < FORWARD_BOUND
    for tag in G.D_NOISES:
        want, _ = G.guided_run("m_fold", tag, True)
        got = gen(ctx, bt, G.noise_of(case, cfg, tag), cond_scale=SCALE)
        assert torch.equal(got, want), tag + ": " + _flip_report(got, want)
    assert ctx.status() == 0
    ctx.close()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_guided_generate_with_init_ids_and_samples_per_layout(precision):
    from bevgen_amd import synthetic

    case, cfg, sd, bt = G.fixture("m_tiny_rays")
    ctx = make_ctx(cfg, sd, precision=precision)
    rows, T, V = case.batch * cfg.num_cams, cfg.num_cam_tokens, cfg.vocab_size
    # partial decoding: camera 0 of every scene is given (muse_net:543-544, 573-574)
    init = torch.full((rows, T), cfg.vocab_size, dtype=torch.long)
    init[0::cfg.num_cams] = torch.randint(0, V, (case.batch, T), generator=torch.Generator().manual_seed(11))
    trace = []
    want = G.maskgit_generate_guided(sd, cfg, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads, cond_scale=SCALE,
                                     timesteps=TS, init_ids=init, trace=trace)
    got = gen(ctx, bt, None, cond_scale=SCALE, init_ids=init)
    assert torch.equal(got.reshape(rows, T)[0::cfg.num_cams], init[0::cfg.num_cams])
    assert G.pick_margins(trace).min() >= G.MARGIN   # (the condition of the test above, for this run: its picks are decided)
    assert torch.equal(got, want), _flip_report(got, want)
    # samples_per_layout = 2: the same scenes generated without sharing the condition side
    S, layouts = 2, 2
    lay = synthetic.make_batch(cfg, layouts, seed=21)
    rep = {k: v.repeat_interleave(S, dim=0) for k, v in lay.items()}
    n = layouts * S * cfg.num_cams
    noise = {"gumbel_u": synthetic.uniform_noise((TS, n, T, V), 31, 0), "critic_u": synthetic.uniform_noise((TS, n, T), 31, 1)}
    a = gen(ctx, rep, noise, cond_scale=SCALE)
    b = gen(ctx, rep, noise, cond_scale=SCALE, samples_per_layout=S)
    assert torch.equal(a, b)
    assert not torch.equal(a, gen(ctx, rep, noise)), "guidance must change the tokens"
    ctx.close()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_guidance_off_changes_nothing(precision):
    """guidance=None with cond_scale=3 (what the reference's callers pass) and guidance='null' with cond_scale=1: the ids of today's generate, bit for bit."""
    from bevgen_amd.modules.stage2.muse_maskgit_pytorch import MaskGit, MaskGitTransformerMultiView

    case, cfg, sd, bt = G.fixture("m_tiny_rays")
    ctx = make_ctx(cfg, sd, precision=precision)
    noise = cases.maskgit_noise(case, cfg, seed=5)
    plain = {tag: gen(ctx, bt, nz) for tag, nz in (("greedy", None), ("noisy", noise))}
    assert torch.equal(plain["greedy"], R.maskgit_generate(sd, cfg, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads,
                                                           timesteps=TS))
    for tag, nz in (("greedy", None), ("noisy", noise)):
        assert torch.equal(gen(ctx, bt, nz, cond_scale=1), plain[tag]) and torch.equal(gen(ctx, bt, nz, cond_scale=None), plain[tag])
    ctx.close()
    tr = MaskGitTransformerMultiView(num_tokens=cfg.vocab_size, dim=cfg.num_embed, seq_len=cfg.cam_latent_res, depth=cfg.num_layers, dim_head=64, heads=cfg.num_heads,
                                     ff_mult=4, cfg=cfg)
    mg = MaskGit(image_size=cfg.cam_latent_res, transformer=tr, self_token_critic=True, precision=precision)
    mg.load_state_dict(sd, strict=False)
    mg = mg.to("cuda")
    batch = {"intrinsics_inv": bt["intrinsics_inv"].cuda(), "extrinsics_inv": bt["extrinsics_inv"].cuda()}
    kw = dict(cond_images=bt["cond_ids"].cuda(), fmap_size=cfg.cam_latent_res, batch=batch, timesteps=TS, noise="greedy")
    assert torch.equal(mg.generate(cond_scale=3, **kw).cpu(), plain["greedy"])
    assert torch.equal(mg.generate(cond_scale=3, guidance="off", **kw).cpu(), plain["greedy"])
    assert torch.equal(mg.generate(cond_scale=1, guidance="null", **kw).cpu(), plain["greedy"])
    guided = mg.generate(cond_scale=3, guidance="null", **kw).cpu()
    assert torch.equal(guided, G.guided_run("m_tiny_rays", "greedy", True)[0])
    with pytest.raises(ValueError):
        mg.generate(guidance="yes", **kw)


def test_net2net_dropin_hands_guidance_to_generate():
    """The Route M Net2NetTransformer built with guidance='null', cond_scale=3 among its kwargs (`+model.guidance=null +model.cond_scale=3`) samples the ids of the
    direct Context call; without them, the unguided ids."""
    from bevgen_amd import presets, weights as W
    from bevgen_amd.modules.stage1.vqgan import VQModel
    from bevgen_amd.modules.stage2.cond_transformer_multi_view_muse import Net2NetTransformer
    from bevgen_amd.modules.stage2.muse_maskgit_pytorch import MaskGit, MaskGitTransformerMultiView

    case, cfg, sd, bt = G.fixture("m_tiny_rays")
    ctx = make_ctx(cfg, sd, precision="f16x3")
    want = {s: ctx.maskgit_generate(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], timesteps=TS, cond_scale=s).cpu() for s in (None, SCALE)}
    ctx.close()
    batch = {"intrinsics_inv": bt["intrinsics_inv"].cuda(), "extrinsics_inv": bt["extrinsics_inv"].cuda()}
    for kwargs, key in ((dict(guidance="null", cond_scale=3), SCALE), ({}, None), (dict(cond_scale=3), None)):
        tr = MaskGitTransformerMultiView(num_tokens=cfg.vocab_size, dim=cfg.num_embed, seq_len=cfg.cam_latent_res, depth=cfg.num_layers, dim_head=64, heads=cfg.num_heads,
                                         ff_mult=4, cfg=cfg)
        mg = MaskGit(image_size=cfg.cam_latent_res, transformer=tr, self_token_critic=True)
        vq = VQModel(ddconfig=presets.VQ_DDCONFIG_TINY, n_embed=64, embed_dim=64, cam_res=(64, 64), cam_latent_res=cfg.cam_latent_res, cam_emd_dim=64)
        model = Net2NetTransformer(mg, vq, None, cfg, sample_iterations=TS, **kwargs)
        assert (model.guidance, model.cond_scale) == (kwargs.get("guidance"), kwargs.get("cond_scale"))
        model.load_state_dict({("maskgit." + k): v for k, v in sd.items()}, strict=False)
        model = model.to("cuda")
        got = model.sample(bt["cond_ids"].cuda(), batch, noise="greedy").cpu()
        assert torch.equal(got, want[key]), (kwargs, _flip_report(got, want[key]))
    assert not torch.equal(want[None], want[SCALE])


@pytest.mark.parametrize("mode", [dict(precision="f16x3", weights="f16"), dict(precision="f16x1")], ids=["weights_f16", "f16x1"])
def test_guided_generate_in_the_rounded_modes(mode):
    """weights='f16' and precision='f16x1' run guided and match the restatement evaluated on the ROUNDED matrices (the null rows come from the rounded to_out) by the
    near-tie rule of tests/test_models_gpu.py (_assert_flips_only_at_near_ties: an arg-max may differ only where the reference's top-2 margin is below twice the observed
    logit error of the row): teacher-forced on the restatement's ids, per iteration, over the picked rows.  The free run is compared only when no iteration has such a
    flip - behind one the two runs re-mask different tokens and have no common state."""
    case, cfg, sd, bt = G.fixture("m_tiny_rays")
    sdr = _round_gemm_weights_route_m(sd)
    trace = []
    want = G.maskgit_generate_guided(sdr, cfg, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads, cond_scale=SCALE,
                                     timesteps=TS, trace=trace)
    ctx = make_ctx(cfg, sd, **mode)           # the UNROUNDED weights: rounding is the library's job
    got = gen(ctx, bt, None, cond_scale=SCALE)
    assert int(got.min()) >= 0 and int(got.max()) < cfg.vocab_size
    first_flip = None
    for step, t in enumerate(trace):
        x_in = torch.where(t["picked"], torch.full_like(t["ids"], cfg.vocab_size), t["ids"])
        lc, _ = ctx.muse_forward(x_in, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], want_embed=False)
        ln, _ = ctx.muse_forward(x_in, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], want_embed=False, null_condition=True)
        V = lc.shape[-1]
        ours = ctx.op_cfg_combine(lc.reshape(-1, V), ln.reshape(-1, V), SCALE).reshape(lc.shape).cpu().double()
        flips = _assert_flips_only_at_near_ties(ours[t["picked"]], t["logits"][t["picked"]], f"{mode} iteration {step}")
        if flips.any() and first_flip is None:
            first_flip = step
    print(f"rounded mode {mode}: first near-tie flip at iteration {first_flip}; free run: {_flip_report(got, want)}")
    if first_flip is None:
        assert torch.equal(got, want), _flip_report(got, want)
    assert ctx.status() == 0
    ctx.close()
