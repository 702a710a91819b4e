"""Route A one-pass teacher-forced forward and token scoring (bevgen_ar_forward, GPT.score / forward_onepass, Net2NetTransformer.shared_step).

Tolerances come from the project: the stepwise GPT.forward is held to max|logits - ref| / max|ref| < 1e-4 against the oracle (tests/test_dropin_gpu.py); call
e = 1e-4 max|ref|.  Log-sum-exp is 1-Lipschitz in the max norm, so a per-token nll (logsumexp - target logit) and the mean loss may differ from the reference value by
at most 2 e.  Two computations that are each within e of the oracle may differ from each other by 2 e.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import cases, restate as R

pytestmark = pytest.mark.gpu

FIXTURES = ["a_tiny_blk16", "a_tiny_blk4", "a_tiny_6cam", "a_tiny_d06", "a_tiny_heavy"]


def _t(a, dtype=None):
    t = torch.from_numpy(np.asarray(a))
    return t.to(dtype) if dtype is not None else t


def make_ctx(cfg, sd, **kw):
    from bevgen_amd.runtime import Context

    ctx = Context(cfg, route="ar", **kw)
    ctx.load_state_dict(sd)
    ctx.set_tables()
    ctx.finalize()
    return ctx


def _fixture(name):
    case = cases.CASES[name]
    g = golden("route_a_" + name)
    cfg = case.make_cfg()
    sd = cases.golden_state_dict(case, cfg, g)
    cond, I, E = _t(g["cond_ids"], torch.long), _t(g["I_inv"]), _t(g["E_inv"])
    ids = _t(g["ids_in"], torch.long).reshape(cond.shape[0], -1)
    return cfg, sd, cond, I, E, ids, _t(g["logits_full"])


def _cam(cfg, dec):
    """decode order -> camera-major along dim 1"""
    return dec[:, cfg.backward_shuffle_idx.to(dec.device)]


def _ce(logits, target):
    """per-token cross-entropy [B, N] on the CPU"""
    return F.cross_entropy(logits.reshape(-1, logits.shape[-1]), target.reshape(-1), reduction="none").reshape(target.shape)


# ------------------------------------------------------------------------------------------------ 1. logits vs the imported reference
@pytest.mark.parametrize("kv", ["f32", "f16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_onepass_logits_match_the_reference(name, kv):
    cfg, sd, cond, I, E, ids, ref = _fixture(name)
    ctx = make_ctx(cfg, sd, kv_cache=kv)
    logits, nll, loss = ctx.ar_forward(cond, I, E, ids)
    assert nll is None and loss is None
    got = _cam(cfg, logits).cpu()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"{name} kv={kv}: one-pass logits rel err {err:.3e}")
    assert err < 1e-4
    assert ctx.status() == 0
    ctx.close()


@pytest.mark.parametrize("heavy", [False, True])
def test_onepass_logits_f16_decode_weights_match_the_rounded_weights_oracle(heavy):
    """decode_weights='f16' = the model with fp16-representable projection matrices: the oracle on the rounded state_dict, built as the existing f16-weight tests build
    it (tests/test_status_gpu.py, tests/test_models_gpu.py) - the mode needs dim % 256 == 0, so the dim-128 fixtures cannot run in it: the dim-256 preset, with the
    reference initialisation and with heavy-tailed weights."""
    from bevgen_amd import presets, synthetic
    from test_models_gpu import _round_projection_weights

    cfg = presets.route_a(3, num_layers=2, dim=256, heads=4, vocab=64, cam_res=(64, 64), cam_latent_res=(4, 5), bev_latent_res=(4, 4), block=16, window_len=8)
    sd = cases.gpt_state_dict(cfg, 1234)
    if heavy:
        sd = cases.heavy_tail(sd, 53)
    bt = synthetic.make_batch(cfg, 3, seed=3)
    cond, I, E = bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"]
    ids = torch.randint(0, cfg.vocab_size, (3, cfg.num_img_tokens), generator=torch.Generator().manual_seed(8))
    ref = R.gpt_forward(_round_projection_weights(sd), cfg, ids.reshape(-1, cfg.num_cams, cfg.num_cam_tokens), cond, I, E)
    e = 1e-4 * ref.abs().max().item()
    for kv in ("f32", "f16"):
        ctx = make_ctx(cfg, sd, decode_weights="f16", kv_cache=kv)
        logits, nll, loss = ctx.ar_forward(cond, I, E, ids, target=ids)
        err = ((_cam(cfg, logits).cpu() - ref).abs().max() / ref.abs().max()).item()
        ref_nll = _ce(ref, ids)
        d_nll = (_cam(cfg, nll).cpu() - ref_nll).abs().max().item()
        print(f"heavy={heavy} decode_weights=f16 kv={kv}: one-pass logits rel err {err:.3e}  |nll - ref| {d_nll:.3e}  e {e:.3e}")
        assert err < 1e-4 and d_nll <= 2 * e and abs(loss.item() - ref_nll.mean().item()) <= 2 * e
        ctx.close()


# ------------------------------------------------------------------------------------------------ 2. loss and nll
@pytest.mark.parametrize("name", FIXTURES)
def test_nll_and_loss_match_cross_entropy_of_the_reference_logits(name):
    cfg, sd, cond, I, E, ids, ref = _fixture(name)
    e = 1e-4 * ref.abs().max().item()
    ctx = make_ctx(cfg, sd)
    # target = the input tokens
    logits, nll, loss = ctx.ar_forward(cond, I, E, ids, target=ids)
    ref_nll = _ce(ref, ids)
    d_nll = (_cam(cfg, nll).cpu() - ref_nll).abs().max().item()
    d_loss = abs(loss.item() - ref_nll.mean().item())
    print(f"{name}: e {e:.3e}  |nll - ref| {d_nll:.3e}  |loss - ref| {d_loss:.3e}  loss {loss.item():.6f}")
    assert d_nll <= 2 * e and d_loss <= 2 * e
    # the logits never materialised: the same bits
    _, nll2, loss2 = ctx.ar_forward(cond, I, E, ids, target=ids, want_logits=False)
    assert torch.equal(nll2, nll) and torch.equal(loss2, loss)
    # two identical calls: the same bits
    _, nll3, loss3 = ctx.ar_forward(cond, I, E, ids, target=ids, want_logits=False)
    assert torch.equal(loss3, loss2) and torch.equal(nll3, nll2)
    # sampling=False: the camera-major last token enters as the pad id (gpt:328-329); the target keeps it
    sub = ids.clone()
    sub[:, -1] = cfg.vocab_size
    ref_s = R.gpt_forward(sd, cfg, sub.reshape(-1, cfg.num_cams, cfg.num_cam_tokens), cond, I, E)
    es = 1e-4 * ref_s.abs().max().item()
    lg_s, nll_s, loss_s = ctx.ar_forward(cond, I, E, sub, target=ids)
    ref_nll_s = _ce(ref_s, ids)
    d_lg = ((_cam(cfg, lg_s).cpu() - ref_s).abs().max() / ref_s.abs().max()).item()
    d_nll = (_cam(cfg, nll_s).cpu() - ref_nll_s).abs().max().item()
    d_loss = abs(loss_s.item() - ref_nll_s.mean().item())
    print(f"{name} pad-substituted: logits rel {d_lg:.3e}  |nll - ref| {d_nll:.3e}  |loss - ref| {d_loss:.3e}")
    assert d_lg < 1e-4 and d_nll <= 2 * es and d_loss <= 2 * es
    # a non-trivial weight in [0, 1] (|w| <= 1: the bound of the weighted mean is still 2 e); nll stays unweighted
    w = torch.rand(ids.shape, generator=torch.Generator().manual_seed(5))
    _, nll_w, loss_w = ctx.ar_forward(cond, I, E, ids, target=ids, weight=w, want_logits=False)
    d_loss = abs(loss_w.item() - (w * ref_nll).mean().item())
    print(f"{name} weighted: |loss - ref| {d_loss:.3e}")
    assert torch.equal(nll_w, nll) and d_loss <= 2 * e
    assert ctx.status() == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. full size
def test_config1_full_size_logits_and_loss_against_the_oracle():
    case = cases.CASES["a_config1"]
    cfg = case.make_cfg()
    sd = cases.gpt_state_dict(cfg, case.weight_seed)
    bt = cases.inputs(case, cfg)
    cond, I, E = bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"]
    ids = torch.randint(0, cfg.vocab_size, (cond.shape[0], cfg.num_img_tokens), generator=torch.Generator().manual_seed(3))
    ref = R.gpt_forward(sd, cfg, ids.reshape(-1, cfg.num_cams, cfg.num_cam_tokens), cond, I, E)
    e = 1e-4 * ref.abs().max().item()
    ctx = make_ctx(cfg, sd)
    logits, nll, loss = ctx.ar_forward(cond, I, E, ids, target=ids)
    err = ((_cam(cfg, logits).cpu() - ref).abs().max() / ref.abs().max()).item()
    ref_nll = _ce(ref, ids)
    d_nll = (_cam(cfg, nll).cpu() - ref_nll).abs().max().item()
    d_loss = abs(loss.item() - ref_nll.mean().item())
    print(f"config1: logits rel err {err:.3e}  e {e:.3e}  |nll - ref| {d_nll:.3e}  |loss - ref| {d_loss:.3e}")
    assert err < 1e-4 and d_nll <= 2 * e and d_loss <= 2 * e
    ctx.close()


@pytest.fixture(scope="module")
def config4_weights():
    cfg = cases.CASES["a_config4_head"].make_cfg()
    return cfg, cases.gpt_state_dict(cfg, 1234)


@pytest.mark.parametrize("kv", ["f32", "f16"])
def test_config4_onepass_against_the_stepwise_path(config4_weights, kv):
    """Config 4 (L = 2368), B = 2, 300 image rows: the one-pass logits against the library's own stepwise path (prefill + 300 decode steps) within 2 e."""
    from bevgen_amd import synthetic

    cfg, sd = config4_weights
    B, n = 2, 300
    bt = synthetic.make_batch(cfg, B, seed=21)
    cond, I, E = bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"]
    ids = torch.randint(0, cfg.vocab_size, (B, cfg.num_img_tokens), generator=torch.Generator().manual_seed(4))
    ctx = make_ctx(cfg, sd, kv_cache=kv)
    flat = ids.cuda()
    ctx.ar_prefill(cond, I, E)
    rows = []
    for s in range(n):
        rows.append(ctx.ar_logits())
        ctx.ar_decode_step(flat[:, int(cfg.forward_shuffle_idx[s])])
    ctx.synchronize()
    step = torch.stack(rows, dim=1).cpu()
    one = ctx.ar_forward(cond, I, E, ids, n_steps=n)[0].cpu()
    e = 1e-4 * step.abs().max().item()
    d = (one - step).abs().max().item()
    print(f"config4 kv={kv}: e {e:.3e}  max |one-pass - stepwise| {d:.3e}  ({d / e:.2f} e)")
    assert d <= 2 * e
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. state hand-over
@pytest.mark.parametrize("kv", ["f32", "f16"])
def test_decode_steps_continue_after_a_partial_onepass_forward(kv):
    """ar_forward(n_steps = s0) leaves the context as after prefill + s0 decode steps: the K/V cache rows are where the decode kernels read them."""
    cfg, sd, cond, I, E, ids, ref = _fixture("a_tiny_blk16")
    fwd = cfg.forward_shuffle_idx
    ref_dec = ref[:, fwd]   # decode order
    scale = ref.abs().max().item()
    e = 1e-4 * scale
    ctx = make_ctx(cfg, sd, kv_cache=kv)
    full = ctx.ar_forward(cond, I, E, ids)[0].cpu()
    s0 = cfg.num_img_tokens // 3
    part = ctx.ar_forward(cond, I, E, ids, n_steps=s0)[0].cpu()
    assert (part - full[:, :s0]).abs().max().item() <= 2 * e
    row = ctx.ar_logits().cpu()
    d = (row - full[:, s0]).abs().max().item()
    print(f"kv={kv}: e {e:.3e}  |ar_logits - one-pass row s0| {d:.3e}")
    assert d <= 2 * e
    flat = ids.cuda()
    for j in range(8):
        ctx.ar_decode_step(flat[:, int(fwd[s0 + j])])
        row = ctx.ar_logits().cpu()
        err = (row - ref_dec[:, s0 + j + 1]).abs().max().item() / scale
        print(f"kv={kv}: decode step {s0 + j + 1}: rel err vs the oracle {err:.3e}")
        assert err < 1e-4
    ctx.synchronize()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. status word
def test_non_finite_logits_raise_instead_of_returning_a_loss():
    from bevgen_amd import _lib

    case = cases.CASES["a_tiny_blk16"]
    cfg = case.make_cfg()
    sd = dict(cases.gpt_state_dict(cfg, case.weight_seed))
    sd["head.weight"] = sd["head.weight"].clone()
    sd["head.weight"][3, 1] = float("inf")
    bt = cases.inputs(case, cfg)
    ids = torch.zeros((case.batch, cfg.num_img_tokens), dtype=torch.long)
    ctx = make_ctx(cfg, sd)
    for want_logits in (True, False):
        with pytest.raises(_lib.BevgenError, match="NaN / inf logit") as ei:
            ctx.ar_forward(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], ids, target=ids, want_logits=want_logits, check=True)
        assert ei.value.code == _lib.ERR_NUMERIC
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. drop-in modules
def test_net2net_shared_step_test_step_and_forward():
    from bevgen_amd.modules.stage2.cond_transformer_multi_view import Net2NetTransformer
    from bevgen_amd.modules.transformer.mingpt_sparse import GPT

    cfg, sd, cond, I, E, ids, _ = _fixture("a_tiny_blk16")
    from bevgen_amd import weights as W
    from bevgen_amd.modules.stage1.vqgan import VQModel

    dd = cases.VQ_TINY["dd"]
    gpt = GPT(cfg, precision="fp32")
    vq = VQModel(ddconfig=dd, n_embed=64, embed_dim=64, cam_res=(64, 64), cam_latent_res=(4, 5), cam_emd_dim=64)
    model = Net2NetTransformer(gpt, vq, None)
    full = {("transformer." + k): v for k, v in sd.items()}
    full.update({("first_stage_model." + k): v for k, v in W.vq_state_dict(dd, 64, 64, 99, with_encoder=True).items()})
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected, unexpected
    model = model.to("cuda")
    z = ids.reshape(-1, cfg.num_cams, cfg.num_cam_tokens)
    batch = {"z_ids": z, "cond_ids": cond, "intrinsics_inv": I, "extrinsics_inv": E}
    sub = ids.clone()
    sub[:, -1] = cfg.vocab_size
    ref = R.gpt_forward(sd, cfg, sub.reshape(z.shape), cond, I, E)
    e = 1e-4 * ref.abs().max().item()
    ref_nll = _ce(ref, ids)
    loss = model.shared_step(batch, 0)
    print(f"shared_step loss {loss.item():.6f}  reference {ref_nll.mean().item():.6f}  e {e:.3e}")
    assert abs(loss.item() - ref_nll.mean().item()) <= 2 * e
    # the same number as the C entry point gives for the same tokens (item 2's loss)
    _, _, direct = gpt.context().ar_forward(cond, I, E, sub, target=ids, want_logits=False)
    assert torch.equal(direct, loss)
    nll, loss2 = gpt.score(z.cuda(), cond.cuda(), {"intrinsics_inv": I, "extrinsics_inv": E}, sampling=False)
    assert torch.equal(loss2, loss) and (nll.cpu() - ref_nll).abs().max().item() <= 2 * e
    # forward(x, c, batch) -> (logits, target); forward_onepass = the stepwise GPT.forward
    logits, target = model(None, None, batch)
    assert torch.equal(target.cpu(), ids) and ((logits.cpu() - ref).abs().max() / ref.abs().max()).item() < 1e-4
    stepwise = gpt(z.cuda(), cond.cuda(), {"intrinsics_inv": I.cuda(), "extrinsics_inv": E.cuda()}, sampling=False)
    assert (logits - stepwise).abs().max().item() <= 2 * e
    # validation_step / inference_step
    assert model.inference_step(batch).shape == logits.shape
    # test_step: same keys as before, test/loss logged once through a stub log
    calls = []
    object.__setattr__(model, "log", lambda name, value, **kw: calls.append((name, float(value))))
    out = model.test_step(batch, 0)
    assert set(out) == {"gen", "rec", "gt"}
    assert [c[0] for c in calls] == ["test/loss"] and calls[0][1] == loss.item()
    # no ground truth in the batch: nothing logged, same keys
    calls.clear()
    out = model.test_step({k: v for k, v in batch.items() if k != "z_ids"}, 0)
    assert set(out) == {"gen", "rec", "gt"} and not calls
    # the weighted branch is refused by shared_step, not by the constructor
    weighted = Net2NetTransformer(gpt, None, None, bbox_ce_weight=0.5)
    with pytest.raises(NotImplementedError, match="ar_lm:281-347"):
        weighted.shared_step(batch, 0)
