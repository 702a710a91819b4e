"""Host logic of the Route A scoring path (GPT.score / forward_onepass, Net2NetTransformer.shared_step / forward(x, c, batch)) without a GPU: the Context is a stub
whose ar_forward answers with the CPU oracle in the library's conventions (camera-major inputs, DECODE-order outputs), so what is checked here is exactly what the
modules add - the pad substitution of the last camera-major token (gpt:328-329), which tensor is the target, and the decode-order -> camera-major permutation."""
import pytest
import torch
import torch.nn.functional as F

from bevgen_amd import presets, synthetic, weights as W
from oracle import restate as R


class StubContext:
    """Context.ar_forward with the oracle behind it; records what it was given."""

    def __init__(self, cfg, sd):
        self.cfg, self.sd, self.device, self.calls = cfg, sd, torch.device("cpu"), []

    def ar_forward(self, cond_ids, I_inv, E_inv, ids, *, n_steps=None, target=None, weight=None, want_logits=True, check=True):
        cfg = self.cfg
        self.calls.append(dict(ids=ids.clone(), target=None if target is None else target.clone(), weight=weight, want_logits=want_logits))
        B = cond_ids.shape[0]
        cam = R.gpt_forward(self.sd, cfg, ids.reshape(B, cfg.num_cams, cfg.num_cam_tokens), cond_ids, I_inv, E_inv)
        fwd = cfg.forward_shuffle_idx
        dec = cam[:, fwd]
        nll = loss = None
        if target is not None:
            t = target.reshape(B, -1)[:, fwd]
            nll = F.cross_entropy(dec.reshape(-1, dec.shape[-1]), t.reshape(-1), reduction="none").reshape(t.shape)
            w = torch.ones_like(nll) if weight is None else weight.reshape(B, -1)[:, fwd]
            loss = (w * nll).mean()
        return (dec if want_logits else None), nll, loss

    def close(self):
        pass


@pytest.fixture()
def tiny():
    from bevgen_amd.modules.transformer.mingpt_sparse import GPT

    cfg = presets.tiny_route_a(3, block=4)
    sd = W.gpt_state_dict(cfg, 1234)
    gpt = GPT(cfg)
    gpt.load_state_dict(sd)
    gpt._ctx = StubContext(cfg, sd)
    B = 2
    bt = synthetic.make_batch(cfg, B, seed=2)
    ids = torch.randint(0, cfg.vocab_size, (B, cfg.num_cams, cfg.num_cam_tokens), generator=torch.Generator().manual_seed(1))
    assert not torch.equal(cfg.forward_shuffle_idx, torch.arange(cfg.num_img_tokens)), "the decode order of the fixture must differ from camera-major order"
    return cfg, sd, gpt, bt, ids


def _ref(cfg, sd, bt, ids_in, target):
    logits = R.gpt_forward(sd, cfg, ids_in, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])
    nll = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), target.reshape(-1), reduction="none").reshape(target.shape[0], -1)
    return logits, nll


@pytest.mark.parametrize("sampling", [True, False])
def test_score_substitutes_the_last_token_and_returns_camera_major_nll(tiny, sampling):
    cfg, sd, gpt, bt, ids = tiny
    batch = {"intrinsics_inv": bt["intrinsics_inv"], "extrinsics_inv": bt["extrinsics_inv"]}
    before = ids.clone()
    nll, loss = gpt.score(ids, bt["cond_ids"], batch, sampling=sampling)
    assert torch.equal(ids, before), "the caller's tokens must not be modified"
    call = gpt._ctx.calls[-1]
    want_in = before.reshape(2, -1).clone()
    if not sampling:
        want_in[:, -1] = cfg.vocab_size
    assert torch.equal(call["ids"], want_in) and torch.equal(call["target"], before.reshape(2, -1)) and call["want_logits"] is False
    _, ref_nll = _ref(cfg, sd, bt, want_in.reshape(before.shape), before)
    assert torch.allclose(nll, ref_nll, atol=1e-5) and abs(loss.item() - ref_nll.mean().item()) < 1e-5
    # an explicit target and weight travel camera-major, unchanged
    tgt = torch.randint(0, cfg.vocab_size, (2, cfg.num_img_tokens), generator=torch.Generator().manual_seed(7))
    w = torch.rand((2, cfg.num_img_tokens), generator=torch.Generator().manual_seed(8))
    nll_t, loss_t = gpt.score(ids, bt["cond_ids"], batch, sampling=sampling, target=tgt, weight=w)
    _, ref_t = _ref(cfg, sd, bt, want_in.reshape(before.shape), tgt)
    assert torch.allclose(nll_t, ref_t, atol=1e-5) and abs(loss_t.item() - (w * ref_t).mean().item()) < 1e-5


def test_forward_onepass_returns_camera_major_logits(tiny):
    cfg, sd, gpt, bt, ids = tiny
    batch = {"intrinsics_inv": bt["intrinsics_inv"], "extrinsics_inv": bt["extrinsics_inv"]}
    logits = gpt.forward_onepass(ids, bt["cond_ids"], batch, sampling=True)
    ref, _ = _ref(cfg, sd, bt, ids, ids)
    assert torch.allclose(logits, ref, atol=1e-6)


def test_net2net_shared_step_forward_and_refusals(tiny):
    from bevgen_amd.modules.stage2.cond_transformer_multi_view import Net2NetTransformer

    cfg, sd, gpt, bt, ids = tiny
    model = Net2NetTransformer(gpt, None, None)
    batch = {"z_ids": ids, "cond_ids": bt["cond_ids"], "intrinsics_inv": bt["intrinsics_inv"], "extrinsics_inv": bt["extrinsics_inv"]}
    sub = ids.clone()
    sub[:, -1, -1] = cfg.vocab_size
    ref_logits, ref_nll = _ref(cfg, sd, bt, sub, ids)
    loss = model.shared_step(batch, 0)
    assert abs(loss.item() - ref_nll.mean().item()) < 1e-5           # ar_lm:349: the unweighted mean over sequences and tokens
    assert abs(model.validation_step(batch, 1)["loss"].item() - ref_nll.mean().item()) < 1e-5
    logits, target = model(None, None, batch)                          # ar_lm:109-136
    assert torch.equal(target, ids.reshape(2, -1)) and torch.allclose(logits, ref_logits, atol=1e-6)
    with pytest.raises(TypeError):
        model(None, batch)
    weighted = Net2NetTransformer(gpt, None, None, bbox_ce_weight=0.5)   # accepted by the constructor, refused where the branch would run
    with pytest.raises(NotImplementedError, match="ar_lm:281-347"):
        weighted.shared_step(batch, 0)
    pad = model.inference_step(batch)                                  # ar_lm:144-152: the all-pad image sequence
    assert torch.equal(gpt._ctx.calls[-1]["ids"], torch.full((2, cfg.num_img_tokens), cfg.vocab_size)) and pad.shape == ref_logits.shape


def test_context_ar_forward_checks_its_arguments_before_the_library_is_called():
    """Shape / range errors are Python errors (no GPU needed: they precede the C call)."""
    from bevgen_amd.runtime import Context

    cfg = presets.tiny_route_a(3, block=4)
    ctx = Context.__new__(Context)
    ctx.cfg, ctx.device = cfg, torch.device("cpu")
    bt = synthetic.make_batch(cfg, 2, seed=2)
    ids = torch.zeros((2, cfg.num_img_tokens), dtype=torch.long)
    args = (bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"])
    with pytest.raises(ValueError, match="n_steps"):
        ctx.ar_forward(*args, ids, n_steps=0)
    with pytest.raises(ValueError, match="n_steps"):
        ctx.ar_forward(*args, ids, n_steps=cfg.num_img_tokens + 1)
    with pytest.raises(ValueError, match="camera-major"):
        ctx.ar_forward(*args, ids[:, :-1])
    with pytest.raises(ValueError, match="weight needs a target"):
        ctx.ar_forward(*args, ids, weight=torch.ones(2, cfg.num_img_tokens))
