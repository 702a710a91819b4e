"""decode_weights='i8' (int8 projection weights with one fp32 scale per output row, BEVGEN_W_I8) through the whole Route A model, modelled on
tests/test_models_gpu.py::test_route_a_f16_decode_weights.

The mode DEFINES a model - every projection matrix replaced by code * scale at bevgen_finalize - that the CPU oracle can run exactly
(tests/decode_w_i8_ref.py::quantize_projection_weights_i8 builds its state_dict), so with an fp32 KV cache the acceptance is token equality on every fused-like decode
path and logits within the 2e-4 relative bound that test uses; lossy KV storage on top is held to the near-tie criterion of tests/test_models_gpu.py.  The library is
always given the UNQUANTISED state_dict: quantising is its job.

Two presets: the `small` one of that test (dim 256: the two skinny MLP launches) and the same with dim 1024 (the fused MLP launch and the auto rule's "fused at every
batch size" are actually taken)."""
import pytest
import torch

import decode_w_i8_ref as W
from oracle import cases, restate as R
from test_models_gpu import _assert_flips_only_at_near_ties, _assert_free_run_equal_until_first_near_tie, _decode_order, _flip_report, rel

pytestmark = pytest.mark.gpu

B = 3
_REF = {}


def _cfg(size):
    from bevgen_amd import presets

    dim, heads = {"small": (256, 4), "dim1024": (1024, 16)}[size]
    return presets.route_a(3, num_layers=2, dim=dim, heads=heads, vocab=64, cam_res=(64, 64), cam_latent_res=(4, 5), bev_latent_res=(4, 4), block=16, window_len=8)


def _reference(size):
    """(cfg, unquantised state_dict, dequantised state_dict, batch, oracle tokens, oracle logits [N, B, V]) of a preset: the oracle runs once per preset and is
    shared, unchanged"""
    if size not in _REF:
        from bevgen_amd import synthetic

        cfg = _cfg(size)
        sd = cases.gpt_state_dict(cfg, 1234)
        sdq = W.quantize_projection_weights_i8(sd)
        assert not torch.equal(sd["head.weight"], sdq["head.weight"])
        bt = synthetic.make_batch(cfg, B, seed=3)
        lc = []
        ref = R.ar_sample_cached(sdq, cfg, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], logits_out=lc, steps=cfg.num_img_tokens)
        _REF[size] = (cfg, sd, sdq, bt, ref, torch.stack(lc))
    return _REF[size]


def _ctx(cfg, sd, **kw):
    from bevgen_amd.runtime import Context

    ctx = Context(cfg, route="ar", decode_weights="i8", **kw)
    ctx.load_state_dict(sd)            # the UNQUANTISED weights
    ctx.set_tables()
    ctx.finalize()
    return ctx


@pytest.mark.parametrize("path", ["auto", "fused", "split", "auto-late"])
@pytest.mark.parametrize("size", ["small", "dim1024"])
def test_route_a_i8_decode_weights_tokens_equal_the_oracle_on_the_dequantised_model(size, path):
    """auto-late: a context created for eight sequences and called with three - at dim 256 the auto rule then takes the split layer, whose q | k | v image is packed
    on that first call (from the dequantised master matrix) instead of at bevgen_finalize"""
    cfg, sd, _, bt, ref, ref_logits = _reference(size)
    ctx = _ctx(cfg, sd, kv_cache="f32", max_batch=8) if path == "auto-late" else _ctx(cfg, sd, kv_cache="f32", decode_path=path)
    x, logits = ctx.ar_sample(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], greedy=True, steps=cfg.num_img_tokens, return_logits=True)
    ctx.synchronize()
    assert ctx.status() == 0
    err = rel(logits.cpu(), ref_logits)
    print(f"{size} decode_path={path}: logits rel err {err:.3e}")
    assert torch.equal(x.cpu(), ref), _flip_report(x.cpu(), ref)
    assert err < 2e-4
    ctx.close()


@pytest.mark.parametrize("kv", ["f16", "i8"])
@pytest.mark.parametrize("size", ["small", "dim1024"])
def test_route_a_i8_decode_weights_with_lossy_kv_cache_flips_only_at_near_ties(size, kv):
    cfg, sd, _, bt, ref, rl = _reference(size)
    ctx = _ctx(cfg, sd, kv_cache=kv)
    x, logits = ctx.ar_sample(bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], greedy=True, steps=cfg.num_img_tokens, return_logits=True)
    ctx.synchronize()
    assert ctx.status() == 0
    ctx.close()
    n = logits.shape[0]
    agree_prefix = (_decode_order(x.cpu(), cfg)[:n] == _decode_order(ref, cfg)[:n]).long().cumprod(0)   # [N, B]: 1 while the inputs are still the oracle's
    ol = logits.cpu()
    flips = torch.zeros(n, B, dtype=torch.bool)
    for q in range(B):
        m = int(agree_prefix[:, q].sum())            # rows 0..m were computed from identical inputs (row m is where the first flip happened, if any)
        rows = slice(0, min(m + 1, n))
        flips[rows, q] = _assert_flips_only_at_near_ties(ol[rows, q:q + 1], rl[rows, q:q + 1], f"i8 weights + {kv} KV, sequence {q}")[:, 0]
    _assert_free_run_equal_until_first_near_tie(x.cpu(), ref, flips, cfg, f"i8 weights + {kv} KV")
    print(f"{size} kv={kv}: {int(flips.sum())} near-tie flips, first-row logits rel err {rel(ol[0], rl[0]):.3e}")


@pytest.mark.parametrize("size", ["small", "dim1024"])
def test_scoring_runs_the_same_quantised_model(size):
    """bevgen_ar_forward (GPT.score) on an int8-weights context: logits, per-token nll and loss of the oracle on the dequantised weights, to the tolerance of
    tests/test_ar_forward_gpu.py (e = 1e-4 max |ref|; nll and loss within 2 e) - the one-model rule holds outside the decode step."""
    import torch.nn.functional as F

    cfg, sd, sdq, bt, _, _ = _reference(size)
    cond, I, E = bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"]
    ids = torch.randint(0, cfg.vocab_size, (B, cfg.num_img_tokens), generator=torch.Generator().manual_seed(8))
    ref = R.gpt_forward(sdq, cfg, ids.reshape(-1, cfg.num_cams, cfg.num_cam_tokens), cond, I, E)
    exact = R.gpt_forward(sd, cfg, ids.reshape(-1, cfg.num_cams, cfg.num_cam_tokens), cond, I, E)
    e = 1e-4 * ref.abs().max().item()
    ref_nll = F.cross_entropy(ref.reshape(-1, ref.shape[-1]), ids.reshape(-1), reduction="none").reshape(ids.shape)
    ctx = _ctx(cfg, sd)
    logits, nll, loss = ctx.ar_forward(cond, I, E, ids, target=ids)
    assert ctx.status() == 0
    ctx.close()
    cam = lambda dec: dec[:, cfg.backward_shuffle_idx.to(dec.device)]
    err = ((cam(logits).cpu() - ref).abs().max() / ref.abs().max()).item()
    d_nll = (cam(nll).cpu() - ref_nll).abs().max().item()
    d_model = ((exact - ref).abs().max() / ref.abs().max()).item()
    print(f"{size}: one-pass logits rel err {err:.3e}  |nll - ref| {d_nll:.3e}  e {e:.3e}   (the quantised model is {d_model:.2e} from the unquantised one)")
    assert err < 1e-4 and d_nll <= 2 * e and abs(loss.item() - ref_nll.mean().item()) <= 2 * e
    assert d_model > 10 * 1e-4       # ... and it IS another model: scoring the unquantised weights would miss the bound


def test_refused_combinations():
    from bevgen_amd.runtime import Context

    cfg, sd, _, _, _, _ = _reference("small")
    with pytest.raises(RuntimeError, match="decode_weights = i8 needs the fused decode path"):   # like decode_weights='f16'
        _ctx(cfg, sd, decode_path="per_op")
    with pytest.raises(ValueError, match=r"weights='f16'.*decode_weights='i8'"):
        Context(cfg, route="ar", precision="f16x3", weights="f16", decode_weights="i8")
    # the C library refuses the pair as well, naming both fields (a caller that fills bevgen_cfg itself)
    from bevgen_amd import runtime

    ctx = Context(cfg, route="ar", precision="f16x3", decode_weights="i8")
    ctx.close()
    saved = runtime.decode_weight_dtype
    runtime.decode_weight_dtype = lambda route, weights, decode_weights: runtime.DECODE_WEIGHTS[decode_weights]
    try:
        bad = Context(cfg, route="ar", precision="f16x3", weights="f16", decode_weights="i8")
        bad.load_state_dict(sd)
        bad.set_tables()
        with pytest.raises(RuntimeError, match=r"weight_dtype = f16.*decode_weight_dtype = i8"):
            bad.finalize()
        bad.close()
    finally:
        runtime.decode_weight_dtype = saved
