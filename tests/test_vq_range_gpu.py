"""precision='f16x3r': the range-safe split-precision VQGAN decode (include/bevgen_hip.h bevgen_cfg.vq_range).

The un-normalised residual stream of the decoder becomes an f16 operand in front of the upsample, nin_shortcut and conv_in convolutions; 'f16x3' refuses a checkpoint whose
stream passes 65504 there (test_status_gpu.py), 'f16x3r' rescales the tensor by a per-tensor power of two chosen on the device.  Covered here:
  * the heavy-tailed fixture that 'f16x3' refuses decodes within the decoder's bounds of the other two modes, and at least one site really rescaled;
  * where nothing overflows every exponent is 0 and the output is bit-identical to 'f16x3' in all three output modes;
  * the transformer routes treat the value as 'f16x3';
  * the operand preparation alone (op_range_split) against a numpy restatement: exponent rule, reconstruction, finiteness, NaN / inf refused;
  * exponents are per call.

Measured on the heavy fixture (MI355X, max |a - golden| / max |golden| of the raw pixels): f16x3r 2.66e-5, fp32 1.44e-5 (bound 1e-4); denormalised pixels of f16x3r within
6.3e-4 (bound 1e-3); exponents 0, 0, 0, 0, 0, 3 (experiments/r08.md).
"""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import cases

pytestmark = pytest.mark.gpu


def _t(a, dtype=None):
    t = torch.from_numpy(np.asarray(a))
    return t.to(dtype) if dtype is not None else t


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


_SD = {}


def _vq_sd(v):
    key = (v["seed"], v.get("heavy"), v.get("lo"), v.get("hi"))
    if key not in _SD:      # built once per checkpoint and left unchanged (load_state_dict copies to the device)
        _SD[key] = _build_vq_sd(v)
    return _SD[key]


def _build_vq_sd(v):
    sd = cases.vq_state_dict(v["dd"], v["n_embed"], v["embed_dim"], v["seed"], with_encoder=True)
    if "heavy" in v:
        sd = cases.heavy_tail(sd, v["heavy"], lo=v.get("lo", 30.0), hi=v.get("hi", 100.0))
    return sd


def _vq_ctx(v, precision):
    from bevgen_amd.runtime import Context

    ctx = Context(None, vq_ddconfig=v["dd"], vq_n_embed=v["n_embed"], vq_embed_dim=v["embed_dim"], precision=precision)
    ctx.load_state_dict(_vq_sd(v), prefix="first_stage_model.")
    ctx.finalize()
    return ctx


def _make_ctx(cfg, route, sd, **kw):
    from bevgen_amd.runtime import Context

    ctx = Context(cfg, route=route, **kw)
    ctx.load_state_dict(sd)
    ctx.set_tables()
    ctx.finalize()
    return ctx


@pytest.fixture(scope="module")
def heavy_ctx():
    """One 'f16x3r' context on the heavy-tailed checkpoint for the tests that only decode with it."""
    ctx = _vq_ctx(cases.VQ_TINY_HEAVY, "f16x3r")
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------ the checkpoint 'f16x3' refuses
def test_heavy_tailed_checkpoint_decodes_in_f16x3r(heavy_ctx):
    v = cases.VQ_TINY_HEAVY
    g = golden("vq_tiny_heavy")
    ids = _t(g["ids"], torch.long)
    want_raw, want_px = _t(g["pixels_raw"]), _t(g["pixels_denorm"])
    ctx = heavy_ctx
    raw = ctx.vq_decode(ids, denormalize=False).cpu()
    exps = ctx.vq_range_exponents()
    px = ctx.vq_decode(ids, denormalize=True).cpu()
    assert ctx.status() == 0
    ref = _vq_ctx(v, "fp32")
    raw32 = ref.vq_decode(ids, denormalize=False).cpu()
    ref.close()
    print(f"vq_tiny_heavy raw pixels vs golden: f16x3r rel {rel(raw, want_raw):.3e}, fp32 rel {rel(raw32, want_raw):.3e}; "
          f"denormalised max abs (f16x3r) {(px - want_px).abs().max().item():.3e}; exponents {exps.tolist()}")
    assert rel(raw, want_raw) < 1e-4
    assert (px - want_px).abs().max() < 1e-3
    assert len(exps) > 0 and exps.min() >= 0 and exps.max() >= 1, "no site rescaled: the fixture no longer leaves the f16 range"


def test_heavy_tailed_checkpoint_decode_latents_in_f16x3r(heavy_ctx):
    v = cases.VQ_TINY_HEAVY
    g = golden("vq_tiny_heavy")
    ids = _t(g["ids"], torch.long)
    lat = v["dd"]["resolution"] >> (len(v["dd"]["ch_mult"]) - 1)
    codebook = _vq_sd(v)["quantize.embedding.weight"]
    zq = codebook[ids].reshape(ids.shape[0], lat, lat, v["embed_dim"]).permute(0, 3, 1, 2).contiguous()
    ctx = heavy_ctx
    raw = ctx.vq_decode_latents(zq, denormalize=False).cpu()
    exps = ctx.vq_range_exponents()
    px = ctx.vq_decode_latents(zq, denormalize=True).cpu()
    assert ctx.status() == 0
    assert rel(raw, _t(g["pixels_raw"])) < 1e-4
    assert (px - _t(g["pixels_denorm"])).abs().max() < 1e-3
    assert exps.max() >= 1


# ------------------------------------------------------------------------------------------------ e = 0: the bits of 'f16x3'
@pytest.mark.parametrize("name", ["vq_tiny_heavy_mild", "vq_tiny"])
def test_f16x3r_is_bit_identical_to_f16x3_where_nothing_overflows(name):
    v = {"vq_tiny_heavy_mild": cases.VQ_TINY_HEAVY_MILD, "vq_tiny": cases.VQ_TINY}[name]
    ids = _t(golden(name)["ids"], torch.long)
    a, b = _vq_ctx(v, "f16x3r"), _vq_ctx(v, "f16x3")
    for kw in (dict(denormalize=False), dict(denormalize=True), dict(uint8=True)):
        out_r, out_x = a.vq_decode(ids, **kw).cpu(), b.vq_decode(ids, **kw).cpu()
        assert torch.equal(out_r, out_x), kw
        exps = a.vq_range_exponents()
        assert len(exps) > 0 and (exps == 0).all(), exps
    assert len(b.vq_range_exponents()) == 0     # 'f16x3' has no sites
    assert a.status() == 0 and b.status() == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ the transformer routes: 'f16x3r' is 'f16x3'
def test_route_m_tokens_under_f16x3r_equal_f16x3():
    case = cases.CASES["m_tiny_heavy"]
    g = golden("route_m_m_tiny_heavy")
    cfg = case.make_cfg()
    sd = cases.case_state_dict(case, cfg)
    cond, I, E = _t(g["cond_ids"], torch.long), _t(g["I_inv"]), _t(g["E_inv"])
    out = {}
    for precision in ("f16x3r", "f16x3"):
        ctx = _make_ctx(cfg, "maskgit", sd, precision=precision)
        out[precision] = ctx.maskgit_generate(cond, I, E, timesteps=case.timesteps).cpu()
        assert ctx.status() == 0
        ctx.close()
    assert torch.equal(out["f16x3r"], out["f16x3"])
    assert torch.equal(out["f16x3r"], _t(g["gen_greedy"], torch.long))


def test_route_a_tokens_under_f16x3r_equal_f16x3():
    case = cases.CASES["a_tiny_heavy"]
    g = golden("route_a_a_tiny_heavy")
    cfg = case.make_cfg()
    sd = cases.golden_state_dict(case, cfg, g)
    cond, I, E = _t(g["cond_ids"], torch.long), _t(g["I_inv"]), _t(g["E_inv"])
    out = {}
    for precision in ("f16x3r", "f16x3"):
        ctx = _make_ctx(cfg, "ar", sd, precision=precision)
        out[precision] = ctx.ar_sample(cond, I, E, greedy=True).cpu()
        assert ctx.status() == 0
        ctx.close()
    assert torch.equal(out["f16x3r"], out["f16x3"])
    assert torch.equal(out["f16x3r"], _t(g["sample_greedy"], torch.long))


# ------------------------------------------------------------------------------------------------ the operand preparation alone
def _want_exponent(absmax: float) -> int:
    """0 where absmax < 32768, else the smallest e with absmax 2^-e < 32768 (fp64 restatement of the rule)."""
    e = 0
    while absmax * 2.0 ** -e >= 32768.0:
        e += 1
    return e


def _range_case(n, hw, extreme):
    C = 32
    g = torch.Generator().manual_seed(1000 * n + hw)
    if extreme is None:
        return torch.zeros(n, hw, C)
    x = torch.randn(n, hw, C, generator=g)
    x.view(-1)[(7 * n + 3 * hw) % x.numel()] = -extreme if (n + hw) % 2 else extreme
    return x


@pytest.mark.parametrize("extreme", [None, 1.0, 32767.9, 32768.0, 65519.0, 65520.0, 1e30, 3e38])
@pytest.mark.parametrize("hw", [1, 37])
@pytest.mark.parametrize("n", [1, 2])
def test_op_range_split(gpu_ctx, n, hw, extreme):
    x = _range_case(n, hw, extreme)
    planes, e = gpu_ctx.op_range_split(x.cuda())
    assert gpu_ctx.status() == 0
    e = int(e.item())
    x64 = x.double()
    absmax = x64.abs().max().item()
    assert e == _want_exponent(absmax), (e, absmax)
    assert absmax * 2.0 ** -e < 32768.0
    p = planes.cpu()                                                   # [n hw, C / 32, 2, 32]: hi | lo of every 32-channel block
    assert p.shape == (n * hw, 1, 2, 32) and torch.isfinite(p.float()).all()
    recon = ((p[:, :, 0].double() + p[:, :, 1].double() * 2.0 ** -11) * 2.0 ** e).reshape(n, hw, 32)
    assert rel(recon, x64) < 2e-6                                      # the split's own precision, relative to absmax (as the split-precision operator tests measure it)
    if extreme is not None and extreme >= 32768.0:
        assert e >= 1


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_op_range_split_refuses_non_finite_values(gpu_ctx, bad):
    from bevgen_amd import _lib

    x = _range_case(2, 37, 1.0)
    x[1, 5, 9] = bad
    with pytest.raises(_lib.BevgenError) as ei:
        gpu_ctx.op_range_split(x.cuda())
    assert ei.value.code == _lib.ERR_NUMERIC
    assert gpu_ctx.status() == 0                                       # reported once, then cleared: the shared context stays usable
    planes, e = gpu_ctx.op_range_split(_range_case(1, 1, 1.0).cuda())
    assert int(e.item()) == 0


# ------------------------------------------------------------------------------------------------ exponents belong to a call
def test_exponents_are_per_call(heavy_ctx):
    v = cases.VQ_TINY_HEAVY
    ids_a = _t(golden("vq_tiny_heavy")["ids"], torch.long)
    ids_b = torch.randint(0, v["n_embed"], ids_a.shape, generator=torch.Generator().manual_seed(5))
    ctx = heavy_ctx
    out_a = ctx.vq_decode(ids_a, denormalize=False).cpu()
    exp_a = ctx.vq_range_exponents()
    out_b = ctx.vq_decode(ids_b, denormalize=False).cpu()
    exp_b = ctx.vq_range_exponents()
    out_a2 = ctx.vq_decode(ids_a, denormalize=False).cpu()
    exp_a2 = ctx.vq_range_exponents()
    assert ctx.status() == 0
    fresh = _vq_ctx(v, "f16x3r")
    out_b_fresh = fresh.vq_decode(ids_b, denormalize=False).cpu()
    exp_b_fresh = fresh.vq_range_exponents()
    fresh.close()
    assert len(exp_a) == len(exp_b) == len(exp_a2)
    assert (exp_a == exp_a2).all() and torch.equal(out_a, out_a2)
    assert (exp_b == exp_b_fresh).all() and torch.equal(out_b, out_b_fresh)
