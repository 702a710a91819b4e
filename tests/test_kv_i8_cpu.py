"""The int8 KV-cache format on the CPU (tests/kv_i8_ref.py: the quantiser the device kernels must reproduce byte for byte) and how the mode reaches the host:
options.py, _lib and the C header agree on kv_cache='i8' = BEVGEN_KV_I8 = 2.  No GPU."""
import os
import re

import pytest
import torch

import kv_i8_ref as Q
from bevgen_amd import _lib
from bevgen_amd.modules import options as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(seed, shape, heavy=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(*shape, 64, generator=g)
    if heavy:   # heavy-tailed rows: a few elements carry the amax
        v = v * torch.exp(2.0 * torch.randn(*shape, 64, generator=g))
    return v


@pytest.mark.parametrize("heavy", [False, True], ids=["gauss", "heavy"])
def test_pack_unpack_round_trip(heavy):
    B, H, L = 2, 3, 5
    v = rows(1, (B, H, L), heavy) * 3
    buf = Q.pack(v)
    assert buf.dtype == torch.uint8 and buf.numel() == Q.ROW_BYTES * B * H * L
    codes, scales, deq = Q.unpack(buf, B, H, L)
    c0, s0 = Q.quantise(v)
    assert torch.equal(codes, c0) and torch.equal(scales, s0)
    assert torch.equal(Q.pack_planes(codes, scales), buf)
    # the scale plane starts at byte 64 B H Lmax
    assert torch.equal(buf[64 * B * H * L:].view(torch.float32).reshape(B, H, L), s0)
    # a dequantised row is a fixed point of the quantiser's codes (|code| <= 127 and the amax element maps to +-127 again)
    c1, _ = Q.quantise(deq)
    assert torch.equal(c1, codes)
    # per element half a step, evaluated in fp64.  (In fp32 the four roundings of scale, inv, r * inv and code * scale can push an element that sits within 127 s 2^-22
    # of a half step past it - 2 elements in 1.3 million random ones; these rows keep 4e-5 of distance from the bound, the rounding is 1e-7.)
    err = (deq.double() - v.double()).abs()
    bound = scales.double().unsqueeze(-1) * 0.5
    assert bool((err <= bound).all()), f"worst excess {(err - bound).max().item():.3e}"
    assert bool((scales == v.abs().amax(-1) / torch.tensor(127.0)).all())
    # the element that carries the amax is reproduced to fp32 rounding
    idx = v.abs().argmax(-1, keepdim=True)
    assert bool((codes.gather(-1, idx).abs() == 127).all())


def test_zero_and_tiny_rows():
    v = rows(2, (1, 1, 4))
    v[0, 0, 1] = 0.0
    v[0, 0, 2] = torch.linspace(-9e-31, 9e-31, 64)           # amax < 1e-30: treated as a zero row
    v[0, 0, 3] = torch.linspace(-2e-30, 2e-30, 64)           # just above: quantised like any other row
    codes, scales, deq = Q.unpack(Q.pack(v), 1, 1, 4)
    for r in (1, 2):
        assert scales[0, 0, r] == 0.0 and not codes[0, 0, r].any() and not deq[0, 0, r].any()
    assert scales[0, 0, 3] > 0 and codes[0, 0, 3, 0] == -127 and codes[0, 0, 3, 63] == 127
    assert scales[0, 0, 0] > 0


def test_codes_never_reach_minus_128():
    v = torch.cat([rows(3, (1, 1, 64)), rows(4, (1, 1, 64), heavy=True)], 2)
    v[0, 0, 0] = -v[0, 0, 0].abs()                           # a row whose amax sits on a negative element ...
    v[0, 0, 1, :] = -7.25                                    # ... and one made of it alone
    v[0, 0, 2, :] = 3.0e38                                   # a row at the top of the fp32 range (code 127 x scale must not round past it)
    v[0, 0, 2, 1] = -3.0e38
    codes, scales, deq = Q.unpack(Q.pack(v), 1, 1, 128)
    assert int(codes.min()) == -127 and int(codes.max()) == 127
    assert bool((codes[0, 0, 1] == -127).all())
    assert bool(scales.isfinite().all()) and bool(deq.isfinite().all())


def test_options_accept_i8(monkeypatch):
    for name in O.ENV.values():
        monkeypatch.delenv(name, raising=False)
    kw = {"kv_cache": "i8", "lr": 1e-4}
    assert O.pop_runtime_options(kw) == {"kv_cache": "i8"} and kw == {"lr": 1e-4}
    assert O.resolve({"kv_cache": "i8"}, "ar")["kv_cache"] == "i8"
    monkeypatch.setenv("BEVGEN_KV_CACHE", "i8")
    assert O.resolve(None, "ar")["kv_cache"] == "i8"
    assert O.resolve({"kv_cache": "f16"}, "ar")["kv_cache"] == "f16"       # an explicit key still wins
    assert O.resolve(None, "ar")["kv_cache"] != O.DROPIN_DEFAULTS["kv_cache"] == "f32"   # opt-in: never the default
    with pytest.raises(ValueError, match="kv_cache"):
        O.pop_runtime_options({"kv_cache": "bf16"})
    monkeypatch.setenv("BEVGEN_KV_CACHE", "bf16")
    with pytest.raises(ValueError, match="kv_cache"):
        O.resolve(None, "ar")


def test_gpt_takes_i8_as_a_constructor_key(monkeypatch):
    for name in O.ENV.values():
        monkeypatch.delenv(name, raising=False)
    from bevgen_amd import presets
    from bevgen_amd.modules.transformer.mingpt_sparse import GPT

    gpt = GPT(presets.tiny_route_a(3, block=4), kv_cache="i8")
    assert gpt.runtime_options("ar")["kv_cache"] == "i8"


def test_header_lib_and_options_agree():
    header = open(os.path.join(ROOT, "include", "bevgen_hip.h")).read()
    assert int(re.search(r"BEVGEN_KV_I8\s*=\s*(\d+)", header).group(1)) == _lib.KV_I8 == 2
    assert int(re.search(r"BEVGEN_KV_F16\s*=\s*(\d+)", header).group(1)) == _lib.KV_F16 == 1
    assert int(re.search(r"BEVGEN_STATUS_KV_NONFINITE\s*=\s*(\d+)", header).group(1)) == _lib.STATUS_KV_NONFINITE == 64
    assert O.CHOICES["kv_cache"] == ("f32", "f16", "i8")
    assert "i8" in O.__doc__


@pytest.mark.parametrize("name", ["a_tiny_blk16", "a_tiny_6cam", "a_tiny_d06"])
def test_oracle_with_i8_rows_stays_under_the_model_cap(name):
    """What tests/test_kv_i8_models_gpu.py relies on: with its K / V rows passed through the int8 quantiser, the oracle's Route A restatement (teacher forced) stays
    below the 0.1 cap on the per-step relative logit distance from the golden fp32 logits - a wrong plane, stride or scale on the device gives O(1)."""
    import numpy as np

    from conftest import golden
    from oracle import cases, restate as R

    case = cases.CASES[name]
    g = golden("route_a_" + name)
    cfg = case.make_cfg()
    sd = cases.golden_state_dict(case, cfg, g)
    t = lambda a, dt=None: torch.from_numpy(np.asarray(a)).to(dt) if dt is not None else torch.from_numpy(np.asarray(a))
    cond, I, E = t(g["cond_ids"], torch.long), t(g["I_inv"]), t(g["E_inv"])
    want, ref = t(g["sample_greedy"], torch.long), t(g["step_logits"])
    exact = Q.teacher_forced_logits(R.ARCache(sd, cfg, cond, I, E), cfg, want)
    i8 = Q.teacher_forced_logits(Q.i8_cache_class(R.ARCache)(sd, cfg, cond, I, E), cfg, want)
    d_exact, d_i8 = Q.step_distance(exact, ref), Q.step_distance(i8, ref)
    agree = (i8.argmax(-1) == ref.argmax(-1)).float().mean().item()
    print(f"{name}: oracle fp32 rows {d_exact:.2e}, int8 rows {d_i8:.2e}, top-1 agreement {agree:.3f}")
    assert d_exact < 1e-4            # the wrapper changes nothing but the stored rows
    assert 1e-4 < d_i8 < 0.1         # ... and the stored rows are really quantised
