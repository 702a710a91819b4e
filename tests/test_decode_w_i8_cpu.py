"""decode_weights='i8' (int8 projection weights with one fp32 scale per output row, BEVGEN_W_I8) without a GPU: the CPU quantiser's properties, the mode's way through
the options and the Context constructor, the header, and the decode plan (bevgen_amd/csrc/ar_plan.h) for int8 against fp16 images."""
import json
import os
import re
import subprocess

import pytest
import torch

import decode_w_i8_ref as W
from bevgen_amd import _lib, presets
from bevgen_amd.modules import options as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def matrix(seed, n, k, heavy=False):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    if heavy:
        w = w * torch.exp(2.0 * torch.randn(n, k, generator=g))
    return w


# ------------------------------------------------------------------------------------------------ quantiser
def test_zero_row_gives_scale_zero_and_rows_below_the_threshold_too():
    w = matrix(1, 6, 96)
    w[2] = 0.0
    w[4] *= 1e-33 / w[4].abs().max()
    codes, scales, deq = W.quantise_rows(w)
    for r in (2, 4):
        assert float(scales[r]) == 0.0 and bool((codes[r] == 0).all()) and bool((deq[r] == 0).all())
    assert bool((scales[[0, 1, 3, 5]] > 0).all())


def test_row_whose_largest_value_is_negative():
    w = matrix(2, 3, 64)
    w[1, 17] = -3.0 * w[1].abs().max()
    w[2, :] = -7.25
    codes, scales, deq = W.quantise_rows(w)
    assert float(codes[1, 17]) == -127.0 and float(scales[1]) > 0                 # the scale is a magnitude
    assert bool((codes[2] == -127).all()) and torch.equal(deq[2], codes[2] * scales[2])
    assert abs(float(deq[1, 17]) - float(w[1, 17])) <= 1e-6 * abs(float(w[1, 17]))


@pytest.mark.parametrize("heavy", [False, True])
def test_codes_stay_within_127_and_the_error_within_half_a_step(heavy):
    w = matrix(3, 48, 256, heavy)
    w[0, 0], w[0, 1] = 3.0e38, -3.0e38                                            # the top of the fp32 range: code 127 x scale must not round past it
    codes, scales, deq = W.quantise_rows(w)
    assert float(codes.abs().max()) == 127.0 and float(codes.min()) >= -127.0
    assert bool((codes == codes.round()).all())
    assert bool((codes.abs().amax(-1) == 127).all())                              # every live row uses the whole range
    assert bool(scales.isfinite().all()) and bool(deq.isfinite().all())
    # |w - code * scale| <= scale / 2, up to the fp32 rounding of w * inv (one part in 2^23 of 127 steps) and of code * scale
    err = (deq.double() - w.double()).abs()
    bound = scales.double().unsqueeze(-1) * (0.5 + 127 * 2.0 ** -22)
    assert bool((err <= bound).all()), float((err / scales.double().unsqueeze(-1)).max())


def test_the_quantiser_reproduces_itself_on_its_own_output():
    """bevgen_finalize replaces the master matrices by code * scale and packs the decode images from THAT matrix: quantising the dequantised row must give the same
    codes and the same scale.  The scale, for every fp32 mantissa of the row maximum in three binades; codes and values on random rows."""
    mant = (torch.arange(1 << 23, dtype=torch.int32) | 0x3F800000).view(torch.float32)          # every float in [1, 2)
    for binade in (1.0, 2.0 ** -9, 2.0 ** 6):
        amax = mant * binade
        scale = amax / torch.tensor(127.0)
        again = (torch.tensor(127.0) * scale) / torch.tensor(127.0)                            # the row maximum is code 127: its dequantised value is 127 * scale
        assert torch.equal(again, scale)
    for heavy in (False, True):
        codes, scales, deq = W.quantise_rows(matrix(4, 64, 512, heavy))
        c2, s2, d2 = W.quantise_rows(deq)
        assert torch.equal(c2, codes) and torch.equal(s2, scales) and torch.equal(d2, deq)


def test_state_dict_helper_quantises_the_projection_matrices_only_and_qkv_row_by_row():
    from oracle import cases

    cfg = presets.route_a(3, num_layers=2, dim=256, heads=4, vocab=64, cam_res=(64, 64), cam_latent_res=(4, 5), bev_latent_res=(4, 4), block=16, window_len=8)
    sd = cases.gpt_state_dict(cfg, 1234)
    sdq = W.quantize_projection_weights_i8(sd)
    changed = sorted(k for k in sd if not torch.equal(sd[k], sdq[k]))
    want = sorted(["head.weight"] + [f"blocks.{i}.{m}.weight" for i in range(2) for m in ("attention.query", "attention.key", "attention.value", "mlp.0", "mlp.2")])
    assert changed == want
    # the library fuses q | k | v into [3 D, D] and quantises its rows: the same as each matrix row by row
    q = [sd[f"blocks.0.attention.{n}.weight"] for n in ("query", "key", "value")]
    fused = W.quantise_rows(torch.cat(q, 0))[2]
    assert torch.equal(fused, torch.cat([sdq[f"blocks.0.attention.{n}.weight"] for n in ("query", "key", "value")], 0))


# ------------------------------------------------------------------------------------------------ options, constructor, header
def test_options_accept_i8(monkeypatch):
    for name in O.ENV.values():
        monkeypatch.delenv(name, raising=False)
    kw = {"decode_weights": "i8", "lr": 1e-4}
    assert O.pop_runtime_options(kw) == {"decode_weights": "i8"} and kw == {"lr": 1e-4}
    assert O.resolve({"decode_weights": "i8"}, "ar")["decode_weights"] == "i8"
    monkeypatch.setenv("BEVGEN_DECODE_WEIGHTS", "i8")
    assert O.resolve(None, "ar")["decode_weights"] == "i8"
    assert O.resolve({"decode_weights": "f16"}, "ar")["decode_weights"] == "f16"          # an explicit key still wins
    assert O.DROPIN_DEFAULTS["decode_weights"] == "f32"                                   # opt-in: never the default
    monkeypatch.setenv("BEVGEN_DECODE_WEIGHTS", "i4")
    with pytest.raises(ValueError, match="decode_weights"):
        O.resolve(None, "ar")


def test_runtime_maps_i8_to_2_and_refuses_it_next_to_f16_weights():
    """the check the Context constructor runs on its modes (a Context itself needs a GPU: tests/test_decode_w_i8_models_gpu.py constructs the refused pair there)"""
    from bevgen_amd import runtime

    assert runtime.DECODE_WEIGHTS == {"f32": 0, "f16": 1, "i8": 2} and runtime.DECODE_WEIGHTS["i8"] == _lib.W_I8
    assert runtime.decode_weight_dtype("ar", "f32", "i8") == 2 and runtime.decode_weight_dtype("ar", "f16", "f16") == 1 and runtime.decode_weight_dtype("ar", "f32", "f32") == 0
    with pytest.raises(ValueError, match="decode_weights"):
        runtime.decode_weight_dtype("ar", "f32", "i4")
    # weights='f16' rounds the prefill matrices to fp16; dequantised int8 values are not fp16-representable: no single model, refused
    with pytest.raises(ValueError, match=r"weights='f16'.*decode_weights='i8'"):
        runtime.decode_weight_dtype("ar", "f16", "i8")
    assert runtime.decode_weight_dtype("maskgit", "f16", "i8") == 2       # (Route M has no decode weights: the key is carried, never read)


def test_gpt_takes_i8_as_a_constructor_key(monkeypatch):
    for name in O.ENV.values():
        monkeypatch.delenv(name, raising=False)
    from bevgen_amd.modules.transformer.mingpt_sparse import GPT

    gpt = GPT(presets.tiny_route_a(3, block=4), decode_weights="i8")
    assert gpt.runtime_options("ar")["decode_weights"] == "i8" and gpt.runtime_options("ar")["kv_cache"] == "f32"


def test_header_lib_and_options_agree():
    header = open(os.path.join(ROOT, "include", "bevgen_hip.h")).read()
    assert int(re.search(r"BEVGEN_W_I8\s*=\s*(\d+)", header).group(1)) == _lib.W_I8 == 2
    assert int(re.search(r"BEVGEN_W_F16\s*=\s*(\d+)", header).group(1)) == _lib.W_F16 == 1
    assert int(re.search(r"BEVGEN_W_F32\s*=\s*(\d+)", header).group(1)) == _lib.W_F32 == 0
    assert int(re.search(r"#define\s+BEVGEN_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == 10
    assert "bevgen_op_quantize_rows_i8" in header and "bevgen_op_quantize_rows_i8" in _lib.SIGNATURES
    assert O.CHOICES["decode_weights"] == ("f32", "f16", "i8")
    assert "i8" in O.__doc__.split("decode_weights")[1].split("decode_path")[0]


# ------------------------------------------------------------------------------------------------ the decode plan
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_int8_plan_equals_fp16_plan(tmp_path):
    """tests/host/ar_plan_i8_dump.cpp, built for the host with the address and undefined-behaviour sanitizers as tests/test_ar_plan_cpu.py builds its harness."""
    exe = str(tmp_path / "ar_plan_i8_dump")
    r = subprocess.run([HIPCC, "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "bevgen_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "host", "ar_plan_i8_dump.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
    got = json.loads(p.stdout)
    assert got["cases"] > 5000 and got["differ"] == 0, got
    assert got["f32_differs"] > 0, got                       # the grid does tell storage kinds apart
    FUSED, SPLIT = 0, 2
    assert got["i8_auto_b1"] == [FUSED, 1, 1] and got["f32_auto_b1"] == [SPLIT, 1, 0], got   # auto: the fused layer with its single MLP launch at every batch size
