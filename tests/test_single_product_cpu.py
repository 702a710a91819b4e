"""precision='f16x1' (Route M's single-product mode: f16(A) f16(W)^T with fp32 accumulation, one MFMA per projection product) without a GPU: how the key reaches the
drop-in modules, the launch plan of a single-product GEMM, and the preconditions of tests/test_single_product_gpu.py.

Preconditions (measured on the CPU; the GPU tests rest on them):
  (a) on the operator inputs of the GPU tests, gelu(f16(a) f16(w)^T + b) + r with `a` rounded lies 1.77e-4 .. 1.83e-4 (relative Frobenius, fp64) from the same expression with
      `a` unrounded - two orders above the 2e-6 bound of the operator test, which therefore tells a kernel that still multiplies a's low plane from one that does not;
  (b) on m_tiny_rays / m_tiny_6cam the single-product emulation of the oracle with its products accumulated in fp32 and in fp64 gives logits 2.2e-4 / 1.9e-4 apart, against
      the mode's own distance d_mode = 5.7e-4 / 5.6e-4 from the rounded-weights oracle: a rounding to f16 flips where its input moves by an fp32 ulp, so two faithful
      evaluations of the mode differ by about 0.4 d_mode, and the GPU test's window [0.5, 2] d_mode leaves room for that."""
import json
import os
import subprocess

import pytest
import torch

import single_product_common as SP
from bevgen_amd import presets
from bevgen_amd.modules import options as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _clean_env(monkeypatch):
    for v in O.ENV.values():
        monkeypatch.delenv(v, raising=False)


# ================================================================================================ the key
@pytest.mark.parametrize("route", ["maskgit", "vq", "ar"])
def test_resolve_accepts_f16x1(monkeypatch, route):
    _clean_env(monkeypatch)
    assert O.resolve({"precision": "f16x1"}, route)["precision"] == "f16x1"
    monkeypatch.setenv("BEVGEN_PRECISION", "f16x1")
    assert O.resolve(None, route)["precision"] == "f16x1"
    assert O.resolve({"precision": "f16x3"}, route)["precision"] == "f16x3"        # explicit > environment


def test_unknown_precision_still_raises(monkeypatch):
    _clean_env(monkeypatch)
    for bad in ("f16x2", "bf16", "f16"):
        with pytest.raises(ValueError, match="precision"):
            O.resolve({"precision": bad}, "maskgit")
        with pytest.raises(ValueError, match="precision"):
            O.pop_runtime_options({"precision": bad})
    monkeypatch.setenv("BEVGEN_PRECISION", "f16x1r")
    with pytest.raises(ValueError, match="precision"):
        O.resolve(None, "maskgit")


def test_maskgit_dropin_hands_f16x1_down(monkeypatch):
    _clean_env(monkeypatch)
    from bevgen_amd.modules.stage1.vqgan import VQModel
    from bevgen_amd.modules.stage2.cond_transformer_multi_view_muse import Net2NetTransformer
    from bevgen_amd.modules.stage2.muse_maskgit_pytorch import MaskGit, MaskGitTransformerMultiView

    cfg = presets.tiny_route_m(3, legacy=False, latent=(8, 8))

    def transformer(**kw):
        return MaskGitTransformerMultiView(num_tokens=cfg.vocab_size, dim=cfg.num_embed, seq_len=cfg.cam_latent_res, depth=cfg.num_layers, dim_head=64, heads=cfg.num_heads,
                                           ff_mult=4, cfg=cfg, **kw)

    # a key next to the transformer's `_target_`
    mg = MaskGit(image_size=cfg.cam_latent_res, transformer=transformer(precision="f16x1"), self_token_critic=True)
    assert mg.runtime_options("maskgit") == {"precision": "f16x1", "weights": "f32"}
    # MaskGit's own constructor key
    mg = MaskGit(image_size=cfg.cam_latent_res, transformer=transformer(), self_token_critic=True, precision="f16x1")
    assert mg.runtime_options("maskgit")["precision"] == "f16x1"
    # the owner's key reaches the modules it owns; one given to a module itself wins
    mg = MaskGit(image_size=cfg.cam_latent_res, transformer=transformer(), self_token_critic=True)
    vq = VQModel(ddconfig=presets.VQ_DDCONFIG_TINY, n_embed=64, embed_dim=64)
    vq3 = VQModel(ddconfig=presets.VQ_DDCONFIG_TINY, n_embed=64, embed_dim=64, precision="f16x3")
    Net2NetTransformer(mg, vq, vq3, cfg, precision="f16x1")
    assert mg.runtime_options("maskgit")["precision"] == "f16x1" and vq.runtime_options("vq")["precision"] == "f16x1" and vq3.runtime_options("vq")["precision"] == "f16x3"


def test_route_a_dropin_hands_f16x1_down(monkeypatch):
    _clean_env(monkeypatch)
    from bevgen_amd.modules.stage1.vqgan import VQModel
    from bevgen_amd.modules.stage2.cond_transformer_multi_view import Net2NetTransformer
    from bevgen_amd.modules.transformer.mingpt_sparse import GPT

    gpt = GPT(presets.tiny_route_a(3, block=4))
    vq = VQModel(ddconfig=presets.VQ_DDCONFIG_TINY, n_embed=64, embed_dim=64)
    Net2NetTransformer(gpt, vq, None, precision="f16x1")
    assert gpt.runtime_options("ar")["precision"] == "f16x1" and vq.runtime_options("vq")["precision"] == "f16x1"


def test_binding_names_the_mode():
    import re

    from bevgen_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"BEVGEN_PRECISION_F16X1\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == _lib.PRECISION_F16X1 and _lib.PRECISION_F16X1 not in (_lib.PRECISION_FP32, _lib.PRECISION_BF16, _lib.PRECISION_F16X3)


# ================================================================================================ the launch plan
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_single_product_plan_is_the_w16_plan_and_never_stream_k(tmp_path):
    from test_gemm_plan_cpu import EXPECTED

    exe = str(tmp_path / "gemm_plan_single")
    r = subprocess.run([HIPCC, "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "bevgen_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "host", "gemm_plan_single.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = list(EXPECTED)
    p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])   # (a sanitizer report goes to stderr)
    out = [json.loads(line) for line in p.stdout.splitlines()]
    assert len(out) == len(cases)
    for c, res in zip(cases, out):
        assert res.get("same") == 1 and res["launches"] == len(EXPECTED[c]), (c, res)
        assert res["sk_single"] == 0 and res["sk_same"] == 1, (c, res)
    # ... while the same switch and force do route launches without the flag to the stream-K kernel: the count above is not zero for want of a candidate
    assert sum(res["sk_plain"] for res in out) >= 4, out


# ================================================================================================ preconditions of the GPU tests
@pytest.mark.parametrize("shape", [s for s, _ in SP.OP_CASES])
def test_precondition_a_rounding_the_activation_shows(shape):
    rounded, unrounded = SP.op_references(*shape)
    d = SP.rel_fro(rounded, unrounded)
    print(f"single_product precondition (a) M,N,K={shape}: rel_fro(rounded a, unrounded a) = {d:.3e}")
    assert d >= 1e-4, (shape, d)


@pytest.mark.parametrize("name", SP.MODEL_CASES)
def test_precondition_b_two_evaluations_of_the_mode_agree_within_half_its_distance(name, monkeypatch):
    lr, er = SP.oracle_forward(name, monkeypatch)
    le, ee = SP.oracle_forward(name, monkeypatch, torch.float32)
    l64, e64 = SP.oracle_forward(name, monkeypatch, torch.float64)
    d_mode, noise = SP.rel_fro(le, lr), SP.rel_fro(le, l64)
    print(f"single_product precondition (b) {name}: d_mode = {d_mode:.3e} (embed {SP.rel_fro(ee, er):.3e}), fp32 vs fp64 products = {noise:.3e} (embed {SP.rel_fro(ee, e64):.3e})")
    assert noise < 0.5 * d_mode, (name, noise, d_mode)
    assert d_mode > 1e-4, (name, d_mode)   # (the mode is not the two-product mode)
