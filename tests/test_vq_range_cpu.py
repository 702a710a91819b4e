"""precision='f16x3r' (range-safe VQGAN decode) as the option plumbing and the binding see it; no GPU."""
import ctypes
import re

import pytest

from bevgen_amd import _lib, presets
from bevgen_amd.modules import options as O


def _clean_env(monkeypatch):
    for v in O.ENV.values():
        monkeypatch.delenv(v, raising=False)


def test_options_accept_f16x3r_as_key_and_environment(monkeypatch):
    _clean_env(monkeypatch)
    assert "f16x3r" in O.CHOICES["precision"]
    assert O.pop_runtime_options({"precision": "f16x3r", "lr": 1.0}) == {"precision": "f16x3r"}
    assert O.resolve({"precision": "f16x3r"}, "vq") == {"precision": "f16x3r", "weights": "f32"}
    assert O.resolve(None, "vq") == {"precision": "f16x3", "weights": "f32"}          # the default keeps refusing
    monkeypatch.setenv("BEVGEN_PRECISION", "f16x3r")
    for route in ("vq", "maskgit", "ar"):
        assert O.resolve(None, route)["precision"] == "f16x3r"
    assert O.resolve({"precision": "fp32"}, "vq")["precision"] == "fp32"               # explicit key > environment
    monkeypatch.setenv("BEVGEN_PRECISION", "f16x3s")
    with pytest.raises(ValueError, match="precision"):
        O.resolve(None, "vq")


def test_no_new_route_key(monkeypatch):
    _clean_env(monkeypatch)
    assert set(O.resolve(None, "vq")) == {"precision", "weights"}
    assert set(O.resolve(None, "maskgit")) == {"precision", "weights"}
    assert set(O.CHOICES) == set(O.ENV) == set(O.DROPIN_DEFAULTS)


def test_net2net_hands_f16x3r_down_to_stage1_and_maskgit(monkeypatch):
    _clean_env(monkeypatch)
    from bevgen_amd.modules.stage1.vqgan import VQModel
    from bevgen_amd.modules.stage2.cond_transformer_multi_view_muse import Net2NetTransformer
    from bevgen_amd.modules.stage2.muse_maskgit_pytorch import MaskGit, MaskGitTransformerMultiView

    cfg = presets.tiny_route_m(3, legacy=False, latent=(8, 8))
    tr = MaskGitTransformerMultiView(num_tokens=cfg.vocab_size, dim=cfg.num_embed, seq_len=cfg.cam_latent_res, depth=cfg.num_layers, dim_head=64,
                                     heads=cfg.num_heads, ff_mult=4, cfg=cfg)
    mg = MaskGit(image_size=cfg.cam_latent_res, transformer=tr, self_token_critic=True)
    vq = VQModel(ddconfig=presets.VQ_DDCONFIG_TINY, n_embed=64, embed_dim=64)
    Net2NetTransformer(mg, vq, None, cfg, precision="f16x3r")
    assert mg.runtime_options("maskgit") == {"precision": "f16x3r", "weights": "f32"}
    assert vq.runtime_options("vq") == {"precision": "f16x3r", "weights": "f32"}


def test_net2net_hands_f16x3r_down_to_gpt(monkeypatch):
    _clean_env(monkeypatch)
    from bevgen_amd.modules.stage1.vqgan import VQModel
    from bevgen_amd.modules.stage2.cond_transformer_multi_view import Net2NetTransformer
    from bevgen_amd.modules.transformer.mingpt_sparse import GPT

    gpt = GPT(presets.tiny_route_a(3, block=4))
    vq = VQModel(ddconfig=presets.VQ_DDCONFIG_TINY, n_embed=64, embed_dim=64, precision="f16x3")
    Net2NetTransformer(gpt, vq, None, precision="f16x3r")
    assert gpt.runtime_options("ar")["precision"] == "f16x3r"
    assert vq.runtime_options("vq")["precision"] == "f16x3"                            # a module's own key wins over its owner's


def test_cfg_struct_keeps_its_size_and_gains_vq_range():
    assert ctypes.sizeof(_lib.bevgen_cfg) == 4 * (3 + 5 + 3 + 3 + 3 + 2 + 8 + 8 + 1 + 16)
    # the field is the first of the former ten reserved words
    assert _lib.bevgen_cfg.vq_range.offset == ctypes.sizeof(_lib.bevgen_cfg) - 4 * 10
    assert _lib.bevgen_cfg.reserved.offset == _lib.bevgen_cfg.vq_range.offset + 4 and _lib.bevgen_cfg.reserved.size == 4 * 9
    assert _lib.bevgen_cfg().vq_range == 0                                             # zero = refuse, as before
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"int32_t\s+vq_range;", header) and re.search(r"int32_t\s+reserved\[9\];", header)


def test_new_symbols_are_declared_in_header_and_binding():
    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in ("bevgen_vq_range_exponents", "bevgen_op_range_split"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert len(_lib.SIGNATURES["bevgen_vq_range_exponents"][1]) == 4 and len(_lib.SIGNATURES["bevgen_op_range_split"][1]) == 8
    m = re.search(r"#define\s+BEVGEN_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.ABI_VERSION
