"""MaskGit.forward's validation losses without a GPU: the fp64 restatement (tests/maskgit_loss_common.py) against the imported reference's results stored in
tests/golden/route_m_loss.npz (mask, x and critic input equal; the three losses within 1e-6 relative), the conditions of the inputs those comparisons rest on, the new
entries of the C ABI, the refusals of MaskGit.forward that need no device, and the validation surface of the Route M Net2NetTransformer."""
import inspect
import os

import numpy as np
import pytest
import torch

import maskgit_loss_common as M
from bevgen_amd import _lib

CASES = list(M.LOSS_CASES)
NEW_EXPORTS = ["bevgen_maskgit_loss", "bevgen_op_maskgit_train_mask", "bevgen_op_masked_ce", "bevgen_op_critic_bce"]


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name):
    g, r = M.fixture(), M.fixture_restated(name)
    assert np.array_equal(r["mask"].numpy(), g[name + "_mask"])
    assert np.array_equal(r["x"].numpy(), g[name + "_x"].astype(np.int64))
    assert np.array_equal(r["critic_input"].numpy(), g[name + "_critic_input"].astype(np.int64))
    assert np.array_equal(r["labels"].numpy().astype(np.uint8), g[name + "_labels"])
    errs = {k: _rel(r[k], g[name + "_" + k]) for k in ("ce", "bce", "loss")}
    print(f"{name}: restatement against the reference, relative: {errs}; max |logit| {r['max_logit']:.2f}, max |critic logit| {r['max_critic_logit']:.3f}")
    assert all(e < M.LOSS_RTOL for e in errs.values()), errs
    assert float(g[name + "_ce_only"]) == float(g[name + "_ce"])           # train_only_generator=True returns the same cross-entropy, alone
    assert _rel(g[name + "_max_logit"], r["max_logit"]) < 1e-9 and _rel(g[name + "_max_critic_logit"], r["max_critic_logit"]) < 1e-9
    alone = M.restate(name, M.fixture_inputs(name), with_critic=False)
    assert float(alone["loss"]) == float(r["ce"])


@pytest.mark.parametrize("name", CASES)
def test_input_conditions(name):
    inp, r = M.fixture_inputs(name), M.fixture_restated(name)
    distinct, margin_ok = M.input_conditions(inp, r)
    print(f"{name}: top-2 margin at the masked positions {r['margin']:.3e} (>= {M.MIN_MARGIN}), counts {[int(v) for v in r['n']]}")
    assert distinct and margin_ok and M.count_conditions(inp)
    assert int(r["mask"].sum()) == int(r["n"].sum()) and torch.equal(r["mask"].sum(-1), r["n"].long())    # no position is left out of any comparison
    # the stored inputs are the rule's: drawn from the recorded seed
    drawn = M.draw_inputs(name, M.LOSS_CASES[name])
    assert all(torch.equal(drawn[k], inp[k]) for k in ("ids", "time_u", "perm_u", "gumbel_u")) and drawn["temperature"] == inp["temperature"]
    assert float(np.float32(inp["temperature"])) == inp["temperature"]        # the library takes the temperature as a float: nothing is lost


def test_tie_rule_is_an_argsort_order():
    """equal uniforms rank by index: the mask of train_mask is what argsort gives for SOME valid order, and the one a stable sort gives"""
    u = torch.tensor([[0.5, 0.25, 0.5, 0.75, 0.25]])
    for n in range(1, 6):   # perm = argsort(u) with ties by index = [1, 4, 0, 2, 3]; mask[i] = perm[i] < n
        assert M.train_mask(u, torch.tensor([float(n)])).int().tolist() == [[int(p < n) for p in (1, 4, 0, 2, 3)]]


def test_fixture_is_small_and_holds_arrays_only():
    g = M.fixture()
    assert all(g[k].dtype != object for k in g.files)
    golden = os.path.dirname(M.GOLDEN)
    assert os.path.getsize(M.GOLDEN) < max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != os.path.basename(M.GOLDEN))


def test_new_entries_are_bound_and_declared():
    header = open(_lib.HEADER_PATH).read()
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES, name
        assert f"int {name}(bevgen_ctx* ctx" in header, name
    assert _lib.ABI_VERSION == 10            # additions only: the version and the configuration struct stay
    import ctypes

    assert ctypes.sizeof(_lib.bevgen_cfg) == 4 * 52


def test_library_exports_the_new_entries():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name


def _tiny_maskgit(**kw):
    from bevgen_amd import presets
    from bevgen_amd.modules.stage2.muse_maskgit_pytorch import MaskGit, MaskGitTransformerMultiView

    cfg = presets.tiny_route_m(3, legacy=False)
    tr = MaskGitTransformerMultiView(num_tokens=cfg.vocab_size, dim=cfg.num_embed, seq_len=cfg.cam_latent_res, depth=cfg.num_layers, dim_head=64, heads=cfg.num_heads,
                                     ff_mult=4, cfg=cfg)
    return cfg, MaskGit(image_size=cfg.cam_latent_res, transformer=tr, self_token_critic=True, cond_drop_prob=0.1, **kw)


def test_forward_refusals_need_no_device():
    cfg, mg = _tiny_maskgit()
    mg.eval()
    ids = torch.zeros((3, cfg.num_cam_tokens), dtype=torch.int64)
    cond = torch.zeros((1, cfg.num_cond_tokens), dtype=torch.int64)
    batch = {"intrinsics_inv": torch.eye(3).expand(1, 3, 3, 3), "extrinsics_inv": torch.eye(4).expand(1, 3, 4, 4)}
    with pytest.raises(NotImplementedError, match="muse_net:375"):
        mg(ids, cond_images=cond, batch=batch, weights=torch.ones(3 * cfg.num_cam_tokens))
    with pytest.raises(AssertionError, match="cannot pass in both"):
        mg(ids, cond_images=cond, cond_token_ids=cond, batch=batch)
    for bad in (0, 5, cfg.vocab_size):
        with pytest.raises(ValueError, match="muse_net:669"):
            mg(ids, ignore_index=bad, cond_images=cond, batch=batch)
    mg.train()
    with pytest.raises(NotImplementedError, match="muse_net:310"):
        mg(ids, cond_images=cond, batch=batch)
    with pytest.raises(NotImplementedError, match="muse_net:310"):
        mg.eval().transformer.train()
        mg(ids, cond_images=cond, batch=batch, cond_drop_prob=0.3)
    _, mg2 = _tiny_maskgit(no_mask_token_prob=0.1)
    with pytest.raises(NotImplementedError, match="muse_net:671"):
        mg2.eval()(ids, cond_images=cond, batch=batch)
    # past the refusals the call needs the device: a CPU model says so instead of computing anything in torch
    with pytest.raises(RuntimeError, match="ROCm device|ROCm GPU"):
        mg.eval()(ids, cond_images=cond, batch=batch, noise=7)


def test_route_m_net2net_has_the_validation_surface():
    from bevgen_amd.modules.stage2.cond_transformer_multi_view_muse import Net2NetTransformer
    from bevgen_amd.modules.stage2.muse_maskgit_pytorch import MaskGit

    assert list(inspect.signature(Net2NetTransformer.get_xc).parameters) == ["self", "batch", "N"]
    assert list(inspect.signature(Net2NetTransformer.shared_step).parameters)[:4] == ["self", "batch", "batch_idx", "inference"]
    assert list(inspect.signature(Net2NetTransformer.validation_step).parameters) == ["self", "batch", "batch_idx"]
    assert list(inspect.signature(MaskGit.forward).parameters) == ["self", "images_or_ids", "ignore_index", "cond_images", "cond_token_ids", "cond_drop_prob",
                                                                    "train_only_generator", "sample_temperature", "batch", "weights", "noise"]
    model = Net2NetTransformer.__new__(Net2NetTransformer)
    torch.nn.Module.__init__(model)
    model.first_stage_key, model.cond_stage_key = "image", "segmentation"
    model.cfg = type("Cfg", (), {"num_cams": 3})()
    batch = {"image": torch.zeros(2, 3, 8, 8, 3), "segmentation": torch.zeros(2, 8, 8, 7)}
    x, c = model.get_xc(batch)
    assert x.shape == (6, 3, 8, 8) and c.shape == (2, 7, 8, 8)
    x, c = model.get_xc(batch, N=1)
    assert x.shape == (1, 3, 8, 8) and c.shape == (1, 7, 8, 8)
