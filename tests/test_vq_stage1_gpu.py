"""Stage-1 VQGAN on the GPU with the geometric embedding, the codebook loss and the reconstruction forward: Context.vq_encode_ex, VQModel(geometric_embedding=True)
and the Route M drop-in's 'rec' image, in fp32, f16x3 and f16x3r, against the fp64 restatement of tests/test_vq_stage1_cpu.py (cases sq, rect, many; the conditions
the comparisons rest on are asserted there).

Compared: ids equal the fp64 ids on the rows whose relative margin is at least MARGIN = 1e-4 (tests/test_vq_encode_range_cpu.py); per row
|row_err - d64[row, id]| <= MARGIN max_j |d64[row, j]| (the movement of a distance the id comparison already allows; d64[row, id] is the fp64 error of the id the GPU
chose, which is the fp64 row_err wherever the ids agree); |loss - loss64| <= (1 + beta) / D times the mean of those row bounds; the loss is bit for bit the fixed-order
sum of the rows the library wrote; pixels within 1e-3 (the project's pixel bound) of the restated decoder on the ids the GPU returned.

Measured on an MI355X (worst over the three cases; `pytest -s` prints them), as fractions of the bound:
    mode     row_err / bound   loss / bound
    fp32     0.004             < 0.001
    f16x3    0.002             < 0.001
    f16x3r   0.002             < 0.001
Not compared by the margin rule: 2 of 192 rows (sq), 0 of 30 (rect), 18 of 3136 (many).  Pixels: forward 1.0e-5 (fp32) / 6.7e-6 (f16x3, f16x3r), log_images 2.4e-6,
the Route M 'rec' image 1.6e-6, each against the bound 1e-3.
"""
import numpy as np
import pytest
import torch

from bevgen_amd import presets, synthetic, weights as W
from conftest import golden
from oracle import cases
from oracle import restate as R
from test_vq_encode_range_cpu import MARGIN, MAX_EXCLUDED, want_exponent
from test_vq_stage1_cpu import (BETA, CASES, case_inputs, decode_ref, encode_images, encode_ref, fixed_order_loss, geo_sd, plain_sd, plane_of, scaled_quant_conv_absmax,
                                scaled_sd)

pytestmark = pytest.mark.gpu

MODES = ("fp32", "f16x3", "f16x3r")
PIXEL_BOUND = 1e-3
SITES = 7                       # range-safe sites of the tiny encoder per pass (tests/test_vq_encode_range_cpu.py SITE_NAMES)


def _ctx(precision, sd):
    from bevgen_amd.runtime import Context

    v = cases.VQ_TINY
    ctx = Context(None, vq_ddconfig=v["dd"], vq_n_embed=v["n_embed"], vq_embed_dim=v["embed_dim"], precision=precision)
    ctx.load_state_dict(sd, prefix="first_stage_model.")
    ctx.finalize()
    return ctx


@pytest.fixture(scope="module", params=MODES)
def geo_ctx(request):
    ctx = _ctx(request.param, geo_sd())
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def plain_ctx():
    ctx = _ctx("fp32", plain_sd())
    yield ctx
    ctx.close()


def encode_case(ctx, name, rows=slice(None)):
    c = case_inputs(name)
    plane = plane_of(c["lat"], c["cam_res"])
    return ctx.vq_encode_ex(c["x"][rows], c["I_inv"][rows], c["E_inv"][rows], plane, beta=BETA)


def check_against_ref(tag, ids, row_err, loss, ref, D):
    """the three comparisons of the module docstring; returns (worst row_err error / bound, loss error / bound)"""
    ids, row_err = ids.cpu(), row_err.cpu().double()
    keep = ref["keep"]
    assert torch.equal(ids[keep], ref["ids"][keep]), f"{tag}: {(ids != ref['ids'])[keep].sum().item()} compared ids differ from fp64"
    d = ref["d"]
    own = d.gather(1, ids.reshape(-1, 1)).reshape(ids.shape)              # fp64 error of the id the GPU chose
    row_bound = (MARGIN * d.abs().amax(1)).reshape(ids.shape)
    e_row = ((row_err - own).abs() / row_bound).max().item()
    loss_bound = (1 + BETA) / D * row_bound.mean().item()
    e_loss = abs(float(loss) - float(ref["loss"])) / loss_bound
    print(f"{tag}: row_err error {e_row:.3f} of its bound, loss {float(loss):.8g} vs {float(ref['loss']):.8g}: {e_loss:.3f} of its bound {loss_bound:.2e}; "
          f"{(~keep).sum().item()} rows not compared")
    assert bool(row_err.isfinite().all()) and e_row <= 1 and e_loss <= 1
    return e_row, e_loss


@pytest.mark.parametrize("name", CASES)
def test_vq_encode_ex_against_the_restatement(geo_ctx, name):
    ref = encode_ref(name)
    assert 1 - ref["keep"].double().mean().item() <= MAX_EXCLUDED
    ids, row_err, loss = encode_case(geo_ctx, name)
    D = cases.VQ_TINY["embed_dim"]
    assert loss.dim() == 0 and loss.is_cuda and ids.shape == ref["ids"].shape == row_err.shape
    check_against_ref(f"{geo_ctx.precision} {name}", ids, row_err, loss, ref, D)
    # the loss: taken once over all rows of all passes, in the fixed order
    assert np.float32(loss.item()) == fixed_order_loss(row_err.cpu().numpy(), D)
    assert geo_ctx.status() == 0
    passes = -(-ref["ids"].shape[0] // 48)
    e = geo_ctx.vq_range_exponents().tolist()
    if geo_ctx.precision == "f16x3r":
        # 7 sites per pass, in the same order; quant_conv's exponent is chosen from the SUM h + embedding
        assert len(e) == SITES * passes
        assert e[SITES - 1::SITES] == [want_exponent(ref["h_absmax"])] * passes
    else:
        assert e == []
    # two calls give the same bits
    ids2, row2, loss2 = encode_case(geo_ctx, name)
    assert torch.equal(ids2, ids) and torch.equal(row2.view(torch.int32), row_err.view(torch.int32)) and torch.equal(loss2.view(torch.int32), loss.view(torch.int32))


def test_f16x3r_quant_conv_site_takes_a_nonzero_exponent_from_the_scaled_sum():
    """conv_out x 2^14: the operand of quant_conv (encoder output + embedding) passes 32768; the seventh site rescales it by the exponent of its fp64 absmax"""
    ctx = _ctx("f16x3r", scaled_sd())
    c = case_inputs("sq")
    ids, row_err, loss = ctx.vq_encode_ex(c["x"], c["I_inv"], c["E_inv"], plane_of(c["lat"], c["cam_res"]))
    want = want_exponent(scaled_quant_conv_absmax())
    e = ctx.vq_range_exponents().tolist()
    print("exponents", e, "want the last to be", want)
    assert len(e) == SITES and e[-1] == want >= 1
    assert bool(row_err.isfinite().all()) and bool(loss.isfinite()) and ctx.status() == 0
    ctx.close()


def test_last_image_of_the_second_pass_equals_itself_alone(geo_ctx):
    """49 images = a pass of 48 and a pass of one: the geometry, the ids and row_err of image 48 are offset by the pass's first image"""
    ids, row_err, _ = encode_case(geo_ctx, "many")
    ids1, row1, loss1 = encode_case(geo_ctx, "many", slice(48, 49))
    assert torch.equal(ids[48:], ids1) and torch.equal(row_err[48:].view(torch.int32), row1.view(torch.int32))
    assert not torch.equal(ids[48], ids[0])                                # (another geometry: tests/test_vq_stage1_cpu.py test_conditions)
    assert np.float32(loss1.item()) == fixed_order_loss(row1.cpu().numpy(), cases.VQ_TINY["embed_dim"])
    # without the loss: nothing else changes
    c = case_inputs("many")
    ids3, row3, none = geo_ctx.vq_encode_ex(c["x"], c["I_inv"], c["E_inv"], plane_of(c["lat"], c["cam_res"]), want_loss=False)
    assert none is None and torch.equal(ids3, ids) and torch.equal(row3.view(torch.int32), row_err.view(torch.int32))


def test_context_without_the_embedding_is_unchanged_and_mismatches_are_errors(plain_ctx, geo_ctx):
    from bevgen_amd import _lib

    c = case_inputs("sq")
    plane = plane_of(c["lat"], c["cam_res"])
    want = torch.from_numpy(golden("vq_tiny")["enc_img_ids"].astype(np.int64))
    ids, row_err, loss = plain_ctx.vq_encode_ex(c["x"])
    assert torch.equal(ids, plain_ctx.vq_encode(c["x"])) and torch.equal(ids.cpu(), want)
    ref = encode_ref("sq", embed=False)
    check_against_ref("fp32 sq without the embedding", ids, row_err, loss, ref, cases.VQ_TINY["embed_dim"])
    with pytest.raises(_lib.BevgenError, match="no geometric embedding"):
        plain_ctx.vq_encode_ex(c["x"], c["I_inv"], c["E_inv"], plane)
    with pytest.raises(_lib.BevgenError, match="needs I_inv"):
        geo_ctx.vq_encode_ex(c["x"])
    with pytest.raises(_lib.BevgenError, match="needs I_inv"):
        geo_ctx.vq_encode(c["x"])
    with pytest.raises(ValueError, match="go together"):
        geo_ctx.vq_encode_ex(c["x"], c["I_inv"], c["E_inv"])
    assert plain_ctx.status() == 0 and geo_ctx.status() == 0


def test_finalize_refuses_half_an_embedding():
    from bevgen_amd import _lib
    from bevgen_amd.runtime import Context

    v = cases.VQ_TINY
    for drop, match in (("cam_embed.weight", "come together"), (None, "z_channels")):
        sd = dict(geo_sd())
        if drop:
            del sd[drop]
        else:
            sd["img_embed.weight"] = sd["img_embed.weight"][:32].contiguous()
        ctx = Context(None, vq_ddconfig=v["dd"], vq_n_embed=v["n_embed"], vq_embed_dim=v["embed_dim"])
        ctx.load_state_dict(sd, prefix="first_stage_model.")
        with pytest.raises(_lib.BevgenError, match=match):
            ctx.finalize()
        ctx.close()


# ------------------------------------------------------------------------------------------------ the drop-in modules
def _vqmodel(name, precision):
    from bevgen_amd.modules.stage1.vqgan import VQModel

    v, c = cases.VQ_TINY, case_inputs(name)
    m = VQModel(ddconfig=v["dd"], n_embed=v["n_embed"], embed_dim=v["embed_dim"], cam_res=c["cam_res"], cam_latent_res=c["lat"], cam_emd_dim=v["dd"]["z_channels"],
                geometric_embedding=True, precision=precision)
    m.load_state_dict(geo_sd(), strict=True)
    return m.cuda(), c


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", ["sq", "rect"])
def test_vqmodel_encode_forward_log_images(name, precision):
    m, c = _vqmodel(name, precision)
    ref = encode_ref(name)
    n, (lh, lw), D = c["x"].shape[0], c["lat"], cases.VQ_TINY["embed_dim"]
    batch = {"intrinsics_inv": c["I_inv"][None], "extrinsics_inv": c["E_inv"][None]}            # [B = 1, cam = n, ., .]
    x = c["x"].cuda()
    quant, emb_loss, info = m.encode(x, batch)
    ids = info[2].reshape(n, -1)
    assert info[0] is None and info[1] is None and emb_loss.dim() == 0 and emb_loss.is_cuda
    assert torch.equal(ids.cpu()[ref["keep"]], ref["ids"][ref["keep"]])
    E = geo_sd()["quantize.embedding.weight"]
    assert torch.equal(quant.cpu(), E[ids.cpu().reshape(-1)].reshape(n, lh, lw, D).permute(0, 3, 1, 2))
    assert torch.equal(m.encode_ids(x, batch), ids)
    # already flattened geometry: the same call
    assert torch.equal(m.encode(x, {"intrinsics_inv": c["I_inv"].cuda(), "extrinsics_inv": c["E_inv"].cuda()})[2][2].reshape(n, -1), ids)
    dec, diff = m(x, batch)
    assert torch.equal(diff.view(torch.int32), emb_loss.view(torch.int32))
    e_dec = (dec.cpu() - decode_ref(ids.cpu(), c["lat"])).abs().max().item()
    out = m.log_images({"image": c["x"].movedim(1, -1)[None].contiguous(), **batch})                # [1, cam, H, W, 3]
    assert set(out) == {"inputs", "reconstructions"}
    rec, inp = out["reconstructions"].cpu(), out["inputs"].cpu()
    e_rec = (rec - decode_ref(ids.cpu(), c["lat"], denorm=True)).abs().max().item()
    print(f"{precision} {name}: forward {e_dec:.2e}, log_images {e_rec:.2e} (bound {PIXEL_BOUND:g})")
    assert e_dec < PIXEL_BOUND and e_rec < PIXEL_BOUND
    assert rec.shape == inp.shape == c["x"].shape and rec.min() >= 0 and rec.max() <= 1 and inp.min() >= 0 and inp.max() <= 1
    assert (inp - R.denormalize(c["x"])).abs().max() < 1e-6
    with pytest.raises(ValueError, match="intrinsics_inv"):
        m.encode(x)
    m.invalidate()


def test_route_m_log_images_with_a_geometric_first_stage():
    """muse_lm Net2NetTransformer.log_images: 'rec' = decode(encode_to_z(images, batch)) through a first stage with the embedding (the m_tiny setup of test_dropin_gpu.py)"""
    from bevgen_amd.modules.stage1.vqgan import VQModel
    from bevgen_amd.modules.stage2.cond_transformer_multi_view_muse import Net2NetTransformer
    from bevgen_amd.modules.stage2.muse_maskgit_pytorch import MaskGit, MaskGitTransformerMultiView

    cfg = presets.tiny_route_m(3, legacy=False, latent=(8, 8))
    dd = presets.VQ_DDCONFIG_TINY
    tr = MaskGitTransformerMultiView(num_tokens=cfg.vocab_size, dim=cfg.num_embed, seq_len=cfg.cam_latent_res, depth=cfg.num_layers, dim_head=64,
                                     heads=cfg.num_heads, ff_mult=4, cfg=cfg)
    mg = MaskGit(image_size=cfg.cam_latent_res, transformer=tr, self_token_critic=True, cond_drop_prob=0.1)
    vq = VQModel(ddconfig=dd, n_embed=64, embed_dim=64, cam_res=(64, 64), cam_latent_res=(8, 8), cam_emd_dim=64, geometric_embedding=True)
    model = Net2NetTransformer(mg, vq, None, cfg, sample_iterations=3)
    full = {("maskgit." + k): v for k, v in W.maskgit_state_dict(cfg, 1234).items()}
    full.update({("first_stage_model." + k): v for k, v in geo_sd().items()})
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and all(k.startswith("cond_stage") for k in missing)
    model = model.to("cuda")
    B = 2
    bt = synthetic.make_batch(cfg, B, seed=4)
    images = torch.randn(B, cfg.num_cams, 64, 64, 3, generator=torch.Generator().manual_seed(5))
    batch = {"cond_ids": bt["cond_ids"], "intrinsics_inv": bt["intrinsics_inv"], "extrinsics_inv": bt["extrinsics_inv"], "image": images}
    x = images.movedim(-1, -3).reshape(-1, 3, 64, 64)
    ref = encode_images(x, bt["intrinsics_inv"], bt["extrinsics_inv"], (64, 64))
    assert 1 - ref["keep"].double().mean().item() <= MAX_EXCLUDED
    _, z = model.encode_to_z(x.cuda(), {k: v.cuda() for k, v in batch.items()})
    z = z.cpu()
    assert torch.equal(z[ref["keep"]], ref["ids"][ref["keep"]])
    out = model.log_images(batch, noise="greedy")
    rec = out["rec"].cpu()
    want = decode_ref(z, (8, 8), denorm=True).reshape(rec.shape)
    err = (rec - want).abs().max().item()
    print(f"Route M 'rec' with a geometric first stage: {err:.2e} (bound {PIXEL_BOUND:g}); {(~ref['keep']).sum().item()} of {z.numel()} rows not compared")
    assert rec.shape == (B, cfg.num_cams, 3, 64, 64) and err < PIXEL_BOUND


def test_route_a_partial_decoding_and_shared_step_with_a_geometric_first_stage():
    """ar_lm Net2NetTransformer with a first stage that has the embedding: the fixed cameras of partial decoding take the tokens of encode_ids(images, batch), and
    shared_step scores the tokens of encode_to_z(images, batch) - both on the six-camera 32 x 40 -> 4 x 5 setup of test_dropin_gpu.py, ids against the restatement."""
    from bevgen_amd.modules.stage1.vqgan import VQModel
    from bevgen_amd.modules.stage2.cond_transformer_multi_view import Net2NetTransformer
    from bevgen_amd.modules.transformer.mingpt_sparse import GPT

    cfg = presets.route_a(6, num_layers=2, dim=128, heads=2, vocab=64, cam_res=(32, 40), cam_latent_res=(4, 5), bev_latent_res=(8, 8), block=16, window_len=8)
    dd = cases.VQ_TINY["dd"]
    vq = VQModel(ddconfig=dd, n_embed=64, embed_dim=64, cam_res=(32, 40), cam_latent_res=(4, 5), cam_emd_dim=64, geometric_embedding=True)
    model = Net2NetTransformer(GPT(cfg), vq, None)
    full = {("transformer." + k): v for k, v in W.gpt_state_dict(cfg, 1234).items()}
    full.update({("first_stage_model." + k): v for k, v in geo_sd().items()})
    missing, unexpected = model.load_state_dict(full, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    model = model.to("cuda")
    B, C, T = 2, cfg.num_cams, cfg.num_cam_tokens
    bt = synthetic.make_batch(cfg, B, seed=9)
    images = torch.randn(B, C, 32, 40, 3, generator=torch.Generator().manual_seed(6))
    batch = {"image": images, "cond_ids": bt["cond_ids"], "intrinsics_inv": bt["intrinsics_inv"], "extrinsics_inv": bt["extrinsics_inv"]}
    x = images.movedim(-1, -3).reshape(B * C, 3, 32, 40)
    ref = encode_images(x, bt["intrinsics_inv"], bt["extrinsics_inv"], (32, 40))
    assert 1 - ref["keep"].double().mean().item() <= MAX_EXCLUDED
    dev_batch = {k: v.cuda() for k, v in batch.items()}
    _, z = model.encode_to_z(x.cuda(), dev_batch)
    assert torch.equal(z.cpu()[ref["keep"]], ref["ids"][ref["keep"]])
    plain = encode_images(x, bt["intrinsics_inv"], bt["extrinsics_inv"], (32, 40), embed=False)
    assert (plain["ids"] != ref["ids"]).double().mean().item() >= 0.10          # (the check cannot pass without the embedding)
    fixed = [3, 0, 2]
    out = model.sample(None, dev_batch["cond_ids"], dev_batch, sample=False, partial_decoding_idx=fixed)
    assert torch.equal(out[:, fixed], z.reshape(B, C, T)[:, fixed])
    # shared_step encodes the images with the batch's geometry: the same loss, bit for bit, as with those tokens handed in
    loss = model.shared_step(batch, 0)
    loss_z = model.shared_step({**batch, "z_ids": z.reshape(B, C, T)}, 0)
    assert loss.dim() == 0 and bool(loss.isfinite()) and torch.equal(loss.view(torch.int32), loss_z.view(torch.int32))
