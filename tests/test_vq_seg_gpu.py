"""Stage-1 BEV segmentation model on the GPU (7 -> 7 channels, cases.VQ_TINY_SEG): Context.vq_decode with out_ch = 7 (fused tail and, in a child process with
BEVGEN_VQ_TAIL=0, the three-kernel tail), VQSegmentationModel.forward / validation_step / log_images / test_step with BCELossWithQuant, in fp32, f16x3 and f16x3r, against
the fp64 restatement of tests/test_vq_seg_cpu.py (cases sq, rect; the conditions the comparisons rest on are asserted there and, for the ids the GPU chose, again here).

Compared: logits within PIXEL_BOUND = 1e-3 (the project's pixel bound) of the restated fp64 decoder on the ids the GPU returned; bce within max |logit - logit64| of the
fp64 value (|dl/dx| <= 1); total bit for bit the loss op applied to the model's own xrec and emb_loss; `reconstructions` within colorize_bound() of the fp64 image at
every location none of whose 7 logits is inside the margin, the locations left out that way being at most MAX_INSIDE = 1 % of all (asserted); `inputs` within colorize_bound() everywhere.

Measured on an MI355X (worst over sq and rect; `pytest -s` prints them):
    mode     logits (bound 1e-3)   |bce - bce64| / max |dlogit|   reconstructions / bound   inputs / bound
    fp32     9.3e-6                0.003                          0.030                     0.033
    f16x3    5.4e-6                0.006                          0.030                     0.033
    f16x3r   5.4e-6                0.006                          0.030                     0.033
Three-kernel tail (child process): fp32 9.5e-6, f16x3 and f16x3r 5.7e-6.  Locations left out of the comparison of `reconstructions`: 79 of 8192 = 0.96 % (sq), 9 of 960 =
0.94 % (rect) in every mode (the GPU's ids are the fp64 ids; logits inside the margin 0.138 % / 0.134 %); the extremes are attained at 108 / 69 and 18 / 12 compared
locations.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_vq_seg_cpu import (CASES, MAX_INSIDE, bce64, case_x, colorize_bound, decode64, encode64, extremes_cannot_be_passed, inside_share, lat_of, left_out_share, margin_conditions, rgb64, seg_model, seg_sd)   # (first: its conftest import puts the repository root on sys.path, also in the child process below)
from oracle import cases

pytestmark = pytest.mark.gpu

MODES = ("fp32", "f16x3", "f16x3r")
PIXEL_BOUND = 1e-3


def _ctx(precision):
    from bevgen_amd.runtime import Context

    v = cases.VQ_TINY_SEG
    ctx = Context(None, vq_ddconfig=v["dd"], vq_n_embed=v["n_embed"], vq_embed_dim=v["embed_dim"], precision=precision)
    ctx.load_state_dict({k: t for k, t in seg_sd().items() if k != "colorize"}, prefix="first_stage_model.")
    ctx.finalize()
    return ctx


def decode_errors(ctx):
    """{case: max |vq_decode - fp64 restatement|} on the fp64 ids of the cases, with the shape and status checks of every decode"""
    out = {}
    for name in CASES:
        x, ids = case_x(name), encode64(name)["ids"]
        px = ctx.vq_decode(ids, denormalize=False, latent_hw=lat_of(x))
        assert tuple(px.shape) == tuple(x.shape) and px.dtype == torch.float32 and ctx.status() == 0
        again = ctx.vq_decode(ids, denormalize=False, latent_hw=lat_of(x))
        assert torch.equal(px.view(torch.int32), again.view(torch.int32))
        out[name] = (px.cpu().double() - decode64(ids, lat_of(x))).abs().max().item()
    return out


# ------------------------------------------------------------------------------------------------ Context.vq_decode, out_ch = 7
@pytest.mark.parametrize("precision", MODES)
def test_vq_decode_seven_channels(precision):
    ctx = _ctx(precision)
    errs = decode_errors(ctx)
    print(f"vq_decode out_ch=7 {precision} (fused tail): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {PIXEL_BOUND:g})")
    assert all(e < PIXEL_BOUND for e in errs.values())
    with pytest.raises(Exception, match="3 output channels"):
        ctx.vq_decode(encode64("rect")["ids"], denormalize=True, latent_hw=(3, 5))
    ctx.close()


def test_vq_decode_seven_channels_three_kernel_tail():
    """BEVGEN_VQ_TAIL is read once per process: a child process decodes with the three-kernel tail (its pixel staging holds out_ch = 7 floats per pixel)"""
    env = dict(os.environ, BEVGEN_VQ_TAIL="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    errs = json.loads(r.stdout.strip().splitlines()[-1])
    print("vq_decode out_ch=7 (three-kernel tail): " + ", ".join(f"{p} {k} {v:.2e}" for p, d in errs.items() for k, v in d.items()) + f" (bound {PIXEL_BOUND:g})")
    assert set(errs) == set(MODES) and all(e < PIXEL_BOUND for d in errs.values() for e in d.values())


# ------------------------------------------------------------------------------------------------ the drop-in model
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", CASES)
def test_model_forward_validation_step_log_images(name, precision):
    m = seg_model(precision=precision).cuda()
    x = case_x(name)
    colorize = seg_sd()["colorize"]
    batch = {"segmentation": x.permute(0, 2, 3, 1).contiguous()}                          # channel-last, as get_input takes it
    xd = x.cuda()
    xrec, qloss = m(xd, batch)
    ids = m.encode_ids(xd).cpu()
    l64 = decode64(ids, lat_of(x))
    assert xrec.shape == x.shape and qloss.dim() == 0 and qloss.is_cuda
    e_logit = (xrec.cpu().double() - l64).abs().max().item()
    # the loss: validation_step without and with the images
    ret1 = m.validation_step(batch, 1)
    ret10 = m.validation_step(batch, 10)
    assert set(ret1) == {"loss"} and set(ret10) == {"loss", "inputs", "reconstructions"}
    bce, total = m.context().bce_logits(xrec, xd, qloss, 1.0)
    assert ret1["loss"].dim() == 0 and ret1["loss"].is_cuda
    assert torch.equal(ret1["loss"].view(torch.int32), total.view(torch.int32)) and torch.equal(ret10["loss"].view(torch.int32), total.view(torch.int32))
    assert np.float32(total.item()) == np.float32(np.float32(bce.item()) + np.float32(np.float32(1.0) * np.float32(qloss.item())))
    want_bce = float(bce64(l64, x))
    e_bce = abs(float(bce) - want_bce)
    # the coloured images
    out = m.log_images(batch)
    assert set(out) == {"inputs", "reconstructions"} and all(torch.equal(out[k].view(torch.int32), ret10[k].view(torch.int32)) for k in out)
    assert all(torch.equal(v.view(torch.int32), out[k].view(torch.int32)) for k, v in m.test_step(batch, 0).items())
    rec, inp = out["reconstructions"].cpu().double(), out["inputs"].cpu().double()
    assert rec.shape == inp.shape == (x.shape[0], 3, x.shape[2], x.shape[3])
    inside, n_min, n_max = margin_conditions(l64, colorize)
    share = left_out_share(l64)
    d_rec = (rec - rgb64(l64, colorize, True)).abs()
    e_rec = d_rec[~inside[:, None].expand_as(d_rec)].max().item() / colorize_bound(l64, colorize, True)
    e_inp = (inp - rgb64(x, colorize, False)).abs().max().item() / colorize_bound(x, colorize, False)
    print(f"{precision} {name}: logits {e_logit:.2e} (bound {PIXEL_BOUND:g}); bce {float(bce):.8g} vs {want_bce:.8g}: {e_bce:.2e} = {e_bce / e_logit:.3f} of max |dlogit|; "
          f"reconstructions {e_rec:.3f}, inputs {e_inp:.3f} of the colorize bound; {int(inside.sum())} of {inside.numel()} locations left out = {100 * share:.2f} % (cap {100 * MAX_INSIDE:g} %), "
          f"logits inside the margin {100 * inside_share(l64):.3f} %; extremes attained at {n_min} / {n_max} compared locations")
    assert e_logit <= PIXEL_BOUND
    assert e_bce <= e_logit
    assert share <= MAX_INSIDE and n_min >= 1 and n_max >= 1 and extremes_cannot_be_passed(l64, colorize)
    assert e_rec <= 1 and e_inp <= 1
    assert rec.min() == 0 and rec.max() == 1 and inp.min() == 0 and inp.max() == 1
    assert m.context().status() == 0
    m.invalidate()


def test_three_channel_segmentation_model_logs_raw_tensors():
    """3 or fewer channels: log_images returns x and xrec as they are - no denormalisation with the camera statistics, no clamp"""
    from bevgen_amd.modules.stage1.vqgan import VQSegmentationModel

    v = cases.VQ_TINY
    torch.manual_seed(5)
    m = VQSegmentationModel(n_labels=3, ddconfig=v["dd"], n_embed=v["n_embed"], embed_dim=v["embed_dim"], image_key="segmentation").cuda()
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(6))
    out = m.log_images({"segmentation": x})
    xd = x.permute(0, 3, 1, 2).contiguous().cuda()
    xrec, _ = m(xd, None)
    assert torch.equal(out["inputs"], xd) and torch.equal(out["reconstructions"].view(torch.int32), xrec.view(torch.int32))
    assert out["inputs"].min() < 0 and out["inputs"].max() > 1
    m.invalidate()


def test_standalone_loss_opens_its_own_context():
    from bevgen_amd.modules.losses.segmentation import BCELoss

    x = case_x("rect")
    logits = decode64(encode64("rect")["ids"], lat_of(x)).float()
    loss, logs = BCELoss()(logits.cuda(), x.cuda())
    assert logs == {} and loss.is_cuda and loss.dim() == 0
    assert abs(float(loss) - float(bce64(logits, x))) <= 1e-6


if __name__ == "__main__":   # the child of test_vq_decode_seven_channels_three_kernel_tail
    assert os.environ.get("BEVGEN_VQ_TAIL") == "0"
    res = {}
    for mode in MODES:
        c = _ctx(mode)
        res[mode] = decode_errors(c)
        c.close()
    print(json.dumps(res))
