"""precision='f16x3r' on the VQGAN encoder (include/bevgen_hip.h bevgen_cfg.vq_range): vq_encode rescales the image in front of conv_in, the residual stream in front of
every nin_shortcut and downsample convolution and conv_out's output in front of quant_conv by a per-tensor power of two.  Recipes, fp64 reference and input builders:
tests/test_vq_encode_range_cpu.py.  Covered here:
  * the two recipes that 'f16x3' refuses encode to the fp64 ids on every row that is not a near-tie, with exactly the exponents the rule gives on the fp64 absmax;
  * where nothing leaves the range every exponent is 0 and the ids are those of 'f16x3' and of the golden;
  * exponents belong to a call (encode / decode / encode), and a second pass of 48 images repeats the first;
  * the image's own exponent (the fused layout change) on a scaled image;
  * one site on its own (op_conv_ranged) against fp64 at the bound of the unscaled convolution, its exponent, NaN / inf refused;
  * the drop-in VQModel.

Measured on an MI355X (experiments/r11.md): R1 exponents 0 0 0 0 2 0 0, R3 0 0 1 1 7 4 0; ids of 'f16x3r' and 'fp32' equal the fp64 ids on all 128 rows of either recipe
(124 / 125 of them compared); op_conv_ranged max |y - ref| / max |ref| at most 1.7e-7 (1x1), 4.3e-7 (3x3), 3.5e-7 (Downsample) over the four scales, bound 2e-6.
"""
import re

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import cases
from test_vq_encode_range_cpu import (CONV_C, CONV_HW, CONV_KINDS, CONV_N, CONV_SCALES, conv_case, conv_ref, recipe_ref, recipe_sd, recipe_x, want_exponent)
from test_vq_ref_cpu import CONV_BOUND, nchw, nhwc, rel

pytestmark = pytest.mark.gpu

N_SITES = 7      # tiny ddconfig: conv_in, three downsamples, two nin_shortcuts, quant_conv


def _t(a, dtype=None):
    t = torch.from_numpy(np.asarray(a))
    return t.to(dtype) if dtype is not None else t


def dev(t):
    return t.cuda().contiguous()


def raised_word(excinfo):
    """The device status word a BevgenError reports (csrc/context.cpp check_status)."""
    m = re.search(r"device status word (\d+)", str(excinfo.value))
    assert m, str(excinfo.value)
    return int(m.group(1))


def _ctx(v, sd, precision):
    from bevgen_amd.runtime import Context

    ctx = Context(None, vq_ddconfig=v["dd"], vq_n_embed=v["n_embed"], vq_embed_dim=v["embed_dim"], precision=precision)
    ctx.load_state_dict(sd, prefix="first_stage_model.")
    ctx.finalize()
    return ctx


_SD = {}


def _plain_sd(v):
    key = (v["seed"], v["dd"]["in_channels"])
    if key not in _SD:
        _SD[key] = cases.vq_state_dict(v["dd"], v["n_embed"], v["embed_dim"], v["seed"], with_encoder=True)
    return _SD[key]


@pytest.fixture(scope="module")
def r1_ctx():
    ctx = _ctx(cases.VQ_TINY_HEAVY, recipe_sd("R1"), "f16x3r")
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def split_ctx():
    from bevgen_amd.runtime import Context

    ctx = Context(None, precision="f16x3")
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------ the checkpoints 'f16x3' refuses
@pytest.mark.parametrize("name", ["R1", "R3"])
def test_recipe_encodes_in_f16x3r(name):
    v, ref, x = cases.VQ_TINY_HEAVY, recipe_ref(name), recipe_x()
    keep = ref["keep"]
    out = {}
    for precision in ("f16x3r", "fp32"):
        ctx = _ctx(v, recipe_sd(name), precision)
        out[precision] = ctx.vq_encode(x).cpu()
        assert ctx.status() == 0
        if precision == "f16x3r":
            exps = ctx.vq_range_exponents().tolist()
        else:
            assert len(ctx.vq_range_exponents()) == 0
        ctx.close()
    miss = {p: int((out[p] != ref["ids"])[keep].sum()) for p in out}
    print(f"{name}: exponents {exps}; ids differing from fp64 on the {int(keep.sum())} compared rows: {miss}; on all {keep.numel()} rows: "
          f"{ {p: int((out[p] != ref['ids']).sum()) for p in out} }")
    assert exps == ref["exponents"]
    assert miss["fp32"] == 0
    assert miss["f16x3r"] == 0
    assert max(exps) >= 1


def test_r1_is_still_refused_in_f16x3():
    from bevgen_amd import _lib

    ctx = _ctx(cases.VQ_TINY_HEAVY, recipe_sd("R1"), "f16x3")
    with pytest.raises(_lib.BevgenError) as ei:
        ctx.vq_encode(recipe_x())
    assert ei.value.code == _lib.ERR_NUMERIC and raised_word(ei) & _lib.STATUS_F16_RANGE
    assert len(ctx.vq_range_exponents()) == 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ e = 0: the ids of 'f16x3'
@pytest.mark.parametrize("case", ["img", "seg", "rect"])
def test_f16x3r_ids_equal_f16x3_where_nothing_overflows(case):
    v = cases.VQ_TINY_SEG if case == "seg" else cases.VQ_TINY
    if case == "rect":
        g = golden("vq_rect")
        x, want = _t(g["tiny_enc_x"]), _t(g["tiny_enc_ids"], torch.long)
    else:
        g = golden("vq_tiny")
        x, want = _t(g[f"enc_{case}_x"]), _t(g[f"enc_{case}_ids"], torch.long)
    a, b = _ctx(v, _plain_sd(v), "f16x3r"), _ctx(v, _plain_sd(v), "f16x3")
    ids_r, ids_x = a.vq_encode(x).cpu(), b.vq_encode(x).cpu()
    exps = a.vq_range_exponents()
    assert a.status() == 0 and b.status() == 0
    assert len(exps) == N_SITES and (exps == 0).all(), exps
    assert len(b.vq_range_exponents()) == 0                  # 'f16x3' has no sites
    assert torch.equal(ids_r, ids_x)
    assert torch.equal(ids_r, want), f"{(ids_r != want).sum().item()} of {want.numel()} ids differ from the golden"
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ exponents belong to a call
def test_exponents_follow_the_most_recent_call(r1_ctx):
    v, ref, x = cases.VQ_TINY_HEAVY, recipe_ref("R1"), recipe_x()
    ctx = r1_ctx
    ids_a = ctx.vq_encode(x).cpu()
    exp_a = ctx.vq_range_exponents().tolist()
    ctx.vq_decode(ids_a, denormalize=False)
    exp_d = ctx.vq_range_exponents().tolist()
    ids_b = ctx.vq_encode(x).cpu()
    exp_b = ctx.vq_range_exponents().tolist()
    assert ctx.status() == 0
    fresh = _ctx(v, recipe_sd("R1"), "f16x3r")
    dec_fresh = (fresh.vq_decode(ids_a, denormalize=False), fresh.vq_range_exponents().tolist())[1]
    ids_f = fresh.vq_encode(x).cpu()
    exp_f = fresh.vq_range_exponents().tolist()
    fresh.close()
    assert exp_a == ref["exponents"] == exp_b == exp_f
    assert len(exp_d) == 6 and exp_d == dec_fresh           # the decoder's sites: conv_in, two nin_shortcuts, three upsamples
    assert torch.equal(ids_a, ids_b) and torch.equal(ids_a, ids_f)


def test_two_passes_repeat_the_exponents(r1_ctx):
    ref = recipe_ref("R1")
    x = recipe_x()[:1].repeat(49, 1, 1, 1)                   # 48 + 1 images: two passes
    ids = r1_ctx.vq_encode(x).cpu()
    exps = r1_ctx.vq_range_exponents().tolist()
    assert r1_ctx.status() == 0
    assert len(exps) == 2 * N_SITES and exps[:N_SITES] == exps[N_SITES:]
    assert exps[:N_SITES] == [want_exponent(a) for a in _single_image_absmax()]
    assert (ids == ids[:1]).all()
    assert torch.equal(ids[0][ref["keep"][0]], ref["ids"][0][ref["keep"][0]])


def _single_image_absmax():
    """Site absmax of image 0 alone (GroupNorm and attention are per image: the same tensors as in the batch of two, but the maxima are per tensor)."""
    from test_vq_encode_range_cpu import BOUNDARY_CLEARANCE, encode_with_sites

    _, _, sites = encode_with_sites(recipe_sd("R1"), cases.VQ_TINY_HEAVY["dd"], recipe_x()[:1])
    absmax = [a for _, a in sites]
    for a in absmax:                                         # the exactness condition of the CPU file, for this input
        for j in range(12):
            assert abs(a - 32768.0 * 2.0 ** j) > BOUNDARY_CLEARANCE * 32768.0 * 2.0 ** j, a
    return absmax


@pytest.mark.parametrize("scale", [8192.0, 1e5, 2.0 ** 40])
def test_image_exponent_from_the_layout_change(scale):
    """conv_in's operand is the caller's image itself: its exponent is the rule on the image's own absmax, exactly (no arithmetic in front of it)."""
    v = cases.VQ_TINY
    x = _t(golden("vq_tiny")["enc_img_x"])[:2] * scale
    ctx = _ctx(v, _plain_sd(v), "f16x3r")
    ctx.vq_encode(x)
    exps = ctx.vq_range_exponents().tolist()
    assert ctx.status() == 0
    ctx.close()
    assert len(exps) == N_SITES and exps[0] == want_exponent(x.double().abs().max().item()), exps


# ------------------------------------------------------------------------------------------------ one site on its own
@pytest.mark.parametrize("absmax", CONV_SCALES)
@pytest.mark.parametrize("kind", CONV_KINDS)
def test_op_conv_ranged(split_ctx, kind, absmax):
    worst = 0.0
    for n in CONV_N:
        for H, W in CONV_HW:
            for Cin in CONV_C:
                for Cout in CONV_C:
                    x, w, b = conv_case(kind, n, H, W, Cin, Cout, absmax)
                    ref = conv_ref(kind, x, w, b)
                    y, e = split_ctx.op_conv_ranged(dev(nhwc(x)), dev(w), dev(b), kind)
                    assert split_ctx.status() == 0
                    assert int(e.item()) == want_exponent(x.double().abs().max().item())
                    err = rel(nchw(y.cpu()), ref)
                    worst = max(worst, err)
                    assert err <= CONV_BOUND, (kind, n, H, W, Cin, Cout, absmax, err)
                    if kind == 2 and int(e.item()) == 0:     # exponent 0 writes the bits of the convolution with its bias in the epilogue
                        assert torch.equal(y, split_ctx.op_conv3x3_down(dev(nhwc(x)), dev(w), dev(b)))
    print(f"op_conv_ranged kind {kind} absmax {absmax:g}: max rel err {worst:.3e} (bound {CONV_BOUND:g})")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind", CONV_KINDS)
def test_op_conv_ranged_refuses_non_finite_values(split_ctx, kind, bad):
    from bevgen_amd import _lib

    x, w, b = conv_case(kind, 2, 6, 8, 32, 64, 4e4)
    x[1, 5, 3, 2] = bad
    with pytest.raises(_lib.BevgenError) as ei:
        split_ctx.op_conv_ranged(dev(nhwc(x)), dev(w), dev(b), kind)
    assert ei.value.code == _lib.ERR_NUMERIC and raised_word(ei) & _lib.STATUS_F16_RANGE
    assert split_ctx.status() == 0                           # reported once, then cleared
    x, w, b = conv_case(kind, 1, 2, 2, 32, 32, 1.0)
    y, e = split_ctx.op_conv_ranged(dev(nhwc(x)), dev(w), dev(b), kind)
    assert int(e.item()) == 0 and rel(nchw(y.cpu()), conv_ref(kind, x, w, b)) <= CONV_BOUND


def test_op_conv_ranged_needs_a_split_precision_context(gpu_ctx):
    from bevgen_amd import _lib

    x, w, b = conv_case(0, 1, 2, 2, 32, 32, 1.0)
    with pytest.raises(_lib.BevgenError, match="split-precision") as ei:
        gpu_ctx.op_conv_ranged(dev(nhwc(x)), dev(w), dev(b), 0)
    assert ei.value.code == -1                               # BEVGEN_ERR_INVALID


# ------------------------------------------------------------------------------------------------ the drop-in module
def test_vqmodel_encode_under_f16x3r(r1_ctx):
    from bevgen_amd.modules.stage1.vqgan import VQModel

    v = cases.VQ_TINY_HEAVY
    x = recipe_x()
    want = r1_ctx.vq_encode(x).cpu()
    m = VQModel(ddconfig=v["dd"], n_embed=v["n_embed"], embed_dim=v["embed_dim"], precision="f16x3r").cuda()
    missing, unexpected = m.load_state_dict(recipe_sd("R1"), strict=False)
    assert not unexpected and not [k for k in missing if k.startswith(("encoder.", "quant_conv.", "quantize."))], (missing, unexpected)
    ids = m.encode(x.cuda())[2][2]
    assert m.context().vq_range_exponents().tolist() == recipe_ref("R1")["exponents"]
    assert torch.equal(ids.cpu().reshape(want.shape), want)
