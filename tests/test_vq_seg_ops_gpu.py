"""Operator-level parity of what the stage-1 BEV segmentation model adds (bevgen_amd/csrc/vq.hip vq_out_conv_kernel<7>, csrc/vqseg_kernels.hip): bevgen_op_vq_out_tail_ex,
bevgen_op_bce_logits and bevgen_op_seg_colorize against fp64, on the fp32 and the f16x3 context (the two new kernels are fp32 in both).

vq_out_tail_ex, cout = 7: fused and as three kernels against fp64 conv(swish(groupnorm(x))) at C = 32 and 64; shapes 2 x 24 x 40 (partial 16 x 16 tiles on both edges),
1 x 16 x 16 (exactly one tile), 2 x 1 x 1 (halo only).  Bound: TAIL_BOUND x max |ref| of tests/test_vq_ref_cpu.py, the bound of the 3-channel tail test.  cout = 3 through
the new export equals the old export bit for bit (raw, denorm, u8; fused and three kernels); cout = 5 takes the three-kernel path whatever `fused` says.

bce_logits: counts 1, 63, 64, 65, 257 x 7 x 3 and 2 x 7 x 64 x 64, binary and soft targets, logits that include 0, -0, +-80 and +-1e4.  Bound against fp64:
B = 2^-24 mean_i (3 |x_i| + 3) + 2^-24 |loss64| - one rounding each for x t, the subtraction and the final add on magnitudes at most |x| + 0.7, about 3 ulp for exp / log1p
on a value at most 0.7, and the store.  Two calls give the same bits; total = float32(bce + float32(w q)) exactly; a NaN logit gives a NaN loss.

seg_colorize: C = 7 and 3, shapes 2 x 24 x 40 and 1 x 1 x 5, threshold 0 and 1.  Against fp64 within colorize_bound() of tests/test_vq_seg_cpu.py
(8 C 2^-24 S / (max64 - min64) + 2^-23); output min exactly 0, max exactly 1; two calls give the same bits; with selector matrices as `colorize` the thresholded
bits themselves come out and equal torch.round(torch.sigmoid(x)) computed on the CPU (logits with |x| >= 1e-6 or exactly +-0); a batch whose extremes sit in
different images shows that the reduction is global.

Measured on an MI355X (worst over the cases; `pytest -s` prints each), as fractions of the bound:
    vq_out_tail cout = 7   fused 0.073 (fp32 and f16x3); three kernels 0.072 (fp32), 0.027 (f16x3); cout = 5: 0.048 (fp32), 0.022 (f16x3)
    bce_logits             0.204 (count 64, soft targets: the +-1e4 logits carry the sum); 0.026 at 2 x 7 x 64 x 64; the same in both contexts
    seg_colorize           0.079 (2 x 24 x 40, C = 3, plain); threshold cases at most 0.045
The halo-only case at C = 32 is a GroupNorm group of ONE value: it normalises to beta exactly (csrc/norm.hip groupnorm_finalize_kernel writes rstd = 0 for it; with
rstd = eps^-1/2 the three-kernel form measured 14.2 of the bound there, the fused kernel 0.004).  test_groupnorm_of_a_one_value_group_is_beta: C = 32 gives beta bit for
bit (1.3e-8 after the swish), C = 64 (two values per group) 5.1e-6 of max |ref| against the 1e-5 of test_groupnorm.
"""
import math

import numpy as np
import pytest
import torch

from test_vq_ref_cpu import TAIL_BOUND, TAIL_SHAPES, _gen, nhwc, tail_case, tail_ref
from test_vq_seg_cpu import colorize_bound, rgb64

pytestmark = pytest.mark.gpu


def dev(t):
    return None if t is None else t.cuda().contiguous()


@pytest.fixture(scope="module")
def gpu_ctx_split():
    from bevgen_amd.runtime import Context

    ctx = Context(None, precision="f16x3")
    yield ctx
    ctx.close()


@pytest.fixture(params=["fp32", "f16x3"])
def any_ctx(request, gpu_ctx, gpu_ctx_split):
    return gpu_ctx if request.param == "fp32" else gpu_ctx_split


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ================================================================================================ decoder tail with cout output channels
TAIL7_SHAPES = [(2, 24, 40), (1, 16, 16), (2, 1, 1)]     # n, H, W (two 1 x 1 images: torch's group_norm refuses a single value per channel)
_TAIL = {}


def tail_case_cout(n, H, W, C, cout):
    g = _gen(14, n, H, W, C, cout)
    return {"x": torch.randn(n, C, H, W, generator=g) * 2 + 0.7, "norm_w": 1 + 0.3 * torch.randn(C, generator=g), "norm_b": 0.3 * torch.randn(C, generator=g),
            "w": torch.randn(cout, C, 3, 3, generator=g) * (1.1 / math.sqrt(9 * C)), "b": 0.1 * torch.randn(cout, generator=g)}


def _tail(shape, C, cout):
    key = (shape, C, cout)
    if key not in _TAIL:
        p = tail_case_cout(*shape, C, cout)
        ref = tail_ref(p)
        _TAIL[key] = (p, ref, TAIL_BOUND * ref.abs().max().item())
    return _TAIL[key]


def _run(ctx, p, fused, cout, mode="raw", mean=None, std=None):
    return ctx.op_vq_out_tail(dev(nhwc(p["x"])), dev(p["norm_w"]), dev(p["norm_b"]), dev(p["w"]), dev(p["b"]), mode=mode, mean=mean, std=std, fused=fused, cout=cout).cpu()


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("shape", TAIL7_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vq_out_tail_seven_channels(any_ctx, shape, C):
    p, ref, bound = _tail(shape, C, 7)
    fused, three = _run(any_ctx, p, True, 7), _run(any_ctx, p, False, 7)
    e1, e2 = ((a.double() - ref).abs().max().item() for a in (fused, three))
    print(f"vq_out_tail cout=7 {any_ctx.precision} {shape} C={C}: fused {e1 / bound:.3f}, three kernels {e2 / bound:.3f} of the bound {bound:.2e}")
    assert fused.shape == three.shape == ref.shape == (shape[0], 7, shape[1], shape[2])
    assert e1 <= bound and e2 <= bound
    assert same_bits(fused, _run(any_ctx, p, True, 7))
    assert any_ctx.status() == 0


@pytest.mark.parametrize("mode", ["raw", "denorm", "u8"])
@pytest.mark.parametrize("fused", [True, False])
def test_three_channels_through_the_new_export_are_the_old_export(any_ctx, fused, mode):
    p = tail_case(*TAIL_SHAPES[2])
    args = (dev(nhwc(p["x"])), dev(p["norm_w"]), dev(p["norm_b"]), dev(p["w"]), dev(p["b"]))
    kw = dict(mode=mode, mean=dev(p["mean"]), std=dev(p["std"]), fused=fused)
    assert same_bits(any_ctx.op_vq_out_tail(*args, **kw).cpu(), any_ctx.op_vq_out_tail(*args, cout=3, **kw).cpu())


def test_five_channels_take_the_three_kernel_path_and_denormalise_is_refused(any_ctx):
    from bevgen_amd import _lib

    shape = TAIL7_SHAPES[0]
    p, ref, bound = _tail(shape, 32, 5)
    a, b = _run(any_ctx, p, True, 5), _run(any_ctx, p, False, 5)
    e = (a.double() - ref).abs().max().item()
    print(f"vq_out_tail cout=5 {any_ctx.precision} {shape}: {e / bound:.3f} of the bound {bound:.2e}")
    assert same_bits(a, b) and e <= bound                                           # `fused` changes nothing: there is no fused kernel for 5 channels
    p7, _, _ = _tail(shape, 32, 7)
    mean = std = torch.ones(7).cuda()
    with pytest.raises(_lib.BevgenError, match="3 output channels"):
        _run(any_ctx, p7, True, 7, mode="denorm", mean=mean, std=std)
    with pytest.raises(ValueError, match="cout = 7"):
        _run(any_ctx, p, True, 7)


@pytest.mark.parametrize("swish", [False, True])
def test_groupnorm_of_a_one_value_group_is_beta(gpu_ctx, swish):
    """32 channels at a 1 x 1 image: every group holds ONE value, x - mean = 0 and the output is beta (its swish) whatever x is; with two
    values per group (C = 64) nothing changed: the bound of test_groupnorm (tests/test_ops_gpu.py, 1e-5 of max |ref|)"""
    g = _gen(18, int(swish))
    for C in (32, 64):
        x, gamma, beta = 5 * torch.randn(2, C, 1, 1, generator=g) + 3, 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
        ref = torch.nn.functional.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-6)
        ref = ref * torch.sigmoid(ref) if swish else ref
        out = gpu_ctx.op_groupnorm(dev(nhwc(x)), dev(gamma), dev(beta), swish=swish).cpu().permute(0, 3, 1, 2)
        e = (out.double() - ref).abs().max().item()
        print(f"groupnorm 2 x 1 x 1 C={C} swish={swish}: {e:.2e}")
        if C == 32:
            exact = (beta.double() * torch.sigmoid(beta.double()) if swish else beta.double()).reshape(1, C, 1, 1).expand_as(ref)
            assert (ref - exact).abs().max() < 1e-9                                     # (torch's fp64 evaluation: beta up to its own rounding)
            ref = exact
            e = (out.double() - ref).abs().max().item()
            assert e <= 2.0 ** -23 * ref.abs().max().item()                             # beta, and with swish one exp and one division of it
            if not swish:
                assert torch.equal(out, beta.reshape(1, C, 1, 1).expand_as(out))
        else:
            assert e <= 1e-5 * ref.abs().max().item()


# ================================================================================================ binary cross entropy with logits
BCE_COUNTS = [1, 63, 64, 65, 257 * 7 * 3, 2 * 7 * 64 * 64]
BCE_SPECIALS = [0.0, -0.0, 80.0, -80.0, 1e4, -1e4]


def bce_case(count, soft):
    g = _gen(15, count, int(soft))
    x = 3 * torch.randn(count, generator=g)
    k = min(count, len(BCE_SPECIALS))
    x[:k] = torch.tensor(BCE_SPECIALS[:k])
    t = torch.rand(count, generator=g) if soft else (torch.rand(count, generator=g) < 0.3).float()
    return x, t


def bce_ref(x, t):
    x, t = x.double(), t.double()
    loss = (x.clamp_min(0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean().item()
    return loss, 2.0 ** -24 * (3 * x.abs() + 3).mean().item() + 2.0 ** -24 * abs(loss)


@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
@pytest.mark.parametrize("count", BCE_COUNTS)
def test_bce_logits(any_ctx, count, soft):
    x, t = bce_case(count, soft)
    want, B = bce_ref(x, t)
    q = torch.tensor([1.2345], device="cuda")
    w = 0.37
    out = any_ctx.op_bce_logits(dev(x), dev(t), q, w)
    again = any_ctx.op_bce_logits(dev(x), dev(t), q, w)
    bce, total = out.cpu().numpy()
    e = abs(float(bce) - want)
    print(f"bce_logits {any_ctx.precision} count={count} {'soft' if soft else 'binary'}: {float(bce):.8g} vs {want:.8g}: error {e:.2e} = {e / B:.3f} of B = {B:.2e}")
    assert e <= B
    assert same_bits(out, again)
    assert total == np.float32(bce + np.float32(np.float32(w) * np.float32(1.2345)))
    alone = any_ctx.op_bce_logits(dev(x), dev(t)).cpu()
    assert same_bits(alone[:1], out.cpu()[:1]) and bool(alone[1].isnan())           # without qloss: out[1] stays as allocated
    if count >= 6:
        assert set(BCE_SPECIALS) <= set(x.tolist()) and math.copysign(1, x[1].item()) == -1
    assert any_ctx.status() == 0


def test_bce_logits_propagates_a_nan(gpu_ctx):
    x, t = bce_case(65, True)
    x[40] = float("nan")
    out = gpu_ctx.op_bce_logits(dev(x), dev(t), torch.tensor([0.5], device="cuda"), 1.0).cpu()
    assert bool(out.isnan().all())
    x, t = bce_case(65, False)
    t[3] = float("nan")
    assert bool(gpu_ctx.op_bce_logits(dev(x), dev(t)).cpu()[0].isnan())


def test_context_bce_logits_returns_zero_dim_device_tensors(gpu_ctx):
    x, t = bce_case(2 * 7 * 64 * 64, False)
    x, t = x.reshape(2, 7, 64, 64), t.reshape(2, 7, 64, 64)
    q = torch.tensor(0.75)                                                           # (a CPU tensor: brought to the device)
    bce, total = gpu_ctx.bce_logits(x, t, q, 2.0)
    assert bce.dim() == 0 and total.dim() == 0 and bce.is_cuda and total.is_cuda
    assert np.float32(total.item()) == np.float32(np.float32(bce.item()) + np.float32(1.5))
    assert abs(bce.item() - bce_ref(x.reshape(-1), t.reshape(-1))[0]) <= bce_ref(x.reshape(-1), t.reshape(-1))[1]
    assert gpu_ctx.bce_logits(x, t)[1] is None
    with pytest.raises(ValueError, match="differ in shape"):
        gpu_ctx.op_bce_logits(dev(x), dev(t[:1]))


# ================================================================================================ to_rgb
RGB_SHAPES = [(2, 24, 40), (1, 1, 5)]


def rgb_case(n, H, W, C, threshold):
    g = _gen(16, n, H, W, C, int(threshold))
    x = 2 * torch.randn(n, C, H, W, generator=g)
    if threshold:
        x[x.abs() < 1e-6] = 0.0
        flat = x.view(-1)
        flat[:4] = torch.tensor([0.0, -0.0, 1e-6, -1e-6])                            # the step itself and the nearest values the contract covers
    return x, torch.randn(3, C, generator=g)


@pytest.mark.parametrize("threshold", [False, True], ids=["plain", "threshold"])
@pytest.mark.parametrize("C", [7, 3])
@pytest.mark.parametrize("shape", RGB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seg_colorize(any_ctx, shape, C, threshold):
    x, colorize = rgb_case(*shape, C, threshold)
    v = torch.round(torch.sigmoid(x)) if threshold else x                            # on the CPU, as the reference evaluates it
    want, bound = rgb64(v, colorize, False), colorize_bound(v, colorize, False)
    out = any_ctx.op_seg_colorize(dev(x), dev(colorize), threshold)
    again = any_ctx.op_seg_colorize(dev(x), dev(colorize), threshold)
    e = (out.cpu().double() - want).abs().max().item()
    print(f"seg_colorize {any_ctx.precision} {shape} C={C} threshold={threshold}: {e:.2e} = {e / bound:.3f} of the bound {bound:.2e}")
    assert out.shape == (shape[0], 3, shape[1], shape[2]) and e <= bound
    assert out.min().item() == 0.0 and out.max().item() == 1.0
    assert same_bits(out, again)
    assert any_ctx.status() == 0


@pytest.mark.parametrize("C", [7, 3])
def test_threshold_bits_are_round_sigmoid(gpu_ctx, C):
    """selector matrices as colorize: y_k = v_c for one channel c per k, min 0 and max 1, so the output IS the thresholded tensor"""
    x, _ = rgb_case(2, 24, 40, C, True)
    want = torch.round(torch.sigmoid(x))
    assert set(want.unique().tolist()) == {0.0, 1.0} and want.view(-1)[:4].tolist() == [0.0, 0.0, 1.0, 0.0]
    for c0 in range(0, C, 3):
        chans = [(c0 + k) % C for k in range(3)]
        sel = torch.zeros(3, C)
        for k, c in enumerate(chans):
            sel[k, c] = 1.0
        out = gpu_ctx.op_seg_colorize(dev(x), dev(sel), True).cpu()
        assert torch.equal(out, want[:, chans]), chans


def test_min_max_are_taken_over_the_whole_batch(gpu_ctx):
    g = _gen(17)
    x = torch.rand(2, 7, 24, 40, generator=g)
    x[1] += 2.0                                                                      # image 0 holds the minimum, image 1 the maximum
    colorize = torch.rand(3, 7, generator=g) + 0.1                                   # positive weights: the projection keeps the two images apart
    out = gpu_ctx.op_seg_colorize(dev(x), dev(colorize), False).cpu()
    want, bound = rgb64(x, colorize, False), colorize_bound(x, colorize, False)
    assert (out.double() - want).abs().max().item() <= bound
    assert out[0].min() == 0 and out[1].max() == 1 and out[0].max() < out[1].min()   # per-image extremes would put a 0 and a 1 into BOTH images
    rgb = gpu_ctx.seg_to_rgb(x, colorize.reshape(3, 7, 1, 1), threshold=False)
    assert same_bits(rgb.cpu(), out)
    with pytest.raises(ValueError, match="does not project"):
        gpu_ctx.op_seg_colorize(dev(x), dev(colorize[:, :5].contiguous()), False)
