"""The building blocks of LPIPS at shapes of their own, on an fp32 and on an f16x3 context: the 3x3 convolution with the ReLU epilogue (register-staged fp32 kernel /
LDS-DMA split-precision kernel) against float64, the 2x2 max-pool bit for bit (fp32 and the plane image), the tap distance inside its first-order bound
(tests/lpips_ref.py) and bit-identical from run to run.

Measured on an MI355X (pytest -s prints each case; experiments/r17.md): conv + ReLU at most 0.691 (fp32 kernel) / 0.314 (LDS-DMA kernel) of CONV_BOUND, the tap distance at
most 0.032 of its bound."""
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as LR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["fp32", "f16x3"])
def ctx(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bevgen_amd.runtime import Context

    c = Context(None, precision=request.param)
    yield c
    c.close()


# (n, H, W, Cin, Cout): odd sizes and one block; two images, whole rows of tiles; deep and narrow; padding only
CONV_CASES = [(1, 9, 13, 32, 64), (2, 16, 16, 64, 128), (1, 4, 6, 256, 512), (1, 1, 1, 512, 512)]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3x3_relu_against_float64(ctx, case):
    n, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn((n, H, W, Cin), generator=g)
    w = torch.randn((Cout, 3, 3, Cin), generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn((Cout,), generator=g) * 0.5           # outputs are zero-mean with a spread of ~1.4: about half stay negative
    ref = F.relu(F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    kernel = "auto" if ctx.precision == "fp32" else "dma"
    y = ctx.op_conv3x3(x.cuda(), w.cuda(), b.cuda(), kernel=kernel, act="relu").cpu()
    plain = ctx.op_conv3x3(x.cuda(), w.cuda(), b.cuda(), kernel=kernel).cpu()
    zero = (ref == 0).double().mean().item()
    err = (y.double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"conv+relu {case} {kernel}: {err / LR.CONV_BOUND:.3f} of {LR.CONV_BOUND:.1e}; {zero:.2f} of the outputs clipped")
    assert 0.3 < zero < 0.7 and bool((y >= 0).all())
    assert err <= LR.CONV_BOUND
    assert torch.equal(y, plain.clamp_min(0))             # the epilogue is the plain one followed by max(0, .): no other bit moves
    assert ctx.status() == 0


POOL_CASES = [(1, 9, 13, 64), (2, 16, 16, 128), (1, 2, 3, 512)]


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_maxpool2x2_bit_for_bit(ctx, case):
    n, H, W, C = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn((n, H, W, C), generator=g) * 3
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    assert want.shape == (n, H // 2, W // 2, C)
    y, planes = ctx.op_maxpool2x2(x.cuda(), planes=True)
    only = ctx.op_maxpool2x2(x.cuda())
    assert torch.equal(y.cpu().view(torch.int32), want.view(torch.int32)) and torch.equal(only, y)
    split, e = ctx.op_range_split(y.reshape(n, (H // 2) * (W // 2), C))
    assert e.item() == 0 and planes.shape == split.shape
    assert torch.equal(planes.view(torch.int16), split.view(torch.int16))
    # the planes hold the pooled tensor: hi + lo 2^-11 to fp32's last bit or two
    back = (planes[:, :, 0].float() + planes[:, :, 1].float() / 2048).reshape(want.shape).cpu()
    assert (back - want).abs().max().item() <= 2.0 ** -21 * want.abs().max().item()
    assert ctx.status() == 0


@pytest.mark.parametrize("pixels", LR.TAP_PIXEL_CASES)
@pytest.mark.parametrize("C", LR.TAP_CHANNEL_CASES)
def test_tap_distance_inside_its_bound_and_reproducible(ctx, C, pixels):
    fa, fb, w = LR.tap_case(C, pixels)
    d64, bound = LR.tap_bound(fa.transpose(1, 2), fb.transpose(1, 2), w)
    a, b, wd = fa.cuda(), fb.cuda(), w.cuda()
    got = ctx.op_lpips_tap(a, b, wd)
    again = ctx.op_lpips_tap(a, b, wd)
    frac = ((got.cpu() - d64).abs() / bound).max().item()
    print(f"tap C={C} pixels={pixels}: {frac:.3f} of the bound (k = {LR.TAP_K}), d = {d64.tolist()}")
    assert got.dtype == torch.float64 and torch.equal(got.view(torch.int64), again.view(torch.int64))
    assert frac <= 1.0
    assert torch.equal(ctx.op_lpips_tap(b, a, wd).view(torch.int64), got.view(torch.int64))        # (x - y)^2: the same roundings either way
    assert bool((ctx.op_lpips_tap(a, a.clone(), wd) == 0).all())
    if pixels > 2:
        # pixel 2 is all zero in both images: exactly 0; pixel 1 in fa alone: sum_c w_c fb^_c^2, inside the bound
        assert bool((ctx.op_lpips_tap(a[:, 2:3].contiguous(), b[:, 2:3].contiguous(), wd) == 0).all())
        one64, one_bound = LR.tap_bound(fa[:, 1:2].transpose(1, 2), fb[:, 1:2].transpose(1, 2), w)
        one = ctx.op_lpips_tap(a[:, 1:2].contiguous(), b[:, 1:2].contiguous(), wd).cpu()
        assert bool((one64 > 0).all()) and bool(((one - one64).abs() <= one_bound).all())
    assert ctx.status() == 0
