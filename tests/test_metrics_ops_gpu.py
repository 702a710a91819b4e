"""Operator-level parity of the image-metric kernels (bevgen_amd/csrc/metrics.hip): bevgen_op_ssim and bevgen_op_image_sqerr against the float64 restatement of
tests/metrics_ref.py.  Cases, references and bounds are that file's; every bound comes from the reference arithmetic's own fp32 error or the number format.

ssim: shapes (1,1,11,11), (2,3,12,75), (2,3,24,40), (1,3,33,65), (2,3,64,64) x inputs smooth + noise 0.05, uniform noise, the bright-flat pair (0.97 + 0.02 smooth, noise
1e-3), a pair quantised to k / 255 as fp32 and as uint8; one case with kernel_size 7, sigma 1.0, and one with kernel_size 33 (the 16-row tile).  Map maximum and per-image
mean against float64 within max(4 e_naive32, floor), the bright-flat pair also within max(8 e_centred32, floor); floors 2^-20 (map) and 2^-22 (mean).
image_sqerr: counts per image 1, 63, 64, 65, 257, 3 x 64 x 64; fp32 within 3 x 2^-24 relative, uint8 the integer sum bit for bit; min / max equal torch's and are merged
into the buffer that comes in.
Both: two calls give the same bits, an image in a batch of 2 gives the bits it gives alone, the fp32 and f16x3 contexts give the same bits, a NaN pixel makes its own
image NaN and raises no status bit, every refusal raises BEVGEN_ERR_INVALID.

Measured on an MI355X (`pytest -s` prints each case), worst fraction of the bound over the cases (experiments/r16.md has the table):
    ssim map    0.120 (bright-flat 2 x 3 x 12 x 75; every bright-flat case 0.096 .. 0.120 of max(8 e_centred32, 2^-20)); other inputs at most 0.085; k = 7: 0.122; k = 33: 0.094
    ssim mean   0.125 (bright-flat 1 x 1 x 11 x 11); other inputs at most 0.068; k = 7: 0.149 (smooth + noise 2 x 3 x 24 x 40); k = 33: 0.094
    image_sqerr 0.048 of 3 x 2^-24 (count 65); uint8 exact
The uint8 and fp32 forms of the quantised pair give the same bits (sums and map).
"""
import pytest
import torch

import metrics_ref as MR
from bevgen_amd import _lib

pytestmark = pytest.mark.gpu


def dev(t):
    return t.cuda().contiguous()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def gpu_ctx_split():
    from bevgen_amd.runtime import Context

    ctx = Context(None, precision="f16x3")
    yield ctx
    ctx.close()


def _check_ssim(ctx, kind, shape, k=11, sigma=1.5):
    c = MR.ssim_case(kind, shape, k, sigma)
    p, t = dev(c["p"]), dev(c["t"])
    sums, smap = ctx.op_ssim(p, t, kernel_size=k, sigma=sigma, return_map=True)
    n, C, H, W = shape
    assert smap.shape == c["map64"].shape == (n, C, H - k + 1, W - k + 1) and sums.shape == (n,) and sums.dtype == torch.float64 and sums.is_cuda
    means = sums.cpu() / (C * (H - k + 1) * (W - k + 1))
    e_map, e_mean = (smap.cpu().double() - c["map64"]).abs().max().item(), (means - c["mean64"]).abs().max().item()
    b_map, b_mean = MR.ssim_bounds(c, kind)
    print(f"ssim {kind} {shape} k={k}: map {e_map:.2e} = {e_map / b_map:.3f} of {b_map:.2e}, mean {e_mean:.2e} = {e_mean / b_mean:.3f} of {b_mean:.2e} "
          f"(e_naive32 {c['e_naive_map']:.1e} / {c['e_naive_mean']:.1e}, e_centred32 {c['e_centred_map']:.1e} / {c['e_centred_mean']:.1e})")
    # the sum the kernel reports is the sum of the map it reports (fp32 values added in double: exact to a few ulp of the double)
    assert (sums.cpu() - smap.cpu().double().sum((1, 2, 3))).abs().max().item() <= 1e-12 * smap[0].numel()
    assert e_map <= b_map and e_mean <= b_mean
    assert same_bits(sums, ctx.op_ssim(p, t, kernel_size=k, sigma=sigma))          # two calls, and with / without the map
    assert ctx.status() == 0
    return sums, smap


@pytest.mark.parametrize("kind", MR.SSIM_KINDS)
@pytest.mark.parametrize("shape", MR.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_against_float64(gpu_ctx, shape, kind):
    _check_ssim(gpu_ctx, kind, shape)


def test_ssim_kernel_size_7_sigma_1(gpu_ctx):
    _check_ssim(gpu_ctx, "smooth_noise", (2, 3, 24, 40), k=7, sigma=1.0)
    _check_ssim(gpu_ctx, "bright_flat", (1, 3, 33, 65), k=7, sigma=1.0)


def test_ssim_largest_kernel_size_takes_the_16_row_tile(gpu_ctx):
    _check_ssim(gpu_ctx, "smooth_noise", (1, 2, 50, 66), k=33, sigma=4.0)        # map 18 x 34: two tiles in both directions
    _check_ssim(gpu_ctx, "uniform", (1, 1, 33, 33), k=33, sigma=1.5)            # one window


def test_quantised_pair_as_uint8_and_as_fp32_agree(gpu_ctx):
    shape = (2, 3, 64, 64)
    f, u = MR.ssim_case("quant_f32", shape), MR.ssim_case("quant_u8", shape)
    sf, mf = gpu_ctx.op_ssim(dev(f["p"]), dev(f["t"]), return_map=True)
    su, mu = gpu_ctx.op_ssim(dev(u["p"]), dev(u["t"]), return_map=True)
    assert u["p"].dtype == torch.uint8 and torch.equal(MR.as_float(u["p"]), f["p"])
    assert same_bits(sf, su) and same_bits(mf, mu)                                 # v / 255 is one IEEE division in both forms


@pytest.mark.parametrize("kind", ["smooth_noise", "quant_u8"])
def test_ssim_image_of_a_batch_equals_the_image_alone_and_both_contexts_agree(gpu_ctx, gpu_ctx_split, kind):
    c = MR.ssim_case(kind, (2, 3, 24, 40))
    p, t = dev(c["p"]), dev(c["t"])
    both, mboth = gpu_ctx.op_ssim(p, t, return_map=True)
    for i in range(2):
        one, mone = gpu_ctx.op_ssim(p[i:i + 1].contiguous(), t[i:i + 1].contiguous(), return_map=True)
        assert same_bits(one, both[i:i + 1]) and same_bits(mone, mboth[i:i + 1])
    split, msplit = gpu_ctx_split.op_ssim(p, t, return_map=True)
    assert same_bits(split, both) and same_bits(msplit, mboth)
    assert gpu_ctx_split.status() == 0


def test_ssim_nan_pixel_stays_in_its_image(gpu_ctx):
    c = MR.ssim_case("smooth_noise", (2, 3, 64, 64))
    p, t = c["p"].clone(), c["t"]
    p[1, 2, 40, 7] = float("nan")
    sums, smap = gpu_ctx.op_ssim(dev(p), dev(t), return_map=True)
    clean = gpu_ctx.op_ssim(dev(c["p"]), dev(t))
    assert bool(sums[1].isnan()) and same_bits(sums[:1], clean[:1])
    bad = smap.cpu().isnan()
    assert bad[1, 2].any() and not bad[0].any() and not bad[1, :2].any()
    assert bad[1, 2, 30:41, 0:8].all() and not bad[1, 2, :29].any()                 # exactly the windows that hold the pixel
    assert gpu_ctx.status() == 0
    t2 = t.clone()
    t2[0, 0, 21, 21] = float("nan")                                                # the middle of the first tile's 42 x 42 halo: the pixel its shift is read from
    sums = gpu_ctx.op_ssim(dev(c["p"]), dev(t2))
    assert bool(sums[0].isnan()) and same_bits(sums[1:], clean[1:])
    assert gpu_ctx.status() == 0


# ================================================================================================ squared error
@pytest.mark.parametrize("count", MR.SQERR_COUNTS)
def test_image_sqerr_fp32(gpu_ctx, gpu_ctx_split, count):
    p, t = MR.sqerr_pair(count, torch.float32)
    want = MR.sse64(p, t)
    sse, minmax = gpu_ctx.op_image_sqerr(dev(p), dev(t))
    assert sse.dtype == torch.float64 and sse.shape == (2,) and minmax.dtype == torch.float32 and minmax.shape == (2,) and sse.is_cuda and minmax.is_cuda
    rel = ((sse.cpu() - want).abs() / want.clamp_min(1e-300)).max().item()
    print(f"image_sqerr fp32 count={count}: relative error {rel:.2e} = {rel / MR.SSE_REL:.3f} of {MR.SSE_REL:.2e}")
    assert rel <= MR.SSE_REL
    assert minmax.cpu().tolist() == [t.min().item(), t.max().item()]
    again, _ = gpu_ctx.op_image_sqerr(dev(p), dev(t))
    assert same_bits(sse, again)
    for i in range(2):
        one, mm = gpu_ctx.op_image_sqerr(dev(p[i:i + 1]), dev(t[i:i + 1]))
        assert same_bits(one, sse[i:i + 1]) and mm.cpu().tolist() == [t[i].min().item(), t[i].max().item()]
    split, mms = gpu_ctx_split.op_image_sqerr(dev(p), dev(t))
    assert same_bits(split, sse) and same_bits(mms, minmax)
    assert gpu_ctx.status() == 0 and gpu_ctx_split.status() == 0


@pytest.mark.parametrize("count", MR.SQERR_COUNTS)
def test_image_sqerr_uint8_is_the_integer_sum(gpu_ctx, count):
    p, t = MR.sqerr_pair(count, torch.uint8)
    want = ((p.long() - t.long()) ** 2).sum((1, 2, 3))
    sse, minmax = gpu_ctx.op_image_sqerr(dev(p), dev(t))
    assert same_bits(sse.cpu(), want.double())
    assert minmax.cpu().tolist() == [(t.min().float() / 255).item(), (t.max().float() / 255).item()]
    assert same_bits(sse, gpu_ctx.op_image_sqerr(dev(p), dev(t))[0])
    one, _ = gpu_ctx.op_image_sqerr(dev(p[1:]), dev(t[1:]))
    assert same_bits(one, sse[1:])


def test_image_sqerr_merges_into_the_incoming_minmax(gpu_ctx):
    p, t = MR.sqerr_pair(257, torch.float32)
    t = 0.25 + 0.5 * t                                                           # inside [0.25, 0.75]
    mm = torch.tensor([0.5, 2.0], device="cuda")                                 # a lower max and a higher min than the buffer holds must not overwrite it
    _, out = gpu_ctx.op_image_sqerr(dev(p), dev(t), mm)
    assert out.data_ptr() == mm.data_ptr() and mm.cpu().tolist() == [t.min().item(), 2.0]
    _, out = gpu_ctx.op_image_sqerr(dev(p), dev(t * 0 + 0.875), mm)              # a second call merges again
    assert mm.cpu().tolist() == [t.min().item(), 2.0]
    _, out = gpu_ctx.op_image_sqerr(dev(p), dev(t * 0 + 3.0), mm)
    assert mm.cpu().tolist() == [t.min().item(), 3.0]


def test_image_sqerr_nan_pixel_stays_in_its_image(gpu_ctx):
    p, t = MR.sqerr_pair(3 * 64 * 64, torch.float32)
    clean, _ = gpu_ctx.op_image_sqerr(dev(p), dev(t))
    q = p.clone()
    q[1, 1, 5, 60] = float("nan")
    sse, minmax = gpu_ctx.op_image_sqerr(dev(q), dev(t))
    assert bool(sse[1].isnan()) and same_bits(sse[:1], clean[:1])
    assert minmax.cpu().tolist() == [t.min().item(), t.max().item()]            # the extremes are the target's
    assert gpu_ctx.status() == 0


# ================================================================================================ refusals
def _refused(fn):
    with pytest.raises(_lib.BevgenError) as e:
        fn()
    assert e.value.code == -1, e.value          # BEVGEN_ERR_INVALID: raised by the argument checks, before any launch


def test_refusals(gpu_ctx):
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device="cuda")
    _refused(lambda: gpu_ctx.op_ssim(z(1, 1, 10, 16), z(1, 1, 10, 16)))                       # H < k
    _refused(lambda: gpu_ctx.op_ssim(z(1, 1, 16, 10), z(1, 1, 16, 10)))                       # W < k
    _refused(lambda: gpu_ctx.op_ssim(z(1, 1, 16, 16), z(1, 1, 16, 16), kernel_size=10))       # even k
    _refused(lambda: gpu_ctx.op_ssim(z(1, 1, 40, 40), z(1, 1, 40, 40), kernel_size=35))       # k > 33
    _refused(lambda: gpu_ctx.op_ssim(z(0, 3, 16, 16), z(0, 3, 16, 16)))                       # n C H W == 0
    _refused(lambda: gpu_ctx.op_image_sqerr(z(0, 3, 16, 16), z(0, 3, 16, 16)))
    _refused(lambda: gpu_ctx.op_image_sqerr(z(2, 3, 0, 16), z(2, 3, 0, 16)))
    for dt in (torch.float64, torch.int64, torch.float16):                                    # a dtype other than fp32 / uint8
        _refused(lambda: gpu_ctx.op_ssim(z(1, 1, 16, 16, dtype=dt), z(1, 1, 16, 16, dtype=dt)))
        _refused(lambda: gpu_ctx.op_image_sqerr(z(1, 1, 16, 16, dtype=dt), z(1, 1, 16, 16, dtype=dt)))
    with pytest.raises(ValueError):                                                           # preds and target differ: refused by the wrapper
        gpu_ctx.op_ssim(z(1, 1, 16, 16), z(1, 1, 16, 17))
    with pytest.raises(ValueError):
        gpu_ctx.op_image_sqerr(z(1, 1, 16, 16), z(1, 1, 16, 16, dtype=torch.uint8))
    assert gpu_ctx.status() == 0
    # the context still works
    c = MR.ssim_case("uniform", (1, 1, 11, 11))
    assert abs(gpu_ctx.op_ssim(dev(c["p"]), dev(c["t"])).cpu().item() - c["mean64"].item()) <= MR.ssim_bounds(c, "uniform")[1]
