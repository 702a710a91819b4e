"""Input builders and fp64 references of the stage-1 VQGAN building blocks that tests/test_vq_ops_gpu.py runs through their bevgen_op_* entries, checked here without a GPU:
every reference (plain torch in float64, restating the lines of the stage-1 model it names) against an independent fp32 formulation, and every "left out" cap of the GPU
tests on the seeds they use, from the references alone."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import restate as R

EPS24 = 2.0 ** -24

# ------------------------------------------------------------------------------------------------ shapes (the GPU file imports them)
DOWN_SHAPES = [(1, 2, 2, 32, 32), (3, 4, 6, 32, 96), (2, 16, 16, 64, 128), (1, 14, 26, 128, 64)]   # n, H, W, Cin, Cout
ATTN_SHAPES = [(1, 4, 4, 32), (3, 8, 8, 128), (1, 14, 25, 128), (2, 2, 17, 64)]                     # n, h, w, C
TAIL_SHAPES = [(1, 5, 7, 32), (2, 16, 16, 128), (1, 17, 33, 64)]                                    # n, H, W, C
QUANT_ROWS, QUANT_NE, QUANT_D = [1, 5, 37], [1, 63, 64, 65, 1000, 1024], [32, 256]
GN_EPI_SHAPES = [(1, 16, 16, 128, 128), (2, 16, 32, 32, 256)]                                        # n, H, W, Cin, Cout
GN_EPI_R = (0.0, 3.0, 30.0)                     # per-group mean / std of the convolution output, cycling over the 32 groups
GN_EPI_LADDER = (0.0, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0, 20.0, 24.0, 30.0, 40.0, 60.0, 100.0, 200.0)   # measurement only: where the path leaves the 1e-5 of test_groupnorm
GN_EPI_K = 8                                    # roundings of an fp32 partial sum in the epilogue (see gn_epi_bounds)

CONV_BOUND = 2e-6                               # tests/test_ops_gpu.py test_conv3x3 (fp32 and f16x3)
GN_BOUND = 1e-5                                 # tests/test_ops_gpu.py test_groupnorm
ATTN_BOUND = 1e-5
TAIL_BOUND = 1.2e-5                             # GroupNorm + convolution
MAX_EXCLUDED = 0.02

TAIL_MEAN = (0.5, 0.45, 0.55)
TAIL_STD = (0.9, 0.95, 0.8)                     # all below 1: the denormalised error is below the raw one, which leaves room for the roundings of x std + mean and of 255 x


def _gen(*seed):
    g = torch.Generator()
    g.manual_seed(1000003 * len(seed) + sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)))
    return g


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def rel(a, b):
    """max |a - b| over max |b|, as tests/test_ops_gpu.py measures."""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


# ================================================================================================ downsample convolution
def down_case(n, H, W, Cin, Cout):
    g = _gen(1, n, H, W, Cin, Cout)
    x = torch.randn(n, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    return x, w, b


def down_ref(x, w, b):
    """Downsample.forward with_conv (stage1/model.py:68-72): pad = (0, 1, 0, 1); x = F.pad(x, pad, mode="constant", value=0); x = self.conv(x)  (3x3, stride 2, padding 0)."""
    return F.conv2d(F.pad(x.double(), (0, 1, 0, 1), mode="constant", value=0), w.double(), None if b is None else b.double(), stride=2)


def down_probe_case(which, n=2, H=6, W=8, Cin=32, Cout=32):
    """Asymmetric probes.  'last': x is zero except its last row and last column, the only non-zero tap is (2, 2).  That tap reads input (2 oy + 2, 2 ox + 2): even
    coordinates, or the implied bottom / right padding - never the last row or column (odd coordinates), so the output is exactly the bias.  A kernel that pads the top /
    left instead reads (2 oy + 1, 2 ox + 1) and meets the last row and column.  'first': x is zero except its first row and column, the only tap is (0, 0), which reads
    (2 oy, 2 ox): the first output row and column see them; under top / left padding nothing does."""
    g = _gen(2, H, W, 0 if which == "last" else 1)
    x = torch.zeros(n, Cin, H, W)
    w = torch.zeros(Cout, Cin, 3, 3)
    if which == "last":
        x[:, :, H - 1, :] = torch.randn(n, Cin, W, generator=g) + 2
        x[:, :, :, W - 1] = torch.randn(n, Cin, H, generator=g) + 2
        w[:, :, 2, 2] = torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin)
    else:
        x[:, :, 0, :] = torch.randn(n, Cin, W, generator=g) + 2
        x[:, :, :, 0] = torch.randn(n, Cin, H, generator=g) + 2
        w[:, :, 0, 0] = torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin)
    b = torch.randn(Cout, generator=g)
    return x, w, b


# ================================================================================================ AttnBlock
def attn_case(n, h, w, C):
    """q / k weights of standard deviation 2 / sqrt(C): the scores q.k C^-0.5 then have a standard deviation of about 4 (a spread of +-10 and more), the softmax rows are
    peaked, and a wrong scale or a missing max-subtraction shows.  The v bias differs along C."""
    g = _gen(3, n, h, w, C)
    p = {"x": torch.randn(n, C, h, w, generator=g) * 1.5 + 0.3,
         "norm_w": 1 + 0.2 * torch.randn(C, generator=g), "norm_b": 0.2 * torch.randn(C, generator=g)}
    for name, s in (("q", 2.0), ("k", 2.0), ("v", 1.0), ("p", 1.0)):
        p["w" + name] = torch.randn(C, C, generator=g) * (s / math.sqrt(C))
        p["b" + name] = 0.3 * torch.randn(C, generator=g)
    p["bv"] = torch.linspace(-2, 2, C) + 0.3 * torch.randn(C, generator=g)
    return p


def attn_ref(p, dtype=torch.float64, collect=None):
    """AttnBlock.forward (stage1/model.py:168-192), on NHWC rows:
        h_ = self.norm(x); q, k, v = self.q(h_), self.k(h_), self.v(h_)           GroupNorm(32, eps 1e-6), 1x1 convolutions
        w_ = torch.bmm(q, k) * int(c) ** (-0.5); w_ = softmax(w_, dim=2)         q [b, hw, c], k [b, c, hw]
        h_ = torch.bmm(v, w_.permute(0, 2, 1)); return x + self.proj_out(h_)"""
    x = p["x"].to(dtype)
    n, C, h, w = x.shape
    hn = F.group_norm(x, 32, p["norm_w"].to(dtype), p["norm_b"].to(dtype), 1e-6)
    rows = hn.permute(0, 2, 3, 1).reshape(n, h * w, C)
    q = rows @ p["wq"].to(dtype).t() + p["bq"].to(dtype)
    k = rows @ p["wk"].to(dtype).t() + p["bk"].to(dtype)
    v = rows @ p["wv"].to(dtype).t() + p["bv"].to(dtype)
    s = torch.einsum("bic,bjc->bij", q, k) * (int(C) ** (-0.5))
    if collect is not None:
        collect["scores"] = s
    o = torch.softmax(s, dim=2) @ v
    y = x.permute(0, 2, 3, 1).reshape(n, h * w, C) + o @ p["wp"].to(dtype).t() + p["bp"].to(dtype)
    return y.reshape(n, h, w, C).permute(0, 3, 1, 2)


def attn_state_dict(p):
    """The same parameters under the names oracle/restate.py reads."""
    sd = {"norm.weight": p["norm_w"], "norm.bias": p["norm_b"]}
    for name, full in (("q", "q"), ("k", "k"), ("v", "v"), ("p", "proj_out")):
        sd[full + ".weight"] = p["w" + name].reshape(*p["w" + name].shape, 1, 1)
        sd[full + ".bias"] = p["b" + name]
    return sd


# ================================================================================================ decoder tail
def tail_case(n, H, W, C):
    g = _gen(4, n, H, W, C)
    return {"x": torch.randn(n, C, H, W, generator=g) * 2 + 0.7,
            "norm_w": 1 + 0.3 * torch.randn(C, generator=g), "norm_b": 0.3 * torch.randn(C, generator=g),
            "w": torch.randn(3, C, 3, 3, generator=g) * (1.1 / math.sqrt(9 * C)), "b": 0.1 * torch.randn(3, generator=g),
            "mean": torch.tensor(TAIL_MEAN), "std": torch.tensor(TAIL_STD)}


def tail_ref(p, mode="raw", dtype=torch.float64):
    """Decoder.forward's end (stage1/model.py:532-536): h = self.norm_out(h); h = nonlinearity(h) (x * sigmoid(x)); h = self.conv_out(h), then for 'denorm' / 'u8'
    util.denormalize_tensor (bev_utils/util.py:97-118): clamp(x * std + mean, 0, 1) per channel, and for 'u8' 255 times that (NOT yet rounded: the caller rounds)."""
    h = F.group_norm(p["x"].to(dtype), 32, p["norm_w"].to(dtype), p["norm_b"].to(dtype), 1e-6)
    h = h * torch.sigmoid(h)
    y = F.conv2d(h, p["w"].to(dtype), p["b"].to(dtype), padding=1)
    if mode == "raw":
        return y
    y = torch.clamp(y * p["std"].to(dtype).reshape(1, 3, 1, 1) + p["mean"].to(dtype).reshape(1, 3, 1, 1), 0, 1)
    return y if mode == "denorm" else 255 * y


def tail_u8_decidable(ref255, float_bound):
    """Pixels whose rounding the float bound decides: 255 ref farther from every k + 1/2 than 255 x the bound."""
    frac = ref255 - torch.floor(ref255)
    return (frac - 0.5).abs() > 255 * float_bound


# ================================================================================================ quantizer
def quant_ref(z, cb):
    """VectorQuantizer2.forward (stage1/quantize.py:279-285): d = sum(z ** 2, dim=1, keepdim=True) + sum(embedding.weight ** 2, dim=1) - 2 * einsum('bd,dn->bn', z, e^T);
    min_encoding_indices = argmin(d, dim=1) - the lowest index among equal minima.  Returns (ids, d) in fp64."""
    z, cb = z.double(), cb.double()
    d = (z ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1) - 2 * torch.einsum("bd,dn->bn", z, cb.t())
    n_e = cb.shape[0]
    idx = torch.arange(n_e).expand_as(d)
    ids = torch.where(d == d.min(1, keepdim=True).values, idx, torch.full_like(idx, n_e)).min(1).values
    return ids, d


# pairs (first, duplicate) of codebook rows: the lower index in the lower lane; in the same lane (lane = index % 64) at two values of j; the lower index in the HIGHER lane
QUANT_DUPES = [(5, 42), (3, 67), (40, 70), (130, 962)]


def quant_exact_case(rows, n_e, D, variant=0):
    """Integer-valued z and codebook in [-8, 8]: products <= 64, sums <= 64 * 256 = 2^14, distances <= 2^16 - every fp32 product and sum is exact, so the ids must EQUAL the
    fp64 ones.  Duplicated codebook rows (QUANT_DUPES, those that fit n_e) are the exact nearest entry of some rows (z = that entry, distance 0): a tied minimum."""
    g = _gen(5, rows, n_e, D, variant)
    cb = torch.randint(-8, 9, (n_e, D), generator=g).float()
    z = torch.randint(-8, 9, (rows, D), generator=g).float()
    dup = [(a, b) for a, b in QUANT_DUPES if b < n_e]
    for a, b in dup:
        cb[b] = cb[a]
    for r in range(rows):
        if dup and r % 2 == 0:
            z[r] = cb[dup[(r // 2 + variant) % len(dup)][0]]
    return z, cb, dup


def quant_float_case(rows, n_e, D):
    g = _gen(6, rows, n_e, D)
    return torch.randn(rows, D, generator=g), torch.randn(n_e, D, generator=g)


def quant_decidable(z, cb):
    """Rows whose two smallest fp64 distances are at least 4 * 2^-24 * (|z|^2 + |e|^2 + 2 |z.e|) apart (the larger of the two candidates' magnitudes): the fp32 evaluation
    of (|z|^2 + |e|^2) - 2 z.e cannot order them differently.  One codebook entry: every row."""
    ids, d = quant_ref(z, cb)
    if cb.shape[0] == 1:
        return torch.ones(z.shape[0], dtype=torch.bool)
    z, cb = z.double(), cb.double()
    two = torch.topk(d, 2, dim=1, largest=False)
    mag = (z ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1)[two.indices] + 2 * torch.einsum("bd,bkd->bk", z, cb[two.indices]).abs()
    return (two.values[:, 1] - two.values[:, 0]) >= 4 * EPS24 * mag.max(1).values


def quant_nonfinite_case(rows, n_e, D):
    """Row 1 of z holds a NaN, row 3 holds 3e38 (|z|^2 overflows to inf): no finite distance in either."""
    z, cb = quant_float_case(rows, n_e, D)
    z = z.clone()
    z[1, D // 2] = float("nan")
    z[3, 0] = 3e38
    return z, cb, [1, 3]


# ================================================================================================ GroupNorm statistics of the convolution epilogue
def gn_epi_case(n, H, W, Cin, Cout, ladder=GN_EPI_R):
    """A convolution whose output has unit variance per channel, plus a bias that is constant inside a GroupNorm group: group g gets mean / std = ladder[g % len(ladder)]."""
    g = _gen(7, n, H, W, Cin, Cout, len(ladder))
    x = torch.randn(n, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    cpg = Cout // 32
    b = torch.tensor([ladder[(c // cpg) % len(ladder)] for c in range(Cout)], dtype=torch.float32) + 0.05 * torch.randn(Cout, generator=g)
    return x, w, b


def gn_stats_ref(y):
    """GroupNorm(32, eps = 1e-6) statistics of y [n, C, H, W] in its own dtype: mean, rstd = 1 / sqrt(biased variance + eps), E|y| and the ratio r = |mean| / std, each [n, 32]."""
    n, C = y.shape[:2]
    v = y.reshape(n, 32, -1)
    mean = v.mean(2)
    var = ((v - mean[..., None]) ** 2).mean(2)
    return mean, 1 / torch.sqrt(var + 1e-6), v.abs().mean(2), mean.abs() / torch.sqrt(var)


def gn_epi_bounds(y):
    """Derived bounds of the epilogue path against fp64 statistics of the fp64 convolution output y.
    A partial (sum, sum of squares) over 32 pixels x 4 channels is a balanced tree of depth k = 8 in fp32 (sum of squares: the product v1 v1, the fmaf onto it, the pair
    add, four DPP steps of row16_sum, one xor16 step; the plain sum has 7); everything after it is fp64.  So each partial carries a relative error of at most k 2^-24
    against the sum of the magnitudes it adds: |d S1| <= k u sum |y|, |d S2| <= k u sum y^2 (u = 2^-24).  With var = S2 / N - mean^2:
        |d var| <= k u E[y^2] + 2 |mean| k u E|y| <= 3 k u E[y^2] = 3 k u var (1 + r^2),   d rstd / rstd = d var / (2 var)   =>   1.5 k u (1 + r^2)
    plus 2^-23 for the two fp32 roundings of the result and its inputs' share, plus the convolution's own 2e-6.  |d mean| <= k u E|y| + 2e-6 absmax."""
    mean, rstd, eabs, r = gn_stats_ref(y.double())
    k = GN_EPI_K
    rstd_rel = 1.5 * k * EPS24 * (1 + r ** 2) + 2.0 ** -23 + CONV_BOUND
    mean_abs = k * EPS24 * eabs + CONV_BOUND * y.double().abs().max()
    return mean, rstd, r, rstd_rel, mean_abs


# ================================================================================================ the references against independent fp32 formulations
@pytest.mark.parametrize("shape", DOWN_SHAPES)
def test_down_ref_is_the_explicit_tap_sum(shape):
    x, w, b = down_case(*shape)
    n, Cin, H, W = x.shape
    xp = torch.zeros(n, Cin, H + 1, W + 1)
    xp[:, :, :H, :W] = x
    out = b.reshape(1, -1, 1, 1).expand(n, -1, H // 2, W // 2).clone()
    for kh in range(3):
        for kw in range(3):
            out += torch.einsum("nchw,oc->nohw", xp[:, :, kh:kh + H - 1:2, kw:kw + W - 1:2], w[:, :, kh, kw])
    ref = down_ref(x, w, b)
    assert ref.shape == (n, w.shape[0], H // 2, W // 2)
    assert rel(out, ref) < 1e-5


def test_down_probes_tell_bottom_right_from_top_left_padding():
    for which in ("last", "first"):
        x, w, b = down_probe_case(which)
        right = down_ref(x, w, b)
        wrong = F.conv2d(F.pad(x.double(), (1, 0, 1, 0)), w.double(), b.double(), stride=2)
        bias_only = b.double().reshape(1, -1, 1, 1).expand_as(right)
        if which == "last":
            assert torch.equal(right, bias_only) and not torch.equal(wrong, bias_only)
        else:
            assert torch.equal(wrong, bias_only)
            assert not torch.equal(right[:, :, 0, :], bias_only[:, :, 0, :]) and torch.equal(right[:, :, 1:, 1:], bias_only[:, :, 1:, 1:])


@pytest.mark.parametrize("shape", ATTN_SHAPES)
def test_attn_ref_matches_the_restated_block_and_is_peaked(shape):
    p = attn_case(*shape)
    col = {}
    ref = attn_ref(p, collect=col)
    other = R._attn_block(attn_state_dict(p), "", p["x"])
    assert rel(other, ref) < 2e-5
    s = col["scores"]
    assert s.abs().max() > 10 and (s.max(2).values - s.min(2).values).median() > 10     # a spread of +-10 and beyond
    assert torch.softmax(s, 2).max(2).values.median() > 0.2                             # peaked rows (uniform would be 1 / hw)
    assert p["bv"].std() > 1


@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_tail_ref_matches_the_restated_decoder_end_and_its_caps_hold(shape):
    p = tail_case(*shape)
    raw = tail_ref(p)
    h = R._gn_swish(p["x"], p["norm_w"], p["norm_b"])
    other = F.conv2d(h, p["w"], p["b"], padding=1)
    assert rel(other, raw) < 1e-5
    den = tail_ref(p, "denorm")
    mean = p["mean"].reshape(1, 3, 1, 1)
    std = p["std"].reshape(1, 3, 1, 1)
    assert rel(torch.clamp(other * std + mean, 0, 1), den) < 1e-5
    assert float(p["std"].max()) < 1
    # part of the image clamps at each end
    assert (den == 0).double().mean() > 0.03 and (den == 1).double().mean() > 0.03 and ((den > 0) & (den < 1)).double().mean() > 0.3
    # the share of pixels whose uint8 value the float bound does not decide
    bound = TAIL_BOUND * raw.abs().max().item()
    undecided = 1 - tail_u8_decidable(tail_ref(p, "u8"), bound).double().mean().item()
    assert undecided <= MAX_EXCLUDED, undecided


@pytest.mark.parametrize("D", QUANT_D)
@pytest.mark.parametrize("n_e", QUANT_NE)
@pytest.mark.parametrize("rows", QUANT_ROWS)
def test_quant_ref_and_margin_cap(rows, n_e, D):
    # exact cases: fp32 evaluates the same integers; the tie cases are ties, and the reference takes the lower index
    for variant in range(3):
        z, cb, dup = quant_exact_case(rows, n_e, D, variant)
        ids, d = quant_ref(z, cb)
        d32 = (z ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1) - 2 * z @ cb.t()
        assert torch.equal(d32.double(), d) and d.abs().max() < 2 ** 24
        assert torch.equal(ids, torch.argmin(d32, dim=1))
        for r in range(0, rows, 2):
            if dup:
                a, b = dup[(r // 2 + variant) % len(dup)]
                assert d[r, a] == 0 and d[r, b] == 0 and ids[r] <= a
    # float cases: the margin rule leaves out at most 2 % of the rows, and on the others fp32 torch agrees
    z, cb = quant_float_case(rows, n_e, D)
    keep = quant_decidable(z, cb)
    assert (~keep).double().mean().item() <= MAX_EXCLUDED
    ids, _ = quant_ref(z, cb)
    other = torch.cdist(z[None], cb[None])[0].argmin(1)
    assert torch.equal(other[keep], ids[keep])


@pytest.mark.parametrize("shape", GN_EPI_SHAPES)
def test_gn_epi_case_reaches_the_ratios_and_the_reference_agrees_with_group_norm(shape):
    x, w, b = gn_epi_case(*shape)
    y = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    mean, rstd, r, rstd_rel, mean_abs = gn_epi_bounds(y)
    for i, target in enumerate(GN_EPI_R):
        got = r[:, i::len(GN_EPI_R)]
        assert ((got - target).abs() <= 0.15 * target + 0.15).all(), (target, got)
    # the statistics are the ones F.group_norm applies
    gamma, beta = torch.ones(y.shape[1], dtype=torch.float64), torch.zeros(y.shape[1], dtype=torch.float64)
    n, C = y.shape[:2]
    mine = ((y.reshape(n, 32, -1) - mean[..., None]) * rstd[..., None]).reshape(y.shape)
    assert rel(mine, F.group_norm(y, 32, gamma, beta, 1e-6)) < 1e-12
    # an fp32 two-pass evaluation sits far inside the derived bounds
    m32, r32, _, _ = gn_stats_ref(y.float())
    assert ((r32.double() - rstd).abs() / rstd <= rstd_rel).all() and ((m32.double() - mean).abs() <= mean_abs).all()
    assert rstd_rel.max() < 1e-3 and rstd_rel.min() < 4e-6
