"""Operator-level parity of the stage-1 VQGAN building blocks (csrc/vqdec.cpp, vq.hip, vqenc_kernels.hip, the GroupNorm-statistics epilogue of gemm_split_glds.hip) through
their bevgen_op_* entries, each against an fp64 statement of the same operation (builders and references: tests/test_vq_ref_cpu.py, which checks them without a GPU).

Worst errors measured on an MI355X (each test prints its own, `pytest -s`); the bounds are the ones of the existing operator tests or derived in test_vq_ref_cpu.py:
  conv3x3_down    7.7e-7 (fp32) / 2.9e-7 (f16x3) relative, bound 2e-6; both padding probes exact
  vq_attn_block   8.9e-7 (fp32) / 8.7e-7 (f16x3) relative, bound 1e-5 (0.09 of it)
  vq_out_tail     float modes: at most 0.082 of the bound 1.2e-5 absmax (fused), 0.072 (three kernels), 0.097 (fused against three kernels); uint8: no pixel differs from
                  round(255 ref) in any case, 2 / 13 / 13 pixels (1.9 % / 0.85 % / 0.77 %) left undecided by the bound
  vq_quantize     no row left out by the margin rule in any of the 36 float cases; |z|^2, |e|^2 at most 1.7e-7 relative
  conv3x3_gn_stats (epilogue statistics, k = 8): relative rstd error at r ~ 0 / 3 / 30: 6.9e-8 / 2.7e-7 / 1.7e-5 (bounds 2.8e-6 / 9.1e-6 / 6.5e-4); mean error at most 1.3e-6
                  (bound 6.8e-5); bit-identical run to run and to the range-safe route.  Ladder of r over the groups of one tensor: the normalised tensor stays within the
                  1e-5 of test_groupnorm at every step up to r ~ 24 (7.0e-6 at r ~ 16, 5.3e-6 at r ~ 24) and leaves it at r ~ 30 (1.7e-5; 4.1e-5 at 60, 1.2e-4 at 100,
                  1.1e-3 at 200): the error grows like 0.3 r^2 2^-24, where the derived bound allows 12 r^2 2^-24."""
import pytest
import torch
import torch.nn.functional as F

from test_vq_ref_cpu import (ATTN_BOUND, ATTN_SHAPES, CONV_BOUND, DOWN_SHAPES, GN_BOUND, GN_EPI_K, GN_EPI_LADDER, GN_EPI_R, GN_EPI_SHAPES, QUANT_D, QUANT_NE, QUANT_ROWS,
                             TAIL_BOUND, TAIL_SHAPES, attn_case, attn_ref, down_case, down_probe_case, down_ref, gn_epi_bounds, gn_epi_case, nchw, nhwc,
                             quant_decidable, quant_exact_case, quant_float_case, quant_nonfinite_case, quant_ref, rel, tail_case, tail_ref, tail_u8_decidable)

pytestmark = pytest.mark.gpu


def dev(t):
    return t.cuda().contiguous()


@pytest.fixture(scope="module")
def gpu_ctx_split():
    """A model-less context in split-precision mode: the entries register their weights as split weights, so the convolutions and 1x1 projections take the kernels the
    model takes under precision='f16x3'."""
    from bevgen_amd.runtime import Context

    ctx = Context(None, precision="f16x3")
    yield ctx
    ctx.close()


@pytest.fixture(params=["fp32", "f16x3"])
def any_ctx(request, gpu_ctx, gpu_ctx_split):
    return gpu_ctx if request.param == "fp32" else gpu_ctx_split


def refused(match):
    from bevgen_amd import _lib

    return pytest.raises(_lib.BevgenError, match=match)


def consume_status(ctx, bit, text):
    """After a call whose kernel may have raised a bit: the word as the host sees it, reported and cleared the way a caller meets it (synchronize()).  bit 0: none."""
    from bevgen_amd import _lib

    torch.cuda.synchronize()
    word = ctx.status()
    try:
        if bit:
            assert word == bit, word
            with pytest.raises(_lib.BevgenError, match=text) as ei:
                ctx.synchronize()
            assert ei.value.code == _lib.ERR_NUMERIC
        else:
            assert word == 0
            ctx.synchronize()
    finally:
        if ctx.status():   # never leave a word behind for the next test of the shared context
            try:
                ctx.synchronize()
            except _lib.BevgenError:
                pass
    assert ctx.status() == 0


# ================================================================================================ downsample convolution
@pytest.mark.parametrize("shape", DOWN_SHAPES)
def test_conv3x3_down(any_ctx, shape):
    x, w, b = down_case(*shape)
    ref = down_ref(x, w, b)
    out = nchw(any_ctx.op_conv3x3_down(dev(nhwc(x)), dev(w), dev(b)).cpu())
    err = rel(out, ref)
    print(f"conv3x3_down {any_ctx.precision} {shape}: {err:.2e} (bound {CONV_BOUND:.0e})")
    assert out.shape == ref.shape
    assert err < CONV_BOUND


@pytest.mark.parametrize("which", ["last", "first"])
def test_conv3x3_down_pads_bottom_and_right(any_ctx, which):
    x, w, b = down_probe_case(which)
    ref = down_ref(x, w, b)
    out = nchw(any_ctx.op_conv3x3_down(dev(nhwc(x)), dev(w), dev(b)).cpu())
    assert rel(out, ref) < CONV_BOUND
    bias_only = b.reshape(1, -1, 1, 1).expand_as(out)
    if which == "last":   # nothing but padding and zeros under the (2, 2) tap: the bias, exactly
        assert torch.equal(out, bias_only)
    else:
        assert torch.equal(out[:, :, 1:, 1:], bias_only[:, :, 1:, 1:]) and (out[:, :, 0, :] != bias_only[:, :, 0, :]).any()


def test_conv3x3_down_refuses_odd_sizes(gpu_ctx):
    with refused("even H, W"):
        gpu_ctx.op_conv3x3_down(torch.zeros(1, 3, 4, 32).cuda(), torch.zeros(32, 32, 3, 3).cuda(), None)


# ================================================================================================ AttnBlock
@pytest.mark.parametrize("shape", ATTN_SHAPES)
def test_vq_attn_block(any_ctx, shape):
    p = attn_case(*shape)
    ref = attn_ref(p)
    d = {k: dev(v) for k, v in p.items() if k != "x"}
    out = any_ctx.op_vq_attn_block(dev(nhwc(p["x"])), d["norm_w"], d["norm_b"], d["wq"], d["bq"], d["wk"], d["bk"], d["wv"], d["bv"], d["wp"], d["bp"])
    consume_status(any_ctx, 0, None)   # (a NaN that reached an f16 operand writer would sit in the shared context's status word)
    out = nchw(out.cpu())
    err = rel(out, ref)
    print(f"vq_attn_block {any_ctx.precision} {shape}: {err:.2e} (bound {ATTN_BOUND:.0e})")
    assert torch.isfinite(out).all()
    assert err < ATTN_BOUND


# ================================================================================================ decoder tail
_TAIL = {}


def _tail(shape):
    """The case, its fp64 references and the float bound, computed once per shape."""
    if shape not in _TAIL:
        p = tail_case(*shape)
        raw = tail_ref(p)
        _TAIL[shape] = (p, {"raw": raw, "denorm": tail_ref(p, "denorm"), "u8": tail_ref(p, "u8")}, TAIL_BOUND * raw.abs().max().item())
    return _TAIL[shape]


def _run_tail(ctx, p, mode, fused, x=None):
    return ctx.op_vq_out_tail(dev(nhwc(p["x"] if x is None else x)), dev(p["norm_w"]), dev(p["norm_b"]), dev(p["w"]), dev(p["b"]), mode=mode, mean=dev(p["mean"]), std=dev(p["std"]),
                              fused=fused).cpu()


@pytest.mark.parametrize("mode", ["raw", "denorm"])
@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_vq_out_tail_float_modes(any_ctx, shape, mode):
    p, refs, bound = _tail(shape)
    fused = _run_tail(any_ctx, p, mode, True)
    three = _run_tail(any_ctx, p, mode, False)
    e1, e2, e3 = ((a.double() - b.double()).abs().max().item() for a, b in ((fused, refs[mode]), (three, refs[mode]), (fused, three)))
    print(f"vq_out_tail {any_ctx.precision} {mode} {shape}: fused {e1 / bound:.3f}, three kernels {e2 / bound:.3f}, fused vs three {e3 / bound:.3f} of the bound {bound:.2e}")
    assert fused.shape == refs[mode].shape == three.shape
    assert e1 <= bound and e2 <= bound and e3 <= bound
    if mode == "denorm":
        assert fused.min() >= 0 and fused.max() <= 1 and (fused == 0).any() and (fused == 1).any()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_vq_out_tail_uint8(any_ctx, shape, fused):
    p, refs, bound = _tail(shape)
    out = _run_tail(any_ctx, p, "u8", fused)
    assert out.dtype == torch.uint8
    ref8 = torch.round(refs["u8"])
    diff = (out.double() - ref8).abs()
    decidable = tail_u8_decidable(refs["u8"], bound)
    print(f"vq_out_tail {any_ctx.precision} u8 {shape} fused={fused}: {int((diff != 0).sum())} of {diff.numel()} pixels differ, {int((~decidable).sum())} undecided by the bound")
    assert diff.max() <= 1
    assert (diff[decidable] == 0).all()
    assert (out == 0).any() and (out == 255).any()


@pytest.mark.parametrize("fused", [True, False])
def test_vq_out_tail_flags_a_nan_pixel(gpu_ctx, fused):
    from bevgen_amd import _lib

    p, _, _ = _tail(TAIL_SHAPES[0])
    x = p["x"].clone()
    x[0, 3, 2, 4] = float("nan")
    _run_tail(gpu_ctx, p, "u8", fused, x=x)
    consume_status(gpu_ctx, _lib.STATUS_NONFINITE_PIXELS, "NaN / inf pixel")
    _run_tail(gpu_ctx, p, "u8", fused)
    consume_status(gpu_ctx, 0, None)


# ================================================================================================ quantizer
@pytest.mark.parametrize("D", QUANT_D)
@pytest.mark.parametrize("n_e", QUANT_NE)
@pytest.mark.parametrize("rows", QUANT_ROWS)
def test_vq_quantize_exact_cases_and_ties(gpu_ctx, rows, n_e, D):
    for variant in range(3):
        z, cb, _ = quant_exact_case(rows, n_e, D, variant)
        ref, _ = quant_ref(z, cb)
        ids, zz, ee = gpu_ctx.op_vq_quantize(dev(z), dev(cb), want_norms=True)
        assert torch.equal(ids.cpu(), ref), variant
        assert torch.equal(zz.cpu(), (z ** 2).sum(1)) and torch.equal(ee.cpu(), (cb ** 2).sum(1))   # (integers: exact)


@pytest.mark.parametrize("D", QUANT_D)
@pytest.mark.parametrize("n_e", QUANT_NE)
@pytest.mark.parametrize("rows", QUANT_ROWS)
def test_vq_quantize_float_cases(gpu_ctx, rows, n_e, D):
    z, cb = quant_float_case(rows, n_e, D)
    ref, _ = quant_ref(z, cb)
    keep = quant_decidable(z, cb)
    ids, zz, ee = gpu_ctx.op_vq_quantize(dev(z), dev(cb), want_norms=True)
    ids = ids.cpu()
    zz_ref, ee_ref = (z.double() ** 2).sum(1), (cb.double() ** 2).sum(1)
    ez = ((zz.cpu().double() - zz_ref).abs() / zz_ref).max().item()
    ec = ((ee.cpu().double() - ee_ref).abs() / ee_ref).max().item()
    print(f"vq_quantize rows={rows} n_e={n_e} D={D}: {int((~keep).sum())} rows left out, |z|^2 {ez:.1e}, |e|^2 {ec:.1e}")
    assert ((ids >= 0) & (ids < n_e)).all()
    assert torch.equal(ids[keep], ref[keep])
    depth = max(D // 64, 1) + 6   # a sum of squares: an fmaf chain of D / 64 terms per lane, then a six-level tree over the wave - each level rounds once
    assert ez <= depth * 2.0 ** -24 and ec <= depth * 2.0 ** -24


@pytest.mark.parametrize("n_e", [63, 1000])
def test_vq_quantize_rows_without_a_finite_distance(gpu_ctx, n_e):
    from bevgen_amd import _lib

    z, cb, bad = quant_nonfinite_case(5, n_e, 32)
    good = [r for r in range(5) if r not in bad]
    ref, _ = quant_ref(z[good], cb)
    ids = gpu_ctx.op_vq_quantize(dev(z), dev(cb))
    consume_status(gpu_ctx, _lib.STATUS_NONFINITE_LATENTS, "without a finite distance")
    ids = ids.cpu()
    assert (ids[bad] == 0).all()
    assert torch.equal(ids[good], ref)
    # a NaN in one codebook row: that entry never wins, nothing is raised
    z, cb = quant_float_case(5, n_e, 32)
    ref, _ = quant_ref(z, cb)
    poisoned = int(ref[0])
    cb2 = cb.clone()
    cb2[poisoned, 7] = float("nan")
    rest = [j for j in range(n_e) if j != poisoned]
    ref2 = torch.tensor(rest)[quant_ref(z, cb[rest])[0]]
    keep = quant_decidable(z, cb[rest])
    ids = gpu_ctx.op_vq_quantize(dev(z), dev(cb2))
    consume_status(gpu_ctx, 0, None)
    ids = ids.cpu()
    assert (ids != poisoned).all() and keep[0]
    assert torch.equal(ids[keep], ref2[keep])


# ================================================================================================ GroupNorm statistics out of the convolution epilogue
_GN = {}


def _gn_epi(shape, ladder=GN_EPI_R):
    if (shape, ladder) not in _GN:
        x, w, b = gn_epi_case(*shape, ladder=ladder)
        y = F.conv2d(x.double(), w.double(), b.double(), padding=1)
        _GN[(shape, ladder)] = (x, w, b, y, gn_epi_bounds(y))
    return _GN[(shape, ladder)]


def _gn_errors(stats, y, bounds):
    mean, rstd, r, rstd_rel, mean_abs = bounds
    d_rstd = (stats[..., 1].double() - rstd).abs() / rstd
    d_mean = (stats[..., 0].double() - mean).abs()
    # what the error does to the normalised tensor, as test_groupnorm measures it: max |(y - mean') rstd' - (y - mean) rstd| over the output's absmax
    n = y.shape[0]
    v = y.reshape(n, 32, -1)
    norm = (v - mean[..., None]) * rstd[..., None]
    got = (v - stats[..., 0].double()[..., None]) * stats[..., 1].double()[..., None]
    d_out = (got - norm).abs().amax(2) / norm.abs().max()
    return d_rstd, d_mean, d_out


@pytest.mark.parametrize("shape", GN_EPI_SHAPES)
def test_conv3x3_gn_stats_epilogue(gpu_ctx_split, shape):
    """k = 8 roundings per fp32 partial (the product, the fmaf, the pair add, four DPP steps, one xor16 step; the plain sum has 7): bounds in test_vq_ref_cpu.gn_epi_bounds."""
    x, w, b, y_ref, bounds = _gn_epi(shape)
    mean, rstd, r, rstd_rel, mean_abs = bounds
    args = (dev(nhwc(x)), dev(w), dev(b))
    y, part, stats = gpu_ctx_split.op_conv3x3_gn_stats(*args)
    y2, part2, stats2 = gpu_ctx_split.op_conv3x3_gn_stats(*args)
    yr, partr, statsr = gpu_ctx_split.op_conv3x3_gn_stats(*args, range_route=True)
    consume_status(gpu_ctx_split, 0, None)
    y, part, stats = y.cpu(), part.cpu(), stats.cpu()
    assert rel(nchw(y), y_ref) < CONV_BOUND
    # the partials are what they claim to be: sums over 32 pixels x 4 channels of the tensor that was written
    n, H, W, Cout = y.shape
    blocks = y.double().reshape(n * H * W // 32, 32, Cout // 4, 4)
    assert rel(part[..., 0], blocks.sum((1, 3))) < 2 * GN_EPI_K * 2.0 ** -24 and rel(part[..., 1], (blocks ** 2).sum((1, 3))) < 2 * GN_EPI_K * 2.0 ** -24
    d_rstd, d_mean, d_out = _gn_errors(stats, y_ref, bounds)
    for i, target in enumerate(GN_EPI_R):
        sl = slice(i, None, len(GN_EPI_R))
        print(f"conv3x3_gn_stats {shape} r~{target:g}: rstd error {d_rstd[:, sl].max():.2e} (bound {rstd_rel[:, sl].min():.2e}), mean error {d_mean[:, sl].max():.2e} "
              f"(bound {mean_abs[:, sl].min():.2e}), normalised output {d_out[:, sl].max():.2e}")
    assert (d_rstd <= rstd_rel).all(), (d_rstd / rstd_rel).max()
    assert (d_mean <= mean_abs).all(), (d_mean / mean_abs).max()
    # bit-identical run to run, and the range-safe route leaves the same bits (vq.hip: "same layout, same order of additions")
    assert torch.equal(part, part2.cpu()) and torch.equal(stats, stats2.cpu()) and torch.equal(y, y2.cpu())
    assert torch.equal(part, partr.cpu()) and torch.equal(stats, statsr.cpu()) and torch.equal(y, yr.cpu())


def test_conv3x3_gn_stats_where_the_epilogue_leaves_the_groupnorm_bound(gpu_ctx_split):
    """A ladder of mean / std ratios over the groups of one tensor: the derived bounds hold at every step; printed: the largest r at which the statistics still give a
    normalised tensor within the 1e-5 of test_groupnorm (measured on an MI355X: every step up to r ~ 24 inside, r ~ 30 outside at 1.7e-5; module docstring)."""
    shape = GN_EPI_SHAPES[0]
    x, w, b, y_ref, bounds = _gn_epi(shape, GN_EPI_LADDER)
    mean, rstd, r, rstd_rel, mean_abs = bounds
    _, _, stats = gpu_ctx_split.op_conv3x3_gn_stats(dev(nhwc(x)), dev(w), dev(b))
    consume_status(gpu_ctx_split, 0, None)
    d_rstd, d_mean, d_out = _gn_errors(stats.cpu(), y_ref, bounds)
    L = len(GN_EPI_LADDER)
    worst = [(GN_EPI_LADDER[i], d_rstd[:, i::L].max().item(), d_out[:, i::L].max().item()) for i in range(L)]
    for t, a, o in worst:
        print(f"conv3x3_gn_stats ladder r~{t:g}: rstd error {a:.2e}, normalised output error {o:.2e}")
    first_out = min([t for t, _, o in worst if o > GN_BOUND], default=None)
    inside = [t for t, _, o in worst if first_out is None or t < first_out]
    print(f"conv3x3_gn_stats: every step up to r~{max(inside) if inside else None:g} within {GN_BOUND:.0e}; first r beyond it: {first_out}")
    assert (d_rstd <= rstd_rel).all(), (d_rstd / rstd_rel).max()
    assert (d_mean <= mean_abs).all(), (d_mean / mean_abs).max()


def test_conv3x3_gn_stats_refuses_shapes_without_partials(gpu_ctx_split, gpu_ctx):
    for n, H, W, Cin, Cout in ((1, 8, 8, 32, 128), (2, 16, 8, 32, 128), (1, 16, 16, 32, 64)):
        with refused("groupnorm from partials: unsupported shape"):
            gpu_ctx_split.op_conv3x3_gn_stats(torch.zeros(n, H, W, Cin).cuda(), torch.zeros(Cout, Cin, 3, 3).cuda(), torch.zeros(Cout).cuda())
    with refused("split-precision"):
        gpu_ctx.op_conv3x3_gn_stats(torch.zeros(1, 16, 16, 32).cuda(), torch.zeros(128, 32, 3, 3).cuda(), torch.zeros(128).cuda())
