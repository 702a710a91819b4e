"""LPIPS (VGG16) end to end on the GPU, on an fp32 and on an f16x3 context, against the float64 restatement (tests/lpips_ref.py): every case and every tap separately,
then the total, inside 4 e32 (fp32) / 16 e32 (f16x3); identical pairs exactly 0; symmetry; uint8 and normalize against the fp32 call on the converted images, bit for bit;
the metric class over three updates; the f16 range flag; and one `generate --metrics --lpips-weights` run on the tiny configuration tree of tests/test_generate_gpu.py.

Achieved / bound (pytest -s prints them; experiments/r17.md has the table).  Measured on an MI355X, worst over the cases, taps and both argument orders: fp32 context 0.252
of 4 e32 (tap 4, independent 2 x 32 x 48), f16x3 context 0.153 of 16 e32 (tap 3, independent 1 x 16 x 16); the class over three updates 0.035 / 0.007.  (Before the fp32
convolution kernel's accumulation chain was cut in two levels - GemmArgs::acc_flush - the fp32 context missed one value: uint8 1 x 16 x 16, tap 3, 1.41 of the bound.)"""
import json
import textwrap

import pytest
import torch
import torch.nn.functional as F

import lpips_ref as LR
from bevgen_amd import _lib
from bevgen_amd import metrics as M

pytestmark = pytest.mark.gpu

FACTOR = {"fp32": 4.0, "f16x3": 16.0}


@pytest.fixture(scope="module", params=["fp32", "f16x3"])
def lp(request):
    """(context, prepared weights) of one precision"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bevgen_amd.runtime import Context

    c = Context(None, precision=request.param)
    yield c, c.lpips_prepare(LR.make_state())
    c.close()


def _check(name, precision, total, layers, ref):
    """every tap of every image, then the total, against float64 within FACTOR e32; -> the largest achieved / bound"""
    total, layers = total.cpu(), layers.cpu()
    worst = 0.0
    for k in range(6):
        got, want = (layers[:, k], ref["layers64"][:, k]) if k < 5 else (total, ref["total64"])
        bound = FACTOR[precision] * ref["e32"][k].item() * want.abs()
        frac = ((got - want).abs() / bound).max().item()
        worst = max(worst, frac)
        print(f"{name} [{precision}] {'tap %d' % k if k < 5 else 'total'}: {frac:.3f} of {FACTOR[precision]:.0f} e32 = {FACTOR[precision] * ref['e32'][k].item():.2e} (value {want.tolist()})")
        assert bool(((got - want).abs() <= bound).all()), (name, precision, k, got.tolist(), want.tolist(), bound.tolist())
    return worst


@pytest.mark.parametrize("shape", LR.CASE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", LR.CASE_KINDS)
def test_every_case_and_tap_against_float64(lp, kind, shape):
    ctx, prepared = lp
    ref = LR.case_reference(kind, shape)
    total, layers = ctx.lpips(prepared, ref["a"], ref["b"], return_layers=True)
    assert total.is_cuda and total.dtype == torch.float64 and total.shape == (shape[0],) and layers.shape == (shape[0], 5)
    if kind == "identical":
        assert bool((layers == 0).all()) and bool((total == 0).all())
    else:
        _check(f"{kind} {shape}", ctx.precision, total, layers, ref)
        # the other way round: inside the same bound
        t2, l2 = ctx.lpips(prepared, ref["b"], ref["a"], return_layers=True)
        _check(f"{kind} {shape} swapped", ctx.precision, t2, l2, ref)
    # the same bits on a second call, and without the layers
    again = ctx.lpips(prepared, ref["a"], ref["b"])
    assert torch.equal(again.view(torch.int64), total.view(torch.int64))
    assert ctx.status() == 0


def test_uint8_equals_the_fp32_call_on_v_over_255(lp):
    ctx, prepared = lp
    a, b = LR.make_pair("uint8", (2, 32, 48))
    t8, l8 = ctx.lpips(prepared, a, b, return_layers=True)
    tf, lf = ctx.lpips(prepared, a.float() / 255.0, b.float() / 255.0, return_layers=True)
    assert torch.equal(l8.view(torch.int64), lf.view(torch.int64)) and torch.equal(t8.view(torch.int64), tf.view(torch.int64))


def test_normalize_equals_the_call_on_2x_minus_1(lp):
    ctx, prepared = lp
    a, b = LR.make_pair("independent", (2, 32, 48))
    tn, ln = ctx.lpips(prepared, a, b, normalize=True, return_layers=True)
    tp, lpl = ctx.lpips(prepared, 2 * a - 1, 2 * b - 1, return_layers=True)
    assert torch.equal(ln.view(torch.int64), lpl.view(torch.int64)) and torch.equal(tn.view(torch.int64), tp.view(torch.int64))
    ref = LR.case_reference("independent", (2, 32, 48), True)
    _check("normalize=True", ctx.precision, tn, ln, ref)


def test_more_pairs_than_a_chunk_give_the_same_per_image_values(lp):
    """66 pairs of 16 x 16 run as a chunk of 64 and one of 2: each image's value is what it is alone"""
    ctx, prepared = lp
    assert ctx.lib.bevgen_lpips_workspace_bytes(66, 16, 16, _lib.PRECISION_FP32) == ctx.lib.bevgen_lpips_workspace_bytes(64, 16, 16, _lib.PRECISION_FP32)
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand((66, 3, 16, 16), generator=g), torch.rand((66, 3, 16, 16), generator=g)
    t, l = ctx.lpips(prepared, a, b, return_layers=True)
    for i in (0, 63, 64, 65):
        t1, l1 = ctx.lpips(prepared, a[i:i + 1], b[i:i + 1], return_layers=True)
        assert torch.equal(l1[0].view(torch.int64), l[i].view(torch.int64)) and torch.equal(t1[0].view(torch.int64), t[i].view(torch.int64)), i


def test_small_images_are_refused_before_any_launch(lp):
    ctx, prepared = lp
    for shape in ((1, 3, 15, 16), (1, 3, 16, 15), (0, 3, 16, 16)):
        with pytest.raises(ValueError):
            ctx.lpips(prepared, torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError):
        ctx.lpips(prepared, torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 17))
    work = torch.empty((1 << 20,), dtype=torch.uint8, device=ctx.device)
    out = torch.zeros((1,), dtype=torch.float64, device=ctx.device)
    x = torch.zeros((1, 3, 15, 16), device=ctx.device)
    code = ctx.lib.bevgen_lpips(ctx._h, prepared.data_ptr(), x.data_ptr(), x.data_ptr(), _lib.DTYPE_F32, 1, 15, 16, 0, out.data_ptr(), None, work.data_ptr(), ctx._s())
    assert code == -1 and b"relu5_3" in ctx.lib.bevgen_last_error(ctx._h)


def test_the_class_over_three_updates_and_five_dimensional_input(lp):
    ctx, prepared = lp
    shape = (5, 32, 48)
    ref = LR.case_reference("near", shape)
    a, b = ref["a"], ref["b"]
    parts = [(a[:2], b[:2]), (a[2:3].cuda(), b[2:3].cuda()), (a[3:].reshape(1, 2, 3, 32, 48), b[3:].reshape(1, 2, 3, 32, 48))]
    mean, none = M.LearnedPerceptualImagePatchSimilarity(weights=LR.make_state(), ctx=ctx), M.LearnedPerceptualImagePatchSimilarity(reduction="none", weights=LR.make_state(), ctx=ctx)
    total = M.LearnedPerceptualImagePatchSimilarity(reduction="sum", weights=LR.make_state(), ctx=ctx)
    for x, y in parts:
        mean.update(x, y)
        total.update(x, y)
        last = none(x, y)
    want = ref["total64"].mean().item()
    bound = FACTOR[ctx.precision] * ref["e32"][5].item() * want
    got = mean.compute()
    print(f"class, three updates [{ctx.precision}]: {abs(got.item() - want) / bound:.3f} of the bound, mean {want:.6e}")
    assert got.is_cuda and got.dtype == torch.float64 and mean.sum_scores.is_cuda and abs(got.item() - want) <= bound
    assert mean.state()["total"] == 5 and abs(total.compute().item() - 5 * want) <= 5 * bound
    # reduction='none': the per-image scores of the last batch (what filter_generated.py reads), from __call__ and from compute()
    assert last.shape == (2,) and torch.equal(last, none.compute())
    assert bool(((last.cpu() - ref["total64"][3:]).abs() <= FACTOR[ctx.precision] * ref["e32"][5].item() * ref["total64"][3:]).all())
    # state -> JSON -> a fresh object without a context
    again = M.LearnedPerceptualImagePatchSimilarity(weights=LR.make_state()).load_state(json.loads(json.dumps(mean.state())))
    assert again.compute().item() == got.item() and not again.compute().is_cuda
    assert ctx.status() == 0


def test_compute_metrics_prints_the_lpips_line_first(lp, capsys):
    ctx, _ = lp
    ref = LR.case_reference("near", (5, 32, 48))
    pairs = [(ref["b"][:3], ref["a"][:3]), (ref["b"][3:], ref["a"][3:])]          # (gt, gen)
    plain = M.compute_metrics(pairs, ctx=ctx)
    first = capsys.readouterr().out.splitlines()
    assert set(plain) == {"ssim", "psnr"} and first == ["SSIM Score for dataset is: %.2f" % plain["ssim"], "PSNR Score for dataset is: %.2f" % plain["psnr"]]
    out = M.compute_metrics(pairs, ctx=ctx, lpips_weights=LR.make_state())
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["PSIM/LPIPS Score for dataset is: %.2f" % out["lpips"]] + first and out["ssim"] == plain["ssim"] and out["psnr"] == plain["psnr"]
    want = ref["total64"].mean().item()
    assert abs(out["lpips"] - want) <= FACTOR[ctx.precision] * ref["e32"][5].item() * want


def test_an_activation_outside_the_f16_range_is_flagged_in_f16x3_and_runs_in_fp32(lp):
    ctx, prepared = lp
    st = LR.make_state()
    g = torch.Generator().manual_seed(9)
    a, b = torch.rand((1, 3, 16, 16), generator=g) * 2.0e4, torch.rand((1, 3, 16, 16), generator=g) * 2.0e4
    # the premise: the scaled input is inside the f16 range, relu1_1 is not
    x0 = (a - st["shift"][None, :, None, None]) / st["scale"][None, :, None, None]
    r11 = F.relu(F.conv2d(x0, st["conv_w"][0], st["conv_b"][0], padding=1))
    assert x0.abs().max().item() < 6.0e4 and r11.max().item() > 7.0e4
    if ctx.precision == "fp32":
        total = ctx.lpips(prepared, a, b)
        assert bool(torch.isfinite(total).all()) and ctx.status() == 0
    else:
        with pytest.raises(_lib.BevgenError) as e:
            ctx.lpips(prepared, a, b, check=True)
        assert e.value.code == _lib.ERR_NUMERIC
        assert ctx.status() == 0                      # reported once, then cleared
        ref = LR.case_reference("independent", (1, 16, 16))
        assert bool(torch.isfinite(ctx.lpips(prepared, ref["a"], ref["b"])).all())


def test_generate_with_lpips_weights(tmp_path, monkeypatch, capsys):
    from test_generate_gpu import CALLBACKS, MAIN, MODEL
    from bevgen_amd import generate

    cfgdir = tmp_path / "configs"
    for rel, text in {"train.yaml": MAIN, "model/tiny_muse.yaml": MODEL, "callbacks/default.yaml": CALLBACKS}.items():
        f = cfgdir / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(text).lstrip("\n"))
    sd = LR.reference_state_dict(spelling="torchvision")
    torch.save({k: v for k, v in sd.items() if k.startswith("features.")}, tmp_path / "vgg16_features.pth")
    torch.save({k: v for k, v in LR.reference_state_dict().items() if k.startswith("lin")}, tmp_path / "vgg.pth")
    argv = ["--config-dir", str(cfgdir), "--synthetic", "2", "--random-weights", "model.cfg.bev_latent_res=[4,4]", "--metrics"]
    out = tmp_path / "with"
    monkeypatch.setenv("BEVGEN_TEST_OUT", str(out))
    assert generate.main(argv + ["--lpips-weights", str(tmp_path / "vgg.pth"), str(tmp_path / "vgg16_features.pth")]) == 0
    st = json.loads((out / "metrics_rank0.json").read_text())
    assert set(st) == set(M.METRIC_KEYS) | set(M.LPIPS_KEYS)
    printed = capsys.readouterr().out
    for split in ("gen", "rec"):
        assert st[f"{split}_lpips"]["total"] == 2 * 3 and st[f"{split}_lpips"]["sum_scores"] > 0
        value = st[f"{split}_lpips"]["sum_scores"] / st[f"{split}_lpips"]["total"]
        print(f"generate --metrics --lpips-weights [{split}]: lpips {value:.5f}")
        assert f"[{split}] PSIM/LPIPS Score for dataset is: {value:.2f}" in printed
        assert printed.index(f"[{split}] PSIM/LPIPS") < printed.index(f"[{split}] SSIM")
    out2 = tmp_path / "without"
    monkeypatch.setenv("BEVGEN_TEST_OUT", str(out2))
    assert generate.main(argv) == 0
    plain = json.loads((out2 / "metrics_rank0.json").read_text())
    assert set(plain) == set(M.METRIC_KEYS) and "PSIM/LPIPS" not in capsys.readouterr().out
    for k in M.METRIC_KEYS:                                                                  # the four states do not depend on the flag
        assert plain[k].get("images", plain[k].get("count")) == st[k].get("images", st[k].get("count"))
    assert plain["rec_psnr"] == st["rec_psnr"] and plain["rec_ssim"] == st["rec_ssim"]
