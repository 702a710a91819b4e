"""bevgen_amd/metrics.py on the GPU: the two metric classes over several updates against the float64 restatement (tests/metrics_ref.py, within the bounds of
tests/test_metrics_ops_gpu.py), `__call__`, the JSON round trip of the states, uint8 against fp32, accumulate_metrics / compute_metrics, the directory form on a small
JPEG tree, and one `generate --metrics` run on the tiny configuration tree of tests/test_generate_gpu.py."""
import json
import math
import textwrap

import pytest
import torch

import metrics_ref as MR
from bevgen_amd import metrics as M

pytestmark = pytest.mark.gpu

SHAPE = (24, 40)


def _batches(kind="smooth_noise"):
    """three updates of different sizes, the last as [B, cams, C, H, W]; -> [(preds, target)], and everything as one [n, C, H, W] pair"""
    p, t = MR.make_pair(kind, (7, 3, *SHAPE), seed=5)
    parts = [(p[:2], t[:2]), (p[2:3], t[2:3]), (p[3:].reshape(2, 2, 3, *SHAPE), t[3:].reshape(2, 2, 3, *SHAPE))]
    return parts, p, t


def _bounds(p, t):
    """the generic mean bound for SSIM (the mean over images of per-image means is off by at most the largest per-image error) and the squared-error bound carried to dB"""
    pf, tf = MR.as_float(p), MR.as_float(t)
    m64, m32 = MR.ssim_map(pf, tf), MR.ssim_map(pf, tf, torch.float32)
    e = (MR.image_means(m32) - MR.image_means(m64)).abs().max().item()
    # PSNR = 10 log10(R^2 n / sse): a relative error r of sse moves it by 10 log10(1 + r) <= 4.35 r dB; R comes from exact extremes
    return MR.image_means(m64).mean().item(), max(4 * e, MR.MEAN_FLOOR), 4.35 * MR.SSE_REL + 1e-12


def test_metric_classes_over_three_updates(gpu_ctx):
    parts, p, t = _batches()
    ssim, psnr = M.StructuralSimilarityIndexMeasure(data_range=1.0, ctx=gpu_ctx), M.PeakSignalNoiseRatio(ctx=gpu_ctx)
    for a, b in parts:
        ssim.update(a, b)
        psnr.update(a.cuda(), b.cuda())          # host or device tensors
    want_ssim, b_ssim, b_db = _bounds(p, t)
    want_psnr = MR.psnr64(MR.sse64(p, t).sum(), p.numel(), (t.max() - t.min()).double()).item()
    got_ssim, got_psnr = ssim.compute(), psnr.compute()
    assert got_ssim.is_cuda and got_ssim.dtype == torch.float64 and got_psnr.is_cuda and all(v.is_cuda for v in (ssim.sum, ssim.images, psnr.sse, psnr.count, psnr.min, psnr.max))
    print(f"ssim {got_ssim.item():.9f} vs {want_ssim:.9f}: {abs(got_ssim.item() - want_ssim) / b_ssim:.3f} of {b_ssim:.2e}; "
          f"psnr {got_psnr.item():.9f} vs {want_psnr:.9f} dB: {abs(got_psnr.item() - want_psnr) / b_db:.3f} of {b_db:.2e}")
    assert abs(got_ssim.item() - want_ssim) <= b_ssim and abs(got_psnr.item() - want_psnr) <= b_db
    assert ssim.state()["images"] == 7 and psnr.state()["count"] == p.numel()
    assert psnr.state()["min"] == t.min().item() and psnr.state()["max"] == t.max().item()
    # state -> JSON -> a fresh object (no context, on the CPU) -> the same value
    s2 = M.StructuralSimilarityIndexMeasure().load_state(json.loads(json.dumps(ssim.state())))
    p2 = M.PeakSignalNoiseRatio().load_state(json.loads(json.dumps(psnr.state())))
    assert s2.compute().item() == got_ssim.item() and abs(p2.compute().item() - got_psnr.item()) <= 1e-12 and not s2.compute().is_cuda
    # a fixed data_range takes the place of the extremes
    fixed = M.PeakSignalNoiseRatio(data_range=1.0, ctx=gpu_ctx)
    fixed.update(p, t)
    assert abs(fixed.compute().item() - MR.psnr64(MR.sse64(p, t).sum(), p.numel(), 1.0).item()) <= b_db
    ssim.reset()
    assert ssim.state() == {"sum": 0.0, "images": 0} and ssim.sum.is_cuda
    assert gpu_ctx.status() == 0


def test_call_returns_the_value_of_the_batch_and_updates(gpu_ctx):
    parts, p, t = _batches()
    ssim, psnr = M.StructuralSimilarityIndexMeasure(ctx=gpu_ctx), M.PeakSignalNoiseRatio(ctx=gpu_ctx)
    for a, b in parts:
        vs, vp = ssim(a, b), psnr(a, b)
        a4, b4 = a.reshape(-1, 3, *SHAPE), b.reshape(-1, 3, *SHAPE)
        want_s, b_s, b_db = _bounds(a4, b4)
        assert abs(vs.item() - want_s) <= b_s
        assert abs(vp.item() - MR.psnr64(MR.sse64(a4, b4).sum(), a4.numel(), (b4.max() - b4.min()).double()).item()) <= b_db
    whole_s, whole_p = M.StructuralSimilarityIndexMeasure(ctx=gpu_ctx), M.PeakSignalNoiseRatio(ctx=gpu_ctx)
    whole_s.update(p, t)
    whole_p.update(p, t)
    assert abs(ssim.compute().item() - whole_s.compute().item()) <= 1e-15 * 7     # per-image values do not depend on the batch they came in: only the order of 7 adds differs
    assert abs(psnr.compute().item() - whole_p.compute().item()) <= 1e-12
    assert ssim.state()["images"] == 7


def test_uint8_and_fp32_forms_of_the_quantised_pair_agree(gpu_ctx):
    (pu, tu), (pf, tf) = MR.make_pair("quant_u8", (2, 3, 64, 64)), MR.make_pair("quant_f32", (2, 3, 64, 64))
    out = {}
    for name, (a, b) in {"u8": (pu, tu), "f32": (pf, tf)}.items():
        s, q = M.StructuralSimilarityIndexMeasure(ctx=gpu_ctx), M.PeakSignalNoiseRatio(ctx=gpu_ctx)
        s.update(a, b)
        q.update(a, b)
        out[name] = (s.compute().item(), q.compute().item(), q.state())
    want_s, b_s, b_db = _bounds(pf, tf)
    assert abs(out["u8"][0] - out["f32"][0]) <= b_s and abs(out["u8"][0] - want_s) <= b_s
    assert abs(out["u8"][1] - out["f32"][1]) <= b_db
    exact = ((pu.long() - tu.long()) ** 2).sum().item() / 65025.0
    assert abs(out["u8"][2]["sse"] - exact) <= 1e-15 * exact and out["u8"][2]["min"] == out["f32"][2]["min"] and out["u8"][2]["max"] == out["f32"][2]["max"]


def test_accumulate_metrics_equals_the_direct_calls(gpu_ctx):
    parts, p, t = _batches()
    gen, gt = parts[2][0].cuda(), parts[2][1].cuda()                 # [2, 2, 3, H, W]
    rec = (0.5 * gen + 0.5 * gt).contiguous()
    ms = M.make_run_metrics(ctx=gpu_ctx)
    assert M.accumulate_metrics(ms, {"gen": gen, "rec": rec, "gt": gt}) == 4
    assert M.accumulate_metrics(ms, {"gen": gen[:1], "rec": None, "gt": gt[:1]}) == 2
    assert M.accumulate_metrics(ms, {"gen": gen, "rec": None, "gt": None}) == 0
    direct = {"gen_psnr": M.PeakSignalNoiseRatio(ctx=gpu_ctx), "gen_ssim": M.StructuralSimilarityIndexMeasure(ctx=gpu_ctx),
              "rec_psnr": M.PeakSignalNoiseRatio(ctx=gpu_ctx), "rec_ssim": M.StructuralSimilarityIndexMeasure(ctx=gpu_ctx)}
    for k in ("gen_psnr", "gen_ssim"):
        direct[k].update(gen, gt)
        direct[k].update(gen[:1], gt[:1])
    for k in ("rec_psnr", "rec_ssim"):
        direct[k].update(rec, gt)
    st = M.metrics_state(ms)
    assert st == {k: direct[k].state() for k in M.METRIC_KEYS}
    assert st["gen_ssim"]["images"] == 6 and st["rec_ssim"]["images"] == 4 and st["rec_psnr"]["count"] == 4 * 3 * SHAPE[0] * SHAPE[1]
    vals = M.report_metrics(ms)
    assert vals["rec_psnr"] > vals["gen_psnr"] and vals["rec_ssim"] > vals["gen_ssim"]        # half the error


def test_compute_metrics_prints_the_reference_lines(gpu_ctx, capsys):
    parts, p, t = _batches()
    out = M.compute_metrics([(b, a) for a, b in parts], ctx=gpu_ctx)                          # (gt, gen) pairs, as metrics_eval.compute_metrics takes them
    want_s, b_s, b_db = _bounds(p, t)
    assert abs(out["ssim"] - want_s) <= b_s
    assert abs(out["psnr"] - MR.psnr64(MR.sse64(p, t).sum(), p.numel(), (t.max() - t.min()).double()).item()) <= b_db
    assert capsys.readouterr().out.splitlines() == ["SSIM Score for dataset is: %.2f" % out["ssim"], "PSNR Score for dataset is: %.2f" % out["psnr"]]


def test_directory_form_on_a_small_jpeg_tree(gpu_ctx, tmp_path, capsys):
    """gt/ and gen/ JPEG trees -> the uint8 kernels; the expectation is computed from the decoded files, so JPEG's loss is on both sides"""
    import numpy as np
    from PIL import Image

    (pu, tu) = MR.make_pair("quant_u8", (3, 3, 24, 40), seed=2)
    for i in range(3):
        for tree, x in (("gt", tu), ("gen", pu)):
            d = tmp_path / tree / f"scene{i}"
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(x[i].permute(1, 2, 0).contiguous().numpy()).save(d / "cam.jpg", quality=95)
    (tmp_path / "gen" / "scene9").mkdir()
    Image.fromarray(pu[0].permute(1, 2, 0).contiguous().numpy()).save(tmp_path / "gen" / "scene9" / "cam.jpg")
    psnr, ssim = M.evaluate_directory(str(tmp_path), ctx=gpu_ctx)
    assert "Removed at least 1" in capsys.readouterr().out
    load = lambda tree: torch.stack([torch.from_numpy(np.asarray(Image.open(tmp_path / tree / f"scene{i}" / "cam.jpg")).copy()).permute(2, 0, 1) for i in range(3)])
    g, o = load("gt"), load("gen")
    want_s, b_s, b_db = _bounds(o, g)
    assert ssim.state()["images"] == 3 and abs(ssim.compute().item() - want_s) <= b_s
    R = (g.max().float() / 255 - g.min().float() / 255).double()
    assert abs(psnr.compute().item() - MR.psnr64(((o.long() - g.long()) ** 2).sum().item() / 65025.0, o.numel(), R).item()) <= b_db


def test_generate_with_and_without_the_metrics_flag(tmp_path, monkeypatch, capsys):
    from test_generate_gpu import CALLBACKS, MAIN, MODEL
    from bevgen_amd import generate

    cfgdir = tmp_path / "configs"
    for rel, text in {"train.yaml": MAIN, "model/tiny_muse.yaml": MODEL, "callbacks/default.yaml": CALLBACKS}.items():
        f = cfgdir / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(text).lstrip("\n"))
    argv = ["--config-dir", str(cfgdir), "--synthetic", "2", "--random-weights", "model.cfg.bev_latent_res=[4,4]"]
    out = tmp_path / "with"
    monkeypatch.setenv("BEVGEN_TEST_OUT", str(out))
    assert generate.main(argv + ["--metrics"]) == 0
    st = json.loads((out / "metrics_rank0.json").read_text())
    assert set(st) == set(M.METRIC_KEYS)
    scenes, cams, pixels = 2, 3, 3 * 64 * 64
    for split in ("gen", "rec"):
        assert st[f"{split}_ssim"]["images"] == scenes * cams and st[f"{split}_psnr"]["count"] == scenes * cams * pixels
        psnr = M.PeakSignalNoiseRatio().load_state(st[f"{split}_psnr"]).compute().item()
        ssim = M.StructuralSimilarityIndexMeasure().load_state(st[f"{split}_ssim"]).compute().item()
        print(f"generate --metrics [{split}]: ssim {ssim:.4f} psnr {psnr:.3f} dB")
        assert math.isfinite(psnr) and -1.0 <= ssim <= 1.0
    printed = capsys.readouterr().out
    assert "[gen] SSIM Score for dataset is: " in printed and "[rec] PSNR Score for dataset is: " in printed
    out2 = tmp_path / "without"
    monkeypatch.setenv("BEVGEN_TEST_OUT", str(out2))
    assert generate.main(argv) == 0
    assert (out2 / "sample").is_dir() and not list(out2.glob("metrics_rank*.json"))
