"""LPIPS (VGG16) without a GPU: the weight loader and its three key spellings, the metric class's states, the refusals, the new exports and the pure size functions,
the unchanged two-metric output of compute_metrics / main without weights, and the restatement's own checks (tests/lpips_ref.py): the seeded weights behave as stated,
the fp32 restatement stays inside the tap operator's bound, identical pairs give exactly 0."""
import json
import re

import pytest
import torch

import lpips_ref as LR
from bevgen_amd import _lib
from bevgen_amd import metrics as M


# ================================================================================================ weights
def test_the_three_key_spellings_load_to_the_same_tensors(tmp_path):
    want = LR.make_state()
    ref = LR.reference_state_dict(spelling="reference", dropout=True)
    tv = LR.reference_state_dict(spelling="torchvision", dropout=False)
    assert "net.slice3.14.weight" in ref and "lin4.model.1.weight" in ref and "features.28.bias" in tv and "lin0.model.0.weight" in tv
    # two files, as a user of the reference has them: the features under torchvision's names, the lin layers under the reference's
    feats = {k: v for k, v in tv.items() if k.startswith("features.")}
    lins = {k: v for k, v in ref.items() if k.startswith("lin")}
    torch.save(feats, tmp_path / "vgg16_features.pth")
    torch.save(lins, tmp_path / "vgg.pth")
    for got in (M.load_lpips_state(ref), M.load_lpips_state(tv), M.load_lpips_state(str(tmp_path / "vgg16_features.pth"), str(tmp_path / "vgg.pth")), M.load_lpips_state(feats, lins)):
        assert len(got["conv_w"]) == 13 and len(got["conv_b"]) == 13 and len(got["lin"]) == 5
        for key in ("conv_w", "conv_b", "lin"):
            assert all(torch.equal(g, w.reshape(g.shape)) and g.dtype == torch.float32 for g, w in zip(got[key], want[key])), key
        assert torch.equal(got["shift"], torch.tensor(M.LPIPS_SHIFT)) and torch.equal(got["scale"], torch.tensor(M.LPIPS_SCALE))
    assert [tuple(w.shape[:2]) for w in want["conv_w"]] == list(M.LPIPS_CONV_SHAPES) and M.LPIPS_CONV_INDEX == LR.CONV_INDEX


def test_scaling_layer_buffers_override_the_constants():
    sd = LR.reference_state_dict(scaling=True)
    sd["scaling_layer.shift"] = torch.tensor([0.1, 0.2, 0.3]).reshape(1, 3, 1, 1)
    got = M.load_lpips_state(sd)
    assert torch.equal(got["shift"], torch.tensor([0.1, 0.2, 0.3])) and torch.equal(got["scale"], torch.tensor(M.LPIPS_SCALE))


def test_a_missing_key_or_a_wrong_shape_is_named():
    sd = LR.reference_state_dict()
    del sd["net.slice4.19.bias"], sd["lin2.model.1.weight"]
    with pytest.raises(ValueError) as e:
        M.load_lpips_state(sd)
    assert "net.slice4.19.bias" in str(e.value) and "features.19.bias" in str(e.value) and "lin2.model.1.weight" in str(e.value) and "net.slice4.19.weight" not in str(e.value)
    sd = LR.reference_state_dict()
    sd["net.slice2.7.weight"] = torch.zeros(128, 64, 3, 3)
    with pytest.raises(ValueError, match=r"net\.slice2\.7\.weight.*\(128, 64, 3, 3\).*\(128, 128, 3, 3\)"):
        M.load_lpips_state(sd)
    sd = LR.reference_state_dict()
    sd["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        M.load_lpips_state(sd)


# ================================================================================================ the metric class
def _metric(**kw):
    return M.LearnedPerceptualImagePatchSimilarity(weights=LR.make_state(), **kw)


def test_states_merge_and_compute_without_a_gpu():
    a, b = _metric(), _metric(reduction="sum")
    assert a.state() == {"sum_scores": 0.0, "total": 0} and (a.net_type, a.reduction, a.normalize) == ("vgg", "mean", False)
    assert a.sum_scores.dtype == torch.float64 and a.total.dtype == torch.int64
    a.load_state({"sum_scores": 0.5, "total": 4})
    b.load_state(json.loads(json.dumps({"sum_scores": 0.25, "total": 2})))
    a.merge_state(b).merge_state({"sum_scores": 0.25, "total": 2})
    assert a.state() == {"sum_scores": 1.0, "total": 8} and a.compute().item() == 0.125 and b.compute().item() == 0.25
    with pytest.raises(RuntimeError, match="last update"):
        _metric(reduction="none").load_state({"sum_scores": 0.5, "total": 4}).compute()
    a.reset()
    assert a.state() == {"sum_scores": 0.0, "total": 0}


def test_compute_before_update_raises():
    with pytest.raises(RuntimeError, match="before any update"):
        _metric().compute()


def test_update_without_a_gpu_raises_the_no_cpu_path_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p, t = LR.make_pair("independent", (1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU path in the product"):
        _metric().update(p, t)
    with pytest.raises(RuntimeError, match="no CPU path in the product"):
        _metric()(p, t)


def test_other_networks_missing_weights_and_bad_reductions_are_refused():
    with pytest.raises(NotImplementedError):
        M.LearnedPerceptualImagePatchSimilarity(net_type="alex", weights=LR.make_state())
    with pytest.raises(ValueError, match=r"vgg\.pth.*VGG16 features"):
        M.LearnedPerceptualImagePatchSimilarity()
    with pytest.raises(ValueError):
        _metric(reduction="median")
    p, t = LR.make_pair("independent", (1, 16, 16))
    with pytest.raises(ValueError):
        _metric().update(p, t[..., :15])
    with pytest.raises(ValueError):
        _metric().update(p.double(), t.double())


# ================================================================================================ header, binding, size functions
NEW_EXPORTS = ("bevgen_lpips_prepared_bytes", "bevgen_lpips_prepare", "bevgen_lpips", "bevgen_lpips_workspace_bytes", "bevgen_op_conv3x3_act", "bevgen_op_maxpool2x2",
               "bevgen_op_lpips_tap")


def test_the_new_exports_are_declared_and_bound_and_the_abi_is_still_10():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 10 and re.search(r"#define\s+BEVGEN_ABI_VERSION\s+10\b", text) and lib.bevgen_abi_version() == 10
    assert len(_lib.SIGNATURES["bevgen_op_conv3x3_act"][1]) == len(_lib.SIGNATURES["bevgen_op_conv3x3"][1]) + 1


def test_workspace_and_prepared_sizes_are_pure_functions():
    lib = _lib.load()
    ws, prep = lib.bevgen_lpips_workspace_bytes, lib.bevgen_lpips_prepared_bytes
    fp32, f16x3, f16x1 = _lib.PRECISION_FP32, _lib.PRECISION_F16X3, _lib.PRECISION_F16X1
    for bad in ((1, 15, 16, fp32), (1, 16, 15, fp32), (0, 16, 16, fp32), (-3, 64, 64, f16x3), (1, 16, 16, _lib.PRECISION_BF16), (1, 16, 16, 7), (1, 2048, 2048, fp32)):
        assert ws(*bad) == -1, bad
    assert prep(_lib.PRECISION_BF16) == -1 and prep(9) == -1
    # the prepared image: every weight as fp32 [Cout][3][3][max(Cin, 32)] (+ the same bytes again as (hi, lo) planes in the split modes), biases, lin vectors, shift / scale
    weights = sum(co * 9 * max(ci, 32) for co, ci in LR.CONV_SHAPES) * 4
    assert weights <= prep(fp32) < weights + 64 * 1024 and 2 * weights <= prep(f16x3) < 2 * weights + 64 * 1024 and prep(f16x1) == prep(f16x3)
    # the workspace: two activation buffers of 2 m H W 64 floats (three in the split modes) and the partial sums; m = min(n, chunk): four pairs of 256 x 256, 64 of 64 x 64
    for H, W, chunk in ((256, 256, 4), (64, 64, 64), (16, 16, 64), (36, 52, 64), (512, 512, 1), (1024, 1024, 1)):
        sizes = [ws(n, H, W, fp32) for n in (1, chunk, chunk + 1, 8 * chunk + 3)]
        assert sizes[0] > 0 and sizes[1] == sizes[2] == sizes[3] and (chunk == 1 or sizes[0] < sizes[1]), (H, W, sizes)
        act = 2 * chunk * H * W * 64 * 4
        assert 2 * act <= sizes[1] < 2 * act + (1 << 20) and 3 * act <= ws(chunk, H, W, f16x3) < 3 * act + (1 << 20)
        assert ws(5, H, W, f16x3) == ws(5, H, W, f16x1) and ws(5, H, W, fp32) == ws(5, H, W, fp32)


# ================================================================================================ the two-metric output is unchanged without weights
def test_merge_only_command_line_prints_and_saves_what_it_did_before_and_adds_lpips_states_when_present(tmp_path, capsys):
    state = {"gen_psnr": {"sse": 3.0, "count": 150, "min": 0.0, "max": 1.0}, "gen_ssim": {"sum": 1.5, "images": 2},
             "rec_psnr": {"sse": 0.0, "count": 0, "min": float("inf"), "max": float("-inf")}, "rec_ssim": {"sum": 0.0, "images": 0}}
    (tmp_path / "plain.json").write_text(json.dumps(state))
    assert M.main(["--merge", str(tmp_path / "plain.json"), "--save", str(tmp_path / "all.json")]) == 0
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 2 and out[0] == "SSIM Score for dataset is: 0.75" and out[1].startswith("PSNR Score for dataset is: ")
    assert set(json.loads((tmp_path / "all.json").read_text())) == {"gen_psnr", "gen_ssim"}
    # files of a run with --lpips-weights carry gen_lpips / rec_lpips: merged and reported first, as the reference prints it
    for r, (s, t) in enumerate(((0.5, 4), (0.25, 2))):
        (tmp_path / f"metrics_rank{r}.json").write_text(json.dumps(dict(state, gen_lpips={"sum_scores": s, "total": t}, rec_lpips={"sum_scores": 0.0, "total": 0})))
    assert M.main(["--merge", str(tmp_path / "metrics_rank0.json"), str(tmp_path / "metrics_rank1.json"), "--save", str(tmp_path / "all.json")]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "PSIM/LPIPS Score for dataset is: 0.12" and out[1] == "SSIM Score for dataset is: 0.75" and len(out) == 3
    assert json.loads((tmp_path / "all.json").read_text())["gen_lpips"] == {"sum_scores": 0.75, "total": 6}


def test_run_metrics_without_weights_keep_their_four_keys(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert M.METRIC_KEYS == ("gen_psnr", "gen_ssim", "rec_psnr", "rec_ssim") and M.LPIPS_KEYS == ("gen_lpips", "rec_lpips")
    ms = M.make_run_metrics()
    assert set(ms) == set(M.METRIC_KEYS) and set(M.metrics_state(ms)) == set(M.METRIC_KEYS)
    with_lpips = M.make_run_metrics(lpips_weights=LR.make_state())
    assert set(M.metrics_state(with_lpips)) == set(M.METRIC_KEYS) | set(M.LPIPS_KEYS) and M.metrics_state(with_lpips)["rec_lpips"] == {"sum_scores": 0.0, "total": 0}
    assert M.report_metrics(with_lpips) == {"gen_ssim": None, "gen_psnr": None, "rec_ssim": None, "rec_psnr": None}


def test_the_command_lines_take_lpips_weights():
    import inspect

    from bevgen_amd import generate

    assert "--lpips-weights" in inspect.getsource(generate.main) and "--lpips-weights" in inspect.getsource(M.main)
    assert "lpips_weights" in inspect.signature(M.compute_metrics).parameters and inspect.signature(M.compute_metrics).parameters["lpips_weights"].default is None


# ================================================================================================ the restatement itself
def test_the_seeded_weights_behave_as_stated():
    st = LR.make_state()
    a, b = LR.make_pair("independent", (2, 64, 64))
    for t in LR.taps(st, a, torch.float32):
        assert 0.4 < (t > 0).float().mean().item() < 0.6 and 3 < t.max().item() < 13
    assert all(bool((v >= 0).all()) for v in st["lin"])
    total, layers = LR.lpips(st, a, b)
    assert 1.0e-2 < total.mean().item() < 1.5e-2 and 0.7 < (layers[:, 0] / total).mean().item() < 0.85
    a, b = LR.make_pair("near", (2, 64, 64))
    assert 3e-5 < LR.lpips(st, a, b)[0].mean().item() < 8e-5


@pytest.mark.parametrize("shape", LR.CASE_SHAPES)
def test_identical_pairs_give_exactly_zero(shape):
    ref = LR.case_reference("identical", shape)
    assert bool((ref["layers64"] == 0).all()) and bool((ref["total64"] == 0).all()) and bool((ref["e32"] == 0).all())
    t32, l32 = LR.lpips(LR.make_state(), ref["a"], ref["b"], torch.float32)
    assert bool((l32 == 0).all()) and bool((t32 == 0).all())


@pytest.mark.parametrize("shape", LR.CASE_SHAPES)
@pytest.mark.parametrize("kind", ["independent", "near", "uint8"])
def test_case_references_have_a_finite_positive_error_scale(kind, shape):
    ref = LR.case_reference(kind, shape)
    assert ref["layers64"].shape == (shape[0], 5) and bool((ref["layers64"] > 0).all())
    assert bool(torch.isfinite(ref["e32"]).all()) and bool((ref["e32"] > 0).all()) and ref["e32"].max().item() < 1e-3, ref["e32"]


@pytest.mark.parametrize("pixels", LR.TAP_PIXEL_CASES)
@pytest.mark.parametrize("C", LR.TAP_CHANNEL_CASES)
def test_the_fp32_restatement_stays_inside_the_tap_bound(C, pixels):
    fa, fb, w = LR.tap_case(C, pixels)
    x, y = fa.transpose(1, 2), fb.transpose(1, 2)
    d64, bound = LR.tap_bound(x, y, w)
    d32 = LR.tap_distance(x, y, w).double()
    print(f"C={C} pixels={pixels}: fp32 restatement at {((d32 - d64).abs() / bound).max().item():.3f} of the bound, d = {d64.tolist()}")
    assert bool(((d32 - d64).abs() <= bound).all()) and bool((d64 > 0).all())
    if pixels > 2:   # the pixel that is zero in both images contributes exactly 0, the one that is zero in fa alone sum_c w_c fb^_c^2
        one = LR.tap_distance(x[:, :, 2:3], y[:, :, 2:3], w)
        assert bool((one == 0).all()) and bool((LR.tap_distance(x[:, :, 1:2], y[:, :, 1:2], w) > 0).all())
