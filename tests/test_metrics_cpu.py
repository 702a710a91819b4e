"""PSNR / SSIM without a GPU: the float64 restatement (tests/metrics_ref.py) against closed forms, the metric classes of bevgen_amd/metrics.py on injected states
(merge, load, compute need no device), the directory pairing of `python -m bevgen_amd.metrics`, and the three new exports in the header and the binding."""
import json
import math
import re

import pytest
import torch

import metrics_ref as MR
from bevgen_amd import _lib, metrics as M


# ================================================================================================ the restatement against closed forms
@pytest.mark.parametrize("k", [11, 7])
def test_valid_windows_equal_reflect_pad_and_crop(k):
    p, t = MR.make_pair("smooth_noise", (2, 3, 24, 40))
    valid, padcrop = MR.ssim_map(p, t, k=k), MR.ssim_map_padcrop(p, t, k=k)
    assert valid.shape == padcrop.shape == (2, 3, 24 - k + 1, 40 - k + 1)
    assert (valid - padcrop).abs().max().item() <= 1e-14


def test_ssim_of_an_image_with_itself_is_one():
    _, t = MR.make_pair("uniform", (2, 3, 24, 40))
    assert torch.equal(MR.ssim_map(t, t), torch.ones(2, 3, 14, 30, dtype=torch.float64))


def test_ssim_is_invariant_under_a_common_scaling():
    p, t = MR.make_pair("smooth_noise", (1, 3, 33, 65))
    a, b = MR.ssim_map(p, t, R=1.0), MR.ssim_map(255.0 * p.double(), 255.0 * t.double(), R=255.0)
    assert (a - b).abs().max().item() <= 1e-12


def test_gaussian_window_is_normalised_and_symmetric():
    g = MR.gauss(11, 1.5, torch.float64)
    assert abs(g.sum().item() - 1) < 1e-15 and torch.equal(g, g.flip(0))
    assert abs((g[5] / g[4]).item() - math.exp(0.5 / 1.5 ** 2)) < 1e-14


def test_psnr_of_a_hand_computed_case():
    p, t = torch.tensor([[[[0.0, 0.5], [1.0, 0.25]]]]), torch.tensor([[[[0.0, 1.0], [0.5, 0.25]]]])
    sse = MR.sse64(p, t)
    assert sse.tolist() == [0.5]                                                     # 0 + 1/4 + 1/4 + 0
    assert abs(MR.psnr64(0.5, 4, 1.0).item() - 10 * math.log10(8.0)) < 1e-12     # mse 1/8, R = max - min of the target = 1
    assert abs(MR.psnr64(0.5, 4, 2.0).item() - 10 * math.log10(32.0)) < 1e-12


@pytest.mark.parametrize("shape", MR.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_bright_flat_bound_fails_the_unshifted_formula_and_holds_for_the_centred_one(shape):
    """what makes the bright-flat bound of the GPU tests mean something: the unshifted fp32 restatement is outside it (the map by orders of magnitude), the centred one inside"""
    c = MR.ssim_case("bright_flat", shape)
    b_map, b_mean = MR.ssim_bounds(c, "bright_flat")
    assert c["e_naive_map"] > 100 * b_map and c["e_naive_mean"] > b_mean
    assert c["e_centred_map"] <= b_map and c["e_centred_mean"] <= b_mean
    generic = MR.ssim_case("uniform", shape)
    assert MR.ssim_bounds(generic, "uniform") == (max(4 * generic["e_naive_map"], 2.0 ** -20), max(4 * generic["e_naive_mean"], 2.0 ** -22))


# ================================================================================================ metric classes on injected states
def _psnr_state(p, t):
    return {"sse": MR.sse64(p, t).sum().item(), "count": p.numel(), "min": t.min().item(), "max": t.max().item()}


def _ssim_state(p, t, **kw):
    m = MR.image_means(MR.ssim_map(p, t, **kw))
    return {"sum": m.sum().item(), "images": m.numel()}


def test_merge_of_two_halves_equals_one_pass():
    p, t = MR.make_pair("smooth_noise", (2, 3, 24, 40))
    whole_p, whole_s = M.PeakSignalNoiseRatio().load_state(_psnr_state(p, t)), M.StructuralSimilarityIndexMeasure().load_state(_ssim_state(p, t))
    half_p, half_s = M.PeakSignalNoiseRatio().load_state(_psnr_state(p[:1], t[:1])), M.StructuralSimilarityIndexMeasure().load_state(_ssim_state(p[:1], t[:1]))
    other_p = M.PeakSignalNoiseRatio().load_state(_psnr_state(p[1:], t[1:]))
    half_p.merge_state(other_p)                        # an object ...
    half_s.merge_state(_ssim_state(p[1:], t[1:]))      # ... or its dict
    assert abs(half_p.compute().item() - whole_p.compute().item()) < 1e-12
    assert abs(half_s.compute().item() - whole_s.compute().item()) < 1e-15
    assert half_p.state()["count"] == p.numel() and half_s.state()["images"] == 2
    want = MR.psnr64(MR.sse64(p, t).sum(), p.numel(), (t.max() - t.min()).double())
    assert abs(whole_p.compute().item() - want.item()) < 1e-12
    assert whole_p.compute().dtype == torch.float64 and whole_s.compute().dtype == torch.float64


def test_psnr_without_a_data_range_uses_the_extremes_of_all_merged_targets():
    a = M.PeakSignalNoiseRatio().load_state({"sse": 2.0, "count": 100, "min": 0.25, "max": 0.5})
    a.merge_state({"sse": 1.0, "count": 50, "min": 0.125, "max": 0.375})
    assert a.state() == {"sse": 3.0, "count": 150, "min": 0.125, "max": 0.5}
    assert abs(a.compute().item() - 10 * math.log10(0.375 ** 2 / (3.0 / 150))) < 1e-12
    fixed = M.PeakSignalNoiseRatio(data_range=1.0).load_state(a.state())
    assert abs(fixed.compute().item() - 10 * math.log10(1.0 / (3.0 / 150))) < 1e-12


def test_state_survives_json():
    a = M.StructuralSimilarityIndexMeasure().load_state({"sum": 1.2345678901234567, "images": 3})
    b = M.StructuralSimilarityIndexMeasure().load_state(json.loads(json.dumps(a.state())))
    assert b.compute().item() == a.compute().item() == 1.2345678901234567 / 3
    empty = M.PeakSignalNoiseRatio()
    assert json.loads(json.dumps(empty.state())) == {"sse": 0.0, "count": 0, "min": float("inf"), "max": float("-inf")}
    a.reset()
    assert a.state() == {"sum": 0.0, "images": 0}


@pytest.mark.parametrize("cls", [M.PeakSignalNoiseRatio, M.StructuralSimilarityIndexMeasure])
def test_compute_on_an_empty_metric_raises(cls):
    with pytest.raises(RuntimeError, match="before any update"):
        cls().compute()


def test_constructor_arguments():
    s = M.StructuralSimilarityIndexMeasure(data_range=1.0)
    assert (s.data_range, s.kernel_size, s.sigma, s.k1, s.k2) == (1.0, 11, 1.5, 0.01, 0.03)
    assert M.PeakSignalNoiseRatio().data_range is None
    with pytest.raises(ValueError):
        M.StructuralSimilarityIndexMeasure(kernel_size=10)


@pytest.mark.parametrize("cls", [M.PeakSignalNoiseRatio, M.StructuralSimilarityIndexMeasure])
def test_update_without_a_gpu_raises_the_no_cpu_path_error(cls, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    p, t = MR.make_pair("uniform", (1, 1, 11, 11))
    with pytest.raises(RuntimeError, match="no CPU path in the product"):
        cls().update(p, t)
    with pytest.raises(RuntimeError, match="no CPU path in the product"):
        cls()(p, t)


def test_mismatched_inputs_are_refused_before_any_device_is_needed():
    p, t = MR.make_pair("uniform", (1, 1, 11, 11))
    m = M.PeakSignalNoiseRatio()
    with pytest.raises(ValueError):
        m.update(p, t[..., :10])
    with pytest.raises(ValueError):
        m.update(p, (t * 255).to(torch.uint8))
    with pytest.raises(ValueError):
        m.update(p.double(), t.double())


def test_accumulate_metrics_without_ground_truth_counts_nothing(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ms = M.make_run_metrics()
    assert M.accumulate_metrics(ms, {"gen": torch.zeros(1, 3, 3, 16, 16), "rec": None, "gt": None}) == 0
    assert set(M.metrics_state(ms)) == set(M.METRIC_KEYS) and M.metrics_state(ms)["gen_ssim"] == {"sum": 0.0, "images": 0}
    assert M.report_metrics(ms) == {"gen_ssim": None, "gen_psnr": None, "rec_ssim": None, "rec_psnr": None}


# ================================================================================================ directory pairing
def _touch(root, rels):
    for r in rels:
        p = root / r
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")


def test_pair_paths_is_a_pure_function_of_two_lists():
    both, dropped = M.pair_paths(["b/1.jpg", "a/1.jpg", "a/2.jpg"], ["a/2.jpg", "b/1.jpg", "c/9.jpg", "c/8.jpg"])
    assert both == ["a/2.jpg", "b/1.jpg"] and dropped == 2       # the larger tree has 4
    assert M.pair_paths([], []) == ([], 0)
    assert M.pair_paths(["x.jpg"], ["x.jpg"]) == (["x.jpg"], 0)


def test_directory_pairing_gen_rec_and_argoverse(tmp_path):
    _touch(tmp_path / "gt", ["s0/cam_a.jpg", "s0/cam_b.jpg", "s1/cam_a.jpg", "s1/notes.txt"])
    _touch(tmp_path / "gen", ["s0/cam_a.jpg", "s0/cam_b.jpg", "s1/cam_a.jpg"])
    _touch(tmp_path / "rec", ["s0/cam_a.jpg", "s1/cam_a.jpg", "s2/cam_a.jpg", "s3/cam_a.jpg"])
    gt_tree, other, rel, dropped = M.directory_pairs(str(tmp_path))
    assert (gt_tree, other) == (str(tmp_path / "gt"), str(tmp_path / "gen"))
    assert rel == ["s0/cam_a.jpg", "s0/cam_b.jpg", "s1/cam_a.jpg"] and dropped == 0
    _, other, rel, dropped = M.directory_pairs(str(tmp_path), rec=True)
    assert other == str(tmp_path / "rec") and rel == ["s0/cam_a.jpg", "s1/cam_a.jpg"] and dropped == 2
    _touch(tmp_path / "sample_gt", ["tok0/ring_front_center.jpg", "tok1/ring_front_center.jpg"])
    _touch(tmp_path / "sample", ["tok1/ring_front_center.jpg", "tok1/bev.npz"])
    gt_tree, other, rel, dropped = M.directory_pairs(str(tmp_path), argoverse=True)
    assert (gt_tree, other) == (str(tmp_path / "sample_gt"), str(tmp_path / "sample"))
    assert rel == ["tok1/ring_front_center.jpg"] and dropped == 1
    assert M.tree_names(False, False) == ("gt", "gen") and M.tree_names(False, True) == ("gt", "rec") and M.tree_names(True, True) == ("sample_gt", "sample")


def test_merge_only_command_line(tmp_path, capsys):
    state = {"gen_psnr": {"sse": 3.0, "count": 150, "min": 0.0, "max": 1.0}, "gen_ssim": {"sum": 1.5, "images": 2},
             "rec_psnr": {"sse": 0.0, "count": 0, "min": float("inf"), "max": float("-inf")}, "rec_ssim": {"sum": 0.0, "images": 0}}
    for r in (0, 1):
        (tmp_path / f"metrics_rank{r}.json").write_text(json.dumps(state))
    rc = M.main(["--merge", str(tmp_path / "metrics_rank0.json"), str(tmp_path / "metrics_rank1.json"), "--save", str(tmp_path / "all.json")])
    assert rc == 0
    out = capsys.readouterr().out.splitlines()
    assert out == ["SSIM Score for dataset is: 0.75", "PSNR Score for dataset is: %.2f" % (10 * math.log10(1 / (6.0 / 300)))]
    assert json.loads((tmp_path / "all.json").read_text())["gen_ssim"] == {"sum": 3.0, "images": 4}


# ================================================================================================ header and binding
def test_the_three_exports_are_declared_and_bound_and_the_abi_is_still_10():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in ("bevgen_op_image_sqerr", "bevgen_op_ssim", "bevgen_metrics_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 10 and re.search(r"#define\s+BEVGEN_ABI_VERSION\s+10\b", text)
    assert len(_lib.SIGNATURES["bevgen_op_image_sqerr"][1]) == 12 and len(_lib.SIGNATURES["bevgen_op_ssim"][1]) == 17


def test_workspace_size_is_a_pure_function_of_the_shapes():
    lib = _lib.load()
    f = lib.bevgen_metrics_workspace_bytes
    # squared error: ceil(count / 2048) workgroups per image (at most 128), one double and two floats each
    assert f(0, 2, 1, 1, 1, 0) == 2 * 16 and f(0, 1, 3, 64, 64, 0) == 6 * 16 and f(0, 96, 3, 256, 256, 0) == 96 * 96 * 16 and f(0, 1, 3, 1024, 1024, 0) == 128 * 16
    # ssim: one double per (plane, 32 x 32 tile of the map); 16-row tiles from kernel_size 23 on
    assert f(1, 1, 1, 11, 11, 11) == 8 and f(1, 2, 3, 12, 75, 11) == 2 * 3 * 1 * 3 * 8 and f(1, 1, 3, 33, 65, 11) == 3 * 1 * 2 * 8 and f(1, 2, 3, 64, 64, 11) == 2 * 3 * 2 * 2 * 8
    assert f(1, 96, 3, 256, 256, 11) == 96 * 3 * 8 * 8 * 8 and f(1, 1, 1, 64, 64, 33) == 2 * 8
    for bad in ((1, 1, 1, 10, 11, 11), (1, 1, 1, 11, 10, 11), (1, 1, 1, 40, 40, 10), (1, 1, 1, 40, 40, 35), (1, 0, 3, 16, 16, 11), (0, 1, 0, 16, 16, 0), (2, 1, 1, 16, 16, 11)):
        assert f(*bad) == -1, bad
