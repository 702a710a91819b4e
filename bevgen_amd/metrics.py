"""PSNR, SSIM and LPIPS of generated / reconstructed views against ground truth, where the pixels already are (reference scripts/metrics_eval.py:29-132).

``PeakSignalNoiseRatio`` and ``StructuralSimilarityIndexMeasure`` take the constructor arguments ``metrics_eval.compute_metrics`` gives torchmetrics' classes of the
same names; ``compute_metrics(pairs)`` is that function, ``python -m bevgen_amd.metrics DIR`` its directory form.  The sums run in libbevgen_hip's kernels
(csrc/metrics.hip: ``Context.op_image_sqerr`` / ``Context.op_ssim``), fp32 or uint8 images, reduced in a fixed order; the states are small device tensors and
``compute()`` is float64 torch arithmetic on them.  ``update`` needs the GPU - there is no CPU path in the product - while ``load_state`` / ``merge_state`` /
``compute`` work on saved states anywhere (merging the ``metrics_rank<r>.json`` files of a multi-GPU run).

The contract is this definition, not a third-party implementation:
  PSNR  10 log10(R^2 / (sse / count)), sse = sum (preds - target)^2 and count = number of elements over everything seen, R = data_range, or with data_range=None
        max - min of every TARGET seen.
  SSIM  mean over images of the mean of that image's map ((2 mx my + c1)(2 sxy + c2)) / ((mx^2 + my^2 + c1)(sxx + syy + c2)), c1 = (k1 R)^2, c2 = (k2 R)^2, moments under
        a normalised Gaussian window (kernel_size, sigma) over the VALID window positions - which equals reflect-padding by (kernel_size - 1) / 2, filtering and cropping
        the pad - no clamp.
That is what metrics_eval.py asks for through its constructor arguments.  torchmetrics' own arithmetic is not part of the reference tree and the package is not installed
where this library is built, so parity with torchmetrics is UNPINNED ("Evaluation").

  LPIPS ``LearnedPerceptualImagePatchSimilarity(net_type='vgg')``: the reference's modules/losses/lpips.py (41-54, 57-64, 116-122) in eval mode - (x - shift) / scale, the
        thirteen 3x3 convolution + ReLU layers of VGG16 features[0:30] with their four 2x2 max-pools, and at relu1_2 .. relu5_3
        d_k = mean_{h,w} sum_c lin_k[c] (fa^ - fb^)^2, f^ = f / (sqrt(sum_c f^2) + 1e-10); LPIPS = sum_k d_k per image pair (``Context.lpips``, csrc/lpips.cpp).
        The network is a fixed description; its weights are an ordinary state_dict the user of the reference has on disk (``load_lpips_state``), like the VQGAN and
        stage-2 checkpoints.  Inputs are [0, 1] images with normalize=False, as metrics_eval.py feeds them.  torchmetrics' host-side check that the inputs lie in the
        expected range (scripts/lpip.py:40-43, 136) would need a synchronising device-to-host min / max per update and is NOT reproduced.  Parity with the `lpips` /
        torchmetrics packages is unpinned like the other two.
FID needs an Inception network plus a matrix square root and stays out of scope.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Any, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import torch


def _planes(t: torch.Tensor, name: str) -> torch.Tensor:
    """[n, C, H, W] or [B, cams, C, H, W] -> [n, C, H, W]"""
    if t.dim() == 5:
        t = t.reshape(-1, *t.shape[2:])
    if t.dim() != 4:
        raise ValueError(f"{name}: images are [n, C, H, W] or [B, cams, C, H, W], got {tuple(t.shape)}")
    return t


class _Metric:
    """States are tensors (on the context's device once update() has run); state() / load_state() move them through plain Python numbers (JSON)."""
    _STATES: Tuple[Tuple[str, torch.dtype, float], ...] = ()

    def __init__(self, ctx=None):
        self._ctx, self._own_ctx = ctx, False
        self.reset()

    # ---- context: made on first use, so that a metric that only merges and computes never needs a GPU
    def context(self):
        if self._ctx is None:
            from .runtime import Context

            self._ctx, self._own_ctx = Context(None), True   # (raises "no CPU path in the product" without a GPU)
        return self._ctx

    def close(self):
        if self._own_ctx and self._ctx is not None:
            self._ctx.close()
        self._ctx, self._own_ctx = None, False

    def reset(self):
        dev = self._ctx.device if self._ctx is not None else torch.device("cpu")
        for name, dtype, init in self._STATES:
            setattr(self, name, torch.tensor(init, dtype=dtype, device=dev))

    def _pair(self, preds, target):
        if not isinstance(preds, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise TypeError("preds and target are tensors")
        if preds.shape != target.shape or preds.dtype != target.dtype:
            raise ValueError(f"preds {tuple(preds.shape)} {preds.dtype} and target {tuple(target.shape)} {target.dtype} differ in shape or dtype")
        if preds.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"images are float32 in [0, 1] or uint8, got {preds.dtype}")
        ctx = self.context()
        a, b = _planes(preds.detach(), "preds").to(ctx.device).contiguous(), _planes(target.detach(), "target").to(ctx.device).contiguous()
        self._to(ctx.device)
        return ctx, a, b

    def _to(self, device):
        for name, _, _ in self._STATES:
            setattr(self, name, getattr(self, name).to(device))

    def __call__(self, preds, target):
        """update(), and the value of this batch alone"""
        one = self._fresh()
        one._ctx = self.context()
        one.update(preds, target)
        self._to(one._ctx.device)
        self.merge_state(one)
        return one.compute()

    def state(self) -> Dict[str, Any]:
        return {name: getattr(self, name).item() for name, _, _ in self._STATES}

    def load_state(self, d: Mapping[str, Any]):
        dev = getattr(self, self._STATES[0][0]).device
        for name, dtype, _ in self._STATES:
            setattr(self, name, torch.tensor(d[name], dtype=dtype, device=dev))
        return self

    def merge_state(self, other):
        d = other if isinstance(other, Mapping) else {name: getattr(other, name) for name, _, _ in other._STATES}
        for name, dtype, _ in self._STATES:
            mine = getattr(self, name)
            theirs = torch.as_tensor(d[name], dtype=dtype).to(mine.device)
            setattr(self, name, torch.minimum(mine, theirs) if name == "min" else torch.maximum(mine, theirs) if name == "max" else mine + theirs)
        return self


# ---- LPIPS weights ----------------------------------------------------------------------------------------------------------------------------------------------------
LPIPS_CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # torchvision's vgg16().features indices of the thirteen convolutions
LPIPS_CONV_SHAPES = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512), (512, 512), (512, 512), (512, 512))
LPIPS_TAP_CHANNELS = (64, 128, 256, 512, 512)
LPIPS_SHIFT, LPIPS_SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
LPIPS_WEIGHT_FILES = ("vgg.pth (the lin layers, taming's vgg_lpips checkpoint)", "the VGG16 features state_dict (torchvision's vgg16, IMAGENET1K_V1)")


def _lpips_slice(index: int) -> int:
    return 1 if index < 4 else 2 if index < 9 else 3 if index < 16 else 4 if index < 23 else 5


def load_lpips_state(*sources) -> Dict[str, Any]:
    """Merges state dicts (mappings, or paths given to torch.load) into {'conv_w': 13 x [Cout, Cin, 3, 3], 'conv_b': 13 x [Cout], 'lin': 5 x [C_k], 'shift': [3],
    'scale': [3]} (float32, CPU).  Three key spellings are accepted: the reference's (net.slice{1..5}.{N}.{weight,bias}, lin{k}.model.1.weight, optional
    scaling_layer.{shift,scale}), torchvision's features.{N}.{weight,bias} for the same N, and lin{k}.model.0.weight (a NetLinLayer built without dropout).  Every shape
    is checked and whatever is missing is named."""
    merged: Dict[str, Any] = {}
    for src in sources:
        if not isinstance(src, Mapping):
            src = torch.load(src, map_location="cpu")
        if isinstance(src, Mapping) and "state_dict" in src and isinstance(src["state_dict"], Mapping):
            src = src["state_dict"]
        merged.update(src)

    def pick(names):
        for nm in names:
            if nm in merged:
                return nm, torch.as_tensor(merged[nm]).detach().to("cpu", torch.float32)
        return None, None

    missing: List[str] = []
    out: Dict[str, Any] = {"conv_w": [], "conv_b": [], "lin": []}
    for idx, (co, ci) in zip(LPIPS_CONV_INDEX, LPIPS_CONV_SHAPES):
        for kind, shape, dst in (("weight", (co, ci, 3, 3), "conv_w"), ("bias", (co,), "conv_b")):
            names = (f"net.slice{_lpips_slice(idx)}.{idx}.{kind}", f"features.{idx}.{kind}")
            nm, t = pick(names)
            if t is None:
                missing.append(" or ".join(names))
                continue
            if tuple(t.shape) != shape:
                raise ValueError(f"load_lpips_state: {nm} has shape {tuple(t.shape)}, VGG16 needs {shape}")
            out[dst].append(t.contiguous())
    for k, c in enumerate(LPIPS_TAP_CHANNELS):
        names = (f"lin{k}.model.1.weight", f"lin{k}.model.0.weight")
        nm, t = pick(names)
        if t is None:
            missing.append(" or ".join(names))
            continue
        if t.numel() != c or tuple(t.shape) not in ((1, c, 1, 1), (c,), (1, c)):
            raise ValueError(f"load_lpips_state: {nm} has shape {tuple(t.shape)}, lin{k} needs (1, {c}, 1, 1)")
        out["lin"].append(t.reshape(c).contiguous())
    if missing:
        raise ValueError("load_lpips_state: missing " + "; ".join(missing) + " - LPIPS needs " + " and ".join(LPIPS_WEIGHT_FILES))
    for key, default in (("shift", LPIPS_SHIFT), ("scale", LPIPS_SCALE)):
        nm, t = pick((f"scaling_layer.{key}",))
        if t is None:
            t = torch.tensor(default, dtype=torch.float32)
        if t.numel() != 3:
            raise ValueError(f"load_lpips_state: {nm} has shape {tuple(t.shape)}, the scaling layer has 3 channels")
        out[key] = t.reshape(3).contiguous()
    return out


class PeakSignalNoiseRatio(_Metric):
    """10 log10(R^2 / mse) over everything seen; R = data_range, or (None) max - min of the targets seen."""
    _STATES = (("sse", torch.float64, 0.0), ("count", torch.int64, 0), ("min", torch.float32, float("inf")), ("max", torch.float32, float("-inf")))

    def __init__(self, data_range: Optional[float] = None, ctx=None):
        self.data_range = None if data_range is None else float(data_range)
        super().__init__(ctx)

    def _fresh(self):
        return PeakSignalNoiseRatio(self.data_range)

    def update(self, preds, target):
        ctx, a, b = self._pair(preds, target)
        minmax = torch.stack([self.min, self.max])
        sse, minmax = ctx.op_image_sqerr(a, b, minmax)
        total = sse.sum()
        self.sse = self.sse + (total / 65025.0 if a.dtype == torch.uint8 else total)   # (uint8 sums are exact integers in units of 1 / 255^2)
        self.count = self.count + a.numel()
        self.min, self.max = minmax[0], minmax[1]

    def compute(self) -> torch.Tensor:
        if int(self.count.item()) == 0:
            raise RuntimeError("PeakSignalNoiseRatio.compute() before any update()")
        R = torch.tensor(self.data_range, dtype=torch.float64, device=self.sse.device) if self.data_range is not None else self.max.double() - self.min.double()
        return 10.0 * torch.log10(R * R / (self.sse / self.count.double()))


class StructuralSimilarityIndexMeasure(_Metric):
    """mean over images of each image's SSIM-map mean (torchmetrics' reduction='elementwise_mean')."""
    _STATES = (("sum", torch.float64, 0.0), ("images", torch.int64, 0))

    def __init__(self, data_range: float = 1.0, kernel_size: int = 11, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03, ctx=None):
        if int(kernel_size) % 2 == 0 or int(kernel_size) < 1:
            raise ValueError(f"kernel_size is odd, got {kernel_size}")
        self.data_range, self.kernel_size, self.sigma, self.k1, self.k2 = float(data_range), int(kernel_size), float(sigma), float(k1), float(k2)
        super().__init__(ctx)

    def _fresh(self):
        return StructuralSimilarityIndexMeasure(self.data_range, self.kernel_size, self.sigma, self.k1, self.k2)

    def update(self, preds, target):
        ctx, a, b = self._pair(preds, target)
        n, C, H, W = a.shape
        sums = ctx.op_ssim(a, b, self.kernel_size, self.sigma, self.data_range, self.k1, self.k2)
        per_map = C * (H - self.kernel_size + 1) * (W - self.kernel_size + 1)
        self.sum = self.sum + (sums / per_map).sum()
        self.images = self.images + n

    def compute(self) -> torch.Tensor:
        if int(self.images.item()) == 0:
            raise RuntimeError("StructuralSimilarityIndexMeasure.compute() before any update()")
        return self.sum / self.images.double()


class LearnedPerceptualImagePatchSimilarity(_Metric):
    """LPIPS (VGG16) of preds against target: mean / sum over every image pair seen, or (reduction='none') the per-image scores of the last update - what
    filter_generated.py reads.  weights: what load_lpips_state takes (a path, a state dict, or a sequence of them) or its result.  Without `ctx` the metric makes its own
    context with precision='f16x3' (the drop-in modules' default); a passed context is used as it is.  The input range is not checked (module docstring)."""
    _STATES = (("sum_scores", torch.float64, 0.0), ("total", torch.int64, 0))

    def __init__(self, net_type: str = "vgg", reduction: str = "mean", normalize: bool = False, weights=None, ctx=None):
        if net_type != "vgg":
            raise NotImplementedError(f"net_type {net_type!r}: only the VGG16 LPIPS ('vgg'), the one the reference uses, is implemented")
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
        if weights is None:
            raise ValueError("LearnedPerceptualImagePatchSimilarity needs weights=: " + " and ".join(LPIPS_WEIGHT_FILES))
        if isinstance(weights, Mapping) and "conv_w" in weights:
            self.weights = weights
        else:
            self.weights = load_lpips_state(*(weights if isinstance(weights, (list, tuple)) else (weights,)))
        self.net_type, self.reduction, self.normalize = net_type, reduction, bool(normalize)
        self._prepared, self._prepared_for, self.last_scores = None, None, None
        super().__init__(ctx)

    def context(self):
        if self._ctx is None:
            from .runtime import Context

            self._ctx, self._own_ctx = Context(None, precision="f16x3"), True   # (raises "no CPU path in the product" without a GPU)
        return self._ctx

    def _fresh(self):
        one = LearnedPerceptualImagePatchSimilarity(self.net_type, self.reduction, self.normalize, self.weights)
        one._prepared, one._prepared_for = self._prepared, self._prepared_for
        return one

    def _ensure_prepared(self, ctx):
        """the weights in the form this context's kernels read, made once per context"""
        if self._prepared is None or self._prepared_for is not ctx:
            self._prepared, self._prepared_for = ctx.lpips_prepare(self.weights), ctx
        return self._prepared

    def __call__(self, preds, target):
        self._ensure_prepared(self.context())   # (so that the one-batch metric of _Metric.__call__ shares them)
        return super().__call__(preds, target)

    def update(self, preds, target):
        ctx, a, b = self._pair(preds, target)
        scores = ctx.lpips(self._ensure_prepared(ctx), a, b, normalize=self.normalize)
        self.last_scores = scores
        self.sum_scores = self.sum_scores + scores.sum()
        self.total = self.total + scores.numel()

    def merge_state(self, other):
        super().merge_state(other)
        if isinstance(other, LearnedPerceptualImagePatchSimilarity) and other.last_scores is not None:
            self.last_scores = other.last_scores
        return self

    def compute(self) -> torch.Tensor:
        if int(self.total.item()) == 0:
            raise RuntimeError("LearnedPerceptualImagePatchSimilarity.compute() before any update()")
        if self.reduction == "none":
            if self.last_scores is None:
                raise RuntimeError("reduction='none' returns the last update's per-image scores; a merged or loaded state has none")
            return self.last_scores
        return self.sum_scores / self.total.double() if self.reduction == "mean" else self.sum_scores


def _report(ssim_value: float, psnr_value: float, label: str = "", lpips_value: Optional[float] = None) -> None:
    if lpips_value is not None:
        print(f"{label}PSIM/LPIPS Score for dataset is: {lpips_value:.2f}")
    print(f"{label}SSIM Score for dataset is: {ssim_value:.2f}")
    print(f"{label}PSNR Score for dataset is: {psnr_value:.2f}")


def compute_metrics(pairs: Iterable, ctx=None, lpips_weights=None) -> Dict[str, float]:
    """metrics_eval.compute_metrics: `pairs` yields (gt, gen) batches; prints the reference's lines and returns {'ssim', 'psnr'}.  With lpips_weights (what
    LearnedPerceptualImagePatchSimilarity takes as weights=) the "PSIM/LPIPS" line comes first, as in the reference, and the result also holds 'lpips'; without them
    the output and the result are the two-metric ones."""
    psnr, ssim = PeakSignalNoiseRatio(ctx=ctx), StructuralSimilarityIndexMeasure(data_range=1.0, ctx=ctx)
    lp = LearnedPerceptualImagePatchSimilarity(weights=lpips_weights, ctx=ctx) if lpips_weights is not None else None
    if ctx is None:
        ssim._ctx = psnr.context()
    for gt, gen in pairs:
        if lp is not None:
            lp.update(gen, gt)
        ssim.update(gen, gt)
        psnr.update(gen, gt)
    out = {"ssim": float(ssim.compute().item()), "psnr": float(psnr.compute().item())}
    if lp is not None:
        out["lpips"] = float(lp.compute().item())
        lp.close()
    psnr.close()
    _report(out["ssim"], out["psnr"], lpips_value=out.get("lpips"))
    return out


# ---- generate.py --metrics --------------------------------------------------------------------------------------------------------------------------------------------
METRIC_KEYS = ("gen_psnr", "gen_ssim", "rec_psnr", "rec_ssim")
LPIPS_KEYS = ("gen_lpips", "rec_lpips")   # present only in a run with --lpips-weights


def make_run_metrics(ctx=None, lpips_weights=None) -> Dict[str, _Metric]:
    """the four states a generate run accumulates: gen-vs-gt and rec-vs-gt, on ONE context; with lpips_weights also LPIPS_KEYS (their two metrics share one context
    of their own, precision f16x3, unless `ctx` is given)"""
    first = PeakSignalNoiseRatio(ctx=ctx)
    out: Dict[str, _Metric] = {"gen_psnr": first, "gen_ssim": StructuralSimilarityIndexMeasure(ctx=ctx), "rec_psnr": PeakSignalNoiseRatio(ctx=ctx),
                               "rec_ssim": StructuralSimilarityIndexMeasure(ctx=ctx)}
    if ctx is None and torch.cuda.is_available():
        shared = first.context()
        for m in out.values():
            m._ctx = shared
    if lpips_weights is not None:
        state = lpips_weights if isinstance(lpips_weights, Mapping) and "conv_w" in lpips_weights else load_lpips_state(
            *(lpips_weights if isinstance(lpips_weights, (list, tuple)) else (lpips_weights,)))
        gen = LearnedPerceptualImagePatchSimilarity(weights=state, ctx=ctx)
        rec = LearnedPerceptualImagePatchSimilarity(weights=state, ctx=ctx)
        if ctx is None and torch.cuda.is_available():
            rec._ctx = gen.context()
        out["gen_lpips"], out["rec_lpips"] = gen, rec
    return out


def accumulate_metrics(metrics: Mapping[str, _Metric], outputs: Mapping[str, Any]) -> int:
    """One forward's {'gen', 'rec', 'gt'} (float [B, cams, 3, H, W] in [0, 1], on the device) into `metrics`; a batch without 'gt' counts nothing, one without
    'rec' only gen.  -> number of images counted against gt."""
    gt = outputs.get("gt")
    if gt is None:
        return 0
    for split in ("gen", "rec"):
        x = outputs.get(split)
        if x is not None:
            metrics[f"{split}_psnr"].update(x, gt)
            metrics[f"{split}_ssim"].update(x, gt)
            if f"{split}_lpips" in metrics:
                metrics[f"{split}_lpips"].update(x, gt)
    return _planes(gt, "gt").shape[0]


def metrics_state(metrics: Mapping[str, _Metric]) -> Dict[str, Dict[str, Any]]:
    return {k: metrics[k].state() for k in METRIC_KEYS + tuple(k for k in LPIPS_KEYS if k in metrics)}


def report_metrics(metrics: Mapping[str, _Metric]) -> Dict[str, Optional[float]]:
    """prints the reference's lines for gen (and rec where it was seen) -> the values (None for a split without images)"""
    out: Dict[str, Optional[float]] = {}
    for split in ("gen", "rec"):
        p, s = metrics[f"{split}_psnr"], metrics[f"{split}_ssim"]
        if int(s.images.item()) == 0:
            out[f"{split}_ssim"] = out[f"{split}_psnr"] = None
            continue
        out[f"{split}_ssim"], out[f"{split}_psnr"] = float(s.compute().item()), float(p.compute().item())
        lp = metrics.get(f"{split}_lpips")
        if lp is not None:
            out[f"{split}_lpips"] = float(lp.compute().item())
        _report(out[f"{split}_ssim"], out[f"{split}_psnr"], label=f"[{split}] ", lpips_value=out.get(f"{split}_lpips"))
    return out


# ---- directory form (metrics_eval.py:29-111) ---------------------------------------------------------------------------------------------------------------------------
def tree_names(argoverse: bool, rec: bool) -> Tuple[str, str]:
    """(ground-truth tree, compared tree) under the dataset directory"""
    return ("sample_gt", "sample") if argoverse else ("gt", "rec" if rec else "gen")


def pair_paths(gt_rel: Sequence[str], other_rel: Sequence[str]) -> Tuple[List[str], int]:
    """Relative paths of the two trees -> (sorted intersection, number dropped = the larger tree's size - the intersection's, the reference's 'Removed at least')."""
    a, b = set(map(str, gt_rel)), set(map(str, other_rel))
    both = sorted(a & b)
    return both, max(len(a), len(b)) - len(both)


def list_jpgs(root: str) -> List[str]:
    out = []
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".jpg"):
                out.append(os.path.relpath(os.path.join(d, f), root))
    return sorted(out)


def directory_pairs(dataset_dir: str, argoverse: bool = False, rec: bool = False) -> Tuple[str, str, List[str], int]:
    gt_tree, other_tree = (os.path.join(dataset_dir, t) for t in tree_names(argoverse, rec))
    rel, dropped = pair_paths(list_jpgs(gt_tree), list_jpgs(other_tree))
    return gt_tree, other_tree, rel, dropped


def _load_u8(path: str) -> torch.Tensor:
    import numpy as np
    from PIL import Image

    a = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(a.copy()).permute(2, 0, 1)


def evaluate_directory(dataset_dir: str, argoverse: bool = False, rec: bool = False, batch_size: int = 20, ctx=None, lpips=None):
    """PIL decode on the host, uint8 upload, the uint8 kernels; images of one size are batched.  -> (psnr, ssim); `lpips` (a LearnedPerceptualImagePatchSimilarity)
    is updated with the same batches."""
    gt_tree, other_tree, rel, dropped = directory_pairs(dataset_dir, argoverse, rec)
    if dropped:
        print(f"Removed at least {dropped}")
    print(f"Total of {len(rel)} samples")
    psnr, ssim = PeakSignalNoiseRatio(ctx=ctx), StructuralSimilarityIndexMeasure(data_range=1.0, ctx=ctx)
    ssim._ctx = psnr.context()
    gts: List[torch.Tensor] = []
    others: List[torch.Tensor] = []

    def flush():
        if gts:
            g, o = torch.stack(gts), torch.stack(others)
            if lpips is not None:
                lpips.update(o, g)
            ssim.update(o, g)
            psnr.update(o, g)
            gts.clear()
            others.clear()

    for r in rel:
        g, o = _load_u8(os.path.join(gt_tree, r)), _load_u8(os.path.join(other_tree, r))
        if gts and (g.shape != gts[0].shape or len(gts) >= batch_size):
            flush()
        gts.append(g)
        others.append(o)
    flush()
    return psnr, ssim


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m bevgen_amd.metrics", description="PSNR / SSIM (and, with --lpips-weights, LPIPS) of a generated tree against its ground truth "
                                 "(metrics_eval.py without FID)")
    ap.add_argument("dataset_dir", nargs="?", default=None, help="directory holding gt/ and gen/ (rec/), or with --argoverse sample_gt/ and sample/")
    ap.add_argument("--argoverse", action="store_true")
    ap.add_argument("--rec", action="store_true", help="compare rec/ instead of gen/")
    ap.add_argument("--merge", nargs="*", default=[], metavar="STATE.json", help="metrics_rank<r>.json files of a generate --metrics run (or files written by --save) to add")
    ap.add_argument("--save", default=None, metavar="STATE.json", help="write the merged states here")
    ap.add_argument("--lpips-weights", nargs="+", default=None, metavar="FILE", help="state dict file(s) holding the VGG16 features and the LPIPS lin layers: also report PSIM/LPIPS")
    args = ap.parse_args(argv)
    if args.dataset_dir is None and not args.merge:
        ap.error("pass a dataset directory, --merge files, or both")
    split = "rec" if args.rec else "gen"
    lp = LearnedPerceptualImagePatchSimilarity(weights=list(args.lpips_weights)) if args.lpips_weights else None
    if args.dataset_dir is not None:
        psnr, ssim = evaluate_directory(args.dataset_dir, args.argoverse, args.rec, lpips=lp)
    else:
        psnr, ssim = PeakSignalNoiseRatio(), StructuralSimilarityIndexMeasure(data_range=1.0)
    lp_state: Optional[Dict[str, Any]] = lp.state() if lp is not None else None   # (--merge adds LPIPS states where the files carry them, with or without weights here)
    for path in args.merge:
        with open(path) as f:
            d = json.load(f)
        psnr.merge_state(d[f"{split}_psnr"])
        ssim.merge_state(d[f"{split}_ssim"])
        if f"{split}_lpips" in d:
            theirs = d[f"{split}_lpips"]
            lp_state = dict(theirs) if lp_state is None else {"sum_scores": lp_state["sum_scores"] + theirs["sum_scores"], "total": lp_state["total"] + theirs["total"]}
    lp_value = lp_state["sum_scores"] / lp_state["total"] if lp_state is not None and lp_state["total"] > 0 else None
    _report(float(ssim.compute().item()), float(psnr.compute().item()), lpips_value=lp_value)
    if args.save:
        saved = {f"{split}_psnr": psnr.state(), f"{split}_ssim": ssim.state()}
        if lp_state is not None:
            saved[f"{split}_lpips"] = lp_state
        with open(args.save, "w") as f:
            json.dump(saved, f)
    if lp is not None:
        lp.close()
    psnr.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
