"""Restatement of LPIPS (VGG16) as bevgen_amd/metrics.py defines it, in plain torch on the CPU (float64 and float32), the seeded weights, the cases and the bounds of the
LPIPS tests (tests/test_lpips_cpu.py, tests/test_lpips_ops_gpu.py, tests/test_lpips_gpu.py).  Not a test file and not part of the product: the product has no CPU path.
Nothing here imports the reference's LPIPS / vgg16 classes (their constructors fetch checkpoints) or torchvision.

Weights (torch CPU Generator, seed WEIGHT_SEED): convolutions N(0, sqrt(2 / (9 Cin))), biases N(0, 0.05), lin vectors 4 U(0, 1) / C.  With them about half of every ReLU
tap is active at every depth (0.46-0.53), the taps' largest values are 6-11 (rms 1.3-1.8), LPIPS is ~1.26e-2 for independent uniform images and ~5.5e-5 for a pair that
differs by noise of sigma 0.02 (checked in tests/test_lpips_cpu.py).  Tap 0 carries ~77 % of the total of an independent pair (~54 % of a near one), so an error in the
deep layers is invisible in the sum: every accuracy test compares the five taps separately, then the total.

Bounds, from the reference arithmetic's own error and the number format, never from what the kernels give:
  end to end   e32_k = the largest |fp32 - fp64| / fp64 of tap k (k = 5: the total) over the images of REALISATIONS seeded input realisations of the case;
               bound = 4 e32_k on an fp32 context (the factor the PSNR / SSIM tests give their e_naive32), 16 e32_k on an f16x3 context (~2^-22 per product, two bits short
               of fp32: four times more)
  tap operator first order in float64 on the operands: TAP_K 2^-24 mean_p sum_c w_c 2 |x^ - y^| (|x^| + |y^|) + 2^-50 d (the double sum); TAP_K = 20 is the rounding count
               stated next to the kernel (csrc/lpips_kernels.hip, LPIPS_TAP_K)
  conv + ReLU  CONV_BOUND = 2e-6 max error / max reference, the project's bound for this kernel in both modes (tests/test_vq_ref_cpu.py); ReLU does not increase an error
  max-pool     bit for bit
"""
import functools

import torch
import torch.nn.functional as F

WEIGHT_SEED = 20
REALISATIONS = 8
TAP_K = 20
CONV_BOUND = 2e-6
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_SHAPES = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512), (512, 512), (512, 512), (512, 512))
POOL_BEFORE = (2, 4, 7, 10)
TAP_AFTER = {1: 0, 3: 1, 6: 2, 9: 3, 12: 4}
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)

# (n, H, W): one relu5_3 pixel; two images, a non-square size; 36 -> 18 -> 9 -> 4 -> 2 and 52 -> 26 -> 13 -> 6 -> 3 (two floors); whole tiles
CASE_SHAPES = [(1, 16, 16), (2, 32, 48), (1, 36, 52), (2, 64, 64)]
CASE_KINDS = ["independent", "near", "identical", "uint8"]


def slice_of(index):
    return 1 if index < 4 else 2 if index < 9 else 3 if index < 16 else 4 if index < 23 else 5


@functools.lru_cache(maxsize=None)
def make_state(seed=WEIGHT_SEED):
    """{'conv_w', 'conv_b', 'lin', 'shift', 'scale'}: the form metrics.load_lpips_state returns"""
    g = torch.Generator().manual_seed(seed)
    st = {"conv_w": [], "conv_b": [], "lin": []}
    for co, ci in CONV_SHAPES:
        st["conv_w"].append(torch.randn((co, ci, 3, 3), generator=g) * (2.0 / (9 * ci)) ** 0.5)
        st["conv_b"].append(torch.randn((co,), generator=g) * 0.05)
    for c in TAP_CHANNELS:
        st["lin"].append(4.0 * torch.rand((c,), generator=g) / c)
    st["shift"], st["scale"] = torch.tensor(SHIFT), torch.tensor(SCALE)
    return st


def reference_state_dict(state=None, spelling="reference", dropout=True, scaling=False):
    """the same tensors under the key spellings load_lpips_state accepts: 'reference' (net.slice{s}.{N}) or 'torchvision' (features.{N}); lin{k}.model.{1 | 0}.weight"""
    state = state or make_state()
    sd = {}
    for idx, w, b in zip(CONV_INDEX, state["conv_w"], state["conv_b"]):
        stem = f"net.slice{slice_of(idx)}.{idx}" if spelling == "reference" else f"features.{idx}"
        sd[stem + ".weight"], sd[stem + ".bias"] = w, b
    for k, v in enumerate(state["lin"]):
        sd[f"lin{k}.model.{1 if dropout else 0}.weight"] = v.reshape(1, -1, 1, 1)
    if scaling:
        sd["scaling_layer.shift"], sd["scaling_layer.scale"] = state["shift"].reshape(1, 3, 1, 1), state["scale"].reshape(1, 3, 1, 1)
    return sd


# ------------------------------------------------------------------------------------------------ the restatement
def as_unit(x):
    """uint8 -> float(v) / 255 in fp32 (one division); fp32 stays"""
    return x.to(torch.float32) / 255.0 if x.dtype == torch.uint8 else x


def taps(state, x, dtype, normalize=False):
    """x [n, 3, H, W] fp32 / uint8 -> the five ReLU taps (NCHW, `dtype`)"""
    x = as_unit(x)
    if normalize:
        x = 2 * x - 1              # (fp32: 2 x is exact, one rounding)
    x = x.to(dtype)
    x = (x - state["shift"].to(dtype)[None, :, None, None]) / state["scale"].to(dtype)[None, :, None, None]
    out = []
    for l in range(13):
        if l in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, state["conv_w"][l].to(dtype), state["conv_b"][l].to(dtype), padding=1))
        if l in TAP_AFTER:
            out.append(x)
    return out


def unit(f):
    return f / (torch.sqrt(torch.sum(f * f, dim=1, keepdim=True)) + 1e-10)


def tap_distance(fa, fb, w):
    """fa, fb [n, C, ...], w [C] -> d [n]: mean over the pixels of sum_c w_c (fa^ - fb^)^2"""
    d = (unit(fa) - unit(fb)) ** 2
    shape = (1, -1) + (1,) * (fa.dim() - 2)
    return (d * w.to(fa.dtype).reshape(shape)).sum(1).flatten(1).mean(1)


def lpips(state, a, b, dtype=torch.float64, normalize=False):
    """-> (total [n], layers [n, 5]) in `dtype`"""
    ta, tb = taps(state, a, dtype, normalize), taps(state, b, dtype, normalize)
    layers = torch.stack([tap_distance(x, y, state["lin"][k]) for k, (x, y) in enumerate(zip(ta, tb))], dim=1)
    total = layers[:, 0]
    for k in range(1, 5):
        total = total + layers[:, k]
    return total, layers


def tap_bound(fa, fb, w, k=TAP_K):
    """first-order bound of the tap operator for fp32 operands fa, fb [n, C, ...] -> (d64 [n], bound [n])"""
    x, y, w64 = unit(fa.double()), unit(fb.double()), w.double()
    shape = (1, -1) + (1,) * (fa.dim() - 2)
    first = (w64.reshape(shape) * 2 * (x - y).abs() * (x.abs() + y.abs())).sum(1).flatten(1).mean(1)
    d64 = tap_distance(fa.double(), fb.double(), w)
    return d64, k * 2.0 ** -24 * first + 2.0 ** -50 * d64


# ------------------------------------------------------------------------------------------------ cases
def make_pair(kind, shape, seed=0):
    n, H, W = shape
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "uint8":
        return torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8), torch.randint(0, 256, (n, 3, H, W), generator=g, dtype=torch.uint8)
    a = torch.rand((n, 3, H, W), generator=g)
    if kind == "independent":
        return a, torch.rand((n, 3, H, W), generator=g)
    if kind == "near":
        return a, (a + 0.02 * torch.randn((n, 3, H, W), generator=g)).clamp(0, 1)
    if kind == "identical":
        return a, a.clone()
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case_reference(kind, shape, normalize=False):
    """The case's inputs (realisation 0), its float64 values and e32.  -> dict(a, b, total64 [n], layers64 [n, 5], e32 [6]: taps 0 .. 4 and the total).
    The realisations run as ONE batch (a convolution's value for an image does not depend on the batch)."""
    n = shape[0]
    pairs = [make_pair(kind, shape, seed) for seed in range(REALISATIONS)]
    a, b = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    state = make_state()
    t64, l64 = lpips(state, a, b, torch.float64, normalize)
    t32, l32 = lpips(state, a, b, torch.float32, normalize)
    v64, v32 = torch.cat([l64, t64[:, None]], dim=1), torch.cat([l32.double(), t32.double()[:, None]], dim=1)
    rel = torch.zeros_like(v64)   # (a value that is exactly 0 in both - the identical pairs - has no error; 0 in float64 alone would be an infinite one)
    rel[v64 != 0] = ((v32 - v64).abs() / v64.abs())[v64 != 0]
    rel[(v64 == 0) & (v32 != 0)] = float("inf")
    return {"a": pairs[0][0], "b": pairs[0][1], "total64": t64[:n], "layers64": l64[:n], "e32": rel.max(dim=0).values}


def tap_case(C, pixels, seed=0, n=2):
    """ReLU-like features [n, pixels, C] (about half active, magnitudes of a few units); fb = fa + noise for image 0, independent for image 1; where there are enough pixels,
    pixel 1 is all zero in fa only and pixel 2 all zero in both.  -> (fa, fb, w)"""
    g = torch.Generator().manual_seed(77 + 13 * C + pixels + seed)
    fa = torch.relu(torch.randn((n, pixels, C), generator=g)) * 6
    fb = torch.relu(torch.randn((n, pixels, C), generator=g)) * 6
    fb[0] = torch.relu(fa[0] + 0.1 * torch.randn((pixels, C), generator=g))
    if pixels > 2:
        fa[:, 1] = 0
        fa[:, 2] = 0
        fb[:, 2] = 0
    return fa, fb, 4.0 * torch.rand((C,), generator=g) / C


TAP_CHANNEL_CASES = [64, 128, 256, 512]
TAP_PIXEL_CASES = [1, 6, 117, 1536]
