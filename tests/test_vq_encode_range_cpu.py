"""precision='f16x3r' on the VQGAN ENCODER (include/bevgen_hip.h bevgen_cfg.vq_range): the checkpoints, the fp64 reference and the input builders that
tests/test_vq_encode_range_gpu.py runs on the GPU, checked here without one.

cases.VQ_TINY_HEAVY does not overflow any encoder operand (its residual stream passes 65504 only behind the last site that reads it), so the two recipes below scale one
more tensor of that checkpoint:
    R1  encoder.down.2.block.0.nin_shortcut.{weight, bias} x 8        the stream in front of down.2's downsample passes 65504
    R3  encoder.down.1.block.1.conv2.{weight, bias} x 512             four sites pass 32768, the largest by a factor 2^7
both on golden("vq_tiny")["enc_img_x"][:2].  The reference is an fp64 restatement of the encoder from oracle.restate's blocks that records the absmax of every site operand
(conv_in, every nin_shortcut and downsample convolution in execution order, quant_conv).

Measured here (fp64; site order conv_in, down0, down1, nin of down.2.block.0, down2, nin of down.3.block.0, quant_conv):
    R1  3.78  140  238     165     1.004e5  1.695e4  41      exponents 0 0 0 0 2 0 0      rows with relative margin < 1e-4: 3.1 %
    R3  3.78  140  6.04e4  4.40e4  2.63e6   5.14e5   38      exponents 0 0 1 1 7 4 0      rows with relative margin < 1e-4: 2.3 %
The closest a site comes to a boundary 32768 2^j is R3's last nin_shortcut, 1.9 % below 2^19; fp32 ids equal the fp64 ids on all 128 rows of either recipe.
"""
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import cases
from oracle import restate as R
from test_vq_ref_cpu import _gen, down_case, down_ref

# ------------------------------------------------------------------------------------------------ the recipes (the GPU file imports everything below)
RECIPES = {"R1": ("encoder.down.2.block.0.nin_shortcut", 8.0), "R3": ("encoder.down.1.block.1.conv2", 512.0)}
SITE_NAMES = ("conv_in", "down.0.downsample", "down.1.downsample", "down.2.block.0.nin_shortcut", "down.2.downsample", "down.3.block.0.nin_shortcut", "quant_conv")
WANT_EXPONENTS = {"R1": [0, 0, 0, 0, 2, 0, 0], "R3": [0, 0, 1, 1, 7, 4, 0]}
MARGIN = 1e-4            # relative margin (d2 - d1) / max |d| below which a row's id is not compared: vq_tiny has min relative margin 1.13e-4 and is exact in both modes
MAX_EXCLUDED = 0.05
BOUNDARY_CLEARANCE = 0.01

_CACHE = {}


def recipe_sd(name):
    """The VQ_TINY_HEAVY state dict with one convolution (weight and bias) scaled; built once and left unchanged."""
    if ("sd", name) not in _CACHE:
        v = cases.VQ_TINY_HEAVY
        sd = cases.heavy_tail(cases.vq_state_dict(v["dd"], v["n_embed"], v["embed_dim"], v["seed"], with_encoder=True), v["heavy"])
        key, fac = RECIPES[name]
        for suffix in (".weight", ".bias"):
            sd[key + suffix] = sd[key + suffix] * fac
        _CACHE["sd", name] = sd
    return _CACHE["sd", name]


def recipe_x():
    return torch.from_numpy(golden("vq_tiny")["enc_img_x"][:2])


def want_exponent(absmax: float) -> int:
    """0 where absmax < 32768, else the smallest e with absmax 2^-e < 32768 (the rule at bevgen_cfg.vq_range)."""
    e = 0
    while absmax * 2.0 ** -e >= 32768.0:
        e += 1
    return e


def encode_with_sites(sd, dd, x, dtype=torch.float64):
    """Encoder.forward + quant_conv + the quantizer's distances (oracle.restate.vq_encoder / vq_encode_ids, restated block by block) in `dtype`.
    Returns (ids [n, h w], d [n h w, n_embed], sites): sites = [(name, absmax of the operand)] for every place where an un-normalised tensor is a convolution's input."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = x.to(dtype)
    sites = []

    def site(name, t):
        sites.append((name, float(t.abs().max())))

    def res(p, h):
        if ("encoder." + p + "nin_shortcut.weight") in sd:
            site(p + "nin_shortcut", h)
        return R._resnet(sd, "encoder." + p, h)

    nres = len(dd["ch_mult"])
    site("conv_in", x)
    h = F.conv2d(x, sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"], padding=1)
    for lvl in range(nres):
        for b in range(dd["num_res_blocks"]):
            h = res(f"down.{lvl}.block.{b}.", h)
            if f"encoder.down.{lvl}.attn.{b}.norm.weight" in sd:
                h = R._attn_block(sd, f"encoder.down.{lvl}.attn.{b}.", h)
        if lvl != nres - 1:
            site(f"down.{lvl}.downsample", h)
            h = F.conv2d(F.pad(h, (0, 1, 0, 1), mode="constant", value=0), sd[f"encoder.down.{lvl}.downsample.conv.weight"], sd[f"encoder.down.{lvl}.downsample.conv.bias"], stride=2)
    h = res("mid.block_1.", h)
    h = R._attn_block(sd, "encoder.mid.attn_1.", h)
    h = res("mid.block_2.", h)
    h = R._gn_swish(h, sd["encoder.norm_out.weight"], sd["encoder.norm_out.bias"])
    h = F.conv2d(h, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"], padding=1)
    site("quant_conv", h)
    h = F.conv2d(h, sd["quant_conv.weight"], sd["quant_conv.bias"])
    zf = h.permute(0, 2, 3, 1).reshape(-1, h.shape[1])
    E = sd["quantize.embedding.weight"]
    d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(E ** 2, dim=1) - 2 * torch.einsum("bd,dn->bn", zf, E.t())
    return torch.argmin(d, dim=1).view(x.shape[0], -1), d, sites


def relative_margins(d):
    """Per row: (second smallest - smallest distance) / max |d| over the whole distance matrix."""
    top2 = d.topk(2, dim=1, largest=False).values
    return (top2[:, 1] - top2[:, 0]) / d.abs().max()


def recipe_ref(name):
    """fp64 reference of a recipe, computed once: dict(ids [2, 64], margins [128], keep [2, 64] = rows whose id is compared, sites, exponents)."""
    if ("ref", name) not in _CACHE:
        dd = cases.VQ_TINY_HEAVY["dd"]
        ids, d, sites = encode_with_sites(recipe_sd(name), dd, recipe_x())
        m = relative_margins(d)
        _CACHE["ref", name] = dict(ids=ids, d=d, margins=m, keep=(m >= MARGIN).view(ids.shape), sites=sites, exponents=[want_exponent(a) for _, a in sites])
    return _CACHE["ref", name]


# ------------------------------------------------------------------------------------------------ op_conv_ranged: inputs and fp64 references
CONV_KINDS = (0, 1, 2)                                   # 1x1, 3x3 stride 1, the Downsample
CONV_N = (1, 2)
CONV_HW = ((2, 2), (6, 8))
CONV_C = (32, 64)
CONV_SCALES = (1.0, 4e4, 1e5, 1e30)


def conv_case(kind, n, H, W, Cin, Cout, absmax):
    """kind 2: test_vq_ref_cpu.down_case; kinds 0 / 1: the same construction with a 1x1 / 3x3 kernel of unit output variance.  x is then scaled to the given absmax
    (in fp32: the reference reads the scaled fp32 tensor)."""
    if kind == 2:
        x, w, b = down_case(n, H, W, Cin, Cout)
    else:
        k = 1 if kind == 0 else 3
        g = _gen(8, kind, n, H, W, Cin, Cout)
        x = torch.randn(n, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(k * k * Cin)
        b = torch.randn(Cout, generator=g)
    x = x * (absmax / x.abs().max().item())
    return x, w, b


def conv_ref(kind, x, w, b):
    if kind == 2:
        return down_ref(x, w, b)
    return F.conv2d(x.double(), w.double(), b.double(), padding=0 if kind == 0 else 1)


# ================================================================================================ the recipes against the conditions the GPU tests rest on
@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_reference_and_conditions(name):
    v = cases.VQ_TINY_HEAVY
    sd, x, ref = recipe_sd(name), recipe_x(), recipe_ref(name)
    # the restatement with sites is the oracle's encoder
    sd64 = {k: (t.double() if t.is_floating_point() else t) for k, t in sd.items()}
    assert torch.equal(ref["ids"], R.vq_encode_ids(sd64, v["dd"], x.double()))
    assert tuple(s for s, _ in ref["sites"]) == SITE_NAMES
    absmax = [a for _, a in ref["sites"]]
    print(name, "site absmax", [f"{a:.4g}" for a in absmax], "exponents", ref["exponents"])
    # the recipe leaves the f16 operand range, and no site sits where fp32 rounding of the GPU's tensor could move the exponent
    assert max(absmax) >= 65520.0
    for a in absmax:
        for j in range(0, 12):
            edge = 32768.0 * 2.0 ** j
            assert abs(a - edge) > BOUNDARY_CLEARANCE * edge, (a, edge)
    assert ref["exponents"] == WANT_EXPONENTS[name]
    # fp32 stays finite and agrees on the ids; few rows are near-ties
    ids32, d32, sites32 = encode_with_sites(sd, v["dd"], x, torch.float32)
    assert torch.isfinite(d32).all() and all(math.isfinite(a) for _, a in sites32)
    assert torch.equal(ids32, ref["ids"]), f"{(ids32 != ref['ids']).sum().item()} of {ids32.numel()} fp32 ids differ from fp64"
    excluded = 1 - ref["keep"].double().mean().item()
    print(name, f"rows with relative margin < {MARGIN:g}: {100 * excluded:.1f} %, min margin {ref['margins'].min().item():.3e}")
    assert excluded <= MAX_EXCLUDED


def test_heavy_fixture_itself_overflows_no_encoder_operand():
    """Why the recipes exist: on VQ_TINY_HEAVY every site operand stays inside the f16 range."""
    v = cases.VQ_TINY_HEAVY
    sd = cases.heavy_tail(cases.vq_state_dict(v["dd"], v["n_embed"], v["embed_dim"], v["seed"], with_encoder=True), v["heavy"])
    _, _, sites = encode_with_sites(sd, v["dd"], recipe_x())
    assert max(a for _, a in sites) < 32768.0


def test_want_exponent_rule():
    assert [want_exponent(a) for a in (0.0, 1.0, 32767.9, 32768.0, 65519.0, 65536.0, 1e30)] == [0, 0, 0, 1, 1, 2, 85]


@pytest.mark.parametrize("kind", CONV_KINDS)
def test_conv_case_reaches_its_absmax_and_the_reference_scales(kind):
    for absmax in CONV_SCALES:
        x, w, b = conv_case(kind, 2, 6, 8, 32, 64, absmax)
        assert abs(x.abs().max().item() / absmax - 1) < 1e-6
        ref = conv_ref(kind, x, w, b)
        assert ref.shape == ((2, 64, 3, 4) if kind == 2 else (2, 64, 6, 8)) and torch.isfinite(ref.float()).all()
    # linear in x up to the bias: the large cases are the unit case scaled
    x1, w, b = conv_case(kind, 2, 6, 8, 32, 64, 1.0)
    zero = torch.zeros_like(b)
    big, one = conv_ref(kind, x1.double() * 2.0 ** 20, w, zero), conv_ref(kind, x1, w, zero)
    assert torch.equal(big, one * 2.0 ** 20)            # (a power of two: exact)


# ================================================================================================ plumbing
def test_abi_and_binding():
    from bevgen_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"#define\s+BEVGEN_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == 10
    assert "bevgen_op_conv_ranged" in _lib.SIGNATURES and len(_lib.SIGNATURES["bevgen_op_conv_ranged"][1]) == 13
    assert re.search(r"\bint\s+bevgen_op_conv_ranged\s*\(", header)
    assert ctypes.sizeof(_lib.bevgen_cfg) == 4 * (3 + 5 + 3 + 3 + 3 + 2 + 8 + 8 + 1 + 16)
