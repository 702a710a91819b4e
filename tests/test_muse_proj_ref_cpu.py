"""Route M's projections with fused epilogues (bevgen_amd/csrc/gemm_split_glds.hip: EPI_MUSE_Q / _KV / _QKV, EPI_GEGLU, the folded LayerNorm) and the kernels that feed
them (LayerNorm to planes, the q / k / v preparation kernels, the weight preparations): case tables, input builders and fp64 references of tests/test_muse_proj_ops_gpu.py,
checked here without a GPU.

* The references restate stage2/muse_maskgit_pytorch.py:71-88 (GEGLU, FeedForward) and :132-146 (q, k, v of Attention.forward) in fp64 and are compared with an
  independent fp32 formulation of the same lines.
* The precision floor: the f16x3 mode emulated in plain torch - both operands split into (f16 hi, f16((v - hi) 2048)), three fp32 products, the epilogue in fp32, the result
  split again - against fp64.  It says what the FORMAT can deliver, which is what the GPU bound must leave room for; no project code is involved.
* The launch plan: every GPU case's launches go through tests/host/gemm_plan_dump.cpp (built as tests/test_gemm_plan_cpu.py builds it) and must land on the variant the
  case was chosen for, so that a later change of the launcher's rules cannot silently move a case off its block shape.

Bounds (metric: max |out - ref| / max |ref| per output tensor, against fp64):
  FLAT_BOUND = 2e-6, the bound this kernel's product is already held to (test_gemm_split_precision, test_gemm_plan_variants_run): 3 .. 7 x the emulation floors asserted
  below (< 1e-6), more than 100 x below the error of a lost low plane (> 1e-4, asserted below).
  The offset case (GEGLU rows with mean / std near 2): OFFSET_FACTOR = 4 x the emulation floor of that exact input - the fold computes rstd (acc - mean cs) and cancels;
  4 is the ratio of the flat bound to the emulation's ~5e-7 on the plain product."""
import math
import os
import subprocess
import zlib
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

FLAT_BOUND = 2e-6
OFFSET_FACTOR = 4.0
LN_PLANES_BOUND = 1e-5          # the bound of test_layernorm (tests/test_ops_gpu.py)
POST = 8.0 * 1.4426950408889634  # the score scale the model folds into q (muse.cpp q_args): 8 log2(e)
SENTINEL_BITS = 0x5B3D           # a finite f16 (-> 231.625) no case produces in every element of a region

# ================================================================================================ case tables
# Variants are written [MODE, WM, S, KS, TI, TJ] as gemm_plan_dump prints them; `plan` = the launches (first row, end row, variant) of the case's (first) GEMM.
QkvCase = namedtuple("QkvCase", "name kind B T H K ld block form ksplit plan")
T64, T8W, T2S, T32x32, T256 = (0, 1, 4, 0, 1, 2), (0, 2, 4, 0, 1, 2), (0, 2, 2, 0, 2, 2), (0, 1, 4, 0, 1, 1), (0, 4, 3, 0, 2, 2)
QKV_CASES = [
    # query preparation
    QkvCase("q-a", "q", 2, 48, 3, 192, 0, 0, 0, 1, [(0, 96, T64)]),            # the fold models' shape; N = 192 leaves the last tile's second wave without columns
    QkvCase("q-b", "q", 3, 100, 4, 64, 0, 0, 0, 1, [(0, 300, T64)]),           # ragged M = 300; patches straddle batch elements
    QkvCase("q-c", "q", 7, 300, 16, 64, 0, 0, 0, 1, [(0, 2100, T8W)]),         # eight-wave 32 x 64 patches
    QkvCase("q-d", "q", 14, 300, 16, 64, 0, 0, 0, 1, [(0, 4200, T2S)]),        # two-stage block: direct forms only
    QkvCase("q-e1", "q", 2, 320, 3, 64, 0, 4, 0, 1, [(0, 640, T256)]),         # staged 64 x 64; whole waves past M
    QkvCase("q-e2", "q", 3, 100, 3, 64, 0, 4, 0, 1, [(0, 300, T256)]),
    QkvCase("q-u", "q", 3, 100, 4, 192, 0, 0, 1, 2, [(0, 300, (0, 2, 4, 1, 1, 2))]),   # split-K + muse_q_prep_split
    # key / value preparation
    QkvCase("kv-a", "kv", 2, 48, 3, 192, 64, 0, 0, 1, [(0, 96, T64)]),         # T % 32 != 0: direct transposed values, staged keys
    QkvCase("kv-b", "kv", 2, 96, 2, 64, 104, 0, 0, 1, [(0, 192, T64)]),        # staged transposed values on 32-row patches
    QkvCase("kv-c", "kv", 2, 320, 3, 64, 328, 4, 0, 1, [(0, 640, T256)]),      # staged values: patches with nk0 = 0 (rows 0 and 320) and nk0 != 0, the last-token lane
    QkvCase("kv-d", "kv", 2, 320, 3, 64, 327, 4, 0, 1, [(0, 640, T256)]),      # ld % 8 != 0: direct values beside staged keys
    QkvCase("kv-e", "kv", 8, 288, 8, 64, 296, 0, 0, 1, [(0, 2304, T8W)]),      # eight-wave block, staged
    QkvCase("kv-f", "kv", 14, 300, 8, 64, 304, 0, 0, 1, [(0, 4200, T2S)]),     # no staging at all
    QkvCase("kv-g", "kv", 9, 1024, 8, 64, 1032, 0, 0, 1, [(0, 8192, T256), (8192, 9216, T64)]),   # row split: the second launch has m_base != 0
    QkvCase("kv-u", "kv", 3, 100, 3, 64, 104, 0, 1, 1, [(0, 300, T32x32)]),    # plain projection + muse_kv_prep_split
    # merged q | k | v
    QkvCase("qkv-a", "qkv", 2, 320, 3, 64, 328, 4, 0, 1, [(0, 640, T256)]),    # column tile 1 holds a query head in wave 0 and a key head in wave 1
    QkvCase("qkv-b1", "qkv", 3, 100, 3, 64, 104, 0, 0, 1, [(0, 300, T64)]),    # ragged
    QkvCase("qkv-b2", "qkv", 2, 48, 3, 192, 64, 0, 0, 1, [(0, 96, T64)]),      # the fold models' shape
]
QKV = {c.name: c for c in QKV_CASES}
# (case, weights, ln_gamma): every case as it is, four of them also with the f16-rounded weight (two products) and single-product forms, two with the LayerNorm kernel in front
QKV_RUNS = [(c.name, 0, False) for c in QKV_CASES] + [(n, wt, False) for n in ("q-b", "q-e1", "q-e2", "kv-c", "qkv-a") for wt in (1, 2)] + [("q-b", 0, True), ("kv-c", 0, True)]
RANGE_CASES = ["kv-c", "kv-d"]
STAGED_VS_DIRECT_QKV = ["q-e1", "q-e2", "kv-c", "kv-d", "qkv-a"]

# feed-forward chain: (M, D, F, Dout, block) -> the variants of the up-projection (GEGLU) and of the down-projection
FfCase = namedtuple("FfCase", "name M D F Dout block up down")
FF_CASES = [
    FfCase("ff-fold", 96, 192, 512, 192, 0, [(0, 96, T64)], [(0, 96, T32x32)]),                 # the fold models' shape
    FfCase("ff-ragged", 300, 64, 341, 192, 0, [(0, 300, T64)], [(0, 300, T32x32)]),             # ragged M, Fpad = 384; down-projection on 32 x 32 patches
    FfCase("ff-staged", 640, 64, 341, 192, 4, [(0, 640, T256)], [(0, 640, T256)]),              # staged producer forms, consumer on 256-row blocks
    FfCase("ff-8w", 3000, 64, 341, 192, 0, [(0, 3000, T8W)], [(0, 3000, T32x32)]),              # producer on eight waves of 32 x 64 patches
    FfCase("ff-2s", 4200, 64, 341, 1024, 0, [(0, 4200, T8W)], [(0, 4200, T2S)]),                # consumer and (level 2) producer on the two-stage block
]
FF = {c.name: c for c in FF_CASES}
FF_FORMS = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)]   # (level, merge)
OFFSET_CASE = FfCase("ff-offset", 300, 64, 341, 192, 0, [(0, 300, T64)], [(0, 300, T32x32)])
OFFSET_SHIFT = 4.5   # common offset of the `a` and `gate` columns of the offset case (see ff_inputs)

LN_PLANES_SHAPES = [(5, 128, 128), (37, 1024, 1024), (9, 341, 384), (130, 2730, 2752), (3, 192, 192)]   # (rows, D, ldy): fast path = D % 256 == 0 and ldy == D
GEGLU_LN_SHAPES = [(9, 341, 384), (130, 2730, 2752)]


def fpad(F_):
    return (F_ + 63) // 64 * 64


# ================================================================================================ helpers
def seed_of(name, extra=0):
    return zlib.crc32(name.encode()) % (2 ** 31) + extra


def rel(out, ref):
    """max |out - ref| / max |ref|"""
    return float((out.double() - ref.double()).abs().max() / ref.double().abs().max())


def planes_to_float(hi, lo):
    """value of an (hi, lo) f16 plane pair, in fp64"""
    return hi.double() + lo.double() * 2.0 ** -11


def decode_plane_image(img, rows, ld):
    """interleaved plane image [rows][ld / 32][hi 32 | lo 32] (f16) -> (hi, lo) as [rows, ld] f16 tensors"""
    v = img.reshape(rows, ld // 32, 2, 32)
    return v[:, :, 0, :].reshape(rows, ld), v[:, :, 1, :].reshape(rows, ld)


def l2norm64(t):
    return t / t.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def round_f16(t):
    return t.half().float()


# ================================================================================================ q / k / v: inputs and fp64 reference
def qkv_inputs(c, ln=False):
    """a ~ 3 N(0, 1), w ~ N(0, 1) / sqrt(K), scales ~ 1 + 0.3 N(0, 1), null_kv ~ N(0, 1) (the existing GEMM tests' distributions)"""
    g = torch.Generator().manual_seed(seed_of(c.name))
    n_out = 64 * c.H * {"q": 1, "kv": 2, "qkv": 3}[c.kind]
    p = {"a": torch.randn(c.B * c.T, c.K, generator=g) * 3.0, "w": torch.randn(n_out, c.K, generator=g) / math.sqrt(c.K),
         "q_scale": 1.0 + 0.3 * torch.randn(64, generator=g), "k_scale": 1.0 + 0.3 * torch.randn(64, generator=g), "null_kv": torch.randn(2, c.H, 64, generator=g)}
    p["ln_gamma"] = 1.0 + 0.3 * torch.randn(c.K, generator=g) if ln else None
    return p


def qkv_operands(p, weights):
    """the operands as the mode rounds them: weights >= 1 the matrix rounded to f16, weights == 2 also the activation (its hi plane alone is multiplied)"""
    a, w = p["a"], p["w"]
    if weights >= 1:
        w = round_f16(w)
    if weights == 2:
        a = round_f16(a)
    return a, w


def null_ref(p):
    """the prepared null key / value [H, 64] (launch_muse_null_kv_prep): l2norm(null_k) * k_scale, null_v"""
    nk, nv = p["null_kv"][0].double(), p["null_kv"][1].double()
    return l2norm64(nk) * p["k_scale"].double(), nv


def qkv_ref(c, p, weights=0, post=POST):
    """fp64 restatement of muse_maskgit_pytorch.py:132-146 in the kernels' output layout, positions [0, T] only:
    Q [B, H, T, 64] = l2norm(8 x) * q_scale * post; K [B, H, T + 1, 64] = l2norm(k) * k_scale at row 1 + token, the prepared null key at row 0;
    VT [B, H, 64, T + 1] = v transposed at column 1 + token, the null value at column 0."""
    a, w = qkv_operands(p, weights)
    x = a.double()
    if p["ln_gamma"] is not None:
        x = F.layer_norm(x, (c.K,), p["ln_gamma"].double(), None, 1e-5)
    proj = x @ w.double().t()
    HD = 64 * c.H
    heads = lambda t: t.reshape(c.B, c.T, c.H, 64).permute(0, 2, 1, 3)   # [B T, H 64] -> [B, H, T, 64]
    out, col = {}, 0
    if c.kind in ("q", "qkv"):
        out["Q"] = l2norm64(heads(proj[:, :HD]) * 8.0) * p["q_scale"].double() * post
        col = HD
    if c.kind in ("kv", "qkv"):
        nk, nv = null_ref(p)
        k = l2norm64(heads(proj[:, col:col + HD])) * p["k_scale"].double()
        v = heads(proj[:, col + HD:col + 2 * HD])
        out["K"] = torch.cat([nk.reshape(1, c.H, 1, 64).expand(c.B, -1, -1, -1), k], dim=2)
        out["VT"] = torch.cat([nv.reshape(1, c.H, 1, 64).expand(c.B, -1, -1, -1), v], dim=2).transpose(2, 3).contiguous()
    return out


def qkv_alt_fp32(c, p, post=POST):
    """the same lines in fp32 as the reference module writes them: Linear, chunk, rearrange, cat of the null kv, F.normalize - one formulation for every head at once"""
    x = p["a"]
    if p["ln_gamma"] is not None:
        x = F.layer_norm(x, (c.K,), p["ln_gamma"], torch.zeros(c.K), 1e-5)
    x = x.reshape(c.B, c.T, c.K)
    HD = 64 * c.H
    parts = F.linear(x, p["w"]).split(HD, dim=-1)
    to_heads = lambda t: t.reshape(c.B, c.T, c.H, 64).transpose(1, 2)
    out = {}
    if c.kind in ("q", "qkv"):
        q = to_heads(parts[0] * 8)
        out["Q"] = F.normalize(q, dim=-1) * p["q_scale"] * post
    if c.kind in ("kv", "qkv"):
        k, v = (to_heads(t) for t in parts[-2:])
        nk, nv = (t.reshape(1, c.H, 1, 64).repeat(c.B, 1, 1, 1) for t in p["null_kv"])
        out["K"] = F.normalize(torch.cat((nk, k), dim=-2), dim=-1) * p["k_scale"]
        out["VT"] = torch.cat((nv, v), dim=-2).transpose(-1, -2)
    return out


def range_inputs(c, where):
    """kv inputs whose token `where` (a row of a) is aligned with one value row of w so that this token's value column leaves the f16 range (|v| = 8e4 > 65504) while every
    element of a stays inside it.  Returns (p, row)."""
    p = qkv_inputs(c)
    row = where
    wv = p["w"][64 * c.H + 5].double()   # value column 5 of head 0
    p["a"][row] = (8.0e4 * wv / (wv @ wv)).float()
    return p, row


# ================================================================================================ feed-forward: inputs and fp64 reference
def ff_inputs(c, offset=0.0):
    """x ~ 3 N(0, 1), w ~ N(0, 1) / sqrt(K), gamma ~ 1 + 0.3 N(0, 1), residual ~ N(0, 1).  offset != 0: x gets a constant first column (1) and w1's first column the offset, so
    that every `a` and `gate` value is raised by the same positive amount and the GEGLU rows get a mean well away from 0."""
    g = torch.Generator().manual_seed(seed_of(c.name))
    x = torch.randn(c.M, c.D, generator=g) * 3.0
    w1 = torch.randn(2 * c.F, c.D, generator=g) / math.sqrt(c.D)
    if offset:
        x[:, 0] = 1.0
        w1[:, 0] = offset
        x[:, 1:] *= 1.5 / 3.0 * math.sqrt(c.D / (c.D - 1.0))   # the raw rows at std 1.5
    return {"x": x, "w1": w1, "gamma3": 1.0 + 0.3 * torch.randn(c.F, generator=g), "w4": torch.randn(c.Dout, c.F, generator=g) / math.sqrt(c.F),
            "residual": torch.randn(c.M, c.Dout, generator=g)}


def group_sums(t, ld):
    """(sum, sum of squares) per (32 columns, row) of t [M, n <= ld] zero-padded to ld columns, as [ld / 32][M][2]"""
    M = t.shape[0]
    pad = torch.zeros(M, ld, dtype=t.dtype)
    pad[:, :t.shape[1]] = t
    v = pad.reshape(M, ld // 32, 32)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], dim=-1).transpose(0, 1).contiguous()


def ff_ref(c, p):
    """fp64 restatement of muse_maskgit_pytorch.py:71-88 behind the first LayerNorm: h = gate * gelu(a) with (a | gate) = x W1^T, y = LN_gamma(h) W4^T + R, plus what the folded
    forms leave on the way: h zero-padded to Fpad columns, its per-group (sum, sum of squares), (mean, rstd) per row, and the group sums of y."""
    Fp = fpad(c.F)
    proj = p["x"].double() @ p["w1"].double().t()
    a, gate = proj[:, :c.F], proj[:, c.F:]
    h = gate * (0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0))))
    mean = h.mean(-1)
    var = (h * h).mean(-1) - mean * mean
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    y = ((h - mean[:, None]) * rstd[:, None] * p["gamma3"].double()) @ p["w4"].double().t() + p["residual"].double()
    hp = torch.zeros(c.M, Fp, dtype=torch.float64)
    hp[:, :c.F] = h
    return {"h": hp, "g_sums": group_sums(h, Fp), "rowstat": torch.stack([mean, rstd], dim=-1), "y": y, "y_sums": group_sums(y, c.Dout)}


def ff_alt_fp32(p):
    """the same lines in fp32 as the reference module writes them"""
    c_f = p["gamma3"].numel()
    a, gate = F.linear(p["x"], p["w1"]).chunk(2, dim=-1)
    h = gate * F.gelu(a)
    return h, F.linear(F.layer_norm(h, (c_f,), p["gamma3"], torch.zeros(c_f)), p["w4"]) + p["residual"]


def ln_planes_inputs(rows, D, ldx, beta, geglu=False):
    g = torch.Generator().manual_seed(rows * 7919 + D)
    x = torch.randn(rows, ldx, generator=g) * 2.0 + 0.5
    return x, 1.0 + 0.3 * torch.randn(D, generator=g), (0.3 * torch.randn(D, generator=g) if beta else None)


def ln_planes_ref(x, gamma, beta, D, geglu=False):
    xd = x.double()
    if geglu:
        a, gate = xd[:, :D], xd[:, D:2 * D]
        xd = gate * (0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0))))
    return F.layer_norm(xd[:, :D], (D,), gamma.double(), None if beta is None else beta.double(), 1e-5)


# ================================================================================================ the precision floor: the mode in plain torch
def em_split(v):
    """(f16 hi, f16((v - hi) 2048)) of an fp32 tensor, both back in fp32"""
    hi = v.half().float()
    return hi, ((v - hi) * 2048.0).half().float()


def em_join(hi, lo):
    return hi + lo * (1.0 / 2048.0)


def em_product(ah, al, bh, bl):
    """three fp32 products: Ah Bh^T + 2^-11 (Ah Bl^T + Al Bh^T)"""
    return ah @ bh.t() + (ah @ bl.t() + al @ bh.t()) * (1.0 / 2048.0)


def em_ff(c, p):
    """the folded feed-forward chain (levels 1 / 2) emulated in fp32 on emulated planes; statistics merged in fp64 from fp32 group sums, as the kernels do"""
    Fp = fpad(c.F)
    proj = em_product(*em_split(p["x"]), *em_split(p["w1"]))
    a, gate = proj[:, :c.F], proj[:, c.F:]
    h = torch.zeros(c.M, Fp)
    h[:, :c.F] = gate * F.gelu(a)
    hh, hl = em_split(h)
    gs = group_sums(h, Fp)
    mean = gs[..., 0].double().sum(0) / c.F
    var = (gs[..., 1].double().sum(0) / c.F - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    w4g = torch.zeros(c.Dout, Fp)
    w4g[:, :c.F] = p["w4"] * p["gamma3"]
    cs = w4g.double().sum(1).float()
    acc = em_product(hh, hl, *em_split(w4g))
    y = rstd.float()[:, None] * (acc - mean.float()[:, None] * cs) + p["residual"]
    return {"h": em_join(hh, hl), "g_sums": gs, "rowstat": torch.stack([mean, rstd], dim=-1).float(), "y": y, "y_planes": em_join(*em_split(y)), "y_sums": group_sums(y, c.Dout)}


def ff_errors(c, out, ref):
    """per-output errors of a feed-forward result dict (the keys of ff_ref plus y_planes) against the fp64 reference; sums and sums of squares, mean and rstd separately"""
    e = {}
    for k in out:
        r = ref["y"] if k == "y_planes" else ref[k]
        if k in ("g_sums", "y_sums", "rowstat"):
            e[k + ".0"], e[k + ".1"] = rel(out[k][..., 0], r[..., 0]), rel(out[k][..., 1], r[..., 1])
        else:
            e[k] = rel(out[k], r)
    return e


_offset_cache = {}


def offset_case():
    """(inputs, fp64 reference, per-output bound) of the offset case: OFFSET_FACTOR x the emulation floor where the fold's cancellation enters (y, its planes and sums, the
    row statistics), the flat bound elsewhere."""
    if not _offset_cache:
        p = ff_inputs(OFFSET_CASE, OFFSET_SHIFT)
        ref = ff_ref(OFFSET_CASE, p)
        floor = ff_errors(OFFSET_CASE, em_ff(OFFSET_CASE, p), ref)
        bound = {k: (max(FLAT_BOUND, OFFSET_FACTOR * v) if k.startswith(("y", "rowstat")) else FLAT_BOUND) for k, v in floor.items()}
        _offset_cache.update(p=p, ref=ref, floor=floor, bound=bound)
    return _offset_cache["p"], _offset_cache["ref"], _offset_cache["bound"]


# ================================================================================================ tests: references against an independent fp32 formulation
@pytest.mark.parametrize("name,ln", [("q-a", False), ("q-b", True), ("kv-a", False), ("kv-u", True), ("qkv-b1", False), ("qkv-b2", True)])
def test_qkv_reference_against_fp32_formulation(name, ln):
    c = QKV[name]
    p = qkv_inputs(c, ln)
    ref, alt = qkv_ref(c, p), qkv_alt_fp32(c, p)
    assert set(ref) == set(alt) == {"q": {"Q"}, "kv": {"K", "VT"}, "qkv": {"Q", "K", "VT"}}[c.kind]
    for k in ref:
        assert ref[k].shape == alt[k].shape, k
        assert rel(alt[k], ref[k]) < 1e-5, (k, rel(alt[k], ref[k]))   # fp32 evaluation of K <= 192 deep products and a normalisation
    if "K" in ref:   # the layout statements the kernels are held to: null row / column first, token t at 1 + t
        nk, nv = null_ref(p)
        assert torch.equal(ref["K"][1, :, 0], nk) and torch.equal(ref["VT"][1, :, :, 0], nv)
        assert ref["K"].shape == (c.B, c.H, c.T + 1, 64) and ref["VT"].shape == (c.B, c.H, 64, c.T + 1)


def test_epi_post_is_a_plain_factor():
    c = QKV["q-a"]
    p = qkv_inputs(c)
    assert rel(qkv_ref(c, p, post=POST)["Q"], qkv_ref(c, p, post=1.0)["Q"] * POST) < 1e-15
    assert abs(POST - 11.5415603) < 1e-6


@pytest.mark.parametrize("name", ["ff-fold", "ff-ragged"])
def test_ff_reference_against_fp32_formulation(name):
    c = FF[name]
    p = ff_inputs(c)
    ref = ff_ref(c, p)
    h, y = ff_alt_fp32(p)
    assert rel(h, ref["h"][:, :c.F]) < 1e-5 and rel(y, ref["y"]) < 1e-5
    assert torch.equal(ref["h"][:, c.F:], torch.zeros(c.M, fpad(c.F) - c.F, dtype=torch.float64))
    # the group sums add up to the row statistics they are merged into
    s = ref["g_sums"].sum(0)
    mean = s[:, 0] / c.F
    assert rel(mean, ref["rowstat"][:, 0]) < 1e-12
    assert rel(1.0 / torch.sqrt(s[:, 1] / c.F - mean * mean + 1e-5), ref["rowstat"][:, 1]) < 1e-10
    assert ref["g_sums"].shape == (fpad(c.F) // 32, c.M, 2) and ref["y_sums"].shape == (c.Dout // 32, c.M, 2)


@pytest.mark.parametrize("shape", GEGLU_LN_SHAPES[:1] + LN_PLANES_SHAPES[:1])
def test_ln_planes_reference(shape):
    rows, D, ldy = shape
    x, gamma, beta = ln_planes_inputs(rows, D, 2 * D, True)
    assert rel(F.layer_norm(x[:, :D], (D,), gamma, beta), ln_planes_ref(x, gamma, beta, D)) < 1e-5
    a, gate = x[:, :D], x[:, D:]
    assert rel(F.layer_norm(gate * F.gelu(a), (D,), gamma, None), ln_planes_ref(x, gamma, None, D, geglu=True)) < 1e-5


def test_plane_helpers_round_trip():
    g = torch.Generator().manual_seed(5)
    v = torch.randn(6, 96, generator=g) * 7.0
    hi, lo = em_split(v)
    img = torch.stack([hi.reshape(6, 3, 32), lo.reshape(6, 3, 32)], dim=2).half()   # [rows][ld / 32][hi | lo][32]
    dh, dl = decode_plane_image(img.reshape(-1), 6, 96)
    assert torch.equal(dh.float(), hi) and torch.equal(dl.float(), lo)
    assert rel(planes_to_float(dh, dl), v) < 2.0 ** -21          # two 11-bit significands
    assert rel(dh, v) > 2.0 ** -14                                # ... against one
    assert torch.tensor([SENTINEL_BITS], dtype=torch.int16).view(torch.float16).isfinite().all()


# ================================================================================================ tests: the precision floor
FLOOR_SHAPES = [(300, 64, 4), (600, 192, 3), (1200, 512, 8), (2100, 1024, 16)]   # (M, K, H)
FLOOR_MAX, HI_ONLY_MIN = 1e-6, 1e-4   # half the flat bound; fifty times the flat bound


@pytest.mark.parametrize("M,K,H", FLOOR_SHAPES)
def test_precision_floor(M, K, H):
    """What two f16 planes and three fp32 products can deliver, epilogue included - this emulation on the four shapes gives: product 2.6e-7 .. 6.2e-7, q planes
    2.8e-7 .. 6.1e-7, GEGLU planes 2.3e-7 .. 8.2e-7, group sums 2.4e-7 .. 5.4e-7, sums of squares 2.8e-7 .. 8.4e-7 (the folded consumer, next test: 3.9e-7 .. 7.3e-7);
    a result that kept only its hi plane 2.4e-4 .. 3.9e-4."""
    g = torch.Generator().manual_seed(M + K)
    a = torch.randn(M, K, generator=g) * 3.0
    w = torch.randn(64 * H, K, generator=g) / math.sqrt(K)
    qs = 1.0 + 0.3 * torch.randn(64, generator=g)
    ref = a.double() @ w.double().t()
    prod = em_product(*em_split(a), *em_split(w))
    e = {"product": rel(prod, ref)}
    q = F.normalize((prod * 8.0).reshape(M, H, 64), dim=-1) * qs * POST
    qref = l2norm64((ref * 8.0).reshape(M, H, 64)) * qs.double() * POST
    qh, ql = em_split(q)
    e["q planes"] = rel(em_join(qh.double(), ql.double()), qref)
    hi_only = rel(qh, qref)
    n2 = 32 * H   # GEGLU over the same product: the first half of the columns as `a`, the second as `gate`
    h = prod[:, n2:] * F.gelu(prod[:, :n2])
    href = ref[:, n2:] * (0.5 * ref[:, :n2] * (1.0 + torch.erf(ref[:, :n2] / math.sqrt(2.0))))
    e["geglu planes"] = rel(em_join(*(t.double() for t in em_split(h))), href)
    gs, gref = group_sums(h, n2), group_sums(href, n2)
    e["group sums"], e["group sums of squares"] = rel(gs[..., 0], gref[..., 0]), rel(gs[..., 1], gref[..., 1])
    print(f"floor M={M} K={K} H={H}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()) + f", hi plane only {hi_only:.2e}")
    for k, v in e.items():
        assert v < FLOOR_MAX, (k, v)
    assert hi_only > HI_ONLY_MIN, hi_only


@pytest.mark.parametrize("name", ["ff-fold", "ff-ragged", "ff-staged"])
def test_precision_floor_folded_consumer(name):
    c = FF[name]
    p = ff_inputs(c)
    e = ff_errors(c, em_ff(c, p), ff_ref(c, p))
    print(f"floor {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < FLOOR_MAX, (k, v)


def test_offset_case_ratio_and_bound():
    """The offset case's GEGLU rows have mean / std near 2 (from the reference alone), and its bound comes out of the emulation of this exact input: the flat bound no longer
    fits the fold, which cancels in rstd (acc - mean cs).  The emulated error of y for raw (a, gate) rows at std 1.5 offset by 0 / 3 / 4.5 / 6 / 8: 7.3e-7 / 9.3e-7 / 1.2e-6 /
    1.6e-6 / 2.5e-6; the case uses 4.5 (mean / std of the GEGLU rows 1.5 .. 2.7, median 2.1)."""
    p, ref, bound = offset_case()
    h = ref["h"][:, :OFFSET_CASE.F]
    ratio = (h.mean(-1) / h.std(-1, unbiased=False))
    print(f"offset case: mean / std of the GEGLU rows {float(ratio.min()):.2f} .. {float(ratio.max()):.2f} (median {float(ratio.median()):.2f}); floors "
          + ", ".join(f"{k} {v:.2e}" for k, v in _offset_cache["floor"].items()))
    assert 1.5 < float(ratio.median()) < 2.5 and float(ratio.min()) > 1.0
    plain = ff_inputs(OFFSET_CASE)
    e0 = ff_errors(OFFSET_CASE, em_ff(OFFSET_CASE, plain), ff_ref(OFFSET_CASE, plain))
    assert _offset_cache["floor"]["y"] > e0["y"]                  # the cancellation costs precision ...
    assert FLAT_BOUND <= bound["y"] < 10 * FLAT_BOUND             # ... a small multiple of it, not orders of magnitude
    assert bound["h"] == bound["g_sums.0"] == FLAT_BOUND


# ================================================================================================ tests: the launch plan of every GPU case
def qkv_plan_case(c, weights=0):
    n_out = 64 * c.H * {"q": 1, "kv": 2, "qkv": 3}[c.kind]
    s = f"M={c.B * c.T} N={n_out} K={c.K} force_wm={c.block} w16={int(weights >= 1)}"
    if c.form == 1:
        return s + (f" ksplit={c.ksplit} kpart=1" if c.ksplit > 1 else "")
    return s + f" epi={ {'q': 1, 'kv': 3, 'qkv': 4}[c.kind] } epi_rows={c.T} epi_heads={c.H}" + (f" epi_ld={c.ld}" if c.kind != "q" else "")


def ff_plan_cases(c, level, merge):
    Fp = fpad(c.F)
    up = f"M={c.M} N={2 * Fp} K={c.D} epi=2 ldc={Fp} force_wm={c.block}" + (f" ln_out=1 ln_out_ld={Fp}" if level >= 1 else "")
    down = f"M={c.M} N={c.Dout} K={Fp} R=1 force_wm={c.block}"
    if level >= 1:
        down += " ln_in_stats=1" if merge == 0 else f" ln_in_gsums=1 ln_in_groups={Fp // 32} ln_in_count={c.F}"
    if level == 2:
        down += f" ln_out=1 ln_out_ld={c.Dout}"
    return up, down


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    import json

    # (the same program tests/test_gemm_plan_cpu.py builds: where that module ran earlier in this session its binary is taken, a minute of compilation less)
    built = sorted(tmp_path_factory.getbasetemp().glob("gemm_plan*/gemm_plan_dump"))
    exe = str(built[0]) if built else str(tmp_path_factory.mktemp("muse_proj_plan") / "gemm_plan_dump")
    if not built:
        r = subprocess.run([HIPCC, "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "bevgen_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                            os.path.join(ROOT, "tests", "host", "gemm_plan_dump.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
        out = [json.loads(line) for line in p.stdout.splitlines()][:-1]
        assert len(out) == len(cases)
        res = []
        for case, o in zip(cases, out):
            assert "launches" in o, (case, o)
            res.append([(l["rows"][0], l["rows"][1], tuple(l["variant"])) for l in o["launches"]])
            assert all(l["in_table"] == 1 and l["sk"] == 0 and l["w16"] == int("w16=1" in case) for l in o["launches"]), (case, o)
        return res

    return run


def test_launch_plan_of_the_qkv_cases(dump):
    runs = [(QKV[n], wt) for (n, wt, _) in QKV_RUNS]
    for (c, wt), plan in zip(runs, dump([qkv_plan_case(c, wt) for c, wt in runs])):
        assert plan == c.plan, (c.name, wt, plan)
    # the shapes the table stands for: every block shape of the fused epilogues, the split-K instantiation and a launch with m_base != 0
    seen = {v for c in QKV_CASES for (_, _, v) in c.plan}
    assert seen >= {T64, T8W, T2S, T256, T32x32, (0, 2, 4, 1, 1, 2)} and any(r0 != 0 for c in QKV_CASES for (r0, _, _) in c.plan)


def test_launch_plan_of_the_ff_cases(dump):
    jobs = [(c, lv, mg) for c in FF_CASES + [OFFSET_CASE] for (lv, mg) in FF_FORMS]
    lines = [s for (c, lv, mg) in jobs for s in ff_plan_cases(c, lv, mg)]
    plans = dump(lines)
    for i, (c, lv, mg) in enumerate(jobs):
        assert plans[2 * i] == c.up and plans[2 * i + 1] == c.down, (c.name, lv, mg, plans[2 * i], plans[2 * i + 1])
