"""Route M's split-precision attention (bevgen_amd/csrc/attention_split.hip) as muse.cpp launches it - pre-split (hi, lo) f16 operand planes, the packed bias, kv_group,
the key split, the plane-image output: case table, input builders, fp64 reference, bound and the arithmetic floor of tests/test_muse_attn_ops_gpu.py, checked here
without a GPU.

* Inputs: q and k are l2-normalised random rows times a per-dimension scale (1 + 0.3 N(0, 1)), q additionally times POST (the score scale 8 log2 e the projection epilogue
  folds in); v ~ N(0, 1); everything split with em_split.  K rows and V^T columns from `keys` on hold a fill value (zero or the finite sentinel): the fused epilogues never
  clear them.  The bias is the model's [Nq, Nk_pad] matrix in the base-2 domain: (0 | BIAS_SPREAD N(0, 1), a third of it hidden | hidden from column `keys` on) x log2 e
  with hidden = -1e30.  Column 0 (the null key) is visible in every row - except the rows of the `self-ks2` case that are to see nothing of key range 0: those see the
  last key instead.  Every query row sees a key (asserted per case).
* Reference: fp64 softmax attention, 2^x domain, over the JOINED plane values hi + lo / 2048: the error of splitting the operands is no part of the comparison.
* Bound: ATTN_BOUND = 5e-6 of max |ref|, the bound this kernel is held to in its fp32-operand form (tests/test_ops_gpu.py test_attention_split_precision).  The floor: the
  kernel's arithmetic in plain fp32 torch (three-product scores with the f16 q_hi 2^-11 / q_lo 2^-11 operands, exp2, P split to (hi, lo unscaled), three-product PV, the
  multiplication by 1 / l, the output split) against the reference; OFFSET_FACTOR x floor <= ATTN_BOUND is asserted for every case.
* KEY_SPLIT_BOUND = 2e-6: key-split against unsplit launch (test_attention_split_precision_key_ranges)."""
import math
from collections import namedtuple

import pytest
import torch

from test_muse_proj_ref_cpu import OFFSET_FACTOR, POST, SENTINEL_BITS, decode_plane_image, em_split, l2norm64, planes_to_float, rel, seed_of

ATTN_BOUND = 5e-6
KEY_SPLIT_BOUND = 2e-6
LOG2E = 1.4426950408889634
HIDDEN = -1.0e30
BIAS_SPREAD = 1.0
SENTINEL_F16 = 231.625           # the value of SENTINEL_BITS

# keys: visible key rows [0, keys) (null key included); Nk_pad = round_up(keys, 32); kv_group: batch elements per K / V slot; ks: key ranges
AttnCase = namedtuple("AttnCase", "name B H Nq keys Nk_pad kv_group ks")
ATTN_CASES = [
    AttnCase("one-tile", 1, 1, 32, 17, 32, 1, 1),          # one wave, one tile
    AttnCase("one-row", 1, 2, 1, 33, 64, 1, 1),            # the qc clamp on every other lane
    AttnCase("full-block", 2, 1, 256, 64, 64, 1, 1),       # no ragged rows
    AttnCase("cross", 1, 2, 300, 257, 288, 1, 1),          # ragged second block (a wave with 12 valid rows, six empty waves); 9 tiles: the model's cross shape
    AttnCase("group-xcd", 4, 2, 300, 257, 288, 2, 1),      # 16 workgroups: the XCD remap is taken; the two layouts' K / V differ
    AttnCase("group-3", 3, 1, 77, 250, 256, 3, 1),         # 3 workgroups, no remap
    AttnCase("self-ks2", 1, 2, 300, 1537, 1568, 1, 2),     # 49 tiles in ranges of 24 and 25; remap with the key split (8 workgroups); late spike key, rows blind in range 0
    AttnCase("ks3-one-tile", 2, 1, 257, 90, 96, 1, 3),     # one tile per range; the second block has a single row
]
ATTN = {c.name: c for c in ATTN_CASES}
KS_CASES = [c.name for c in ATTN_CASES if c.ks > 1]
GROUP_CASES = [c.name for c in ATTN_CASES if c.kv_group > 1]
PADDED_CASES = [c.name for c in ATTN_CASES if c.keys < c.Nk_pad]
SPIKE = ("self-ks2", 0, 0, 5, 1537 - 3)   # (case, batch, head, query row, key row): the key is that query's direction - its row maximum lies in the last key range


def workgroups(c, ks=None):
    """(grid size, XCD remap taken) of the case's launch: cdiv(Nq, 256) x H x (B x ranges) workgroups, remapped when their number is a multiple of 8"""
    n = -(-c.Nq // 256) * c.H * c.B * (c.ks if ks is None else ks)
    return n, n % 8 == 0


def tile_ranges(c, ks=None):
    """[first tile, end tile) of every key range, as the kernel cuts them"""
    ks = c.ks if ks is None else ks
    nt = c.Nk_pad // 32
    return [(k * nt // ks, (k + 1) * nt // ks) for k in range(ks)]


# ================================================================================================ inputs
def attn_bias(c, g):
    """[Nq, Nk_pad] fp32, base-2 domain"""
    b = torch.randn(c.Nq, c.Nk_pad, generator=g) * BIAS_SPREAD
    b[torch.rand(c.Nq, c.Nk_pad, generator=g) < 1.0 / 3.0] = HIDDEN
    b[:, 0] = 0.0
    b[:, c.keys:] = HIDDEN
    if c.name == "self-ks2":   # rows that see nothing of key range 0 (its partial result is the empty one: maximum -1e30, row sum 0)
        end0 = tile_ranges(c)[0][1] * 32
        b[1::4, :end0] = HIDDEN
        b[1::4, c.keys - 1] = 0.5
        b[SPIKE[3], SPIKE[4]] = 0.0
    return b * LOG2E


def attn_inputs(c, fill=SENTINEL_F16):
    """{Qh, Ql [B, H, Nq, 64], Kh, Kl [B / kv_group, H, Nk_pad, 64], VTh, VTl [B / kv_group, H, 64, Nk_pad]} as f16 tensors, bias [Nq, Nk_pad] fp32; `fill`: the value of
    every plane element at key positions >= keys"""
    g = torch.Generator().manual_seed(seed_of(c.name))
    Bk = c.B // c.kv_group
    q_scale, k_scale = 1.0 + 0.3 * torch.randn(64, generator=g), 1.0 + 0.3 * torch.randn(64, generator=g)
    q = l2norm64(torch.randn(c.B, c.H, c.Nq, 64, generator=g)) * q_scale * POST
    k = l2norm64(torch.randn(Bk, c.H, c.keys, 64, generator=g)) * k_scale
    v = torch.randn(Bk, c.H, c.keys, 64, generator=g)
    if c.name == SPIKE[0]:
        _, b, h, row, key = SPIKE
        k[b, h, key] = l2norm64(q[b, h, row]) * k_scale
    p = {}
    p["Qh"], p["Ql"] = (t.half() for t in em_split(q))
    kh, kl = em_split(k)
    vh, vl = em_split(v.transpose(2, 3).contiguous())
    for name, t, shape, sl in (("Kh", kh, (Bk, c.H, c.Nk_pad, 64), (Ellipsis, slice(0, c.keys), slice(None))), ("Kl", kl, (Bk, c.H, c.Nk_pad, 64), (Ellipsis, slice(0, c.keys), slice(None))),
                               ("VTh", vh, (Bk, c.H, 64, c.Nk_pad), (Ellipsis, slice(0, c.keys))), ("VTl", vl, (Bk, c.H, 64, c.Nk_pad), (Ellipsis, slice(0, c.keys)))):
        full = torch.full(shape, fill, dtype=torch.float16)
        full[sl] = t.half()
        p[name] = full
    p["bias"] = attn_bias(c, g)
    return p


# ================================================================================================ fp64 reference
def attn_ref(p, keys, kv_group=1):
    """softmax_2(Q K^T + bias) V in fp64 over the joined planes, key rows [0, keys) -> [B, Nq, 64 H]; batch element b reads K / V slot b // kv_group"""
    q = planes_to_float(p["Qh"], p["Ql"])
    k = planes_to_float(p["Kh"][:, :, :keys], p["Kl"][:, :, :keys]).repeat_interleave(kv_group, dim=0)
    vt = planes_to_float(p["VTh"][..., :keys], p["VTl"][..., :keys]).repeat_interleave(kv_group, dim=0)
    s = torch.einsum("bhid,bhjd->bhij", q, k) + p["bias"][:, :keys].double()
    w = torch.exp2(s - s.amax(-1, keepdim=True))
    o = torch.einsum("bhij,bhdj->bhid", w / w.sum(-1, keepdim=True), vt)
    B, H, Nq, _ = q.shape
    return o.permute(0, 2, 1, 3).reshape(B, Nq, H * 64)


def attn_alt_fp32(p, keys, kv_group=1):
    """the same attention as the reference module writes it, in fp32 and the natural domain: softmax(sim + bias) v with the visible keys selected by a boolean mask"""
    ln2 = math.log(2.0)
    q = planes_to_float(p["Qh"], p["Ql"]).float()
    k = planes_to_float(p["Kh"], p["Kl"]).float().repeat_interleave(kv_group, dim=0)
    v = planes_to_float(p["VTh"], p["VTl"]).float().repeat_interleave(kv_group, dim=0).transpose(2, 3)
    visible = p["bias"] > -1.0e29
    sim = (q @ k.transpose(2, 3)) * ln2 + torch.where(visible, p["bias"] * ln2, torch.zeros(()))
    sim = sim.masked_fill(~visible, -torch.finfo(torch.float32).max)
    o = sim.softmax(-1) @ v
    B, H, Nq, _ = q.shape
    return o.permute(0, 2, 1, 3).reshape(B, Nq, H * 64)


def out_image(o):
    """fp32 output [B, Nq, 64 H] -> the f16 plane image [B Nq][64 H / 32][hi 32 | lo 32] of its split"""
    rows, hd = o.shape[0] * o.shape[1], o.shape[2]
    hi, lo = em_split(o.reshape(rows, hd))
    return torch.stack([hi.reshape(rows, hd // 32, 32), lo.reshape(rows, hd // 32, 32)], dim=2).half()


def image_value(img, B, Nq, HD):
    """plane image -> its values in fp64 as [B, Nq, 64 H]"""
    hi, lo = decode_plane_image(img.reshape(-1), B * Nq, HD)
    return planes_to_float(hi, lo).reshape(B, Nq, HD)


# ================================================================================================ the precision floor: the kernel's arithmetic in plain torch
def em_attention(p, kv_group=1):
    """fp32 emulation over the whole key axis at once (one maximum per row: the online rescale of the tiled kernel is left out - the floor is what the number formats
    deliver).  Returns the fp32 output [B, Nq, 64 H]; its plane form is out_image() of it."""
    f = lambda t: t.float()
    qh, ql = f(p["Qh"]), f(p["Ql"])
    kh, kl = f(p["Kh"]).repeat_interleave(kv_group, dim=0), f(p["Kl"]).repeat_interleave(kv_group, dim=0)
    vh, vl = f(p["VTh"]).repeat_interleave(kv_group, dim=0), f(p["VTl"]).repeat_interleave(kv_group, dim=0)
    qs, qls = (qh * (1.0 / 2048.0)).half().float(), (ql * (1.0 / 2048.0)).half().float()   # f16 operands: subnormals kept, what lies below them dropped
    s = (p["bias"] + qh @ kh.transpose(2, 3)) + (qls @ kh.transpose(2, 3) + qs @ kl.transpose(2, 3))
    w = torch.exp2(s - s.amax(-1, keepdim=True))
    l = w.sum(-1, keepdim=True)
    wh = w.half().float()
    wl = (w - wh).half().float()
    o = (wh @ vh.transpose(2, 3) + wl @ vh.transpose(2, 3)) + (wh @ vl.transpose(2, 3)) * (1.0 / 2048.0)
    o = o * (1.0 / l)
    B, H, Nq, _ = qh.shape
    return o.permute(0, 2, 1, 3).reshape(B, Nq, H * 64).contiguous()


_case_cache = {}


def attn_case(name):
    """(inputs, fp64 reference) of a case, computed once"""
    if name not in _case_cache:
        c = ATTN[name]
        p = attn_inputs(c)
        _case_cache[name] = (p, attn_ref(p, c.keys, c.kv_group))
    return _case_cache[name]


# ================================================================================================ tests
def test_case_table_reaches_what_it_is_for():
    for c in ATTN_CASES:
        assert c.Nk_pad == (c.keys + 31) // 32 * 32 and c.B % c.kv_group == 0 and 1 <= c.ks <= min(8, c.Nk_pad // 32), c.name
    assert workgroups(ATTN["one-tile"]) == (1, False) and workgroups(ATTN["cross"]) == (4, False) and workgroups(ATTN["group-3"]) == (3, False)
    assert workgroups(ATTN["group-xcd"]) == (16, True) and workgroups(ATTN["self-ks2"]) == (8, True) and workgroups(ATTN["ks3-one-tile"]) == (12, False)
    assert tile_ranges(ATTN["self-ks2"]) == [(0, 24), (24, 49)] and tile_ranges(ATTN["ks3-one-tile"]) == [(0, 1), (1, 2), (2, 3)]
    assert ATTN["cross"].Nq - 256 - 32 == 12 and ATTN["ks3-one-tile"].Nq - 256 == 1 and ATTN["full-block"].Nq % 256 == 0
    assert all(ATTN[n].keys < ATTN[n].Nk_pad for n in PADDED_CASES) and "full-block" not in PADDED_CASES
    assert SPIKE[4] >= tile_ranges(ATTN["self-ks2"])[1][0] * 32


@pytest.mark.parametrize("name", [c.name for c in ATTN_CASES])
def test_every_query_row_sees_a_key(name):
    c = ATTN[name]
    p, ref = attn_case(name)
    visible = p["bias"] > -1.0e29
    assert bool(visible[:, :c.keys].any(-1).all()) and not bool(visible[:, c.keys:].any())
    blind0 = ~visible[:, :tile_ranges(c)[0][1] * 32].any(-1)
    if name == "self-ks2":
        assert int(blind0.sum()) == len(range(1, c.Nq, 4))     # rows that see nothing of key range 0 ...
        assert bool(visible[~blind0][:, 0].all())              # ... every other row sees the null key
        _, b, h, row, key = SPIKE                              # the spike key holds its row's maximum, in the last range, and the row sees it
        s = planes_to_float(p["Qh"], p["Ql"])[b, h, row] @ planes_to_float(p["Kh"], p["Kl"])[b, h, :c.keys].t() + p["bias"][row, :c.keys].double()
        assert int(s.argmax()) == key and bool(visible[row, key]) and bool(blind0[row])
    else:
        assert bool(visible[:, 0].all()) and not bool(blind0.any())
    frac = float((~visible[:, 1:c.keys]).double().mean()) if c.keys > 1 else 0.0
    assert 0.2 < frac < 0.5, frac                              # partly hidden
    for k in ("Kh", "Kl"):                                     # behind the last key: the sentinel, in every plane
        assert bool((p[k][:, :, c.keys:].view(torch.int16) == SENTINEL_BITS).all())
    for k in ("VTh", "VTl"):
        assert bool((p[k][..., c.keys:].view(torch.int16) == SENTINEL_BITS).all())
    assert ref.shape == (c.B, c.Nq, 64 * c.H) and bool(ref.isfinite().all())
    if c.B // c.kv_group > 1 and c.kv_group > 1:   # the layouts' keys and values differ, and so do the results of a query row read against either
        assert not torch.equal(p["Kh"][0], p["Kh"][1]) and not torch.equal(p["VTh"][0], p["VTh"][1])
        other = dict(p, Kh=p["Kh"].flip(0), Kl=p["Kl"].flip(0), VTh=p["VTh"].flip(0), VTl=p["VTl"].flip(0))
        assert rel(attn_ref(other, c.keys, c.kv_group), ref) > 1e-2


@pytest.mark.parametrize("name", ["one-tile", "one-row", "group-3", "ks3-one-tile"])
def test_reference_against_fp32_formulation(name):
    c = ATTN[name]
    p, ref = attn_case(name)
    zero_fill = attn_inputs(c, fill=0.0)   # (the fp32 formulation multiplies the hidden keys by a zero weight: it needs finite products, which both fills give)
    assert rel(attn_alt_fp32(p, c.keys, c.kv_group), ref) < 1e-5
    assert torch.equal(attn_ref(zero_fill, c.keys, c.kv_group), ref)


@pytest.mark.parametrize("name", [c.name for c in ATTN_CASES])
def test_precision_floor_leaves_the_bound_room(name):
    """Floors of this emulation (fp32 form / plane form), printed per case; OFFSET_FACTOR x floor must fit under ATTN_BOUND, and a result that kept only its hi plane must
    miss the bound by far."""
    c = ATTN[name]
    p, ref = attn_case(name)
    o = em_attention(p, c.kv_group)
    img = out_image(o)
    floor32, floor_pl = rel(o, ref), rel(image_value(img, c.B, c.Nq, 64 * c.H), ref)
    hi_only = rel(decode_plane_image(img.reshape(-1), c.B * c.Nq, 64 * c.H)[0].reshape(ref.shape), ref)
    print(f"floor {name}: fp32 form {floor32:.2e}, plane form {floor_pl:.2e}, hi plane only {hi_only:.2e} (bound {ATTN_BOUND:.0e})")
    assert OFFSET_FACTOR * max(floor32, floor_pl) <= ATTN_BOUND, (floor32, floor_pl)
    assert hi_only > 20 * ATTN_BOUND, hi_only


def test_host_split_of_joined_planes_gives_the_same_bits():
    """em_split(hi + lo / 2048) == (hi, lo): the host split the bit-identity tests apply to the device's fp32 output is the inverse of the join the reference reads, on the
    planes of every case and on the split of N(0, 1) x 7 values.  The one exception is arithmetic, not a defect: |lo| / 2048 exactly half an ulp of hi is a tie of the
    first rounding, which then goes to the even neighbour - such pairs (counted here) are left out."""
    g = torch.Generator().manual_seed(11)
    pairs = [em_split(torch.randn(1 << 16, generator=g) * 7.0)]
    for c in ATTN_CASES:
        p, _ = attn_case(c.name)
        pairs += [(p["Qh"].float(), p["Ql"].float()), (p["Kh"][:, :, :c.keys].float(), p["Kl"][:, :, :c.keys].float()), (p["VTh"][..., :c.keys].float(), p["VTl"][..., :c.keys].float())]
    ties = total = 0
    for hi, lo in pairs:
        joined = planes_to_float(hi, lo)
        assert torch.equal(joined.float().double(), joined)          # the join is exact in fp32
        h2, l2 = em_split(joined.float())
        _, e = torch.frexp(hi)
        half_ulp = torch.ldexp(torch.ones(()), (e - 12).clamp_min(-25))
        tie = (lo.abs() * (1.0 / 2048.0)) == half_ulp
        ties, total = ties + int(tie.sum()), total + hi.numel()
        assert torch.equal(h2[~tie], hi[~tie]) and torch.equal(l2[~tie], lo[~tie])
    print(f"host split of joined planes: {total} pairs, {ties} ties left out")
    assert ties < total * 1e-3
