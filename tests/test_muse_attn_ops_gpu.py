"""Operator-level parity of Route M's split-precision attention kernel (bevgen_amd/csrc/attention_split.hip) in the form muse.cpp launches - pre-split operand planes as
the projection epilogues write them, the packed bias, kv_group, the key split with its combine kernel, and the plane-image output (staged 16-byte row-major stores;
store_planes4 in the combine) - through bevgen_op_muse_attention.  Case table, inputs, fp64 reference, bound and arithmetic floor: tests/test_muse_attn_ref_cpu.py.

Every output sits in a finite-sentinel buffer with a guard region on both sides; K rows / V^T columns behind the last key hold the sentinel, as the fused epilogues
leave whatever was there.

Worst errors measured on an MI355X (max |out - ref| / max |ref|, bound 5e-6; each test prints its own, `pytest -s`): plane form and fp32 form alike 1.2e-6 (cross),
8.3e-7 (group-xcd), 5.6e-7 / 5.1e-7 (group-3), 4.9e-7 (full-block), 4.1e-7 (ks3-one-tile), 3.8e-7 (one-row), 3.3e-7 (self-ks2), 2.6e-7 (one-tile); behind the fused
q | k | v projection 2.4e-7; key split against the unsplit launch 1.8e-7 / 2.3e-7 (bound 2e-6).  The emulation floors of the CPU file: 1.9e-7 .. 8.8e-7.
The plane image equals the split of the fp32 output bit for bit in every case, staged store and combine kernel alike: no kernel change was needed.
Scratch-build mutants of attention_split.hip (none committed, all in bounds) and how many of these 33 tests each fails:
  `b / a.kv_group` replaced by 0                                   6  (every case with more than one K / V slot; both kv_group tests of group-xcd)
  `lo_sel ? lo8 : hi8` swapped                                    15
  `t_first` dropped from the bias pointer only                     6
  the combine taking its maximum from range 0 only                 3  (self-ks2: the rows that see nothing of range 0)
  `head * 128` -> `head * 64` in the staged plane store           10"""
import pytest
import torch

from test_muse_attn_ref_cpu import (ATTN, ATTN_BOUND, ATTN_CASES, GROUP_CASES, KEY_SPLIT_BOUND, KS_CASES, LOG2E, HIDDEN, PADDED_CASES, attn_case, attn_inputs, attn_ref, image_value,
                                    out_image)
from test_muse_proj_ops_gpu import Guarded, consume_status, dev, qkv_device_inputs, run_qkv
from test_muse_proj_ref_cpu import QkvCase, qkv_inputs, rel

pytestmark = pytest.mark.gpu

ALL = [c.name for c in ATTN_CASES]


@pytest.fixture(scope="module")
def ctx():
    from bevgen_amd.runtime import Context

    c = Context(None, precision="f16x3")
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_status_word(ctx):
    """a test that fails with a raised status word must not hand it to the next test of the shared context"""
    yield
    from bevgen_amd import _lib

    torch.cuda.synchronize()
    if ctx.status():
        try:
            ctx.synchronize()
        except _lib.BevgenError:
            pass


def device_inputs(p):
    return {k: dev(v) for k, v in p.items()}


def run_attn(ctx, d, *, B, H, Nq, Nk_pad, kv_group=1, ks=1, form="planes"):
    """one launch on device inputs d (planes + bias) -> the Guarded output: the plane image [B Nq, 64 H / 32, 2, 32] (form 'planes') or fp32 [B, Nq, 64 H] ('f32')"""
    out = Guarded((B * Nq, 2 * H, 2, 32), torch.float16) if form == "planes" else Guarded((B, Nq, 64 * H), torch.float32)
    ctx.op_muse_attention(d, d["bias"], B=B, H=H, Nq=Nq, Nk_pad=Nk_pad, kv_group=kv_group, key_splits=ks, **{"out_planes" if form == "planes" else "out": out.view})
    return out


_dev_cache, _run_cache = {}, {}


def case_device(name):
    if name not in _dev_cache:
        _dev_cache[name] = device_inputs(attn_case(name)[0])
    return _dev_cache[name]


def case_run(ctx, name, form, ks=None):
    """(host tensor, bits of the whole buffer) of the case's launch in `form`, run once per module (guards checked, status word clean)"""
    c = ATTN[name]
    ks = c.ks if ks is None else ks
    key = (name, form, ks)
    if key not in _run_cache:
        g = run_attn(ctx, case_device(name), B=c.B, H=c.H, Nq=c.Nq, Nk_pad=c.Nk_pad, kv_group=c.kv_group, ks=ks, form=form)
        _run_cache[key] = g.host()
        assert ctx.status() == 0, key
    return _run_cache[key]


# ================================================================================================ 1. parity against fp64, both output forms
@pytest.mark.parametrize("name", ALL)
def test_muse_attention_parity(ctx, name):
    c = ATTN[name]
    _, ref = attn_case(name)
    img, _ = case_run(ctx, name, "planes")
    o, _ = case_run(ctx, name, "f32")
    e_pl, e_32 = rel(image_value(img, c.B, c.Nq, 64 * c.H), ref), rel(o, ref)
    print(f"muse_attention {name}: plane form {e_pl:.2e}, fp32 form {e_32:.2e} (bound {ATTN_BOUND:.0e})")
    assert e_pl < ATTN_BOUND and e_32 < ATTN_BOUND, (name, e_pl, e_32)


# ================================================================================================ 2. the plane form is the split of the fp32 form
@pytest.mark.parametrize("name", ALL)
def test_plane_form_is_the_split_of_the_fp32_form(ctx, name):
    """staged row-major store (one key range) and the combine kernel's store_planes4 (key split): (hi, lo) of exactly the fp32 value the other form stores"""
    img, _ = case_run(ctx, name, "planes")
    o, _ = case_run(ctx, name, "f32")
    want = out_image(o).view(torch.int16)
    got = img.view(torch.int16)
    differ = (want != got).reshape(got.shape[0], -1).any(-1).nonzero().flatten()
    print(f"muse_attention {name}: plane image rows that differ from the split of the fp32 output: {differ.numel()} of {got.shape[0]}")
    assert torch.equal(want, got), (name, differ[:8].tolist())


# ================================================================================================ 3. kv_group
@pytest.mark.parametrize("name", GROUP_CASES)
@pytest.mark.parametrize("form", ["planes", "f32"])
def test_kv_group_reads_the_layouts_slot(ctx, name, form):
    """the grouped launch equals, bit for bit, one launch per layout with kv_group = 1 on that layout's K / V slot and its samples' queries"""
    c = ATTN[name]
    d = case_device(name)
    whole, _ = case_run(ctx, name, form)
    whole = whole.reshape(c.B, -1)
    S = c.kv_group
    for lay in range(c.B // S):
        sub = {k: d[k][lay * S:(lay + 1) * S].contiguous() for k in ("Qh", "Ql")}
        for k in ("Kh", "Kl", "VTh", "VTl"):   # one slot, handed to every sample of the layout
            sub[k] = d[k][lay:lay + 1].expand(S, -1, -1, -1).contiguous()
        sub["bias"] = d["bias"]
        part, _ = run_attn(ctx, sub, B=S, H=c.H, Nq=c.Nq, Nk_pad=c.Nk_pad, kv_group=1, ks=c.ks, form=form).host()
        bits = torch.int16 if form == "planes" else torch.int32
        assert torch.equal(part.reshape(S, -1).view(bits), whole[lay * S:(lay + 1) * S].contiguous().view(bits)), (name, form, lay)
    assert ctx.status() == 0


# ================================================================================================ 4. what lies behind the last key contributes nothing
@pytest.mark.parametrize("name", PADDED_CASES)
def test_masked_padding_contributes_nothing(ctx, name):
    """K rows and V^T columns from `keys` on filled with zeros instead of the sentinel: the same bits in both output forms"""
    c = ATTN[name]
    p0 = attn_inputs(c, fill=0.0)
    p1, _ = attn_case(name)
    assert bool((p0["Kh"][:, :, c.keys:] == 0).all()) and bool((p0["VTl"][..., c.keys:] == 0).all()) and torch.equal(p0["Kh"][:, :, :c.keys], p1["Kh"][:, :, :c.keys])
    d0 = device_inputs(p0)
    for form in ("planes", "f32"):
        _, bits1 = case_run(ctx, name, form)
        _, bits0 = run_attn(ctx, d0, B=c.B, H=c.H, Nq=c.Nq, Nk_pad=c.Nk_pad, kv_group=c.kv_group, ks=c.ks, form=form).host()
        assert torch.equal(bits0, bits1), (name, form)
    assert ctx.status() == 0


# ================================================================================================ 5. key split
@pytest.mark.parametrize("name", KS_CASES)
def test_key_split_against_the_unsplit_launch(ctx, name):
    c = ATTN[name]
    _, ref = attn_case(name)
    for form in ("planes", "f32"):
        value = (lambda t: image_value(t, c.B, c.Nq, 64 * c.H)) if form == "planes" else (lambda t: t.double())
        split, bits = case_run(ctx, name, form)
        one, _ = case_run(ctx, name, form, ks=1)
        e_ref, e_one, e_one_ref = rel(value(split), ref), rel(value(split), value(one)), rel(value(one), ref)
        print(f"muse_attention {name} {form}: {c.ks} ranges {e_ref:.2e}, one range {e_one_ref:.2e} (bound {ATTN_BOUND:.0e}); split against unsplit {e_one:.2e} (bound {KEY_SPLIT_BOUND:.0e})")
        assert e_ref < ATTN_BOUND and e_one_ref < ATTN_BOUND and e_one < KEY_SPLIT_BOUND, (name, form, e_ref, e_one_ref, e_one)
        _, again = run_attn(ctx, case_device(name), B=c.B, H=c.H, Nq=c.Nq, Nk_pad=c.Nk_pad, kv_group=c.kv_group, ks=c.ks, form=form).host()
        assert torch.equal(bits, again), f"{name} {form}: two runs differ"
    assert ctx.status() == 0


# ================================================================================================ 6. the status word
@pytest.mark.parametrize("ks", [1, 2])
def test_nan_query_raises_f16_range_in_the_plane_form(ctx, ks):
    """one NaN in a Qh element: the plane writers' guard (guard_half8 in the staged store, guard_half4 in the combine's store_planes4) raises BEVGEN_STATUS_F16_RANGE, that
    (batch, row, head) alone is non-finite and every other output element keeps its bits; the clean launch leaves the word 0 (case_run asserts it for every case)"""
    from bevgen_amd import _lib

    name = "ks3-one-tile"
    c = ATTN[name]
    b, row = 1, 130
    clean, _ = case_run(ctx, name, "planes", ks=ks)
    d = dict(case_device(name))
    d["Qh"] = d["Qh"].clone()
    d["Qh"][b, 0, row, 7] = float("nan")
    out = run_attn(ctx, d, B=c.B, H=c.H, Nq=c.Nq, Nk_pad=c.Nk_pad, ks=ks, form="planes")
    consume_status(ctx, _lib.STATUS_F16_RANGE, "f16 operand")
    img, _ = out.host()
    bad = ~image_value(img, c.B, c.Nq, 64 * c.H).isfinite()
    assert bool(bad[b, row].all()) and int(bad.sum()) == 64 * c.H
    keep = torch.ones(c.B * c.Nq, dtype=torch.bool)
    keep[b * c.Nq + row] = False
    assert torch.equal(img.view(torch.int16)[keep], clean.view(torch.int16)[keep])
    run_attn(ctx, case_device(name), B=c.B, H=c.H, Nq=c.Nq, Nk_pad=c.Nk_pad, ks=ks, form="planes")   # the clean operands again: nothing is raised
    consume_status(ctx, 0, None)


# ================================================================================================ 7. contract with the producer
def test_planes_of_the_fused_projection_feed_the_attention(ctx):
    """bevgen_op_muse_qkv (merged q | k | v epilogue) writes its planes into sentinel-filled buffers and those buffers are the attention's operands: null key at row 0,
    token t at key row 1 + t, V^T with pitch ld, everything behind the last token never written.  Reference: fp64 attention over the planes read back from the device."""
    c = QkvCase("attn-feed", "qkv", 1, 40, 2, 64, 64, 0, 0, 1, [])
    planes = run_qkv(ctx, c, qkv_device_inputs(qkv_inputs(c)))
    host = {k: g.host()[0] for k, g in planes.items()}
    for k in ("Kh", "Kl"):
        assert planes[k].untouched(host[k][:, :, c.T + 1:])
    for k in ("VTh", "VTl"):
        assert planes[k].untouched(host[k][..., c.T + 1:])
    g = torch.Generator().manual_seed(40)
    bias = torch.randn(c.T, c.ld, generator=g)
    bias[torch.rand(c.T, c.ld, generator=g) < 1.0 / 3.0] = HIDDEN
    bias[:, 0] = 0.0
    bias[:, c.T + 1:] = HIDDEN
    bias *= LOG2E
    ref = attn_ref(dict(host, bias=bias), c.T + 1)
    d = {k: g_.view for k, g_ in planes.items()}
    d["bias"] = dev(bias)
    img, _ = run_attn(ctx, d, B=c.B, H=c.H, Nq=c.T, Nk_pad=c.ld, form="planes").host()
    o, _ = run_attn(ctx, d, B=c.B, H=c.H, Nq=c.T, Nk_pad=c.ld, form="f32").host()
    e_pl, e_32 = rel(image_value(img, c.B, c.T, 64 * c.H), ref), rel(o, ref)
    print(f"muse_attention behind muse_qkv: plane form {e_pl:.2e}, fp32 form {e_32:.2e} (bound {ATTN_BOUND:.0e})")
    assert e_pl < ATTN_BOUND and e_32 < ATTN_BOUND, (e_pl, e_32)
    assert torch.equal(out_image(o).view(torch.int16), img.view(torch.int16))
    assert ctx.status() == 0


# ================================================================================================ 8. refusals
def test_muse_attention_refuses_unsupported_arguments(ctx, gpu_ctx):
    from bevgen_amd import _lib

    c = ATTN["group-3"]
    d = case_device(c.name)
    img, o = Guarded((c.B * c.Nq, 2 * c.H, 2, 32), torch.float16), Guarded((c.B, c.Nq, 64 * c.H), torch.float32)
    common = dict(B=c.B, H=c.H, Nq=c.Nq, Nk_pad=c.Nk_pad)
    for bad in (dict(kv_group=2, out_planes=img.view), dict(kv_group=0, out_planes=img.view), dict(kv_group=3, out_planes=img.view, out=o.view), dict(kv_group=3),
                dict(kv_group=3, key_splits=c.Nk_pad // 32 + 1, out=o.view), dict(kv_group=3, key_splits=0, out_planes=img.view)):
        with pytest.raises(_lib.BevgenError, match="op_muse_attention") as ei:
            ctx.op_muse_attention(d, d["bias"], **common, **bad)
        assert ei.value.code == -1   # BEVGEN_ERR_INVALID
    small = ATTN["one-tile"]   # key_splits 2 on a single tile
    with pytest.raises(_lib.BevgenError, match="op_muse_attention"):
        ctx.op_muse_attention(case_device(small.name), case_device(small.name)["bias"], B=1, H=1, Nq=32, Nk_pad=32, key_splits=2, out_planes=img.view)
    with pytest.raises(_lib.BevgenError, match="op_muse_attention") as ei:   # an fp32 context
        gpu_ctx.op_muse_attention(d, d["bias"], **common, kv_group=3, out_planes=img.view)
    assert ei.value.code == -1
    torch.cuda.synchronize()
    assert img.untouched(img.host()[0]) and o.untouched(o.host()[0])   # nothing was launched
    assert ctx.status() == 0
