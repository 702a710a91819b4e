"""Operator-level fp64 parity of Route M's projections with fused epilogues (bevgen_amd/csrc/gemm_split_glds.hip gemm_tile: EPI_MUSE_Q / _KV / _QKV, EPI_GEGLU, the
folded LayerNorm's producer and consumer sides - direct and staged row-major forms, every block shape) and of the kernels around them (launch_layernorm_planes,
launch_geglu_layernorm_planes, launch_muse_q_prep_split / _kv_prep_split / _null_kv_prep, launch_ln_fold_weight, launch_geglu_weight_order, launch_ln_stats_finalize)
through bevgen_op_muse_qkv, bevgen_op_muse_ff and bevgen_op_layernorm_planes.  Case tables, inputs, references and bounds: tests/test_muse_proj_ref_cpu.py, which also
pins every case to the launcher variant it was chosen for.

Every output buffer starts as a finite sentinel with a guard region on both sides: what a case must not write (key rows / value columns behind the last token, rows >= M,
the outputs of another fold level, the guards) must still hold the sentinel bit for bit.

Worst errors measured on an MI355X (max |out - ref| / max |ref| per output tensor; each test prints its own, `pytest -s`):
  q / k / v, fused (flat bound 2e-6)          Q 2.8e-7, K 2.6e-7, V^T 2.4e-7, null key 1.4e-7, null value 9.5e-8; f16-rounded weight 2.5e-7 / 2.1e-7 / 1.8e-7,
                                             single product 2.1e-7 / 2.0e-7 / 1.6e-7, LayerNorm kernel in front 1.8e-7 / 1.8e-7 / 1.9e-7
  q / k / v, un-fused                        Q 1.6e-7 (split-K), K 1.6e-7, V^T 2.0e-7
  feed-forward, flat cases (bound 2e-6)      GEGLU fp32 2.5e-7, GEGLU planes 2.7e-7, group sums 2.7e-7, sums of squares 3.4e-7, mean 1.9e-7, rstd 8.2e-8, y 3.0e-7 (level 0:
                                             2.9e-7), y planes 3.0e-7, sums of y 2.4e-7 / 2.3e-7
  feed-forward, offset case                  y 5.5e-7 folded (3.3e-7 at level 0) against its bound 4.8e-6 = 4 x the emulation floor 1.2e-6; rstd 2.2e-7, sums of y 4.2e-7
  LayerNorm to planes (bound 1e-5)           1.9e-7; GEGLU form 1.5e-7
  staged against direct store forms: every output bit-identical - after gemm_tile's last epilogue product was made a rounded fp32 value (mul_rounded): before, the direct
  forms' fma on the unrounded product gave other last bits in the q and k low planes and in the GEGLU group sums (and what follows from them) than the staged forms.
Reverting, in a scratch build, the 1 + key-row offset, the null-row write, the epi_post factor, the - mean cs term or the staged value path's last-token store fails
15 / 16 / 19 / 6 / 11 of these tests."""
import hashlib
import os
import subprocess
import sys

import pytest
import torch

from test_muse_proj_ref_cpu import (FF, FF_CASES, FF_FORMS, FLAT_BOUND, GEGLU_LN_SHAPES, LN_PLANES_BOUND, LN_PLANES_SHAPES, OFFSET_CASE, POST, QKV, QKV_RUNS, RANGE_CASES,
                                    SENTINEL_BITS, STAGED_VS_DIRECT_QKV, decode_plane_image, ff_inputs, ff_ref, fpad, ln_planes_inputs, ln_planes_ref, null_ref, offset_case,
                                    planes_to_float, qkv_inputs, qkv_ref, range_inputs, rel)

pytestmark = pytest.mark.gpu

GUARD = 4096                    # elements in front of and behind every output tensor
F32_SENTINEL = 231.625          # the fp32 outputs' sentinel (the value of SENTINEL_BITS as an f16)
STAGED_VS_DIRECT_FF = "ff-staged"


@pytest.fixture(scope="module")
def ctx():
    from bevgen_amd.runtime import Context

    c = Context(None, precision="f16x3")
    yield c
    c.close()


def dev(t):
    return None if t is None else t.cuda().contiguous()


# ================================================================================================ sentinel-filled, guarded outputs
class Guarded:
    """an output tensor inside a sentinel-filled buffer with GUARD elements on both sides"""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.shape, self.n, self.dtype = tuple(shape), n, dtype
        if dtype == torch.float16:
            self.buf = torch.full((n + 2 * GUARD,), SENTINEL_BITS, dtype=torch.int16, device="cuda").view(torch.float16)
        else:
            self.buf = torch.full((n + 2 * GUARD,), F32_SENTINEL, dtype=torch.float32, device="cuda")
        self.view = self.buf[GUARD:GUARD + n].view(self.shape)

    def bits(self, t):
        return t.contiguous().view(torch.int16 if self.dtype == torch.float16 else torch.int32)

    def sentinel_bits(self):
        return SENTINEL_BITS if self.dtype == torch.float16 else int(torch.tensor([F32_SENTINEL]).view(torch.int32))

    def host(self):
        """(tensor on the host, the whole buffer's bits) - after asserting that both guards are intact"""
        b = self.bits(self.buf.cpu())
        assert bool((b[:GUARD] == self.sentinel_bits()).all()) and bool((b[GUARD + self.n:] == self.sentinel_bits()).all()), "a byte outside the tensor was written"
        return self.buf.cpu()[GUARD:GUARD + self.n].view(self.shape), b

    def untouched(self, t):
        """is every element of this part of the (host) tensor still the sentinel?"""
        return bool((self.bits(t) == self.sentinel_bits()).all())


# ================================================================================================ q / k / v
def qkv_outputs(c):
    shapes = {"Qh": (c.B, c.H, c.T, 64), "Ql": (c.B, c.H, c.T, 64), "Kh": (c.B, c.H, c.ld, 64), "Kl": (c.B, c.H, c.ld, 64), "VTh": (c.B, c.H, 64, c.ld),
              "VTl": (c.B, c.H, 64, c.ld)}
    names = (("Qh", "Ql") if c.kind != "kv" else ()) + (("Kh", "Kl", "VTh", "VTl") if c.kind != "q" else ())
    return {k: Guarded(shapes[k], torch.float16) for k in names}


def run_qkv(ctx, c, d, weights=0):
    """one call of the case on device inputs d -> {name: Guarded}"""
    out = qkv_outputs(c)
    ctx.op_muse_qkv(c.kind, d["a"], d["w"], B=c.B, T=c.T, H=c.H, ld=c.ld, q_scale=d["q_scale"], k_scale=d["k_scale"], null_kv=d["null_kv"], ln_gamma=d["ln_gamma"], post=POST,
                    block=c.block, weights=weights, form=c.form, ksplit=c.ksplit, out={k: g.view for k, g in out.items()})
    return out


def qkv_device_inputs(p):
    return {k: dev(v) for k, v in p.items()}


def check_qkv(c, out, ref, tag):
    """planes against the fp64 reference over positions [0, T]; the rest of every tensor and the guards still the sentinel (un-fused values: zero-filled)"""
    host = {k: g.host() for k, g in out.items()}
    errs = {}
    if "Qh" in out:
        errs["Q"] = rel(planes_to_float(host["Qh"][0], host["Ql"][0]), ref["Q"])
    if "Kh" in out:
        T = c.T
        errs["K"] = rel(planes_to_float(host["Kh"][0][:, :, :T + 1], host["Kl"][0][:, :, :T + 1]), ref["K"])
        errs["VT"] = rel(planes_to_float(host["VTh"][0][..., :T + 1], host["VTl"][0][..., :T + 1]), ref["VT"])
        # row / column 0 against the prepared null key / value alone (launch_muse_null_kv_prep, and the epilogue's copy of it)
        errs["null K"] = rel(planes_to_float(host["Kh"][0][:, :, 0], host["Kl"][0][:, :, 0]), ref["K"][:, :, 0])
        errs["null V"] = rel(planes_to_float(host["VTh"][0][..., 0], host["VTl"][0][..., 0]), ref["VT"][..., 0])
        for k in ("Kh", "Kl"):
            assert out[k].untouched(host[k][0][:, :, T + 1:]), f"{tag}: {k} rows behind the last token were written"
        for k in ("VTh", "VTl"):
            tail = host[k][0][..., T + 1:]
            if c.form == 0:
                assert out[k].untouched(tail), f"{tag}: {k} columns behind the last token were written"
            else:   # launch_muse_kv_prep_split zero-fills them (documented in bevgen_hip.h)
                assert bool((tail.view(torch.int16) == 0).all()), f"{tag}: {k} columns behind the last token are not zero"
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {FLAT_BOUND:.0e})")
    for k, v in errs.items():
        assert v < FLAT_BOUND, (tag, k, v)
    return {k: h[1] for k, h in host.items()}


_qkv_ref_cache = {}


def qkv_case_data(name, weights, ln):
    key = (name, weights, ln)
    if key not in _qkv_ref_cache:
        c = QKV[name]
        p = qkv_inputs(c, ln)
        _qkv_ref_cache[key] = (p, qkv_ref(c, p, weights))
    return _qkv_ref_cache[key]


@pytest.mark.parametrize("name,weights,ln", QKV_RUNS, ids=[f"{n}-w{w}{'-ln' if l else ''}" for (n, w, l) in QKV_RUNS])
def test_muse_qkv(ctx, name, weights, ln):
    c = QKV[name]
    p, ref = qkv_case_data(name, weights, ln)
    d = qkv_device_inputs(p)
    first = check_qkv(c, run_qkv(ctx, c, d, weights), ref, f"muse_qkv {name} weights={weights} ln={int(ln)}")
    torch.cuda.synchronize()
    assert ctx.status() == 0
    again = {k: g.host()[1] for k, g in run_qkv(ctx, c, d, weights).items()}
    for k in first:
        assert torch.equal(first[k], again[k]), f"{name}: {k} differs between two runs"
    assert ctx.status() == 0


def test_muse_qkv_null_prep_is_the_reference_null(ctx):
    """the prepared null key / value a kv case writes at row / column 0 of EVERY (batch, head) is the same pair of planes"""
    c = QKV["kv-a"]
    p, ref = qkv_case_data("kv-a", 0, False)
    out = {k: g.host()[0] for k, g in run_qkv(ctx, c, qkv_device_inputs(p)).items()}
    nk, nv = null_ref(p)
    for b in range(c.B):
        assert torch.equal(out["Kh"][b, :, 0], out["Kh"][0, :, 0]) and torch.equal(out["VTl"][b, :, :, 0], out["VTl"][0, :, :, 0])
    assert rel(planes_to_float(out["Kh"][0, :, 0], out["Kl"][0, :, 0]), nk) < FLAT_BOUND
    assert rel(planes_to_float(out["VTh"][0, :, :, 0], out["VTl"][0, :, :, 0]), nv) < FLAT_BOUND


def consume_status(ctx, bit, text):
    from test_vq_ops_gpu import consume_status as consume

    consume(ctx, bit, text)


@pytest.mark.parametrize("name", RANGE_CASES)
def test_muse_kv_range_guard(ctx, name):
    """One token's value column leaves the f16 range: the call raises exactly BG_ST_F16_RANGE - with the token first and last in its 64-row patch (the two positions the
    staged store's guard masks: the patch's position 0 belongs to its neighbour, its last token leaves through a lane of its own) - and an in-range call leaves 0."""
    from bevgen_amd import _lib

    c = QKV[name]
    for row in (64, 127, c.T + 64, c.T + 127):   # patches with nk0 != 0 of both batch elements
        p, _ = range_inputs(c, row)
        ref = qkv_ref(c, p)
        assert float(p["a"].abs().max()) < 60000.0 and float(ref["VT"].abs().max()) > 65520.0
        run_qkv(ctx, c, qkv_device_inputs(p))
        consume_status(ctx, _lib.STATUS_F16_RANGE, "f16 operand")
    run_qkv(ctx, c, qkv_device_inputs(qkv_inputs(c)))
    consume_status(ctx, 0, None)


def test_muse_qkv_refuses_unsupported_arguments(ctx):
    from bevgen_amd import _lib

    c = QKV["kv-a"]
    d = qkv_device_inputs(qkv_inputs(c))
    out = qkv_outputs(c)
    views = {k: g.view for k, g in out.items()}
    common = dict(B=c.B, T=c.T, H=c.H, q_scale=d["q_scale"], k_scale=d["k_scale"], null_kv=d["null_kv"], out=views)
    for bad in (dict(ld=c.T), dict(ld=c.ld, block=3), dict(ld=c.ld, weights=3), dict(ld=c.ld, ksplit=2), dict(ld=c.ld, form=2)):
        with pytest.raises(_lib.BevgenError, match="op_muse_qkv"):
            ctx.op_muse_qkv("kv", d["a"], d["w"], **common, **bad)
    with pytest.raises(_lib.BevgenError, match="op_muse_qkv"):   # the merged form has no un-fused path
        ctx.op_muse_qkv("qkv", d["a"], torch.zeros(64 * c.H * 3, c.K, device="cuda"), form=1, ld=c.ld, **common)
    torch.cuda.synchronize()
    for g in out.values():   # nothing was launched
        assert g.untouched(g.host()[0])
    assert ctx.status() == 0


# ================================================================================================ feed-forward / folded LayerNorm
def ff_outputs(c):
    Fp = fpad(c.F)
    return {"h": Guarded((c.M, Fp), torch.float32), "g_planes": Guarded((c.M, Fp // 32, 2, 32), torch.float16), "g_sums": Guarded((Fp // 32, c.M, 2), torch.float32),
            "rowstat": Guarded((c.M, 2), torch.float32), "y_planes": Guarded((c.M, c.Dout // 32, 2, 32), torch.float16), "y_sums": Guarded((c.Dout // 32, c.M, 2), torch.float32),
            "y": Guarded((c.M, c.Dout), torch.float32)}


def ff_written(level, merge):
    return {"y"} | ({"h"} if level == 0 else {"g_planes", "g_sums"}) | ({"rowstat"} if level >= 1 and merge == 0 else set()) | ({"y_planes", "y_sums"} if level == 2 else set())


def run_ff(ctx, c, d, level, merge):
    out = ff_outputs(c)
    ctx.op_muse_ff(d["x"], d["w1"], d["gamma3"], d["w4"], d["residual"], level=level, merge=merge, block=c.block, out={k: g.view for k, g in out.items()})
    return out


def check_ff(c, out, ref, level, merge, bound, tag):
    """every output the form writes against fp64 (guards = rows >= M intact), every other output untouched, pad columns exactly zero.  Returns (host tensors, bits)."""
    host = {k: g.host() for k, g in out.items()}
    written = ff_written(level, merge)
    for k, g in out.items():
        if k not in written:
            assert g.untouched(host[k][0]), f"{tag}: {k} belongs to another form and was written"
    Fp = fpad(c.F)
    res, errs = {}, {}
    if level == 0:
        res["h"] = host["h"][0]
        assert bool((res["h"][:, c.F:] == 0).all()), f"{tag}: pad columns of the GEGLU result"
    else:
        hi, lo = decode_plane_image(host["g_planes"][0], c.M, Fp)
        assert bool((hi[:, c.F:].view(torch.int16) == 0).all()) and bool((lo[:, c.F:].view(torch.int16) == 0).all()), f"{tag}: pad columns of the GEGLU planes"
        res["h"] = planes_to_float(hi, lo)
        res["g_sums"] = host["g_sums"][0]
        if Fp - c.F >= 32:
            assert bool((res["g_sums"][(c.F + 31) // 32:] == 0).all()), f"{tag}: sums of an all-pad group"
        if merge == 0:
            res["rowstat"] = host["rowstat"][0]
    res["y"] = host["y"][0]
    if level == 2:
        res["y_planes"] = planes_to_float(*decode_plane_image(host["y_planes"][0], c.M, c.Dout))
        res["y_sums"] = host["y_sums"][0]
    for k, v in res.items():
        r = ref["y"] if k == "y_planes" else ref[k]
        if k in ("g_sums", "y_sums", "rowstat"):
            errs[k + ".0"], errs[k + ".1"] = rel(v[..., 0], r[..., 0]), rel(v[..., 1], r[..., 1])
        else:
            errs[k] = rel(v, r)
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}/{bound.get(k, FLAT_BOUND):.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bound.get(k, FLAT_BOUND), (tag, k, v, bound.get(k, FLAT_BOUND))
    return res, {k: h[1] for k, h in host.items()}


def ff_all_forms(ctx, c, p, ref, bound):
    d = {k: dev(v) for k, v in p.items()}
    results = {}
    for level, merge in FF_FORMS:
        tag = f"muse_ff {c.name} level={level} merge={merge}"
        res, bits = check_ff(c, run_ff(ctx, c, d, level, merge), ref, level, merge, bound, tag)
        torch.cuda.synchronize()
        assert ctx.status() == 0, tag
        again = {k: g.host()[1] for k, g in run_ff(ctx, c, d, level, merge).items()}
        for k in bits:
            assert torch.equal(bits[k], again[k]), f"{tag}: {k} differs between two runs"
        results[(level, merge)] = res
    y0 = results[(0, 0)]["y"]
    for (level, merge), res in results.items():
        if level:   # the folded forms lie within the bound of the un-folded result, and kernel merge and tile merge of one another (their fp64 addition orders differ)
            assert rel(res["y"], y0) < bound.get("y", FLAT_BOUND), (c.name, level, merge, rel(res["y"], y0))
            assert rel(res["y"], results[(level, 1 - merge)]["y"]) < bound.get("y", FLAT_BOUND), (c.name, level, merge)
            assert rel(res["h"], results[(0, 0)]["h"]) < FLAT_BOUND
    assert ctx.status() == 0


@pytest.mark.parametrize("name", [c.name for c in FF_CASES])
def test_muse_ff(ctx, name):
    c = FF[name]
    p = ff_inputs(c)
    ff_all_forms(ctx, c, p, ff_ref(c, p), {})


def test_muse_ff_offset_rows(ctx):
    """GEGLU rows with mean / std near 2: the fold's rstd (acc - mean cs) cancels; bound = 4 x the emulation floor of this input (test_muse_proj_ref_cpu.offset_case)"""
    p, ref, bound = offset_case()
    ff_all_forms(ctx, OFFSET_CASE, p, ref, bound)


def test_muse_ff_refuses_unsupported_arguments(ctx):
    from bevgen_amd import _lib

    c = FF["ff-fold"]
    d = {k: dev(v) for k, v in ff_inputs(c).items()}
    for bad in (dict(level=3), dict(merge=2), dict(block=2)):
        with pytest.raises(_lib.BevgenError, match="op_muse_ff"):
            ctx.op_muse_ff(d["x"], d["w1"], d["gamma3"], d["w4"], d["residual"], **bad)
    with pytest.raises(_lib.BevgenError, match="op_muse_ff"):   # D % 32 != 0
        ctx.op_muse_ff(d["x"][:, :100].contiguous(), d["w1"][:, :100].contiguous(), d["gamma3"], d["w4"], d["residual"])
    assert ctx.status() == 0


# ================================================================================================ LayerNorm to planes
def check_ln_planes(ctx, rows, D, ldy, beta, geglu):
    ldx = 2 * D if geglu else ldy
    x, gamma, b = ln_planes_inputs(rows + 2, D, ldx, beta, geglu)
    ref = ln_planes_ref(x[:rows], gamma, b, D, geglu)
    out = Guarded((rows + 2, ldy // 32, 2, 32), torch.float16)
    ctx.op_layernorm_planes(dev(x), dev(gamma), dev(b), D=D, ldy=ldy, geglu=geglu, planes=out.view, rows=rows)
    img, bits = out.host()
    assert out.untouched(img[rows:]), "rows behind the last one were written"
    hi, lo = decode_plane_image(img[:rows], rows, ldy)
    assert bool((hi[:, D:].view(torch.int16) == 0).all()) and bool((lo[:, D:].view(torch.int16) == 0).all()), "pad columns are not zero"
    err = rel(planes_to_float(hi, lo)[:, :D], ref)
    print(f"layernorm_planes rows={rows} D={D} ldy={ldy} beta={int(beta)} geglu={int(geglu)}: {err:.2e} (bound {LN_PLANES_BOUND:.0e})")
    assert err < LN_PLANES_BOUND
    torch.cuda.synchronize()
    assert ctx.status() == 0


@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("shape", LN_PLANES_SHAPES)
def test_layernorm_planes(ctx, shape, beta):
    check_ln_planes(ctx, *shape, beta, False)


@pytest.mark.parametrize("shape", GEGLU_LN_SHAPES)
def test_geglu_layernorm_planes(ctx, shape):
    check_ln_planes(ctx, *shape, False, True)


# ================================================================================================ staged against direct store forms
def digest_lines(ctx):
    """sha256 of every output buffer (guards included) of the cases whose launches take a staged row-major epilogue; run by the child processes below"""
    lines = []
    for name in STAGED_VS_DIRECT_QKV:
        c = QKV[name]
        for k, g in sorted(run_qkv(ctx, c, qkv_device_inputs(qkv_inputs(c))).items()):
            lines.append(f"digest {name} {k} {hashlib.sha256(g.buf.cpu().view(torch.int16).numpy().tobytes()).hexdigest()}")
    c = FF[STAGED_VS_DIRECT_FF]
    d = {k: dev(v) for k, v in ff_inputs(c).items()}
    for k, g in sorted(run_ff(ctx, c, d, 2, 0).items()):
        lines.append(f"digest {c.name} {k} {hashlib.sha256(g.bits(g.buf.cpu()).numpy().tobytes()).hexdigest()}")
    torch.cuda.synchronize()
    assert ctx.status() == 0
    return lines


def test_staged_and_direct_store_forms_are_bit_identical():
    """gemm_tile's row-major (staged through LDS) epilogues promise "bit-identical, only the store instructions change": the same cases under $BEVGEN_GEMM_RME = 1 and 0
    (read once per process, hence one fresh child process each) must give the same bytes in every output."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = r'''
import sys
sys.path[:0] = [%r, %r]
from bevgen_amd.runtime import Context
from test_muse_proj_ops_gpu import digest_lines
ctx = Context(None, precision="f16x3")
print("\n".join(digest_lines(ctx)))
ctx.close()
''' % (os.path.dirname(here), here)
    outs = []
    for flag in ("1", "0"):
        res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BEVGEN_GEMM_RME=flag), capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        outs.append([l for l in res.stdout.splitlines() if l.startswith("digest")])
    assert len(outs[0]) == len(outs[1]) == 2 * 2 + 2 * 4 + 6 + 7, (len(outs[0]), len(outs[1]))
    differ = [" ".join(a.split()[1:3]) for a, b in zip(outs[0], outs[1]) if a != b]
    print("staged against direct forms: outputs that differ:", differ or "none")
    assert not differ, differ
