"""int8 decode weights (decode_weights='i8', BEVGEN_W_I8) at operator level: the quantiser against the CPU one byte for byte, and the three decode kernels that stream
the int8 images - skinny_fused_kernel (bevgen_op_ln_gemm on a context created with decode_weights='i8'), ar_mlp_fused_kernel (bevgen_op_mlp_fused, w_f16 = 2) and
ar_attn_fused_kernel (bevgen_op_ar_attn_fused, w_f16 = 2) - against fp64 on the DEQUANTISED matrices.  Quantisation error is no part of these comparisons: the
bounds are the ones tests/test_ops_gpu.py asserts for the fp16-weight cases of the same operators (6e-6, 8e-6, 2e-5; 2e-5 over the int8 KV cache as
tests/test_kv_i8_ops_gpu.py has it) - the arithmetic is the same, the epilogue gains one fp32 multiply.  Format and quantiser: tests/decode_w_i8_ref.py."""
import math

import pytest
import torch
import torch.nn.functional as F

import decode_w_i8_ref as W
import kv_i8_ref as Q
from test_kv_i8_ops_gpu import _KeepsItsRows
from test_ops_gpu import _ar_attn_reference, dev, rel
from test_vq_ops_gpu import consume_status

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def i8_ctx():
    """a model-less context whose decode_weight_dtype is BEVGEN_W_I8: bevgen_op_ln_gemm follows it"""
    from bevgen_amd.runtime import Context

    ctx = Context(None, decode_weights="i8")
    yield ctx
    ctx.close()


def randw(g, n, k):
    return torch.randn(n, k, generator=g) / math.sqrt(k)


# ================================================================================================ the quantiser
def _special_matrix():
    """K = 256: a zero row, a row of one repeated (negative) value, a row whose codes are exactly -127 .. 127 (then one zero), a row below the 1e-30 threshold,
    and random rows around them"""
    g = torch.Generator().manual_seed(11)
    w = randw(g, 8, 256)
    w[1] = 0.0
    w[3] = -0.3125
    w[5] = torch.cat([torch.arange(-127, 128, dtype=torch.float32), torch.zeros(1)]) * 0.01
    w[6] *= 1e-33 / w[6].abs().max()
    return w


@pytest.mark.parametrize("name", ["48x256", "1024x1024", "special"])
def test_quantize_rows_matches_the_cpu_quantiser_byte_for_byte(gpu_ctx, name):
    if name == "special":
        w, rows = _special_matrix(), slice(0, 8)
    elif name == "48x256":
        w, rows = randw(torch.Generator().manual_seed(1), 48, 256) * 3.0, slice(0, 48)
    else:
        g = torch.Generator().manual_seed(2)
        w, rows = randw(g, 1024, 1024) * torch.exp(torch.randn(1024, 1, generator=g)), slice(0, 64)   # (compared on rows 0-63)
    codes, scales, deq = gpu_ctx.op_quantize_rows_i8(dev(w))
    consume_status(gpu_ctx, 0, None)
    rc, rs, rd = W.quantise_rows(w[rows])
    assert torch.equal(codes.cpu()[rows], rc.to(torch.int8))
    assert torch.equal(scales.cpu()[rows].view(torch.int32), rs.view(torch.int32))
    assert torch.equal(deq.cpu()[rows].view(torch.int32), rd.view(torch.int32))
    if name == "special":
        c = codes.cpu()
        assert bool((c[1] == 0).all()) and float(scales[1]) == 0.0 and bool((c[6] == 0).all()) and float(scales[6]) == 0.0
        assert bool((c[3] == -127).all())
        assert torch.equal(c[5, :255].to(torch.int32), torch.arange(-127, 128, dtype=torch.int32)) and int(c[5, 255]) == 0
    # in place: the dequantised values may overwrite the matrix (bevgen_finalize replaces the master weights this way)
    dw = dev(w)
    codes2 = torch.empty_like(codes)
    scales2 = torch.empty_like(scales)
    from bevgen_amd.runtime import _ptr

    gpu_ctx._check(gpu_ctx.lib.bevgen_op_quantize_rows_i8(gpu_ctx._h, _ptr(dw), w.shape[0], w.shape[1], _ptr(codes2), _ptr(scales2), _ptr(dw), gpu_ctx._s()))
    assert torch.equal(dw, deq) and torch.equal(codes2, codes) and torch.equal(scales2, scales)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_quantize_rows_flags_a_nonfinite_row(gpu_ctx, bad):
    from bevgen_amd import _lib

    w = randw(torch.Generator().manual_seed(3), 5, 256)
    w[3, 77] = bad
    gpu_ctx.op_quantize_rows_i8(dev(w))
    consume_status(gpu_ctx, _lib.STATUS_F16_RANGE, "device status word")


# ================================================================================================ skinny_fused_kernel
LN_GEMM_M = (1, 5, 16, 33, 64)


@pytest.mark.parametrize("K", [256, 1024, 4096])
@pytest.mark.parametrize("N", [16, 40, 768])      # 40: not a multiple of the 16-column tile
def test_ln_gemm_int8_weights(i8_ctx, N, K):
    """Every form the decode step launches: plain and LayerNorm-ed A, the folded LayerNorm (ksplit = -1), GELU, K split over workgroups (the partial sums added on the
    host: every partial carries the column's scale).  The matrix holds a row whose codes span -127 .. 127 (the sign extension of the conversion) and a zero row."""
    g = torch.Generator().manual_seed(N * 7 + K)
    w = randw(g, N, K) * torch.exp(0.5 * torch.randn(N, 1, generator=g))      # rows of different scale
    w[1] = 0.0
    w[2, :255] = torch.arange(-127, 128, dtype=torch.float32) * 0.003
    w[2, 255:] = 0.0
    wd = W.quantise_rows(w)[2].double()
    assert torch.equal(W.quantise_rows(w)[0][2, :255], torch.arange(-127, 128, dtype=torch.float32))
    b = torch.randn(N, generator=g) * 0.2
    lw, lb = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.1
    a_all = torch.randn(max(LN_GEMM_M), K, generator=g) * 1.7 + 0.3
    dw, db, dlw, dlb = dev(w), dev(b), dev(lw), dev(lb)
    ln_ok = K <= 1024                                                         # (LayerNorm needs the whole row in one workgroup: K <= 1024)
    ksplits = {256: (0,), 1024: (0, 2, 4), 4096: (0,)}[K]                     # 0 = the library's choice (4 at K = 4096); explicit splits: slices of 512 and 256
    worst = {}
    for M in LN_GEMM_M:
        a = a_all[:M]
        da = dev(a)
        plain = a.double() @ wd.t()
        for ks in ksplits:
            out = i8_ctx.op_ln_gemm(da, dw, ksplit=ks)
            worst["plain"] = max(worst.get("plain", 0.0), rel(out.cpu().double(), plain))
        if ln_ok:
            h = F.layer_norm(a.double(), (K,), lw.double(), lb.double(), 1e-5) @ wd.t() + b.double()
            for gelu in (False, True):
                ref = F.gelu(h) if gelu else h
                for ks, tag in ((0, "ln"), (-1, "folded")):
                    out = i8_ctx.op_ln_gemm(da, dw, ln_w=dlw, ln_b=dlb, bias=db, gelu=gelu, ksplit=ks)
                    worst[tag] = max(worst.get(tag, 0.0), rel(out.cpu().double(), ref))
    consume_status(i8_ctx, 0, None)
    print(f"ln_gemm int8 N={N} K={K}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v < 6e-6 for v in worst.values()), worst


def test_ln_gemm_on_an_fp32_context_is_unchanged(gpu_ctx, i8_ctx):
    """the operator follows the CONTEXT's mode: the default context multiplies by the matrix it is given, the int8 one by its quantised image"""
    g = torch.Generator().manual_seed(5)
    a, w = torch.randn(16, 256, generator=g), randw(g, 64, 256)
    exact = a.double() @ w.double().t()
    assert rel(gpu_ctx.op_ln_gemm(dev(a), dev(w)).cpu().double(), exact) < 6e-6
    assert rel(i8_ctx.op_ln_gemm(dev(a), dev(w)).cpu().double(), exact) > 1e-4           # quantisation error: ~1e-2 here


# ================================================================================================ ar_mlp_fused_kernel
@pytest.mark.parametrize("M", [5, 16, 64])
def test_mlp_fused_int8_weights(gpu_ctx, M):
    D = 1024
    g = torch.Generator().manual_seed(7 * M + D + 2)
    x = torch.randn(M, D, generator=g) * 1.3 + 0.2
    lw, lb = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.1
    w1, b1 = randw(g, 4 * D, D) * torch.exp(0.5 * torch.randn(4 * D, 1, generator=g)), torch.randn(4 * D, generator=g) * 0.2
    w2, b2 = randw(g, D, 4 * D) * torch.exp(0.5 * torch.randn(D, 1, generator=g)), torch.randn(D, generator=g) * 0.2
    w1[3, :255] = torch.arange(-127, 128, dtype=torch.float32) * 0.002        # codes -127 .. 127 in both matrices
    w2[9, 4 * D - 255:] = torch.arange(-127, 128, dtype=torch.float32) * 0.001
    w1d, w2d = W.quantise_rows(w1)[2].double(), W.quantise_rows(w2)[2].double()
    h = F.layer_norm(x.double(), (D,), lw.double(), lb.double(), 1e-5)
    ref = F.gelu(h @ w1d.t() + b1.double()) @ w2d.t() + b2.double()
    args = [dev(t) for t in (x, lw, lb, w1, b1, w2, b2)]
    out = gpu_ctx.op_mlp_fused(*args, w_f16=2)
    err = rel(out.cpu().double(), ref)
    print(f"mlp_fused int8 M={M}: {err:.2e}")
    assert err < 8e-6
    out2 = gpu_ctx.op_mlp_fused(*args, w_f16=2)
    assert torch.equal(out, out2), "two launches of the same operator differ"


# ================================================================================================ ar_attn_fused_kernel
def _run_attn(gpu_ctx, B, G, H, n, Lmax, form, kv, seed):
    D = H * 64
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    partial = torch.randn(4, B, D, generator=g) * 0.3
    rbias = torch.randn(D, generator=g) * 0.1
    ln_w, ln_b = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.1
    wqkv = randw(g, 3 * D, D) * torch.exp(0.5 * torch.randn(3 * D, 1, generator=g))
    wqkv[70, :255] = torch.arange(-127, 128, dtype=torch.float32) * 0.002     # a q row, a k row and a v row whose codes span -127 .. 127
    wqkv[D + 5, :255] = torch.arange(127, -128, -1, dtype=torch.float32) * 0.002
    wqkv[2 * D + 64, :255] = torch.arange(-127, 128, dtype=torch.float32) * 0.003
    bqkv = torch.randn(3 * D, generator=g) * 0.1
    wd = W.quantise_rows(wqkv)[2]
    bias = torch.randn(Lmax, Lmax, generator=g)
    prefix = 0 if G == 1 else 64
    kc, vc = torch.randn(B, H, Lmax, 64, generator=g), torch.randn(B, H, Lmax, 64, generator=g) * 2
    common = dict(partial=dev(partial), rbias=dev(rbias), bias=dev(bias), G=G, prefix=prefix, w_f16=2, split=form)
    if kv == 2:
        kbuf, vbuf = Q.pack(kc), Q.pack(vc)
        dk, dv = dev(kbuf), dev(vbuf)
        out = gpu_ctx.op_ar_attn_fused(dev(x), dev(ln_w), dev(ln_b), dev(wqkv), dev(bqkv), dk, dv, n, kv_dtype=2, Lmax=Lmax, **common)
        stored = [Q.unpack(t.cpu(), B, H, Lmax)[2].as_subclass(_KeepsItsRows) for t in (dk, dv)]   # the dequantised cache, the appended row as the device stored it
        ref, _, _ = _ar_attn_reference(x, partial, rbias, ln_w, ln_b, wd, bqkv, stored[0], stored[1], n, bias, None, None, 16, G, prefix)
    else:
        dk, dv = dev(kc), dev(vc)
        out = gpu_ctx.op_ar_attn_fused(dev(x), dev(ln_w), dev(ln_b), dev(wqkv), dev(bqkv), dk, dv, n, kv_dtype=0, **common)
        ref, k_new, v_new = _ar_attn_reference(x, partial, rbias, ln_w, ln_b, wd, bqkv, kc, vc, n, bias, None, None, 16, G, prefix)
        assert rel(dk[:, :, n - 1].cpu().double(), k_new) < 1e-5 and rel(dv[:, :, n - 1].cpu().double(), v_new) < 1e-5
    consume_status(gpu_ctx, 0, None)
    err = rel(out.cpu().double(), ref)
    print(f"ar_attn_fused int8 weights B={B} G={G} H={H} n={n} form={form} kv_dtype={kv}: {err:.2e}")
    assert err < 2e-5


@pytest.mark.parametrize("kv", [0, 2])
@pytest.mark.parametrize("form", [0, -1, 1, 2])   # the fused kernel with / without staged K/V pieces, the split form (LayerNorm + QKV kernel on the packed int8 image), its key split
def test_ar_attn_fused_int8_weights(gpu_ctx, form, kv):
    """(3, 8, 129, 256): the smallest shape tests/test_ops_gpu.py::test_ar_attn_fused2_operator runs with fp16 weights"""
    _run_attn(gpu_ctx, 3, 1, 8, 129, 256, form, kv, seed=3129)


@pytest.mark.parametrize("kv", [0, 2])
@pytest.mark.parametrize("form", [0, 1])
def test_ar_attn_fused_int8_weights_two_sequences_per_layout(gpu_ctx, form, kv):
    """(4, G = 2, H = 4, 300, 512): that file's shared-prefix shape; D = 256 is the narrowest width the mode admits"""
    _run_attn(gpu_ctx, 4, 2, 4, 300, 512, form, kv, seed=4300)


# ================================================================================================ refusals
def test_refusals_without_a_launch(gpu_ctx, i8_ctx):
    g = torch.Generator().manual_seed(9)
    D = 1024
    x, lw, lb = dev(torch.randn(4, D, generator=g)), dev(torch.ones(D)), dev(torch.zeros(D))
    w1, b1, w2, b2 = dev(randw(g, 4 * D, D)), dev(torch.zeros(4 * D)), dev(randw(g, D, 4 * D)), dev(torch.zeros(D))
    with pytest.raises(Exception, match="w_f16 = 3"):
        gpu_ctx.op_mlp_fused(x, lw, lb, w1, b1, w2, b2, w_f16=3)
    H, Lmax = 2, 64                                       # D = 128: a multiple of 8 (the fused kernel runs) but not of 256 (the split form's packed image refuses, as for fp16)
    Dn = H * 64
    xs, lws, lbs = dev(torch.randn(2, Dn, generator=g)), dev(torch.ones(Dn)), dev(torch.zeros(Dn))
    wq, bq = dev(randw(g, 3 * Dn, Dn)), dev(torch.zeros(3 * Dn))
    kc, vc = dev(torch.randn(2, H, Lmax, 64, generator=g)), dev(torch.randn(2, H, Lmax, 64, generator=g))
    with pytest.raises(Exception, match="w_f16 = 3"):
        gpu_ctx.op_ar_attn_fused(xs, lws, lbs, wq, bq, kc, vc, 5, w_f16=3)
    for wf in (1, 2):
        with pytest.raises(Exception, match="split form does not support"):
            gpu_ctx.op_ar_attn_fused(xs, lws, lbs, wq, bq, kc, vc, 5, w_f16=wf, split=1)
    before = kc.clone()
    gpu_ctx.op_ar_attn_fused(xs, lws, lbs, wq, bq, kc, vc, 5, w_f16=2)                       # the fused form at D = 128 runs
    assert not torch.equal(kc[:, :, 4], before[:, :, 4]) and torch.equal(kc[:, :, :4], before[:, :, :4])
    # the skinny kernel's int8 image needs K slices of 256 (32 per wave), like the fp16 one: K = 128 runs in fp32 and is refused in int8
    a, w = dev(torch.randn(4, 128, generator=g)), dev(randw(g, 32, 128))
    gpu_ctx.op_ln_gemm(a, w)
    with pytest.raises(Exception, match="int8 weights need a K slice"):
        i8_ctx.op_ln_gemm(a, w)
    consume_status(gpu_ctx, 0, None)
    consume_status(i8_ctx, 0, None)
