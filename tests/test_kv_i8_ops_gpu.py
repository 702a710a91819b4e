"""The int8 KV cache (kv_dtype 2, BEVGEN_KV_I8) at operator level: the writers against the CPU quantiser byte for byte, the per-operator and the fused decode attention
against fp64 attention over the DEQUANTISED cache (storage error is not part of these comparisons: the tolerance is the fp32 mode's 2e-5), the appended row against
the quantiser's definition.  Format and quantiser: tests/kv_i8_ref.py.

Shapes: the writers take those of tests/test_frontend_ops_gpu.py (KV / REPLICATE); the attention kernels take those of tests/test_ops_gpu.py cut to one case per
path of the walk (dense / chunk list, G = 1, 2, 4, fused and split form, key split + combine, the staging boundaries of the fp16 form - int8 rows are never staged,
form 0 and -1 must agree with the same reference) and one BASELINE config 4 shape."""
import math

import pytest
import torch

import kv_i8_ref as Q
from test_frontend_ref_cpu import KV, REPLICATE, gen, kv_inputs
from test_ops_gpu import _ar_attn_reference, dev, rel
from test_vq_ops_gpu import consume_status

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 1024


class GuardedBytes:
    """a flat uint8 cache of `rows` cached rows inside a sentinel-filled buffer with GUARD bytes on both sides"""

    def __init__(self, rows, fill=None):
        self.n = Q.ROW_BYTES * rows
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.n]
        if fill is not None:
            self.view.copy_(fill)

    def host(self):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + self.n:] == SENTINEL).all()), "a byte outside the cache was written"
        return b[GUARD:GUARD + self.n].clone()


def planes(buf, B, H, L):
    """writable views of a flat host buffer: codes int8 [B, H, L, 64], scales fp32 [B, H, L]"""
    rows = B * H * L
    return buf[:64 * rows].view(torch.int8).reshape(B, H, L, 64), buf[64 * rows:].view(torch.float32).reshape(B, H, L)


def expect_rows(c, qkv, n, pos):
    """the sentinel cache with rows [pos, pos + n) of every (b, h) holding the CPU quantiser's codes and scales of the k / v rows of qkv [B n, (q | k | v) 64 H]"""
    t = qkv.reshape(c.B, n, 3, c.H, 64).permute(2, 0, 3, 1, 4)   # [3, B, H, n, 64]
    out = []
    for part in (t[1], t[2]):
        buf = torch.full((Q.ROW_BYTES * c.B * c.H * c.Lmax,), SENTINEL, dtype=torch.uint8)
        codes, scales = planes(buf, c.B, c.H, c.Lmax)
        qc, qs = Q.quantise(part.contiguous())
        codes[:, :, pos:pos + n] = qc
        scales[:, :, pos:pos + n] = qs
        out.append(buf)
    return t[0].contiguous(), out[0], out[1]


# ================================================================================================ writers
@pytest.mark.parametrize("with_q", [False, True], ids=["kv", "qkv"])
@pytest.mark.parametrize("name", list(KV))
def test_kv_i8_scatter(gpu_ctx, name, with_q):
    c = KV[name]
    qkv = kv_inputs(c, c.n)
    qkv[0, c.H * 64: c.H * 64 + 64] = 0.0                    # a zero key row: codes 0, scale 0
    qkv[-1, 2 * c.H * 64: 2 * c.H * 64 + 64] *= 1e-32        # a value row below the 1e-30 threshold
    kc, vc = GuardedBytes(c.B * c.H * c.Lmax), GuardedBytes(c.B * c.H * c.Lmax)
    q = torch.full((c.B, c.H, c.n, 64), 231.625, device="cuda") if with_q else None
    gpu_ctx.op_kv_cache_write("scatter", kc.view, vc.view, kv_dtype=2, B=c.B, H=c.H, Lmax=c.Lmax, qkv=dev(qkv), q=q, n=c.n, pos0=c.pos0)
    rq, rk, rv = expect_rows(c, qkv, c.n, c.pos0)
    assert torch.equal(kc.host(), rk) and torch.equal(vc.host(), rv)      # codes, scales, and the sentinel in every other row of both planes
    if with_q:
        assert torch.equal(q.cpu(), rq)
    consume_status(gpu_ctx, 0, None)


@pytest.mark.parametrize("name", list(KV))
def test_kv_i8_append(gpu_ctx, name):
    """the device-side position plus pos0 lands on the cache's last row"""
    c = KV[name]
    qkv = kv_inputs(c, 1)
    kc, vc = GuardedBytes(c.B * c.H * c.Lmax), GuardedBytes(c.B * c.H * c.Lmax)
    pos = torch.tensor([c.dpos], dtype=torch.int32, device="cuda")
    gpu_ctx.op_kv_cache_write("append", kc.view, vc.view, kv_dtype=2, B=c.B, H=c.H, Lmax=c.Lmax, qkv=dev(qkv), pos0=c.pos0, pos=pos)
    _, rk, rv = expect_rows(c, qkv, 1, c.Lmax - 1)
    assert torch.equal(kc.host(), rk) and torch.equal(vc.host(), rv)
    consume_status(gpu_ctx, 0, None)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_kv_i8_nonfinite_row_raises_its_bit(gpu_ctx, bad):
    from bevgen_amd import _lib

    c = KV["b3-h3-n5-l40"]
    for col in (c.H * 64 + 70, 2 * c.H * 64 + 3):              # a key element of head 1, a value element of head 0
        qkv = kv_inputs(c, c.n).clone()
        qkv[7, col] = bad
        kc, vc = GuardedBytes(c.B * c.H * c.Lmax), GuardedBytes(c.B * c.H * c.Lmax)
        gpu_ctx.op_kv_cache_write("scatter", kc.view, vc.view, kv_dtype=2, B=c.B, H=c.H, Lmax=c.Lmax, qkv=dev(qkv), n=c.n, pos0=c.pos0)
        consume_status(gpu_ctx, _lib.STATUS_KV_NONFINITE, "int8 KV cache")      # this bit and nothing else
    # the largest finite row is representable: no range refusal
    qkv = kv_inputs(c, c.n).clone()
    qkv[7, c.H * 64 + 70] = 3.0e38
    kc, vc = GuardedBytes(c.B * c.H * c.Lmax), GuardedBytes(c.B * c.H * c.Lmax)
    gpu_ctx.op_kv_cache_write("scatter", kc.view, vc.view, kv_dtype=2, B=c.B, H=c.H, Lmax=c.Lmax, qkv=dev(qkv), n=c.n, pos0=c.pos0)
    consume_status(gpu_ctx, 0, None)
    _, rk, _ = expect_rows(c, qkv, c.n, c.pos0)
    assert torch.equal(kc.host(), rk)


@pytest.mark.parametrize("name", list(REPLICATE))
def test_kv_i8_replicate_prefix(gpu_ctx, name):
    """both planes of the first `rows` rows of slot `src` reach the slots [dst0, dst0 + count) of every layer; everything else keeps its bytes"""
    c = REPLICATE[name]
    per_layer = c.B * c.H * c.L
    caches, want = [], []
    for which in range(2):
        layers = [Q.pack(torch.randn(c.B, c.H, c.L, 64, generator=gen(len(name) + which + 10 * l)) * (1 + l)) for l in range(c.layers)]
        caches.append(GuardedBytes(c.layers * per_layer, torch.cat(layers)))
        for buf in layers:
            codes, scales = planes(buf, c.B, c.H, c.L)
            src_c, src_s = codes[c.src, :, :c.rows].clone(), scales[c.src, :, :c.rows].clone()
            for d in range(c.dst0, c.dst0 + c.count):
                if d != c.src:
                    codes[d, :, :c.rows] = src_c
                    scales[d, :, :c.rows] = src_s
        want.append(torch.cat(layers))
    gpu_ctx.op_kv_cache_write("replicate_prefix", caches[0].view, caches[1].view, kv_dtype=2, B=c.B, H=c.H, Lmax=c.L, layers=c.layers, rows=c.rows, src=c.src,
                              dst0=c.dst0, count=c.count)
    assert torch.equal(caches[0].host(), want[0]) and torch.equal(caches[1].host(), want[1])


# ================================================================================================ per-operator decode attention
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,H,n,Lmax", [(1, 2, 1, 64), (2, 4, 77, 128), (3, 16, 600, 640)])
def test_kv_i8_decode_attention(gpu_ctx, B, H, n, Lmax, masked):
    g = torch.Generator().manual_seed(n)
    q = torch.randn(B, H * 64, generator=g)
    kbuf, vbuf = Q.pack(torch.randn(B, H, Lmax, 64, generator=g) * 1.5), Q.pack(torch.randn(B, H, Lmax, 64, generator=g))
    kc, vc = Q.unpack(kbuf, B, H, Lmax)[2], Q.unpack(vbuf, B, H, Lmax)[2]
    bias = torch.randn(Lmax, Lmax, generator=g)
    keep = None
    scale = 0.125
    s = (torch.einsum("bhd,bhjd->bhj", q.reshape(B, H, 64).double(), kc[:, :, :n].double()) + bias[n - 1, :n].double()) * scale
    if masked:
        keep = (torch.rand(H, Lmax, Lmax, generator=g) > 0.3).to(torch.uint8)
        keep[:, :, 0] = 1
        s = s.masked_fill(keep[:, n - 1, :n][None] == 0, float("-inf"))
    ref = torch.einsum("bhj,bhjd->bhd", s.softmax(-1), vc[:, :, :n].double()).reshape(B, H * 64)
    dk, dv = dev(kbuf), dev(vbuf)
    out = gpu_ctx.op_decode_attention(dev(q), dk, dv, n, bias=dev(bias), keep=dev(keep) if masked else None, scale=scale, kv_dtype=2, Lmax=Lmax)
    err = rel(out.cpu().double(), ref)
    print(f"decode_attention i8 B={B} H={H} n={n}: {err:.2e}")
    assert err < 2e-5
    assert torch.equal(dk.cpu(), kbuf) and torch.equal(dv.cpu(), vbuf)     # a read-only call


# ================================================================================================ fused decode attention
class _KeepsItsRows(torch.Tensor):
    """A cache handed to _ar_attn_reference whose row n - 1 already holds the appended row AS THE DEVICE STORED IT: the reference's own `kcd[:, :, n - 1] = k`
    (its exact fp64 row) is ignored, every read sees the stored values."""

    def __setitem__(self, index, value):
        pass


def _run_fused(gpu_ctx, B, G, H, n, Lmax, blk, sparse, split, seed, masked=None, hide_new=False, partials=3):
    D = H * 64
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    partial = torch.randn(partials, B, D, generator=g) * 0.3
    rbias = torch.randn(D, generator=g) * 0.1
    ln_w, ln_b = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.1
    wqkv = torch.randn(3 * D, D, generator=g) / math.sqrt(D)
    bqkv = torch.randn(3 * D, generator=g) * 0.1
    kbuf, vbuf = Q.pack(torch.randn(B, H, Lmax, 64, generator=g)), Q.pack(torch.randn(B, H, Lmax, 64, generator=g) * 2)
    bias = torch.randn(Lmax, Lmax, generator=g)
    prefix = 0 if G == 1 else (48 if n <= 64 else 64)
    mask = layout = None
    if sparse:
        mask = (torch.rand(Lmax, Lmax, generator=g) > 0.2).float()
        layout = (torch.rand(H, Lmax // blk, Lmax // blk, generator=g) < 0.4).long()
        mask[:, 0] = 1
        layout[:, :, 0] = 1
        if sparse == "offset":
            idx = torch.arange(Lmax // blk)
            layout[:, :, 0] = 0
            layout[:, idx, idx] = 1
            mask[torch.arange(Lmax), torch.arange(Lmax)] = 1
    elif masked:
        mask = (torch.rand(Lmax, Lmax, generator=g) > 0.2).float()
        mask[:, 0] = 1
        mask[torch.arange(Lmax), torch.arange(Lmax)] = 0 if hide_new else 1
    dk, dv = dev(kbuf), dev(vbuf)
    out = gpu_ctx.op_ar_attn_fused(dev(x), dev(ln_w), dev(ln_b), dev(wqkv), dev(bqkv), dk, dv, n, partial=dev(partial), rbias=dev(rbias), bias=dev(bias),
                                   attn_mask=None if mask is None else dev(mask), layout=None if layout is None else dev(layout), block=blk, G=G, prefix=prefix,
                                   kv_dtype=2, split=split, Lmax=Lmax)
    consume_status(gpu_ctx, 0, None)
    after = [Q.unpack(t.cpu(), B, H, Lmax) for t in (dk, dv)]
    before = [Q.unpack(t, B, H, Lmax) for t in (kbuf, vbuf)]
    # the reference reads the dequantised cache, the appended row as the device stored it
    stored = [a[2].as_subclass(_KeepsItsRows) for a in after]
    ref, k_new, v_new = _ar_attn_reference(x, partial, rbias, ln_w, ln_b, wqkv, bqkv, stored[0], stored[1], n, bias, mask, layout, blk, G, prefix)
    err = rel(out.cpu().double(), ref)
    print(f"ar_attn_fused i8 B={B} G={G} H={H} n={n} Lmax={Lmax} split={split}: {err:.2e}")
    assert err < 2e-5
    # the appended row against the quantiser's definition
    for (codes, scales, deq), new in zip(after, (k_new, v_new)):
        amax = new.abs().amax(-1)                                            # [B, H] fp64
        s_row, d_row = scales[:, :, n - 1].double(), deq[:, :, n - 1].double()
        assert bool(((s_row - amax / 127.0).abs() <= 1e-5 * amax / 127.0).all())
        assert bool(((d_row - new).abs() <= s_row.unsqueeze(-1) / 2 + 1e-5 * amax.unsqueeze(-1)).all())
        assert int(codes[:, :, n - 1].min()) >= -127
    # every other byte is unchanged
    keep = torch.ones(Lmax, dtype=torch.bool)
    keep[n - 1] = False
    for (c1, s1, _), (c0, s0, _) in zip(after, before):
        assert torch.equal(c1[:, :, keep], c0[:, :, keep]) and torch.equal(s1[:, :, keep].view(torch.int32), s0[:, :, keep].view(torch.int32))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("B,G,H,n,Lmax,blk,sparse", [
    (1, 1, 2, 1, 64, 16, False),        # first key only
    (2, 1, 4, 77, 128, 4, True),        # ragged length, 4-key blocks
    (4, 2, 4, 300, 512, 16, True),      # two sequences per layout sharing a 64-key prefix
    (8, 4, 8, 64, 512, 16, False),      # four per layout, nothing beyond the shared prefix except the new key
    (2, 1, 4, 300, 480, 24, "offset"),  # 24-key blocks, chunk lists that start behind chunk 0
    (3, 1, 16, 600, 640, 16, True),
])
def test_kv_i8_ar_attn_fused(gpu_ctx, B, G, H, n, Lmax, blk, sparse, split):
    """dense and chunk-list walks, G = 1 / 2 / 4, the fused kernel and the attention-only kernel of the split form"""
    _run_fused(gpu_ctx, B, G, H, n, Lmax, blk, sparse, split, seed=B * 1000 + n)


@pytest.mark.parametrize("form", [0, -1])
@pytest.mark.parametrize("B,H,n,Lmax,hide_new", [(3, 8, 128, 256, False), (3, 8, 129, 256, False), (2, 16, 257, 512, False), (2, 4, 2, 64, True), (2, 16, 512, 512, False)])
def test_kv_i8_ar_attn_fused_dense(gpu_ctx, B, H, n, Lmax, hide_new, form):
    """one sequence per workgroup, dense walk, at the context lengths where the fp16 form changes its staging (int8 rows are not staged: form 0 and -1 launch the same
    walk), the new key hidden by the mask, n = L"""
    _run_fused(gpu_ctx, B, 1, H, n, Lmax, 16, False, form, seed=B * 1000 + n, masked=True, hide_new=hide_new, partials=4)


@pytest.mark.parametrize("B,H,n,Lmax,sparse,ks", [(1, 4, 40, 512, False, 4), (1, 4, 1, 128, False, 3), (3, 8, 511, 512, True, 2)])
def test_kv_i8_ar_attn_key_split(gpu_ctx, B, H, n, Lmax, sparse, ks):
    """the attention-only kernel with its key walk cut into ks ranges + the combine kernel"""
    _run_fused(gpu_ctx, B, 1, H, n, Lmax, 16, sparse, ks, seed=B * 77 + n)


def test_kv_i8_ar_attn_fused_config4(gpu_ctx):
    """the launch geometry of the real workload (BASELINE config 4 mid-decode), once"""
    _run_fused(gpu_ctx, 16, 1, 16, 1301, 2368, 16, False, False, seed=16 * 1000 + 1301)
