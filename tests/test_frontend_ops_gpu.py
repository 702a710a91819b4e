"""Operator-level parity of the kernels around the layer stacks, each through the launcher the model calls: the embedding kernels and Route M's fp32 q / k / v
preparation (bevgen_amd/csrc/embed.hip), the KV-cache writers, the setup tables and row helpers (tables.hip), the key-tile lists and the tile-list path of the
flash-attention kernel (attention.hip) - through bevgen_op_camera_embed, _cond_embed, _token_rows, _muse_qkv_prep_f32, _kv_cache_write, _attn_tables and
_attention_tiles.  Case tables, inputs, references and bounds: tests/test_frontend_ref_cpu.py.

Every output buffer starts as a sentinel with a guard region on both sides: what a case must not write (cache rows outside [pos, pos + n), key rows behind the last
token, list slots behind the count, rows around a decode-order range, the guards) must still hold the sentinel bit for bit.

Exact (bit equality with the fp32 / integer reference): token, step and sequence rows, gathers, store_tokens, every table, the value half of the key / value
preparation, both cache dtypes, the condition rows without the grid term.  Bounded, per row max |out - ref64| / max |ref64|, bound = 4 x e_cpu (the fp32 torch
evaluation's own error, test_frontend_ref_cpu.e_cpu, recomputed where the tests run: its last digits follow the host's torch); worst error measured on an MI355X beside
it (each test prints its own, `pytest -s`):
  kernel                          e_cpu     bound     measured
  camera_embed, img               2.2e-7    8.7e-7    1.9e-7   (2.1e-7 / 8.3e-7 with another host's torch kernels)
  camera_embed, c_embed           1.2e-7    4.6e-7    1.4e-7
  cond_embed with the grid        1.6e-7    6.3e-7    1.6e-7
  muse_qkv_prep_f32, q            1.7e-7    6.8e-7    1.2e-7
  muse_qkv_prep_f32, k            1.5e-7    5.8e-7    1.6e-7
  attention through tile lists    -         5e-6      2.4e-7 (the whole-tensor metric and bound of test_attention); with against without the list: bit-identical (bound 2e-6)
Everything listed as exact was bit-equal on the MI355X.

The chunk lists of block sizes 20, 24 and 40 failed here until build_layout_kernel probed every block a 16-key chunk overlaps.  One-line source mutations tried once in a
scratch build, and the tests of this module they fail: r (r + 1) / 2 -> r (r - 1) / 2 in the triangular scatter 4; j - 1 -> j in build_muse_bias 3; present[c / KT] ->
present[min(c / KT + 1, nt - 1)] in the tile builder 9; pos0 + i -> pos0 + i + 1 in the cache scatter 19; vocab_rows - 1 -> vocab_rows - 2 in token_embed's clamp 4; the
camera embedding without its - ce term 4; the chunk probe as it was 7 (and the 24-key decode-attention cases of test_ops_gpu.py).
"""
import pytest
import torch

from test_frontend_ref_cpu import (ATTN, ATTN_BIAS_L, ATTN_BOUND, ATTN_LIST_VS_DENSE, ATTN_SCALE, CAMERA, COND, F16_BAD, F16_FINITE, KV, LAYOUT, MASK_SCALE, MASKED, MUSE_BIAS,
                                   PREP, REPLICATE, TILES, TOKEN, VOCAB, attn_bias_inputs, attn_bias_ref, attn_inputs, attn_ref, camera_inputs, camera_ref, chunk_lists_ref,
                                   cond_inputs, cond_ref, gen, gpu_bound, kv_inputs, kv_scatter_ref, layout_inputs, masked_bias_ref, masked_inputs, muse_bias_ref,
                                   nk_pad, pack_lists, prep_inputs, prep_ref, rel, replicate_ref, row_err, seq_ref, tile_lists_ref, tiles_inputs, token_inputs, token_ref)

pytestmark = pytest.mark.gpu

GUARD = 1024                    # elements in front of and behind every output tensor (a multiple of 8: the tensors stay 16-byte aligned)
SENTINEL = {torch.float32: 231.625, torch.float16: 231.625, torch.int64: -777, torch.uint8: 0xA5, torch.int16: 0x5A5A}
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.int64: torch.int64, torch.uint8: torch.uint8, torch.int16: torch.int16}


def dev(t):
    return None if t is None else t.cuda().contiguous()


class Guarded:
    """an output tensor inside a sentinel-filled buffer with GUARD elements on both sides (uint16 tables are held as int16: their values stay below 2^15)"""

    def __init__(self, shape, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.shape, self.n, self.dtype = tuple(shape), n, dtype
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n].view(self.shape)

    def host(self):
        """the tensor on the host - after asserting that both guards are intact"""
        b = self.buf.cpu()
        s = torch.full((1,), SENTINEL[self.dtype], dtype=self.dtype).view(BITS[self.dtype])
        bits = b.view(BITS[self.dtype])
        assert bool((bits[:GUARD] == s).all()) and bool((bits[GUARD + self.n:] == s).all()), "an element outside the tensor was written"
        return b[GUARD:GUARD + self.n].view(self.shape)

    def untouched(self, t):
        return bool((t.contiguous().view(BITS[self.dtype]) == torch.full((1,), SENTINEL[self.dtype], dtype=self.dtype).view(BITS[self.dtype])).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def consume_status(ctx, bit, text):
    from test_vq_ops_gpu import consume_status as consume

    consume(ctx, bit, text)


def refused(match):
    from bevgen_amd import _lib

    return pytest.raises(_lib.BevgenError, match=match)


# ================================================================================================ camera embedding
@pytest.mark.parametrize("name", list(CAMERA))
def test_camera_embed(gpu_ctx, name):
    c, p = CAMERA[name], camera_inputs(name)
    T = c.h * c.w
    d = {k: dev(p[k]) for k in ("I_inv", "E_inv", "plane", "Wimg", "Wcam")}
    runs = []
    for _ in range(2):
        img, ce = Guarded((c.B, c.C, T, c.D)), Guarded((c.B, c.C, c.D))
        gpu_ctx.op_camera_embed(d["I_inv"], d["E_inv"], d["plane"], d["Wimg"], d["Wcam"], img.view, ce.view)
        runs.append((img.host(), ce.host()))
    (img, ce), again = runs
    assert same_bits(img, again[0]) and same_bits(ce, again[1])
    ref_img, ref_ce = camera_ref(p, torch.float64)
    e_img, e_ce = row_err(img, ref_img), row_err(ce, ref_ce)       # c_embed: the t == T block alone, E_inv[..., 3] through cam_embed
    print(f"camera_embed {name}: img {e_img:.2e} (bound {gpu_bound('camera_img'):.2e}), c_embed {e_ce:.2e} (bound {gpu_bound('camera_c_embed'):.2e})")
    assert bool(img.isfinite().all()) and bool(ce.isfinite().all())
    assert e_img < gpu_bound("camera_img") and e_ce < gpu_bound("camera_c_embed")
    if c.zero_cols == "all":
        assert img.abs().max() == 0 and ce.abs().max() == 0        # 0 / (sqrt(0) + 1e-7)
    else:
        # |e| / (|e| + 1e-7) with |e| > 0.3 here is within 3.4e-7 of 1; the division, the square root and the sum of squares add a few 2^-24
        assert (img.double().norm(dim=-1) - 1).abs().max() < 1e-6
        for o in c.zero_cols:
            assert img[..., o].abs().max() == 0 and ce[..., o].abs().max() == 0
    assert gpu_ctx.status() == 0


# ================================================================================================ condition embedding
@pytest.mark.parametrize("grid", [False, True], ids=["plain", "grid"])
@pytest.mark.parametrize("name", list(COND))
def test_cond_embed(gpu_ctx, name, grid):
    c, p = COND[name], cond_inputs(name)
    d = {k: dev(v) for k, v in p.items()}
    out = Guarded((c.B, c.K, c.D))
    if grid:
        gpu_ctx.op_cond_embed(d["ids"], d["tok"], d["pos"], out.view, bev_grid=d["grid"], wbev=d["Wbev"], bbev=d["bbev"], bev_cam_pos=d["cam_pos"], c_embed=d["c_embed"])
        err = row_err(out.host(), cond_ref(p, torch.float64, True))
        print(f"cond_embed {name}: {err:.2e} (bound {gpu_bound('cond_embed'):.2e})")
        assert err < gpu_bound("cond_embed")
    else:
        gpu_ctx.op_cond_embed(d["ids"], d["tok"], d["pos"], out.view, C=c.C)
        assert same_bits(out.host(), cond_ref(p, torch.float32, False))          # one fp32 add
    assert gpu_ctx.status() == 0


# ================================================================================================ token rows
@pytest.mark.parametrize("img", [False, True], ids=["plain", "img"])
@pytest.mark.parametrize("name", list(TOKEN))
def test_token_embed(gpu_ctx, name, img):
    c, p = TOKEN[name], token_inputs(name)
    N = c.C * c.T
    d = {k: dev(v) for k, v in p.items()}
    out = Guarded((c.B, N, c.D))
    gpu_ctx.op_token_rows("token_embed", out.view, ids=d["ids"], table=d["tok"], img=d["img"] if img else None, pos=d["pos"], B=c.B, N=N, D=c.D, vocab_rows=VOCAB + 1)
    assert same_bits(out.host(), token_ref(p, torch.float32, img))               # (tok + img) + pos: two fp32 adds in the written order


@pytest.mark.parametrize("img", [False, True], ids=["plain", "img"])
@pytest.mark.parametrize("name", list(TOKEN))
def test_ar_step_and_seq_embed(gpu_ctx, name, img):
    c, p = TOKEN[name], token_inputs(name)
    N = c.C * c.T
    d = {k: dev(v) for k, v in p.items()}
    dimg = d["img"] if img else None
    ref = seq_ref(p, torch.float32, img, c.n_steps)                              # [B, n_steps, D]
    rows = c.K + c.n_steps + 2                                                   # row0 = K > 0 and two rows behind the range
    seq = Guarded((c.B, rows, c.D))
    gpu_ctx.op_token_rows("ar_seq_embed", seq.view, ids=d["ids"], table=d["tok"], img=dimg, pos=d["pos"], fwd_idx=d["fwd"], B=c.B, N=N, D=c.D, vocab_rows=VOCAB + 1,
                          n_steps=c.n_steps, rows_per_seq=rows, row0=c.K)
    hs = seq.host()
    assert same_bits(hs[:, c.K:c.K + c.n_steps], ref)
    assert seq.untouched(hs[:, :c.K]) and seq.untouched(hs[:, c.K + c.n_steps:])
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    for s in c.steps:
        step.fill_(s)
        tok = dev(p["ids"][:, p["fwd"][s]])
        x = Guarded((c.B, c.D))
        gpu_ctx.op_token_rows("ar_step_embed", x.view, ids=tok, table=d["tok"], img=dimg, pos=d["pos"], fwd_idx=d["fwd"], step=step, B=c.B, D=c.D, vocab_rows=VOCAB + 1,
                              C_=c.C, T=c.T)
        hx = x.host()
        assert same_bits(hx, hs[:, c.K + s]), f"step {s}: the step kernel's row differs from the sequence kernel's"
        assert same_bits(hx, ref[:, s])


@pytest.mark.parametrize("B,rows,row,D", [(1, 3, 2, 100), (3, 5, 0, 1024), (3, 4, 3, 64)])
def test_gather_rows(gpu_ctx, B, rows, row, D):
    x = torch.randn(B, rows, D, generator=gen(B + D))
    out = Guarded((B, D))
    gpu_ctx.op_token_rows("gather_rows", out.view, table=dev(x), B=B, D=D, rows_per_seq=rows, row0=row)
    assert same_bits(out.host(), x[:, row])


@pytest.mark.parametrize("name", list(TOKEN))
def test_store_tokens(gpu_ctx, name):
    c, p = TOKEN[name], token_inputs(name)
    N = c.C * c.T
    out = Guarded((c.B, N), torch.int64)
    want = torch.full((c.B, N), SENTINEL[torch.int64], dtype=torch.int64)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    fwd = dev(p["fwd"])
    for s in c.steps:
        step.fill_(s)
        tok = torch.randint(0, VOCAB, (c.B,), generator=gen(s)) + 100 * s
        gpu_ctx.op_token_rows("store_tokens", out.view, ids=dev(tok), fwd_idx=fwd, step=step, B=c.B, N=N)
        want[:, p["fwd"][s]] = tok
    assert torch.equal(out.host(), want)                                          # the other slots still hold the sentinel


def test_token_rows_refuse_a_width_that_is_no_multiple_of_4(gpu_ctx):
    ids = torch.zeros(1, 2, dtype=torch.int64, device="cuda")
    tok, pos, fwd = torch.zeros(3, 6, device="cuda"), torch.zeros(2, 6, device="cuda"), torch.arange(2, device="cuda")
    out = Guarded((1, 4, 6))
    with refused("multiple of 4"):
        gpu_ctx.op_token_rows("token_embed", out.view, ids=ids, table=tok, pos=pos, B=1, N=2, D=6, vocab_rows=3)
    with refused("multiple of 4"):
        gpu_ctx.op_token_rows("ar_seq_embed", out.view, ids=ids, table=tok, pos=pos, fwd_idx=fwd, B=1, N=2, D=6, vocab_rows=3, n_steps=2, rows_per_seq=4, row0=1)
    assert out.untouched(out.host())


# ================================================================================================ Route M fp32 q / k / v preparation
@pytest.mark.parametrize("name", list(PREP))
def test_muse_qkv_prep_f32(gpu_ctx, name):
    c, p = PREP[name], prep_inputs(name)
    pad = nk_pad(c.Nk)
    d = {k: dev(v) for k, v in p.items()}
    q, k, v = Guarded((c.B, c.H, c.Nq, 64)), Guarded((c.B, c.H, pad, 64)), Guarded((c.B, c.H, pad, 64))
    gpu_ctx.op_muse_qkv_prep_f32(B=c.B, H=c.H, qraw=d["qraw"], kvraw=d["kvraw"], null_kv=d["null_kv"], q_scale=d["q_scale"], k_scale=d["k_scale"], q=q.view, k=k.view,
                                 v=v.view, Nq=c.Nq, Nk=c.Nk, Nk_pad=pad)
    hq, hk, hv = q.host(), k.host(), v.host()
    rq, rk, rv = prep_ref(c, p, torch.float64)
    eq, ek = row_err(hq, rq), row_err(hk[:, :, :c.Nk + 1], rk)                   # a zero raw row must come out as exact zeros (row_err)
    print(f"muse_qkv_prep_f32 {name}: q {eq:.2e} (bound {gpu_bound('prep_q'):.2e}), k {ek:.2e} (bound {gpu_bound('prep_k'):.2e})")
    assert eq < gpu_bound("prep_q") and ek < gpu_bound("prep_k")
    assert same_bits(hv[:, :, :c.Nk + 1], prep_ref(c, p, torch.float32)[2].contiguous())   # values are copied; row 0 of every (batch, head) is the null value
    assert same_bits(hv[:, :, 0], p["null_kv"][1][None].expand(c.B, -1, -1).contiguous())
    assert k.untouched(hk[:, :, c.Nk + 1:]) and v.untouched(hv[:, :, c.Nk + 1:])


# ================================================================================================ KV-cache writers
def cache_pair(c, dtype, layers=None):
    shape = (c.B, c.H, c.Lmax, 64) if layers is None else (layers, c.B, c.H, c.L, 64)
    return Guarded(shape, dtype), Guarded(shape, dtype)


@pytest.mark.parametrize("with_q", [False, True], ids=["kv", "qkv"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", list(KV))
def test_kv_cache_scatter(gpu_ctx, name, dtype, with_q):
    c = KV[name]
    qkv = kv_inputs(c, c.n)
    kc, vc = cache_pair(c, dtype)
    q = Guarded((c.B, c.H, c.n, 64)) if with_q else None
    gpu_ctx.op_kv_cache_write("scatter", kc.view, vc.view, kv_dtype=int(dtype == torch.float16), B=c.B, H=c.H, Lmax=c.Lmax, qkv=dev(qkv), q=q.view if with_q else None,
                              n=c.n, pos0=c.pos0)
    blank = torch.full((c.B, c.H, c.Lmax, 64), SENTINEL[dtype], dtype=dtype)
    rq, rk, rv = kv_scatter_ref(c, qkv, c.n, c.pos0, blank, blank)
    assert same_bits(kc.host(), rk) and same_bits(vc.host(), rv)                 # rows [pos0, pos0 + n) in the cache's rounding, every other row the sentinel
    if with_q:
        assert same_bits(q.host(), rq)
    consume_status(gpu_ctx, 0, None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", list(KV))
def test_kv_cache_append(gpu_ctx, name, dtype):
    """the device-side position plus pos0 lands on the cache's last row"""
    c = KV[name]
    qkv = kv_inputs(c, 1)
    kc, vc = cache_pair(c, dtype)
    pos = torch.tensor([c.dpos], dtype=torch.int32, device="cuda")
    gpu_ctx.op_kv_cache_write("append", kc.view, vc.view, kv_dtype=int(dtype == torch.float16), B=c.B, H=c.H, Lmax=c.Lmax, qkv=dev(qkv), pos0=c.pos0, pos=pos)
    blank = torch.full((c.B, c.H, c.Lmax, 64), SENTINEL[dtype], dtype=dtype)
    _, rk, rv = kv_scatter_ref(c, qkv, 1, c.Lmax - 1, blank, blank)
    assert same_bits(kc.host(), rk) and same_bits(vc.host(), rv)
    consume_status(gpu_ctx, 0, None)


def test_kv_cache_f16_range(gpu_ctx):
    from bevgen_amd import _lib

    c = KV["b3-h3-n5-l40"]
    base = kv_inputs(c, c.n)

    def run(value, dtype, col):
        qkv = base.clone()
        qkv[7, col] = value
        kc, vc = cache_pair(c, dtype)
        gpu_ctx.op_kv_cache_write("scatter", kc.view, vc.view, kv_dtype=int(dtype == torch.float16), B=c.B, H=c.H, Lmax=c.Lmax, qkv=dev(qkv), n=c.n, pos0=c.pos0)
        return kc.host(), vc.host()

    kcol, vcol = c.H * 64 + 70, 2 * c.H * 64 + 3                                 # a key element of head 1, a value element of head 0 (row 7 = batch 1, i = 2)
    for x in F16_FINITE:
        hk, hv = run(x, torch.float16, kcol)
        consume_status(gpu_ctx, 0, None)
        assert hk[1, 1, c.pos0 + 2, 6] == torch.tensor(x).half() and bool(hk[:, :, c.pos0:].float().isfinite().all())
    for x in F16_BAD:
        for col in (kcol, vcol):
            run(x, torch.float16, col)
            consume_status(gpu_ctx, _lib.STATUS_F16_RANGE, "f16 operand")
        hk, _ = run(x, torch.float32, kcol)                                       # the fp32 cache stores anything and never raises
        consume_status(gpu_ctx, 0, None)
        assert same_bits(hk[1, 1, c.pos0 + 2, 6], torch.tensor(x))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", list(REPLICATE))
def test_replicate_prefix(gpu_ctx, name, dtype):
    c = REPLICATE[name]
    kc, vc = cache_pair(c, dtype, layers=c.layers)
    k0 = torch.randn(kc.shape, generator=gen(len(name))).to(dtype)
    v0 = torch.randn(kc.shape, generator=gen(len(name) + 1)).to(dtype)
    kc.view.copy_(k0)
    vc.view.copy_(v0)
    gpu_ctx.op_kv_cache_write("replicate_prefix", kc.view, vc.view, kv_dtype=int(dtype == torch.float16), B=c.B, H=c.H, Lmax=c.L, layers=c.layers, rows=c.rows, src=c.src,
                              dst0=c.dst0, count=c.count)
    assert same_bits(kc.host(), replicate_ref(c, k0)) and same_bits(vc.host(), replicate_ref(c, v0))   # rows >= rows and slots outside the range keep their values


# ================================================================================================ tables
@pytest.mark.parametrize("use_prob", [False, True], ids=["noprob", "prob"])
@pytest.mark.parametrize("use_emb", [False, True], ids=["noemb", "emb"])
@pytest.mark.parametrize("L", ATTN_BIAS_L)
def test_attn_bias(gpu_ctx, L, use_emb, use_prob):
    emb, prob = attn_bias_inputs(L)
    out = Guarded((L, L))
    gpu_ctx.op_attn_tables("attn_bias", out.view, in0=dev(emb) if use_emb else None, in1=dev(prob) if use_prob else None, L=L)
    assert same_bits(out.host(), attn_bias_ref(emb if use_emb else None, prob if use_prob else None, L))


@pytest.mark.parametrize("name", list(MUSE_BIAS))
def test_muse_bias(gpu_ctx, name):
    c = MUSE_BIAS[name]
    ab = torch.randn(c.L, c.L, generator=gen(c.L))
    bs, bc = Guarded((c.N, c.ldS)), Guarded((c.N, c.ldC))
    gpu_ctx.op_attn_tables("muse_bias", bs.view, bc.view, in0=dev(ab), L=c.L, rows=c.N, cols=c.K, ld0=c.ldS, ld1=c.ldC)
    rs, rc = muse_bias_ref(c, ab)
    assert same_bits(bs.host(), rs) and same_bits(bc.host(), rc)


def test_allowed(gpu_ctx):
    rows, cols = 33, 35                                                           # 1155 elements: no multiple of the block size
    vals = torch.tensor([0.0, -0.0, 1.0, 1e-30, -2.0, 1e-45])                     # signed zero is hidden; a denormal counts
    mask = vals[torch.randint(0, len(vals), (rows, cols), generator=gen(1))]
    out = Guarded((rows * cols,), torch.uint8)
    gpu_ctx.op_attn_tables("allowed", out.view, in0=dev(mask), rows=rows, cols=cols)
    assert torch.equal(out.host(), (mask != 0).to(torch.uint8).flatten())


def run_layout(gpu_ctx, lay, blk, L):
    H, nb, _ = lay.shape
    ld = (L + 15) // 16 + 3                                                       # two slots more than the model allocates
    lay8, chunks = Guarded((H, nb, nb), torch.uint8), Guarded((H, nb, ld), torch.int16)
    gpu_ctx.op_attn_tables("layout", lay8.view, chunks.view, in0=dev(lay), heads=H, L=L, blk=blk, ld1=ld)
    ref8, _, present = chunk_lists_ref(lay, blk, L)
    assert torch.equal(lay8.host(), ref8)
    got, want = chunks.host().long(), pack_lists(present, ld, SENTINEL[torch.int16])
    assert torch.equal(got, want), f"chunk lists differ in {(got != want).any(-1).sum().item()} of {want[..., 0].numel()} rows"   # counts, ascending ids, untouched slots behind


@pytest.mark.parametrize("name", list(LAYOUT))
def test_layout_chunk_lists(gpu_ctx, name):
    c = LAYOUT[name]
    run_layout(gpu_ctx, layout_inputs(name), c.blk, c.L)


def test_layout_chunk_straddling_two_blocks(gpu_ctx):
    """layout row [0, 1], 24-key blocks, L = 48: chunk 1 (keys 16-31) holds the visible keys 24-31 and must be listed"""
    run_layout(gpu_ctx, torch.tensor([[[0, 1], [0, 1]]]), 24, 48)


@pytest.mark.parametrize("name", list(MASKED))
def test_masked_bias(gpu_ctx, name):
    c, p = MASKED[name], masked_inputs(name)
    nb = c.L // c.blk
    out = Guarded((c.heads, c.rows, c.ldout))
    gpu_ctx.op_attn_tables("masked_bias", out.view, in0=dev(p["add"]) if c.add else None, in1=dev(p["mask"]) if c.mask else None, in2=dev(p["lay"]) if c.lay else None,
                           heads=c.heads, L=c.L, rows=c.rows, cols=c.cols, blk=c.blk, ld0=c.L, ld1=c.ldout, hs0=c.L * c.L if c.per_head_mask else 0,
                           hs1=0 if c.shared_lay else nb * nb, scale=MASK_SCALE)
    assert same_bits(out.host(), masked_bias_ref(c, p))


@pytest.mark.parametrize("name", list(TILES))
def test_attn_tiles(gpu_ctx, name):
    c, bias = TILES[name], tiles_inputs(name)
    nqb, nt = (c.Nq + 127) // 128, c.Nk_pad // 32
    out = Guarded((c.H, nqb, nt + 1), torch.int16)
    gpu_ctx.op_attn_tables("attn_tiles", out.view, in0=dev(bias), heads=c.H, rows=c.Nq, cols=c.Nk_pad, ld0=bias.shape[-1], hs0=c.Nq * bias.shape[-1])
    assert torch.equal(out.host().long(), pack_lists(tile_lists_ref(bias, c.Nk_pad), nt + 1, SENTINEL[torch.int16]))


# ================================================================================================ attention through tile lists
@pytest.mark.parametrize("name", list(ATTN))
def test_attention_tiles(gpu_ctx, name):
    c, p = ATTN[name], attn_inputs(name)
    ref = attn_ref(c, p, torch.float64)
    d = {k: dev(p[k]) for k in ("q", "k", "v", "bias", "res")}

    def run(use_tiles):
        out = Guarded(ref.shape)
        gpu_ctx.op_attention_tiles(d["q"], d["k"], d["v"], d["bias"], out.view, scale=ATTN_SCALE, residual=d["res"], kv_group=c.kv_group, use_tiles=use_tiles,
                                   out_layout=c.out_layout)
        return out.host()

    listed, dense, again = run(True), run(False), run(True)
    e_l, e_d, e_ld = rel(listed, ref), rel(dense, ref), rel(listed, dense)
    print(f"attention_tiles {name}: with the list {e_l:.2e}, without {e_d:.2e} (bound {ATTN_BOUND:.0e}); one against the other {e_ld:.2e} (bound {ATTN_LIST_VS_DENSE:.0e})")
    assert e_l < ATTN_BOUND and e_d < ATTN_BOUND and e_ld < ATTN_LIST_VS_DENSE
    assert same_bits(listed, again)
    assert gpu_ctx.status() == 0
