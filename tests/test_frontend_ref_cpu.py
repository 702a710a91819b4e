"""Case tables, inputs, references and bounds of the operator-level tests of the kernels around the layer stacks (tests/test_frontend_ops_gpu.py): the embedding
kernels and Route M's fp32 q / k / v preparation (bevgen_amd/csrc/embed.hip), the KV-cache writers, the setup tables and row helpers (tables.hip) and the key-tile lists
of the flash-attention kernel (attention.hip).  Runs without a GPU: here the references are checked against themselves.

References come from oracle/restate.py where it states the operation (camera_embeddings, bev_embedding, attention_bias, sparse_self_attention_dense, gpt_embed, and
the q / k / v preparation inside muse_attention, restated below line by line because it is not a function of its own); the rest is plain torch.

  * every floating-point reference is evaluated in fp64 and agrees with its own fp32 evaluation;
  * every integer reference agrees with a second, naive formulation (chunk lists: a per-key loop; tile lists: any bias value of the 128-row block in the 32-key tile
    above 0.5 * -1e30; triangular scatter: torch.tril_indices);
  * in every attention case each query row sees a key in a listed tile (a row that sees nothing has no reference, and an empty list divides by zero in the kernel).

Error metric of the bounded kernels: per row, max |out - ref64| over the row's max |ref64|, maximised over the rows - one wrong low-magnitude row fails.  Their GPU
bound is 4 x e_cpu, e_cpu = the same error of the reference's fp32 evaluation over the kernel's case table: same number of roundings, another summation tree and
fused multiply-adds; a dropped term is orders of magnitude above it.  e_cpu itself must stay below 1e-5 so that an ill-conditioned case cannot buy the kernel slack.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

from oracle import restate as R

NEG = float(torch.tensor(-1.0e30, dtype=torch.float32))      # kNegBig as an fp32 value
HALF_NEG = float(torch.tensor(-1.0e30, dtype=torch.float32) * 0.5)
ECPU_CAP = 1e-5                                               # the loosest operator bound tests/test_ops_gpu.py uses
GPU_FACTOR = 4.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def row_err(out, ref):
    """max over rows (last dimension) of max |out - ref| / max |ref|; a row whose reference is all zero must be reproduced exactly"""
    out, ref = out.double(), ref.double()
    num = (out - ref).abs().reshape(-1, ref.shape[-1]).amax(-1)
    den = ref.abs().reshape(-1, ref.shape[-1]).amax(-1)
    err = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)))
    return err.max().item()


def rel(a, b):
    """the whole-tensor metric of tests/test_ops_gpu.py (attention only)"""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def cast(p, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in p.items()}


# ================================================================================================ camera embedding
Cam = namedtuple("Cam", "name B C h w D kind zero_cols")
CAMERA = {c.name: c for c in [
    Cam("rand-b1-c1-t1-d100", 1, 1, 1, 1, 100, "random", ()),            # D no multiple of 4 nor of 256, a single token
    Cam("rand-b3-c3-t35-d256", 3, 3, 5, 7, 256, "random", (0, 77, 255)),  # one pass of the 256 threads; three output columns with zero weights
    Cam("rig-b1-c6-t35-d1024", 1, 6, 5, 7, 1024, "rig", ()),              # four passes; a realistic six-camera rig
    Cam("rig-b3-c3-t1-d100", 3, 3, 1, 1, 100, "rig", (99,)),
    Cam("zero-b1-c1-t35-d100", 1, 1, 5, 7, 100, "random", "all"),         # every weight zero: 0 / (0 + 1e-7) = 0, the + 1e-7 sits outside the square root
]}


@functools.lru_cache(maxsize=None)
def camera_inputs(name):
    c = CAMERA[name]
    g = gen(100 + len(name) + c.D)
    B, C, D = c.B, c.C, c.D
    if c.kind == "random":
        cfg = SimpleNamespace(cam_latent_h=c.h, cam_latent_w=c.w, cam_res=(1.0, 1.0))
        I_inv = torch.randn(B, C, 3, 3, generator=g)
        E_inv = torch.randn(B, C, 4, 4, generator=g)
    else:
        # pinhole cameras of ~1260 px focal length on 1600 x 900 images, yawed around the vehicle, mounted a few metres from its origin; the pixel plane is scaled by
        # cam_res as bevgen_amd.tables.image_plane scales it
        cfg = SimpleNamespace(cam_latent_h=c.h, cam_latent_w=c.w, cam_res=(1600.0, 900.0))
        Kmat = torch.zeros(B, C, 3, 3, dtype=torch.float64)
        Kmat[..., 0, 0] = 1260.0 + 8.0 * torch.randn(B, C, generator=g, dtype=torch.float64)
        Kmat[..., 1, 1] = 1260.0 + 8.0 * torch.randn(B, C, generator=g, dtype=torch.float64)
        Kmat[..., 0, 2] = 800.0 + 20.0 * torch.randn(B, C, generator=g, dtype=torch.float64)
        Kmat[..., 1, 2] = 450.0 + 20.0 * torch.randn(B, C, generator=g, dtype=torch.float64)
        Kmat[..., 2, 2] = 1.0
        I_inv = torch.linalg.inv(Kmat).float()
        E = torch.zeros(B, C, 4, 4, dtype=torch.float64)
        for b in range(B):
            for cam in range(C):
                yaw = 2 * math.pi * cam / C + 0.05 * b
                pitch = 0.03 * (cam + 1)
                Rz = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]], dtype=torch.float64)
                Rx = torch.tensor([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]], dtype=torch.float64)
                # camera axes (x right, y down, z forward) to vehicle axes (x forward, y left, z up), then the mounting rotation
                axes = torch.tensor([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], dtype=torch.float64)
                E[b, cam, :3, :3] = Rz @ Rx @ axes
                E[b, cam, :3, 3] = torch.tensor([1.5 * math.cos(yaw), 1.5 * math.sin(yaw), 1.6], dtype=torch.float64) + 0.2 * torch.randn(3, generator=g, dtype=torch.float64)
                E[b, cam, 3, 3] = 1.0
        E_inv = E.float()
    plane = R.image_plane(cfg)
    Wimg = torch.randn(D, 4, generator=g) * 0.3
    Wcam = torch.randn(D, 4, generator=g) * 0.3
    if c.zero_cols == "all":
        Wimg.zero_(), Wcam.zero_()
    for o in (() if c.zero_cols == "all" else c.zero_cols):
        Wimg[o] = 0
        Wcam[o] = 0
    return dict(I_inv=I_inv, E_inv=E_inv, plane=plane, Wimg=Wimg, Wcam=Wcam, cfg=cfg)


def camera_ref(p, dtype):
    """restate.camera_embeddings on the case's plane -> (img [B, C, T, D], c_embed [B, C, D])"""
    q = cast(p, dtype)
    sd = {"img_embed.weight": q["Wimg"], "cam_embed.weight": q["Wcam"]}
    with mock.patch.object(R, "image_plane", lambda cfg: q["plane"]):   # the plane is an operand (a table of the context): the same fp32 values in both evaluations
        return R.camera_embeddings(sd, "", p["cfg"], q["I_inv"], q["E_inv"])


# ================================================================================================ condition embedding
Cond = namedtuple("Cond", "name B C K D")
COND = {c.name: c for c in [Cond("b2-c1-k9-d100", 2, 1, 9, 100), Cond("b3-c3-k16-d1024", 3, 3, 16, 1024)]}
COND_VOCAB = 7


@functools.lru_cache(maxsize=None)
def cond_inputs(name):
    c = COND[name]
    g = gen(200 + c.K)
    ids = torch.randint(0, COND_VOCAB, (c.B, c.K), generator=g)
    ids[0, :4] = torch.tensor([-3, 0, COND_VOCAB - 1, COND_VOCAB + 5])   # below the table, first row, last row, beyond the table
    ids[-1, -1] = COND_VOCAB + 5
    return dict(ids=ids, tok=torch.randn(COND_VOCAB, c.D, generator=g), pos=torch.randn(c.K, c.D, generator=g), grid=torch.randn(3, c.K, generator=g) * 3,
                Wbev=torch.randn(c.D, 2, generator=g) * 0.5, bbev=torch.randn(c.D, generator=g) * 0.5, cam_pos=torch.randn(c.C, c.K, c.D, generator=g),
                c_embed=torch.randn(c.B, c.C, c.D, generator=g))


def cond_ref(p, dtype, grid):
    """restate.muse_context's condition rows: (cond_tok[id] + bev_embedding) + cond_pos, ids clamped to the table (the kernel's contract)"""
    q = cast(p, dtype)
    ctx = q["tok"][p["ids"].clamp(0, COND_VOCAB - 1)]
    if grid:
        sd = {"bev_grid": q["grid"], "bev_embed.weight": q["Wbev"], "bev_embed.bias": q["bbev"], "bev_cam_pos_emb": q["cam_pos"]}
        ctx = ctx + R.bev_embedding(sd, "", None, q["c_embed"])
    return ctx + q["pos"][None]


# ================================================================================================ token rows
Tok = namedtuple("Tok", "name B C T D K n_steps steps")
VOCAB = 11                       # table rows = VOCAB + 1: the mask / pad id VOCAB has a row of its own
TOKEN = {c.name: c for c in [
    Tok("b1-n1-d64", 1, 1, 1, 64, 2, 1, (0,)),
    Tok("b3-n35-d1024", 3, 5, 7, 1024, 3, 20, (0, 1, 17, 19)),
    Tok("b3-n35-d64", 3, 5, 7, 64, 1, 35, (34,)),
]}


@functools.lru_cache(maxsize=None)
def token_inputs(name):
    c = TOKEN[name]
    N = c.C * c.T
    g = gen(300 + c.D + N)
    ids = torch.randint(0, VOCAB, (c.B, N), generator=g)
    special = torch.tensor([-1, 0, VOCAB, VOCAB + 7])
    ids.view(-1)[: min(4, ids.numel())] = special[: min(4, ids.numel())]
    if ids.numel() < 4:
        ids.view(-1)[0] = VOCAB
    else:
        ids.view(-1)[-4:] = special                     # the same ids on the last rows as well
    fwd = torch.randperm(N, generator=g)
    if N > 1:
        assert not torch.equal(fwd, torch.arange(N))
    return dict(ids=ids, tok=torch.randn(VOCAB + 1, c.D, generator=g), img=torch.randn(c.B, N, c.D, generator=g), pos=torch.randn(N, c.D, generator=g), fwd=fwd)


def clamp_rows(ids):
    return ids.clamp(0, VOCAB)   # rows [0, VOCAB] of a table of VOCAB + 1 rows


def token_ref(p, dtype, img):
    """camera-major rows x[b, n] = (tok[id] + img[b, n]) + pos[n] (restate.gpt_embed / muse_forward: the geometric term first, then the position)"""
    q = cast(p, dtype)
    x = q["tok"][clamp_rows(p["ids"])]
    if img:
        x = x + q["img"]
    return x + q["pos"][None]


def seq_ref(p, dtype, img, n_steps):
    """decode-order rows: row s = camera-major row forward_shuffle_idx[s]"""
    return token_ref(p, dtype, img)[:, p["fwd"][:n_steps]]


# ================================================================================================ Route M fp32 q / k / v preparation
Prep = namedtuple("Prep", "name B H Nq Nk")
PREP = {c.name: c for c in [Prep("b1-h1-q1-k1", 1, 1, 1, 1), Prep("b2-h3-q5-k31", 2, 3, 5, 31), Prep("b3-h3-q37-k32", 3, 3, 37, 32)]}


def nk_pad(Nk):
    return (Nk + 1 + 31) // 32 * 32      # context.cpp: round_up(N + 1, 32)


@functools.lru_cache(maxsize=None)
def prep_inputs(name):
    c = PREP[name]
    g = gen(400 + c.Nq + c.Nk)
    qraw = torch.randn(c.B * c.Nq, c.H * 64, generator=g)
    kvraw = torch.randn(c.B * c.Nk, 2 * c.H * 64, generator=g)
    if c.B * c.Nq > 1:
        qraw[-1, (c.H - 1) * 64:] = 0                # one zero query row of the last head: the max(norm, 1e-12) branch
    if c.B * c.Nk > 1:
        kvraw[-1, :64] = 0                           # one zero key row of head 0 (its value row stays)
    return dict(qraw=qraw, kvraw=kvraw, null_kv=torch.randn(2, c.H, 64, generator=g), q_scale=torch.rand(64, generator=g) + 0.5, k_scale=torch.rand(64, generator=g) * 2 + 1)


def prep_ref(c, p, dtype):
    """restate.muse_attention's lines between the projections and the similarity: q = normalize(8 q) o q_scale; k, v = (null | projected), k = normalize(k) o k_scale"""
    q_ = cast(p, dtype)
    split = lambda t: t.reshape(c.B, -1, c.H, 64).permute(0, 2, 1, 3)
    q = split(q_["qraw"]) * 8.0
    k, v = (split(t) for t in q_["kvraw"].chunk(2, dim=-1))
    nk, nv = q_["null_kv"][0][:, None], q_["null_kv"][1][:, None]          # [H, 1, 64] each
    k = torch.cat([nk[None].expand(c.B, -1, -1, -1), k], dim=2)
    v = torch.cat([nv[None].expand(c.B, -1, -1, -1), v], dim=2)
    return F.normalize(q, dim=-1) * q_["q_scale"], F.normalize(k, dim=-1) * q_["k_scale"], v


# ================================================================================================ KV-cache writers
Kv = namedtuple("Kv", "name B H n Lmax pos0 dpos")   # scatter: rows [pos0, pos0 + n); append: row dpos + pos0 = Lmax - 1
KV = {c.name: c for c in [Kv("b1-h1-n1-l8", 1, 1, 1, 8, 3, 4), Kv("b3-h3-n5-l40", 3, 3, 5, 40, 35, 4), Kv("b3-h1-n5-l8", 3, 1, 5, 8, 2, 5)]}
F16_FINITE = (65504.0, -65504.0, 65519.0)            # 65519 rounds to 65504
F16_BAD = (65520.0, float("inf"), float("nan"))      # 65520 is the first value that rounds to inf


def kv_inputs(c, n):
    g = gen(500 + c.B * 10 + c.H + n)
    return torch.randn(c.B * n, 3 * c.H * 64, generator=g) * 4


def kv_scatter_ref(c, qkv, n, pos, kc, vc):
    """-> (q [B, H, n, 64], kc, vc) with rows [pos, pos + n) of every (b, h) replaced (values converted to the cache's dtype, round to nearest even)"""
    t = qkv.reshape(c.B, n, 3, c.H, 64).permute(2, 0, 3, 1, 4)   # [3, B, H, n, 64]
    kc, vc = kc.clone(), vc.clone()
    kc[:, :, pos:pos + n] = t[1].to(kc.dtype)
    vc[:, :, pos:pos + n] = t[2].to(vc.dtype)
    return t[0].contiguous(), kc, vc


Rep = namedtuple("Rep", "name layers B H L rows src dst0 count")
REPLICATE = {c.name: c for c in [Rep("src-inside", 2, 4, 2, 8, 5, 1, 0, 3), Rep("src-outside", 2, 4, 3, 8, 3, 3, 1, 2), Rep("single", 2, 3, 1, 8, 7, 0, 2, 1)]}


def replicate_ref(c, cache):
    out = cache.clone()                                  # [layers, B, H, L, 64]
    for d in range(c.dst0, c.dst0 + c.count):
        if d != c.src:
            out[:, d, :, :c.rows] = cache[:, c.src, :, :c.rows]
    return out


# ================================================================================================ tables
def attn_bias_ref(emb, prob, L):
    """entry (r, c <= r) = element r (r + 1) / 2 + c of the parameter, + prob: one fp32 add, in the kernel's order"""
    out = torch.zeros(L, L)
    if emb is not None:
        for r in range(L):
            out[r, :r + 1] = emb[r * (r + 1) // 2: r * (r + 1) // 2 + r + 1]
    return out + prob if prob is not None else out


ATTN_BIAS_L = (1, 5, 33)


def attn_bias_inputs(L):
    g = gen(600 + L)
    return torch.randn(L * (L + 1) // 2, generator=g), torch.randn(L, L, generator=g)


MuseBias = namedtuple("MuseBias", "name K N L ldS ldC")
MUSE_BIAS = {c.name: c for c in [MuseBias("k4-n5", 4, 5, 11, 32, 32), MuseBias("k16-n35", 16, 35, 51, 64, 32), MuseBias("k16-n5-wide", 16, 5, 24, 36, 40)]}


def muse_bias_ref(c, ab):
    """muse_attention: self bias = pad_left0(bias[K:, K:]), cross bias = pad_left0(bias[K:, :K]); columns behind the real keys -1e30"""
    bs = torch.full((c.N, c.ldS), NEG)
    bc = torch.full((c.N, c.ldC), NEG)
    bs[:, :c.N + 1] = F.pad(ab[c.K:c.K + c.N, c.K:c.K + c.N], (1, 0), value=0.0)
    bc[:, :c.K + 1] = F.pad(ab[c.K:c.K + c.N, :c.K], (1, 0), value=0.0)
    return bs, bc


Lay = namedtuple("Lay", "name blk L")
LAYOUT = {c.name: c for c in [Lay(f"blk{b}-l{L}", b, L) for b, L in
                              [(1, 48), (1, 64), (1, 96), (4, 48), (4, 64), (4, 96), (16, 48), (16, 64), (16, 96), (32, 64), (32, 96), (4, 40),
                               (20, 40), (20, 60), (24, 48), (24, 96), (40, 80), (40, 120)]]}   # the last six: blocks that straddle 16-key chunks
LAYOUT_HEADS = 4                                          # densities ~0.1, 0.5, 1 and the two-block rows [0, 1], [1, 0] pattern


@functools.lru_cache(maxsize=None)
def layout_inputs(name):
    c = LAYOUT[name]
    nb = c.L // c.blk
    g = gen(700 + c.blk * 7 + c.L)
    lay = torch.stack([(torch.rand(nb, nb, generator=g) < d).long() for d in (0.1, 0.5, 1.0)] + [torch.zeros(nb, nb, dtype=torch.long)])
    lay[1, nb // 2] = 0                                   # an all-zero row (count 0)
    lay[3, :, -1] = 1                                     # only the LAST block present: with 24-key blocks and L = 48 this is the row [0, 1] whose chunk 1 was dropped
    lay[3, 0] = 0
    lay[3, 0, 0] = 3                                      # any non-zero value counts as present
    return lay


def chunk_lists_ref(lay, blk, L):
    """-> (uint8 layout, counts [H, nb], present [H, nb, nc]): chunk c is present when a present block overlaps keys [16 c, 16 c + 16)"""
    nc = (L + 15) // 16
    keys = (lay != 0).repeat_interleave(blk, dim=-1)                       # [H, nb, L] per-key presence
    keys = F.pad(keys, (0, nc * 16 - L))
    present = keys.reshape(*lay.shape[:2], nc, 16).any(-1)
    return (lay != 0).to(torch.uint8), present.sum(-1), present


def chunk_lists_naive(lay, blk, L):
    H, nb, _ = lay.shape
    nc = (L + 15) // 16
    present = torch.zeros(H, nb, nc, dtype=torch.bool)
    for h in range(H):
        for r in range(nb):
            for k in range(L):
                if lay[h, r, k // blk] != 0:
                    present[h, r, k // 16] = True
    return present


def chunk_lists_first_key_probe(lay, blk, L):
    """the probe the kernel had before it was fixed: keys 16 c, 16 c + min(blk, 16), ... - wrong for block sizes above 16 that are no multiple of 16"""
    H, nb, _ = lay.shape
    nc = (L + 15) // 16
    present = torch.zeros(H, nb, nc, dtype=torch.bool)
    for h in range(H):
        for r in range(nb):
            for c in range(nc):
                present[h, r, c] = any(lay[h, r, k // blk] != 0 for k in range(16 * c, min(L, 16 * c + 16), min(blk, 16)))
    return present


def pack_lists(present, ld, fill):
    """[..., n] presence -> [..., ld] (count, ascending ids, then `fill`) as int64"""
    flat = present.reshape(-1, present.shape[-1])
    out = torch.full((flat.shape[0], ld), fill, dtype=torch.int64)
    for i, row in enumerate(flat):
        ids = row.nonzero().flatten()
        out[i, 0] = ids.numel()
        out[i, 1:1 + ids.numel()] = ids
    return out.reshape(*present.shape[:-1], ld)


Masked = namedtuple("Masked", "name heads L blk rows cols ldout mask lay add per_head_mask shared_lay")
MASKED = {c.name: c for c in [
    Masked("both", 3, 40, 4, 20, 20, 32, True, True, True, False, False),
    Masked("mask-only", 3, 40, 4, 20, 20, 32, True, False, True, False, False),
    Masked("layout-only", 3, 40, 4, 20, 20, 32, False, True, True, False, False),
    Masked("neither", 2, 40, 4, 20, 20, 32, False, False, True, False, False),
    Masked("no-add", 3, 40, 4, 20, 20, 32, True, True, False, False, False),
    Masked("per-head-mask-shared-layout", 3, 48, 16, 33, 31, 36, True, True, True, True, True),   # ragged rows / cols, the layout plane shared by the heads
    Masked("full-l", 2, 40, 4, 40, 40, 64, True, True, True, False, False),
]}


@functools.lru_cache(maxsize=None)
def masked_inputs(name):
    c = MASKED[name]
    g = gen(800 + len(name))
    nb = c.L // c.blk
    mask = (torch.rand(c.heads if c.per_head_mask else 1, c.L, c.L, generator=g) > 0.4).to(torch.uint8)
    lay = (torch.rand(1 if c.shared_lay else c.heads, nb, nb, generator=g) < 0.5).to(torch.uint8)
    return dict(add=torch.randn(c.L, c.L, generator=g), mask=mask, lay=lay)


MASK_SCALE = 0.125


def masked_bias_ref(c, p):
    """[heads, rows, ldout]: visible ? scale * add : -1e30 (one fp32 product), padding columns -1e30"""
    vis = torch.ones(c.heads, c.rows, c.cols, dtype=torch.bool)
    if c.mask:
        vis &= p["mask"][:, :c.rows, :c.cols].bool()
    if c.lay:
        vis &= torch.kron(p["lay"].float(), torch.ones(c.blk, c.blk))[:, :c.rows, :c.cols] > 0
    val = (p["add"][:c.rows, :c.cols] * MASK_SCALE) if c.add else torch.zeros(c.rows, c.cols)
    out = torch.full((c.heads, c.rows, c.ldout), NEG)
    out[:, :, :c.cols] = torch.where(vis, val[None].expand(c.heads, -1, -1), torch.tensor(NEG))
    return out


Tiles = namedtuple("Tiles", "name H Nq Nk_pad")
TILES = {c.name: c for c in [Tiles("h1-q48-k32", 1, 48, 32), Tiles("h3-q200-k320", 3, 200, 320), Tiles("h3-q300-k320", 3, 300, 320), Tiles("h1-q300-k32", 1, 300, 32)]}
TILES_LD_PAD = 4                                          # columns behind Nk_pad hold visible-looking zeros: they must not be read


@functools.lru_cache(maxsize=None)
def tiles_inputs(name):
    c = TILES[name]
    g = gen(900 + c.Nq + c.Nk_pad)
    nt, nqb = c.Nk_pad // 32, (c.Nq + 127) // 128
    bias = torch.full((c.H, c.Nq, c.Nk_pad + TILES_LD_PAD), NEG)
    bias[:, :, c.Nk_pad:] = 0.0
    for h in range(c.H):
        for qb in range(nqb):
            r0, r1 = qb * 128, min(c.Nq, qb * 128 + 128)
            for t in range(nt):
                if torch.rand((), generator=g) < 0.4:    # a tile some rows of the block see
                    blk = torch.where(torch.rand(r1 - r0, 32, generator=g) < 0.3, torch.randn(r1 - r0, 32, generator=g), torch.tensor(NEG))
                    blk[0, 0] = 1.0
                    bias[h, r0:r1, t * 32:t * 32 + 32] = blk
    if nt > 3:
        bias[0, :, 32:64] = NEG                            # tile 1 of head 0: masked for every row
        bias[0, :, 64:96] = NEG
        bias[0, c.Nq - 1, 64 + 31] = -2.5                   # tile 2: visible to exactly one row, the LAST of the last block, in the tile's last column
        bias[0, :, 96:128] = NEG
        bias[0, 0, 96] = HALF_NEG                          # tile 3: a value exactly at the threshold is NOT above it ...
    else:
        bias[0, :, :32] = NEG
        bias[0, c.Nq - 1, 31] = -2.5
    if c.H > 1:
        bias[1, :, 0:32] = NEG
        bias[1, 0, 5] = float(torch.nextafter(torch.tensor(HALF_NEG), torch.tensor(0.0)))   # ... one ulp above it is
    return bias


def tile_lists_ref(bias, Nk_pad):
    """[H, nqb, nt] presence: any value of the 128-row block in the 32-key tile above 0.5 * -1e30"""
    H, Nq, _ = bias.shape
    nqb = (Nq + 127) // 128
    vis = F.pad(bias[:, :, :Nk_pad] > HALF_NEG, (0, 0, 0, nqb * 128 - Nq))
    return vis.reshape(H, nqb, 128, Nk_pad // 32, 32).permute(0, 1, 3, 2, 4).reshape(H, nqb, Nk_pad // 32, -1).any(-1)


def tile_lists_naive(bias, Nk_pad):
    H, Nq, _ = bias.shape
    nqb, nt = (Nq + 127) // 128, Nk_pad // 32
    out = torch.zeros(H, nqb, nt, dtype=torch.bool)
    for h in range(H):
        for qb in range(nqb):
            for t in range(nt):
                out[h, qb, t] = bool((bias[h, qb * 128:min(Nq, qb * 128 + 128), t * 32:t * 32 + 32] > 0.5 * -1e30).any())
    return out


# ================================================================================================ attention through tile lists
Attn = namedtuple("Attn", "name B H Nq Nk_pad Nk blk diag kv_group residual out_layout")
ATTN = {c.name: c for c in [
    Attn("q48-k64-blk4", 2, 3, 48, 64, 64, 4, False, 1, False, 0),
    Attn("q200-k320-blk16-res", 2, 3, 200, 320, 315, 16, False, 1, True, 0),
    Attn("q300-k320-blk4-bhnd", 2, 3, 300, 320, 320, 4, False, 1, False, 1),
    Attn("q300-k64-blk16-group2", 4, 3, 300, 64, 59, 16, False, 2, False, 0),
    Attn("q200-k64-blk4-res-bhnd", 2, 3, 200, 64, 64, 4, False, 1, True, 1),
    # block column 0 absent in places, the diagonal block present: rows whose leading listed tiles are fully masked (the -1e30 running-maximum rescale)
    Attn("q48-k64-blk4-diag", 2, 3, 48, 64, 64, 4, True, 1, False, 0),
    Attn("q300-k320-blk16-diag-res", 2, 3, 300, 320, 320, 16, True, 1, True, 0),
]}
ATTN_SCALE = 0.125                                        # head dim 64: the scale sparse_self_attention_dense applies
ATTN_BOUND = 5e-6                                         # test_attention's bound on the same kernel
ATTN_LIST_VS_DENSE = 2e-6                                 # with against without the list: the bound of the key-split test for the same claim


@functools.lru_cache(maxsize=None)
def attn_inputs(name):
    c = ATTN[name]
    g = gen(1000 + c.Nq + c.Nk_pad + c.blk)
    Ls = (max(c.Nq, c.Nk_pad) + c.blk - 1) // c.blk * c.blk          # the square problem the reference operator is stated on
    nb = Ls // c.blk
    lay = (torch.rand(c.H, nb, nb, generator=g) < 0.4).long()
    if c.diag:
        lay[:, :, 0] = (torch.rand(c.H, nb, generator=g) < 0.3).long()
        lay[:, 0, 0] = 1
        lay[:, torch.arange(nb), torch.arange(nb)] = 1
        lay[:, (c.Nq - 1) // c.blk] = 0                   # the last query rows see their diagonal block only
        lay[:, (c.Nq - 1) // c.blk, (c.Nq - 1) // c.blk] = 1
    else:
        lay[:, :, 0] = 1                                  # block column 0 always present
    lay[:, :, -(-c.Nk // c.blk):] = 0                     # no block behind the real keys
    mask = torch.tril(torch.ones(Ls, Ls))                 # causal element mask
    mask[:, c.Nk:] = 0                                    # keys behind the real ones
    add = torch.randn(Ls, Ls, generator=g)
    Bk = c.B // c.kv_group
    q = torch.randn(c.B, c.H, c.Nq, 64, generator=g)
    k = torch.zeros(Bk, c.H, c.Nk_pad, 64)
    v = torch.zeros(Bk, c.H, c.Nk_pad, 64)
    k[:, :, :c.Nk] = torch.randn(Bk, c.H, c.Nk, 64, generator=g)
    v[:, :, :c.Nk] = torch.randn(Bk, c.H, c.Nk, 64, generator=g)
    res = torch.randn(c.B, c.Nq, c.H * 64, generator=g) if c.residual else None
    if res is not None and c.out_layout == 1:
        res = res.reshape(c.B, c.Nq, c.H, 64).permute(0, 2, 1, 3).contiguous()
    vis = (torch.kron(lay.float(), torch.ones(c.blk, c.blk)) > 0) & (mask != 0)[None]             # [H, Ls, Ls]
    vis = vis[:, :c.Nq, :c.Nk_pad]
    bias = torch.where(vis, (add[:c.Nq, :c.Nk_pad] * ATTN_SCALE)[None].expand(c.H, -1, -1), torch.tensor(NEG))   # what launch_build_masked_bias hands the kernel
    return dict(q=q, k=k, v=v, res=res, lay=lay, mask=mask, add=add, bias=bias, Ls=Ls, vis=vis)


def attn_ref(c, p, dtype):
    """restate.sparse_self_attention_dense on the square problem (queries and keys zero-padded to Ls, the padding keys hidden), cut back to the Nq rows; output in
    the case's layout with the residual added"""
    Ls = p["Ls"]
    q = F.pad(p["q"].to(dtype), (0, 0, 0, Ls - c.Nq))
    k, v = (F.pad(t.to(dtype), (0, 0, 0, Ls - c.Nk_pad)).repeat_interleave(c.kv_group, dim=0) for t in (p["k"], p["v"]))
    mask = p["mask"].clone()
    mask[c.Nq:, 0] = 1                                    # the padding query rows see key 0 (they are cut off; without a key their softmax is NaN)
    lay = p["lay"].clone()
    lay[:, :, 0] = torch.where(torch.arange(lay.shape[1])[None] * c.blk >= c.Nq, torch.ones_like(lay[:, :, 0]), lay[:, :, 0])
    o = R.sparse_self_attention_dense(q, k, v, lay, c.blk, mask, p["add"].to(dtype))[:, :, :c.Nq]   # [B, H, Nq, 64]
    if c.out_layout == 0:
        o = o.permute(0, 2, 1, 3).reshape(c.B, c.Nq, c.H * 64)
    return o + p["res"].to(dtype) if c.residual else o


# ================================================================================================ e_cpu: the fp32 evaluation's own error, per bounded kernel
@functools.lru_cache(maxsize=None)
def e_cpu():
    e = {"camera_img": 0.0, "camera_c_embed": 0.0, "cond_embed": 0.0, "prep_q": 0.0, "prep_k": 0.0}
    for name in CAMERA:
        p = camera_inputs(name)
        (i32, c32), (i64, c64) = camera_ref(p, torch.float32), camera_ref(p, torch.float64)
        e["camera_img"] = max(e["camera_img"], row_err(i32, i64))
        e["camera_c_embed"] = max(e["camera_c_embed"], row_err(c32, c64))
    for name in COND:
        p = cond_inputs(name)
        e["cond_embed"] = max(e["cond_embed"], row_err(cond_ref(p, torch.float32, True), cond_ref(p, torch.float64, True)))
    for name, c in PREP.items():
        p = prep_inputs(name)
        (q32, k32, _), (q64, k64, _) = prep_ref(c, p, torch.float32), prep_ref(c, p, torch.float64)
        e["prep_q"] = max(e["prep_q"], row_err(q32, q64))
        e["prep_k"] = max(e["prep_k"], row_err(k32, k64))
    return e


def gpu_bound(kernel):
    return GPU_FACTOR * e_cpu()[kernel]


# ================================================================================================ the self-checks
def test_e_cpu_is_small_and_not_zero():
    for k, v in e_cpu().items():
        print(f"e_cpu {k}: {v:.3e} -> GPU bound {GPU_FACTOR * v:.3e}")
        assert 0 < v < ECPU_CAP, (k, v)


@pytest.mark.parametrize("name", list(CAMERA))
def test_camera_reference(name):
    c, p = CAMERA[name], camera_inputs(name)
    img, ce = camera_ref(p, torch.float64)
    assert img.shape == (c.B, c.C, c.h * c.w, c.D) and ce.shape == (c.B, c.C, c.D) and img.dtype == torch.float64
    if c.zero_cols == "all":
        assert img.abs().max() == 0 and ce.abs().max() == 0
    else:
        assert (img.norm(dim=-1) - 1).abs().max() < 1e-6                           # unit rows (1e-7 against a norm of order 1)
        for o in c.zero_cols:
            assert img[..., o].abs().max() == 0 and ce[..., o].abs().max() == 0
    # c_embed is the t-independent term alone: E_inv[..., :, 3] through cam_embed
    assert torch.allclose(ce, p["E_inv"].double()[..., 3] @ p["Wcam"].double().t(), rtol=0, atol=1e-12)


def test_rig_plane_is_the_products_plane():
    from bevgen_amd import tables

    for name in ("rig-b1-c6-t35-d1024", "rig-b3-c3-t1-d100"):
        p = camera_inputs(name)
        assert torch.equal(tables.image_plane(p["cfg"]).reshape(3, -1), p["plane"])
        assert p["plane"][0].max() == (1600.0 if p["plane"].shape[1] > 1 else 0.0)
        f = 1.0 / p["I_inv"][..., 0, 0]
        assert 1200 < f.min() and f.max() < 1320


@pytest.mark.parametrize("name", list(COND))
def test_cond_reference(name):
    c, p = COND[name], cond_inputs(name)
    for grid in (False, True):
        r64, r32 = cond_ref(p, torch.float64, grid), cond_ref(p, torch.float32, grid)
        assert r64.shape == (c.B, c.K, c.D)
        assert row_err(r32, r64) < ECPU_CAP
    # the clamp: ids below / beyond the table fetch its first / last row
    plain = cond_ref(p, torch.float32, False) - p["pos"][None]
    assert torch.allclose(plain[0, 0], p["tok"][0], atol=1e-5) and torch.allclose(plain[0, 3], p["tok"][COND_VOCAB - 1], atol=1e-5)
    assert {-3, 0, COND_VOCAB - 1, COND_VOCAB + 5} <= set(p["ids"].flatten().tolist())


@pytest.mark.parametrize("name", list(TOKEN))
def test_token_references(name):
    c, p = TOKEN[name], token_inputs(name)
    N = c.C * c.T
    for img in (False, True):
        assert row_err(token_ref(p, torch.float32, img), token_ref(p, torch.float64, img)) < 2e-7   # two fp32 adds
    assert VOCAB in p["ids"] and (N == 1 or {-1, 0, VOCAB, VOCAB + 7} <= set(p["ids"].flatten().tolist()))
    # the pad id fetches the table's last row, not row VOCAB - 1
    b, n = (p["ids"] == VOCAB).nonzero()[0].tolist()
    assert torch.equal(token_ref(p, torch.float32, False)[b, n], p["tok"][VOCAB] + p["pos"][n])
    # decode-order rows against restate.gpt_embed (in-range ids, no geometric term): [cond | image rows in decode order]
    ids = clamp_rows(p["ids"]).reshape(c.B, c.C, c.T)
    cfg = SimpleNamespace(num_embed=c.D, image_embed=False, bev_embed=False, forward_shuffle_idx=p["fwd"], num_pad_tokens=0, vocab_size=VOCAB)
    sd = {"x_tok_emb.weight": p["tok"], "cond_tok_emb.weight": torch.zeros(2, c.D), "x_pos_emb": p["pos"][None], "cond_pos_emb": torch.zeros(1, c.K, c.D)}
    seq = R.gpt_embed(sd, cfg, ids, torch.zeros(c.B, c.K, dtype=torch.long), None, None)
    assert torch.equal(seq[:, c.K:c.K + c.n_steps], seq_ref(p, torch.float32, False, c.n_steps))


@pytest.mark.parametrize("name", list(PREP))
def test_prep_reference(name):
    c, p = PREP[name], prep_inputs(name)
    q, k, v = prep_ref(c, p, torch.float64)
    assert q.shape == (c.B, c.H, c.Nq, 64) and k.shape == (c.B, c.H, c.Nk + 1, 64) and v.shape == k.shape
    q32, k32, v32 = prep_ref(c, p, torch.float32)
    assert row_err(q32, q) < ECPU_CAP and row_err(k32, k) < ECPU_CAP and torch.equal(v32.double(), v)
    zero_q, zero_k = q.abs().amax(-1) == 0, k.abs().amax(-1) == 0
    assert int(zero_q.sum()) == (c.B * c.Nq > 1) and int(zero_k.sum()) == (c.B * c.Nk > 1) and v.abs().amax(-1).min() > 0   # the zero raw rows
    if c.B * c.Nq > 1:
        assert zero_q[-1, -1, -1] and zero_k[-1, 0, -1]
    # rows are scale vectors of unit rows; the x8 cancels in the normalisation
    assert ((q / p["q_scale"].double()).norm(dim=-1)[~zero_q] - 1).abs().max() < 1e-12
    assert torch.allclose(k[:, :, 0], (F.normalize(p["null_kv"][0].double(), dim=-1) * p["k_scale"].double())[None].expand(c.B, -1, -1))
    assert nk_pad(c.Nk) % 32 == 0 and nk_pad(c.Nk) >= c.Nk + 1 and nk_pad(31) == 32 and nk_pad(32) == 64


def test_kv_references():
    for c in KV.values():
        assert c.pos0 > 0 and c.pos0 + c.n <= c.Lmax and c.dpos + c.pos0 == c.Lmax - 1
        qkv = kv_inputs(c, c.n)
        for dt in (torch.float32, torch.float16):
            kc = torch.full((c.B, c.H, c.Lmax, 64), 7.0, dtype=dt)
            q, k2, v2 = kv_scatter_ref(c, qkv, c.n, c.pos0, kc, kc)
            assert torch.equal(q[1 % c.B, c.H - 1, c.n - 1], qkv[(1 % c.B) * c.n + c.n - 1, (c.H - 1) * 64:c.H * 64])
            assert torch.equal(k2[0, 0, c.pos0].float(), qkv[0, c.H * 64:c.H * 64 + 64].to(dt).float())
            assert torch.equal(v2[0, 0, c.pos0].float(), qkv[0, 2 * c.H * 64:2 * c.H * 64 + 64].to(dt).float())
            changed = (k2 != kc).any(-1)
            assert not changed[:, :, :c.pos0].any() and not changed[:, :, c.pos0 + c.n:].any()
    assert all(math.isfinite(float(torch.tensor(x).half())) for x in F16_FINITE) and not any(math.isfinite(float(torch.tensor(x).half())) for x in F16_BAD)
    for c in REPLICATE.values():
        cache = torch.arange(c.layers * c.B * c.H * c.L * 64, dtype=torch.float32).reshape(c.layers, c.B, c.H, c.L, 64)
        out = replicate_ref(c, cache)
        assert c.rows < c.L and torch.equal(out[:, :, :, c.rows:], cache[:, :, :, c.rows:])
        outside = [d for d in range(c.B) if not c.dst0 <= d < c.dst0 + c.count or d == c.src]
        assert torch.equal(out[:, outside], cache[:, outside])
    assert (REPLICATE["src-inside"].dst0 <= REPLICATE["src-inside"].src < REPLICATE["src-inside"].dst0 + REPLICATE["src-inside"].count)


@pytest.mark.parametrize("L", ATTN_BIAS_L)
def test_attn_bias_reference(L):
    emb, prob = attn_bias_inputs(L)
    ref = attn_bias_ref(emb, prob, L)
    cfg = SimpleNamespace(gpt_block_size=L, prob_matrix=prob)
    assert torch.equal(ref, R.attention_bias({"camera_bias_emb": emb}, "", cfg))                  # torch.tril_indices' order
    idx = torch.tril_indices(L, L)
    assert torch.equal(attn_bias_ref(emb, None, L)[idx[0], idx[1]], emb)
    up = torch.triu(torch.ones(L, L), 1).bool()
    assert torch.equal(ref[up], prob[up])                                                        # the strict upper triangle holds prob alone
    assert ((attn_bias_ref(emb, None, L).double() + prob.double()).float() == ref).all()               # one add: the fp64 sum rounds to it
    assert attn_bias_ref(None, None, L).abs().max() == 0


@pytest.mark.parametrize("name", list(MUSE_BIAS))
def test_muse_bias_reference(name):
    c = MUSE_BIAS[name]
    ab = torch.randn(c.L, c.L, generator=gen(5))
    bs, bc = muse_bias_ref(c, ab)
    assert (bs[:, 0] == 0).all() and (bc[:, 0] == 0).all()
    for q in range(c.N):
        for j in range(1, c.ldS):
            assert bs[q, j] == (ab[c.K + q, c.K + j - 1] if j <= c.N else NEG)
        for j in range(1, c.ldC):
            assert bc[q, j] == (ab[c.K + q, j - 1] if j <= c.K else NEG)


@pytest.mark.parametrize("name", list(LAYOUT))
def test_chunk_list_reference(name):
    c, lay = LAYOUT[name], layout_inputs(name)
    lay8, counts, present = chunk_lists_ref(lay, c.blk, c.L)
    assert torch.equal(present, chunk_lists_naive(lay, c.blk, c.L))
    assert torch.equal(lay8.bool(), lay != 0) and (counts[1, (c.L // c.blk) // 2] == 0)
    packed = pack_lists(present, (c.L + 15) // 16 + 3, -1)
    for row, pr in zip(packed.reshape(-1, packed.shape[-1]), present.reshape(-1, present.shape[-1])):
        n = int(row[0])
        ids = row[1:1 + n]
        assert n == int(pr.sum()) and (ids[1:] > ids[:-1]).all() and (row[1 + n:] == -1).all()
    straddles = c.blk > 16 and c.blk % 16 != 0
    assert torch.equal(chunk_lists_first_key_probe(lay, c.blk, c.L), present) != straddles       # the old probe is wrong exactly at the straddling block sizes


def test_chunk_list_defect_case():
    """layout row [0, 1], 24-key blocks, L = 48: keys 24-31 of chunk 1 are visible"""
    lay = torch.tensor([[[0, 1], [0, 1]]])
    assert chunk_lists_ref(lay, 24, 48)[2][0, 0].tolist() == [False, True, True]
    assert chunk_lists_first_key_probe(lay, 24, 48)[0, 0].tolist() == [False, False, True]


@pytest.mark.parametrize("name", list(MASKED))
def test_masked_bias_reference(name):
    c, p = MASKED[name], masked_inputs(name)
    ref = masked_bias_ref(c, p)
    for h in range(c.heads):
        for r in range(0, c.rows, 3):
            for col in range(c.ldout):
                vis = col < c.cols and (not c.mask or p["mask"][h if c.per_head_mask else 0, r, col] != 0) and \
                      (not c.lay or p["lay"][0 if c.shared_lay else h, r // c.blk, col // c.blk] != 0)
                want = (p["add"][r, col] * MASK_SCALE if c.add else 0.0) if vis else NEG
                assert ref[h, r, col] == want
    assert ((p["add"][:c.rows, :c.cols].double() * MASK_SCALE).float() == p["add"][:c.rows, :c.cols] * MASK_SCALE).all()   # a power-of-two product: exact


@pytest.mark.parametrize("name", list(TILES))
def test_tile_list_reference(name):
    c, bias = TILES[name], tiles_inputs(name)
    present = tile_lists_ref(bias, c.Nk_pad)
    assert torch.equal(present, tile_lists_naive(bias, c.Nk_pad))
    assert present.shape == (c.H, (c.Nq + 127) // 128, c.Nk_pad // 32)
    if c.Nk_pad > 96:
        assert not present[0, :, 1].any() and present[0, -1, 2] and not present[0, 0, 3]          # masked for all; one row; exactly the threshold
        assert (bias[0, :, 64:96] > HALF_NEG).sum() == 1
    else:
        assert present[0, -1, 0] and (bias[0, :, :32] > HALF_NEG).sum() == 1                        # exactly one visible element
    if c.H > 1:
        assert present[1, 0, 0] and (bias[1, :128, :32] > HALF_NEG).sum() == 1                     # one ulp above the threshold


@pytest.mark.parametrize("name", list(ATTN))
def test_attention_reference_and_masks(name):
    c, p = ATTN[name], attn_inputs(name)
    r64, r32 = attn_ref(c, p, torch.float64), attn_ref(c, p, torch.float32)
    assert r64.shape == ((c.B, c.Nq, c.H * 64) if c.out_layout == 0 else (c.B, c.H, c.Nq, 64)) and bool(r64.isfinite().all())
    assert rel(r32, r64) < ECPU_CAP
    # the bias operand says what the visibility says, and every row sees a key in a listed tile
    assert torch.equal(p["bias"] > HALF_NEG, p["vis"])
    present = tile_lists_ref(p["bias"], c.Nk_pad)
    assert torch.equal(present, tile_lists_naive(p["bias"], c.Nk_pad))
    nqb = (c.Nq + 127) // 128
    listed = present[:, torch.arange(c.Nq) // 128].repeat_interleave(32, dim=-1)                  # [H, Nq, Nk_pad]
    assert present.shape[1] == nqb and bool((p["vis"] & listed).any(-1).all())
    assert not p["vis"][:, :, c.Nk:].any()
    # the same reference from the bias operand alone (what the kernel is handed): softmax(scale q k^T + bias) v
    s = torch.einsum("bhid,bhjd->bhij", p["q"].double(), p["k"].double().repeat_interleave(c.kv_group, dim=0)) * ATTN_SCALE + p["bias"].double()[None]
    o = torch.einsum("bhij,bhjd->bhid", s.softmax(-1), p["v"].double().repeat_interleave(c.kv_group, dim=0))
    if c.out_layout == 0:
        o = o.permute(0, 2, 1, 3).reshape(c.B, c.Nq, c.H * 64)
    assert rel(o + p["res"].double() if c.residual else o, r64) < 1e-12
    # the sparsity the case was chosen for: some tiles are skipped, and in the diag cases some row's first listed tile is fully masked for it
    assert c.Nk_pad == 64 or not present.all()           # (two key tiles: every block sees both)
    if c.diag:
        first = present.float().argmax(-1)[:, torch.arange(c.Nq) // 128]                         # [H, Nq] first listed tile of the row's block
        lead = torch.gather(p["vis"].reshape(c.H, c.Nq, -1, 32).any(-1), 2, first[..., None])[..., 0]
        assert bool((~lead).any())
