"""Operator-level checks of the classifier-free-guidance kernels: add_row_layernorm (norm.hip), cfg_combine (sampler.hip) and the finalize-time null-row table
(tables.hip), each through its C-ABI entry."""
import pytest
import torch
import torch.nn.functional as F

from oracle import cases

pytestmark = pytest.mark.gpu

LN_BOUND = 1e-5   # what tests/test_ops_gpu.py::test_layernorm holds the LayerNorm kernel to (tests/test_muse_proj_ref_cpu.py cites it as LN_PLANES_BOUND)
SENTINEL = 12345.0


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def planes_value(p):
    """[rows, ld / 32, 2, 32] raw f16 words -> fp64 [rows, ld]: hi + lo 2^-11 (the split of common.h)."""
    h = p.view(torch.float16).double()
    return (h[:, :, 0] + h[:, :, 1] * 2.0 ** -11).reshape(p.shape[0], -1)


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("D", [128, 192, 1024])
@pytest.mark.parametrize("rows", [1, 300])
def test_add_row_layernorm(gpu_ctx, rows, D, planes):
    """x += r in place, then LayerNorm: within 1e-5 of fp64, bit-equal to the existing LayerNorm op applied to x + r (fp32 rows and plane image), nothing written behind
    the last row.  Rows 1 and 300 (no multiple of the four rows of a workgroup), D 128 / 192 (the plane writer's generic path) / 1024 (its whole-line path); the last row
    has mean / std ~ 50, where a one-pass variance would cancel."""
    g = torch.Generator().manual_seed(rows * 7 + D)
    x = torch.randn(rows, D, generator=g) * 3 + 1
    x[-1] = torch.randn(D, generator=g) * 0.1 + 5.0
    r = torch.randn(D, generator=g)
    gamma = torch.randn(D, generator=g)
    guard = 3   # rows behind the last one, never to be touched
    xd = torch.full((rows + guard, D), SENTINEL, device="cuda")
    xd[:rows] = x.cuda()
    shape = (rows + guard, D // 32, 2, 32) if planes else (rows + guard, D)
    yd = torch.full(shape, 0x7B7B if planes else SENTINEL, dtype=torch.int16 if planes else torch.float32, device="cuda")
    gpu_ctx.op_add_row_layernorm(xd, r.cuda(), gamma.cuda(), planes=planes, rows=rows, out=yd)
    s = (x + r).cuda()                                     # the fp32 add the kernel stands in for
    assert torch.equal(xd[:rows], s), "x must hold the fp32 sum x + r"
    assert (xd[rows:] == SENTINEL).all() and (yd[rows:] == (0x7B7B if planes else SENTINEL)).all(), "written behind the last row"
    if planes:
        want = gpu_ctx.op_layernorm_planes(s, gamma.cuda(), D=D, ldy=D)
        assert torch.equal(yd[:rows], want.view(torch.int16)), "not the bits of layernorm_planes(x + r)"
        got = planes_value(yd[:rows].cpu())
    else:
        want = gpu_ctx.op_layernorm(s, gamma.cuda())
        assert torch.equal(yd[:rows], want), "not the bits of layernorm(x + r)"
        got = yd[:rows].cpu().double()
    ref = F.layer_norm(x.double() + r.double(), (D,), gamma.double(), None, 1e-5)
    e = rel(got, ref)
    print(f"add_row_layernorm rows={rows} D={D} planes={planes}: {e:.2e} of max|ref|")
    assert e < LN_BOUND


CFG_SHAPES = [(rows, V, ld, scale) for rows in (1, 4099) for V, ld in ((64, 96), (1024, 1056), (1024, 1024), (63, 70)) for scale in (0.0, 1.0, 3.0, -0.5)]
# the launch has at most 8192 workgroups of 256 threads: more than 2 097 152 elements per launch send a thread round its loop again - 8200 x 1024 / 4 vectors, 34000 x 63 scalars
CFG_SHAPES += [(8200, 1024, 1024, 3.0), (34000, 63, 64, 3.0)]


@pytest.mark.parametrize("rows,V,ld,scale", CFG_SHAPES)
def test_cfg_combine(gpu_ctx, rows, V, ld, scale):
    """In place, bit-equal to the fp32 torch expression null + (cond - null) * scale (three roundings, no FMA); pad columns of a leading dimension above V untouched.
    Rows 1 and 4099, V = 63 the scalar path, and one shape per path with more elements than one sweep of the grid."""
    g = torch.Generator().manual_seed(rows + V)
    cond = torch.randn(rows, ld, generator=g) * 7
    null = torch.randn(rows, ld + 4, generator=g) * 7
    cd, nd = cond.cuda(), null.cuda()
    gpu_ctx.op_cfg_combine(cd, nd, scale, V=V)
    c, n = cond[:, :V], null[:, :V]
    want = n + (c - n) * torch.tensor(scale, dtype=torch.float32)
    assert torch.equal(cd[:, :V].cpu(), want)
    assert torch.equal(cd[:, V:].cpu(), cond[:, V:]), "pad columns were written"
    assert torch.equal(nd.cpu(), null)


def test_null_row_table_through_the_null_forward():
    """The [layers, D] table bevgen_finalize computes (r = to_out vec(null_v), fp64 accumulation), read back through bevgen_muse_forward_ex on a one-layer model whose
    self-attention and feed-forward add nothing (their output projections are zero) and whose rows start from the token embedding alone: embed = LayerNorm(token_emb[id]
    + r).  null_v is scaled up so that r carries the row.  Versus fp64 at 1e-6 of the largest value (the LayerNorm's own fp32 round-off is a few 1e-7)."""
    from bevgen_amd import presets
    from bevgen_amd.runtime import Context

    cfg = presets.route_m(3, num_layers=1, dim=128, heads=2, vocab=64, cam_res=(64, 64), cam_latent_res=(4, 4), bev_latent_res=(4, 4))
    sd = dict(cases.maskgit_state_dict(cfg, 4321))
    p = "transformer."
    lp = p + "transformer_blocks.layers.0."
    for k in (p + "pos_emb.weight", p + "img_embed.weight", p + "cam_embed.weight", lp + "0.to_out.weight", lp + "2.4.weight"):
        sd[k] = torch.zeros_like(sd[k])
    nkv = sd[lp + "1.null_kv"].clone()
    nkv[1] *= 40.0 / nkv[1].abs().max()
    sd[lp + "1.null_kv"] = nkv
    sd = {k: (sd["transformer." + k[len("token_critic.net."):]] if k.startswith("token_critic.net.") else v) for k, v in sd.items()}
    bt = cases.inputs(cases.CASES["m_tiny_rays"], cfg)
    rows, T = bt["cond_ids"].shape[0] * cfg.num_cams, cfg.num_cam_tokens
    ids = torch.randint(0, cfg.vocab_size + 1, (rows, T), generator=torch.Generator().manual_seed(3))
    r = sd[lp + "1.to_out.weight"].double() @ nkv[1].reshape(-1).double()
    x = sd[p + "token_emb.weight"].double()[ids] + r
    assert r.abs().max() > 20 * sd[p + "token_emb.weight"].abs().max(), "r must carry the row"
    ref = F.layer_norm(x, (cfg.num_embed,), sd[p + "transformer_blocks.norm.gamma"].double(), None, 1e-5)
    ctx = Context(cfg, route="maskgit")
    ctx.load_state_dict({k: v for k, v in sd.items() if not k.startswith("token_critic.net.")})
    ctx.set_tables()
    ctx.finalize()
    _, embed = ctx.muse_forward(ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], want_logits=False, null_condition=True)
    e = rel(embed.cpu().double(), ref)
    print(f"null rows through the null forward: {e:.2e}")
    assert e < 1e-6
    _, cond = ctx.muse_forward(ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], want_logits=False)
    assert rel(cond.cpu().double(), ref) > 1e-2, "the conditional forward attends to the layout"
    ctx.close()
