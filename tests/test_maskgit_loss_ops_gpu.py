"""Operator-level tests of the three kernels behind bevgen_maskgit_loss (csrc/sampler.hip) through their bevgen_op_* entries.  Every output goes into a sentinel-filled
buffer with guard elements on both sides: a kernel that writes outside its rows, or leaves a row unwritten, is caught.

maskgit_train_mask: bit-exact against argsort(u, stable) < n on (rows, T) = (6, 16), (3, 350), (2, 256), (1, 1); counts 1, T and values between; one row with two equal
uniforms and a count that separates their ranks (the other order of the tie gives another mask: asserted); seeded run == explicit run on the written-out Philox stream 2.

masked_ce (V in {64, 65, 1000, 1024}, row pitch V + 3, padding 1e30, 13 positions = four workgroups) and critic_bce (D in {128, 192, 1024}, row pitch D + 4, 13 rows):
the rule of tests/test_frontend_ops_gpu.py, per element: |out - ref64| <= max(4 e_cpu, one fp32 ulp of ref64), where e_cpu is the largest error of the plain fp32 torch
statement of the same formula against fp64 on the same inputs - taken per case (one V / one D, all mask / label variants) and separately for the ordinary rows and the
extreme rows (logits at +-80, critic logits near +-90), so that the large magnitudes buy the ordinary rows no slack.  Same number of roundings, another summation tree and
fused multiply-adds; a dropped term is orders of magnitude above it.  The means: one fp32 ulp of the double mean of the kernel's own rows.

Measured on an MI355X (worst over the cases, `pytest -s` prints each), as fractions of the bound: masked_ce 0.25 on the ordinary rows and 0.25 on the +-80 rows (errors
2.1e-6 and 1.1e-5: on most rows the kernel's value is the fp32 torch statement's, bit for bit); critic_bce 0.67 on the ordinary rows (D = 192, labels all 1: 4.1e-7 against
e_cpu 1.5e-7), 0.21 on the +-90 rows (3.5e-6); every mean equals the rounded double mean of the kernel's rows."""
import numpy as np
import pytest
import torch

from bevgen_amd import _lib

pytestmark = pytest.mark.gpu

PAD = 1e30
GUARD = 64


class Guarded:
    """A [n] device buffer inside a sentinel-filled allocation with GUARD elements on both sides."""
    def __init__(self, n, dtype, sentinel):
        self.n, self.sentinel = n, sentinel
        self.buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n]

    def check(self):
        b = self.buf.cpu()
        assert (b[:GUARD] == self.sentinel).all() and (b[GUARD + self.n:] == self.sentinel).all(), "a kernel wrote outside its output"
        return b[GUARD:GUARD + self.n]


def ulp32(x):
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def clean_status(ctx):
    torch.cuda.synchronize()
    assert ctx.status() == 0
    ctx.synchronize()


# ================================================================================================ maskgit_train_mask
def _mask_case(rows, T):
    g = torch.Generator().manual_seed(900 + 7 * rows + T)
    ids = torch.randint(0, 64, (rows, T), generator=g)
    u = torch.rand(rows, T, generator=g)
    n = torch.randint(2, max(T, 3), (rows,), generator=g).clamp(max=T)
    n[0] = 1
    if rows > 1:
        n[1] = T
    tie_row = None
    if rows > 2 and T >= 8:
        tie_row = 2
        u[tie_row, 7] = u[tie_row, 3]
        n[tie_row] = 5    # argsort holds the indices 3 and 7 at neighbouring ranks r, r + 1: mask[r] = (3 < 5), mask[r + 1] = (7 < 5) - the other order swaps the two
    return ids, u, n.to(torch.int32), tie_row


def _mask_ref(u, n):
    return torch.argsort(u, dim=-1, stable=True) < n[:, None].long()


@pytest.mark.parametrize("rows,T", [(6, 16), (3, 350), (2, 256), (1, 1)])
def test_train_mask_is_argsort_below_n(gpu_ctx, rows, T):
    ids, u, n, tie_row = _mask_case(rows, T)
    mask_id = 64
    want = _mask_ref(u, n)
    assert torch.equal(want.sum(-1), n.long())
    if tie_row is not None:   # the other order of the tie is another mask: the test pins the rule
        r3 = int((u[tie_row] < u[tie_row, 3]).sum())
        other = torch.argsort(u[tie_row], stable=True).clone()
        other[r3], other[r3 + 1] = other[r3 + 1].clone(), other[r3].clone()
        assert not torch.equal(other < int(n[tie_row]), want[tie_row])
    gx, gm = Guarded(rows * T, torch.int64, -7), Guarded(rows * T, torch.uint8, 0xAB)
    gpu_ctx.op_maskgit_train_mask(ids.cuda(), n.cuda(), mask_id, perm_u=u.cuda(), x=gx.view.view(rows, T), mask=gm.view.view(rows, T))
    x, m = gx.check().view(rows, T), gm.check().view(rows, T)
    assert torch.equal(m, want.to(torch.uint8))
    assert torch.equal(x, torch.where(want, torch.full_like(ids, mask_id), ids))
    # seeded: Philox stream 2, plain element index, iteration 0 - the same mask as the explicit run on the uniforms written out
    seed = 0x1234_5678_9ABC + rows
    pu = gpu_ctx.philox_uniform(seed, 0, 2, rows * T).view(rows, T)
    xs, ms = gpu_ctx.op_maskgit_train_mask(ids.cuda(), n.cuda(), mask_id, seed=seed)
    xe, me = gpu_ctx.op_maskgit_train_mask(ids.cuda(), n.cuda(), mask_id, perm_u=pu)
    assert torch.equal(xs, xe) and torch.equal(ms, me)
    assert torch.equal(ms.cpu().bool(), _mask_ref(pu.cpu(), n))
    clean_status(gpu_ctx)


def test_train_mask_refusals(gpu_ctx):
    ids = torch.zeros((1, 4), dtype=torch.int64).cuda()
    n = torch.ones((1,), dtype=torch.int32).cuda()
    with pytest.raises(_lib.BevgenError, match="randomness"):
        gpu_ctx.op_maskgit_train_mask(ids, n, 64)
    big = torch.zeros((1, 13108), dtype=torch.int64).cuda()
    with pytest.raises(_lib.BevgenError, match="dynamic LDS"):
        gpu_ctx.op_maskgit_train_mask(big, n, 64, seed=5)


# ================================================================================================ masked_ce
P = 13   # positions: four workgroups of four waves, the last one partly empty
NEXT = 4  # of them, the first four are the extreme rows


def _ce_case(V):
    g = torch.Generator().manual_seed(1000 + V)
    x = torch.randn(P, V, generator=g) * 8
    for r in range(NEXT):   # rows at +-80
        x[r] = torch.where(torch.rand(V, generator=g) < 0.5, torch.tensor(80.0), torch.tensor(-80.0)) + torch.randn(V, generator=g) * 0.01
    ids = torch.randint(0, V, (P,), generator=g)
    ids[NEXT] = V - 1                                                     # the last column
    masks = {"one": torch.zeros(P, dtype=torch.bool), "all": torch.ones(P, dtype=torch.bool), "mixed": torch.rand(P, generator=g) < 0.5}
    masks["one"][5] = True
    masks["mixed"][0] = masks["mixed"][NEXT] = True
    return x, ids, masks


def _nll(x, ids):
    return torch.logsumexp(x, -1) - x.gather(-1, ids[:, None])[:, 0]


def _padded(x, ld):
    buf = torch.full((x.shape[0], ld), PAD)
    buf[:, : x.shape[1]] = x
    return buf.cuda()


def _e_cpu(pairs, groups):
    """per group: the largest |fp32 torch statement - fp64| over every (ref32, ref64) pair of the case"""
    return {gname: max(np.abs(r32[sel] - r64[sel]).max() for r32, r64 in pairs) for gname, sel in groups.items()}


def _check_rows(name, out, ref64, e_cpus, groups, written=None):
    """per element against max(4 e_cpu of the element's group, one ulp)"""
    worst = {}
    for gname, sel in groups.items():
        sel = sel if written is None else sel & written
        if not sel.any():
            continue
        e_cpu = e_cpus[gname]
        bound = np.maximum(4 * e_cpu, ulp32(ref64[sel]))
        frac = (np.abs(out[sel] - ref64[sel]) / bound).max()
        print(f"{name} {gname}: e_cpu {e_cpu:.2e}, worst error {np.abs(out[sel] - ref64[sel]).max():.2e} = {frac:.2f} of the bound")
        worst[gname] = frac
    assert all(f <= 1.0 for f in worst.values()), (name, worst)


@pytest.mark.parametrize("V", [64, 65, 1000, 1024])
def test_masked_ce(gpu_ctx, V):
    x, ids, masks = _ce_case(V)
    ld = V + 3
    xd, idd = _padded(x, ld), ids.cuda()
    ref64, ref32 = _nll(x.double(), ids).numpy(), _nll(x, ids).double().numpy()
    extreme = np.arange(P) < NEXT
    groups = {"ordinary": ~extreme, "+-80": extreme}
    e_cpus = _e_cpu([(ref32, ref64)], groups)
    for mname, mask in masks.items():
        gn = Guarded(P, torch.float32, -123.0)
        denom = int(mask.sum())
        _, mean = gpu_ctx.op_masked_ce(xd, V, idd, mask.to(torch.uint8).cuda(), denom=denom, nll=gn.view, ldl=ld)
        out = gn.check().double().numpy()
        m = mask.numpy()
        assert (out[~m] == 0).all(), "unmasked positions hold exactly 0"
        _check_rows(f"masked_ce V={V} {mname}", out, ref64, e_cpus, groups, written=m)
        want_mean = np.float32(out.sum() / denom)
        assert abs(float(mean) - float(want_mean)) <= ulp32(want_mean), (float(mean), want_mean)
        if mname == "all":   # two calls give the same bits
            gn2 = Guarded(P, torch.float32, -123.0)
            _, mean2 = gpu_ctx.op_masked_ce(xd, V, idd, mask.to(torch.uint8).cuda(), denom=denom, nll=gn2.view, ldl=ld)
            assert torch.equal(gn2.check().view(torch.int32), gn.check().view(torch.int32)) and torch.equal(mean2.view(torch.int32), mean.view(torch.int32))
    clean_status(gpu_ctx)


def test_masked_ce_flags_a_nonfinite_logit_of_a_masked_position(gpu_ctx):
    V = 65
    x, ids, masks = _ce_case(V)
    mask = masks["one"].to(torch.uint8).cuda()                 # position 5 alone
    bad = x.clone()
    bad[6, 3] = float("nan")                                   # unmasked: like the pick, the kernel reads masked positions only
    gpu_ctx.op_masked_ce(_padded(bad, V + 3), V, ids.cuda(), mask, ldl=V + 3)
    clean_status(gpu_ctx)
    bad[5, V - 1] = float("inf")
    gpu_ctx.op_masked_ce(_padded(bad, V + 3), V, ids.cuda(), mask, ldl=V + 3)
    torch.cuda.synchronize()
    assert gpu_ctx.status() & _lib.STATUS_NONFINITE_LOGITS
    with pytest.raises(_lib.BevgenError) as ei:
        gpu_ctx.synchronize()
    assert ei.value.code == _lib.ERR_NUMERIC and gpu_ctx.status() == 0
    with pytest.raises(_lib.BevgenError, match="vocabulary"):
        gpu_ctx.op_masked_ce(torch.zeros((1, 1025)).cuda(), 1025, ids[:1].cuda(), mask[:1])


# ================================================================================================ critic_bce
def _bce_case(D):
    g = torch.Generator().manual_seed(2000 + D)
    e = torch.randn(P, D, generator=g)
    w = torch.randn(D, generator=g) / D ** 0.5
    b = torch.tensor([0.1])
    for r in range(NEXT):   # z near +90 (even rows) and -90 (odd rows)
        e[r] = (90.0 if r % 2 == 0 else -90.0) * w / (w * w).sum() + 0.01 * torch.randn(D, generator=g)
    ids = torch.randint(0, 64, (P,), generator=g)
    mixed = torch.where(torch.rand(P, generator=g) < 0.5, ids, ids + 1)
    mixed[0], mixed[1] = ids[0], ids[1] + 1                                  # (+90, y = 0) and (-90, y = 1): the large losses
    return e, w, b, ids, {"all 0": ids.clone(), "all 1": ids + 1, "mixed": mixed}


def _bce(e, w, b, y):
    z = e @ w + b
    return z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs())), z


@pytest.mark.parametrize("D", [128, 192, 1024])
def test_critic_bce(gpu_ctx, D):
    e, w, b, ids, variants = _bce_case(D)
    ld = D + 4
    ed = torch.full((P, ld), PAD)
    ed[:, :D] = e
    ed, wd, bd, idd = ed.cuda(), w.cuda(), b.cuda(), ids.cuda()
    extreme = np.arange(P) < NEXT
    groups = {"ordinary": ~extreme, "+-90": extreme}
    refs = {v: (_bce(e, w, b, (ids != ci).float())[0].double().numpy(), _bce(e.double(), w.double(), b.double(), (ids != ci).double())) for v, ci in variants.items()}
    e_cpus = _e_cpu([(r32, r64.numpy()) for r32, (r64, _) in refs.values()], groups)
    for vname, ci in variants.items():
        ref64, z64 = refs[vname][1]
        assert abs(abs(z64[0].item()) - 90) < 2 and abs(abs(z64[1].item()) - 90) < 2
        gl = Guarded(P, torch.float32, -123.0)
        _, mean = gpu_ctx.op_critic_bce(ed, wd, bd, idd, ci.cuda(), D, loss_rows=gl.view, lde=ld)
        out = gl.check().double().numpy()
        _check_rows(f"critic_bce D={D} labels {vname}", out, ref64.numpy(), e_cpus, groups)
        want_mean = np.float32(out.sum() / P)
        assert abs(float(mean) - float(want_mean)) <= ulp32(want_mean), (float(mean), want_mean)
    clean_status(gpu_ctx)


def test_critic_bce_refusals(gpu_ctx):
    e, w, b, ids, variants = _bce_case(128)
    with pytest.raises(_lib.BevgenError, match="multiple of 4"):
        gpu_ctx.op_critic_bce(e.cuda(), w.cuda(), b.cuda(), ids.cuda(), ids.cuda(), 126)
