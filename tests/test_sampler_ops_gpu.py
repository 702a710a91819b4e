"""Operator-level parity of the token sampling and scoring kernels (csrc/sampler.hip) through their bevgen_op_* entries: every kernel against an fp64 statement of the
same operation (oracle/restate.py where it states it; the builders and references live in tests/test_sampler_ref_cpu.py, which checks them without a GPU).

Shapes: rows in {1, 5, 37} (no multiple of the four waves of a workgroup) x vocabularies in {1, 7, 63, 64, 65, 100, 257, 1000, 1023, 1024} (one value per lane up to the
register limit of sixteen), row strides larger than the vocabulary, and for the scoring kernel both of its paths.  Padding columns hold 1e30: a kernel that reads
past V picks or scores something else.

Worst errors measured on an MI355X (each test prints its own, `pytest -s`): ar_score_rows 2.9e-6 absolute = 0.09 of its bound; critic_scores 2.5e-7 relative (bound 6e-6);
confidence scores 1.1e-7 absolute (bound 5e-6); rows left out of the noisy picks by the margin rule: none in any of the 324 cases."""
import math

import numpy as np
import pytest
import torch

from test_sampler_ref_cpu import (AR_TEMPS, AR_TOP_KS, MAX_EXCLUDED, ROWS, SEEDED, SEEDED_TEMP, TEMPS, U_LAST, VOCABS, _gen, ar_draw_case, ar_edge_case, conf_ref, distinct_logits,
                                  edge_variants, first_argmax, grid_logits, mask_some, maskgit_noisy_case, maskgit_seeded_case, philox_uniform_ref, ref_top_k, remask_case,
                                  remask_ref, score_ref, topk_counts)
from oracle import restate as R

pytestmark = pytest.mark.gpu

PAD = 1e30


def dev(t):
    return t.cuda().contiguous()


def padded(x, ld):
    """x [rows, V] in a [rows, ld] device buffer whose other columns hold PAD."""
    buf = torch.full((x.shape[0], ld), PAD)
    buf[:, : x.shape[1]] = x
    return buf.cuda()


def offset_view(x, ld=None):
    """The same as a view that starts 4 bytes into an aligned allocation."""
    rows, V = x.shape
    ld = ld or V
    buf = torch.full((rows * ld + 1,), PAD).cuda()
    v = buf[1:].view(rows, ld)
    v[:, :V] = x.cuda()
    assert v.data_ptr() % 16 == 4
    return v


def refused(match):
    from bevgen_amd import _lib

    return pytest.raises(_lib.BevgenError, match=match)


def consume_status(ctx, expect):
    """After a call whose kernel may have raised a bit: the word as the host sees it, reported and cleared the way a caller meets it (synchronize())."""
    from bevgen_amd import _lib

    torch.cuda.synchronize()
    word = ctx.status()
    try:
        if expect:
            assert word & _lib.STATUS_NONFINITE_LOGITS, word
            with pytest.raises(_lib.BevgenError, match="NaN / inf logit") as ei:
                ctx.synchronize()
            assert ei.value.code == _lib.ERR_NUMERIC
        else:
            assert word == 0
            ctx.synchronize()
    finally:
        if ctx.status():   # never leave a word behind for the next test of the shared context
            try:
                ctx.synchronize()
            except _lib.BevgenError:
                pass
    assert ctx.status() == 0


# ================================================================================================ remask
@pytest.mark.parametrize("duplicates", [False, True])
@pytest.mark.parametrize("T", [1, 16, 350, 1000])
@pytest.mark.parametrize("rows", ROWS)
def test_remask(gpu_ctx, rows, T, duplicates):
    c = remask_case(rows, T, duplicates)
    scores = dev(c["scores"])
    for n_mask in sorted({0, 1, T // 2, T}):
        for init in (None, c["init_ids"]):
            ids = dev(c["ids"])
            gpu_ctx.op_remask(ids, scores, n_mask, c["mask_id"], None if init is None else dev(init))
            assert torch.equal(ids.cpu(), remask_ref(c["ids"], c["scores"], n_mask, c["mask_id"], init)), (n_mask, init is not None)


def test_remask_refuses_rows_beyond_the_dynamic_lds(gpu_ctx):
    T = 16384 + 1
    with refused("dynamic LDS"):
        gpu_ctx.op_remask(torch.zeros((1, T), dtype=torch.int64).cuda(), torch.zeros((1, T)).cuda(), 1, 7)


# ================================================================================================ maskgit_pick
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("rows", ROWS)
def test_maskgit_pick_noiseless_is_the_first_maximum(gpu_ctx, rows, V):
    g = _gen(51, rows, V)
    x = grid_logits(rows, V, g)
    ids0 = mask_some(rows, V, g)
    exp = torch.where(ids0 == V, first_argmax(x), ids0)
    for ld, k in ((V, V), (V + 3, 1)):   # (without noise the top-k filter does not enter)
        ids = dev(ids0)
        gpu_ctx.op_maskgit_pick(ids, padded(x, ld), V, mask_id=V, k=k, ldl=ld)
        assert torch.equal(ids.cpu(), exp), (ld, k)


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("rows", ROWS)
def test_maskgit_pick_explicit_noise(gpu_ctx, rows, V):
    """argmax(topk_filter(x, k) / max(t, 1e-10) + gumbel(u)) in fp64; rows whose two best perturbed values are closer than 1e-5 relative are left out: none on the seeds
    used (share 0.0 in every case; the cap of 2 % is checked by the reference alone in test_sampler_ref_cpu.py)."""
    for k in topk_counts(V):
        for t in TEMPS:
            c = maskgit_noisy_case(rows, V, k, t)
            left_out = 1.0 - c["ok"].float().mean().item()
            assert left_out <= MAX_EXCLUDED
            ld = V + 5 if t == 0.35 else V
            ids = dev(c["ids"])
            gpu_ctx.op_maskgit_pick(ids, padded(c["logits"], ld), V, mask_id=V, k=k, temperature=t, gumbel_u=dev(c["u"]), ldl=ld)
            out = ids.cpu()
            masked = c["ids"] == V
            assert torch.equal(out[~masked], c["ids"][~masked])
            cmp = masked & c["ok"]
            assert torch.equal(out[cmp], c["pred"][cmp]), (k, t)
            print(f"maskgit_pick explicit noise rows={rows} V={V} k={k} t={t}: left out {left_out:.3f}")


@pytest.mark.parametrize("stream,V", [(0, 64), (0, 100), (0, 1024), (1, 0)])
def test_philox_uniform_is_philox4x32_10(gpu_ctx, stream, V):
    n = 4096 + 37
    for seed, it in ((1, 0), (0x1234567890ABCDEF, 17)):
        out = gpu_ctx.philox_uniform(seed, it, stream, n, V).cpu()
        assert torch.equal(out, philox_uniform_ref(seed, it, stream, n, V))


@pytest.mark.parametrize("V", [100, 1000, 1024])
@pytest.mark.parametrize("rows", ROWS)
def test_maskgit_pick_in_kernel_noise_equals_the_written_uniforms(gpu_ctx, rows, V):
    ids0 = torch.full((rows,), V, dtype=torch.int64)
    for seed, it in SEEDED:
        c = maskgit_seeded_case(rows, V, seed, it)
        u = gpu_ctx.philox_uniform(seed, it, 0, rows * V, V)
        assert torch.equal(u.cpu().reshape(rows, V), c["u"])
        a, b, xd = dev(ids0), dev(ids0), dev(c["logits"])
        gpu_ctx.op_maskgit_pick(a, xd, V, mask_id=V, k=c["k"], temperature=SEEDED_TEMP, seed=seed, it=it)
        gpu_ctx.op_maskgit_pick(b, xd, V, mask_id=V, k=c["k"], temperature=SEEDED_TEMP, gumbel_u=u)
        assert torch.equal(a.cpu(), b.cpu())
        assert 1.0 - c["ok"].float().mean().item() <= MAX_EXCLUDED
        assert torch.equal(a.cpu()[c["ok"]], c["pred"][c["ok"]])


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("rows", ROWS)
def test_maskgit_pick_confidence_scores(gpu_ctx, rows, V):
    """1 - softmax(x)[pred] over the unfiltered logits against fp64, absolute 5e-6.  Worst measured over all cases: 1.1e-7."""
    k, t = math.ceil(0.1 * V), 1.0
    c = maskgit_noisy_case(rows, V, k, t)
    masked = c["ids"] == V
    worst = 0.0
    for noisy in (False, True):
        pred, ok = (c["pred"], c["ok"]) if noisy else (first_argmax(c["logits"]), torch.ones(rows, dtype=torch.bool))
        ref = conf_ref(c["logits"], pred)
        for mode in (1, 2):
            ids, conf = dev(c["ids"]), torch.full((rows,), 7.0).cuda()
            gpu_ctx.op_maskgit_pick(ids, padded(c["logits"], V + 2), V, mask_id=V, k=k, temperature=t, gumbel_u=dev(c["u"]) if noisy else None, conf_scores=conf, conf_mode=mode,
                                    ldl=V + 2)
            out, conf = ids.cpu(), conf.cpu()
            assert torch.equal(out[~masked], c["ids"][~masked])                    # ids change only where masked, in both modes
            assert torch.equal(out[masked & ok], pred[masked & ok])
            scored = ok & (masked if mode == 1 else torch.ones_like(masked))
            if mode == 1:
                assert bool((conf[~masked] == -1e5).all())
            err = (conf[scored].double() - ref[scored]).abs().max().item() if bool(scored.any()) else 0.0
            worst = max(worst, err)
            assert err <= 5e-6, (noisy, mode, err)
    print(f"conf_scores rows={rows} V={V}: worst |err| {worst:.2e}")


def test_maskgit_pick_refusals(gpu_ctx):
    ids = torch.full((5,), 7, dtype=torch.int64).cuda()
    x = torch.zeros((5, 1025)).cuda()
    with refused("vocabulary 1025"):
        gpu_ctx.op_maskgit_pick(ids, x, 1025, mask_id=7, k=3)
    with refused("top-k count 0"):
        gpu_ctx.op_maskgit_pick(ids, x, 100, mask_id=7, k=0, ldl=1025)
    with refused("top-k count 0"):                                                # MaskGit.generate's ceil((1 - 1.0) V) = 0: refused, not a token 0x7fffffff
        gpu_ctx.op_maskgit_pick(ids, x, 100, mask_id=7, topk_filter_thres=1.0, seed=5, ldl=1025)
    with refused("without an output buffer"):
        gpu_ctx.op_maskgit_pick(ids, x, 100, mask_id=7, k=3, conf_mode=1, ldl=1025)
    with refused("without an output buffer"):
        gpu_ctx.op_maskgit_pick(ids, x, 100, mask_id=7, k=3, conf_mode=2, ldl=1025)
    assert bool((ids.cpu() == 7).all())


# ================================================================================================ critic_scores
@pytest.mark.parametrize("D", [4, 252, 256, 1024, 1028])
@pytest.mark.parametrize("rows", ROWS)
def test_critic_scores(gpu_ctx, rows, D):
    """embed . w + b + ((u - 0.5) noise_scale) frac against fp64 at the bound of test_gemm (6e-6 relative).  Worst measured over all cases: 2.5e-7."""
    g = _gen(61, rows, D)
    e = torch.randn(rows, D, generator=g)
    w = torch.randn(D, generator=g) / math.sqrt(D)
    b = torch.randn(1, generator=g) + 2.0
    u = torch.rand(rows, generator=g)
    dot = e.double() @ w.double() + b.double()
    worst = 0.0
    for lde in (D, D + 4):
        for mode in ("explicit", "half", "seeded"):
            for noise_scale, frac in ((0.0, 0.0), (1.0, 0.5), (1.0, 0.0), (0.0, 0.5)):
                if mode == "explicit":
                    kw, uu = dict(u=dev(u)), u
                elif mode == "half":
                    kw, uu = dict(), torch.full((rows,), 0.5)
                else:
                    kw = dict(seed=4242, it=3)
                    uu = gpu_ctx.philox_uniform(4242, 3, 1, rows).cpu()
                    assert torch.equal(uu, philox_uniform_ref(4242, 3, 1, rows))
                ref = dot + ((uu.double() - 0.5) * noise_scale) * frac
                assert float(ref.abs().max()) > 0.1                                 # (a property of the inputs: the relative bound below has something to be relative to)
                out = gpu_ctx.op_critic_scores(padded(e, lde), dev(w), dev(b), D, noise_scale=noise_scale, frac=frac, lde=lde, **kw).cpu().double()
                err = ((out - ref).abs().max() / ref.abs().max()).item()
                worst = max(worst, err)
                assert err < 6e-6, (lde, mode, noise_scale, frac, err)
    print(f"critic_scores rows={rows} D={D}: worst rel {worst:.2e}")


def test_critic_scores_refusals(gpu_ctx):
    e, w, b = torch.zeros((5, 16)).cuda(), torch.zeros((16,)).cuda(), torch.zeros((1,)).cuda()
    with refused("multiple of 4"):
        gpu_ctx.op_critic_scores(e, w, b, 6)
    with refused("lde % 4"):
        gpu_ctx.op_critic_scores(e, w, b, 8, lde=10)
    with refused("aligned"):
        gpu_ctx.op_critic_scores(offset_view(torch.zeros(5, 8), 12), w, b, 8)
    with refused("aligned"):
        gpu_ctx.op_critic_scores(e, offset_view(torch.zeros(1, 8))[0], b, 8)


# ================================================================================================ ar_pick
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("rows", ROWS)
def test_ar_pick_greedy(gpu_ctx, rows, V):
    x = grid_logits(rows, V, _gen(71, rows, V))
    assert V < 2 or int((x[0] == x[0].max()).sum()) >= 2                             # rows with a duplicated maximum are among them
    for t, ld in ((0.5, V), (4.0, V + 3)):
        xd = padded(x, ld)
        for top_k in sorted({0, 1, 3, max(V - 1, 0), V, V + 5}):
            ref = R.pick_token(x.double(), t, ref_top_k(top_k, V), None)
            assert torch.equal(ref, first_argmax(x))
            out = gpu_ctx.op_ar_pick(xd, V, top_k=top_k, temperature=t, ldl=ld).cpu()
            assert torch.equal(out, ref), (t, top_k)


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("rows", ROWS)
def test_ar_pick_draw_returns_the_token_whose_cdf_interval_holds_u(gpu_ctx, rows, V):
    for top_k in AR_TOP_KS:
        for t in AR_TEMPS:
            c = ar_draw_case(rows, V, top_k, t, 3 if (top_k, t) == (8, 1.0) else 1)
            ld = V + 1 if t == 2.0 else V
            out = gpu_ctx.op_ar_pick(padded(c["logits"], ld), V, top_k=top_k, temperature=t, u=dev(c["u"][0]), ldl=ld).cpu()
            assert torch.equal(out, c["target"][0]), (top_k, t)
            assert torch.equal(out, R.pick_token(c["logits"].double(), t, ref_top_k(top_k, V), c["u"][0].double()))


@pytest.mark.parametrize("V", VOCABS)
def test_ar_pick_draw_at_both_ends_of_the_cdf(gpu_ctx, V):
    """u = 0: the first token with probability; u = nextafter(1, 0): the last one, never a filtered token behind it - also where ties at the k-th value keep k + 3 tokens."""
    rows = 5
    for top_k, ties in edge_variants(V):
        c = ar_edge_case(rows, V, top_k, ties)
        xd = dev(c["logits"])
        out0 = gpu_ctx.op_ar_pick(xd, V, top_k=top_k, u=torch.zeros(rows).cuda()).cpu()
        out1 = gpu_ctx.op_ar_pick(xd, V, top_k=top_k, u=torch.full((rows,), U_LAST).cuda()).cpu()
        assert torch.equal(out0, c["first"]), (top_k, ties)
        assert torch.equal(out1, c["last"]), (top_k, ties)
        assert bool(c["kept"].gather(1, out1[:, None]).all())


@pytest.mark.parametrize("V", [100, 1000])
@pytest.mark.parametrize("rows", ROWS)
def test_ar_pick_forced_tokens_and_the_device_step_counter(gpu_ctx, rows, V):
    steps, top_k, t = 3, 8, 1.0
    c = ar_draw_case(rows, V, top_k, t, steps)
    g = _gen(73, rows, V)
    forced = torch.where(torch.rand(steps, rows, generator=g) < 0.4, torch.randint(0, V + 50, (steps, rows), generator=g), torch.full((steps, rows), -1))
    forced[:, 0] = torch.tensor([V + 7, -1, 3])                                       # step 0 forced beyond the vocabulary, step 1 drawn, step 2 forced
    xd, ud, fd = dev(c["logits"]), dev(c["u"]), dev(forced)
    for step in (0, 2):
        counter = torch.tensor([step], dtype=torch.int32).cuda()
        exp = torch.where(forced[step] >= 0, forced[step], c["target"][step])
        assert torch.equal(gpu_ctx.op_ar_pick(xd, V, top_k=top_k, temperature=t, u=ud, step=counter, forced=fd).cpu(), exp)
        assert torch.equal(gpu_ctx.op_ar_pick(xd, V, top_k=top_k, temperature=t, u=ud, step=counter).cpu(), c["target"][step])
        greedy = torch.where(forced[step] >= 0, forced[step], first_argmax(c["logits"]))
        assert torch.equal(gpu_ctx.op_ar_pick(xd, V, top_k=top_k, temperature=t, step=counter, forced=fd).cpu(), greedy)
    # without a counter: the first row of both
    assert torch.equal(gpu_ctx.op_ar_pick(xd, V, top_k=top_k, temperature=t, u=ud, forced=fd).cpu(), torch.where(forced[0] >= 0, forced[0], c["target"][0]))


@pytest.mark.parametrize("with_img", [False, True])
@pytest.mark.parametrize("D", [4, 1020, 1024, 2052])
@pytest.mark.parametrize("rows", ROWS)
def test_ar_pick_tail_writes_the_token_and_the_next_embedding_row(gpu_ctx, rows, D, with_img):
    V, Cn, T, step = 100, 3, 4, 2
    N, vocab_rows = Cn * T, V + 1
    g = _gen(79, rows, D, with_img)
    x = grid_logits(rows, V, g)
    fwd = torch.randperm(N, generator=g)
    j = int(fwd[step])
    tok_emb, pos_emb = torch.randn(vocab_rows, D, generator=g), torch.randn(N, D, generator=g)
    img = torch.randn(rows, N, D, generator=g) if with_img else None
    forced = torch.full((N, rows), -1, dtype=torch.int64)
    if rows > 1:
        forced[step, rows - 1] = vocab_rows + 5                                       # beyond the embedding table: the last row is used
    token = torch.where(forced[step] >= 0, forced[step], first_argmax(x))
    emb = tok_emb[token.clamp(0, vocab_rows - 1)]
    exp_x = ((emb + img[:, j]) if with_img else emb) + pos_emb[j]                     # fp32, in the association of the kernel
    out_all = torch.full((rows, N), -7, dtype=torch.int64).cuda()
    xbuf = torch.full((rows + 1, D), 123.0).cuda()
    counter = torch.tensor([step], dtype=torch.int32).cuda()
    out = gpu_ctx.op_ar_pick(dev(x), V, step=counter, forced=dev(forced), out_all=out_all, fwd_idx=dev(fwd), tok_emb=dev(tok_emb), img_embed=None if img is None else dev(img),
                             pos_emb=dev(pos_emb), x=xbuf[:rows], C_=Cn, T=T).cpu()
    assert torch.equal(out, token)
    exp_all = torch.full((rows, N), -7, dtype=torch.int64)
    exp_all[:, j] = token
    assert torch.equal(out_all.cpu(), exp_all)
    assert torch.equal(xbuf[:rows].cpu(), exp_x)                                      # bit equality
    assert bool((xbuf[rows].cpu() == 123.0).all())
    # out_all alone (no embedding row): x stays untouched
    out_all.fill_(-7)
    gpu_ctx.op_ar_pick(dev(x), V, step=counter, forced=dev(forced), out_all=out_all, fwd_idx=dev(fwd))
    assert torch.equal(out_all.cpu(), exp_all)


def test_ar_pick_refusals(gpu_ctx):
    x = torch.zeros((5, 1025)).cuda()
    with refused("vocabulary 1025"):
        gpu_ctx.op_ar_pick(x, 1025)
    out_all, fwd = torch.zeros((5, 4), dtype=torch.int64).cuda(), torch.arange(4).cuda()
    with refused("device counter"):
        gpu_ctx.op_ar_pick(x, 100, ldl=1025, out_all=out_all, fwd_idx=fwd)
    counter = torch.zeros((1,), dtype=torch.int32).cuda()
    emb = torch.zeros((101, 6)).cuda()
    with refused("D % 4 == 0"):
        gpu_ctx.op_ar_pick(x, 100, ldl=1025, step=counter, out_all=out_all, fwd_idx=fwd, tok_emb=emb, pos_emb=emb, x=torch.zeros((5, 6)).cuda(), C_=1, T=4)


# ================================================================================================ ar_score_rows
SCORE_VARIANTS = {   # name: (V, ldl - V, 4-byte offset)
    "reg4": (4, 0, False), "reg1000": (1000, 0, False), "reg2048": (2048, 0, False), "reg1000_ld": (1000, 8, False),
    "strided1023": (1023, 0, False), "strided2052": (2052, 0, False), "strided1000_offset": (1000, 0, True), "strided1000_ld": (1000, 3, False),
}


def _score_inputs(rows, V):
    g = _gen(83, rows, V)
    B, b, s0 = 3, 2, 4
    N = s0 + rows + 7
    x = torch.randn(rows, V, generator=g) * 8                                         # |x| up to about 30
    return dict(x=x, B=B, b=b, s0=s0, N=N, fwd=torch.randperm(N, generator=g), target=torch.randint(0, V, (B, N), generator=g),
                weight=torch.rand(B, N, generator=g) * 2)


def _score_bound(mag):
    """Twice the fp32 model (2^-24 per rounding): the sum of <= 32 terms per lane and a 6-level tree with expf, ~40 x 2^-24 relative, is absolute after the log; three
    roundings at the magnitudes of the maximum, the logsumexp and the target's logit."""
    return 6e-6 + 4e-7 * mag


@pytest.mark.parametrize("variant", list(SCORE_VARIANTS))
@pytest.mark.parametrize("rows", ROWS)
def test_ar_score_rows(gpu_ctx, rows, variant):
    """fp64 logsumexp - x[t] per row within 6e-6 + 4e-7 (|max| + |logsumexp| + |x_t|).  Worst measured over all cases: 2.9e-6 (register path, V = 2048), 0.09 of
    the bound; the strided path 2.8e-6."""
    V, extra, off = SCORE_VARIANTS[variant]
    c = _score_inputs(rows, V)
    ld = V + extra
    xd = offset_view(c["x"], ld) if off else padded(c["x"], ld)
    sel = c["fwd"][c["s0"] : c["s0"] + rows]
    t, w = c["target"][c["b"], sel], c["weight"][c["b"], sel]
    ref, mag = score_ref(c["x"], t)
    fwd, tgt, wgt = dev(c["fwd"]), dev(c["target"]), dev(c["weight"])
    kw = dict(b=c["b"], s0=c["s0"], N=c["N"], ldl=ld)
    nll, wnll = torch.full((rows + 1,), 7.0).cuda(), torch.full((rows + 1,), 7.0).cuda()
    gpu_ctx.op_ar_score_rows(xd, V, fwd, target=tgt, weight=wgt, rows=rows, nll=nll, wnll=wnll, **kw)
    nll, wnll = nll.cpu(), wnll.cpu()
    ratio = ((nll[:rows].double() - ref).abs() / _score_bound(mag)).max().item()
    print(f"ar_score_rows rows={rows} {variant}: worst |err| {(nll[:rows].double() - ref).abs().max().item():.2e} = {ratio:.3f} of the bound")
    assert ratio <= 1.0
    assert torch.equal(wnll[:rows], w * nll[:rows])                                   # one fp32 product
    assert float(nll[rows]) == 7.0 and float(wnll[rows]) == 7.0
    # no weight, no nll buffer: the weighted buffer carries the plain value
    wn2 = torch.full((rows,), 7.0).cuda()
    gpu_ctx.op_ar_score_rows(xd, V, fwd, target=tgt, rows=rows, wnll=wn2, **kw)
    assert torch.equal(wn2.cpu(), nll[:rows])
    # no target: nothing is written
    n3, w3 = torch.full((rows,), 7.0).cuda(), torch.full((rows,), 7.0).cuda()
    gpu_ctx.op_ar_score_rows(xd, V, fwd, rows=rows, nll=n3, wnll=w3, **kw)
    assert bool((n3.cpu() == 7.0).all()) and bool((w3.cpu() == 7.0).all())
    assert gpu_ctx.status() == 0


@pytest.mark.parametrize("rows", ROWS)
def test_ar_score_rows_register_and_strided_paths_agree(gpu_ctx, rows):
    V = 1000
    c = _score_inputs(rows, V)
    sel = c["fwd"][c["s0"] : c["s0"] + rows]
    _, mag = score_ref(c["x"], c["target"][c["b"], sel])
    outs = []
    for xd in (dev(c["x"]), offset_view(c["x"])):
        nll = torch.empty((rows,)).cuda()
        gpu_ctx.op_ar_score_rows(xd, V, dev(c["fwd"]), target=dev(c["target"]), b=c["b"], s0=c["s0"], N=c["N"], nll=nll, wnll=torch.empty((rows,)).cuda())
        outs.append(nll.cpu().double())
    assert bool(((outs[0] - outs[1]).abs() <= _score_bound(mag)).all())


@pytest.mark.parametrize("variant", ["reg1000", "strided1023"])
def test_ar_score_rows_target_outside_the_vocabulary_is_nan_in_its_row_only(gpu_ctx, variant):
    V, rows = SCORE_VARIANTS[variant][0], 5
    c = _score_inputs(rows, V)
    sel = c["fwd"][c["s0"] : c["s0"] + rows]
    target = c["target"].clone()
    target[c["b"], sel[1]], target[c["b"], sel[3]] = V, -1
    nll, wnll = torch.empty((rows,)).cuda(), torch.empty((rows,)).cuda()
    gpu_ctx.op_ar_score_rows(dev(c["x"]), V, dev(c["fwd"]), target=dev(target), weight=dev(c["weight"]), b=c["b"], s0=c["s0"], N=c["N"], nll=nll, wnll=wnll)
    bad = torch.tensor([False, True, False, True, False])
    assert torch.equal(torch.isnan(nll.cpu()), bad) and torch.equal(torch.isnan(wnll.cpu()), bad)
    ref, mag = score_ref(c["x"][~bad], target[c["b"], sel][~bad])
    assert bool(((nll.cpu()[~bad].double() - ref).abs() <= _score_bound(mag)).all())
    assert gpu_ctx.status() == 0                                                      # (a bad target is not a non-finite logit)


def test_ar_score_rows_refuses_positions_beyond_the_sequence(gpu_ctx):
    x, fwd = torch.zeros((5, 8)).cuda(), torch.arange(8).cuda()
    tgt = torch.zeros((1, 8), dtype=torch.int64).cuda()
    with refused("outside"):
        gpu_ctx.op_ar_score_rows(x, 8, fwd, target=tgt, s0=4, N=8, nll=torch.zeros(5).cuda(), wnll=torch.zeros(5).cuda())
    with refused("weighted-nll buffer"):
        gpu_ctx.op_ar_score_rows(x, 8, fwd, target=tgt, s0=0, N=8, nll=torch.zeros(5).cuda())


# ================================================================================================ mean_fixed_order
@pytest.mark.parametrize("n", [1, 255, 256, 257, 33600])
def test_mean_fixed_order(gpu_ctx, n):
    g = _gen(89, n)
    x = (10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 6 - 3) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()   # six decades, both signs
    ref = np.float32(math.fsum(x.double().tolist()) / n)
    xd = dev(x)
    a, b = gpu_ctx.op_mean_fixed_order(xd).cpu(), gpu_ctx.op_mean_fixed_order(xd).cpu()
    assert abs(float(a) - float(ref)) <= float(np.spacing(np.abs(ref))), (float(a), float(ref))
    assert a.view(torch.int32).item() == b.view(torch.int32).item()


# ================================================================================================ status word
def test_nan_logit_raises_the_status_word_only_where_it_is_read(gpu_ctx):
    rows, V = 5, 100
    g = _gen(97)
    x = distinct_logits(rows, V, g)
    x[2, 70] = float("nan")
    xd = dev(x)
    assert gpu_ctx.status() == 0
    # maskgit_pick: row 2 masked -> raised; row 2 unmasked with conf_mode 0 -> not read
    ids = torch.full((rows,), V, dtype=torch.int64).cuda()
    gpu_ctx.op_maskgit_pick(ids, xd, V, mask_id=V, k=10)
    consume_status(gpu_ctx, True)
    ids = torch.full((rows,), V, dtype=torch.int64)
    ids[2] = 3
    gpu_ctx.op_maskgit_pick(dev(ids), xd, V, mask_id=V, k=10, seed=9)
    consume_status(gpu_ctx, False)
    # ar_pick: drawn -> raised; row 2 forced -> not read
    gpu_ctx.op_ar_pick(xd, V, top_k=8)
    consume_status(gpu_ctx, True)
    forced = torch.full((1, rows), -1, dtype=torch.int64)
    forced[0, 2] = 11
    out = gpu_ctx.op_ar_pick(xd, V, top_k=8, forced=dev(forced)).cpu()
    consume_status(gpu_ctx, False)
    assert int(out[2]) == 11
    # ar_score_rows without a target is the finiteness check of the rows, on both paths
    fwd = torch.arange(rows).cuda()
    gpu_ctx.op_ar_score_rows(xd, V, fwd)
    consume_status(gpu_ctx, True)
    gpu_ctx.op_ar_score_rows(offset_view(x), V, fwd)
    consume_status(gpu_ctx, True)
    gpu_ctx.op_ar_score_rows(dev(x[:2]), V, fwd)
    consume_status(gpu_ctx, False)


def test_nan_critic_score_raises_the_status_word(gpu_ctx):
    e = torch.ones(5, 8)
    e[3, 5] = float("nan")
    w, b = torch.ones(8).cuda(), torch.zeros(1).cuda()
    out = gpu_ctx.op_critic_scores(dev(e), w, b).cpu()
    consume_status(gpu_ctx, True)
    assert torch.equal(torch.isnan(out), torch.tensor([False, False, False, True, False]))
    gpu_ctx.op_critic_scores(dev(torch.ones(5, 8)), w, b)
    consume_status(gpu_ctx, False)
