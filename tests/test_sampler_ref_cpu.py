"""fp64 references and input builders of the sampler operator tests (tests/test_sampler_ops_gpu.py imports them), checked here without a GPU:
the helpers agree with oracle/restate.py, the noisy cases leave out at most 2 % of their rows by the reference alone, the CDF-midpoint construction
round-trips through ``pick_token``, and the numpy Philox4x32-10 reproduces the published known-answer vectors.

Every builder is cached: a case's inputs and reference are computed once per session and shared (callers must not modify them)."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import restate as R

ROWS = (1, 5, 37)                                              # not multiples of the four waves of a workgroup
VOCABS = (1, 7, 63, 64, 65, 100, 257, 1000, 1023, 1024)        # one value per lane ... the register limit of 16
TEMPS = (1.0, 0.35, 0.0)
MARGIN = 1e-5                                                  # ~80 x the fp32 rounding of x / t + gumbel(u): ten roundings of 2^-24 plus two logf
MAX_EXCLUDED = 0.02


def _gen(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------------------------------ Philox4x32-10 (Salmon et al. 2011), layout of csrc/common.h
_M32 = np.uint64(0xFFFFFFFF)


def philox4(seed, idx, it, stream):
    """counter = (idx low, idx high, iteration, stream), key = (seed low, seed high) -> [n, 4] uint32."""
    idx = np.asarray(idx, dtype=np.uint64)
    c0, c1 = idx & _M32, idx >> np.uint64(32)
    c2, c3 = np.full_like(idx, it), np.full_like(idx, stream)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2      # 32 x 32 -> 64 bit: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_uniform_ref(seed, it, stream, n, V=0):
    """What bevgen_op_philox_uniform writes: stream 0 with V > 0 = element (row, i) is word (i / 64) & 3 of block row V + i % 64 + 256 (i / 256); else word 0 of block i.
    Uniform = the upper 24 bits times 2^-24."""
    i = np.arange(n, dtype=np.uint64)
    if stream == 0 and V > 0:
        row, e = i // np.uint64(V), i % np.uint64(V)
        lane, j = e & np.uint64(63), e >> np.uint64(6)
        words = philox4(seed, row * np.uint64(V) + lane + np.uint64(256) * (j >> np.uint64(2)), it, 0)
        x = words[np.arange(n), (j & np.uint64(3)).astype(np.int64)]
    else:
        x = philox4(seed, i, it, stream)[:, 0]
    return torch.from_numpy(((x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)))


# ------------------------------------------------------------------------------------------------ re-masking
def remask_ref(ids, scores, n_mask, mask_id, init_ids=None):
    """Stable descending sort: the n_mask highest scores get mask_id, the lower index first among equals (csrc/kernels.h); init ids != mask_id are re-imposed."""
    order = torch.sort(scores.double(), dim=-1, descending=True, stable=True).indices
    out = ids.clone().scatter_(1, order[:, :n_mask], mask_id)
    if init_ids is not None:
        keep = init_ids != mask_id
        out[keep] = init_ids[keep]
    return out


@functools.lru_cache(maxsize=None)
def remask_case(rows, T, duplicates):
    g = _gen(11, rows, T, duplicates)
    mask_id = 1024
    if duplicates:   # 8 distinct values: ranks are decided by the tie rule almost everywhere
        scores = torch.tensor([-1e5, -0.5, 0.0, 0.125, 0.25, 0.5, 0.75, 1.0])[torch.randint(0, 8, (rows, T), generator=g)]
    else:
        scores = torch.randn(rows, T, generator=g)
    ids = torch.randint(0, mask_id, (rows, T), generator=g)
    init = torch.where(torch.rand(rows, T, generator=g) < 0.3, torch.randint(0, mask_id, (rows, T), generator=g), torch.full((rows, T), mask_id))
    return dict(ids=ids, scores=scores, init_ids=init, mask_id=mask_id)


# ------------------------------------------------------------------------------------------------ MaskGit pick
def first_argmax(x):
    return torch.from_numpy(np.argmax(x.double().numpy(), axis=-1))   # numpy: the first occurrence, by contract


def grid_logits(rows, V, g, forced_ties=True):
    """Multiples of 1/8 in [-5, 5]: exact in fp32 and under division by a power of two; every second row gets its maximum at two places."""
    x = torch.randint(-40, 41, (rows, V), generator=g).float() / 8
    if forced_ties and V >= 2:
        for r in range(0, rows, 2):
            a, b = torch.randperm(V, generator=g)[:2].tolist()
            x[r, a] = x[r, b] = x[r].max() + 0.125
    return x


def distinct_logits(rows, V, g, span=12.0):
    """A permuted, jittered grid over [-span/2, span/2]: all values of a row differ (spacing >= span / 2V), so torch.topk has no tie to break at any k."""
    perm = torch.stack([torch.randperm(V, generator=g) for _ in range(rows)]).double()
    x = (perm + 0.5 * torch.rand(rows, V, generator=g, dtype=torch.float64) - V / 2) * (span / V)
    x = x.float()
    s = x.sort(dim=-1).values
    assert V == 1 or bool((s[:, 1:] > s[:, :-1]).all())
    return x


def topk_counts(V):
    return sorted({1, min(2, V), math.ceil(0.1 * V), V})


def thres_for_k(k, V):
    """A topk_filter_thres for which muse_net:454's ceil((1 - thres) V) is k."""
    thres = 1.0 - (k - 0.5) / V
    assert math.ceil((1 - thres) * V) == k, (k, V)
    return thres


def mask_some(rows, V, g, share=0.75):
    """ids [rows]: mask_id (= V) at about `share` of the positions - at least one - and a token elsewhere."""
    ids = torch.randint(0, V, (rows,), generator=g)
    m = torch.rand(rows, generator=g) < share
    m[int(torch.randint(0, rows, (1,), generator=g))] = True
    return torch.where(m, torch.full_like(ids, V), ids)


def margin_ok(perturbed):
    """Rows whose best perturbed value leads the second best by more than MARGIN * max(1, |best|) in fp64 (-inf = filtered: an infinite lead)."""
    if perturbed.shape[-1] == 1:
        return torch.ones(perturbed.shape[0], dtype=torch.bool)
    top = perturbed.topk(2, dim=-1).values
    return (top[:, 0] - top[:, 1]) > MARGIN * top[:, 0].abs().clamp_min(1.0)


def maskgit_noisy_ref(logits, u, k, temperature):
    """argmax(topk_filter(x, k) / max(t, 1e-10) + gumbel(u)) in fp64 -> (pred, rows to compare)."""
    V = logits.shape[-1]
    pert = R.topk_filter(logits.double(), thres_for_k(k, V)) / max(temperature, 1e-10) + R.gumbel_from_uniform(u.double())
    return first_argmax(pert), margin_ok(pert)


@functools.lru_cache(maxsize=None)
def maskgit_noisy_case(rows, V, k, temperature):
    g = _gen(23, rows, V, k, round(temperature * 100))
    logits = distinct_logits(rows, V, g)
    u = torch.rand(rows, V, generator=g)
    ids = mask_some(rows, V, g)
    pred, ok = maskgit_noisy_ref(logits, u, k, temperature)
    return dict(logits=logits, u=u, ids=ids, pred=pred, ok=ok)


SEEDED = ((99, 0), (0xABCDEF0123, 7))      # (noise seed, iteration) of the in-kernel-noise cases
SEEDED_TEMP = 0.7


@functools.lru_cache(maxsize=None)
def maskgit_seeded_case(rows, V, seed, it):
    """Every position masked, k = ceil(0.1 V); the uniforms are the ones Philox stream 0 gives for (seed, it, V)."""
    x = distinct_logits(rows, V, _gen(53, rows, V))
    u = philox_uniform_ref(seed, it, 0, rows * V, V).reshape(rows, V)
    k = math.ceil(0.1 * V)
    pred, ok = maskgit_noisy_ref(x, u, k, SEEDED_TEMP)
    return dict(logits=x, u=u, k=k, pred=pred, ok=ok)


def conf_ref(logits, pred):
    """1 - softmax(x)[pred] over the unfiltered logits, fp64."""
    return 1.0 - logits.double().softmax(-1).gather(1, pred[:, None])[:, 0]


# ------------------------------------------------------------------------------------------------ Route A pick
def ar_filtered(logits, temperature, top_k):
    x = logits.double() / temperature
    return R.top_k_logits(x, top_k) if 0 < top_k < x.shape[-1] else x


def ref_top_k(top_k, V):
    """The kernel's top_k (0 or >= V: off) as pick_token takes it."""
    return top_k if 0 < top_k < V else None


def cdf_midpoint_u(logits, temperature, top_k, g, min_mass=1e-4):
    """Per row a target token among those that survive the filter with at least `min_mass` of the probability, and the fp32 uniform at the middle of its fp64 CDF
    interval: the draw must return exactly that token (the interval is > 800 fp32 steps of u wide, the fp32 running sum is good to ~22 x 2^-24)."""
    p = ar_filtered(logits, temperature, top_k).softmax(-1)
    cdf = p.cumsum(-1)
    total = cdf[:, -1:]
    target = torch.multinomial((p >= min_mass).double(), 1, generator=g)
    hi = cdf.gather(1, target) / total
    lo = hi - p.gather(1, target) / total
    return ((lo + hi) / 2)[:, 0].float(), target[:, 0]


U_LAST = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
AR_TOP_KS = (0, 8, 100)
AR_TEMPS = (0.5, 1.0, 2.0)


@functools.lru_cache(maxsize=None)
def ar_draw_case(rows, V, top_k, temperature, steps=1):
    """Random logits and, per step, a target token per row with the uniform that draws it."""
    g = _gen(31, rows, V, top_k, round(temperature * 10), steps)
    x = torch.randn(rows, V, generator=g) * 2
    pairs = [cdf_midpoint_u(x, temperature, top_k, g) for _ in range(steps)]
    return dict(logits=x, u=torch.stack([p[0] for p in pairs]), target=torch.stack([p[1] for p in pairs]))


@functools.lru_cache(maxsize=None)
def ar_edge_case(rows, V, top_k, ties):
    x, kept = edge_logits(rows, V, top_k, _gen(37, rows, V, top_k, ties), ties)
    return dict(logits=x, kept=kept, first=first_argmax(kept.float()), last=V - 1 - first_argmax(kept.flip(-1).float()))


def edge_variants(V):
    return [(top_k, ties) for top_k in AR_TOP_KS for ties in (False, True) if not ties or (0 < top_k and top_k + 3 <= V)]


def edge_logits(rows, V, top_k, g, ties=False):
    """Rows for u = 0 and u = nextafter(1, 0): `top_k` survivors (all V without a filter) in [2, 4] at random places, everything else in [-6, 0].  Every survivor then
    carries at least e^-2 / V > 1e-4 of the mass, so both ends of the CDF are decided far from rounding.  ties: three more tokens sit exactly at the k-th largest value."""
    k = top_k if 0 < top_k < V else V
    x = -6.0 * torch.rand(rows, V, generator=g)
    kept = torch.zeros(rows, V, dtype=torch.bool)
    for r in range(rows):
        sel = torch.randperm(V, generator=g)[: min(V, k + 3 if ties else k)]
        x[r, sel] = 2.0 + 2.0 * torch.rand(len(sel), generator=g)
        if ties:
            x[r, sel[-4:]] = 2.0      # the k-th largest and three equals: k + 3 survivors
        kept[r, sel] = True
    return x, kept


# ------------------------------------------------------------------------------------------------ Route A scoring
def score_ref(logits, t):
    """fp64 logsumexp - x[t] per row, with the magnitudes its fp32 error bound is made of."""
    x = logits.double()
    lse = x.logsumexp(-1)
    xt = x.gather(1, t[:, None])[:, 0]
    return lse - xt, x.max(-1).values.abs() + lse.abs() + xt.abs()


# ================================================================================================ checks (no GPU)
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: counter / key all zero, all ones, and the digits of pi."""
    def one(ctr, key):
        return [int(v) for v in philox4(key[0] | (key[1] << 32), [ctr[0] | (ctr[1] << 32)], ctr[2], ctr[3])[0]]

    assert one((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert one((f, f, f, f), (f, f)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert one((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_philox_stream_layouts():
    u = philox_uniform_ref(77, 3, 0, 3 * 1024, 1024).reshape(3, 1024)
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and u.unique().numel() > 3000
    # element (row 2, i = 5 + 64 * 6): word 6 & 3 = 2 of block 2 * 1024 + 5 + 256
    w = philox4(77, [2 * 1024 + 5 + 256], 3, 0)[0]
    assert float(u[2, 5 + 64 * 6]) == float(np.float32(w[2] >> 8) * np.float32(2.0 ** -24))
    c = philox_uniform_ref(77, 3, 1, 10)
    assert float(c[7]) == float(np.float32(philox4(77, [7], 3, 1)[0, 0] >> 8) * np.float32(2.0 ** -24))


@pytest.mark.parametrize("T", [1, 16, 350])
def test_remask_ref_agrees_with_the_restated_loop_and_the_rank_rule(T):
    c = remask_case(5, T, False)
    for n_mask in sorted({0, 1, T // 2, T}):
        out = remask_ref(c["ids"], c["scores"], n_mask, c["mask_id"])
        if n_mask:   # restate.maskgit_generate: ids.scatter(1, scores.topk(n_mask).indices, mask_id) - the same set where no two scores are equal
            assert torch.equal(out, c["ids"].scatter(1, c["scores"].topk(n_mask, dim=-1).indices, c["mask_id"]))
        else:
            assert torch.equal(out, c["ids"])
    d = remask_case(5, T, True)
    s = d["scores"].numpy()
    idx = np.arange(T)
    rank = ((s[:, None, :] > s[:, :, None]) | ((s[:, None, :] == s[:, :, None]) & (idx[None, None, :] < idx[None, :, None]))).sum(-1)   # rank[r, i] = #{j ahead of i}
    for n_mask in sorted({0, 1, T // 2, T}):
        exp = torch.where(torch.from_numpy(rank < n_mask), torch.full_like(d["ids"], d["mask_id"]), d["ids"])
        keep = d["init_ids"] != d["mask_id"]
        assert torch.equal(remask_ref(d["ids"], d["scores"], n_mask, d["mask_id"]), exp)
        exp[keep] = d["init_ids"][keep]
        assert torch.equal(remask_ref(d["ids"], d["scores"], n_mask, d["mask_id"], d["init_ids"]), exp)


@pytest.mark.parametrize("V", VOCABS)
def test_noisy_cases_leave_out_at_most_two_percent_by_the_reference_alone(V):
    for rows in ROWS:
        for k in topk_counts(V):
            thres = thres_for_k(k, V)
            for t in TEMPS:
                c = maskgit_noisy_case(rows, V, k, t)
                s = c["logits"].sort(dim=-1, descending=True).values
                assert k == V or bool((s[:, k - 1] > s[:, k]).all())          # the k-th and (k+1)-th largest differ
                assert int(torch.isfinite(R.topk_filter(c["logits"].double(), thres)).sum(-1).unique()) == k
                left_out = 1.0 - c["ok"].float().mean().item()
                assert left_out <= MAX_EXCLUDED, (rows, V, k, t, left_out)
                assert bool((c["ids"] == V).any())


@pytest.mark.parametrize("V", [100, 1000, 1024])
def test_seeded_cases_leave_out_at_most_two_percent_by_the_reference_alone(V):
    for rows in ROWS:
        for seed, it in SEEDED:
            c = maskgit_seeded_case(rows, V, seed, it)
            assert 1.0 - c["ok"].float().mean().item() <= MAX_EXCLUDED, (rows, V, seed)


def test_margin_filter():
    p = torch.tensor([[1.0, 1.0 + 2e-5, 0.0], [1.0, 1.0 + 5e-6, 0.0], [3e10, 3e10 + 1e4, 0.0], [3e10, 3e10 + 1e6, 0.0], [2.0, float("-inf"), float("-inf")]], dtype=torch.float64)
    assert margin_ok(p).tolist() == [True, False, False, True, True]
    assert margin_ok(torch.zeros(3, 1, dtype=torch.float64)).all()


def test_noiseless_pick_reference_is_the_first_maximum():
    x = grid_logits(37, 257, _gen(5))
    am = first_argmax(x)
    assert bool((x.gather(1, am[:, None])[:, 0] == x.max(-1).values).all())
    for r in range(37):
        assert int(am[r]) == int((x[r] == x[r].max()).nonzero()[0])
    assert sum(int((x[r] == x[r].max()).sum()) > 1 for r in range(37)) >= 19
    # ... and it is what the restated generate loop computes without noise: argmax of the filtered logits
    assert torch.equal(R.pick_token(x.double(), 1.0, None, None), am)


@pytest.mark.parametrize("V", VOCABS)
def test_cdf_midpoint_round_trips_through_pick_token(V):
    for rows in ROWS:
        for top_k in AR_TOP_KS:
            for t in AR_TEMPS:
                c = ar_draw_case(rows, V, top_k, t, 3 if (top_k, t) == (8, 1.0) else 1)
                for u, target in zip(c["u"], c["target"]):
                    assert torch.equal(R.pick_token(c["logits"].double(), t, ref_top_k(top_k, V), u.double()), target)
                    assert bool(torch.isfinite(ar_filtered(c["logits"], t, top_k).gather(1, target[:, None])).all())
                    assert bool((ar_filtered(c["logits"], t, top_k).softmax(-1).gather(1, target[:, None]) >= 1e-4).all())


@pytest.mark.parametrize("V", VOCABS)
def test_edge_rows_decide_both_ends_of_the_cdf_far_from_rounding(V):
    rows = 5
    for top_k, ties in edge_variants(V):
        c = ar_edge_case(rows, V, top_k, ties)
        f = ar_filtered(c["logits"], 1.0, top_k)
        assert torch.equal(torch.isfinite(f), c["kept"])
        assert not ties or bool((c["kept"].sum(-1) == top_k + 3).all())     # more than k tokens survive
        assert float(f.softmax(-1)[c["kept"]].min()) > 1e-4
        for t in AR_TEMPS:   # (the survivors of a row do not depend on the temperature; their mass does: checked where the GPU test uses it, t = 1)
            assert torch.equal(R.pick_token(c["logits"].double(), t, ref_top_k(top_k, V), torch.zeros(rows, dtype=torch.float64)), c["first"])
        assert torch.equal(R.pick_token(c["logits"].double(), 1.0, ref_top_k(top_k, V), torch.full((rows,), U_LAST, dtype=torch.float64)), c["last"])


def test_top_k_tie_golden_is_reproduced():
    g = golden("route_a_a_tiny_blk16")
    if "topk_tie_in" not in g.files:
        return
    x, out = torch.from_numpy(g["topk_tie_in"]), torch.from_numpy(g["topk_tie_out"])
    assert torch.equal(ar_filtered(x, 1.0, 2).float(), out)
    # a draw at either end of such a row stays on a token the filter kept
    for u in (0.0, U_LAST):
        tok = R.pick_token(x.double(), 1.0, 2, torch.full((x.shape[0],), u, dtype=torch.float64))
        assert bool(torch.isfinite(out.gather(1, tok[:, None])).all())


def test_score_ref_is_cross_entropy():
    g = _gen(41)
    x = torch.randn(5, 1000, generator=g) * 8
    t = torch.randint(0, 1000, (5,), generator=g)
    nll, mag = score_ref(x, t)
    assert torch.allclose(nll, torch.nn.functional.cross_entropy(x.double(), t, reduction="none"), rtol=0, atol=1e-12)
    assert bool((mag >= nll.abs()).all())
