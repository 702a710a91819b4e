"""kv_cache='i8' (int8 codes + one fp32 scale per (token, head) row, BEVGEN_KV_I8) through the whole Route A model: teacher forced through the step API on the golden
fixtures, as test_models_gpu.test_route_a_f16_kv_cache runs the fp16 cache.

The mode is lossy and opt-in; what is asserted is a CONDITION, not a measurement: finite logits, a clean status word, run-to-run bit identity, samples_per_layout against
the repeated-input run, and a cap of 0.1 on the worst per-step relative distance from the golden fp32 logits - a wrong plane, layer stride or scale gives O(1), while
the oracle's restatement with its K / V rows passed through the CPU quantiser gives 4e-3 .. 5e-3 on these fixtures (tests/test_kv_i8_cpu.py asserts that it stays below
the cap).  Each case prints its measured distance next to the fp16 cache's from the same run and the top-1 agreement (`pytest -s`)."""
import numpy as np
import pytest
import torch

import kv_i8_ref as Q
from conftest import golden
from oracle import cases

pytestmark = pytest.mark.gpu


def _t(a, dtype=None):
    t = torch.from_numpy(np.asarray(a))
    return t.to(dtype) if dtype is not None else t


def _teacher_forced(ctx, cfg, cond, I, E, want, forward_steps=0):
    """[N - forward_steps, B, V] logits of the steps from `forward_steps` on; the rows before them enter the cache through the one-pass forward (bevgen_ar_forward)"""
    if forward_steps:
        ctx.ar_forward(cond, I, E, want.reshape(want.shape[0], -1), n_steps=forward_steps, want_logits=False)
    else:
        ctx.ar_prefill(cond, I, E)
    T, out = cfg.num_cam_tokens, []
    for s in range(forward_steps, cfg.num_img_tokens):
        out.append(ctx.ar_logits().cpu())
        if s + 1 < cfg.num_img_tokens:
            j = int(cfg.forward_shuffle_idx[s])
            ctx.ar_decode_step(want[:, j // T, j % T])
    ctx.synchronize()                                           # reports (raises on) a pending status word
    assert ctx.status() == 0
    return torch.stack(out)


@pytest.mark.parametrize("name", ["a_tiny_blk16", "a_tiny_6cam", "a_tiny_d06"])
def test_route_a_i8_kv_cache(name):
    from bevgen_amd.runtime import Context

    case = cases.CASES[name]
    g = golden("route_a_" + name)
    cfg = case.make_cfg()
    sd = cases.golden_state_dict(case, cfg, g)
    cond, I, E = _t(g["cond_ids"], torch.long), _t(g["I_inv"]), _t(g["E_inv"])
    want = _t(g["sample_greedy"], torch.long)
    ref = _t(g["step_logits"])                                 # [N, B, V] of the reference's greedy run (fp32 model)
    runs = {}
    for kv in ("i8", "f16"):
        ctx = Context(cfg, route="ar", kv_cache=kv)
        ctx.load_state_dict(sd)
        ctx.set_tables()
        ctx.finalize()
        runs[kv] = _teacher_forced(ctx, cfg, cond, I, E, want)
        if kv == "i8":
            again = _teacher_forced(ctx, cfg, cond, I, E, want)
            assert torch.equal(runs[kv].view(torch.int32), again.view(torch.int32)), "two runs of the int8 cache differ"
            # shared-prefix fan-out: replicate_prefix must carry the codes AND the scales of the condition rows
            S = 2
            rep = lambda t: t.repeat_interleave(S, dim=0)
            x = ctx.ar_sample(cond, I, E, greedy=True).cpu()
            a = ctx.ar_sample(rep(cond), rep(I), rep(E), greedy=True).cpu()
            b = ctx.ar_sample(rep(cond), rep(I), rep(E), greedy=True, samples_per_layout=S).cpu()
            ctx.synchronize()
            assert ctx.status() == 0
            assert torch.equal(a, b) and torch.equal(a[0::S], x)
        ctx.close()
    assert bool(runs["i8"].isfinite().all())
    # every decode path the configuration can name (the default above is 'auto'; a path the shape does not support runs the per-operator step)
    # (chains = 2: every chain's kernels see a slice of a layer and the offset from it to its scale rows; forward: half of the rows are written by bevgen_ar_forward)
    half = cfg.num_img_tokens // 2
    for path, chains, fwd in (("fused", None, 0), ("fused", 2, 0), ("split", None, 0), ("per_op", None, 0), ("fused", None, half)):
        ctx = Context(cfg, route="ar", kv_cache="i8", decode_path=path, decode_chains=chains)
        ctx.load_state_dict(sd)
        ctx.set_tables()
        ctx.finalize()
        d = Q.step_distance(_teacher_forced(ctx, cfg, cond, I, E, want, forward_steps=fwd), ref[fwd:])
        ctx.close()
        print(f"{name}: decode_path={path} chains={chains} rows through ar_forward={fwd}: i8 cache {d:.2e}")
        assert d < 0.1, (path, chains, fwd, d)
    d_i8, d_f16 = Q.step_distance(runs["i8"], ref), Q.step_distance(runs["f16"], ref)
    agree = (runs["i8"].argmax(-1) == ref.argmax(-1)).float().mean().item()
    print(f"{name}: worst per-step relative logit distance from the fp32 model: i8 cache {d_i8:.2e}, f16 cache {d_f16:.2e}; top-1 agreement of the i8 cache {agree:.3f}")
    assert d_i8 < 0.1, d_i8
