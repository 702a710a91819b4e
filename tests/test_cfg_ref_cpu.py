"""Classifier-free guidance of Route M without a GPU: the float64 restatement (tests/cfg_ref.py) against the imported reference, against its own shortcut, against the
unguided loop, and the conditions the exact-token GPU test (tests/test_cfg_gpu.py) rests on."""
import pytest
import torch

import cfg_ref as G
from cfg_ref import D_CASES, D_NOISES, MARGIN, TIMESTEPS, fixture, fp32_agrees, guided_run, noise_of, random_ids, rel
from oracle import restate as R


REFERENCE_CHILD = """
import sys, torch
import cfg_ref as G
from oracle.ref_import import refmodels as RM
case, cfg, sd, bt = G.fixture("m_tiny_rays")
mg, _ = RM.build_ref_maskgit(cfg, dict(sd))
ids = G.random_ids(case, cfg)
batch = {"intrinsics_inv": bt["intrinsics_inv"], "extrinsics_inv": bt["extrinsics_inv"]}
mg.transformer.train()
with torch.no_grad():
    lr, er = mg.transformer(ids, return_embed=True, cond_drop_prob=1.0, conditioning_token_ids=bt["cond_ids"], batch=batch)
    mg.transformer.eval()
    lc, _ = mg.transformer(ids, return_embed=True, conditioning_token_ids=bt["cond_ids"], batch=batch)
torch.save({"lr": lr, "er": er, "lc": lc}, sys.argv[1])
"""


def test_null_forward_equals_the_imported_reference_in_train_mode_with_full_condition_drop(tmp_path):
    """(a) muse_forward_null == the reference's TransformerMultiView in .train() mode with cond_drop_prob = 1.0 (it has no dropout layers) on m_tiny_rays.  Bound: fp32
    round-off - 2e-5 of the largest value, the bound oracle/ref_import/make_golden.py holds the conditional restatement to against the same module (the reference runs
    fp32 on the CPU with other summation trees than fp64).  The reference runs in a child process: importing it installs stand-in modules (hydra, pytorch_lightning,
    ...) into sys.modules, which must not reach the tests that run after this one."""
    import os
    import subprocess
    import sys

    from oracle.ref_import import stubs

    if not stubs.reference_available():
        pytest.skip("the reference tree is not on this machine")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    out = str(tmp_path / "ref.pt")
    r = subprocess.run([sys.executable, "-c", REFERENCE_CHILD, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ref = torch.load(out)
    lr, er, lc = ref["lr"], ref["er"], ref["lc"]
    case, cfg, sd, bt = fixture("m_tiny_rays")
    ids = random_ids(case, cfg)
    lo, eo = G.muse_forward_null(sd, cfg, ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads)
    print("null vs reference: logits", rel(lo, lr.double()), "embed", rel(eo, er.double()), "| null vs conditional", rel(lr, lc))
    assert rel(lo, lr.double()) < 2e-5 and rel(eo, er.double()) < 2e-5
    assert rel(lr, lc) > 0.1, "the null forward must differ from the conditional one"


@pytest.mark.parametrize("name", ["m_tiny_rays", "m_fold", "m_tiny_heavy"])
def test_masked_cross_attention_is_the_constant_row(name):
    """(b) the literal masked form equals x + to_out(null_v) to 1e-12 in fp64: exp(-finfo.max - finite) is exactly 0, the null key takes weight exactly 1."""
    case, cfg, sd, bt = fixture(name)
    ids = random_ids(case, cfg)
    kw = dict(depth=cfg.num_layers, heads=cfg.num_heads)
    la, ea = G.muse_forward_null(sd, cfg, ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], **kw)
    lb, eb = G.muse_forward_null(sd, cfg, ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], shortcut=True, **kw)
    assert rel(la, lb) < 1e-12 and rel(ea, eb) < 1e-12
    # ... and the same identity in fp32, where the library takes the shortcut: finfo(float32).max absorbs every finite score
    la, _ = G.muse_forward_null(sd, cfg, ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], dtype=torch.float32, **kw)
    lb, _ = G.muse_forward_null(sd, cfg, ids, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], dtype=torch.float32, shortcut=True, **kw)
    assert rel(la, lb) < 1e-5


@pytest.mark.parametrize("critic", [True, False])
def test_scale_one_is_the_unguided_loop(critic):
    """(c) maskgit_generate_guided(cond_scale = 1) returns restate.maskgit_generate's ids."""
    case, cfg, sd, bt = fixture("m_tiny_rays")
    for tag in D_NOISES:
        noise = noise_of(case, cfg, tag)
        want = R.maskgit_generate(sd, cfg, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads, timesteps=TIMESTEPS,
                                  noise=noise, use_token_critic=critic)
        got, _ = guided_run("m_tiny_rays", tag, critic, scale=1.0)
        assert torch.equal(got, want), tag


@pytest.mark.parametrize("critic", [True, False])
@pytest.mark.parametrize("tag", D_NOISES)
@pytest.mark.parametrize("name", D_CASES)
def test_guided_picks_are_decided_and_guidance_changes_the_tokens(name, tag, critic):
    """(d) what the exact-token GPU test rests on, from the restatement alone (scale 3, 6 timesteps, topk_filter_thres 0.9): every pick has a relative margin >= 1e-4,
    and at least half the guided ids differ from the unguided ones."""
    case, cfg, sd, bt = fixture(name)
    ids, trace = guided_run(name, tag, critic)
    m = G.pick_margins(trace)
    plain, _ = guided_run(name, tag, critic, scale=1.0)
    differ = (ids != plain).float().mean().item()
    gap = max(rel(t["null"], t["cond"]) for t in trace)
    print(f"{name} {tag} critic={critic}: {m.numel()} picks, smallest margin {m.min().item():.3e}, {100 * differ:.0f} % of ids differ, null vs cond up to {gap:.2f} max|logits|")
    assert m.min().item() >= MARGIN
    assert differ >= 0.5
    # the pinned set of runs whose fp32 evaluation returns the fp64 ids (cfg_ref.FP32_AGREES_WITHOUT_CRITIC says why the others do not): asserted in both directions
    assert fp32_agrees(name, tag, critic) == (critic or name in G.FP32_AGREES_WITHOUT_CRITIC)


@pytest.mark.parametrize("tag", D_NOISES)
def test_confidence_scores_with_remasking_of_earlier_tokens_do_not_agree_in_fp32(tag):
    """can_remask_prev_masked (score_mode 2) under guidance: on none of the cases does the fp32 evaluation return the fp64 ids - the GPU test checks that branch
    iteration by iteration (teacher-forced) and never as a free run."""
    assert not any(fp32_agrees(name, tag, False, remask=True) for name in D_CASES)
