"""MaskGit.forward's validation losses (TEST INFRASTRUCTURE): the case table of tests/golden/route_m_loss.npz, the rule that draws each case's inputs from a seed, and an
fp64 restatement of muse_net:629-729 in eval mode on top of oracle.restate.muse_forward.  Shared by tools/make_maskgit_loss_golden.py (which adds the imported reference's
results) and tests/test_maskgit_loss_{cpu,gpu}.py.  No library code is involved in anything here.
"""
import functools
import math
import os

import numpy as np
import torch

from oracle import cases, restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_m_loss.npz")

# case -> the noise seed its inputs are drawn from (tools/make_maskgit_loss_golden.py: the first seed from SEED_START upward that meets input_conditions)
LOSS_CASES = {"m_tiny_rays": 20260, "m_tiny_6cam": 20260, "m_fold": 20260, "m_tiny_heavy": 20260}
SEED_START = 20260
MIN_MARGIN = 1e-3       # top-2 margin of logits / temperature + gumbel at every masked position, under the fp64 restatement
LOSS_RTOL = 1e-6        # restatement against the reference's fp32 losses (the bound of the stage-1 fixtures)


def model(name):
    """(case, cfg, state_dict, batch) of a Route M parity case."""
    case = cases.CASES[name]
    cfg = case.make_cfg()
    return case, cfg, cases.case_state_dict(case, cfg), cases.inputs(case, cfg)


def draw_inputs(name, seed):
    """The inputs of a case under `seed`: ids [rows, T], time_u [rows], perm_u [rows, T], gumbel_u [rows, T, V], temperature.  time_u: row 0 and row 1 are given the values
    0.03 (n = T) and 0.97 (n = 1) unless the draw already holds a row with that count, so that every case has a fully masked row, a row with one masked token and rows between."""
    case, cfg, _, _ = model(name)
    rows, T, V = case.batch * cfg.num_cams, cfg.num_cam_tokens, cfg.vocab_size
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (rows, T), generator=g)
    time_u = torch.rand(rows, generator=g)
    perm_u = torch.rand(rows, T, generator=g)
    gumbel_u = torch.rand(rows, T, V, generator=g)
    temperature = float(0.25 + 0.5 * torch.rand((), generator=g))
    n = num_masked(time_u, T)
    if not (n == T).any():
        time_u[0] = 0.03
    if not (n == 1).any():
        time_u[1] = 0.97
    return {"ids": ids, "time_u": time_u, "perm_u": perm_u, "gumbel_u": gumbel_u, "temperature": temperature}


def num_masked(time_u, T):
    """muse_net:660-662 with the reference's own fp32 operations: clamp(round(T cos(pi/2 t)), min = 1)."""
    return (T * torch.cos(time_u.float() * math.pi * 0.5)).round().clamp(min=1)


def train_mask(perm_u, n):
    """muse_net:665-666: argsort(u) < n per row; equal uniforms rank by index (a stable sort), one of the orders torch's unstable argsort may return."""
    return torch.argsort(perm_u, dim=-1, stable=True) < n[:, None]


def _to64(sd):
    # (camera_bias_emb stays fp32: oracle.restate scatters it into an fp32 [L, L] matrix, exact either way - it is added to fp64 scores afterwards)
    return {k: (v.double() if v.is_floating_point() and not k.endswith("camera_bias_emb") else v) for k, v in sd.items()}


def restate(name, inp, with_critic=True, critic_loss_weight=1.0, dtype=torch.float64):
    """MaskGit.forward (eval mode, self critic) restated: dict of mask, x, critic_input, n, ce, bce, loss, margin (smallest top-2 margin of the perturbed logits over the
    masked positions), max_logit, max_critic_logit."""
    case, cfg, sd, bt = model(name)
    if dtype == torch.float64:
        sd = _to64(sd)
    I, E = bt["intrinsics_inv"].to(dtype), bt["extrinsics_inv"].to(dtype)
    ids = inp["ids"]
    rows, T = ids.shape
    V = cfg.vocab_size
    n = num_masked(inp["time_u"], T)
    mask = train_mask(inp["perm_u"], n)
    x = torch.where(mask, torch.full_like(ids, V), ids)
    def fwd(ids):
        # oracle.restate builds its constants (pixel plane, ones) in torch's default dtype: float64 for the duration of the call, restored on every exit path
        old = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            return R.muse_forward(sd, cfg, ids, bt["cond_ids"], I, E, depth=cfg.num_layers, heads=cfg.num_heads)
        finally:
            torch.set_default_dtype(old)

    logits, _ = fwd(ids=x)
    nll = torch.logsumexp(logits, -1) - logits.gather(-1, ids[..., None])[..., 0]
    out = {"n": n, "mask": mask, "x": x, "ce": nll[mask].mean(), "max_logit": logits.abs().max().item(), "logits": logits}
    if not with_critic:
        out["loss"] = out["ce"]
        return out
    pert = logits / max(inp["temperature"], 1e-10) + R.gumbel_from_uniform(inp["gumbel_u"].to(dtype))
    top2 = pert.topk(2, -1).values
    out["margin"] = (top2[..., 0] - top2[..., 1])[mask].min().item()
    ci = torch.where(mask, pert.argmax(-1), x)
    labels = (ids != ci).to(dtype)
    _, embed = fwd(ids=ci)
    z = embed @ sd["token_critic.to_pred.weight"][0] + sd["token_critic.to_pred.bias"][0]
    bce = (z.clamp(min=0) - z * labels + torch.log1p(torch.exp(-z.abs()))).mean()
    out.update({"critic_input": ci, "labels": labels, "bce": bce, "max_critic_logit": z.abs().max().item(), "loss": out["ce"] + critic_loss_weight * bce})
    return out


def input_conditions(inp, r):
    """The two conditions the comparisons rest on, decided by the inputs and the fp64 restatement `r` alone: (distinct uniforms within every perm_u row, margin >= MIN_MARGIN)."""
    distinct = all(len(np.unique(row)) == row.size for row in inp["perm_u"].numpy())
    return distinct, r["margin"] >= MIN_MARGIN


def count_conditions(inp):
    """every case: a row with n = 1, a row with n = T and rows in between"""
    T = inp["ids"].shape[1]
    n = num_masked(inp["time_u"], T)
    return bool((n == 1).any() and (n == T).any() and ((n > 1) & (n < T)).any())


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def fixture_inputs(name):
    g = fixture()
    return {"ids": torch.from_numpy(g[name + "_ids"]).long(), "time_u": torch.from_numpy(g[name + "_time_u"]), "perm_u": torch.from_numpy(g[name + "_perm_u"]),
            "gumbel_u": torch.from_numpy(g[name + "_gumbel_u"]), "temperature": float(g[name + "_temperature"])}


@functools.lru_cache(maxsize=None)
def fixture_restated(name):
    """the fp64 restatement on the fixture's inputs: computed once, shared by the tests, never modified"""
    return restate(name, fixture_inputs(name))
