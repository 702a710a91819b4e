"""Float64 restatement of Route M's classifier-free guidance (TEST INFRASTRUCTURE, next to oracle/restate.py whose functions it is built on).

The reference's "null" forward is ``TransformerMultiView.forward`` with ``context_mask = False`` for every scene (muse_net:352-354 with cond_drop_prob = 1, honoured in
``.train()`` mode only); ``forward_with_cond_scale`` mixes it with the conditional one as ``null + (cond - null) * cond_scale`` (muse_net:272-276).  Here:

  muse_forward            the forward in any dtype; ``null_condition`` writes the cross-attention LITERALLY as muse_net:158-166 (masked_fill with -finfo.max, softmax over
                          all K + 1 keys) - not the constant-row shortcut the library takes; ``shortcut=True`` is that shortcut, for the identity test
  muse_forward_null       = muse_forward(null_condition=True)
  maskgit_generate_guided the loop of restate.maskgit_generate with the guided logits (the token critic reads the CONDITIONAL embed, muse_net:272, 394-396)
  pick_margins            per pick of a trace: (top-1 - top-2) of filtered / temperature + gumbel over the largest finite magnitude of the row
"""
from __future__ import annotations

import functools
from typing import Dict, List, Mapping, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import cases, restate as R

Tensor = torch.Tensor


def cast_sd(sd: Mapping[str, Tensor], dtype) -> Dict[str, Tensor]:
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _camera_embeddings(sd, prefix, cfg, I_inv, E_inv):
    """restate.camera_embeddings with the pixel plane in the dtype of the matrices (the fp32 plane holds small integers times a linspace value: its cast is exact)."""
    Wimg = sd[prefix + "img_embed.weight"].reshape(-1, 4)
    Wcam = sd[prefix + "cam_embed.weight"].reshape(-1, 4)
    c_embed = E_inv[..., 3] @ Wcam.t()
    cam = I_inv @ R.image_plane(cfg).to(I_inv.dtype)
    cam = torch.cat([cam, torch.ones_like(cam[..., :1, :])], dim=-2)
    d_embed = torch.einsum("od,bcdt->bcto", Wimg, E_inv @ cam)
    img = d_embed - c_embed[:, :, None, :]
    return img / (img.norm(dim=-1, keepdim=True) + 1e-7), c_embed


def _inputs(sd, cfg, ids, cond_ids, I_inv, E_inv, prefix):
    """x0 [B, N, D], context [B, K, D], bias [L, L] or None of TransformerMultiView.forward (muse_net:309-348) in the dtype of ``sd``."""
    C, T = cfg.num_cams, cfg.num_cam_tokens
    B = ids.shape[0] // C
    x = sd[prefix + "token_emb.weight"][ids.reshape(B, C * T)]
    c_embed = None
    if cfg.image_embed:
        img, c_embed = _camera_embeddings(sd, prefix, cfg, I_inv, E_inv)
        x = x + img.reshape(B, C * T, -1)
    x = x + sd[prefix + "pos_emb.weight"][None, : C * T]
    context = sd[prefix + "cond_token_emb.weight"][cond_ids]
    if cfg.bev_embed:
        context = context + R.bev_embedding(sd, prefix, cfg, c_embed)
    context = context + sd[prefix + "cond_pos_emb.weight"][None]
    return x, context


def masked_cross_attention(sd, p: str, x: Tensor, context: Tensor, bias: Optional[Tensor], heads: int, K: int, context_mask: Tensor, scale: float = 8.0) -> Tensor:
    """Attention.forward (muse_net:117-169) of a cross-attention module with ``context_mask`` [B, K] bool, as the reference writes it."""
    B, N, _ = x.shape
    xn = R._ln_gamma(x, sd[p + "norm.gamma"])
    q = F.linear(xn, sd[p + "to_q.weight"]) * scale
    k, v = F.linear(context, sd[p + "to_kv.weight"]).chunk(2, dim=-1)
    split = lambda t: t.reshape(t.shape[0], t.shape[1], heads, -1).permute(0, 2, 1, 3)
    q, k, v = split(q), split(k), split(v)
    nk, nv = sd[p + "null_kv"]
    k = torch.cat([nk[None].expand(B, -1, -1, -1), k], dim=2)
    v = torch.cat([nv[None].expand(B, -1, -1, -1), v], dim=2)
    q = F.normalize(q, dim=-1) * sd[p + "q_scale"]
    k = F.normalize(k, dim=-1) * sd[p + "k_scale"]
    sim = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    if bias is not None:
        sim = sim + F.pad(bias[K:, :K], (1, 0), value=0.0)
    mask = F.pad(context_mask[:, None, None, :], (1, 0), value=True)          # muse_net:159-160
    sim = sim.masked_fill(~mask, -torch.finfo(sim.dtype).max)                 # muse_net:162-163
    out = torch.einsum("bhij,bhjd->bhid", sim.softmax(dim=-1), v)
    return F.linear(out.permute(0, 2, 1, 3).reshape(B, N, -1), sd[p + "to_out.weight"])


def null_row(sd, p: str) -> Tensor:
    """What the cross-attention module ``p`` returns for every row when no context token is visible: to_out(vec(null_v)) [D]."""
    return F.linear(sd[p + "null_kv"][1].reshape(-1), sd[p + "to_out.weight"])


def muse_forward(sd, cfg, ids: Tensor, cond_ids: Tensor, I_inv: Tensor, E_inv: Tensor, *, depth: int, heads: int, null_condition: bool = False, shortcut: bool = False,
                 dtype=torch.float64, prefix: str = "transformer.") -> Tuple[Tensor, Tensor]:
    """restate.muse_forward evaluated in ``dtype`` -> (logits [(B C), T, V], embed [(B C), T, D]); ``null_condition``: context_mask all False."""
    bias = R.attention_bias(sd, prefix, cfg).to(dtype) if cfg.camera_bias else None   # (formed in fp32 like the reference, muse_net:343-348)
    sd = cast_sd(sd, dtype)
    C, T, K = cfg.num_cams, cfg.num_cam_tokens, cfg.num_cond_tokens
    B = ids.shape[0] // C
    x, context = _inputs(sd, cfg, ids, cond_ids, I_inv.to(dtype), E_inv.to(dtype), prefix)
    none = torch.zeros((B, K), dtype=torch.bool)
    for i in range(depth):
        lp = f"{prefix}transformer_blocks.layers.{i}."
        x = R.muse_attention(sd, lp + "0.", x, None, bias, heads, K) + x
        if not null_condition:
            x = R.muse_attention(sd, lp + "1.", x, context, bias, heads, K) + x
        elif shortcut:
            x = x + null_row(sd, lp + "1.")
        else:
            x = masked_cross_attention(sd, lp + "1.", x, context, bias, heads, K, none) + x
        x = R.muse_feedforward(sd, lp + "2.", x) + x
    embed = R._ln_gamma(x, sd[prefix + "transformer_blocks.norm.gamma"])
    logits = F.linear(embed, sd[prefix + "to_logits.weight"])
    return logits.reshape(B * C, T, -1), embed.reshape(B * C, T, -1)


def muse_forward_null(sd, cfg, ids, cond_ids, I_inv, E_inv, *, depth: int, heads: int, **kw):
    return muse_forward(sd, cfg, ids, cond_ids, I_inv, E_inv, depth=depth, heads=heads, null_condition=True, **kw)


def maskgit_generate_guided(sd, cfg, cond_ids: Tensor, I_inv: Tensor, E_inv: Tensor, *, depth: int, heads: int, cond_scale: float, timesteps: int = 18,
                            temperature: float = 1.0, topk_filter_thres: float = 0.9, critic_noise_scale: float = 1.0, noise: Optional[Mapping[str, Tensor]] = None,
                            init_ids: Optional[Tensor] = None, use_token_critic: bool = True, can_remask_prev_masked: bool = False,
                            trace: Optional[List[Dict[str, Tensor]]] = None, dtype=torch.float64) -> Tensor:
    """restate.maskgit_generate with logits = null + (cond - null) * cond_scale wherever the loop uses logits (muse_net:587-619); cond_scale == 1: the conditional
    logits alone (muse_net:269-270).  ``trace`` receives per iteration {'ids', 'logits', 'cond', 'null', 'picked' (is_mask), 'y' (= filtered / temp + gumbel), 'scores', 'temp', 'pred' (the arg-max at every position)}."""
    C, T = cfg.num_cams, cfg.num_cam_tokens
    B = cond_ids.shape[0]
    mask_id = cfg.vocab_size
    ids = torch.full((B * C, T), mask_id, dtype=torch.long)
    scores = torch.zeros((B * C, T), dtype=dtype)
    init_mask = None if init_ids is None else (init_ids != mask_id)
    fwd = lambda x, null: muse_forward(sd, cfg, x, cond_ids, I_inv, E_inv, depth=depth, heads=heads, null_condition=null, dtype=dtype)
    wc, bc = sd.get("token_critic.to_pred.weight"), sd.get("token_critic.to_pred.bias")
    for step, n_mask in enumerate(R.mask_schedule(timesteps, T)):
        frac = (timesteps - 1 - step) / timesteps
        ids = ids.scatter(1, scores.topk(n_mask, dim=-1).indices, mask_id)
        if init_ids is not None:
            ids[init_mask] = init_ids[init_mask]
        cond, _ = fwd(ids, False)
        null = None
        logits = cond
        if cond_scale != 1:
            null, _ = fwd(ids, True)
            logits = null + (cond - null) * cond_scale
        filtered = R.topk_filter(logits, topk_filter_thres)
        g = torch.zeros_like(filtered) if noise is None else R.gumbel_from_uniform(noise["gumbel_u"][step]).to(dtype)
        y = filtered / max(temperature * frac, 1e-10) + g
        pred = y.argmax(dim=-1)
        is_mask = ids == mask_id
        ids = torch.where(is_mask, pred, ids)
        if use_token_critic:
            _, embed = fwd(ids, False)
            crit = F.linear(embed, wc.to(dtype), bc.to(dtype))[..., 0]
            u = torch.full_like(crit, 0.5) if noise is None else noise["critic_u"][step].to(dtype)
            scores = crit + (u - 0.5) * critic_noise_scale * frac
        else:
            scores = 1 - logits.softmax(dim=-1).gather(2, pred[..., None])[..., 0]
            if not can_remask_prev_masked:
                scores = scores.masked_fill(~is_mask, -1e5)
        if trace is not None:
            trace.append({"ids": ids.clone(), "logits": logits, "cond": cond, "null": null, "picked": is_mask, "y": y, "scores": scores.clone(), "temp": temperature * frac, "pred": pred})
    return ids.reshape(B * C, cfg.cam_latent_h, cfg.cam_latent_w)


def row_margins(y: Tensor) -> Tensor:
    """(top-1 - top-2) of every row of y over the largest finite |y| of the row."""
    top = y.topk(2, dim=-1).values
    big = torch.where(torch.isfinite(y), y.abs(), torch.zeros_like(y)).amax(dim=-1)
    return (top[..., 0] - top[..., 1]) / big


def pick_margins(trace: List[Dict[str, Tensor]]) -> Tensor:
    """One relative margin per pick (masked position of an iteration): (top-1 - top-2) of y = filtered / temperature + gumbel over the largest finite |y| of the row."""
    out = []
    for t in trace:
        y = t["y"][t["picked"]]
        top = y.topk(2, dim=-1).values
        big = torch.where(torch.isfinite(y), y.abs(), torch.zeros_like(y)).amax(dim=-1)
        out.append((top[:, 0] - top[:, 1]) / big)
    return torch.cat(out)


# ================================================================================================ the cases the guidance tests share
SCALE = 3.0
TIMESTEPS = 6
MARGIN = 1e-4
D_CASES = ["m_tiny_rays", "m_fold", "m_tiny_6cam"]   # condition (d) of tests/test_cfg_ref_cpu.py
D_NOISES = ["greedy", "seed5"]
# Without the token critic the scores that choose what the next iteration re-masks are 1 - softmax(logits)[pred] (muse_net:613-619).  Guided logits are peaked (three times
# the distance of two forwards): p[pred] lies within a few fp32 ulps of 1, the fp32 scores collapse onto multiples of 2^-24, many of them equal, and which of them topk
# takes is decided by rounding and by the tie order of the implementation.  On such a run the restatement's own fp32 evaluation does not return its fp64 ids, and no fp32
# implementation can be held to them as a free run.  The cases WITHOUT the critic on which fp32 and fp64 agree (with the critic all of D_CASES do); pinned, and asserted in
# both directions by tests/test_cfg_ref_cpu.py:
FP32_AGREES_WITHOUT_CRITIC = ("m_fold",)


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def fixture(name):
    case = cases.CASES[name]
    cfg = case.make_cfg()
    sd = cases.case_state_dict(case, cfg)
    return case, cfg, sd, cases.inputs(case, cfg)


def noise_of(case, cfg, tag):
    return None if tag == "greedy" else cases.maskgit_noise(case, cfg, seed=5)


def random_ids(case, cfg):
    g = torch.Generator().manual_seed(case.input_seed)
    return torch.randint(0, cfg.vocab_size + 1, (case.batch * cfg.num_cams, cfg.num_cam_tokens), generator=g)


@functools.lru_cache(maxsize=None)
def guided_run(name, tag, critic, scale=SCALE, dtype=torch.float64, remask=False):
    """(ids, trace) of the restatement on a shared case (scale 3, 6 timesteps, topk_filter_thres 0.9 unless said otherwise), computed once per process."""
    case, cfg, sd, bt = fixture(name)
    trace = []
    ids = maskgit_generate_guided(sd, cfg, bt["cond_ids"], bt["intrinsics_inv"], bt["extrinsics_inv"], depth=cfg.num_layers, heads=cfg.num_heads, cond_scale=scale,
                                  timesteps=TIMESTEPS, topk_filter_thres=0.9, noise=noise_of(case, cfg, tag), use_token_critic=critic, can_remask_prev_masked=remask,
                                  trace=trace, dtype=dtype)
    return ids, trace


def fp32_agrees(name, tag, critic, remask=False):
    """The restatement evaluated in fp32 - the arithmetic the reference itself runs in - returns the fp64 ids."""
    return torch.equal(guided_run(name, tag, critic, remask=remask)[0], guided_run(name, tag, critic, dtype=torch.float32, remask=remask)[0])
