"""Drop-in for multi_view_generation/modules/stage2/muse_maskgit_pytorch.py (Route M, MaskGit bidirectional decoder).

Same class names, constructor kwargs, method signatures and ``state_dict`` keys as the reference:
  MaskGitTransformerMultiView   muse_net:204-261, 418-421     (``_target_`` at configs/experiment/muse_stage_two_multi_view.yaml:31)
  SelfCritic                    muse_net:388-396
  MaskGit                       muse_net:467-627              (``_target_`` at muse_stage_two_multi_view.yaml:26)
The modules hold parameters only; ``forward`` / ``generate`` run inside libbevgen_hip (bevgen_muse_forward,
bevgen_maskgit_generate, bevgen_maskgit_loss).  Inference and validation losses only: no gradients (the surveyed branch has no training, README.md:20).
"""
from __future__ import annotations

import math
from typing import Callable, Iterable, Optional

import torch
import torch.nn as nn

from ... import tables
from ... import weights as W
from ...runtime import Context
from ..options import RuntimeOptionsMixin, pop_runtime_options
from ..params import ParamNode, build_tree, module_device


def cosine_schedule(t):
    return torch.cos(t * math.pi * 0.5)


class TransformerMultiView(nn.Module):
    def __init__(self, *, num_tokens, dim, seq_len, dim_out=None, self_cond=False, add_mask_id=False, cfg=None, depth=None, dim_head=64, heads=8, ff_mult=4, **kwargs):
        super().__init__()
        self.runtime_kwargs = pop_runtime_options(kwargs)   # precision / weights next to this module's `_target_` (muse_net:223 takes **kwargs): read by MaskGit
        if cfg is None:
            raise ValueError("cfg (GPTConfig) is required")
        if self_cond:
            raise NotImplementedError("self conditioning is never enabled by the shipped configs (muse_net:240)")
        if dim_head != 64:
            raise ValueError("libbevgen_hip attention kernels are specialised for dim_head = 64")
        self.cfg = cfg
        self.dim = dim
        self.seq_len = seq_len[0] * seq_len[1] if isinstance(seq_len, Iterable) else seq_len
        self.num_tokens = num_tokens
        self.mask_id = num_tokens if add_mask_id else None
        self.dim_out = dim_out if dim_out is not None else num_tokens
        self.self_cond = False
        self.depth, self.heads, self.dim_head, self.ff_mult = depth, heads, dim_head, ff_mult
        if dim != cfg.num_embed or heads != cfg.num_heads or depth != cfg.num_layers:
            raise ValueError("dim / heads / depth must equal cfg.num_embed / num_heads / num_layers (they are interpolated from cfg in the reference YAML)")
        shapes = W.muse_transformer_shapes(cfg, depth=depth, heads=heads, dim_head=dim_head, ff_mult=ff_mult, num_tokens=num_tokens)
        build_tree(self, shapes)
        if cfg.bev_embed:
            self.bev_grid.copy_(tables.get_bev_grid(cfg))
        self._reset_parameters()

    def _reset_parameters(self):
        # reference defaults: gamma = 1, q/k scale = 1, null_kv ~ randn, Linear/Embedding default inits, zeros for the bias tables
        for name, p in self.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if leaf in ("gamma", "q_scale", "k_scale"):
                p.data.fill_(1.0)
            elif leaf == "null_kv":
                p.data.normal_()
            elif leaf in ("bev_cam_pos_emb", "camera_bias_emb") or leaf == "bias":
                p.data.zero_()
            elif "emb.weight" in name:
                p.data.normal_()
            elif p.dim() >= 2:
                fan_in = p[0].numel()
                p.data.uniform_(-1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))


class MaskGitTransformerMultiView(TransformerMultiView):
    def __init__(self, *args, **kwargs):
        assert "add_mask_id" not in kwargs
        super().__init__(*args, add_mask_id=True, **kwargs)


class SelfCritic(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net
        self.to_pred = ParamNode()
        self.to_pred.register_parameter("weight", nn.Parameter(torch.zeros(1, net.dim), requires_grad=False))
        self.to_pred.register_parameter("bias", nn.Parameter(torch.zeros(1), requires_grad=False))
        nn.init.uniform_(self.to_pred.weight, -1 / math.sqrt(net.dim), 1 / math.sqrt(net.dim))


class MaskGit(RuntimeOptionsMixin, nn.Module):
    def __init__(self, image_size, transformer: MaskGitTransformerMultiView, noise_schedule: Callable = cosine_schedule, token_critic=None,
                 self_token_critic=False, cond_image_size=None, cond_drop_prob=0.5, self_cond_prob=0.9, no_mask_token_prob=0.0, critic_loss_weight=1.0,
                 precision=None, weights=None, guidance=None):
        """muse_net:467-509 + the library's modes (``precision`` / ``weights``; bevgen_amd/modules/options.py): explicit here > given to the transformer >
        $BEVGEN_PRECISION / $BEVGEN_WEIGHTS > f16x3 / f32.  ``guidance``: None / 'off' = ``generate`` ignores ``cond_scale`` like the reference's eval mode does in
        effect; 'null' = classifier-free guidance with a real null-condition forward (``generate``'s own keyword overrides this)."""
        super().__init__()
        self.guidance = self._check_guidance(guidance)
        self._ctx: Optional[Context] = None
        opts = dict(getattr(transformer, "runtime_kwargs", {}))
        opts.update({k: v for k, v in (("precision", precision), ("weights", weights)) if v is not None})
        self._init_runtime_options(opts)
        self.image_size = image_size[0] * image_size[1] if isinstance(image_size, Iterable) else image_size
        self.cond_image_size = cond_image_size
        self.cond_drop_prob = cond_drop_prob
        self.transformer = transformer
        self.self_cond = transformer.self_cond
        self.mask_id = transformer.mask_id
        self.noise_schedule = noise_schedule
        assert not (self_token_critic and token_critic is not None)
        self.token_critic = SelfCritic(transformer) if self_token_critic else token_critic
        if self.token_critic is not None and not isinstance(self.token_critic, SelfCritic):
            raise NotImplementedError("a separate TokenCritic network is not implemented: the shipped configuration uses self_token_critic (or none: confidence scores)")
        self.critic_loss_weight = critic_loss_weight
        self.self_cond_prob = self_cond_prob
        self.no_mask_token_prob = no_mask_token_prob

    @staticmethod
    def _check_guidance(guidance):
        if guidance not in (None, "off", "null"):
            raise ValueError(f"guidance must be None, 'off' or 'null', got {guidance!r}")
        return guidance

    # ---------------------------------------------------------------------------------- device context
    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self.invalidate()
        return out

    def invalidate(self):
        """Drop the device copy of the weights (call after modifying parameters in place)."""
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def context(self) -> Context:
        if self._ctx is None:
            dev = module_device(self)
            if dev.type != "cuda":
                raise RuntimeError("MaskGit must be moved to a ROCm device (model.to('cuda')) before sampling; libbevgen_hip has no CPU path")
            cfg = self.transformer.cfg
            ctx = Context(cfg, route="maskgit", device=dev.index if dev.index is not None else torch.cuda.current_device(), **self.runtime_options("maskgit"))
            sd = self.state_dict()
            ctx.load_state_dict({k: v for k, v in sd.items() if not k.startswith("token_critic.net.")})
            ctx.set_tables(cfg)
            ctx.finalize()
            self._ctx = ctx
        return self._ctx

    # ---------------------------------------------------------------------------------- reference API
    @torch.no_grad()
    def generate(self, init_ids: Optional[torch.Tensor] = None, cond_images: Optional[torch.Tensor] = None, fmap_size=None, temperature=1.0,
                 topk_filter_thres=0.9, can_remask_prev_masked=False, force_not_use_token_critic=False, timesteps=12, cond_scale=3,
                 critic_noise_scale=1, batch=None, noise=None, samples_per_layout=1, guidance=None):
        """muse_net:511-627.  ``guidance`` (None = the constructor's): 'null' honours ``cond_scale`` - every iteration also runs the forward with all layout tokens masked
        out of the cross-attention and samples from null + (cond - null) * cond_scale; None / 'off' ignores ``cond_scale`` (the reference passes 3 everywhere, where its
        eval-mode null forward equals the conditional one: muse_net:352).  ``noise``: None -> stochastic like the reference (uniforms drawn in the sampler kernels, seeded from torch's generator);
        an int -> that seed; 'greedy' -> gumbel noise 0 / critic uniform 0.5; or {'gumbel_u','critic_u'} explicit uniforms."""
        use_token_critic = self.token_critic is not None and not force_not_use_token_critic   # muse_net:553
        if not use_token_critic and can_remask_prev_masked:
            assert self.no_mask_token_prob > 0., 'without training with some of the non-masked tokens forced to predict, not sure if the logits will be meaningful for these token'   # muse_net:621
        cfg = self.transformer.cfg
        ctx = self.context()
        guidance = self.guidance if guidance is None else self._check_guidance(guidance)
        if fmap_size is not None and tuple(fmap_size) != (cfg.cam_latent_h, cfg.cam_latent_w):
            raise ValueError(f"fmap_size {tuple(fmap_size)} != cam_latent_res {(cfg.cam_latent_h, cfg.cam_latent_w)}")
        B = len(cond_images)
        rows, T, V = B * cfg.num_cams, cfg.num_cam_tokens, cfg.vocab_size
        gu = cu = None
        seed = 0
        if noise is None:
            # stochastic like the reference: the uniforms are drawn inside the sampler kernels (Philox keyed by a seed taken from torch's CPU generator, so
            # torch.manual_seed / pl.seed_everything make a run reproducible); nothing of size [timesteps, rows, T, V] is ever materialised
            seed = int(torch.randint(1, 2 ** 62, (), dtype=torch.int64).item())
        elif isinstance(noise, int):
            seed = noise
        elif isinstance(noise, str) and noise == "greedy":
            pass
        else:
            gu, cu = noise["gumbel_u"], noise["critic_u"]
        return ctx.maskgit_generate(cond_images, batch["intrinsics_inv"], batch["extrinsics_inv"], timesteps=timesteps, temperature=temperature,
                                    topk_filter_thres=topk_filter_thres, critic_noise_scale=critic_noise_scale, gumbel_u=gu, critic_u=cu, init_ids=init_ids,
                                    noise_seed=seed, use_token_critic=use_token_critic, can_remask_prev_masked=can_remask_prev_masked, samples_per_layout=samples_per_layout,
                                    cond_scale=float(cond_scale) if guidance == "null" else None)

    @torch.no_grad()
    def transformer_forward(self, x, conditioning_token_ids, batch, return_embed=False, null_condition=False):
        """TransformerMultiView.forward in eval mode (muse_net:283-371): x [(B*C),T] -> logits [(B*C),T,V] (and embed).  null_condition: with every layout token masked
        out of the cross-attention (what cond_drop_prob = 1 gives in training mode)."""
        logits, embed = self.context().muse_forward(x, conditioning_token_ids, batch["intrinsics_inv"], batch["extrinsics_inv"], null_condition=null_condition)
        return (logits, embed) if return_embed else logits

    PHILOX_HOST_STREAM = 3   # noise=int: the mask times (elements 0 .. rows-1) and the temperature (element rows) come from this Philox stream at iteration 0

    def _forward_refusals(self, ignore_index, cond_images, cond_token_ids, cond_drop_prob, weights):
        """What MaskGit.forward cannot evaluate, refused before anything touches the device."""
        V = self.transformer.num_tokens
        if weights is not None:
            raise NotImplementedError("weights (muse_net:375-377: the bounding-box weighting of the cross-entropy, training only) is not implemented; refusing rather than ignoring it")
        if self.no_mask_token_prob > 0.:
            raise NotImplementedError("no_mask_token_prob > 0 (muse_net:671-673: part of the masked tokens keep their id) is set by no shipped configuration and is not implemented")
        assert not (cond_images is not None and cond_token_ids is not None), 'if conditioning on low resolution, cannot pass in both images and token ids'   # muse_net:654
        if 0 <= int(ignore_index) <= V:
            raise ValueError(f"ignore_index = {ignore_index} is a token id of this model (0 .. {V}, the mask id included): labels = where(mask, ids, ignore_index) "
                             "(muse_net:669) would drop real tokens from the cross-entropy")
        drop = self.cond_drop_prob if cond_drop_prob is None else cond_drop_prob
        if self.transformer.training and drop > 0:
            raise NotImplementedError(f"the transformer is in training mode with cond_drop_prob = {drop} (muse_net:310-313 would drop conditions at random): this library "
                                      "evaluates the eval-mode arithmetic only; call .eval() first (Lightning's validate loop does)")

    @torch.no_grad()
    def forward(self, images_or_ids: torch.Tensor, ignore_index=-1, cond_images: Optional[torch.Tensor] = None, cond_token_ids: Optional[torch.Tensor] = None,
                cond_drop_prob=None, train_only_generator=False, sample_temperature=None, batch=None, weights=None, noise=None):
        """muse_net:629-729 in eval mode, on the device (bevgen_maskgit_loss): the masked-token cross-entropy and, with a token critic, the critic's BCE ->
        (ce + critic_loss_weight * bce, ce, bce), or ce alone without a critic / with train_only_generator, as 0-dim device tensors.  ``noise``: None -> the reference's
        own sources (mask times from torch's CPU generator, a Philox seed for the permutation and the gumbel noise from it as in ``generate``, the temperature from
        Python's ``random()``: ``seed_everything`` reproduces a run); an int -> everything from that Philox seed; or explicit {'time_u' [rows], 'perm_u' [rows, T],
        'gumbel_u' [rows, T, V], 'temperature'}.  Equal uniforms within a perm_u row rank by index."""
        import random

        self._forward_refusals(ignore_index, cond_images, cond_token_ids, cond_drop_prob, weights)
        cond = cond_images if cond_images is not None else cond_token_ids
        if cond is None or batch is None:
            raise ValueError("MaskGit.forward needs the condition token ids (cond_images) and the batch with intrinsics_inv / extrinsics_inv")
        ids = images_or_ids.reshape(images_or_ids.shape[0], -1)   # 'b ... -> b (...)', muse_net:648
        rows, T = ids.shape
        with_critic = self.token_critic is not None and not train_only_generator   # muse_net:708
        ctx = self.context()
        perm_u = gumbel_u = None
        seed = 0
        if noise is None:
            time_u = torch.zeros(rows).float().uniform_(0, 1)   # muse_net:430-431, 660
            seed = int(torch.randint(1, 2 ** 62, (), dtype=torch.int64).item())
            temperature = sample_temperature if sample_temperature is not None else random.random()   # muse_net:713
        elif isinstance(noise, int):
            seed = noise
            host = ctx.philox_uniform(seed, 0, self.PHILOX_HOST_STREAM, rows + 1).cpu()
            time_u = host[:rows]
            temperature = sample_temperature if sample_temperature is not None else float(host[rows])
        else:
            time_u, perm_u, gumbel_u = noise["time_u"], noise["perm_u"], noise.get("gumbel_u")
            temperature = noise["temperature"] if noise.get("temperature") is not None else sample_temperature
            if with_critic and (gumbel_u is None or temperature is None):
                raise ValueError("explicit noise needs 'gumbel_u' and a temperature for the critic loss")
        # the masked count per row with the reference's own fp32 CPU operations (muse_net:661-662): no device cos can move a count by one
        time_u = torch.as_tensor(time_u, dtype=torch.float32).cpu().reshape(rows)
        num_masked = (T * self.noise_schedule(time_u)).round().clamp(min=1)
        out = ctx.maskgit_loss(ids, cond, batch["intrinsics_inv"], batch["extrinsics_inv"], num_masked.to(torch.int64), perm_u=perm_u, gumbel_u=gumbel_u,
                               temperature=0.0 if temperature is None else float(temperature), noise_seed=seed, with_critic=with_critic,
                               critic_loss_weight=float(self.critic_loss_weight))
        return (out[0], out[1], out[2]) if with_critic else out[1]
