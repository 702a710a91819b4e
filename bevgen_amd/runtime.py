"""Thin Python host over the C ABI: one ``Context`` per (device, model).

PyTorch is used for device memory, streams and (later) ``torch.distributed`` only: every tensor handed to the library is a
raw ``data_ptr()``; all arithmetic of the hot path happens inside libbevgen_hip's HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
import math
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib, tables
from ._lib import bevgen_cfg
from .weights import ff_inner_dim

# Route A projection-weight storage of the decode step: the `decode_weights` choice -> bevgen_cfg.decode_weight_dtype (BEVGEN_W_*)
DECODE_WEIGHTS = {"f32": _lib.W_F32, "f16": _lib.W_F16, "i8": _lib.W_I8}


def decode_weight_dtype(route: str, weights: str, decode_weights: str) -> int:
    """bevgen_cfg.decode_weight_dtype of a Context, or ValueError: an unknown choice, or Route A with weights='f16' and decode_weights='i8' (the library refuses the
    pair at bevgen_finalize as well)."""
    if decode_weights not in DECODE_WEIGHTS:
        raise ValueError(f"decode_weights must be one of {tuple(DECODE_WEIGHTS)}, got {decode_weights!r}")
    if route == "ar" and weights == "f16" and decode_weights == "i8":
        raise ValueError("weights='f16' cannot be combined with decode_weights='i8': the dequantised int8 matrices are not fp16-representable, "
                         "so prefill and decode could not run one model")
    return DECODE_WEIGHTS[decode_weights]


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _req(t: torch.Tensor, dtype, device, name: str) -> torch.Tensor:
    if t.dtype != dtype:
        t = t.to(dtype)
    if t.device != device:
        t = t.to(device)
    return t.contiguous()


def mask_schedule(timesteps: int, seq_len: int):
    """Host logic of MaskGit.generate (muse_net:564-567), evaluated with torch fp32 exactly like the reference:
    n_t = max(int(cos(t*pi/2) * T), 1) for t in linspace(0,1,timesteps)."""
    out = []
    for t in torch.linspace(0, 1, timesteps):
        out.append(max(int((torch.cos(t * math.pi * 0.5) * seq_len).item()), 1))
    return out


def topk_count(thres: float, vocab: int) -> int:
    """muse_net:454: k = ceil((1 - thres) * V)."""
    return math.ceil((1 - thres) * vocab)


class Context:
    """Owns a ``bevgen_ctx`` (weights, KV cache, workspace live on the device inside it)."""

    def __init__(self, cfg=None, *, route: str = "maskgit", vq_ddconfig: Optional[Mapping] = None, vq_n_embed: int = 0, vq_embed_dim: int = 0,
                 device: Optional[int] = None, max_batch: int = 0, precision: Optional[str] = None, kv_cache: Optional[str] = None, decode_path: Optional[str] = None, decode_weights: Optional[str] = None,
                 weights: Optional[str] = None, decode_chains: Optional[int] = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("bevgen_amd needs a ROCm GPU (MI355X / gfx950); there is no CPU path in the product")
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.cfg = cfg
        c = bevgen_cfg()
        c.abi_version = _lib.ABI_VERSION
        c.route = _lib.ROUTE_MASKGIT if route == "maskgit" else _lib.ROUTE_AR
        # every mode: explicit argument, else its environment variable, else this low-level class's default (exact fp32 everywhere; the drop-in modules
        # resolve their own defaults - f16x3 products - in bevgen_amd/modules/options.py and always pass explicit values)
        precision = precision or os.environ.get("BEVGEN_PRECISION") or "fp32"
        kv_cache = kv_cache or os.environ.get("BEVGEN_KV_CACHE") or "f32"
        decode_path = decode_path or os.environ.get("BEVGEN_DECODE_PATH") or "auto"
        decode_weights = decode_weights or os.environ.get("BEVGEN_DECODE_WEIGHTS") or "f32"
        for key, val, ok in (("kv_cache", kv_cache, ("f32", "f16", "i8")), ("decode_path", decode_path, ("auto", "fused", "split", "per_op")),
                             ("decode_weights", decode_weights, tuple(DECODE_WEIGHTS))):
            if val not in ok:
                raise ValueError(f"{key} must be one of {ok}, got {val!r}")
        if precision not in ("fp32", "f16x3", "f16x3r", "f16x1"):
            raise ValueError(f"precision must be 'fp32', 'f16x3', 'f16x3r' or 'f16x1', got {precision!r}")
        self.precision = precision
        # 'f16x3r' ("range-safe") = f16x3 whose VQGAN decoder and encoder rescale their un-normalised activations by a per-tensor power of two instead of refusing a
        # checkpoint whose residual stream leaves the f16 range (bevgen_cfg.vq_range); the transformer routes behave exactly as under 'f16x3'
        # 'f16x1' ("single product") = f16x3 whose Route M projections compute f16(A) f16(W)^T, one MFMA per product, on matrices rounded to f16 at finalize whatever
        # `weights` says (BEVGEN_PRECISION_F16X1 in bevgen_hip.h); the VQGAN and Route A behave exactly as under 'f16x3'
        c.precision = {"fp32": _lib.PRECISION_FP32, "f16x3": _lib.PRECISION_F16X3, "f16x3r": _lib.PRECISION_F16X3, "f16x1": _lib.PRECISION_F16X1}[precision]
        c.vq_range = 1 if precision == "f16x3r" else 0
        c.max_batch = max_batch
        # Route A KV-cache storage: 'f32' (bit-exact tokens), 'f16' (fp16 storage / fp32 accumulate, BASELINE config 4: half the decode traffic) or 'i8' (opt-in, lossy:
        # int8 codes + one fp32 scale per (token, head) row, 68 bytes per row; BEVGEN_KV_I8 in bevgen_hip.h)
        c.kv_cache_dtype = {"f32": _lib.KV_F32, "f16": _lib.KV_F16, "i8": _lib.KV_I8}[kv_cache]
        self.kv_cache = kv_cache
        # Route A decode step: 'auto' (default: 'split' for one or two sequences per call, else 'fused'), 'fused' (three launches per layer), 'split' (LayerNorm + QKV projection kernel, then the attention-only kernel: four launches)
        # or 'per_op' (one kernel per operator, the A/B reference)
        c.decode_path = {"fused": _lib.DECODE_FUSED, "per_op": _lib.DECODE_PER_OP, "split": _lib.DECODE_SPLIT, "auto": _lib.DECODE_AUTO}[decode_path]
        self.decode_path = decode_path
        # Route A projection weights: 'f32', or 'f16' = the model with fp16-representable q/k/v, MLP and head weights (rounded at finalize), whose decode
        # step streams 2-byte weights, or 'i8' (opt-in, lossy) = the model whose projection weights are int8 codes x one fp32 scale per output row (quantised at
        # finalize; prefill, scoring and decode run that one model), whose decode step streams 1-byte weights
        # (bevgen_cfg.decode_weight_dtype is set below, once `weights` is known: decode_weight_dtype())
        self.decode_weights = decode_weights
        # Route A fused decode step: number of independent sequence groups enqueued on separate streams (0 = the library's choice; $BEVGEN_DECODE_CHAINS)
        c.decode_chains = int(os.environ.get("BEVGEN_DECODE_CHAINS", "0")) if decode_chains is None else int(decode_chains)
        # weights='f16' (or $BEVGEN_WEIGHTS): the GEMM / convolution matrices are rounded to f16 at finalize - two MFMAs per product instead of three
        weights = weights or os.environ.get("BEVGEN_WEIGHTS") or "f32"
        if weights not in ("f32", "f16"):
            raise ValueError(f"weights must be 'f32' or 'f16', got {weights!r}")
        c.decode_weight_dtype = decode_weight_dtype(route, weights, decode_weights)
        c.weight_dtype = {"f32": _lib.W_F32, "f16": _lib.W_F16}[weights]
        self.weights = weights
        if cfg is not None:
            c.num_layers, c.num_heads, c.dim = cfg.num_layers, cfg.num_heads, cfg.num_embed
            c.vocab_size, c.cond_vocab_size = cfg.vocab_size, cfg.cond_vocab_size
            c.num_cams, c.cam_latent_h, c.cam_latent_w = cfg.num_cams, cfg.cam_latent_h, cfg.cam_latent_w
            c.num_cond_tokens, c.seq_len, c.sparse_block_size = cfg.num_cond_tokens, cfg.gpt_block_size, cfg.sparse_block_size
            c.image_embed, c.bev_embed, c.camera_bias = int(cfg.image_embed), int(cfg.bev_embed), int(cfg.camera_bias)
            c.ff_inner = ff_inner_dim(cfg.num_embed) if route == "maskgit" else 0
        self.vq_ddconfig = dict(vq_ddconfig) if vq_ddconfig is not None else None
        if vq_ddconfig is not None:
            dd = vq_ddconfig
            mult = list(dd["ch_mult"])
            c.vq_ch, c.vq_num_res_blocks, c.vq_z_channels = dd["ch"], dd["num_res_blocks"], dd["z_channels"]
            c.vq_embed_dim, c.vq_n_embed, c.vq_resolution, c.vq_out_ch = vq_embed_dim, vq_n_embed, dd["resolution"], dd["out_ch"]
            c.vq_num_levels = len(mult)
            for i, m in enumerate(mult):
                c.vq_ch_mult[i] = m
            attn = list(dd["attn_resolutions"])
            c.vq_attn_resolution = attn[0] if attn else 0
            c.vq_in_channels = dd.get("in_channels", 0)
        self._c = c
        self.route = route
        h = C.c_void_p()
        code = self.lib.bevgen_create(C.byref(c), self.device_index, C.byref(h))
        if code != 0:
            raise _lib.BevgenError(code, (self.lib.bevgen_last_error(None) or b"").decode())
        self._h = h
        self._finalized = False

    # ------------------------------------------------------------------------------------------ lifecycle
    def close(self):
        """Destroys the context.  A status word nobody has read yet (asynchronous calls, no synchronize()) is reported here: an explicit close() raises after the
        context is gone; the garbage-collector path (__del__) leaves it to the library's message on stderr."""
        if getattr(self, "_h", None):
            pending = 0
            try:
                if torch.cuda.is_available():
                    torch.cuda.synchronize(self.device)
                    pending = self.status()
            except Exception:
                pending = 0
            self.lib.bevgen_destroy(self._h)
            self._h = None
            if pending:
                raise _lib.BevgenError(_lib.ERR_NUMERIC if pending & 124 else -4, f"context closed with device status word {pending} pending: results of its last calls were invalid "
                                       "(include/bevgen_hip.h BEVGEN_STATUS_*)")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.bevgen_destroy(self._h)   # (prints a pending status word to stderr)
                self._h = None
        except Exception:
            pass

    def _check(self, code):
        _lib.check(self._h, code)

    # ------------------------------------------------------------------------------------------ device status word
    def synchronize(self) -> None:
        """Wait for this context's stream and raise ``BevgenError`` (code ``ERR_NUMERIC`` / internal) if a kernel of the calls enqueued so far flagged a non-finite
        logit / pixel, an operand outside the f16 range of the chosen precision, or a failed fused-MLP launch (include/bevgen_hip.h "Device status word").  This is where
        the reference's per-step ``assert (~logits.isfinite()).sum() == 0`` (gpt:383,388, ar_lm:202) lands: once per call instead of once per token."""
        self._check(self.lib.bevgen_synchronize(self._h, self._s()))

    def status(self) -> int:
        """The raw status word as the host sees it now (no synchronisation, nothing cleared): ``_lib.STATUS_*`` bits."""
        w = C.c_uint(0)
        self._check(self.lib.bevgen_status(self._h, C.byref(w)))
        return int(w.value)

    def _done(self, check: bool) -> None:
        """End of a whole-call wrapper.  check=True (the default of every wrapper that hands results back): synchronise and surface the status word NOW, so a caller can
        never read tokens / pixels of a call that flagged itself.  check=False keeps the call asynchronous (pipelined callers, bench.py); the word is then reported by the next
        call on this context at the latest, or by an explicit ``synchronize()``."""
        if check:
            self.synchronize()

    def _s(self):
        """The current torch stream of THIS context's device (not of whatever device is current)."""
        return _stream(self.device)

    def load_tensor(self, name: str, t) -> None:
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        if a.dtype == np.float32:
            dt = _lib.DTYPE_F32
        elif a.dtype == np.float64:
            dt = _lib.DTYPE_F64
        elif a.dtype == np.int64:
            dt = _lib.DTYPE_I64
        elif a.dtype == np.uint8:
            dt = _lib.DTYPE_U8
        else:
            a = a.astype(np.float32)
            dt = _lib.DTYPE_F32
        a = np.ascontiguousarray(a)
        shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
        self._check(self.lib.bevgen_load_tensor(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), dt, a.ndim, shape))
        self._finalized = False

    def load_state_dict(self, sd: Mapping[str, torch.Tensor], prefix: str = "") -> None:
        """Upload every tensor of a reference-named state_dict under ``prefix`` (e.g. 'first_stage_model.')."""
        for k, v in sd.items():
            self.load_tensor(prefix + k, v)

    def set_tables(self, cfg=None) -> None:
        cfg = cfg or self.cfg
        self.load_tensor("table.forward_shuffle_idx", cfg.forward_shuffle_idx.to(torch.int64))
        self.load_tensor("table.attention_mask", cfg.attention_mask.to(torch.float32))
        self.load_tensor("table.layout", cfg.layout.to(torch.int64))
        if cfg.prob_matrix is not None:
            self.load_tensor("table.prob_matrix", cfg.prob_matrix.to(torch.float32))  # the reference casts the (float64, legacy) prior to the activation dtype
        if cfg.image_embed:
            self.load_tensor("table.image_plane", tables.image_plane(cfg).reshape(3, -1))

    def finalize(self) -> None:
        self._check(self.lib.bevgen_finalize(self._h))
        self._finalized = True

    # ------------------------------------------------------------------------------------------ Route M
    def muse_forward(self, ids, cond_ids, I_inv, E_inv, want_logits=True, want_embed=True, check=True, null_condition=False):
        """null_condition=True: the forward with every layout token masked out of the cross-attention (``bevgen_muse_forward_ex``), the null pass of classifier-free guidance."""
        cfg = self.cfg
        d = self.device
        ids = _req(ids, torch.int64, d, "ids")
        cond_ids = _req(cond_ids, torch.int64, d, "cond_ids")
        I_inv = _req(I_inv, torch.float32, d, "I_inv")
        E_inv = _req(E_inv, torch.float32, d, "E_inv")
        B = cond_ids.shape[0]
        rows = B * cfg.num_cams
        logits = torch.empty((rows, cfg.num_cam_tokens, cfg.vocab_size), dtype=torch.float32, device=d) if want_logits else None
        embed = torch.empty((rows, cfg.num_cam_tokens, cfg.num_embed), dtype=torch.float32, device=d) if want_embed else None
        if null_condition:
            self._check(self.lib.bevgen_muse_forward_ex(self._h, _ptr(ids), _ptr(cond_ids), _ptr(I_inv), _ptr(E_inv), B, _ptr(logits), _ptr(embed), 1, self._s()))
        else:
            self._check(self.lib.bevgen_muse_forward(self._h, _ptr(ids), _ptr(cond_ids), _ptr(I_inv), _ptr(E_inv), B, _ptr(logits), _ptr(embed), self._s()))
        self._done(check)
        return logits, embed

    def maskgit_generate(self, cond_ids, I_inv, E_inv, *, timesteps=18, temperature=1.0, topk_filter_thres=0.9, critic_noise_scale=1.0,
                         gumbel_u=None, critic_u=None, init_ids=None, noise_seed=0, use_token_critic=True, can_remask_prev_masked=False, samples_per_layout=1, check=True,
                         cond_scale=None):
        """cond_scale: None or 1 = no guidance (``bevgen_maskgit_generate_ex``); else classifier-free guidance with the null-condition pass
        (``bevgen_maskgit_generate_guided``): the logits of every iteration are null + (cond - null) * cond_scale.
        gumbel_u / critic_u: explicit uniforms (parity tests); else noise_seed != 0: the samplers draw them in registers (Philox); else deterministic.
        use_token_critic=False: scores = 1 - softmax(logits)[pred] (muse_net:611-622; no critic forwards), can_remask_prev_masked as the reference's flag.
        samples_per_layout S: consecutive groups of S scenes share their condition (cross-attention K / V built once per layout)."""
        cfg = self.cfg
        d = self.device
        cond_ids = _req(cond_ids, torch.int64, d, "cond_ids")
        I_inv = _req(I_inv, torch.float32, d, "I_inv")
        E_inv = _req(E_inv, torch.float32, d, "E_inv")
        B = cond_ids.shape[0]
        rows = B * cfg.num_cams
        T = cfg.num_cam_tokens
        sched = mask_schedule(timesteps, T)
        sched_c = (C.c_int32 * timesteps)(*sched)
        if gumbel_u is not None:
            gumbel_u = _req(gumbel_u, torch.float32, d, "gumbel_u")
            assert tuple(gumbel_u.shape) == (timesteps, rows, T, cfg.vocab_size), gumbel_u.shape
        if critic_u is not None:
            critic_u = _req(critic_u, torch.float32, d, "critic_u")
            assert tuple(critic_u.shape) == (timesteps, rows, T), critic_u.shape
        if init_ids is not None:
            init_ids = _req(init_ids, torch.int64, d, "init_ids").reshape(rows, T)
        out = torch.empty((rows, T), dtype=torch.int64, device=d)
        score_mode = 0 if use_token_critic else (2 if can_remask_prev_masked else 1)
        args = (self._h, _ptr(cond_ids), _ptr(I_inv), _ptr(E_inv), B, timesteps, sched_c, float(temperature), topk_count(topk_filter_thres, cfg.vocab_size),
                float(critic_noise_scale), _ptr(gumbel_u), _ptr(critic_u), _ptr(init_ids), _ptr(out), C.c_uint64(int(noise_seed) & 0xFFFFFFFFFFFFFFFF), score_mode,
                int(samples_per_layout))
        if cond_scale is None or float(cond_scale) == 1.0:
            self._check(self.lib.bevgen_maskgit_generate_ex(*args, self._s()))
        else:
            self._check(self.lib.bevgen_maskgit_generate_guided(*args, float(cond_scale), self._s()))
        self._done(check)
        return out.reshape(rows, cfg.cam_latent_h, cfg.cam_latent_w)

    def maskgit_loss(self, ids, cond_ids, I_inv, E_inv, num_masked, *, perm_u=None, gumbel_u=None, temperature=1.0, noise_seed=0, with_critic=True,
                     critic_loss_weight=1.0, return_aux=False, check=True):
        """MaskGit.forward in eval mode (``bevgen_maskgit_loss``): ids [(B C), T] ground-truth tokens, num_masked [(B C)] host integers in [1, T] (the reference's
        clamp(round(T cos(pi/2 t)), 1), evaluated by the caller).  perm_u [(B C), T] / gumbel_u [(B C), T, V]: explicit uniforms, else Philox streams 2 / 0 of noise_seed.
        Returns out [3] = (ce + critic_loss_weight * bce, ce, bce) - (ce, ce, 0) with with_critic=False - on the device; with return_aux also
        {'mask' bool, 'x', 'critic_input' (None without a critic)}, each [(B C), T]."""
        cfg = self.cfg
        d = self.device
        cond_ids = _req(cond_ids, torch.int64, d, "cond_ids")
        I_inv = _req(I_inv, torch.float32, d, "I_inv")
        E_inv = _req(E_inv, torch.float32, d, "E_inv")
        B = cond_ids.shape[0]
        rows, T, V = B * cfg.num_cams, cfg.num_cam_tokens, cfg.vocab_size
        ids = _req(ids, torch.int64, d, "ids").reshape(ids.shape[0], -1)
        if tuple(ids.shape) != (rows, T):
            raise ValueError(f"ids must be [{rows}, {T}] ((batch x cameras) rows of camera tokens), got {tuple(ids.shape)}")
        n = [int(v) for v in (num_masked.tolist() if hasattr(num_masked, "tolist") else num_masked)]
        if len(n) != rows or min(n) < 1 or max(n) > T:
            raise ValueError(f"num_masked must hold {rows} counts in [1, {T}], got {n}")
        if perm_u is not None:
            perm_u = _req(perm_u, torch.float32, d, "perm_u")
            if tuple(perm_u.shape) != (rows, T):
                raise ValueError(f"perm_u must be [{rows}, {T}], got {tuple(perm_u.shape)}")
        if gumbel_u is not None and with_critic:
            gumbel_u = _req(gumbel_u, torch.float32, d, "gumbel_u")
            if gumbel_u.numel() != rows * T * V:
                raise ValueError(f"gumbel_u must hold [{rows}, {T}, {V}] uniforms, got {tuple(gumbel_u.shape)}")
        else:
            gumbel_u = None
        seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
        if seed == 0 and (perm_u is None or (with_critic and gumbel_u is None)):
            raise ValueError("maskgit_loss: noise_seed = 0 without explicit uniforms (a mask needs randomness)")
        out = torch.empty((3,), dtype=torch.float32, device=d)
        mask = torch.empty((rows, T), dtype=torch.uint8, device=d) if return_aux else None
        x = torch.empty((rows, T), dtype=torch.int64, device=d) if return_aux else None
        ci = torch.empty((rows, T), dtype=torch.int64, device=d) if return_aux and with_critic else None
        self._check(self.lib.bevgen_maskgit_loss(self._h, _ptr(ids), _ptr(cond_ids), _ptr(I_inv), _ptr(E_inv), B, (C.c_int32 * rows)(*n), _ptr(perm_u), _ptr(gumbel_u),
                                                 float(temperature), C.c_uint64(seed), int(bool(with_critic)), float(critic_loss_weight), _ptr(out), _ptr(mask), _ptr(x),
                                                 _ptr(ci), self._s()))
        self._done(check)
        if return_aux:
            return out, {"mask": mask.bool(), "x": x, "critic_input": ci}
        return out

    def philox_uniform(self, seed, it, stream_id, n, V=0):
        """The uniforms maskgit_generate(noise_seed=seed) draws at iteration `it` (stream 0: gumbel [rows*V], 1: critic [rows]); of maskgit_loss: stream 2 = the
        mask permutation's [rows*T] at iteration 0 (stream 3 is MaskGit.forward's own: the mask times and the temperature of an integer seed)."""
        out = torch.empty((n,), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_philox_uniform(self._h, C.c_uint64(int(seed)), int(it), int(stream_id), int(V), int(n), _ptr(out), self._s()))
        return out

    # ------------------------------------------------------------------------------------------ Route A
    def sparse_self_attention(self, q, k, v, layout, attn_mask, add_mask, block):
        d = self.device
        q, k, v = (_req(t, torch.float32, d, "qkv") for t in (q, k, v))
        B, H, L, dh = q.shape
        assert dh == 64, "head dimension must be 64"
        layout = _req(layout, torch.int64, d, "layout")
        attn_mask = _req(attn_mask.reshape(L, L), torch.float32, d, "attn_mask")
        add = None if add_mask is None else _req(add_mask.reshape(L, L), torch.float32, d, "add_mask")
        out = torch.empty_like(q)
        self._check(self.lib.bevgen_sparse_self_attention(self._h, _ptr(q), _ptr(k), _ptr(v), _ptr(layout), _ptr(attn_mask), _ptr(add), B, H, L, int(block), _ptr(out), self._s()))
        return out

    def ar_prefill(self, cond_ids, I_inv, E_inv):
        d = self.device
        cond_ids = _req(cond_ids, torch.int64, d, "cond_ids")
        I_inv = _req(I_inv, torch.float32, d, "I_inv")
        E_inv = _req(E_inv, torch.float32, d, "E_inv")
        self._ar_B = cond_ids.shape[0]
        self._check(self.lib.bevgen_ar_prefill(self._h, _ptr(cond_ids), _ptr(I_inv), _ptr(E_inv), self._ar_B, self._s()))

    def ar_logits(self, check=False):
        """(step-level calls stay asynchronous by default: the status word surfaces at the next call or at synchronize())"""
        out = torch.empty((self._ar_B, self.cfg.vocab_size), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_ar_logits(self._h, _ptr(out), self._s()))
        self._done(check)
        return out

    def ar_decode_step(self, token):
        token = _req(token, torch.int64, self.device, "token")
        self._check(self.lib.bevgen_ar_decode_step(self._h, _ptr(token), self._s()))

    def ar_forward(self, cond_ids, I_inv, E_inv, ids, *, n_steps=None, target=None, weight=None, want_logits=True, check=True):
        """One-pass teacher-forced forward over the condition rows and the first ``n_steps`` image rows (``bevgen_ar_forward``).  ``ids`` / ``target`` / ``weight``
        are camera-major [B, N] as ``GPT.forward`` receives them; the results are in DECODE order: ``logits`` [B, n_steps, V] (None with ``want_logits=False``: they are
        then never materialised), and with a ``target`` ``nll`` [B, n_steps] and ``loss`` (0-d, sum(w * nll) / (B * n_steps)), else None.  Afterwards the context is as
        after ``ar_prefill`` + ``n_steps`` ``ar_decode_step`` calls.  Returns (logits, nll, loss)."""
        cfg = self.cfg
        d = self.device
        cond_ids = _req(cond_ids, torch.int64, d, "cond_ids")
        I_inv = _req(I_inv, torch.float32, d, "I_inv")
        E_inv = _req(E_inv, torch.float32, d, "E_inv")
        B, N = cond_ids.shape[0], cfg.num_img_tokens
        n = N if n_steps is None else int(n_steps)
        if not 1 <= n <= N:
            raise ValueError(f"n_steps={n} out of range [1, {N}]")
        ids = _req(ids, torch.int64, d, "ids").reshape(B, -1)
        if ids.shape[1] != N:
            raise ValueError(f"ids must hold {N} camera-major image tokens per sequence, got {ids.shape[1]}")
        if target is None and weight is not None:
            raise ValueError("weight needs a target")
        if target is not None:
            target = _req(target, torch.int64, d, "target").reshape(B, -1)
            if target.shape[1] != N:
                raise ValueError(f"target must hold {N} camera-major image tokens per sequence, got {target.shape[1]}")
        if weight is not None:
            weight = _req(weight, torch.float32, d, "weight").reshape(B, -1)
            if weight.shape[1] != N:
                raise ValueError(f"weight must hold {N} values per sequence, got {weight.shape[1]}")
        logits = torch.empty((B, n, cfg.vocab_size), dtype=torch.float32, device=d) if want_logits else None
        nll = torch.empty((B, n), dtype=torch.float32, device=d) if target is not None else None
        loss = torch.empty((), dtype=torch.float32, device=d) if target is not None else None
        self._ar_B = B
        self._check(self.lib.bevgen_ar_forward(self._h, _ptr(cond_ids), _ptr(I_inv), _ptr(E_inv), B, _ptr(ids), n, _ptr(logits), _ptr(target), _ptr(weight), _ptr(nll),
                                               _ptr(loss), self._s()))
        self._done(check)
        return logits, nll, loss

    def ar_sample(self, cond_ids, I_inv, E_inv, *, steps=None, top_k=None, temperature=1.0, greedy=True, noise_u=None, samples_per_layout=1, return_logits=False,
                  forced_ids=None, check=True):
        """Route A sampling with the KV cache.  forced_ids [steps, B] int64 in decode order (>= 0: emit this token, < 0: draw) = partial decoding."""
        cfg = self.cfg
        d = self.device
        cond_ids = _req(cond_ids, torch.int64, d, "cond_ids")
        I_inv = _req(I_inv, torch.float32, d, "I_inv")
        E_inv = _req(E_inv, torch.float32, d, "E_inv")
        B = cond_ids.shape[0]
        steps = cfg.num_img_tokens if steps is None else int(steps)
        if noise_u is not None:
            noise_u = _req(noise_u, torch.float32, d, "noise_u")
            assert tuple(noise_u.shape) == (steps, B)
        out = torch.empty((B, cfg.num_cams, cfg.num_cam_tokens), dtype=torch.int64, device=d)
        logits = torch.empty((steps, B, cfg.vocab_size), dtype=torch.float32, device=d) if return_logits else None
        if forced_ids is not None:
            forced_ids = _req(forced_ids, torch.int64, d, "forced_ids")
            assert tuple(forced_ids.shape) == (steps, B)
        self._check(self.lib.bevgen_ar_sample_forced(self._h, _ptr(cond_ids), _ptr(I_inv), _ptr(E_inv), B, steps, int(top_k or 0), float(temperature), int(bool(greedy)),
                                                      _ptr(noise_u), int(samples_per_layout), _ptr(forced_ids), _ptr(out), _ptr(logits), self._s()))
        self._done(check)
        return (out, logits) if return_logits else out

    # ------------------------------------------------------------------------------------------ stage 1
    def _vq_levels(self):
        return len(self.vq_ddconfig["ch_mult"]) - 1

    def _latent_grid(self, latent_hw, tokens=None):
        """(lat_h, lat_w): explicit, else the square grid of ddconfig.resolution.  The decoder is fully convolutional: nuScenes uses 14 x 25."""
        if latent_hw is None:
            lat = self.vq_ddconfig["resolution"] >> self._vq_levels()
            latent_hw = (lat, lat)
        lh, lw = int(latent_hw[0]), int(latent_hw[1])
        if tokens is not None and tokens != lh * lw:
            raise ValueError(f"{tokens} token ids per image do not fill the {lh} x {lw} latent grid: pass latent_hw=cam_latent_res")
        return lh, lw

    def vq_decode(self, ids, denormalize=True, latent_hw=None, uint8=False, check=True):
        """ids [n, lat_h*lat_w] -> [n, out_ch, H, W] fp32 (raw or denormalised to [0,1]) or, with uint8=True, the round(255 x) storage format."""
        dd = self.vq_ddconfig
        ids = _req(ids, torch.int64, self.device, "ids")
        n = ids.shape[0]
        ids = ids.reshape(n, -1)
        lh, lw = self._latent_grid(latent_hw, ids.shape[1])
        f = 1 << self._vq_levels()
        mode = _lib.VQ_OUT_U8 if uint8 else (_lib.VQ_OUT_DENORM if denormalize else _lib.VQ_OUT_RAW)
        out = torch.empty((n, dd["out_ch"], lh * f, lw * f), dtype=torch.uint8 if uint8 else torch.float32, device=self.device)
        self._check(self.lib.bevgen_vq_decode(self._h, _ptr(ids), n, lh, lw, mode, _ptr(out), self._s()))
        self._done(check)
        return out

    def vq_encode(self, x, check=True):
        """VQModel.encode -> token ids: x [n, in_channels, H, W] fp32 (NCHW; H, W multiples of 2^(levels-1)) -> ids [n, h*w] int64.
        precision='f16x3': an image or a residual stream outside the f16 operand range raises BevgenError (ERR_NUMERIC); precision='f16x3r' rescales the image (conv_in),
        the residual stream in front of every nin_shortcut and downsample convolution and conv_out's output (quant_conv) by a per-tensor power of two instead
        (vq_range_exponents); where nothing leaves the range the ids are those of 'f16x3' bit for bit."""
        dd = self.vq_ddconfig
        x = _req(x, torch.float32, self.device, "x")
        n, ch, H, W = x.shape
        f = 1 << self._vq_levels()
        if ch != dd["in_channels"] or H % f or W % f:
            raise ValueError(f"vq_encode: input {tuple(x.shape)} needs {dd['in_channels']} channels and sides divisible by {f}")
        ids = torch.empty((n, (H // f) * (W // f)), dtype=torch.int64, device=self.device)
        self._check(self.lib.bevgen_vq_encode(self._h, _ptr(x), n, H, W, _ptr(ids), self._s()))
        self._done(check)
        return ids

    def vq_encode_ex(self, x, I_inv=None, E_inv=None, plane=None, beta=0.25, want_loss=True, check=True):
        """vq_encode with the geometric embedding of a camera VQGAN and the quantizer's error -> (ids [n, h*w], row_err [n, h*w], loss 0-dim or None).
        I_inv [n, 3, 3], E_inv [n, 4, 4] (one per image) and plane [3, h*w] go together: a context loaded with img_embed / cam_embed needs them, one without refuses them
        (BevgenError).  row_err = |codebook[id] - z|^2 per latent row; loss = (1 + beta) mean(row_err) / embed_dim over all rows, accumulated in double in a fixed order."""
        dd = self.vq_ddconfig
        x = _req(x, torch.float32, self.device, "x")
        n, ch, H, W = x.shape
        f = 1 << self._vq_levels()
        if ch != dd["in_channels"] or H % f or W % f:
            raise ValueError(f"vq_encode_ex: input {tuple(x.shape)} needs {dd['in_channels']} channels and sides divisible by {f}")
        T = (H // f) * (W // f)
        geo = [I_inv, E_inv, plane]
        if any(g is not None for g in geo):
            if any(g is None for g in geo):
                raise ValueError("vq_encode_ex: I_inv, E_inv and plane go together")
            I_inv, E_inv, plane = (_req(g, torch.float32, self.device, "geometry") for g in geo)
            if tuple(I_inv.shape) != (n, 3, 3) or tuple(E_inv.shape) != (n, 4, 4) or plane.numel() != 3 * T:
                raise ValueError(f"vq_encode_ex: geometry {tuple(I_inv.shape)}, {tuple(E_inv.shape)}, {tuple(plane.shape)} does not fit {n} images of {T} latent pixels")
        ids = torch.empty((n, T), dtype=torch.int64, device=self.device)
        row_err = torch.empty((n, T), dtype=torch.float32, device=self.device)
        loss = torch.empty((), dtype=torch.float32, device=self.device) if want_loss else None
        self._check(self.lib.bevgen_vq_encode_ex(self._h, _ptr(x), n, H, W, _ptr(I_inv), _ptr(E_inv), _ptr(plane), float(beta), _ptr(ids), _ptr(row_err), _ptr(loss), self._s()))
        self._done(check)
        return ids, row_err, loss

    def vq_decode_latents(self, zq, denormalize=False, check=True):
        """VQModel.decode(quant): zq [n, embed_dim, h, w] fp32."""
        dd = self.vq_ddconfig
        zq = _req(zq, torch.float32, self.device, "zq")
        n, _, lh, lw = zq.shape
        f = 1 << self._vq_levels()
        out = torch.empty((n, dd["out_ch"], lh * f, lw * f), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_vq_decode_latents(self._h, _ptr(zq), n, lh, lw, _lib.VQ_OUT_DENORM if denormalize else _lib.VQ_OUT_RAW, _ptr(out), self._s()))
        self._done(check)
        return out

    def vq_range_exponents(self, cap: int = 4096):
        """precision='f16x3r': the exponents the most recent vq_decode / vq_decode_latents / vq_encode chose, in site order (per pass of up to 48 images; decode: conv_in,
        then every nin_shortcut and upsample convolution as executed; encode: conv_in, then every nin_shortcut and downsample convolution as executed, then quant_conv),
        as an int32 numpy array; empty in every other mode.  Synchronises."""
        buf = (C.c_int32 * cap)()
        n = C.c_int(0)
        self._check(self.lib.bevgen_vq_range_exponents(self._h, buf, cap, C.byref(n)))
        return np.frombuffer(buf, dtype=np.int32, count=min(n.value, cap)).copy()

    # ------------------------------------------------------------------------------------------ per-kernel HIP-event timing
    PROFILE_KINDS = ("gemm", "conv3x3", "attention", "decode_attention", "gemm_skinny", "gemm_small")

    def profile_begin(self):
        self._check(self.lib.bevgen_profile_begin(self._h))

    def profile_end(self) -> Dict[str, Dict[str, float]]:
        """{kind: {'launches', 'ms', 'work'}}; work = FLOP (gemm/conv/attention) or bytes (decode_attention/gemm_skinny)."""
        buf = (C.c_double * (3 * len(self.PROFILE_KINDS)))()
        self._check(self.lib.bevgen_profile_end(self._h, buf))
        return {k: {"launches": buf[3 * i], "ms": buf[3 * i + 1], "work": buf[3 * i + 2]} for i, k in enumerate(self.PROFILE_KINDS)}

    def ar_step_timing(self, enable: bool = True):
        self._check(self.lib.bevgen_ar_step_timing(self._h, int(enable)))

    def ar_step_times(self, cap: int = 4096):
        """Durations (ms) of the decode steps of the most recent ar_sample (graph replays), as a float32 numpy array."""
        buf = (C.c_float * cap)()
        n = C.c_int(0)
        self._check(self.lib.bevgen_ar_step_times(self._h, buf, cap, C.byref(n)))
        return np.frombuffer(buf, dtype=np.float32, count=n.value).copy()

    def trace_begin(self):
        """Diagnostics: phase timestamps of the fused decode kernels (last launch of each kind)."""
        self._trace = torch.zeros((3, 4096, 8), dtype=torch.int64, device=self.device)
        self._check(self.lib.bevgen_set_trace_buffer(self._h, _ptr(self._trace)))

    def trace_end(self):
        torch.cuda.synchronize()
        self._check(self.lib.bevgen_set_trace_buffer(self._h, None))
        return self._trace.cpu()

    # ------------------------------------------------------------------------------------------ operator level (tests / roofline)
    def op_gemm(self, a, w, bias=None, residual=None, gelu=False, skinny=False):
        M, K = a.shape
        N = w.shape[0]
        c = torch.empty((M, N), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_gemm(self._h, _ptr(a), _ptr(w), _ptr(bias), _ptr(residual), _ptr(c), M, N, K, int(gelu), int(skinny), self._s()))
        return c

    def op_muse_qkv(self, kind, a, w, *, B, T, H, ld=0, q_scale=None, k_scale=None, null_kv=None, ln_gamma=None, post=1.0, block=0, weights=0, form=0, ksplit=1, out=None):
        """Route M's to_q / to_kv / q|k|v projection (kind 'q' | 'kv' | 'qkv') with its fused epilogue (form 0) or un-fused (form 1) on a [B T, K] and w [N, K].
        Returns the f16 planes it wrote as a dict: Qh, Ql [B, H, T, 64]; Kh, Kl [B, H, ld, 64]; VTh, VTl [B, H, 64, ld].  `out`: caller-owned planes of those names
        (any float16 tensors of the right size - the library never clears them); missing ones are allocated zero-filled."""
        k = {"q": 0, "kv": 1, "qkv": 2}[kind]
        K = a.shape[1]
        out = dict(out or {})
        shapes = {"Qh": (B, H, T, 64), "Ql": (B, H, T, 64), "Kh": (B, H, ld, 64), "Kl": (B, H, ld, 64), "VTh": (B, H, 64, ld), "VTl": (B, H, 64, ld)}
        for name in (("Qh", "Ql") if k != 1 else ()) + (("Kh", "Kl", "VTh", "VTl") if k != 0 else ()):
            if name not in out:
                out[name] = torch.zeros(shapes[name], dtype=torch.float16, device=self.device)
        self._check(self.lib.bevgen_op_muse_qkv(self._h, k, _ptr(a), _ptr(w), _ptr(ln_gamma), _ptr(q_scale), _ptr(k_scale), _ptr(null_kv), int(B), int(T), int(H), int(K), int(ld),
                                                float(post), int(block), int(weights), int(form), int(ksplit), _ptr(out.get("Qh")), _ptr(out.get("Ql")), _ptr(out.get("Kh")),
                                                _ptr(out.get("Kl")), _ptr(out.get("VTh")), _ptr(out.get("VTl")), self._s()))
        return out

    def op_muse_ff(self, x, w1, gamma3, w4, residual, *, level=0, merge=0, block=0, out=None):
        """Route M's feed-forward behind its first LayerNorm, y = LN_gamma3(GEGLU(x w1^T)) w4^T + residual, in fold form `level` (include/bevgen_hip.h).  `out`: caller-owned
        outputs by name - h [M, Fpad] fp32, g_planes [M, Fpad / 32, 2, 32] f16, g_sums [Fpad / 32, M, 2], rowstat [M, 2], y_planes [M, Dout / 32, 2, 32] f16,
        y_sums [Dout / 32, M, 2], y [M, Dout]; y is allocated when missing, the others stay library scratch.  Returns the dict."""
        M, D = x.shape
        F, Dout = gamma3.numel(), w4.shape[0]
        out = dict(out or {})
        if "y" not in out:
            out["y"] = torch.empty((M, Dout), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_muse_ff(self._h, _ptr(x), _ptr(w1), _ptr(gamma3), _ptr(w4), _ptr(residual), M, D, F, Dout, int(level), int(merge), int(block),
                                               _ptr(out.get("h")), _ptr(out.get("g_planes")), _ptr(out.get("g_sums")), _ptr(out.get("rowstat")), _ptr(out.get("y_planes")),
                                               _ptr(out.get("y_sums")), _ptr(out["y"]), self._s()))
        return out

    def op_layernorm_planes(self, x, gamma, beta=None, *, D, ldy, geglu=False, planes=None, rows=None):
        """LayerNorm over the first D columns of x's rows (geglu: x = (a | gate) of 2 D columns, the rows normalised are gate * gelu(a)) as the interleaved f16 plane image
        [rows, ldy / 32, 2, 32] = (hi 32 | lo 32) per 32 columns.  `planes`: a caller-owned image (never cleared); `rows`: fewer rows than x / planes hold."""
        rows = x.shape[0] if rows is None else int(rows)
        if planes is None:
            planes = torch.zeros((rows, ldy // 32, 2, 32), dtype=torch.float16, device=self.device)
        self._check(self.lib.bevgen_op_layernorm_planes(self._h, _ptr(x), x.stride(0), _ptr(gamma), _ptr(beta), _ptr(planes), int(ldy), rows, int(D), int(geglu), self._s()))
        return planes

    def op_ln_gemm(self, a, w, ln_w=None, ln_b=None, bias=None, gelu=False, ksplit=0, eps=1e-5):
        """Decode-step projection kernel: act(LN?(a) w^T + bias); with K split over workgroups the partial sums are added here (the model path folds
        that sum into the consumer's row fetch)."""
        M, K = a.shape
        N = w.shape[0]
        ks = C.c_int(0)
        out = torch.empty((4, M, N), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_ln_gemm(self._h, _ptr(a), _ptr(ln_w), _ptr(ln_b), float(eps), _ptr(w), _ptr(bias), _ptr(out), M, N, K, int(gelu), int(ksplit),
                                               C.byref(ks), self._s()))
        return out[0] if ks.value == 1 else out[:ks.value].sum(0)

    def op_quantize_rows_i8(self, w, dequant=True):
        """The row quantiser of decode_weights='i8' alone: w [N, K] fp32 -> (codes [N, K] int8, scales [N] fp32, code * scale [N, K] fp32 or None)."""
        N, K = w.shape
        codes = torch.empty((N, K), dtype=torch.int8, device=self.device)
        scales = torch.empty((N,), dtype=torch.float32, device=self.device)
        deq = torch.empty((N, K), dtype=torch.float32, device=self.device) if dequant else None
        self._check(self.lib.bevgen_op_quantize_rows_i8(self._h, _ptr(w), N, K, _ptr(codes), _ptr(scales), _ptr(deq), self._s()))
        return codes, scales, deq

    def op_mlp_fused(self, x, ln_w, ln_b, w1, b1, w2, b2, w_f16=False, eps=1e-5):
        """Both MLP projections of a Route A decode layer in one launch: Linear2(GELU(Linear1(LayerNorm(x)))) for M <= 64 rows, without the residual.
        w_f16: False / 0 fp32 weights, True / 1 rounded to fp16, 2 int8 codes with row scales (decode_weights='i8')."""
        M, D = x.shape
        out = torch.empty((M, D), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_mlp_fused(self._h, _ptr(x), _ptr(ln_w), _ptr(ln_b), float(eps), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), int(w_f16), _ptr(out), M, D, self._s()))
        return out

    # token samplers / scorers (sampler.hip): the tensors are handed over as they are - a row stride or an offset view is part of what the caller tests
    @staticmethod
    def _ld(t, ld):
        assert t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), "rows must be unit-stride"
        return int(ld) if ld is not None else (t.stride(0) if t.shape[0] > 1 else t.shape[1])

    def op_remask(self, ids, scores, n_mask, mask_id, init_ids=None):
        """In place on ids [rows, T] int64: the n_mask highest scores of each row (ties: lower index first) become mask_id, then init_ids != mask_id are re-imposed."""
        rows, T = ids.shape
        self._check(self.lib.bevgen_op_remask(self._h, _ptr(ids), _ptr(scores), _ptr(init_ids), rows, T, int(n_mask), int(mask_id), self._s()))
        return ids

    def op_maskgit_pick(self, ids, logits, V, *, mask_id, k=None, topk_filter_thres=None, temperature=1.0, gumbel_u=None, seed=0, it=0, conf_scores=None, conf_mode=0, ldl=None):
        """In place on ids [rows] int64 (only entries == mask_id change); logits [rows, ldl >= V].  k, or topk_filter_thres as MaskGit.generate takes it (k = ceil((1 - thres) V);
        a threshold that keeps no logit is refused by the library like k = 0)."""
        if k is None:
            k = V if topk_filter_thres is None else topk_count(topk_filter_thres, V)
        self._check(self.lib.bevgen_op_maskgit_pick(self._h, _ptr(ids), _ptr(logits), self._ld(logits, ldl), _ptr(gumbel_u), ids.numel(), int(V), int(k), float(temperature),
                                                    int(mask_id), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(it), _ptr(conf_scores), int(conf_mode), self._s()))
        return ids

    def op_critic_scores(self, embed, w, b, D=None, *, u=None, noise_scale=0.0, frac=0.0, seed=0, it=0, lde=None):
        """scores [rows] = embed[:, :D] . w + b + ((u - 0.5) * noise_scale) * frac; u explicit, else Philox stream 1 of (seed, it) when seed != 0, else 0.5."""
        rows = embed.shape[0]
        D = embed.shape[1] if D is None else int(D)
        scores = torch.empty((rows,), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_critic_scores(self._h, _ptr(embed), self._ld(embed, lde), _ptr(w), _ptr(b), _ptr(u), float(noise_scale), float(frac),
                                                     C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(it), _ptr(scores), rows, D, self._s()))
        return scores

    def op_maskgit_train_mask(self, ids, num_masked, mask_id, *, perm_u=None, seed=0, x=None, mask=None):
        """(x int64, mask uint8), each [rows, T] (written in place where given): mask = argsort(u) < num_masked[row], ties by index; u = perm_u [rows, T], else Philox
        stream 2 of `seed`; num_masked [rows] int32 on the device."""
        rows, T = ids.shape
        x = torch.empty_like(ids) if x is None else x
        mask = torch.empty((rows, T), dtype=torch.uint8, device=self.device) if mask is None else mask
        self._check(self.lib.bevgen_op_maskgit_train_mask(self._h, _ptr(ids), _ptr(perm_u), _ptr(num_masked), rows, T, int(mask_id), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                                          _ptr(x), _ptr(mask), self._s()))
        return x, mask

    def op_masked_ce(self, logits, V, ids, mask, *, denom=None, nll=None, out=None, ldl=None):
        """(nll [rows], mean) of logits [rows, ldl >= V]: nll = logsumexp - logit[id] where mask (uint8), 0 elsewhere; mean = sum(nll) / denom (None: not computed)."""
        rows = ids.numel()
        nll = torch.empty((rows,), dtype=torch.float32, device=self.device) if nll is None else nll
        if denom is not None and out is None:
            out = torch.empty((), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_masked_ce(self._h, _ptr(logits), self._ld(logits, ldl), _ptr(ids), _ptr(mask), rows, int(V), int(denom or 0), _ptr(nll),
                                                 _ptr(out if denom is not None else None), self._s()))
        return nll, out

    def op_critic_bce(self, embed, w, b, ids, critic_input, D=None, *, loss_rows=None, want_mean=True, lde=None):
        """(loss [rows], mean): BCE-with-logits of z = embed[:, :D] . w + b against the label (ids != critic_input)."""
        rows = ids.numel()
        D = embed.shape[1] if D is None else int(D)
        loss_rows = torch.empty((rows,), dtype=torch.float32, device=self.device) if loss_rows is None else loss_rows
        out = torch.empty((), dtype=torch.float32, device=self.device) if want_mean else None
        self._check(self.lib.bevgen_op_critic_bce(self._h, _ptr(embed), self._ld(embed, lde), _ptr(w), _ptr(b), _ptr(ids), _ptr(critic_input), rows, D, _ptr(loss_rows),
                                                  _ptr(out), self._s()))
        return loss_rows, out

    def op_ar_pick(self, logits, V, *, top_k=0, temperature=1.0, u=None, step=None, forced=None, ldl=None, out_all=None, fwd_idx=None, tok_emb=None, img_embed=None,
                   pos_emb=None, x=None, C_=0, T=0):
        """tokens [rows] of logits [rows, ldl >= V]; u / forced [steps, rows] with `step` a device int32 counter (None: their first row).  Tail: out_all [rows, N] and
        x [rows, D] are written in place (kernels.h ArPickTail)."""
        rows = logits.shape[0]
        out = torch.empty((rows,), dtype=torch.int64, device=self.device)
        self._check(self.lib.bevgen_op_ar_pick(self._h, _ptr(logits), self._ld(logits, ldl), _ptr(u), _ptr(step), _ptr(forced), _ptr(out), rows, int(V), int(top_k),
                                               float(temperature), _ptr(out_all), _ptr(fwd_idx), 0 if out_all is None else out_all.shape[1], _ptr(tok_emb), _ptr(img_embed),
                                               _ptr(pos_emb), _ptr(x), int(C_), int(T), 0 if x is None else x.shape[1], 0 if tok_emb is None else tok_emb.shape[0], self._s()))
        return out

    def op_ar_score_rows(self, logits, V, fwd_idx, *, target=None, weight=None, b=0, s0=0, rows=None, N=None, nll=None, wnll=None, ldl=None):
        """nll / wnll [rows] (written in place where given) of decode positions [s0, s0 + rows) of sequence b; target / weight [B, N] camera-major."""
        rows = logits.shape[0] if rows is None else int(rows)
        N = fwd_idx.numel() if N is None else int(N)
        self._check(self.lib.bevgen_op_ar_score_rows(self._h, _ptr(logits), self._ld(logits, ldl), _ptr(target), _ptr(weight), _ptr(fwd_idx), int(b), int(s0), rows, N, int(V),
                                                     _ptr(nll), _ptr(wnll), self._s()))
        return nll, wnll

    def op_mean_fixed_order(self, x):
        out = torch.empty((), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_mean_fixed_order(self._h, _ptr(x), x.numel(), _ptr(out), self._s()))
        return out

    def op_add_row_layernorm(self, x, r, gamma, *, planes=False, ldy=None, rows=None, out=None):
        """x [rows, D] += r [D] in place, then LayerNorm (gamma, eps 1e-5) of the updated rows -> fp32 [rows, ldy] or (planes) the raw plane image as int16
        [rows, ldy / 32, 2, 32] (``bevgen_op_add_row_layernorm``).  ``rows`` < x.shape[0]: only the leading rows are touched; ``out``: a caller-owned result (never cleared)."""
        D = x.shape[-1]
        n = x.shape[0] if rows is None else int(rows)
        ldy = D if ldy is None else int(ldy)
        y = out
        if y is None:
            y = torch.empty((n, ldy // 32, 2, 32), dtype=torch.int16, device=self.device) if planes else torch.empty((n, ldy), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_add_row_layernorm(self._h, _ptr(x), x.stride(0), _ptr(r), _ptr(gamma), _ptr(y), ldy, n, D, int(bool(planes)), self._s()))
        return y

    def op_cfg_combine(self, cond, null, scale, *, V=None):
        """cond[:, :V] = null + (cond - null) * scale in place on 2-D fp32 tensors with row strides (``bevgen_op_cfg_combine``)."""
        V = cond.shape[1] if V is None else int(V)
        self._check(self.lib.bevgen_op_cfg_combine(self._h, _ptr(cond), cond.stride(0), _ptr(null), null.stride(0), cond.shape[0], V, float(scale), self._s()))
        return cond

    def op_layernorm(self, x, gamma, beta=None, eps=1e-5):
        y = torch.empty_like(x)
        self._check(self.lib.bevgen_op_layernorm(self._h, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), x.shape[0], x.shape[1], float(eps), self._s()))
        return y

    def op_geglu_layernorm(self, h, gamma, ldy=None):
        rows, two_f = h.shape
        F = two_f // 2
        ldy = ldy or F
        y = torch.empty((rows, ldy), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_geglu_layernorm(self._h, _ptr(h), _ptr(gamma), _ptr(y), rows, F, ldy, self._s()))
        return y

    def op_attention(self, q, k, v, bias, scale, key_splits=1):
        B, H, Nq, _ = q.shape
        Nk_pad = k.shape[2]
        out = torch.empty((B, Nq, H * 64), dtype=torch.float32, device=self.device)
        ld = 0 if bias is None else bias.shape[-1]
        self._check(self.lib.bevgen_op_attention_ex(self._h, _ptr(q), _ptr(k), _ptr(v), _ptr(bias), ld, B, H, Nq, Nk_pad, float(scale), int(key_splits), _ptr(out),
                                                    self._s()))
        return out

    def op_muse_attention(self, planes, bias, *, B, H, Nq, Nk_pad, kv_group=1, key_splits=1, out=None, out_planes=None):
        """Route M's split-precision attention as the model launches it, on the f16 planes of op_muse_qkv: planes = dict Qh, Ql [B, H, Nq, 64]; Kh, Kl [B / kv_group, H,
        Nk_pad, 64]; VTh, VTl [B / kv_group, H, 64, Nk_pad].  bias [Nq, ld] fp32 or None: base-2 domain, -1e30 = hidden (include/bevgen_hip.h).  Exactly one of `out`
        (fp32 [B, Nq, 64 H]) and `out_planes` (f16 image [B Nq, 64 H / 32, 2, 32]), both caller-owned and never cleared."""
        ld = 0 if bias is None else bias.shape[-1]
        self._check(self.lib.bevgen_op_muse_attention(self._h, _ptr(planes["Qh"]), _ptr(planes["Ql"]), _ptr(planes["Kh"]), _ptr(planes["Kl"]), _ptr(planes["VTh"]),
                                                      _ptr(planes["VTl"]), _ptr(bias), int(ld), int(B), int(H), int(Nq), int(Nk_pad), int(kv_group), int(key_splits), _ptr(out),
                                                      _ptr(out_planes), self._s()))

    @staticmethod
    def _cache_lmax(kcache, kv_dtype, Lmax):
        # kv_dtype 2 (int8): the cache is a flat uint8 buffer in the BEVGEN_KV_I8 layout (codes, then row scales) and says nothing about Lmax
        if int(kv_dtype) == 2:
            if Lmax is None:
                raise ValueError("kv_dtype=2 (int8 cache): pass Lmax explicitly, the cache is a flat uint8 buffer")
            return int(Lmax)
        return kcache.shape[2] if Lmax is None else int(Lmax)

    def op_decode_attention(self, q, kcache, vcache, n, bias=None, keep=None, scale=0.125, kv_dtype=0, Lmax=None):
        B, HD = q.shape
        H = HD // 64
        Lmax = self._cache_lmax(kcache, kv_dtype, Lmax)
        out = torch.empty((B, HD), dtype=torch.float32, device=self.device)
        ldb = 0 if bias is None else bias.shape[-1]
        ldk = 0 if keep is None else keep.shape[-1]
        khs = 0 if keep is None or keep.dim() < 3 or keep.shape[0] == 1 else keep.shape[1] * keep.shape[2]
        self._check(self.lib.bevgen_op_decode_attention(self._h, _ptr(q), _ptr(kcache), _ptr(vcache), int(kv_dtype), _ptr(bias), ldb, _ptr(keep), ldk, khs,
                                                         B, H, int(n), Lmax, float(scale), _ptr(out), self._s()))
        return out

    def op_ar_attn_fused(self, x, ln_w, ln_b, wqkv, bqkv, kcache, vcache, n, *, partial=None, rbias=None, bias=None, attn_mask=None, layout=None, block=1, G=1, prefix=0,
                         kv_dtype=0, w_f16=False, split=False, Lmax=None):
        """Attention half of a fused Route A decode layer (appends k/v to cache row n-1 in place) -> x2 [B, D].  kv_dtype 2: flat uint8 caches + an explicit Lmax.
        w_f16: False / 0 fp32 projection weights, True / 1 rounded to fp16, 2 int8 codes with row scales (decode_weights='i8')."""
        B, D = x.shape
        H = D // 64
        Lmax = self._cache_lmax(kcache, kv_dtype, Lmax)
        out = torch.empty((B, D), dtype=torch.float32, device=self.device)
        ns = 0 if partial is None else partial.shape[0]
        self._check(self.lib.bevgen_op_ar_attn_fused(self._h, _ptr(x), _ptr(partial), ns, _ptr(rbias), _ptr(ln_w), _ptr(ln_b), _ptr(wqkv), _ptr(bqkv), int(w_f16),
                                                     _ptr(kcache), _ptr(vcache), int(kv_dtype), _ptr(bias), 0 if bias is None else bias.shape[-1], _ptr(attn_mask),
                                                     _ptr(layout), int(block), B, int(G), H, int(n), Lmax, int(prefix), int(split), _ptr(out), self._s()))
        return out

    def op_conv3x3(self, x_nhwc, w_ohwi, bias, residual=None, upsample=False, kernel="auto", act=None):
        """kernel: 'auto' (fp32 input: the register-staged kernel), 'dma' (the LDS-DMA kernel on planes split inside the call), 'dma_general' (its general variant
        also where the stride-1 variant applies).  act: None, or 'relu' = max(0, acc + bias) in the epilogue (bevgen_op_conv3x3_act)."""
        if act not in (None, "relu"):
            raise ValueError(f"op_conv3x3: act must be None or 'relu', got {act!r}")
        n, H, W, Cin = x_nhwc.shape
        Cout = w_ohwi.shape[0]
        oh, ow = (2 * H, 2 * W) if upsample else (H, W)
        y = torch.empty((n, oh, ow, Cout), dtype=torch.float32, device=self.device)
        flags = int(upsample) | {"auto": 0, "dma": 2, "dma_general": 6}[kernel]
        if act is None:
            self._check(self.lib.bevgen_op_conv3x3(self._h, _ptr(x_nhwc), _ptr(w_ohwi), _ptr(bias), _ptr(residual), _ptr(y), n, H, W, Cin, Cout, flags, self._s()))
        else:
            self._check(self.lib.bevgen_op_conv3x3_act(self._h, _ptr(x_nhwc), _ptr(w_ohwi), _ptr(bias), _ptr(residual), _ptr(y), n, H, W, Cin, Cout, flags, 1, self._s()))
        return y

    # LPIPS (csrc/lpips.cpp, lpips_kernels.hip; bevgen_amd/metrics.py builds LearnedPerceptualImagePatchSimilarity on it)
    def op_maxpool2x2(self, x_nhwc, planes=False):
        """MaxPool2d(2, 2) over NHWC fp32 [n, H, W, C] (C % 32 == 0; odd sizes floor) -> y [n, H // 2, W // 2, C]; planes=True: (y, planes) with planes
        [n (H // 2) (W // 2), C / 32, 2, 32] float16 = the (hi, lo) image of y written by the same pass (op_range_split's layout at exponent 0)."""
        n, H, W, Cc = x_nhwc.shape
        y = torch.empty((n, H // 2, W // 2, Cc), dtype=torch.float32, device=self.device)
        pl = torch.empty((n * (H // 2) * (W // 2), Cc // 32, 2, 32), dtype=torch.float16, device=self.device) if planes else None
        self._check(self.lib.bevgen_op_maxpool2x2(self._h, _ptr(x_nhwc), _ptr(y), _ptr(pl), n, H, W, Cc, self._s()))
        return (y, pl) if planes else y

    def op_lpips_tap(self, fa, fb, w):
        """d [n] float64 = mean over the pixels of sum_c w_c (fa^ - fb^)^2, f^ = f / (sqrt(sum_c f^2) + 1e-10): fa, fb [n, pixels, C] fp32 (C = 64, 128, 256 or 512)."""
        if fa.shape != fb.shape or fa.dim() != 3:
            raise ValueError(f"op_lpips_tap: features are two [n, pixels, C] tensors, got {tuple(fa.shape)} and {tuple(fb.shape)}")
        n, pix, Cc = fa.shape
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        self._check(self.lib.bevgen_op_lpips_tap(self._h, _ptr(fa), _ptr(fb), _ptr(w), n, pix, Cc, _ptr(out), self._s()))
        return out

    def _precision_code(self):
        return int(self._c.precision)

    def lpips_prepare(self, state):
        """state: what metrics.load_lpips_state returns ({'conv_w': 13 tensors [Cout, Cin, 3, 3], 'conv_b': 13, 'lin': 5 vectors, 'shift', 'scale'}) -> the prepared
        weight image, a uint8 device tensor this context's lpips() reads (it belongs to this context's precision)."""
        dev = self.device
        ws = [_req(t, torch.float32, dev, "conv weight") for t in state["conv_w"]]
        bs = [_req(t, torch.float32, dev, "conv bias") for t in state["conv_b"]]
        lins = [_req(t.reshape(-1), torch.float32, dev, "lin") for t in state["lin"]]
        if len(ws) != 13 or len(bs) != 13 or len(lins) != 5:
            raise ValueError("lpips_prepare: needs 13 convolution weights, 13 biases and 5 lin vectors (metrics.load_lpips_state)")
        shift, scale = _req(state["shift"].reshape(-1), torch.float32, dev, "shift"), _req(state["scale"].reshape(-1), torch.float32, dev, "scale")
        nbytes = int(self.lib.bevgen_lpips_prepared_bytes(self._precision_code()))
        if nbytes < 0:
            raise ValueError("lpips_prepare: this context's precision has no LPIPS path")
        prepared = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        self._check(self.lib.bevgen_lpips_prepare(self._h, arr(ws), arr(bs), arr(lins), _ptr(shift), _ptr(scale), _ptr(prepared), self._s()))
        self.synchronize()   # (the sources may be freed when this returns; a weight outside the f16 range is reported here)
        return prepared

    def lpips(self, prepared, a, b, normalize=False, return_layers=False, check=True):
        """LPIPS (VGG16) per image pair -> scores [n] float64 on the device (return_layers: (scores, layers [n, 5])).  a, b [n, 3, H, W] or [B, cams, 3, H, W], both fp32
        (nominally in [0, 1]; normalize=True maps x -> 2 x - 1 first, as the reference's metric class does for [0, 1] inputs it rescales - metrics_eval.py feeds [0, 1]
        images with normalize=False, the default here) or both uint8 (v / 255).  H, W >= 16.  torchmetrics' host-side check that the inputs lie in the expected range
        is not reproduced: it would need a synchronising min / max per call."""
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError(f"lpips: preds {tuple(a.shape)} {a.dtype} and target {tuple(b.shape)} {b.dtype} differ in shape or dtype")
        if a.dim() == 5:
            a, b = a.reshape(-1, *a.shape[2:]), b.reshape(-1, *b.shape[2:])
        if a.dim() != 4 or a.shape[1] != 3:
            raise ValueError(f"lpips: images are [n, 3, H, W] or [B, cams, 3, H, W], got {tuple(a.shape)}")
        if a.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"lpips: images are float32 or uint8, got {a.dtype}")
        a, b = _req(a, a.dtype, self.device, "preds"), _req(b, b.dtype, self.device, "target")
        n, _, H, W = a.shape
        nbytes = int(self.lib.bevgen_lpips_workspace_bytes(n, H, W, self._precision_code()))
        if nbytes < 0:
            raise ValueError(f"lpips: images [{n}, 3, {H}, {W}] are refused (needs n >= 1, H and W >= 16 so that relu5_3 has a pixel, H W <= 2^21)")
        work = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        out = torch.empty((n,), dtype=torch.float64, device=self.device)
        layers = torch.empty((n, 5), dtype=torch.float64, device=self.device) if return_layers else None
        self._check(self.lib.bevgen_lpips(self._h, _ptr(prepared), _ptr(a), _ptr(b), self._METRIC_DTYPES[a.dtype], n, H, W, int(bool(normalize)), _ptr(out), _ptr(layers),
                                          _ptr(work), self._s()))
        self._done(check)
        return (out, layers) if return_layers else out

    def op_groupnorm(self, x_nhwc, gamma, beta, swish=True):
        n, H, W, Cc = x_nhwc.shape
        y = torch.empty_like(x_nhwc)
        self._check(self.lib.bevgen_op_groupnorm(self._h, _ptr(x_nhwc), _ptr(gamma), _ptr(beta), _ptr(y), n, H * W, Cc, int(swish), self._s()))
        return y

    def op_range_split(self, x_nhwc, check=True):
        """The range-safe operand preparation of precision='f16x3r' on its own: x [n, hw, C] fp32 (C % 32 == 0) -> (planes, e) with e the exponent (0 where max |x| < 32768,
        else the smallest e with max |x| 2^-e < 32768; a one-element int32 tensor) and planes [n * hw, C / 32, 2, 32] float16 = the (hi, lo) image of x 2^-e:
        x = (hi + lo 2^-11) 2^e.  NaN / inf in x raise BevgenError (ERR_NUMERIC)."""
        x = _req(x_nhwc, torch.float32, self.device, "x")
        n, hw, Cc = x.shape
        planes = torch.empty((n * hw, Cc // 32, 2, 32), dtype=torch.float16, device=self.device)
        e = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._check(self.lib.bevgen_op_range_split(self._h, _ptr(x), n, hw, Cc, _ptr(planes), _ptr(e), self._s()))
        self._done(check)
        return planes, e

    # building blocks of the stage-1 VQGAN (vqdec.cpp): NHWC activations, convolution weights as the checkpoint stores them ([Cout, Cin, kh, kw])
    def op_conv3x3_down(self, x_nhwc, w_oihw, bias=None):
        """The encoder's Downsample: F.pad(x, (0, 1, 0, 1)) + 3x3 convolution, stride 2, padding 0 -> [n, H / 2, W / 2, Cout]."""
        n, H, W, Cin = x_nhwc.shape
        Cout = w_oihw.shape[0]
        y = torch.empty((n, H // 2, W // 2, Cout), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_conv3x3_down(self._h, _ptr(x_nhwc), _ptr(w_oihw), _ptr(bias), _ptr(y), n, H, W, Cin, Cout, self._s()))
        return y

    def op_vq_attn_block(self, x_nhwc, norm_w, norm_b, wq, bq, wk, bk, wv, bv, wp, bp):
        """AttnBlock.forward: x + proj_out(softmax(q k^T C^-0.5) v) over the h w pixels of each image; the four weights are [C, C] (1x1 convolutions)."""
        n, h, w, Cc = x_nhwc.shape
        y = torch.empty_like(x_nhwc)
        self._check(self.lib.bevgen_op_vq_attn_block(self._h, _ptr(x_nhwc), _ptr(norm_w), _ptr(norm_b), _ptr(wq), _ptr(bq), _ptr(wk), _ptr(bk), _ptr(wv), _ptr(bv), _ptr(wp),
                                                     _ptr(bp), _ptr(y), n, h, w, Cc, self._s()))
        return y

    def op_vq_out_tail(self, x_nhwc, norm_w, norm_b, w_oihw, bias, mode="raw", mean=None, std=None, fused=True, cout=None):
        """The decoder's tail conv_out(swish(norm_out(x))) -> NCHW [n, cout, H, W]: mode 'raw' fp32, 'denorm' (x std + mean, clamped to [0, 1]) or 'u8' (round(255 x) of that);
        fused=False: the three-kernel form.  cout=None: the export with three output channels; a number: bevgen_op_vq_out_tail_ex with w_oihw [cout, C, 3, 3] (3 and 7 have
        the fused kernel, every other count runs as three kernels; 'denorm' / 'u8' need 3)."""
        n, H, W, Cc = x_nhwc.shape
        out_mode = {"raw": _lib.VQ_OUT_RAW, "denorm": _lib.VQ_OUT_DENORM, "u8": _lib.VQ_OUT_U8}[mode]
        if cout is not None and (w_oihw.shape[0] != cout or (bias is not None and bias.numel() != cout)):
            raise ValueError(f"op_vq_out_tail: weight {tuple(w_oihw.shape)} / bias do not have cout = {cout} output channels")
        out = torch.empty((n, 3 if cout is None else int(cout), H, W), dtype=torch.uint8 if mode == "u8" else torch.float32, device=self.device)
        args = (self._h, _ptr(x_nhwc), _ptr(norm_w), _ptr(norm_b), _ptr(w_oihw), _ptr(bias), _ptr(mean), _ptr(std), out_mode, int(not fused), _ptr(out), n, H, W, Cc)
        if cout is None:
            self._check(self.lib.bevgen_op_vq_out_tail(*args, self._s()))
        else:
            self._check(self.lib.bevgen_op_vq_out_tail_ex(*args, int(cout), self._s()))
        return out

    def op_bce_logits(self, logits, target, qloss=None, codebook_weight=1.0):
        """out [2] fp32 on the device: out[0] = F.binary_cross_entropy_with_logits(logits, target) (mean; fp32 per element, double sum in a fixed order) and, with qloss
        (a one-element device tensor), out[1] = out[0] + codebook_weight * qloss in fp32; without qloss out[1] is left as allocated (NaN here)."""
        if logits.shape != target.shape:
            raise ValueError(f"op_bce_logits: logits {tuple(logits.shape)} and target {tuple(target.shape)} differ in shape")
        out = torch.full((2,), float("nan"), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_bce_logits(self._h, _ptr(logits), _ptr(target), logits.numel(), _ptr(qloss), float(codebook_weight), _ptr(out), self._s()))
        return out

    def op_seg_colorize(self, x, colorize, threshold=False):
        """VQModel.to_rgb: x [n, C, H, W] (C <= 32), colorize [3, C] -> [n, 3, H, W] = the projection, min-max normalised over the whole tensor; threshold: of (x > 0)
        instead of x, which stands for torch.round(torch.sigmoid(x)) (include/bevgen_hip.h names the one interval where the two differ)."""
        n, Cc, H, W = x.shape
        if colorize.numel() != 3 * Cc:
            raise ValueError(f"op_seg_colorize: colorize {tuple(colorize.shape)} does not project {Cc} channels to 3")
        rgb = torch.empty((n, 3, H, W), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_seg_colorize(self._h, _ptr(x), _ptr(colorize), int(bool(threshold)), _ptr(rgb), n, Cc, H, W, self._s()))
        return rgb

    # image metrics (csrc/metrics.hip; bevgen_amd/metrics.py builds PSNR / SSIM on them): a, b [n, C, H, W] on this context's device, both fp32 (values in [0, 1]) or both
    # uint8 (v / 255); results stay on the device.  The workspace is a tensor of this call, sized by the library's pure function.
    _METRIC_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.uint8: _lib.DTYPE_U8, torch.int64: _lib.DTYPE_I64, torch.float64: _lib.DTYPE_F64}

    def _metric_args(self, name, a, b, kernel_size=0):
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError(f"{name}: preds {tuple(a.shape)} {a.dtype} and target {tuple(b.shape)} {b.dtype} differ in shape or dtype")
        if a.dim() != 4:
            raise ValueError(f"{name}: images are [n, C, H, W], got {tuple(a.shape)}")
        a, b = _req(a, a.dtype, self.device, "preds"), _req(b, b.dtype, self.device, "target")
        n, Cc, H, W = a.shape
        dt = self._METRIC_DTYPES.get(a.dtype, -1)   # (any other number: the library refuses the dtype)
        nbytes = self.lib.bevgen_metrics_workspace_bytes(0 if name == "op_image_sqerr" else 1, n, Cc, H, W, int(kernel_size))
        work = torch.empty((max(int(nbytes), 8) // 8,), dtype=torch.float64, device=self.device)
        return a, b, dt, (n, Cc, H, W), work

    def op_image_sqerr(self, a, b, minmax=None):
        """(sse [n] float64, minmax [2] float32): sse[i] = sum (a - b)^2 over image i (fp32: one fp32 subtraction and product per element, double sum in a fixed order;
        uint8: the exact integer sum, in units of 1 / 255^2); minmax = (min, max) of the target b (uint8: of v / 255) merged INTO the buffer passed in (default: a fresh
        (+inf, -inf)), which is how PeakSignalNoiseRatio(data_range=None) follows the range over many updates."""
        a, b, dt, (n, Cc, H, W), work = self._metric_args("op_image_sqerr", a, b)
        sse = torch.empty((n,), dtype=torch.float64, device=self.device)
        if minmax is None:
            minmax = torch.tensor([float("inf"), float("-inf")], dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_image_sqerr(self._h, _ptr(a), _ptr(b), dt, n, Cc, H, W, _ptr(sse), _ptr(minmax), _ptr(work), self._s()))
        return sse, minmax

    def op_ssim(self, a, b, kernel_size=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, return_map=False):
        """sums [n] float64 = per-image sum of the SSIM map [n, C, H - k + 1, W - k + 1] (Gaussian window over the valid positions, no clamp; second moments about a
        per-tile shift, include/bevgen_hip.h); return_map: (sums, map fp32)."""
        a, b, dt, (n, Cc, H, W), work = self._metric_args("op_ssim", a, b, kernel_size)
        k = int(kernel_size)
        sums = torch.empty((max(n, 1),), dtype=torch.float64, device=self.device)[:n]
        smap = torch.empty((n, Cc, max(H - k + 1, 0), max(W - k + 1, 0)), dtype=torch.float32, device=self.device) if return_map else None
        self._check(self.lib.bevgen_op_ssim(self._h, _ptr(a), _ptr(b), dt, n, Cc, H, W, k, float(sigma), float(data_range), float(k1), float(k2), _ptr(sums), _ptr(smap),
                                            _ptr(work), self._s()))
        return (sums, smap) if return_map else sums

    # the stage-1 BEV segmentation model's loss and visualisation (modules/losses/segmentation.py, VQSegmentationModel.log_images): tensors are brought to this context's
    # device as fp32; results stay on the device
    def bce_logits(self, pred, target, qloss=None, codebook_weight=1.0, check=True):
        """(bce, total): 0-dim device tensors; total = bce + codebook_weight * qloss (fp32, as torch evaluates it), or None without qloss."""
        pred, target = _req(pred, torch.float32, self.device, "pred"), _req(target, torch.float32, self.device, "target")
        if qloss is not None:
            qloss = _req(qloss, torch.float32, self.device, "qloss").reshape(-1)
            if qloss.numel() != 1:
                raise ValueError("bce_logits: qloss is one number (the quantizer's loss)")
        out = self.op_bce_logits(pred, target, qloss, codebook_weight)
        self._done(check)
        return out[0], (out[1] if qloss is not None else None)

    def seg_to_rgb(self, x, colorize, threshold=False, check=True):
        """to_rgb(x) (threshold=False) or to_rgb(round(sigmoid(x))) (threshold=True) with the model's `colorize` buffer [3, C, 1, 1]: [n, C, H, W] -> [n, 3, H, W] in [0, 1]."""
        x = _req(x, torch.float32, self.device, "x")
        colorize = _req(colorize, torch.float32, self.device, "colorize").reshape(3, -1)
        rgb = self.op_seg_colorize(x, colorize, threshold)
        self._done(check)
        return rgb

    def op_vq_quantize(self, z, codebook, want_norms=False):
        """ids [rows] = argmin_j |z - e_j|^2 as the quantizer forms it ((|z|^2 + |e_j|^2) - 2 z.e_j, lowest index on ties); want_norms: also (|z|^2 [rows], |e|^2 [n_e])."""
        rows, D = z.shape
        n_e = codebook.shape[0]
        ids = torch.empty((rows,), dtype=torch.int64, device=self.device)
        zz = torch.empty((rows,), dtype=torch.float32, device=self.device) if want_norms else None
        ee = torch.empty((n_e,), dtype=torch.float32, device=self.device) if want_norms else None
        self._check(self.lib.bevgen_op_vq_quantize(self._h, _ptr(z), _ptr(codebook), _ptr(ids), _ptr(zz), _ptr(ee), rows, n_e, D, self._s()))
        return (ids, zz, ee) if want_norms else ids

    def op_vq_geo_embed(self, h, I_inv, E_inv, plane, wimg, wcam):
        """h [n, T, D] (in place) += normalize(wimg d - wcam c) per latent pixel: I_inv [n, 3, 3], E_inv [n, 4, 4], plane [3, T], wimg / wcam [D, 4]; D % 32 == 0."""
        n, T, D = h.shape
        self._check(self.lib.bevgen_op_vq_geo_embed(self._h, _ptr(h), _ptr(I_inv), _ptr(E_inv), _ptr(plane), _ptr(wimg), _ptr(wcam), n, T, D, self._s()))

    def op_vq_quant_error(self, z, codebook, ids, beta=0.25, want_loss=True):
        """(row_err [rows] = |codebook[ids] - z|^2, loss 0-dim = (1 + beta) / (rows D) sum(row_err) in a fixed order, or None): z [rows, D], codebook [n_e, D], ids [rows]."""
        rows, D = z.shape
        n_e = codebook.shape[0]
        row_err = torch.empty((rows,), dtype=torch.float32, device=self.device)
        loss = torch.empty((), dtype=torch.float32, device=self.device) if want_loss else None
        self._check(self.lib.bevgen_op_vq_quant_error(self._h, _ptr(z), _ptr(codebook), _ptr(ids), float(beta), _ptr(row_err), _ptr(loss), rows, n_e, D, self._s()))
        return row_err, loss

    def op_conv_ranged(self, x_nhwc, w_oihw, bias, kind, check=True):
        """precision='f16x3' / 'f16x3r' contexts: one site of the range-safe mode as vq_decode / vq_encode run it -> (y, e): e (a one-element int32 tensor) is the exponent
        of x (0 where max |x| < 32768, else the smallest e with max |x| 2^-e < 32768), y = 2^e conv(x 2^-e) + bias.  kind 0: 1x1 ([n, H, W, Cout]), 1: 3x3 stride 1
        padding 1, 2: the encoder's Downsample ([n, H / 2, W / 2, Cout]; H, W even).  Cin % 32 == 0; NaN / inf in x raise BevgenError (ERR_NUMERIC)."""
        x = _req(x_nhwc, torch.float32, self.device, "x")
        n, H, W, Cin = x.shape
        Cout = w_oihw.shape[0]
        y = torch.empty((n, H // 2, W // 2, Cout) if kind == 2 else (n, H, W, Cout), dtype=torch.float32, device=self.device)
        e = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._check(self.lib.bevgen_op_conv_ranged(self._h, _ptr(x), _ptr(w_oihw), _ptr(bias), int(kind), _ptr(y), _ptr(e), n, H, W, Cin, Cout, self._s()))
        self._done(check)
        return y, e

    def op_conv3x3_gn_stats(self, x_nhwc, w_oihw, bias, range_route=False):
        """precision='f16x3': the LDS-DMA 3x3 convolution whose epilogue leaves the GroupNorm partial sums of its output -> (y [n, H, W, Cout], partials
        [n H W / 32, Cout / 4, 2], stats [n, 32, 2] = (mean, rstd)); range_route: the bias + statistics pass of the range-safe mode (exponent 0) instead of the epilogue."""
        n, H, W, Cin = x_nhwc.shape
        Cout = w_oihw.shape[0]
        y = torch.empty((n, H, W, Cout), dtype=torch.float32, device=self.device)
        part = torch.zeros((max(n * H * W // 32, 1), max(Cout // 4, 1), 2), dtype=torch.float32, device=self.device)
        stats = torch.zeros((n, 32, 2), dtype=torch.float32, device=self.device)
        self._check(self.lib.bevgen_op_conv3x3_gn_stats(self._h, _ptr(x_nhwc), _ptr(w_oihw), _ptr(bias), int(range_route), _ptr(y), _ptr(part), _ptr(stats), n, H, W, Cin, Cout,
                                                        self._s()))
        return y, part, stats

    # the kernels around the layer stacks (embed.hip, tables.hip, attention.hip's tile lists): every output is a caller-owned tensor the library never clears, so a test
    # can surround it with guards and fill it with a sentinel; all tensors are handed over as they are (contiguous, on this context's device)
    def op_camera_embed(self, I_inv, E_inv, plane, wimg, wcam, img, c_embed):
        """img [B, C, T, D] and c_embed [B, C, D] (written in place) of I_inv [B, C, 3, 3], E_inv [B, C, 4, 4], plane [3, T], wimg / wcam [D, 4]."""
        B, C, T, D = img.shape
        self._check(self.lib.bevgen_op_camera_embed(self._h, _ptr(I_inv), _ptr(E_inv), _ptr(plane), _ptr(wimg), _ptr(wcam), _ptr(img), _ptr(c_embed), B, C, T, D, self._s()))

    def op_cond_embed(self, cond_ids, cond_tok, cond_pos, out, *, bev_grid=None, wbev=None, bbev=None, bev_cam_pos=None, c_embed=None, C=0):
        """out [B, K, D] (in place) = (cond_tok[clamp(id)] + bev term) + cond_pos; the bev term only with bev_grid [2+, K] (then wbev [D, 2], bbev [D], bev_cam_pos [C, K, D],
        c_embed [B, C, D])."""
        B, K, D = out.shape
        C = bev_cam_pos.shape[0] if bev_cam_pos is not None else int(C)
        self._check(self.lib.bevgen_op_cond_embed(self._h, _ptr(cond_ids), _ptr(cond_tok), _ptr(cond_pos), _ptr(bev_grid), _ptr(wbev), _ptr(bbev), _ptr(bev_cam_pos),
                                                  _ptr(c_embed), _ptr(out), B, C, K, D, cond_tok.shape[0], self._s()))

    TOKEN_ROW_KINDS = {"token_embed": 0, "ar_step_embed": 1, "ar_seq_embed": 2, "gather_rows": 3, "store_tokens": 4}

    def op_token_rows(self, kind, out, *, ids=None, table=None, img=None, pos=None, fwd_idx=None, step=None, B, N=0, D=0, vocab_rows=0, C_=0, T=0, n_steps=0, rows_per_seq=0,
                      row0=0):
        """One of the row kernels in TOKEN_ROW_KINDS (include/bevgen_hip.h bevgen_op_token_rows) writing into `out` in place."""
        self._check(self.lib.bevgen_op_token_rows(self._h, self.TOKEN_ROW_KINDS[kind], _ptr(ids), _ptr(table), _ptr(img), _ptr(pos), _ptr(fwd_idx), _ptr(step), _ptr(out), int(B),
                                                  int(N), int(D), int(vocab_rows), int(C_), int(T), int(n_steps), int(rows_per_seq), int(row0), self._s()))

    def op_muse_qkv_prep_f32(self, *, B, H, qraw=None, kvraw=None, null_kv=None, q_scale=None, k_scale=None, q=None, k=None, v=None, Nq=0, Nk=0, Nk_pad=0):
        """The fp32 Route M preparation: q [B, H, Nq, 64] from qraw [B Nq, 64 H]; k / v [B, H, Nk_pad, 64] rows [0, Nk] from null_kv [2, H, 64] and kvraw [B Nk, 128 H]."""
        self._check(self.lib.bevgen_op_muse_qkv_prep_f32(self._h, _ptr(qraw), _ptr(kvraw), _ptr(null_kv), _ptr(q_scale), _ptr(k_scale), _ptr(q), _ptr(k), _ptr(v), int(B), int(H),
                                                         int(Nq), int(Nk), int(Nk_pad), self._s()))

    def op_kv_cache_write(self, kind, kcache, vcache, *, kv_dtype, B, H, Lmax, qkv=None, q=None, n=1, pos0=0, pos=None, layers=1, rows=0, src=0, dst0=0, count=0):
        """kind 'scatter' | 'append' | 'replicate_prefix' on caches [(layers,) B, H, Lmax, 64] of kv_dtype 0 (fp32) / 1 (fp16) / 2 (int8: flat uint8 buffers of 68 B H Lmax bytes per layer); `pos`: the device int32 position of append."""
        k = {"scatter": 0, "append": 1, "replicate_prefix": 2}[kind]
        self._check(self.lib.bevgen_op_kv_cache_write(self._h, k, _ptr(qkv), _ptr(q), _ptr(kcache), _ptr(vcache), int(kv_dtype), int(B), int(H), int(n), int(pos0), _ptr(pos),
                                                      int(Lmax), int(layers), int(rows), int(src), int(dst0), int(count), self._s()))

    ATTN_TABLE_KINDS = {"attn_bias": 0, "muse_bias": 1, "allowed": 2, "layout": 3, "masked_bias": 4, "attn_tiles": 5}

    def op_attn_tables(self, kind, out0, out1=None, *, in0=None, in1=None, in2=None, heads=1, L=0, rows=0, cols=0, blk=1, ld0=0, ld1=0, hs0=0, hs1=0, scale=1.0):
        """One of the table builders in ATTN_TABLE_KINDS writing into out0 / out1 in place; the meaning of the operands per kind: include/bevgen_hip.h bevgen_op_attn_tables."""
        self._check(self.lib.bevgen_op_attn_tables(self._h, self.ATTN_TABLE_KINDS[kind], _ptr(in0), _ptr(in1), _ptr(in2), _ptr(out0), _ptr(out1), int(heads), int(L), int(rows),
                                                   int(cols), int(blk), int(ld0), int(ld1), int(hs0), int(hs1), float(scale), self._s()))

    def op_attention_tiles(self, q, k, v, bias, out, *, scale, residual=None, kv_group=1, use_tiles=True, out_layout=0):
        """Flash attention with a per-head masked bias [H, Nq, ld] and (use_tiles) the key-tile lists built from it; q [B, H, Nq, 64], k / v [B / kv_group, H, Nk_pad, 64];
        out (in place) [B, Nq, 64 H] (out_layout 0) or [B, H, Nq, 64] (1), residual in the same layout."""
        B, H, Nq, _ = q.shape
        self._check(self.lib.bevgen_op_attention_tiles(self._h, _ptr(q), _ptr(k), _ptr(v), _ptr(bias), bias.shape[-1], _ptr(residual), B, H, Nq, k.shape[2], float(scale),
                                                       int(kv_group), int(use_tiles), int(out_layout), _ptr(out), self._s()))
