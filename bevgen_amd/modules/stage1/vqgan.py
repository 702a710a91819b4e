"""Drop-in for multi_view_generation/modules/stage1/vqgan.py (+ the parts of quantize.py / model.py it instantiates).

  VQModel                 stage1/vqgan.py:31-213     (``_target_`` at configs/model/stage_2.yaml:36)
  VQSegmentationModel     stage1/vqgan.py:216-261    (``_target_`` at configs/model/stage_2.yaml:59)
  VectorQuantizer2        stage1/quantize.py:213-329 (``quantize`` attribute; ``get_codebook_entry`` is the decode-side entry)

Parameters carry the reference's ``state_dict`` names (encoder.*, decoder.*, quantize.embedding.weight, quant_conv.*, post_quant_conv.*).
``decode`` runs the hand-written HIP decoder (bevgen_vq_decode / bevgen_vq_decode_latents); ``encode`` (the step BEFORE the path)
runs the HIP encoder + arg-min quantizer (bevgen_vq_encode / bevgen_vq_encode_ex: the geometric embedding of ``geometric_embedding=True`` and the codebook loss);
``forward`` / ``log_images`` are the stage-1 reconstruction (encode, then decode).  ``VQSegmentationModel`` (the stage-1 BEV model, configs/model/stage_1_bev.yaml) adds
``validation_step`` / ``test_step`` with the loss kept in ``self.loss`` (modules/losses/segmentation.py) and its own ``log_images`` through ``to_rgb`` (bevgen_op_seg_colorize).
"""
from __future__ import annotations

from typing import Mapping, Optional

import torch
import torch.nn as nn

from ... import weights as W
from ...runtime import Context
from ..options import RuntimeOptionsMixin
from ..params import ParamNode, build_tree, module_device


DENORM_MEAN, DENORM_STD = (0.4265, 0.4489, 0.4769), (0.2053, 0.2206, 0.2578)   # bev_utils/util.py:99-100


def denormalize_tensor(x: torch.Tensor) -> torch.Tensor:
    """bev_utils/util.py:97-118 (keep_tensor=True): per-channel x*std+mean, clamp [0,1]; [n, 3, H, W]."""
    mean = torch.tensor(DENORM_MEAN, device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(DENORM_STD, device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    return torch.clamp(x * std + mean, 0, 1)


def image_plane(cam_latent_res, cam_res) -> torch.Tensor:
    """vqgan:20-28, 59-66 on the host: [1, 1, 3, h, w] with x = linspace(0, 1, w) * image_width, y = linspace(0, 1, h) * image_height, 1, where
    (h, w) = cam_latent_res and (image_height, image_width) = cam_res.  (The stage-2 transformers build their plane with the two sides of cam_res the other way round.)"""
    h, w = int(cam_latent_res[0]), int(cam_latent_res[1])
    image_height, image_width = cam_res
    plane = torch.ones(3, h, w)
    plane[0] = (torch.linspace(0, 1, w) * image_width)[None, :]
    plane[1] = (torch.linspace(0, 1, h) * image_height)[:, None]
    return plane[None, None]


def geometry_rows(m: torch.Tensor, k: int, n: int) -> torch.Tensor:
    """batch['intrinsics_inv'] (k = 3) / ['extrinsics_inv'] (k = 4) as one k x k matrix per image row: [B, cam, k, k] -> [(B cam), k, k]; [(B cam), k, k] stays."""
    if m.dim() not in (3, 4) or tuple(m.shape[-2:]) != (k, k):
        raise ValueError(f"geometry of shape {tuple(m.shape)}: expected [B, cam, {k}, {k}] or [(B cam), {k}, {k}]")
    m = m.reshape(-1, k, k)
    if m.shape[0] != n:
        raise ValueError(f"{m.shape[0]} {k}x{k} matrices for {n} images: the geometry has one matrix per (batch, camera) row of the input")
    return m.float()


class VectorQuantizer2(ParamNode):
    def __init__(self, n_e, e_dim, beta=0.25, remap=None, unknown_index="random", sane_index_shape=False, legacy=True):
        super().__init__()
        if remap is not None:
            raise NotImplementedError("index remapping is not used by any shipped configuration")
        self.n_e, self.e_dim, self.beta, self.legacy = n_e, e_dim, beta, legacy
        self.re_embed = n_e
        self.sane_index_shape = sane_index_shape

    def get_codebook_entry(self, indices, shape):
        """quant:314-329 - z_q = embedding(indices).view(b,h,w,c).permute(0,3,1,2) (API-compatible helper; the fused path is VQModel.decode_ids)."""
        z_q = self.embedding.weight[indices]
        if shape is not None:
            z_q = z_q.view(shape).permute(0, 3, 1, 2).contiguous()
        return z_q


class VQModel(RuntimeOptionsMixin, nn.Module):
    def __init__(self, ddconfig, lossconfig=None, n_embed=None, embed_dim=None, cam_res=None, cam_latent_res=None, cam_emd_dim=None,
                 geometric_embedding=False, ckpt_path=None, ignore_keys=(), image_key="image", colorize_nlabels=None, monitor=None, remap=None,
                 sane_index_shape=False, denormalize=True, legacy=True, **kwargs):
        super().__init__()
        self._ctx: Optional[Context] = None
        self._init_runtime_options(kwargs)    # precision / weights (bevgen_amd/modules/options.py)
        self.geometric_embedding = bool(geometric_embedding)
        self.ddconfig = dict(ddconfig)
        self.ddconfig["ch_mult"] = list(self.ddconfig["ch_mult"])
        self.ddconfig["attn_resolutions"] = list(self.ddconfig["attn_resolutions"])
        self.n_embed, self.embed_dim = n_embed, embed_dim
        # the networks are fully convolutional: cam_res / cam_latent_res only fix the default latent grid of decode_ids (nuScenes: 224 x 400 -> 14 x 25)
        self.cam_res = tuple(cam_res) if cam_res is not None else None
        self.cam_latent_res = tuple(cam_latent_res) if cam_latent_res is not None else None
        self.image_key = image_key
        self.denormalize = denormalize
        # vqgan:57.  The loss classes of this package hold no parameters (the state_dict does not move) and run on this model's device context
        self.loss = lossconfig
        if hasattr(lossconfig, "bind"):
            lossconfig.bind(self)
        self.quantize = VectorQuantizer2(n_embed, embed_dim, beta=0.25, remap=remap, sane_index_shape=sane_index_shape, legacy=legacy)
        if self.geometric_embedding:
            # vqgan:59-69.  img_embed / cam_embed map 4 -> cam_emd_dim channels and their output is added to the encoder's z_channels (`h_flat += img_embed`, vqgan:111)
            if cam_emd_dim != self.ddconfig["z_channels"]:
                raise ValueError(f"geometric_embedding=True needs cam_emd_dim == ddconfig['z_channels'] (got {cam_emd_dim} and {self.ddconfig['z_channels']}): "
                                 "the embedding is added to the encoder output")
            if self.cam_res is None or self.cam_latent_res is None:
                raise ValueError("geometric_embedding=True needs cam_res and cam_latent_res (the image plane is built from them)")
            self.register_buffer("image_plane", image_plane(self.cam_latent_res, self.cam_res), persistent=False)
        shapes = W.vqmodel_shapes(self.ddconfig, n_embed, embed_dim, with_encoder=True, geometric=self.geometric_embedding)
        build_tree(self, shapes)
        # children in the order the reference constructor creates them (encoder, decoder, [img_embed, cam_embed,] quantize, quant_conv, post_quant_conv): state_dict order
        order = list(dict.fromkeys(k.split(".")[0] for k in shapes))
        mods = dict(self._modules)
        self._modules.clear()
        for name in order + [m for m in mods if m not in order]:
            self._modules[name] = mods[name]
        for name, p in self.named_parameters():
            if p.dim() >= 2:
                nn.init.kaiming_uniform_(p, a=5 ** 0.5)
            elif name.endswith("weight"):
                p.data.fill_(1.0)
        if ckpt_path is not None:
            from ...checkpoint import init_from_ckpt

            init_from_ckpt(self, ckpt_path, ignore_keys=list(ignore_keys), strict=False)

    # ---------------------------------------------------------------------------------- copies (copy.deepcopy, pickle, torch.save of the module)
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_ctx"] = None            # the device context belongs to this object: a copy builds its own on first use
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        if hasattr(self.loss, "bind"):  # the copied loss runs on the COPY's context
            self.loss.bind(self)

    # ---------------------------------------------------------------------------------- device context
    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self.invalidate()
        return out

    def invalidate(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def context(self) -> Context:
        if self._ctx is None:
            dev = module_device(self)
            if dev.type != "cuda":
                raise RuntimeError("VQModel must live on a ROCm device before decode(); libbevgen_hip has no CPU path")
            ctx = Context(None, vq_ddconfig=self.ddconfig, vq_n_embed=self.n_embed, vq_embed_dim=self.embed_dim,
                          device=dev.index if dev.index is not None else torch.cuda.current_device(), **self.runtime_options("vq"))
            sd = {k: v for k, v in self.state_dict().items() if k != "colorize"}
            ctx.load_state_dict(sd, prefix="first_stage_model.")
            ctx.finalize()
            self._ctx = ctx
        return self._ctx

    # ---------------------------------------------------------------------------------- reference API
    @torch.no_grad()
    def decode(self, quant):
        """vqgan:118-121 - post_quant_conv + Decoder on looked-up latents [n, embed_dim, h, w] -> [n, out_ch, H, W]."""
        return self.context().vq_decode_latents(quant, denormalize=False)

    @torch.no_grad()
    def decode_ids(self, ids, denormalize=False, latent_hw=None):
        """Fused get_codebook_entry + decode (+ util.denormalize_tensor): ids [n, h*w] -> pixels; latent grid = latent_hw, else cam_latent_res, else square."""
        return self.context().vq_decode(ids, denormalize=denormalize, latent_hw=latent_hw or self.cam_latent_res)

    def decode_code(self, code_b):
        return self.decode_ids(code_b.reshape(code_b.shape[0], -1))

    def _geometry(self, x, batch):
        """geometric_embedding=True: (I_inv [n, 3, 3], E_inv [n, 4, 4], plane [3, h*w]) for the n rows of x out of batch['intrinsics_inv'] / ['extrinsics_inv']
        ([B, cam, ., .] as vqgan:90-91 rearranges them, or already [(B cam), ., .]); else three Nones (the batch is ignored, as in the reference)."""
        if not self.geometric_embedding:
            return None, None, None
        if batch is None or "intrinsics_inv" not in batch or "extrinsics_inv" not in batch:
            raise ValueError("VQModel(geometric_embedding=True).encode needs batch['intrinsics_inv'] and batch['extrinsics_inv']")
        n = x.shape[0]
        I_inv, E_inv = geometry_rows(batch["intrinsics_inv"], 3, n), geometry_rows(batch["extrinsics_inv"], 4, n)
        f = 2 ** (len(self.ddconfig["ch_mult"]) - 1)
        if (x.shape[-2] // f, x.shape[-1] // f) != tuple(self.image_plane.shape[-2:]):
            raise ValueError(f"input {tuple(x.shape[-2:])} does not give the latent grid {tuple(self.image_plane.shape[-2:])} of the image plane (cam_latent_res)")
        return I_inv, E_inv, self.image_plane.reshape(3, -1)

    @torch.no_grad()
    def encode_ids(self, x, batch=None):
        """Encoder (-> + geometric embedding) -> quant_conv -> arg-min over the codebook: x [n, in_channels, H, W] -> ids [n, h*w]."""
        if not self.geometric_embedding:
            return self.context().vq_encode(x)
        geo = self._geometry(x, batch)
        return self.context().vq_encode_ex(x, *geo, want_loss=False)[0]

    @torch.no_grad()
    def encode(self, x, batch=None):
        """vqgan:84-116 -> (quant [n, e, h, w], emb_loss (0-dim, on the device), (None, None, indices [n*h*w])).  emb_loss is the forward value of the quantizer's loss
        (quant:290-295, the same number with legacy True and False).  quant holds the looked-up codebook rows z_q; the reference returns z + (z_q - z) (its
        straight-through estimator, quant:298), which differs from z_q by at most an ulp of z."""
        geo = self._geometry(x, batch)
        ids, _, emb_loss = self.context().vq_encode_ex(x, *geo, beta=self.quantize.beta)
        f = 2 ** (len(self.ddconfig["ch_mult"]) - 1)
        quant = self.quantize.get_codebook_entry(ids.reshape(-1), (x.shape[0], x.shape[-2] // f, x.shape[-1] // f, self.embed_dim))
        return quant, emb_loss, (None, None, ids.reshape(-1))

    @torch.no_grad()
    def forward(self, input, batch=None):
        """vqgan:128-131 -> (dec [n, out_ch, H, W], diff = emb_loss): encode, then the fused codebook lookup + decoder on the ids."""
        _, diff, info = self.encode(input, batch)
        f = 2 ** (len(self.ddconfig["ch_mult"]) - 1)
        dec = self.decode_ids(info[2].reshape(input.shape[0], -1), latent_hw=(input.shape[-2] // f, input.shape[-1] // f))
        return dec, diff

    def get_input(self, batch, k):
        """vqgan:133-143: channel-last batch[k] -> [n, C, H, W] float; [B, H, W] gains a channel, [B, cam, H, W, C] becomes (B cam) rows (the reference squeezes, which is
        that for B = 1)."""
        x = batch[k]
        if x.dim() == 3:
            x = x[..., None]
        elif x.dim() == 5:
            x = x.reshape(-1, *x.shape[2:])
        return x.permute(0, 3, 1, 2).contiguous().float()

    @torch.no_grad()
    def log_images(self, batch, **kwargs):
        """vqgan:177-199 -> {'inputs', 'reconstructions'} [n, 3, H, W], denormalised to [0, 1] when self.denormalize (the geometric model takes its geometry from
        `batch`, as forward does: the reference's own geometric branch unpacks three values from get_input and cannot run)."""
        x = self.get_input(batch, self.image_key).to(module_device(self))
        if x.shape[1] > 3:
            raise NotImplementedError("log_images of inputs with more than 3 channels goes through to_rgb (vqgan:201-213), which is visualisation only")
        xrec, _ = self(x, batch)
        if self.denormalize:
            x, xrec = denormalize_tensor(x), denormalize_tensor(xrec)
        return {"inputs": x, "reconstructions": xrec}


class VQSegmentationModel(VQModel):
    def __init__(self, n_labels, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.n_labels = n_labels
        self.register_buffer("colorize", torch.randn(3, n_labels, 1, 1))  # checkpoint key (vqgan:219); only used by visualisation

    def to_rgb(self, x, threshold=False):
        """vqgan:201-213: the random projection `colorize` of x [n, C, H, W], min-max normalised over the whole tensor (Context.seg_to_rgb); threshold: of
        round(sigmoid(x)), evaluated as x > 0 (include/bevgen_hip.h bevgen_op_seg_colorize)."""
        self._check_rgb(x.shape[1])
        return self.context().seg_to_rgb(x, self.colorize, threshold)

    def _check_rgb(self, channels):
        assert self.image_key == "segmentation", "to_rgb colours a segmentation (vqgan:202): image_key must be 'segmentation'"
        if channels == 12:
            raise NotImplementedError("12 channels are nuScenes' BEV layers, drawn by a third-party visualiser in the reference (vqgan:203-205)")
        if channels != self.colorize.shape[1]:
            raise ValueError(f"{channels} channels do not fit the colorize buffer {tuple(self.colorize.shape)} (n_labels)")

    @torch.no_grad()
    def log_images(self, batch, **kwargs):
        """vqgan:245-261 -> {'inputs', 'reconstructions'}.  More than 3 channels: to_rgb(x) and to_rgb(round(sigmoid(xrec))), [n, 3, H, W] in [0, 1]; otherwise the raw
        input and the raw reconstruction (this class does not denormalise: VQModel.log_images does, with the camera statistics)."""
        x = self.get_input(batch, self.image_key).to(module_device(self))
        if x.shape[1] > 3:
            self._check_rgb(x.shape[1])   # (before the forward: the refusals need no device)
        xrec, _ = self(x, batch)
        if x.shape[1] > 3:
            assert xrec.shape[1] > 3
            x, xrec = self.to_rgb(x), self.to_rgb(xrec, threshold=True)
        return {"inputs": x, "reconstructions": xrec}

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """vqgan:231-239: {'loss': aeloss} of self.loss(qloss, x, xrec, split='val'), plus the log_images dict on every tenth batch; the logged values go to
        log_dict where the object has one (a LightningModule does)."""
        if self.loss is None:
            raise RuntimeError("validation_step needs a loss: construct the model with lossconfig (modules/losses/segmentation.py BCELossWithQuant)")
        x = self.get_input(batch, self.image_key).to(module_device(self))
        xrec, qloss = self(x, batch)
        aeloss, log_dict_ae = self.loss(qloss, x, xrec, split="val")
        if hasattr(self, "log_dict"):
            self.log_dict(log_dict_ae, prog_bar=False, logger=True, on_step=True, on_epoch=True)
        ret = {"loss": aeloss}
        if batch_idx % 10 == 0:
            ret = {**ret, **self.log_images(batch)}
        return ret

    @torch.no_grad()
    def test_step(self, batch, batch_idx):
        return self.log_images(batch)
