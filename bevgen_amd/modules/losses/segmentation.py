"""Drop-in for multi_view_generation/modules/losses/segmentation.py: the losses of the stage-1 BEV segmentation model (VQSegmentationModel.validation_step, vqgan:231-239).

  BCELoss            segmentation.py:5-8     forward(prediction, target) -> (loss, {})
  BCELossWithQuant   segmentation.py:11-22   forward(qloss, target, prediction, split) -> (bce + codebook_weight * qloss, {split/total_loss, split/bce_loss, split/quant_loss})
  CELossWithQuant    segmentation.py:24-36   the same computation in the reference (its "TODO: Fix"): an alias

Forward values only: F.binary_cross_entropy_with_logits with mean reduction runs as bevgen_op_bce_logits (csrc/vqseg_kernels.hip: fp32 per element, double sum in a fixed
order) through the device context of the model that owns the loss (VQModel.__init__ binds its `lossconfig`); a loss nobody owns opens a model-less context on the
prediction's device.  No torch arithmetic, no CPU path: the returned losses are 0-dim tensors on the device.
"""
from __future__ import annotations

import weakref

import torch
import torch.nn as nn


class _DeviceLoss(nn.Module):
    def __init__(self):
        super().__init__()
        object.__setattr__(self, "_owner", None)   # weak reference to the owning model: not a submodule, not in the state_dict
        object.__setattr__(self, "_own_ctx", None)

    def bind(self, owner) -> None:
        """Called by the model that holds this loss: its context() runs the kernel."""
        object.__setattr__(self, "_owner", weakref.ref(owner))

    # a copy (copy.deepcopy, pickle, torch.save) carries neither the owner nor a context: the model that holds the copy binds it again (VQModel.__setstate__)
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_owner"] = state["_own_ctx"] = None
        return state

    def context(self, like: torch.Tensor):
        owner = self._owner() if self._owner is not None else None
        if owner is not None:
            return owner.context()
        if like.device.type != "cuda":
            raise RuntimeError("the segmentation losses run on a ROCm device (libbevgen_hip has no CPU path): move prediction and target to the device")
        if self._own_ctx is None or self._own_ctx.device != like.device:
            from ...runtime import Context

            if self._own_ctx is not None:
                self._own_ctx.close()
            object.__setattr__(self, "_own_ctx", Context(None, device=like.device.index if like.device.index is not None else torch.cuda.current_device()))
        return self._own_ctx

    def _bce(self, prediction, target, qloss=None, codebook_weight=1.0):
        if prediction.shape != target.shape:
            raise ValueError(f"prediction {tuple(prediction.shape)} and target {tuple(target.shape)} differ in shape")
        return self.context(prediction).bce_logits(prediction, target, qloss, codebook_weight)


class BCELoss(_DeviceLoss):
    @torch.no_grad()
    def forward(self, prediction, target):
        loss, _ = self._bce(prediction, target)
        return loss, {}


class BCELossWithQuant(_DeviceLoss):
    def __init__(self, codebook_weight=1.):
        super().__init__()
        self.codebook_weight = codebook_weight

    @torch.no_grad()
    def forward(self, qloss, target, prediction, split):
        bce_loss, loss = self._bce(prediction, target, qloss, self.codebook_weight)
        return loss, {"{}/total_loss".format(split): loss.clone(),
                      "{}/bce_loss".format(split): bce_loss,
                      "{}/quant_loss".format(split): qloss.detach().reshape(())}


CELossWithQuant = BCELossWithQuant
