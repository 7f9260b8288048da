"""The VQ-SEG stage's reconstruction losses behind the reference's names (reference losses/loss_seg.py:6-41; ``conf/seg_config.yaml``'s
``_target_: losses.VQVAEWithBCELoss``), restated here so that this package never needs a reference checkout at run time (until round 5
``losses/__init__.py`` fell through to the reference's own file).  Pinned against the reference: ``tests/golden/loss_seg.npz``
(``tests/golden/make_golden_r6.py`` runs the reference's classes), ``tests/test_losses_host.py``.

On the GPU the reconstruction terms are ``mas_hip.ops.seg_loss`` (csrc/seg_loss.hip): at [B, 159, 256, 256] the loss reads 10.4 M
elements per image, and the torch expression below walks them many times over and saves several tensors of that size for the backward;
the kernel reads prediction and target once each way, in place in whichever of NCHW / channels_last memory each has, and saves nothing.
CPU tensors, dtypes outside the op's envelope (prediction fp32 / bf16; target fp32 / bf16 / uint8 / bool) and ``MAS_SEG_LOSS=0`` run the
torch expression, exactly as before.

The target may also be a ``mas_hip.seglabels.SegLabels`` (the map as 4 label bytes per pixel): on the GPU the loss is then
``mas_hip.ops.seg_loss_labels`` (csrc/seg_labels.hip), which derives the target in registers, so that no dense target exists anywhere;
``MAS_SEG_LOSS=0``, CPU labels and predictions outside the op's envelope densify the labels and run the torch expression.

Both classes weigh the positive class of the five channels 153..157 twenty-fold (``pos_weight`` of the logits BCE; a persistent buffer
named ``weight``, so ``state_dict`` carries it as the reference's does) and add ``codebook_weight * qloss``;
``VQVAEWithBCELoss`` adds the mean squared error of the sigmoid as well."""
import os

import torch
import torch.nn.functional as F
from torch import nn

from mas_hip.seglabels import SegLabels

_HEAVY_CHANNELS = (153, 158)        # half-open channel range with positive weight 20
_HEAVY_WEIGHT = 20.0
_HIP_MAX_CHANNELS = 7679            # the kernels keep the weights, and for mixed layouts one pixel of targets, in LDS (include/mas_hip.h)


class _SegLossBase(nn.Module):
    def __init__(self, image_channels=159, codebook_weight=1.0):
        super().__init__()
        self.codebook_weight = codebook_weight
        w = torch.ones(image_channels)
        w[_HEAVY_CHANNELS[0]:_HEAVY_CHANNELS[1]] = _HEAVY_WEIGHT
        self.register_buffer("weight", w)

    def _hip(self, target, prediction):
        """the fused kernels take this call: GPU tensors of the op's dtypes, and the switch not thrown"""
        return (prediction.is_cuda and target.is_cuda and prediction.dim() == 4 and prediction.shape == target.shape
                and prediction.dtype in (torch.float32, torch.bfloat16)
                and target.dtype in (torch.float32, torch.bfloat16, torch.uint8, torch.bool) and not target.requires_grad
                and 0 < prediction.numel() and prediction.shape[1] <= _HIP_MAX_CHANNELS and os.environ.get("MAS_SEG_LOSS", "1") != "0")

    def _labels(self, target, prediction, mse):
        """-> the reconstruction terms for a ``SegLabels`` target, or None after which the caller runs the dense expression"""
        if target.shape[1] != self.weight.shape[0] or tuple(target.shape) != tuple(prediction.shape):
            raise ValueError(f"{type(self).__name__}: SegLabels of logical shape {tuple(target.shape)} ({target.layout}) against a prediction "
                             f"{tuple(prediction.shape)} and {self.weight.shape[0]} channel weights")
        if (prediction.is_cuda and target.is_cuda and prediction.dtype in (torch.float32, torch.bfloat16) and 0 < prediction.numel()
                and os.environ.get("MAS_SEG_LOSS", "1") != "0"):
            from mas_hip import ops
            return ops.seg_loss_labels(prediction, target, self.weight, mse=mse)
        return None

    @staticmethod
    def _densify(target, prediction):
        """CPU labels / ``MAS_SEG_LOSS=0``: the dense fp32 map, made where the labels are, beside the prediction"""
        return target.dense(torch.float32).to(prediction.device)

    def _bce(self, target, prediction):
        # channels last, so that the per-channel pos_weight broadcasts over (N, H, W)
        return F.binary_cross_entropy_with_logits(prediction.movedim(1, -1), target.movedim(1, -1), pos_weight=self.weight)


class BCELossWithQuant(_SegLossBase):
    def forward(self, qloss, target, prediction):
        if isinstance(target, SegLabels):
            rec = self._labels(target, prediction, False)
            if rec is not None:
                return rec + self.codebook_weight * qloss
            target = self._densify(target, prediction)
        if self._hip(target, prediction):
            from mas_hip import ops
            return ops.seg_loss(prediction, target, self.weight) + self.codebook_weight * qloss
        return self._bce(target, prediction) + self.codebook_weight * qloss


class VQVAEWithBCELoss(_SegLossBase):
    def forward(self, qloss, target, prediction):
        if isinstance(target, SegLabels):
            rec = self._labels(target, prediction, True)
            if rec is not None:
                return rec + self.codebook_weight * qloss
            target = self._densify(target, prediction)
        if self._hip(target, prediction):
            from mas_hip import ops
            return ops.seg_loss(prediction, target, self.weight, mse=True) + self.codebook_weight * qloss
        rec = F.mse_loss(torch.sigmoid(prediction), target) + self._bce(target, prediction)
        return rec + self.codebook_weight * qloss
