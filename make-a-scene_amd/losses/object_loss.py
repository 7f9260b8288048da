"""Object-aware perceptual loss: the object term of the VQ-IMG objective ("object-aware vector quantisation", Make-A-Scene section 3.2).

The reference wrote this term but left it commented out (losses/loss_img.py: ``self.object_loss = self.perceptual_loss`` and the loop
in ``forward``).  Restated, for ``bbox_obj`` as the reference's ``collate_fn`` makes it (one list of integer [x_min, y_min, x_max, y_max]
boxes per image; a [B, K, 4] tensor is converted with ``int()`` as the collate does, which costs one synchronisation when the tensor
is on the GPU)::

    object_loss = 0
    for img, rec, boxes in zip(images, reconstructions, bbox_obj):
        used = [b for b in boxes if b[3] - b[1] >= 16 and b[2] - b[0] >= 16]
        object_loss += sum(LPIPS(crop(img, b)[None], crop(rec, b)[None]).mean() for b in used) / (len(used) + 1)

``crop`` is torchvision's: the part of a box outside the image is 0 (before LPIPS's ScalingLayer).  LPIPS runs in evaluation mode.
Two deliberate differences from the reference: a box with a side under 16 px is skipped and not counted (the
reference raises on it: VGG's fourth max-pool has no output), and the gradient reaches ``reconstructions`` only (``images`` is data).

``ObjectLoss`` is one autograd node on libmas_hip (``mas_hip.objects``): every crop of the batch goes through VGG16 at once on an
"atlas" of canvases -- thirteen convolution launches per direction for the whole batch instead of thirteen per crop."""
import torch.nn as nn


class ObjectLoss(nn.Module):
    """``ObjectLoss(lpips=None, dtype=None)(images, reconstructions, bbox_obj) -> scalar``.

    ``lpips``: an ``losses.lpips.LPIPS`` whose weights the term uses (the VQ-IMG loss passes its perceptual term's, as the reference
    intended); it is NOT registered as a child, so sharing it adds no ``state_dict`` keys.  ``None`` builds one with LPIPS's checkpoint
    rules (``MAS_LPIPS_CKPT`` / ``MAS_VGG16_CKPT``), owned by this module.  ``dtype``: the activations' precision; ``None`` follows
    ``mas_hip.ops.compute_dtype()`` (bf16 by default, fp32 in the parity mode).  ``last_values``: every used crop's LPIPS of the
    last call, in (image, box) order (None without used boxes).

    ``forward(images, reconstructions, atlas)`` with a ``mas_hip.objects.ObjectAtlas`` instead of the box lists is the same term at
    fixed capacity (``mas_hip.objects.object_loss_static``: the crops are the ones last written into the atlas; nothing is read on the
    host, so a graph can capture it).  ``last_values`` is then the atlas's ``max_cells`` slots, the unused ones 0."""

    def __init__(self, lpips=None, dtype=None):
        super().__init__()
        if lpips is None:
            from .lpips import LPIPS
            self.net = LPIPS().eval()
        else:
            object.__setattr__(self, "net", lpips)          # shared, not owned: no second copy of its keys in a parent's state_dict
        self.dtype = dtype
        self.last_values = None

    def forward(self, images, reconstructions, bbox_obj):
        from mas_hip import objects as O
        if isinstance(bbox_obj, O.ObjectAtlas):
            out = O.object_loss_static(self.net, images, reconstructions, bbox_obj, self.dtype)
            self.last_values = out[1:].detach()
            return out[0]
        out = O.object_loss(self.net, images, reconstructions, bbox_obj, self.dtype)
        if out is None:
            self.last_values = None
            return images.new_tensor(0.0)
        self.last_values = out[1:].detach()
        return out[0]
