"""VQGAN image loss (reference losses/loss_img.py:11-141): L1 (+ perceptual) reconstruction, PatchGAN generator / hinge
discriminator terms, and the adaptive generator weight -- the ratio of two gradient norms at the decoder's last layer, each
obtained with ``torch.autograd.grad(..., retain_graph=True)`` THROUGH the HIP autograd nodes of the decoder (:56-66).

The discriminator runs on the MI355X kernels (``losses.discriminator``).  The two terms of the reference that need pretrained
networks at absolute paths -- LPIPS-VGG16 (``/home/ubuntu/.../vgg.pth``, lpips.py:15) and the face-embedding loss
(face_loss.py:76) -- are pluggable here.  ``perceptual_loss="lpips"`` (the DEFAULT, as the reference's constructor always builds
it, loss_img.py:45) is ``losses.lpips_with_object.LPIPSWithObject`` on the HIP convolutions (weights from ``MAS_LPIPS_CKPT`` /
``MAS_VGG16_CKPT``; missing weights are reported loudly by ``LPIPS.load_from_pretrained``); a callable is used as given; an
explicit ``None`` opts out.  ``face_loss``: the reference always builds ``FaceLoss()`` (loss_img.py:48), a pretrained
face-embedding network whose weights are not part of this repository.  The default here (``"reference"``) builds
``losses.face_loss.FaceLoss`` (HIP, evaluation mode) when its checkpoint exists (``MAS_FACE_CKPT``, or the reference's path);
otherwise it logs ONCE that the face term is absent from the objective and contributes 0.  A callable is used as given, ``None``
opts out silently.  ``object_loss``: the object-aware term the reference left commented out (loss_img.py:49,91-106).  ``None`` (the
default, as in the reference) keeps it a constant 0; ``"lpips"`` is ``losses.object_loss.ObjectLoss`` sharing the perceptual term's
LPIPS weights; a callable(images, reconstructions, bbox_obj) is used as given.  The arithmetic below is the reference's line for
line.  ``forward`` keeps the reference's signature and return shapes (optimizer_idx 0 -> ``loss, (nll_loss, object_loss,
face_loss)``; 1 -> ``d_loss``).

``hip_tail(True)`` / ``MAS_GAN_TAIL_HIP=1`` (off by default): what follows the networks -- the L1 term and its mean with the
perceptual term, the generator and hinge terms over the logits, the norm / ratio / clamp of the adaptive weight, the gate and the sum --
runs on csrc/gan_loss.hip as three autograd nodes (``mas_hip.gan_tail``), in fixed-order sums, and reads nothing on the host:
``global_step`` may then be a 0-dim int64 device tensor (the gate ``global_step >= disc_start`` is evaluated on the device), which is
what lets ``mas_hip.graphs.GraphedGanStep`` capture the whole step.  The two ``autograd.grad`` calls stay as they are.  On this path
``bbox_face`` may also be a ``mas_hip.face.FaceTable`` (a ``FaceLoss`` then runs its fixed-capacity node, which a capture can hold), and a
``FaceLoss`` with ``bbox_face=None`` -- a batch without faces -- is left out of the sum.  With the switch
off ``forward`` is the code below, unchanged, and a tensor ``global_step`` raises."""
import os
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from .discriminator import Discriminator, weights_init
from .face_loss import FaceLoss


_hip = {"on": os.environ.get("MAS_GAN_TAIL_HIP", "0") == "1"}      # read once


class hip_tail:
    """``hip_tail(on)`` switches the HIP tail of ``VQLPIPSWithDiscriminator.forward`` on or off for the process; used as
    ``with hip_tail(on):`` the previous setting comes back at the end of the block."""

    def __init__(self, on=True):
        self._before = _hip["on"]
        _hip["on"] = bool(on)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _hip["on"] = self._before
        return False


def hip_tail_enabled() -> bool:
    return _hip["on"]


def adopt_weight(weight, global_step, threshold=0, value=0.0):
    if global_step < threshold:
        weight = value
    return weight


def hinge_d_loss(logits_real, logits_fake):
    loss_real = torch.mean(F.relu(1.0 - logits_real))
    loss_fake = torch.mean(F.relu(1.0 + logits_fake))
    return 0.5 * (loss_real + loss_fake)


def vanilla_d_loss(logits_real, logits_fake):
    return 0.5 * (torch.mean(F.softplus(-logits_real)) + torch.mean(F.softplus(logits_fake)))


class VQLPIPSWithDiscriminator(nn.Module):
    _face_warned = False
    hip_tail = hip_tail                               # (mas_hip.graphs reaches the switch through the module it is handed)

    def __init__(self, disc_start, codebook_weight=1.0, pixelloss_weight=1.0, disc_factor=1.0, disc_weight=1.0, perceptual_weight=1.0,
                 perceptual_loss="lpips", face_loss="reference", object_loss=None):
        super().__init__()
        self.codebook_weight = codebook_weight
        self.pixel_weight = pixelloss_weight
        if perceptual_loss == "lpips":                 # the reference's default (loss_img.py:45)
            from .lpips_with_object import LPIPSWithObject
            perceptual_loss = LPIPSWithObject().eval()
        self.perceptual_loss = perceptual_loss        # callable(images, reconstructions, bbox_obj) -> per-sample map, or None
        self.perceptual_weight = perceptual_weight
        if isinstance(face_loss, str):
            if face_loss != "reference":
                raise ValueError("face_loss: a callable, None, or 'reference' (the default)")
            from .face_loss import ckpt_path
            if ckpt_path() is not None:
                face_loss = FaceLoss()
            else:
                if not VQLPIPSWithDiscriminator._face_warned:
                    VQLPIPSWithDiscriminator._face_warned = True
                    warnings.warn("VQLPIPSWithDiscriminator: the reference adds FaceLoss() (losses/face_loss.py: a pretrained face-embedding "
                                  "network whose weights are not part of this repository) to the generator objective; no checkpoint was "
                                  "found, so it is ABSENT here and contributes 0.  Set MAS_FACE_CKPT to the reference's "
                                  "face_loss_weights.pt to train with it -- or pass face_loss=<callable(images, reconstructions, "
                                  "bbox_face)> to supply another, face_loss=None to silence this message")
                face_loss = None
        self.face_loss = face_loss                    # callable(images, reconstructions, bbox_face) -> scalar, or None
        if isinstance(object_loss, str):
            if object_loss != "lpips":
                raise ValueError("object_loss: None (the default), 'lpips', or a callable")
            from .lpips import LPIPS
            from .object_loss import ObjectLoss
            # loss_img.py:49 of the reference: the object term shares the perceptual term's network
            object_loss = ObjectLoss(self.perceptual_loss if isinstance(self.perceptual_loss, LPIPS) else None)
        self.object_loss = object_loss                # callable(images, reconstructions, bbox_obj) -> scalar, or None
        self.discriminator = Discriminator().apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_factor = disc_factor
        self.discriminator_weight = disc_weight
        self.advance_global_step = False              # HIP tail, tensor global_step: the generator half adds 1 to it after reading it
        self.last_terms = None                        # HIP tail: the generator half's detached {"g_loss", "d_weight"}
        self._dev_scalars = {}                        # HIP tail: per device, the int64 step scalar an int is written to, and a zero

    def calculate_adaptive_weight(self, nll_loss, g_loss, last_layer):
        nll_grads = torch.autograd.grad(nll_loss, last_layer.weight, retain_graph=True)[0]
        g_grads = torch.autograd.grad(g_loss, last_layer.weight, retain_graph=True)[0]
        d_weight = torch.norm(nll_grads) / (torch.norm(g_grads) + 1e-4)
        d_weight = torch.clamp(d_weight, 0.0, 1e4).detach()
        return d_weight * self.discriminator_weight

    def forward(self, optimizer_idx, global_step, images, reconstructions, codebook_loss=None, bbox_obj=None, bbox_face=None,
                last_layer=None):
        if _hip["on"]:
            return self._forward_hip(optimizer_idx, global_step, images, reconstructions, codebook_loss, bbox_obj, bbox_face, last_layer)
        if isinstance(global_step, torch.Tensor):
            raise TypeError("VQLPIPSWithDiscriminator: a tensor global_step belongs to the HIP tail (losses.loss_img.hip_tail(True) / "
                            "MAS_GAN_TAIL_HIP=1); with the switch off the gate is a host comparison on a Python int")
        if optimizer_idx == 0:  # vqvae loss
            rec_loss = torch.abs(images.contiguous() - reconstructions.contiguous())
            if self.perceptual_loss is not None:
                rec_loss = rec_loss + self.perceptual_weight * self.perceptual_loss(images.contiguous(), reconstructions.contiguous(), bbox_obj)
            nll_loss = torch.mean(rec_loss)
            face_loss = self.face_loss(images, reconstructions, bbox_face) if self.face_loss is not None else images.new_tensor(0)
            if self.object_loss is not None:
                if bbox_obj is None:
                    raise ValueError("VQLPIPSWithDiscriminator: the object term needs bbox_obj (one list of boxes per image)")
                object_loss = self.object_loss(images, reconstructions, bbox_obj)
            else:
                object_loss = images.new_tensor(0)
            logits_fake = self.discriminator(reconstructions.contiguous())
            g_loss = -torch.mean(logits_fake)
            d_weight = self.calculate_adaptive_weight(nll_loss, g_loss, last_layer=last_layer)
            disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
            loss = nll_loss + d_weight * disc_factor * g_loss + self.codebook_weight * codebook_loss.mean() + face_loss + object_loss
            return loss, (nll_loss, object_loss, face_loss)
        if optimizer_idx == 1:  # gan loss
            disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
            logits_real = self.discriminator(images.contiguous().detach())
            logits_fake = self.discriminator(reconstructions.contiguous().detach())
            return disc_factor * hinge_d_loss(logits_real, logits_fake)

    # ---- the tail on csrc/gan_loss.hip (hip_tail / MAS_GAN_TAIL_HIP=1) ---------------------------------------------------------
    def _scalars(self, device):
        s = self._dev_scalars.get(device)
        if s is None:
            s = self._dev_scalars[device] = (torch.zeros((), dtype=torch.int64, device=device), torch.zeros((), dtype=torch.float32, device=device))
        return s

    def _forward_hip(self, optimizer_idx, global_step, images, reconstructions, codebook_loss, bbox_obj, bbox_face, last_layer):
        """the same objective with the L1 term, the logit terms, the adaptive weight, the gate and the sum on the kernels of
        ``mas_hip.gan_tail``: nothing is read on the host.  ``global_step``: a Python int (written to this module's device scalar) or a
        0-dim int64 tensor on the images' device, used as is."""
        from mas_hip import gan_tail as T
        step, zero = self._scalars(images.device)
        if isinstance(global_step, torch.Tensor):
            step = T.check_step(global_step, "VQLPIPSWithDiscriminator")
        else:
            step.fill_(int(global_step))
        if optimizer_idx == 0:  # vqvae loss
            p_loss = None
            if self.perceptual_loss is not None:
                p_loss = self.perceptual_loss(images.contiguous(), reconstructions.contiguous(), bbox_obj)
            nll_loss = T.nll(images, reconstructions, p_loss, self.perceptual_weight)
            # (a FaceLoss takes lists of boxes or a mas_hip.face.FaceTable; with bbox_face=None -- a batch without faces -- the term is
            # absent, as it is with face_loss=None.  Any other callable is handed what the caller gave.)
            face_loss = None
            if self.face_loss is not None and not (bbox_face is None and isinstance(self.face_loss, FaceLoss)):
                face_loss = self.face_loss(images, reconstructions, bbox_face)
            object_loss = None
            if self.object_loss is not None:
                if bbox_obj is None:
                    raise ValueError("VQLPIPSWithDiscriminator: the object term needs bbox_obj (one list of boxes per image)")
                object_loss = self.object_loss(images, reconstructions, bbox_obj)
            g_loss = T.generator_term(self.discriminator(reconstructions.contiguous()))
            nll_grads = torch.autograd.grad(nll_loss, last_layer.weight, retain_graph=True)[0]
            g_grads = torch.autograd.grad(g_loss, last_layer.weight, retain_graph=True)[0]
            loss, terms = T.combine(nll_loss, g_loss, codebook_loss, nll_grads, g_grads, step, disc_start=self.discriminator_iter_start,
                                    disc_factor=self.disc_factor, disc_weight=self.discriminator_weight, codebook_weight=self.codebook_weight,
                                    face_loss=face_loss, object_loss=object_loss,
                                    advance=self.advance_global_step and isinstance(global_step, torch.Tensor))
            self.last_terms = {"g_loss": g_loss.detach(), "d_weight": terms[0]}
            zero = zero.to(images.dtype)
            return loss, (nll_loss, zero if object_loss is None else object_loss, zero if face_loss is None else face_loss)
        if optimizer_idx == 1:  # gan loss
            logits_real = self.discriminator(images.contiguous().detach())
            logits_fake = self.discriminator(reconstructions.contiguous().detach())
            return T.hinge_d_loss(logits_real, logits_fake, step, self.discriminator_iter_start, self.disc_factor)
