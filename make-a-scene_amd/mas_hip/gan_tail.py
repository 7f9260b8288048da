"""The tail of the VQ-IMG objective (``losses.loss_img.VQLPIPSWithDiscriminator.forward`` behind ``hip_tail``) over csrc/gan_loss.hip:
three autograd nodes -- the L1 (+ perceptual mean) term, the PatchGAN logit terms, and the combine of the generator loss with its
adaptive weight -- that read nothing on the host: the discriminator's gate is evaluated on the device from an int64 global-step
scalar, so a whole training step captures into a graph (``mas_hip.graphs.GraphedGanStep``).

Every sum runs in a fixed order without atomics (include/mas_hip.h, "Tail of the VQ-IMG objective", states the scheme and its error
bound), so a step repeats bit for bit.  The functions named ``*_fwd`` / ``*_bwd`` are the bare kernel calls, as the tests drive them."""
from __future__ import annotations

import torch

from . import _DT, _ptr as _p, _require_cuda, _stream, check, constants, lib

NCHW, NHWC, RUN = constants["MAS_SEG_NCHW"], constants["MAS_SEG_NHWC"], constants["MAS_GAN_RUN"]


def _dense(x: torch.Tensor):
    """-> (x as the kernels read it, layout code): dense NCHW and dense channels_last memory are read in place, anything else is made
    dense NCHW first"""
    if x.is_contiguous():
        return x, NCHW
    if x.is_contiguous(memory_format=torch.channels_last):
        return x, NHWC
    return x.contiguous(), NCHW


def _check_images(images, rec, who):
    if images.dim() != 4 or tuple(images.shape) != tuple(rec.shape) or images.numel() == 0:
        raise ValueError(f"{who}: images and reconstructions must be equal, non-empty [N, C, H, W]; got {tuple(images.shape)} and {tuple(rec.shape)}")
    for t in (images, rec):
        _require_cuda(t, who)
        if t.dtype not in _DT:
            raise TypeError(f"{who}: float32 or bfloat16 images, got {t.dtype}")


def _scalar(t, who, name):
    """one fp32 on the device, 0-dim (a differentiable cast when the dtype differs)"""
    if t.numel() != 1:
        raise ValueError(f"{who}: {name} must hold one element, got shape {tuple(t.shape)}")
    _require_cuda(t, who)
    return t.float().reshape(())


def check_step(step, who):
    if not (isinstance(step, torch.Tensor) and step.is_cuda and step.dtype == torch.int64 and step.dim() == 0):
        raise TypeError(f"{who}: the global step must be a 0-dim int64 CUDA tensor")
    return step


# --------------------------------------------------------------------------- #
# kernel calls
# --------------------------------------------------------------------------- #
def l1_fwd(images, rec, perceptual=None, perceptual_weight=1.0):
    """-> fp32 [2]: {sum |rec - images|, sum / numel + perceptual_weight * mean(perceptual)}; images / rec dense NCHW or channels_last"""
    n, c, h, w = rec.shape
    blocks = lib().mas_gan_l1_blocks(n, c, h, w)
    check(min(blocks, 0), "gan_l1_blocks")
    (x, xl), (r, rl) = _dense(images), _dense(rec)
    partials = torch.empty(blocks, dtype=torch.float64, device=rec.device)
    out = torch.empty(2, dtype=torch.float32, device=rec.device)
    check(lib().mas_gan_l1_fwd(_p(x), _DT[x.dtype], xl, _p(r), _DT[r.dtype], rl, n, c, h, w, _p(partials), blocks, _stream()), "gan_l1_fwd")
    check(lib().mas_gan_l1_finalize(_p(partials), blocks, rec.numel(), _p(perceptual), 0 if perceptual is None else perceptual.numel(),
                                    float(perceptual_weight), _p(out), _stream()), "gan_l1_finalize")
    return out


def l1_bwd(images, rec, g, n_perceptual=0, perceptual_weight=1.0):
    """-> (d rec in rec's dtype and layout, d perceptual fp32 [n_perceptual] or None); ``g``: one fp32 on the device"""
    n, c, h, w = rec.shape
    (x, xl), (r, rl) = _dense(images), _dense(rec)
    drec = torch.empty_like(r)
    dp = torch.empty(n_perceptual, dtype=torch.float32, device=rec.device) if n_perceptual else None
    check(lib().mas_gan_l1_bwd(_p(x), _DT[x.dtype], xl, _p(r), _DT[r.dtype], rl, n, c, h, w, _p(g), _p(drec), _p(dp), n_perceptual,
                               float(perceptual_weight), _stream()), "gan_l1_bwd")
    return drec, dp


def logits_fwd(fake, real=None, step=None, disc_start=0, disc_factor=1.0):
    """-> fp32 [5]: {-mean(fake), mean(relu(1 - real)), mean(relu(1 + fake)), gate * 0.5 * (the two hinge means), gate}; fp32 contiguous logits"""
    out = torch.empty(5, dtype=torch.float32, device=fake.device)
    check(lib().mas_gan_logits_fwd(_p(fake), fake.numel(), _p(real), 0 if real is None else real.numel(), _p(step), int(disc_start),
                                   float(disc_factor), _p(out), _stream()), "gan_logits_fwd")
    return out


def logits_bwd(fake, real=None, g_gen=None, g_d=None, gate=None):
    """-> (d fake, d real or None) for the upstream gradients of out[0] (``g_gen``) and out[3] (``g_d``), each one fp32 on the device or None;
    ``gate``: the forward's ``out[4:]``"""
    dfake = torch.empty_like(fake)
    dreal = torch.empty_like(real) if real is not None and g_d is not None else None
    check(lib().mas_gan_logits_bwd(_p(fake), fake.numel(), _p(real), 0 if real is None else real.numel(), _p(g_gen), _p(g_d), _p(gate),
                                   _p(dfake), _p(dreal), _stream()), "gan_logits_bwd")
    return dfake, dreal


def combine_fwd(nll, g_loss, codebook, face, obj, nll_grads, g_grads, step, disc_start, disc_factor, disc_weight, codebook_weight, advance=False):
    """-> fp32 [4]: {loss, d_weight, d_weight * gate, gate}; advances ``step`` by one after reading it when ``advance``"""
    out = torch.empty(4, dtype=torch.float32, device=nll.device)
    check(lib().mas_gan_combine_fwd(_p(nll), _p(g_loss), _p(codebook), codebook.numel(), _p(face), _p(obj), _p(nll_grads), _p(g_grads),
                                    nll_grads.numel(), _p(step), int(disc_start), float(disc_factor), float(disc_weight), float(codebook_weight),
                                    int(bool(advance)), _p(out), _stream()), "gan_combine_fwd")
    return out


def combine_bwd(g, out, codebook_weight, n_codebook):
    """-> fp32 [3]: the gradients of {nll (and face, object), g_loss, each element of codebook_loss}"""
    grads = torch.empty(3, dtype=torch.float32, device=out.device)
    check(lib().mas_gan_combine_bwd(_p(g), _p(out), float(codebook_weight), int(n_codebook), _p(grads), _stream()), "gan_combine_bwd")
    return grads


# --------------------------------------------------------------------------- #
# autograd nodes
# --------------------------------------------------------------------------- #
class _Nll(torch.autograd.Function):
    """nll_loss = mean(|images - rec| + perceptual_weight * perceptual) of loss_img.py; the gradient goes to ``rec`` and ``perceptual``"""

    @staticmethod
    def forward(ctx, images, rec, perceptual, perceptual_weight):
        out = l1_fwd(images, rec, perceptual, perceptual_weight)
        ctx.save_for_backward(images, rec)
        ctx.cfg = (0 if perceptual is None else perceptual.numel(), None if perceptual is None else perceptual.shape, float(perceptual_weight))
        l1_sum = out[0]
        ctx.mark_non_differentiable(l1_sum)
        return out[1], l1_sum

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_sum):
        images, rec = ctx.saved_tensors
        n_p, p_shape, pw = ctx.cfg
        want_p = n_p and ctx.needs_input_grad[2]
        drec, dp = l1_bwd(images, rec, g.float().reshape(1), n_p if want_p else 0, pw)
        return None, drec, dp.view(p_shape) if want_p else None, None


def nll(images, rec, perceptual=None, perceptual_weight=1.0, return_sum=False):
    """``mean(|images - rec| + perceptual_weight * perceptual)`` with ``perceptual`` one fp32 value per image ([B, 1, 1, 1]) or None:
    the reference's ``nll_loss``, an fp32 scalar.  ``images`` is data; ``rec`` and ``perceptual`` get the gradient."""
    _check_images(images, rec, "gan_tail.nll")
    if images.requires_grad:
        raise ValueError("gan_tail.nll: the images are not differentiated; detach them")
    if perceptual is not None:
        if perceptual.numel() != rec.shape[0]:
            raise ValueError(f"gan_tail.nll: the perceptual term must hold one value per image ({rec.shape[0]}), got shape {tuple(perceptual.shape)}")
        perceptual = perceptual.float().contiguous()
    out, l1_sum = _Nll.apply(images, rec, perceptual, float(perceptual_weight))
    return (out, l1_sum) if return_sum else out


class _Logits(torch.autograd.Function):
    """outputs: the generator term -mean(fake), the gated hinge loss, and the two hinge means (not differentiable)"""

    @staticmethod
    def forward(ctx, fake, real, step, disc_start, disc_factor):
        out = logits_fwd(fake, real, step, disc_start, disc_factor)
        ctx.save_for_backward(fake, real, out)
        ctx.gated = step is not None
        ctx.set_materialize_grads(False)
        means = out[1:3]
        ctx.mark_non_differentiable(means)
        return out[0], out[3], means

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_gen, g_d, _g_means):
        fake, real, out = ctx.saved_tensors
        if not ctx.gated:
            g_d = None
        if g_gen is None and g_d is None:
            return None, None, None, None, None
        one = lambda g: None if g is None else g.float().reshape(1)
        dfake, dreal = logits_bwd(fake, real, one(g_gen), one(g_d), out[4:])
        return dfake, dreal, None, None, None


def _logits(t, who):
    _require_cuda(t, who)
    return t.float().contiguous()


def generator_term(logits_fake):
    """``-mean(logits_fake)``: the generator's PatchGAN term, an fp32 scalar"""
    return _Logits.apply(_logits(logits_fake, "gan_tail.generator_term"), None, None, 0, 0.0)[0]


def hinge_d_loss(logits_real, logits_fake, step, disc_start, disc_factor=1.0, return_means=False):
    """``gate * 0.5 * (mean(relu(1 - real)) + mean(relu(1 + fake)))`` with ``gate = disc_factor if step >= disc_start else 0`` evaluated
    on the device from ``step`` (0-dim int64): the discriminator's objective, an fp32 scalar"""
    check_step(step, "gan_tail.hinge_d_loss")
    _, d_loss, means = _Logits.apply(_logits(logits_fake, "gan_tail.hinge_d_loss"), _logits(logits_real, "gan_tail.hinge_d_loss"), step,
                                     int(disc_start), float(disc_factor))
    return (d_loss, means) if return_means else d_loss


class _Combine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nll_loss, g_loss, codebook, face, obj, nll_grads, g_grads, step, cfg):
        disc_start, disc_factor, disc_weight, codebook_weight, advance = cfg
        out = combine_fwd(nll_loss, g_loss, codebook, face, obj, nll_grads, g_grads, step, disc_start, disc_factor, disc_weight, codebook_weight,
                          advance)
        ctx.save_for_backward(out)
        ctx.cfg = (codebook_weight, codebook.shape, face is not None, obj is not None)
        terms = out[1:]
        ctx.mark_non_differentiable(terms)
        return out[0], terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_terms):
        (out,) = ctx.saved_tensors
        codebook_weight, cb_shape, has_face, has_obj = ctx.cfg
        n_cb = 1
        for s in cb_shape:
            n_cb *= s
        grads = combine_bwd(g.float().reshape(1), out, codebook_weight, n_cb)
        return (grads[0], grads[1], grads[2].expand(cb_shape), grads[0] if has_face else None, grads[0] if has_obj else None, None, None,
                None, None)


def combine(nll_loss, g_loss, codebook_loss, nll_grads, g_grads, step, *, disc_start, disc_factor=1.0, disc_weight=1.0, codebook_weight=1.0,
            face_loss=None, object_loss=None, advance=False):
    """The generator objective of loss_img.py:109-111 from its parts: with ``nll_grads`` / ``g_grads`` the gradients of ``nll_loss`` /
    ``g_loss`` at the decoder's last weight, ``d_weight = clamp(|nll_grads| / (|g_grads| + 1e-4), 0, 1e4) * disc_weight`` (a constant of
    the loss, as the reference's ``detach``), ``gate = disc_factor if step >= disc_start else 0`` on the device, and
    ``loss = nll_loss + d_weight * gate * g_loss + codebook_weight * mean(codebook_loss) + face_loss + object_loss``.
    -> ``(loss, terms)``, ``terms`` the detached fp32 ``[d_weight, d_weight * gate, gate]``.  ``advance``: ``step`` becomes ``step + 1``
    after the kernel has read it.  No gradient reaches ``nll_grads`` / ``g_grads``."""
    who = "gan_tail.combine"
    check_step(step, who)
    if nll_grads.shape != g_grads.shape or nll_grads.numel() == 0:
        raise ValueError(f"{who}: the two gradient tensors must have one non-empty shape, got {tuple(nll_grads.shape)} and {tuple(g_grads.shape)}")
    if codebook_loss.numel() == 0:
        raise ValueError(f"{who}: empty codebook_loss")
    _require_cuda(codebook_loss, who)
    opt = lambda t, name: None if t is None else _scalar(t, who, name)
    cfg = (int(disc_start), float(disc_factor), float(disc_weight), float(codebook_weight), bool(advance))
    return _Combine.apply(_scalar(nll_loss, who, "nll_loss"), _scalar(g_loss, who, "g_loss"), codebook_loss.float().contiguous(),
                          opt(face_loss, "face_loss"), opt(object_loss, "object_loss"), nll_grads.detach().float().contiguous(),
                          g_grads.detach().float().contiguous(), step, cfg)
