"""Whole-image LPIPS-VGG16 (losses/lpips.py:LPIPS.forward) as ONE autograd node over libmas_hip (csrc/lpips.hip + the convolution
dispatch): the perceptual term every VQ-IMG training step evaluates on the full images.

The torch expression runs VGG16 on ``cat([real, fake])`` and leaves ReLU, the pools and the distance head to elementwise and reduction
passes, with autograd driving the data gradient of all thirteen convolutions for all 2 B images although ``real`` needs none.  Here:
pack (ScalingLayer, cat, cast), 13 x (convolution, ReLU), 4 pools, 5 heads and one finalize forward; backward on the RECONSTRUCTION
half only -- per level the head's seed, the pool backward with the ReLU mask and the seed folded in, the convolutions' data gradients
with the ReLU masks between them, and the pack adjoint.  ``real`` gets no gradient.  Nothing reads the host.

These are ``mas_hip.objects``' kernels without the atlas; the convolution calls, the ReLU backward and the
weight handling are that module's own."""
from __future__ import annotations

import ctypes as C

import torch

from . import _DT, _image, _ptr as _p, _require_cuda, _stream, check, lib
from . import objects as O

LEVELS = O.LEVELS
CHANNELS = O.CHANNELS
CP = O.CP
MIN_SIDE = 16         # four 2x2 pools: a side under 16 px leaves the fifth level empty (torch raises there)


# --------------------------------------------------------------------------- #
# kernel calls
# --------------------------------------------------------------------------- #
def pack_fwd(real, fake, shift, scale, dtype):
    """[2 B, 8, H, W] (channels_last): (x - shift) / scale of real (first half) and fake (second half) in channels 0..2, zeros above"""
    b, _, h, w = real.shape
    out = O._nhwc(2 * b, CP, h, w, dtype, real.device)
    gr, gf = _image(real, "LPIPS"), _image(fake, "LPIPS")
    check(lib().mas_lpips_pack_fwd(C.byref(gr), C.byref(gf), _p(shift), _p(scale), _p(out), _DT[dtype], _stream()), "lpips_pack_fwd")
    return out


def pack_bwd(dcanvas, scale, like):
    """d ``like`` (its dtype and strides, written in full) from the rec-side canvas gradient [B, 8, H, W]"""
    dfake = torch.empty_like(like)
    g = _image(dfake, "LPIPS")
    check(lib().mas_lpips_pack_bwd(_p(dcanvas), _DT[dcanvas.dtype], _p(scale), C.byref(g), _stream()), "lpips_pack_bwd")
    return dfake


def relu_fwd(y):
    check(lib().mas_lpips_relu_fwd(_p(y), y.numel(), _DT[y.dtype], _stream()), "lpips_relu_fwd")
    return y


def pool_fwd(x):
    n, c, h, w = x.shape
    y = O._nhwc(n, c, h // 2, w // 2, x.dtype, x.device)
    check(lib().mas_lpips_pool_fwd(_p(x), _p(y), n, h, w, c, _DT[x.dtype], _stream()), "lpips_pool_fwd")
    return y


def pool_bwd(a, seed, dz):
    n, c, h, w = a.shape
    dy = torch.empty_like(a)
    check(lib().mas_lpips_pool_bwd(_p(a), _p(seed), _p(dz), _p(dy), n, h, w, c, _DT[a.dtype], _stream()), "lpips_pool_bwd")
    return dy


def head_blocks(h: int, w: int, c: int) -> int:
    """partial sums per image of a level (``mas_lpips_head_blocks``)"""
    n = lib().mas_lpips_head_blocks(h, w, c)
    check(min(n, 0), "lpips_head_blocks")
    return n


def head_fwd(feat, w, partial):
    """feat [2 B, C, H, W] (channels_last) -> partial[b * blocks + j]"""
    n, c, h, wd = feat.shape
    check(lib().mas_lpips_head_fwd(_p(feat), _p(w), n // 2, h, wd, c, _DT[feat.dtype], _p(partial), _stream()), "lpips_head_fwd")


def finalize(partial, b: int, hw, blocks, device):
    """-> out [B] fp32; ``hw`` / ``blocks``: pixels and partial sums per image of every level, in the order of ``partial``"""
    out = torch.empty(b, dtype=torch.float32, device=device)
    n = len(hw)
    check(lib().mas_lpips_finalize(_p(partial), b, n, (C.c_int32 * n)(*hw), (C.c_int32 * n)(*blocks), _p(out), _stream()), "lpips_finalize")
    return out


def head_bwd(feat, w, dout):
    """the rec side's seed [B, C, H, W] (channels_last) for dout [B] fp32"""
    n, c, h, wd = feat.shape
    seed = O._nhwc(n // 2, c, h, wd, feat.dtype, feat.device)
    check(lib().mas_lpips_head_bwd(_p(feat), _p(w), n // 2, h, wd, c, _DT[feat.dtype], _p(dout), _p(seed), _stream()), "lpips_head_bwd")
    return seed


# --------------------------------------------------------------------------- #
# the network
# --------------------------------------------------------------------------- #
def network_forward(convs, canvas):
    """canvas [2 B, 8, H, W] -> (the five ReLU features, every convolution's ReLU output per level)"""
    feats, acts, x = [], [], canvas
    for l in range(LEVELS):
        if l > 0:
            x = pool_fwd(x)
        level_acts = []
        for j, conv in enumerate(convs[l]):
            x = relu_fwd(O._conv(x, conv, l, j, False))
            level_acts.append(x)
        acts.append(level_acts)
        feats.append(x)
    return feats, acts


class _Lpips(torch.autograd.Function):
    """real, fake -> [B] fp32.  Forward: pack, 13 x (convolution, ReLU), 4 pools, 5 heads, finalize -- 37 launches.  Backward (rec
    half): per level the head's seed, the pool backward with the ReLU mask, the convolutions' data gradients with the ReLU masks
    between them, and the pack adjoint -- 32 launches.  Everything the backward reads lives on ``ctx`` and is never written again, so
    the node can be differentiated any number of times (``retain_graph=True``: the adaptive weight does that every step)."""

    @staticmethod
    def forward(ctx, real, fake, lp, dtype):
        dev, b = real.device, real.shape[0]
        shift = lp.scaling_layer.shift.detach().float().reshape(-1).contiguous()
        scale = lp.scaling_layer.scale.detach().float().reshape(-1).contiguous()
        convs = O.vgg_convs(lp)
        lins = O._lin_weights(lp)
        canvas = pack_fwd(real, fake, shift, scale, dtype)
        feats, acts = network_forward(convs, canvas)
        hw = [f.shape[2] * f.shape[3] for f in feats]
        blocks = [head_blocks(f.shape[2], f.shape[3], f.shape[1]) for f in feats]
        partial = torch.empty(b * sum(blocks), dtype=torch.float32, device=dev)
        off = 0
        for l in range(LEVELS):
            head_fwd(feats[l], lins[l], partial[off:])
            off += b * blocks[l]
        out = finalize(partial, b, hw, blocks, dev)
        if ctx.needs_input_grad[1]:
            ctx.convs, ctx.lins, ctx.scale, ctx.feats = convs, lins, scale, feats
            ctx.acts = [[a[b:] for a in level] for level in acts]
            ctx.save_for_backward(fake)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        (fake,) = ctx.saved_tensors
        b = fake.shape[0]
        dout = dout.float().contiguous()
        d = None                                   # gradient of the pooled input of the level above
        for l in range(LEVELS - 1, -1, -1):
            feat = ctx.feats[l]
            seed = head_bwd(feat, ctx.lins[l], dout)
            dy = pool_bwd(feat[b:], seed, d)
            for j in range(len(ctx.convs[l]) - 1, -1, -1):
                da = O._conv(dy, ctx.convs[l][j], l, j, True)
                if j > 0:
                    dy = O.relu_bwd(da, ctx.acts[l][j - 1])
                else:
                    d = da
        return None, pack_bwd(d, ctx.scale, fake), None, None


def envelope(real, fake):
    """None when ``lpips_distance`` takes these inputs, else the reason it does not"""
    if real.dim() != 4 or real.shape[1] != 3:
        return f"images must be [B, 3, H, W], got {tuple(real.shape)}"
    if real.shape != fake.shape:
        return f"images {tuple(real.shape)} and reconstructions {tuple(fake.shape)} differ"
    if real.shape[0] < 1 or min(real.shape[2:]) < MIN_SIDE:
        return f"needs B >= 1 and H, W >= {MIN_SIDE} (four 2x2 pools), got {tuple(real.shape)}"
    if real.dtype not in _DT or fake.dtype not in _DT:
        return f"images must be float32 or bfloat16, got {real.dtype} and {fake.dtype}"
    return None


def lpips_distance(lp, real, fake, dtype=None):
    """LPIPS(real, fake) of ``lp`` (a ``losses.lpips.LPIPS``; its Dropout taken as the identity: evaluation mode) on the HIP path ->
    [B, 1, 1, 1] fp32.  ``dtype``: the activations' precision, ``None`` = bf16 (what the module's convolutions are pinned to),
    ``torch.float32`` = the parity mode.  The gradient reaches ``fake`` only, in its dtype and memory layout."""
    _require_cuda(real, "LPIPS")
    _require_cuda(fake, "LPIPS")
    why = envelope(real, fake)
    if why is not None:
        raise ValueError("LPIPS (HIP path): " + why)
    dtype = dtype or torch.bfloat16
    if dtype not in _DT:
        raise TypeError(f"LPIPS (HIP path): activations' dtype {dtype}")
    return _Lpips.apply(real.detach(), fake, lp, dtype).view(-1, 1, 1, 1)
