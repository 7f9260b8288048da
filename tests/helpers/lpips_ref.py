"""fp64 restatement on the CPU of the whole-image LPIPS path (csrc/lpips.hip, mas_hip/lpips.py): pack, ReLU, the 2x2 max-pool with
first-maximum routing, the distance head, finalize, and the gradient of each as an EXPLICIT formula -- no autograd through ``sqrt``, so
a pixel whose rec features are all zero has a finite gradient (the rule of ``mas_lpips_head_bwd``: the 1 / |f| term is 0 there; torch's
own backward gives NaN).  ``torch_expression`` is today's ``LPIPS.forward`` spelled with ``F.conv2d``, the yardstick the restatement
is pinned to (tests/test_lpips_hip_cpu.py).  Tensors are NCHW; weights are ``oracle.lpips_oracle.synth_lpips_state_dict``'s."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import lpips_oracle as L  # noqa: E402

EPS = 1e-10
CP = 8
CHANNELS = (64, 128, 256, 512, 512)
# eight bf16 numbers (exact in bf16): draws from them give positive ties and all-zero 2x2 windows
BF16_SET = (-1.5, -0.25, 0.0, 0.0, 0.0, 0.5, 0.5, 2.0)


def f64(sd):
    return {k: v.double() for k, v in sd.items()}


# ---- today's module, spelled out -------------------------------------------------------------------------------------------------
def torch_expression(sd, real, fake):
    """losses/lpips.py:LPIPS.forward in the dtype of ``sd`` (one pass over cat([real, fake]), torch's own operators and autograd)"""
    b = real.shape[0]
    x = (torch.cat([real, fake], dim=0) - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
    feats = L.vgg_features(sd, x)
    total = 0
    for i, f in enumerate(feats):
        d = (L.norm_tensor(f[:b]) - L.norm_tensor(f[b:])) ** 2
        w = sd[f"lin{i}.model.1.weight"]
        total = total + (d * w).sum(dim=1, keepdim=True).mean([2, 3], keepdim=True)
    return total


# ---- the pieces ----------------------------------------------------------------------------------------------------------------------
def pack(real, fake, shift, scale):
    x = (torch.cat([real, fake], dim=0).double() - shift.double().view(1, 3, 1, 1)) / scale.double().view(1, 3, 1, 1)
    return F.pad(x, (0, 0, 0, 0, 0, CP - 3))


def pack_adjoint(dcanvas, scale):
    return dcanvas[:, :3].double() / scale.double().view(1, 3, 1, 1)


def relu(x):
    return torch.where(x > 0, x, torch.zeros_like(x))


def relu_bwd(da, a):
    return torch.where(a > 0, da, torch.zeros_like(da))


def _windows(x):
    """[4, N, C, H // 2, W // 2]: the window's pixels in row-major order (torch's scan order)"""
    ho, wo = x.shape[2] // 2, x.shape[3] // 2
    return torch.stack([x[:, :, dy:2 * ho:2, dx:2 * wo:2] for dy in (0, 1) for dx in (0, 1)])


def pool(x):
    return _windows(x).max(dim=0).values


def pool_bwd(a, seed, dz):
    """a > 0 ? seed + routed dz : 0, dz routed to the FIRST maximum of its window; a last odd row / column gets the seed only"""
    g = torch.zeros_like(a) if seed is None else seed.clone()
    if dz is not None:
        win = _windows(a)
        is_max = win == win.max(dim=0, keepdim=True).values
        first = is_max & (is_max.cumsum(dim=0) == 1)
        ho, wo = dz.shape[2:]
        for k, (dy, dx) in enumerate((dy, dx) for dy in (0, 1) for dx in (0, 1)):
            g[:, :, dy:2 * ho:2, dx:2 * wo:2] += first[k] * dz
    return torch.where(a > 0, g, torch.zeros_like(g))


def head_sums(fr, ff, w):
    """[B]: sum over pixels of sum_c w_c (r_c / (|r| + eps) - f_c / (|f| + eps))^2"""
    nr = fr.pow(2).sum(1, keepdim=True).sqrt() + EPS
    nf = ff.pow(2).sum(1, keepdim=True).sqrt() + EPS
    e = fr / nr - ff / nf
    return (e * e * w.view(1, -1, 1, 1)).sum(dim=(1, 2, 3))


def finalize(sums, hw):
    """out[b] = sum_l sums[l][b] / hw[l]"""
    return sum(s / n for s, n in zip(sums, hw))


def head_bwd(fr, ff, w, dout):
    """d (sum_b dout[b] * mean over pixels of the head) / d ff, explicit; the 1 / |f| term is 0 where |f| = 0"""
    coef = (dout.view(-1, 1, 1, 1) / (fr.shape[2] * fr.shape[3]))
    nr = fr.pow(2).sum(1, keepdim=True).sqrt() + EPS
    s = ff.pow(2).sum(1, keepdim=True).sqrt()
    nf = s + EPS
    g = -2.0 * coef * w.view(1, -1, 1, 1) * (fr / nr - ff / nf)
    gf = (g * ff).sum(1, keepdim=True)
    rad = torch.where(s > 0, gf / (nf * nf * torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(s))
    return g / nf - ff * rad


# ---- the whole op -------------------------------------------------------------------------------------------------------------------
def _convs(sd):
    return [[(sd[f"vgg.{s}.{i}.weight"], sd[f"vgg.{s}.{i}.bias"]) for i, _, _ in convs] for s, convs in L.SLICE_CONVS.items()]


def lpips(sd, real, fake, dout=None):
    """-> (out [B], d fake [B, 3, H, W] for ``dout`` [B] (ones when None)), both fp64, gradients by the explicit formulas above"""
    sd = f64(sd)
    b = real.shape[0]
    shift, scale = sd["scaling_layer.shift"].view(-1), sd["scaling_layer.scale"].view(-1)
    convs = _convs(sd)
    x = pack(real, fake, shift, scale)[:, :3]
    feats, acts = [], []
    for l, level in enumerate(convs):
        if l > 0:
            x = pool(x)
        la = []
        for wt, bias in level:
            x = relu(F.conv2d(x, wt, bias, padding=1))
            la.append(x)
        acts.append(la)
        feats.append(x)
    lins = [sd[f"lin{l}.model.1.weight"].view(-1) for l in range(5)]
    out = finalize([head_sums(f[:b], f[b:], lins[l]) for l, f in enumerate(feats)], [f.shape[2] * f.shape[3] for f in feats])
    dout = torch.ones(b, dtype=torch.float64) if dout is None else dout.double()
    d = None
    for l in range(4, -1, -1):
        f = feats[l]
        dy = pool_bwd(f[b:], head_bwd(f[:b], f[b:], lins[l], dout), d)
        for j in range(len(convs[l]) - 1, -1, -1):
            da = F.conv_transpose2d(dy, convs[l][j][0], padding=1)
            if j > 0:
                dy = relu_bwd(da, acts[l][j - 1][b:])
            else:
                d = da
    return out, pack_adjoint(d, scale)


def mask_margin(sd, real, fake):
    """How well-posed a gradient comparison is on these inputs, from the reference alone.  The gradient of a ReLU / max-pool network
    jumps where a pre-activation crosses zero or two entries of a pool window cross each other, and any two fp32 evaluations
    (another summation order is enough) disagree there by a whole unit's share of the gradient, not by a rounding error.
    -> (margin, rms): the smallest |pre-activation| and the smallest gap between the two largest entries of a window with a positive
    maximum, over the rec half in fp64; and the rms error of torch's own fp32 pre-activations against fp64 on the same inputs."""
    b = real.shape[0]

    def walk(sdx, dt):
        x = (torch.cat([real, fake], dim=0).to(dt) - sdx["scaling_layer.shift"]) / sdx["scaling_layer.scale"]
        zs, gap = [], float("inf")
        for l, level in enumerate(_convs(sdx)):
            if l > 0:
                top = _windows(x[b:]).topk(2, dim=0).values
                gap = min(gap, float((top[0] - top[1])[top[0] > 0].min()))
                x = pool(x)
            for wt, bias in level:
                z = F.conv2d(x, wt, bias, padding=1)
                zs.append(z[b:])
                x = relu(z)
        return zs, gap
    z64, gap = walk(f64(sd), torch.float64)
    z32, _ = walk(sd, torch.float32)
    err = torch.cat([(a.double() - c).flatten() for a, c in zip(z32, z64)])
    return min(gap, min(float(z.abs().min()) for z in z64)), float(err.pow(2).mean().sqrt())


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------------------
def images(b, h, w, seed):
    """real / fake in [0, 1], fake a perturbed real (a reconstruction)"""
    g = torch.Generator().manual_seed(seed)
    real = torch.rand(b, 3, h, w, generator=g)
    fake = (real + 0.1 * torch.randn(b, 3, h, w, generator=g)).clamp(0, 1)
    return real, fake


def head_case(c, h, w, seed, b=2, kind="random"):
    """features [2 b, c, h, w] (post-ReLU-like, exact in bf16), head weights [c], dout [b].  kind: "random"; "zeros": pixel 0 all
    zero on the rec side, pixel 1 on the real side, pixel 2 (where there is one) on both; "ulp": fake = real with one channel per
    pixel moved up by one bf16 ulp; "large": magnitude 1e3"""
    g = torch.Generator().manual_seed(seed * 7919 + c * 31 + h * 101 + w)
    f = torch.randn(2 * b, c, h, w, generator=g).clamp_min(0)
    f[:, 0] += 0.5                                        # no accidental all-zero pixel
    if kind == "large":
        f = f * 1e3
    if kind == "ulp":
        f = f + 0.25
    f = f.bfloat16().float()
    if kind == "ulp":
        f[b:] = f[:b]
        ch = torch.randint(0, c, (b, 1, h, w), generator=g)
        v = f[b:].gather(1, ch).bfloat16()
        up = (v.view(torch.int16) + 1).view(torch.bfloat16).float()          # positive values: the next bf16 up
        f[b:] = f[b:].scatter(1, ch, up)
    if kind == "zeros":
        flat = f.view(2 * b, c, h * w)
        flat[b:, :, 0] = 0
        if h * w > 1:
            flat[:b, :, 1] = 0
        if h * w > 2:
            flat[:, :, 2] = 0
    wts = torch.rand(c, generator=g) * (2.0 / c)
    dout = torch.rand(b, generator=g) + 0.5
    return f, wts, dout


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
