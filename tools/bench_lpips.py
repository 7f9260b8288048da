#!/usr/bin/env python3
"""The perceptual term of the VQ-IMG objective (losses.lpips.LPIPS, evaluation mode, synthetic weights) in two forms:

  torch   today's path: the thirteen convolutions on libmas_hip, ReLU / pools / distance head as torch expressions, autograd over
          cat([real, fake])
  hip     losses.lpips.hip_path(True): mas_hip.lpips.lpips_distance, one autograd node on csrc/lpips.hip, backward on the rec half

(a) LPIPS forward + backward (the gradient to ``fake``) at [32, 3, 256, 256] and [2, 3, 512, 512] (the reference's conf/img_config.yaml);
(b) the generator step of VQLPIPSWithDiscriminator (two ``autograd.grad`` calls for the adaptive weight + the backward) on bench.py's VQ-IMG
    model at B = 32, 256 x 256, switch off and on.

One process; a block is n calls between two device synchronisations, n sized from a first short block to fill --seconds; the columns
alternate block by block, two rounds.  Reported: device-synchronised wall time per call, peak memory above what was allocated before the
call, and kernel launches per call (torch.profiler's device-kernel events of one call; --no-launches skips that)."""
import argparse, os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
sys.path.insert(0, ROOT)
os.environ.setdefault("MAS_LPIPS_STRICT", "0")          # synthetic weights: timing does not depend on their values
import torch
from losses.loss_img import VQLPIPSWithDiscriminator
from losses.lpips import LPIPS, hip_path
from models import VQBASE

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0, help="wall time one timed block should fill")
ap.add_argument("--shapes", default="32x256x256,2x512x512", help="BxHxW of part (a)")
ap.add_argument("--step-batch", type=int, default=32, help="batch of part (b); 0 skips it")
ap.add_argument("--no-launches", action="store_true")
a = ap.parse_args()

IMG_CFG = dict(ddconfig=dict(z_channels=256, in_channels=3, out_channels=3, channels=[128, 128, 128, 256, 512, 512], num_res_blocks=2,
                             resolution=512, attn_resolutions=[32], dropout=0.0), n_embed=8192, embed_dim=256, init_steps=3000, reservoir_size=12500)
COLS = (("torch", False), ("hip", True))
dev = torch.device("cuda:0")


def synth_weights(lp, seed=3):
    """He-scaled convolutions, non-negative heads: activations stay O(1) through the thirteen layers"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in lp.named_parameters():
            if name.startswith("lin"):
                p.copy_(torch.rand(p.shape, generator=g) * (2.0 / p.shape[1]))
            elif p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[1] * 9)) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return lp


def block(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, out


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def launches(fn):
    if a.no_launches:
        return None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as e:                              # a build without device tracing: the other figures stand on their own
        print(f"  (launch count unavailable: {type(e).__name__}: {e})", flush=True)
        return None


def measure(title, fns):
    """fns: {column: callable}; prints one line per column"""
    for fn in fns.values():
        for _ in range(2):
            fn()
    n_calls = {k: max(2, int(a.seconds / block(fn, 2)[0])) for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(2):
        for k, fn in fns.items():
            dt, out = block(fn, n_calls[k])
            assert bool(torch.isfinite(out).all()), (title, k)
            times[k].append(dt)
    for k, fn in fns.items():
        mem, nl = peak_above(fn), launches(fn)
        print(f"{title}, {k}: " + " / ".join(f"{t * 1e3:.2f}" for t in times[k]) + f" ms/call ({n_calls[k]} calls per block), peak above the inputs "
              f"{mem:.0f} MiB, launches per call {'n/a' if nl is None else nl}", flush=True)
    best = {k: min(v) for k, v in times.items()}
    print(f"{title}: torch / hip = {best['torch'] / best['hip']:.2f}x", flush=True)


with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    lp = synth_weights(LPIPS()).eval().to(dev)

for spec in filter(None, a.shapes.split(",")):
    b, h, w = (int(v) for v in spec.split("x"))
    g = torch.Generator().manual_seed(0)
    real = torch.rand(b, 3, h, w, generator=g).to(dev)
    fake = (real + 0.1 * torch.randn(b, 3, h, w, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)

    def call(on):
        with hip_path(on):
            out = lp(real, fake)
            (grad,) = torch.autograd.grad(out.sum(), fake)
        return grad
    measure(f"LPIPS forward + backward [{b}, 3, {h}, {w}]", {k: (lambda on=on: call(on)) for k, on in COLS})
    del real, fake
    torch.cuda.empty_cache()

if a.step_batch > 0:
    torch.manual_seed(1)
    model = VQBASE(**IMG_CFG).to(dev).train()
    model.quantize.q_counter = model.quantize.q_re_end          # steady state: lookup, no k-means
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lf = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss="lpips", face_loss=None)
    synth_weights(lf.perceptual_loss)
    lf = lf.to(dev)
    for p in lf.discriminator.parameters():                      # the generator step: the discriminator is frozen (reference train.py:91)
        p.requires_grad_(False)
    x = torch.rand(a.step_batch, 3, 256, 256, generator=torch.Generator().manual_seed(2)).to(dev) * 2 - 1

    def step(on):
        with hip_path(on):
            rec, q = model(x)
            loss, _ = lf(0, 10, x, rec, q, last_layer=model.decoder.model[-1])
            loss.backward()
        model.zero_grad(set_to_none=True)
        return loss.detach()
    measure(f"VQ-IMG generator step (forward, VQLPIPSWithDiscriminator, backward) B={a.step_batch} 256x256", {k: (lambda on=on: step(on)) for k, on in COLS})
