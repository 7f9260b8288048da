#!/usr/bin/env python3
"""ObjectLoss forward + backward on the MI355X: the atlas (losses/object_loss.py) against the obvious composition -- one call of the
existing GPU LPIPS (losses.lpips.LPIPS) per crop, summed as the reference's block does -- in bf16 and in the fp32 parity mode; and the
VQ-IMG generator loss (VQLPIPSWithDiscriminator, optimizer_idx 0, perceptual term on) with the object term on against off.  One JSON
line.

    python tools/object_loss_bench.py [--batch 32] [--size 256] [--boxes 4] [--lo 24] [--hi 160] [--iters 10] [--profile]

Boxes are seeded: ``--boxes`` per image, sides uniform in [lo, hi], placed so that most lie inside the image and some cross an edge.
Weights: oracle.lpips_oracle.synth_lpips_state_dict (the timing does not depend on their values).  ``--profile``: the atlas only,
bf16, ``--iters`` calls (for ``rocprofv3 --kernel-trace --stats``)."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "make-a-scene_amd"), ROOT, os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)
os.environ.setdefault("MAS_LPIPS_STRICT", "0")

import torch  # noqa: E402

import object_ref as R  # noqa: E402


def seeded_boxes(batch, per_image, size, lo, hi, seed=7):
    rng = random.Random(seed)
    out = []
    for _ in range(batch):
        boxes = []
        for _ in range(per_image):
            h, w = rng.randint(lo, hi), rng.randint(lo, hi)
            y0, x0 = rng.randint(-h // 4, size - 3 * h // 4), rng.randint(-w // 4, size - 3 * w // 4)
            boxes.append([x0, y0, x0 + w, y0 + h])
        out.append(boxes)
    return out


def timeit(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=4)
    ap.add_argument("--lo", type=int, default=24)
    ap.add_argument("--hi", type=int, default=160)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from losses.loss_img import VQLPIPSWithDiscriminator
    from losses.lpips_with_object import LPIPSWithObject
    from losses.object_loss import ObjectLoss
    from mas_hip import objects as O
    from mas_hip import ops
    from models.modules import Conv2d
    from oracle.lpips_oracle import synth_lpips_state_dict
    lp = LPIPSWithObject().eval()                # what the VQ-IMG loss builds for its perceptual term
    lp.load_state_dict(synth_lpips_state_dict(3), strict=True)
    lp = lp.to(dev)
    g = torch.Generator().manual_seed(1)
    img = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).to(dev)
    rec0 = (img + 0.2 * torch.randn(img.shape, generator=g).to(dev)).clamp(-1, 1)
    bbox = seeded_boxes(a.batch, a.boxes, a.size, a.lo, a.hi)
    plan = O.make_plan(bbox, a.batch)
    term = ObjectLoss(lp)
    res = {"batch": a.batch, "size": a.size, "boxes_per_image": a.boxes, "box_sides": [a.lo, a.hi], "iters": a.iters,
           "crops": plan.n_cells, "canvases": plan.n_canvas, "canvas_hw": [plan.H, plan.W], "area_efficiency": round(plan.efficiency(), 3)}

    def atlas():
        r = rec0.clone().requires_grad_(True)
        term(img, r, bbox).backward()

    if a.profile:
        ops.set_compute_dtype(torch.bfloat16)
        for _ in range(a.iters):
            atlas()
        torch.cuda.synchronize()
        print(json.dumps(res))
        return

    def loop():
        r = rec0.clone().requires_grad_(True)
        R.object_loss(None, img, r, bbox, net=lambda _sd, x, y: lp(x.contiguous(), y.contiguous()))[0].backward()

    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        ops.set_compute_dtype(dt)
        res[f"atlas_fwd_bwd_ms_{name}"] = round(timeit(atlas, a.iters), 3)
        res[f"per_crop_loop_fwd_bwd_ms_{name}"] = round(timeit(loop, max(2, a.iters // 4), warmup=1), 3)
        res[f"speedup_{name}"] = round(res[f"per_crop_loop_fwd_bwd_ms_{name}"] / res[f"atlas_fwd_bwd_ms_{name}"], 2)

    # the generator loss module (L1 + perceptual + PatchGAN + adaptive weight), object term on and off, bf16
    ops.set_compute_dtype(torch.bfloat16)
    last = Conv2d(64, 3, 3, 1, 1).to(dev)
    zin = torch.randn(a.batch, 64, a.size, a.size, generator=g).to(dev)
    on = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=lp, face_loss=None, object_loss=ObjectLoss(lp)).to(dev)
    off = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=lp, face_loss=None).to(dev)
    off.discriminator.load_state_dict(on.discriminator.state_dict())
    for name, lf in (("on", on), ("off", off)):
        def step(lf=lf):
            z = zin.clone().requires_grad_(True)
            rec = last(z)
            loss, _ = lf(0, 1, img, rec, torch.zeros((), device=dev), bbox_obj=bbox, last_layer=last)
            loss.backward()
        res[f"generator_loss_fwd_bwd_ms_object_{name}"] = round(timeit(step, a.iters), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
