#!/usr/bin/env python3
"""FaceLoss forward + backward on the MI355X: the HIP path (losses/face_loss.py) against the reference's composition (torchvision-rule
crops + the torch modules of the same network, evaluation mode) on the same GPU, fp32 and bf16; and the VQ-IMG generator loss
(VQLPIPSWithDiscriminator, optimizer_idx 0: L1 + PatchGAN + adaptive weight) with the face term on against off.  One JSON line.

    python tools/face_loss_bench.py [--batch 32] [--size 256] [--faces 1 3] [--iters 20] [--kernels]

Inputs and weights are seeded (tests/helpers/face_ref.py: the synthetic weights).  ``--kernels`` also records which convolution kernel
every ResNet shape takes (``ops.last_kernel()``) at N = 1..6.  Launch counts come from a separate ``rocprofv3 --kernel-trace --stats``
run of ``--profile`` (two runs, different ``--iters``: the difference over the extra calls)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "make-a-scene_amd"), ROOT, os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import face_ref as R  # noqa: E402


def boxes_for(batch, faces, size):
    """``faces`` face boxes spread over the first images: 40-90 px, portrait and landscape"""
    out = [[] for _ in range(batch)]
    g = torch.Generator().manual_seed(7)
    for i in range(faces):
        w, h = (int(v) for v in torch.randint(40, 90, (2,), generator=g))
        x0, y0 = int(torch.randint(0, size - w, (1,), generator=g)), int(torch.randint(0, size - h, (1,), generator=g))
        out[i % batch].append([x0, y0, x0 + w, y0 + h])
    return out


def timeit(fn, iters, warmup=3):
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
    ap.add_argument("--faces", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--profile", action="store_true", help="HIP path only, bf16, --iters calls per face count (for rocprofv3)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from mas_hip import ops
    tmp = tempfile.mkdtemp()
    ck = os.path.join(tmp, "face_synth.pt")
    sd = R.synth_face_state_dict(0)
    torch.save(sd, ck)
    os.environ["MAS_FACE_CKPT"] = ck
    from losses.face_loss import FaceLoss
    from losses.loss_img import VQLPIPSWithDiscriminator
    from models.modules import Conv2d
    fl = FaceLoss().to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    img, rec0 = R.synth_images(a.batch, a.size, a.size, 1)
    img, rec0 = img.to(dev), rec0.to(dev)
    res = {"batch": a.batch, "size": a.size, "iters": a.iters}

    if a.profile:                     # (launches per call = the difference of two runs with --iters k1 and k2, over k2 - k1)
        ops.set_compute_dtype(torch.bfloat16)
        for nf in a.faces:
            bb = boxes_for(a.batch, nf, a.size)
            for _ in range(a.iters):
                r = rec0.clone().requires_grad_(True)
                fl(img, r, bb).backward()
        torch.cuda.synchronize()
        print(json.dumps({"profile": True, "faces": a.faces}))
        return

    for nf in a.faces:
        bb = boxes_for(a.batch, nf, a.size)
        row = {}
        for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            ops.set_compute_dtype(dt)

            def hip():
                r = rec0.clone().requires_grad_(True)
                fl(img, r, bb).backward()

            def ref():
                r = rec0.clone().requires_grad_(True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                    loss = R.face_loss(sd_dev, img, r, bb)
                loss.float().backward()

            row[f"hip_{name}_ms"] = round(timeit(hip, a.iters), 3)
            row[f"ref_{name}_ms"] = round(timeit(ref, a.iters), 3)
            # host issue time of the HIP path: the same call without waiting for the GPU in between, timed to its last launch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hip()
            row[f"hip_{name}_issue_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            torch.cuda.synchronize()
        # the generator loss (optimizer_idx 0) with the face term on against off, bf16
        ops.set_compute_dtype(torch.bfloat16)
        torch.manual_seed(0)
        last = Conv2d(32, 3, 3, 1, 1).to(dev)
        z = torch.randn(a.batch, 32, a.size, a.size, device=dev)
        on = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=fl).to(dev)
        off = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None).to(dev)
        for key, lf in (("gen_loss_face_on_ms", on), ("gen_loss_face_off_ms", off)):
            def step():
                zz = z.detach().requires_grad_(True)
                rec = last(zz)
                loss, _ = lf(0, 1, img, rec, torch.zeros((), device=dev), bbox_face=bb, last_layer=last)
                loss.backward()
            row[key] = round(timeit(step, a.iters), 3)
        res[f"faces{nf}"] = row

    if a.kernels:
        ops.set_compute_dtype(torch.bfloat16)
        seen = {}

        def hook(kind, shape, launch):
            launch()
            seen.setdefault(kind + str(shape), ops.last_kernel())

        for n in range(1, 7):
            bb = [[[10, 10, 80, 90]] for _ in range(n)]
            n_img = n
            ii, rr = R.synth_images(n_img, 128, 128, 2)
            r = rr.to(dev).requires_grad_(True)
            ops.set_launch_hook(hook)
            try:
                fl(ii.to(dev), r, bb).backward()
            finally:
                ops.set_launch_hook(None)
        torch.cuda.synchronize()
        res["conv_kernels"] = sorted(set(seen.values()))
        res["conv_shapes"] = len(seen)
        res["conv_kernel_by_shape"] = seen
    print(json.dumps(res))


if __name__ == "__main__":
    main()
