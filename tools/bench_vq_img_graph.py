#!/usr/bin/env python3
"""The VQ-IMG training call (conf/img_config.yaml's model as bench.py builds it, 256 x 256 images, bf16 compute; the whole objective of
train.py:84-103: VQLPIPSWithDiscriminator with LPIPS on its HIP path and no face term, two Adams) in three forms, at B = 2 with accumulate 8
(the reference's own setting) and B = 32 with accumulate 1:

  eager               today's step: the loss's ATen tail, host-step Adams, the Codebook's host reservoir
  eager + HIP tail    hip_tail(True), Adam(device_step=True), the device reservoir: what the graph holds, issued launch by launch
  graphed             mas_hip.graphs.GraphedGanStep(accumulate=k) over the same

One model, loss and optimizer pair per column (same seed), the codebook in its steady phase (collect + lookup, no re-initialisation in
sight), the discriminator's gate open.  A block is n calls (a multiple of accumulate) between two device synchronisations, n sized from a
first short block to fill --seconds; the columns alternate block by block, two rounds.  The figure is device-synchronised wall time per CALL
(an optimizer step is `accumulate` calls).  The graphed column's block runs under torch.cuda.set_sync_debug_mode("error").  Launches per
call: the device activities torch.profiler records for one closing call (kernels and copies; "not measured" where the profiler gives none).

Then the tail alone, switch off against on, in the same process: the loss's two halves (discriminator passes included, no perceptual
term) on a reconstruction that is one 128 -> 3 convolution of a fixed map, forward and backward; device time (the sum of the profiler's
device activities) and their count per call, and the difference of the two columns, which is the tail's."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
os.environ.setdefault("MAS_LPIPS_STRICT", "0")          # LPIPS keeps its initialisation: timing does not depend on the weights' values
import torch
from mas_hip import graphs, ops, optim
from losses.loss_img import VQLPIPSWithDiscriminator, hip_tail
from losses.lpips import hip_path
from models import VQBASE
from models.modules import Conv2d

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0, help="wall time one timed block should fill")
ap.add_argument("--configs", default="2:8,32:1", help="batch:accumulate pairs")
a = ap.parse_args()

IMG_CFG = dict(ddconfig=dict(z_channels=256, in_channels=3, out_channels=3, channels=[128, 128, 128, 256, 512, 512], num_res_blocks=2,
                             resolution=512, attn_resolutions=[32], dropout=0.0), n_embed=8192, embed_dim=256, init_steps=3000, reservoir_size=12500)
COLS = ("eager", "eager + HIP tail", "graphed")
dev = torch.device("cuda:0")
ops.set_compute_dtype(torch.bfloat16)


def device_activities(fn):
    """(count, total microseconds) of what torch.profiler records on the device for one fn(), or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return (len(ev), sum(e.time_range.elapsed_us() for e in ev)) if ev else None
    except Exception as e:                                    # a profiler that cannot trace this device: the times stand without the counts
        print(f"(profiler: {type(e).__name__}: {e})", flush=True)
        return None


def gan_call(model, crit, gopt, dopt, x, step, closing, last_layer=None, rec_fn=None):
    rec, q = model(x) if rec_fn is None else rec_fn()
    d_loss = crit(1, step, x, rec)
    d_loss.backward()
    disc = list(crit.discriminator.parameters())
    for p in disc:
        p.requires_grad_(False)
    try:
        loss, _ = crit(0, step, x, rec, q, last_layer=last_layer if last_layer is not None else model.decoder.model[-1])
        loss.backward()
    finally:
        for p in disc:
            p.requires_grad_(True)
    if closing:
        dopt.step(); dopt.zero_grad(set_to_none=True)
        gopt.step(); gopt.zero_grad(set_to_none=True)
    return loss


def block(fn, n, guarded=False):
    torch.cuda.synchronize()
    if guarded:
        torch.cuda.set_sync_debug_mode("error")
    try:
        t0 = time.perf_counter()
        for _ in range(n):
            loss = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, loss


with hip_path(True):
    for cfg in a.configs.split(","):
        batch, acc = (int(v) for v in cfg.split(":"))
        x = torch.rand(batch, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(dev)
        cols, counts = {}, {}
        for name in COLS:
            torch.manual_seed(1)
            model = VQBASE(**IMG_CFG)
            with torch.no_grad():
                model.quantize.embedding.weight.normal_(0.0, 1.0)
            model = model.to(dev).train()
            model.quantize.q_counter = model.quantize.q_re_end          # steady state: collect + lookup, no k-means
            crit = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss="lpips", face_loss=None).to(dev)
            on = name != "eager"
            if on:
                model.quantize.enable_device_reservoir(seed=7)
            gopt = optim.Adam(model.parameters(), lr=5e-6 / acc, betas=(0.5, 0.9), device_step=on)
            dopt = optim.Adam(crit.discriminator.parameters(), lr=5e-6 / acc, betas=(0.5, 0.9), device_step=on)
            if name == "graphed":
                torch.cuda.synchronize(); t0 = time.perf_counter()
                step = graphs.GraphedGanStep(model, crit, gopt, dopt, x, accumulate=acc, warmup=acc, global_step=0)
                for _ in range(acc):
                    step(x)
                torch.cuda.synchronize()
                print(f"B={batch} accumulate={acc} graphed: {acc} warm-up calls + {step.captures} capture(s) + {acc} replays "
                      f"{time.perf_counter() - t0:.2f} s", flush=True)
                cols[name] = lambda step=step: step(x).loss
            else:
                def eager(model=model, crit=crit, gopt=gopt, dopt=dopt, on=on, n=[0]):
                    n[0] += 1
                    with hip_tail(on):
                        return gan_call(model, crit, gopt, dopt, x, n[0], n[0] % acc == 0)
                for _ in range(2 * acc):
                    eager()
                cols[name] = eager
            for _ in range(acc - 1):                          # the profiled call is a closing one
                cols[name]()
            counts[name] = device_activities(cols[name])
        n_calls = {k: max(2, int(a.seconds / block(fn, acc, k == "graphed")[0]) // acc) * acc for k, fn in cols.items()}
        times = {k: [] for k in cols}
        for _ in range(2):
            for k, fn in cols.items():
                dt, loss = block(fn, n_calls[k], k == "graphed")
                assert bool(torch.isfinite(loss)), (k, float(loss))
                times[k].append(dt)
        for k in cols:
            c = counts[k]
            print(f"VQ-IMG 256x256 B={batch} accumulate={acc} training call, {k}: " + " / ".join(f"{t * 1e3:.2f}" for t in times[k])
                  + f" ms/call ({n_calls[k]} calls per block)  best {batch / min(times[k]):.1f} images/s; device activities of a closing call: "
                  + (f"{c[0]} ({c[1] / 1e3:.2f} ms)" if c else "not measured"), flush=True)
        del cols, model, gopt, dopt, step, crit
        torch.cuda.empty_cache()

        # ---- the tail alone: the loss's two halves on a reconstruction that is one convolution of a fixed map ---------------------------------
        torch.manual_seed(2)
        last = Conv2d(128, 3, 3, 1, 1).to(dev)
        h = torch.randn(batch, 128, 256, 256, generator=torch.Generator().manual_seed(3)).to(dev)
        crit = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None).to(dev)
        q = torch.zeros((), device=dev)
        res = {}
        for on in (False, True, False, True):
            def tail(on=on):
                with hip_tail(on):
                    loss = gan_call(None, crit, None, None, x, 1, False, last_layer=last, rec_fn=lambda: (last(h), q))
                last.zero_grad(set_to_none=True); crit.zero_grad(set_to_none=True)
                return loss
            for _ in range(3):
                tail()
            res.setdefault(on, []).append((device_activities(tail), block(tail, 20)[0]))
        for on in (False, True):
            print(f"loss call (discriminator passes + tail) B={batch}, hip_tail {'on' if on else 'off'}: " + " / ".join(
                (f"{c[0]} device activities, {c[1] / 1e3:.3f} ms on the device" if c else "device activities not measured") + f", {t * 1e3:.3f} ms wall"
                for c, t in res[on]), flush=True)
        if all(c for v in res.values() for c, _ in v):
            d_n = res[False][-1][0][0] - res[True][-1][0][0]
            d_t = min(c[1] for c, _ in res[False]) - min(c[1] for c, _ in res[True])
            print(f"  the HIP tail: {d_n} fewer device activities and {d_t / 1e3:.3f} ms less device time per call at B={batch}", flush=True)
        del last, h, crit
        torch.cuda.empty_cache()
