#!/usr/bin/env python3
"""The VQ-SEG training call (conf/seg_config.yaml's model as bench.py builds it: 159 label channels at 256 x 256, 16 x 16 latents, 256 codes
of 256; VQVAEWithBCELoss over SegLabels; AdamW) in four forms, at B = 2 with accumulate 3 (the reference's own setting) and B = 8 with
accumulate 1:

  host reservoir      eager, the Codebook's default reservoir (two CPU permutations per call), host-step AdamW: the parent's schedule
  device reservoir    eager, Codebook.enable_device_reservoir(), host-step AdamW
  device + dev-step   eager, device reservoir, AdamW(device_step=True)
  graphed             mas_hip.graphs.GraphedTrainStep(accumulate=k) over the same

One model and optimizer per column (same seed), the codebook in its steady phase (collect + lookup, no re-initialisation in sight).  A block
is n calls (a multiple of accumulate) between two device synchronisations, n sized from a first short block to fill --seconds; the columns
alternate block by block, two rounds.  The figure is device-synchronised wall time per CALL (an optimizer step is `accumulate` calls).  The
graphed column's block runs under torch.cuda.set_sync_debug_mode("error")."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch
from mas_hip import graphs, ops, optim
from mas_hip.seglabels import SegLabels
from losses.loss_seg import VQVAEWithBCELoss
from models import VQBASE

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0, help="wall time one timed block should fill")
ap.add_argument("--configs", default="2:3,8:1", help="batch:accumulate pairs")
a = ap.parse_args()

SEG_CFG = dict(ddconfig=dict(z_channels=256, in_channels=159, out_channels=159, channels=[128, 128, 128, 256, 512, 512], num_res_blocks=2,
                             resolution=512, attn_resolutions=[32], dropout=0.0), n_embed=256, embed_dim=256, init_steps=3000, reservoir_size=12500)
COLS = ("host reservoir", "device reservoir", "device + dev-step", "graphed")
dev = torch.device("cuda:0")


def planes(batch, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, hi + 1, (batch, 256, 256), generator=g, dtype=torch.uint8) for hi in (133, 20, 5, 2)], dim=1).to(dev)


for cfg in a.configs.split(","):
    batch, acc = (int(v) for v in cfg.split(":"))
    x = planes(batch, 0)
    cols = {}
    for name in COLS:
        torch.manual_seed(1)
        model, crit = VQBASE(**SEG_CFG).to(dev).train(), VQVAEWithBCELoss().to(dev)
        model.quantize.q_counter = model.quantize.q_re_end          # steady state: collect + lookup, no k-means
        if name != "host reservoir":
            model.quantize.enable_device_reservoir(seed=7)
        opt = optim.AdamW(model.parameters(), lr=4.5e-6, betas=(0.5, 0.9), device_step=name in ("device + dev-step", "graphed"))

        def loss_fn(p, model=model, crit=crit):
            lab = SegLabels(p)
            rec, q = model(lab)
            return crit(q, lab, rec)

        def eager(model=model, opt=opt, loss_fn=loss_fn, n=[0]):
            loss = loss_fn(x)
            loss.backward()
            n[0] += 1
            if n[0] % acc == 0:
                opt.step()
                opt.zero_grad(set_to_none=True)
            return loss
        if name == "graphed":
            torch.cuda.synchronize(); t0 = time.perf_counter()
            step = graphs.GraphedTrainStep(loss_fn, opt, x, warmup=acc, modules=[model], accumulate=acc)
            for _ in range(acc):
                step(x)
            torch.cuda.synchronize()
            print(f"B={batch} accumulate={acc} graphed: {acc} warm-up calls + {step.captures} capture(s) + {acc} replays "
                  f"{time.perf_counter() - t0:.2f} s", flush=True)
            cols[name] = lambda step=step: step(x)
        else:
            for _ in range(2 * acc):
                eager()
            cols[name] = eager

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
    n_calls = {k: max(2, int(a.seconds / block(fn, acc, k == "graphed")[0]) // acc) * acc for k, fn in cols.items()}
    times = {k: [] for k in cols}
    for _ in range(2):
        for k, fn in cols.items():
            dt, loss = block(fn, n_calls[k], k == "graphed")
            assert bool(torch.isfinite(loss)), (k, float(loss))
            times[k].append(dt)
    for k in cols:
        print(f"VQ-SEG 256x256x159 B={batch} accumulate={acc} training call, {k}: " + " / ".join(f"{t * 1e3:.2f}" for t in times[k])
              + f" ms/call ({n_calls[k]} calls per block)  best {batch / min(times[k]):.1f} samples/s", flush=True)
    del cols, model, opt, step, crit
    torch.cuda.empty_cache()
