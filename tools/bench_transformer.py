#!/usr/bin/env python3
"""BASELINE config 4: MakeAScene 24L / 1024d / 16 heads over 256 text + 256 seg + 1024 image tokens (S=1536), one GPU.
fwd + bwd of the cross-entropy on the image tokens (reference train.py:150-152), bf16 autocast for the library GEMMs,
HIP flash attention core.  Prints tokens/s and model TFLOP/s (1185.4 GFLOP/sample fwd full-S^2 count).
--loss: how the objective is computed -- aten: F.cross_entropy(logits.float()...) on forward()'s logits (the default, and bench.py's line);
fused: mas_hip.ops.cross_entropy on the same logits; model: MakeAScene.token_loss (logits for the image positions only).  A comma-separated
list times them in one process, alternating step by step, and prints one line each."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch
from mas_hip import ops
from models.transformer import MakeAScene

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--loss", default="aten", help="aten | fused | model, or a comma-separated list of them (timed alternating)")
ap.add_argument("--graph", action="store_true", help="the whole TRAINING step (token_loss, backward, AdamW) at B = 1, 2, 8 in three forms timed "
                "alternating, each twice: eager with the host-step AdamW, eager with device_step=True, mas_hip.graphs.GraphedTrainStep")
ap.add_argument("--seconds", type=float, default=2.0, help="--graph: wall time one timed block should fill")
a = ap.parse_args()


def graph_bench():
    """One model and optimizer per column (same seed).  A block is n steps between two device synchronisations, n sized from a first short
    block to fill --seconds; the columns alternate block by block, two rounds.  The replay loop of the graph column runs under
    torch.cuda.set_sync_debug_mode("error"): a host read inside it would raise."""
    from mas_hip import graphs, optim
    dev = torch.device("cuda:0")
    for batch in (1, 2, 8):
        torch.manual_seed(0)
        text = torch.randint(1, 49408, (batch, 256), device=dev); text[:, 200:] = 0
        seg = torch.randint(0, 256, (batch, 256), device=dev)
        img = torch.randint(0, 8192, (batch, 1024), device=dev)
        cols = {}
        for name in ("eager host-step", "eager device_step", "graphed"):
            torch.manual_seed(1)
            model = MakeAScene(a.layers, 1024, 16, 8192, 256, 49408 + 256, 32, 16, 256).to(dev)
            opt = optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01, device_step=name != "eager host-step")

            def eager(model=model, opt=opt):
                opt.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    loss = model.token_loss(text, seg, img)
                loss.backward()
                opt.step()
                return loss
            if name == "graphed":
                torch.cuda.synchronize(); t0 = time.perf_counter()
                step = graphs.GraphedTrainStep(lambda t, s, i, model=model: model.token_loss(t, s, i), opt, (text, seg, img),
                                               amp_dtype=torch.bfloat16, warmup=2, modules=[model])
                torch.cuda.synchronize()
                print(f"B={batch} graphed: 2 warm-up steps + capture {time.perf_counter() - t0:.2f} s", flush=True)
                cols[name] = lambda step=step: step(text, seg, img)
            else:
                eager(), eager()
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
        n_steps = {k: max(5, int(a.seconds / block(fn, 3, k == "graphed")[0])) for k, fn in cols.items()}
        times = {k: [] for k in cols}
        for _ in range(2):
            for k, fn in cols.items():
                dt, loss = block(fn, n_steps[k], k == "graphed")
                times[k].append(dt)
        for k in cols:
            best = min(times[k])
            print(f"MakeAScene {a.layers}L/1024d/16h S=1536 B={batch} bf16 training step, {k}: " + " / ".join(f"{t * 1e3:.2f}" for t in times[k])
                  + f" ms/step ({n_steps[k]} steps per block)  best {batch * 1536 / best:.0f} tokens/s", flush=True)
        del cols, model, opt, step
        torch.cuda.empty_cache()


if a.graph:
    graph_bench()
    sys.exit(0)
modes = a.loss.split(",")
if not modes or any(k not in ("aten", "fused", "model") for k in modes):
    ap.error("--loss: aten, fused, model or a comma-separated list of them")
dev = torch.device("cuda:0")
torch.manual_seed(0)
m = MakeAScene(a.layers, 1024, 16, 8192, 256, 49408 + 256, 32, 16, 256).to(dev)
text = torch.randint(1, 49408, (a.batch, 256), device=dev); text[:, 200:] = 0
seg = torch.randint(0, 256, (a.batch, 256), device=dev)
img = torch.randint(0, 8192, (a.batch, 1024), device=dev)
def step(mode="aten"):
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        if mode == "model":
            loss = m.token_loss(text, seg, img)
        else:
            logits = m(text, seg, img)
    if mode == "aten":
        loss = torch.nn.functional.cross_entropy(logits.float().reshape(-1, 8192), img.reshape(-1))
    elif mode == "fused":
        loss = ops.cross_entropy(logits, img)
    loss.backward()
    return loss
gf = 1185.4 * a.layers / 24 * 3 * a.batch
if modes == ["aten"]:
    for _ in range(2): step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(a.steps): loss = step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.steps
    print(f"MakeAScene {a.layers}L/1024d/16h S=1536 B={a.batch} bf16 fwd+bwd: {dt*1e3:.1f} ms/step  {a.batch*1536/dt:.0f} tokens/s  {gf/dt/1e3:.1f} TFLOP/s  loss {float(loss):.3f}")
else:
    for k in modes:
        for _ in range(2): step(k)
    spent, loss = {k: 0.0 for k in modes}, {}
    for _ in range(a.steps):                     # alternating, one step each: what else runs on the machine reaches every mode alike
        for k in modes:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            loss[k] = step(k)
            torch.cuda.synchronize(); spent[k] += time.perf_counter() - t0
    for k in modes:
        dt = spent[k] / a.steps
        print(f"MakeAScene {a.layers}L/1024d/16h S=1536 B={a.batch} bf16 fwd+bwd, loss={k}: {dt*1e3:.1f} ms/step  {a.batch*1536/dt:.0f} tokens/s  "
              f"{gf/dt/1e3:.1f} TFLOP/s (the model's count, not the logits rows computed)  loss {float(loss[k].detach()):.5f}")
