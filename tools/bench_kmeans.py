#!/usr/bin/env python3
"""The codebook re-initialisation's k-means in its two forms, from the same initial rows, in one process:

  host loop     models.kmeans.kmeans_fit(on_device=False) under torch.use_deterministic_algorithms(True, warn_only=True), exactly as
                Codebook._reinit_from_reservoir runs it in device-reservoir mode without device_kmeans: one host read per iteration
  device        ops.kmeans_fit (csrc/kmeans.hip): max_iter iterations enqueued, the stop test on the device, nothing read

The two alternate, each --repeats times (default 2), after one untimed fit each; the figure is device-synchronised wall time per WHOLE fit.
Shapes: conf/img_config.yaml's codebook (K = 8192, D = 256) and conf/seg_config.yaml's (K = 1024, D = 256) on the one-rank and the
eight-rank reservoir pool (M = 12 500 and 100 000), Gaussian rows (which run all max_iter iterations on both paths), and one blob-shaped
input that converges in a handful of iterations: there the device path is timed at max_iter = 100 and at max_iter = its iteration count,
and the difference prices the skipped tail (5 empty launches per skipped iteration)."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch
from mas_hip import ops
from models.kmeans import kmeans_fit

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--max-iter", type=int, default=100)
ap.add_argument("--shapes", default="8192:256:12500,8192:256:100000,1024:256:12500,1024:256:100000", help="K:D:M, comma separated")
a = ap.parse_args()
dev = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def host_loop(pts, k, init, max_iter):
    det, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        return kmeans_fit(pts, k, max_iter=max_iter, init_idx=init, return_info=True, on_device=False)
    finally:
        torch.use_deterministic_algorithms(det, warn_only=warn)


def run(label, pts, k, max_iter):
    m, d = pts.shape
    init = torch.randperm(m, generator=torch.Generator().manual_seed(1))[:k].to(dev)
    paths = {"host loop": lambda: host_loop(pts, k, init, max_iter),
             "device": lambda: ops.kmeans_fit(pts, k, init_idx=init, max_iter=max_iter)}
    times, iters = {n: [] for n in paths}, {}
    for n, fn in paths.items():
        fn()                                                   # untimed: code objects, the allocator
    for _ in range(a.repeats):
        for n, fn in paths.items():
            ms, out = timed(fn)
            times[n].append(ms)
            iters[n] = out[2] if isinstance(out[2], int) else int(out[2][0])      # (read after the clock stopped)
    same = torch.equal(paths["host loop"]()[1], paths["device"]()[1])
    for n in paths:
        best = min(times[n])
        print(f"{label:28s} K={k:5d} D={d:3d} M={m:6d}  {n:9s}  fits (ms): {' '.join(f'{t:9.2f}' for t in times[n])}   iterations {iters[n]:3d}   "
              f"{best / iters[n]:7.3f} ms/iteration", flush=True)
    print(f"{label:28s} device / host loop = {min(times['device']) / min(times['host loop']):.3f}; final assignments equal: {same}", flush=True)
    return iters["device"]


print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, max_iter {a.max_iter}, {a.repeats} timed fits per path, alternating", flush=True)
for shape in a.shapes.split(","):
    k, d, m = (int(v) for v in shape.split(":"))
    pts = torch.randn(m, d, generator=torch.Generator().manual_seed(0)).to(dev)
    run("gaussian", pts, k, a.max_iter)

# blobs: 1024 centres of 12 points each; converges in a handful of iterations
g = torch.Generator().manual_seed(2)
centres = 4.0 * torch.randn(1024, 256, generator=g)
pts = (centres[:, None] + 0.3 * torch.randn(1024, 12, 256, generator=g)).reshape(-1, 256)
pts = pts[torch.randperm(len(pts), generator=g)].contiguous().to(dev)
it = run("blobs", pts, 1024, a.max_iter)
init = torch.randperm(len(pts), generator=torch.Generator().manual_seed(1))[:1024].to(dev)
tail = {}
for mi in (a.max_iter, it) * a.repeats:
    ms, out = timed(lambda: ops.kmeans_fit(pts, 1024, init_idx=init, max_iter=mi))
    tail.setdefault(mi, []).append(ms)
full, cut = min(tail[a.max_iter]), min(tail[it])
skipped = a.max_iter - it
print(f"blobs, device path: max_iter={a.max_iter}: {full:.3f} ms; max_iter={it}: {cut:.3f} ms; the {skipped} skipped iterations "
      f"({5 * skipped} empty launches) cost {full - cut:.3f} ms = {1e3 * (full - cut) / max(1, 5 * skipped):.2f} us per launch", flush=True)
