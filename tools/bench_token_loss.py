#!/usr/bin/env python3
"""The stage-2 loss alone at BASELINE config 4's shape: 8192 rows x 8192 classes, forward + backward, bf16 and fp32 logits, as the
contiguous matrix and as the [8, 1024, V] slice of [8, 1536, V] that ``MakeAScene.forward`` returns.

  aten  : the line bench.py and tools/bench_transformer.py time -- F.cross_entropy(logits.float().reshape(-1, V), target)
  fused : mas_hip.ops.cross_entropy(logits, target)                                    (csrc/token_loss.hip)

Both paths run in ONE process, alternating in rounds after a warm-up, each round a window of calls between two device events; the
rounds of a path add up to at least ``--seconds``.  The gradient with respect to the tensor the model produced (the full [8, 1536, V]
one for the slice) is part of both paths.  Printed per path: ms per call (median and spread over the rounds), the algorithmic bytes
from the shapes (forward: one read of the logits; backward: one read and one write of the gradient in the logits' dtype), GB/s of
those bytes, and the peak memory above the inputs.  There is no fallback: without a GPU this fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def algorithmic_bytes(rows, v, esize):
    """what the operation needs: the logits read once forward, read once and the gradient written once backward (+ targets, row stats)"""
    return 3 * rows * v * esize + rows * (8 * 2 + 4 * 3 * 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--classes", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per path and configuration (at least)")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_loss: no GPU found (there is no CPU path to time)")
    from mas_hip import ops
    dev = torch.device("cuda:0")
    rows, v = a.rows, a.classes
    b, length, s = 8, rows // 8, rows // 8 * 3 // 2
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.randint(0, v, (rows,), device=dev, generator=gen)
    paths = {"aten": lambda x, t: F.cross_entropy(x.float().reshape(-1, v), t.reshape(-1)),
             "fused": lambda x, t: ops.cross_entropy(x, t)}
    print(f"token loss fwd+bwd, {rows} rows x {v} classes, >= {a.seconds:g} s per path in {a.rounds} alternating rounds")
    print(f"{'dtype':5} {'input':7} {'path':5} {'ms':>8} {'min..max':>15} {'alg MB':>8} {'GB/s':>8} {'peak MB':>8} {'loss':>9}")
    for dtype in (torch.bfloat16, torch.float32):
        for layout in ("contig", "slice"):
            if layout == "contig":
                leaf = torch.randn((rows, v), device=dev, generator=gen).to(dtype).requires_grad_(True)
                view, tgt = (lambda: leaf), target
            else:
                leaf = torch.randn((b, s, v), device=dev, generator=gen).to(dtype).requires_grad_(True)
                view, tgt = (lambda: leaf[:, -length - 1:-1, :]), target.view(b, length)

            def call(fn):
                leaf.grad = None
                loss = fn(view(), tgt)
                loss.backward()
                return loss

            calls, peak, last = {}, {}, {}
            for name, fn in paths.items():                       # warm-up, the call count of a round, the peak memory of one call
                for _ in range(3):
                    call(fn)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    call(fn)
                e1.record()
                torch.cuda.synchronize()
                calls[name] = max(3, int(a.seconds / a.rounds / (e0.elapsed_time(e1) / 5 * 1e-3)) + 1)
                leaf.grad = None
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                last[name] = float(call(fn).detach())
                torch.cuda.synchronize()
                peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            ms = {name: [] for name in paths}
            for _ in range(a.rounds):
                for name, fn in paths.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls[name]):
                        call(fn)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / calls[name])
            nbytes = algorithmic_bytes(rows, v, leaf.element_size())
            for name in paths:
                med = statistics.median(ms[name])
                print(f"{str(dtype)[6:]:5} {layout:7} {name:5} {med:8.3f} {min(ms[name]):7.3f}..{max(ms[name]):<7.3f} {nbytes / 1e6:8.1f} "
                      f"{nbytes / med / 1e6:8.1f} {peak[name]:8.1f} {last[name]:9.5f}")
            print(f"{'':5} {'':7} aten / fused = {statistics.median(ms['aten']) / statistics.median(ms['fused']):.2f}x")
            del leaf
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
