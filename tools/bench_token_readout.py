#!/usr/bin/env python3
"""The stage-2 validation read-out alone at BASELINE config 4's shape: 8192 rows x 8192 classes, bf16 and fp32 logits, as the contiguous
matrix and as the [8, 1024, V] slice of [8, 1536, V] that ``MakeAScene.forward`` returns.

  aten  : what a validation loop writes without this kernel -- log_softmax on logits.float(), the gather of the target's log-probability,
          argmax, (x > x_t).sum(-1) plus the tie term for the rank, and the entropy -sum p log p
  fused : mas_hip.ops.token_readout(logits, target)                                  (csrc/token_readout.hip)
  accum : mas_hip.ops.token_agreement(logits, target, out=acc): the same read plus the per-position accumulation launch

The paths run in ONE process, alternating in rounds after a warm-up, each round a window of calls between two device events of at least
``--seconds``; the median over the rounds is reported.  Printed per path: ms per call (median and spread), the algorithmic bytes (ONE read
of the logits in their dtype, the targets and the four per-row results), GB/s of those bytes and their share of the 6.3 TB/s this project
counts with, and the peak memory above the inputs.  There is no fallback: without a GPU this fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402

PEAK_GBS = 6300.0


def aten_readout(x, t):
    """-> (nll, entropy, rank, argmax) with ATen alone"""
    v = x.shape[-1]
    xf = x.float().reshape(-1, v)
    tt = t.reshape(-1, 1)
    logp = torch.log_softmax(xf, dim=-1)
    nll = -logp.gather(1, tt).squeeze(1)
    arg = xf.argmax(-1)
    xt = xf.gather(1, tt)
    cols = torch.arange(v, device=x.device)
    rank = (xf > xt).sum(-1) + ((xf == xt) & (cols < tt)).sum(-1)
    ent = -torch.where(torch.isneginf(logp), torch.zeros_like(logp), logp.exp() * logp).sum(-1)
    return nll, ent, rank, arg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--classes", type=int, default=8192)
    ap.add_argument("--seconds", type=float, default=0.2, help="timed window per path, configuration and round (at least)")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_readout: no GPU found (there is no CPU path to time)")
    from mas_hip import ops
    from mas_hip.tokenmetrics import TokenAgreement
    dev = torch.device("cuda:0")
    rows, v = a.rows, a.classes
    b, length, s = 8, rows // 8, rows // 8 * 3 // 2
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.randint(0, v, (rows,), device=dev, generator=gen)
    acc = TokenAgreement(length, (1, 5), device=dev)
    paths = {"aten": aten_readout,
             "fused": lambda x, t: ops.token_readout(x, t),
             "accum": lambda x, t: ops.token_agreement(x, t, positions=length, ks=(1, 5), out=acc).tensors()}
    print(f"token read-out, {rows} rows x {v} classes, {a.rounds} alternating rounds of >= {a.seconds:g} s per path")
    print(f"{'dtype':5} {'input':7} {'path':5} {'ms':>8} {'min..max':>15} {'alg MB':>8} {'GB/s':>8} {'of peak':>8} {'peak MB':>8} {'top-1':>7}")
    with torch.no_grad():
        for dtype in (torch.bfloat16, torch.float32):
            for layout in ("contig", "slice"):
                if layout == "contig":
                    x = torch.randn((rows, v), device=dev, generator=gen).to(dtype)
                    tgt = target
                else:
                    x = torch.randn((b, s, v), device=dev, generator=gen).to(dtype)[:, -length - 1:-1, :]
                    tgt = target.view(b, length)
                calls, peak, top1 = {}, {}, {}
                for name, fn in paths.items():                   # warm-up, the call count of a round, the peak memory of one call
                    for _ in range(3):
                        fn(x, tgt)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(5):
                        fn(x, tgt)
                    e1.record()
                    torch.cuda.synchronize()
                    calls[name] = max(3, int(a.seconds / (e0.elapsed_time(e1) / 5 * 1e-3)) + 1)
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    out = fn(x, tgt)
                    torch.cuda.synchronize()
                    peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                    top1[name] = float((out[2] == 0).double().mean()) if name != "accum" else float("nan")
                    del out
                ms = {name: [] for name in paths}
                for _ in range(a.rounds):
                    for name, fn in paths.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(calls[name]):
                            fn(x, tgt)
                        e1.record()
                        torch.cuda.synchronize()
                        ms[name].append(e0.elapsed_time(e1) / calls[name])
                nbytes = rows * v * x.element_size() + rows * (8 + 4 * 4)
                for name in paths:
                    med = statistics.median(ms[name])
                    gbs = nbytes / med / 1e6
                    print(f"{str(dtype)[6:]:5} {layout:7} {name:5} {med:8.3f} {min(ms[name]):7.3f}..{max(ms[name]):<7.3f} {nbytes / 1e6:8.1f} "
                          f"{gbs:8.1f} {100 * gbs / PEAK_GBS:7.1f}% {peak[name]:8.1f} {top1[name]:7.4f}")
                ratio = statistics.median(ms["aten"]) / statistics.median(ms["fused"])
                print(f"{'':5} {'':7} aten / fused = {ratio:.2f}x" + ("" if ratio >= 1.0 else "   (this row LOSES to ATen)"))
                del x
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
