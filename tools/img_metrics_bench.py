#!/usr/bin/env python3
"""The VQ-IMG read-out (csrc/img_metrics.hip) measured on one GPU against the way the same numbers could be had before: the
metric written in ATen.  Both in ONE process, alternating in rounds after a warm-up, each round a window of calls between two device
events.

  aten : ``((x - lo) * s).clamp(0, 255).round().to(uint8)`` for both images, the squared error of the bytes in int64, and SSIM from five
         grouped ``F.conv2d`` maps (11 x 11 Gaussian window, "valid") in fp64
  op   : ``ops.image_agreement`` -- two byte launches, the tile kernel, the reduce

Row: [32, 3, 256, 256], a bf16 channels_last reconstruction against an fp32 NCHW target (what ``VQBASE.reconstruction_metrics`` hands
over).  Per path: ms per call (median, min..max over the rounds = the spread of repeated runs of the same code) and peak memory above the
inputs; the two paths' squared errors are asserted equal and their SSIM within 1e-9.  Then ``ops.image_bytes`` alone on both inputs and
``ops.code_usage`` on [32, 256] indices of an 8192-entry codebook (the workload's tokens) and on 2^22 indices.

There is no fallback: without a GPU this fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def aten_bytes(x, lo, hi):
    s = torch.tensor(255.0 / (hi - lo), dtype=torch.float32).item()
    return ((x.float() - lo) * s).clamp(0, 255).round().to(torch.uint8)             # [N, C, H, W]


def aten_agreement(a, b, lo, hi, window):
    pa, pb = aten_bytes(a, lo, hi), aten_bytes(b, lo, hi)
    d = pa.long() - pb.long()
    sse = (d * d).flatten(1).sum(1)
    fa, fb = pa.double(), pb.double()
    c = fa.shape[1]
    w2 = torch.outer(window, window).expand(c, 1, 11, 11).contiguous()
    ma, mb = F.conv2d(fa, w2, groups=c), F.conv2d(fb, w2, groups=c)
    va = F.conv2d(fa * fa, w2, groups=c) - ma * ma
    vb = F.conv2d(fb * fb, w2, groups=c) - mb * mb
    vab = F.conv2d(fa * fb, w2, groups=c) - ma * mb
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    m = ((2 * ma * mb + c1) * (2 * vab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
    return sse, m.flatten(1).mean(1)


def _alternate(paths, seconds, rounds):
    calls, peak = {}, {}
    for name, call in paths.items():
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(2):
            call()
        e1.record()
        torch.cuda.synchronize()
        calls[name] = max(2, int(seconds / rounds / (e0.elapsed_time(e1) / 2 * 1e-3)) + 1)
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        call()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    ms = {name: [] for name in paths}
    for _ in range(rounds):
        for name, call in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[name]):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / calls[name])
    return ms, peak


def _row(name, v, extra=""):
    med = statistics.median(v)
    return f"    {name:12} {med:9.4f} {min(v):9.4f}..{max(v):<9.4f} spread {100 * (max(v) - min(v)) / med:5.1f}% {extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per path (at least)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("img_metrics_bench: medians of at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("img_metrics_bench: no GPU found (there is no CPU path to time)")
    from mas_hip import ops
    from mas_hip.imgmetrics import ssim_window
    dev = torch.device("cuda:0")
    n, s = a.batch, a.size
    print(f"VQ-IMG read-out (csrc/img_metrics.hip) against the ATen expression; >= {a.seconds:g} s per path in {a.rounds} alternating "
          f"rounds; {torch.cuda.get_device_name(0)}")
    gen = torch.Generator(device=dev).manual_seed(7)
    target = (torch.rand((n, 3, s, s), device=dev, generator=gen) * 2.2 - 1.1)                                   # fp32 NCHW
    rec = (target + 0.05 * torch.randn((n, 3, s, s), device=dev, generator=gen)).bfloat16().contiguous(memory_format=torch.channels_last)
    window = torch.tensor(ssim_window(), dtype=torch.float64, device=dev)
    lo, hi = -1.0, 1.0
    out = {}
    paths = {"aten": lambda: out.__setitem__("aten", aten_agreement(rec, target, lo, hi, window)),
             "op": lambda: out.__setitem__("op", ops.image_agreement(rec, target, lo, hi))}
    ms, peak = _alternate(paths, a.seconds, a.rounds)
    sse_a, ssim_a = out["aten"]
    got = out["op"]
    err = float((got.ssim - ssim_a).abs().max())
    # ATen's (x - lo) * s may be contracted or not by its own kernels; the squared errors are compared, and reported if they differ
    same_sse = bool(torch.equal(got.sse, sse_a))
    print(f"image_agreement [{n}, 3, {s}, {s}] bf16 channels_last reconstruction vs fp32 NCHW target: squared errors equal: {same_sse}; "
          f"|ssim op - ssim aten| max {err:.3e}; mean ssim {float(got.mean_ssim):.6f}, mean psnr {float(got.mean_psnr):.3f} dB")
    assert same_sse and err < 1e-9, "the op and the ATen expression disagree"
    print(f"    {'path':12} {'ms':>9} {'min..max':>20}")
    for name in ("aten", "op"):
        print(_row(name, ms[name], f"peak {peak[name] / 2 ** 20:8.1f} MB above the inputs"))
    ma, mo = statistics.median(ms["aten"]), statistics.median(ms["op"])
    gap = min(ms["aten"]) - max(ms["op"])
    print(f"    aten / op = {ma / mo:.2f}x; slowest op round against fastest aten round: {max(ms['op']):.4f} vs {min(ms['aten']):.4f} ms "
          f"({'op faster beyond the spread' if gap > 0 else 'NOT faster beyond the spread'})")
    out.clear()

    parts = {"bytes bf16 cl": lambda: ops.image_bytes(rec, lo, hi), "bytes fp32": lambda: ops.image_bytes(target, lo, hi)}
    pa, pb = ops.image_bytes(rec, lo, hi), ops.image_bytes(target, lo, hi)
    parts["pictures"] = lambda: ops.image_agreement(pa, pb)
    ms, peak = _alternate(parts, a.seconds / 2, a.rounds)
    print("the parts (image_bytes of each input; image_agreement on two uint8 pictures = tile kernel + reduce):")
    for name in parts:
        print(_row(name, ms[name], f"peak {peak[name] / 2 ** 20:8.1f} MB"))

    k = 8192
    for count, shape in ((n * 256, (n, 256)), (1 << 22, (1 << 22,))):
        idx = torch.randint(0, k, shape, device=dev, generator=gen)
        acc = ops.code_usage(idx, k)
        paths = {"bincount": lambda: torch.bincount(idx.flatten(), minlength=k), "op": lambda: ops.code_usage(idx, k, out=acc)}
        ms, peak = _alternate(paths, a.seconds / 2, a.rounds)
        assert torch.equal(ops.code_usage(idx, k).per_code, torch.bincount(idx.flatten(), minlength=k))
        print(f"code_usage, {count} int64 indices, K = {k} (torch.bincount synchronises with the host to size its output; the op does not):")
        for name in paths:
            print(_row(name, ms[name], f"peak {peak[name] / 2 ** 20:8.1f} MB"))


if __name__ == "__main__":
    main()
