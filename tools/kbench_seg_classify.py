#!/usr/bin/env python3
"""VQ-SEG logits -> label planes (csrc/seg_classify.hip) measured on one GPU against the only way the same labels could be
had before: the reference Visualizer's expression (log_utils.py:55-67) in ATen, applied per group to the same tensor.  Both in ONE
process, alternating in rounds after a warm-up, each round a window of calls between two device events.

  aten : per group a slice ``argmax`` (an int64 map), for the gated groups ``sigmoid`` of the slice, ``> 0.2``, the mask gathered at the
         argmax, and the label packed to uint8; the four planes stacked
  op   : ``ops.seg_classify`` -- one kernel, the prediction read once

Rows: [32, 159, 256, 256] (the workload) and B = 1, fp32 and bf16, NCHW and channels_last.  Per row: ms per call (median, min..max over
the rounds = the spread of repeated runs of the same code), GB/s on the algorithmic bytes (the prediction once plus the planes) and its
share of the 6.3 TB/s taken as achievable, peak memory above the input, and whether the two paths' bytes are equal (asserted).  Then
``ops.seg_agreement`` on [32, 4, 256, 256] planes.

There is no fallback: without a GPU this fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402

ACHIEVABLE_HBM_GBS = 6300.0          # float4 copy on this part (8 TB/s on paper)
GROUPS = ((0, 133, None), (133, 153, None), (153, 158, 0.2), (158, 159, 0.2))


def aten_labels(x):
    planes = []
    for lo, hi, t in GROUPS:
        seg = x[:, lo:hi]
        a = torch.argmax(seg, dim=1, keepdim=True)
        label = a + 1
        if t is not None:
            mask = seg.sigmoid() > t
            label = label * mask.gather(1, a)
        planes.append(label.to(torch.uint8))
    return torch.cat(planes, 1)


def _alternate(paths, seconds, rounds, clear):
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
        clear()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        call()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        clear()
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
    return f"    {name:6} {med:9.4f} {min(v):9.4f}..{max(v):<9.4f} spread {100 * (max(v) - min(v)) / med:5.1f}% {extra}"


def classify(dev, a, b, dtype, nhwc):
    from mas_hip import ops
    gen = torch.Generator(device=dev).manual_seed(5 + b)
    x = (2.0 * torch.randn((b, 256, 256, 159), device=dev, generator=gen)).to(dtype).permute(0, 3, 1, 2)
    x[:, 153:158] -= 3.0                                         # face: "none" and every class occur
    if not nhwc:
        x = x.contiguous()
    out = {}
    paths = {"aten": lambda: out.__setitem__("aten", aten_labels(x)), "op": lambda: out.__setitem__("op", ops.seg_classify(x).planes)}
    ms, peak = _alternate(paths, a.seconds, a.rounds, out.clear)
    paths["aten"]()
    paths["op"]()
    # the two can differ only where the fp32 (bf16) sigmoid of a logit next to tau = log(0.25) lands on the other side of 0.2
    tau = -1.3862943611198906
    near = ((x[:, 153:].float() - tau).abs() < (1e-2 if dtype == torch.float32 else 3e-2)).any(1, keepdim=True)
    diff = out["aten"] != out["op"]
    diff[:, 2:] &= ~near
    same = not bool(diff.any())
    assert same, "the op and the ATen expression disagree away from the threshold"
    exact = bool(torch.equal(out["aten"], out["op"]))
    nb = x.numel() * x.element_size() + out["op"].numel()
    print(f"seg_classify [{b}, 159, 256, 256] {str(dtype)[6:]} {'channels_last' if nhwc else 'NCHW'}: {nb / 1e6:.1f} MB algorithmic "
          f"(prediction once + planes); same bytes out: {same} (every byte, the threshold's neighbourhood included: {exact})")
    print(f"    {'path':6} {'ms':>9} {'min..max':>20}")
    for name in ("aten", "op"):
        rate = nb / statistics.median(ms[name]) / 1e6
        print(_row(name, ms[name], f"peak {peak[name] / 2 ** 20:8.1f} MB  {rate:7.1f} GB/s = {100 * rate / ACHIEVABLE_HBM_GBS:5.1f}% of 6.3 TB/s"))
    ma, mo = statistics.median(ms["aten"]), statistics.median(ms["op"])
    gap = min(ms["aten"]) - max(ms["op"])
    print(f"    aten / op = {ma / mo:.2f}x; slowest op round against fastest aten round: {max(ms['op']):.4f} vs {min(ms['aten']):.4f} ms "
          f"({'op faster beyond the spread' if gap > 0 else 'NOT separated'})")
    out.clear()
    return gap > 0


def agreement(dev, a):
    from mas_hip import ops
    from mas_hip.seglabels import SegAgreement, SegLabels
    gen = torch.Generator().manual_seed(3)
    mk = lambda: SegLabels(torch.stack([torch.randint(0, g + 1, (32, 256, 256), generator=gen, dtype=torch.uint8)
                                        for g in (133, 20, 5, 2)], 1).contiguous()).to(dev)
    p, t = mk(), mk()
    acc = SegAgreement(p.layout, device=dev)
    ms, peak = _alternate({"op": lambda: ops.seg_agreement(p, t, out=acc)}, a.seconds, a.rounds, lambda: None)
    nb = 2 * p.planes.numel()
    print(f"seg_agreement [32, 4, 256, 256] x 2 ({nb / 1e6:.1f} MB read), accumulating into one buffer:")
    print(_row("op", ms["op"], f"peak {peak['op'] / 2 ** 20:8.1f} MB  {nb / statistics.median(ms['op']) / 1e6:7.1f} GB/s"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per path and configuration (at least)")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("kbench_seg_classify: medians of at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("kbench_seg_classify: no GPU found (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    print(f"VQ-SEG logits -> label planes (csrc/seg_classify.hip) against the ATen expression; >= {a.seconds:g} s per path in {a.rounds} "
          f"alternating rounds; {torch.cuda.get_device_name(0)}")
    gate = None
    for b in (32, 1):
        for dtype in (torch.float32, torch.bfloat16):
            for nhwc in (False, True):
                ok = classify(dev, a, b, dtype, nhwc)
                if b == 32 and dtype == torch.float32 and not nhwc:
                    gate = ok
                torch.cuda.empty_cache()
    agreement(dev, a)
    print(f"acceptance ([32, 159, 256, 256] fp32 NCHW: the op faster than the ATen path by more than the spread): {'PASS' if gate else 'FAIL'}")
    if not gate:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
