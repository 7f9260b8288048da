#!/usr/bin/env python3
"""The optimizer step alone on BASELINE config 4's parameter set (MakeAScene 24 layers, D = 1024: 398 fp32 tensors, 370.7 M elements,
fp32 gradients), with and without global-norm clipping:

  a  torch.nn.utils.clip_grad_norm_(params, 1.0) + mas_hip.optim.Adam.step()      -- clipping in front of the one-launch Adam
  b  mas_hip.optim.Adam(max_grad_norm=1.0).step()                                 -- norm launch + coefficient launch + adam_multi_ex
  c  mas_hip.optim.Adam.step()                                                    -- no clipping

All three run in ONE process, alternating in rounds after a warm-up, each round a window of steps between two device events (wall time of
the device work, the host running ahead).  Printed per column: ms per step (median and spread over the rounds), the algorithmic bytes from
the shapes (c: 28 B per element -- read p, g, m, v, write p, m, v; b: + 4, one more read of g; a: + 12, g read twice and written once) and
GB/s of those bytes.  The gradients keep their storage from step to step (the item table is built once); column a scales them in place
at every step, as torch's function always does.  There is no fallback: without a GPU this fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402

CFG = dict(num_layers=24, hidden_dim=1024, num_attn_heads=16, image_vocab_size=8192, seg_vocab_size=256, text_vocab_size=49408 + 256,
           image_tokens_per_dim=32, seg_tokens_per_dim=16, text_length=256)        # bench.py's TR_CFG
BYTES_PER_ELEMENT = {"a": 28 + 12, "b": 28 + 4, "c": 28}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=CFG["num_layers"])
    ap.add_argument("--seconds", type=float, default=1.5, help="timed window per column (at least), split over the rounds")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_clip_bench: no GPU found (there is no CPU path to time)")
    from mas_hip.optim import Adam
    from models.transformer import MakeAScene
    dev = torch.device("cuda:0")
    with torch.device("meta"):                       # the shapes only: the values are irrelevant to the step's time
        shapes = [tuple(p.shape) for p in MakeAScene(**dict(CFG, num_layers=a.layers)).parameters()]
    gen = torch.Generator(device=dev).manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    n = sum(p.numel() for p in params)
    plain, clipping = Adam(params, lr=1e-4), Adam(params, lr=1e-4, max_grad_norm=1.0)

    def step_a():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        plain.step()

    cols = {"a": step_a, "b": clipping.step, "c": plain.step}
    calls = {}
    for name, fn in cols.items():                    # warm-up (state, tables, code objects), then the step count of a round
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            fn()
        e1.record()
        torch.cuda.synchronize()
        calls[name] = max(3, int(a.seconds / a.rounds / (e0.elapsed_time(e1) / 5 * 1e-3)) + 1)
    ms = {name: [] for name in cols}
    for _ in range(a.rounds):
        for name, fn in cols.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / calls[name])
    print(f"optimizer step, {len(params)} fp32 tensors, {n / 1e6:.1f} M elements, >= {a.seconds:g} s per column in {a.rounds} alternating rounds")
    print(f"grad norm {float(clipping.grad_norm):.6g}, clip coefficient {float(clipping.clip_coef):.6g}")
    print(f"{'column':40} {'steps':>6} {'ms':>8} {'min..max':>15} {'alg MB':>9} {'GB/s':>8}")
    label = {"a": "a clip_grad_norm_ + Adam", "b": "b Adam(max_grad_norm=1.0)", "c": "c Adam"}
    for name in cols:
        med, nbytes = statistics.median(ms[name]), BYTES_PER_ELEMENT[name] * n
        print(f"{label[name]:40} {calls[name]:6d} {med:8.3f} {min(ms[name]):7.3f}..{max(ms[name]):<7.3f} {nbytes / 1e6:9.1f} {nbytes / med / 1e6:8.1f}")
    med = {name: statistics.median(v) for name, v in ms.items()}
    print(f"b / a = {med['b'] / med['a']:.3f}, b / c = {med['b'] / med['c']:.3f}, b - c = {med['b'] - med['c']:.3f} ms "
          f"(one read of the gradients: {4 * n / 1e6:.1f} MB)")


if __name__ == "__main__":
    main()
