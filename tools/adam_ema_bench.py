#!/usr/bin/env python3
"""The optimizer step with an EMA of the weights on the VQ-IMG parameter set (VQBASE at conf/img_config.yaml's sizes: 95 M fp32 elements),
fused against bolted on:

  a  mas_hip.optim.Adam(ema_decay=0.999).step()                                -- mas_adam_multi_ema: the EMA inside the Adam launch
  b  mas_hip.optim.Adam().step() + torch._foreach_lerp_(emas, params, 0.001)   -- the EMA as a pass of its own after the step
  c  mas_hip.optim.Adam().step()                                               -- no EMA

All columns run in ONE process, alternating in rounds after a warm-up, each round a window of steps between two device events.  The host
part of a step over 345 tensors (1.7 ms of Python) is longer than its device part, so each window is issued behind a calibrated spin kernel
(torch.cuda._sleep) that holds the device until the host has queued the whole window: the events then bracket device time alone
(--no-ahead times the calls as they come, host included).  Printed per
column: ms per step (median and spread over the rounds), the algorithmic bytes from the shapes (c: 28 B per element; a: + 8, one read and one
write of the EMA; b: + 12, the parameter read a second time) and GB/s of those bytes.  The gradients keep their storage (the item table is
built once).  --step times the same a and b over bench.py's VQ step (forward, backward, optimizer, zero_grad) at --batch.
There is no fallback: without a GPU this fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402

IMG_CFG = dict(ddconfig=dict(z_channels=256, in_channels=3, out_channels=3, channels=[128, 128, 128, 256, 512, 512], num_res_blocks=2,
                             resolution=512, attn_resolutions=[32], dropout=0.0),
               n_embed=8192, embed_dim=256, init_steps=3000, reservoir_size=12500)        # bench.py's IMG_CFG
BYTES_PER_ELEMENT = {"a": 28 + 8, "b": 28 + 12, "c": 28}
LABEL = {"a": "a Adam(ema_decay=0.999)", "b": "b Adam + _foreach_lerp_", "c": "c Adam"}
DECAY = 0.999


_SPIN = {}            # spin-kernel cycles per millisecond, measured once


def _hold_device(ms):
    """keeps the device busy for about `ms` milliseconds while the host queues work behind it"""
    if "rate" not in _SPIN:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000000)
        e0.record()
        torch.cuda._sleep(10000000)
        e1.record()
        torch.cuda.synchronize()
        _SPIN["rate"] = 10000000 / e0.elapsed_time(e1)
    torch.cuda._sleep(int(ms * _SPIN["rate"]))


def _window(fn, calls, ahead_ms=0.0):
    """ms per call between two device events; ahead_ms > 0: issued behind a spin of that length, so the device never waits for the host"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if ahead_ms > 0.0:
        _hold_device(ahead_ms)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def _rounds(cols, seconds, rounds, warm=3, ahead=False):
    calls, host = {}, {}
    for name, fn in cols.items():                    # warm-up (state, tables, code objects), then the step count of a round
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_call = _window(fn, 5)
        host[name] = (time.perf_counter() - t0) / 5 * 1e3          # an upper bound of the host's time per call
        calls[name] = max(3, int(seconds / rounds / (per_call * 1e-3)) + 1)
        if ahead:
            calls[name] = min(calls[name], 40)       # the spin covers the whole window's host time: keep it to a fraction of a second
    ms = {name: [] for name in cols}
    for _ in range(rounds):
        for name, fn in cols.items():
            ms[name].append(_window(fn, calls[name], 1.5 * host[name] * calls[name] if ahead else 0.0))
    return ms, calls


def optimizer_alone(a):
    from mas_hip.optim import Adam
    from models import VQBASE
    dev = torch.device("cuda:0")
    shapes = [tuple(p.shape) for p in VQBASE(**IMG_CFG).parameters()]           # the shapes only: the values are irrelevant to the step's time
    gen = torch.Generator(device=dev).manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    n = sum(p.numel() for p in params)
    fused, plain = Adam(params, lr=5e-6, betas=(0.5, 0.9), ema_decay=DECAY), Adam(params, lr=5e-6, betas=(0.5, 0.9))
    emas, datas = [p.detach().clone() for p in params], [p.detach() for p in params]

    def step_b():
        plain.step()
        torch._foreach_lerp_(emas, datas, 1.0 - DECAY)

    cols = {"a": fused.step, "b": step_b, "c": plain.step}
    ms, calls = _rounds(cols, a.seconds, a.rounds, ahead=not a.no_ahead)
    print(f"optimizer step, {len(params)} fp32 tensors, {n / 1e6:.1f} M elements, {a.rounds} alternating rounds, "
          f"{'host time included' if a.no_ahead else 'device time (windows queued behind a spin kernel)'}")
    print(f"{'column':40} {'steps':>6} {'ms':>8} {'min..max':>15} {'alg MB':>9} {'GB/s':>8}")
    for name in cols:
        med, nbytes = statistics.median(ms[name]), BYTES_PER_ELEMENT[name] * n
        print(f"{LABEL[name]:40} {calls[name]:6d} {med:8.3f} {min(ms[name]):7.3f}..{max(ms[name]):<7.3f} {nbytes / 1e6:9.1f} {nbytes / med / 1e6:8.1f}")
    med = {name: statistics.median(v) for name, v in ms.items()}
    print(f"a / b = {med['a'] / med['b']:.3f}, a - c = {med['a'] - med['c']:.3f} ms, b - c = {med['b'] - med['c']:.3f} ms "
          f"(one read and one write of the EMA: {8 * n / 1e6:.1f} MB)")


def whole_step(a):
    from mas_hip import ops
    from mas_hip.optim import Adam
    from models import VQBASE
    dev = torch.device("cuda:0")
    ops.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = VQBASE(**IMG_CFG)
    with torch.no_grad():
        model.quantize.embedding.weight.normal_(0.0, 1.0)
    model = model.to(dev).train()
    model.quantize.q_counter = model.quantize.q_re_end
    x = torch.rand(a.batch, 3, 256, 256, generator=torch.Generator().manual_seed(1234)).to(dev)
    params = list(model.parameters())
    fused, plain = Adam(params, lr=5e-6, betas=(0.5, 0.9), ema_decay=DECAY), Adam(params, lr=5e-6, betas=(0.5, 0.9))
    emas = [p.detach().clone() for p in params]

    def step(opt, lerp):
        rec, q = model(x)
        ((x - rec).abs().mean() + q).backward()
        opt.step()
        if lerp:
            with_grad = [(e, p.detach()) for e, p in zip(emas, params) if p.grad is not None]
            torch._foreach_lerp_([e for e, _ in with_grad], [p for _, p in with_grad], 1.0 - DECAY)
        opt.zero_grad(set_to_none=True)

    cols = {"a": lambda: step(fused, False), "b": lambda: step(plain, True), "c": lambda: step(plain, False)}
    ms, calls = _rounds(cols, a.seconds, a.rounds, warm=6)
    print(f"bench.py's VQ step (VQ-IMG 256x256, batch {a.batch}, bf16), >= {a.seconds:g} s per column in {a.rounds} alternating rounds")
    print(f"{'column':40} {'steps':>6} {'ms':>8} {'min..max':>15}")
    for name in cols:
        print(f"{LABEL[name]:40} {calls[name]:6d} {statistics.median(ms[name]):8.3f} {min(ms[name]):7.3f}..{max(ms[name]):<7.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.5, help="timed window per column (at least), split over the rounds")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="time the whole VQ training step instead of the optimizer alone")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-ahead", action="store_true", help="optimizer alone: do not hold the device while the host queues a window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_ema_bench: no GPU found (there is no CPU path to time)")
    (whole_step if a.step else optimizer_alone)(a)


if __name__ == "__main__":
    main()
