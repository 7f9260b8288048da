#!/usr/bin/env python3
"""The VQ-SEG objective (losses.VQVAEWithBCELoss) measured on one GPU, the torch expression against the fused kernels of
csrc/seg_loss.hip, both in ONE process, alternating in rounds after a warm-up, each round a window of calls between two device events.

  torch : MAS_SEG_LOSS=0 -- sigmoid, mse_loss and binary_cross_entropy_with_logits(pos_weight) as ATen launches (the code before the kernels)
  hip   : mas_hip.ops.seg_loss, which the same module calls by default

 (a) the loss alone, forward + backward, [B, 159, 256, 256] for B = 8 and 32, fp32 channels_last prediction (what the decoder's last
     convolution writes), fp32 NCHW target (what the dataloader delivers): ms per call (median, min..max over the rounds = the spread of
     repeated runs of the same code), peak memory above the inputs, and the algorithmic bytes -- 8 per element forward (read x, read t),
     12 backward (read x, read t, write dx) -- per second, as a share of the 6.3 TB/s a streaming kernel reaches on this part;
     and B = 32 once more with an NCHW prediction (what this repository's decoder returns: the same-layout kernel);
 (b) one VQ-SEG training step at B = 8: VQBASE at conf/seg_config.yaml's widths on 256 x 256 maps, forward, loss, backward,
     mas_hip.optim.Adam, with either loss path;
 (c) one B = 64 evaluation of the loss alone (2.67 GB per tensor: offsets past 2^31 bytes in all three tensors), checked against the
     two B = 32 halves: the loss is their mean, the gradient exactly half of theirs.

There is no fallback: without a GPU this fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402

ACHIEVABLE_HBM_GBS = 6300.0          # float4 copy on this part (8 TB/s on paper)
SEG_CFG = dict(ddconfig=dict(z_channels=256, in_channels=159, out_channels=159, channels=[128, 128, 128, 256, 512, 512],
                             num_res_blocks=2, resolution=256, attn_resolutions=[16], dropout=0.0),
               n_embed=256, embed_dim=256, init_steps=3000, reservoir_size=12500)    # conf/seg_config.yaml:13-32


def _inputs(b, dev, seed, nhwc=True):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = (2.0 * torch.randn((b, 256, 256, 159), device=dev, generator=gen)).permute(0, 3, 1, 2)          # channels_last memory
    if not nhwc:
        x = x.contiguous()                                                                              # NCHW memory, the same values
    t = (torch.rand((b, 159, 256, 256), device=dev, generator=gen) < 0.3).float()                       # NCHW memory
    assert x.is_contiguous(memory_format=torch.channels_last) == nhwc and t.is_contiguous()
    return x, t


def _set_path(name):
    if name == "torch":
        os.environ["MAS_SEG_LOSS"] = "0"
    else:
        os.environ.pop("MAS_SEG_LOSS", None)


def _alternate(paths, call, seconds, rounds):
    """-> {path: [ms per call, one per round]}, {path: peak bytes of one call above what was allocated before it}, {path: last value}"""
    calls, peak, last = {}, {}, {}
    for name in paths:
        _set_path(name)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            call()
        e1.record()
        torch.cuda.synchronize()
        calls[name] = max(3, int(seconds / rounds / (e0.elapsed_time(e1) / 3 * 1e-3)) + 1)
        call(clear=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        last[name] = float(call().detach())
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    ms = {name: [] for name in paths}
    for _ in range(rounds):
        for name in paths:
            _set_path(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[name]):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / calls[name])
    _set_path("hip")
    return ms, peak, last


def loss_alone(b, lf, dev, a, nhwc=True):
    from mas_hip import ops
    x, t = _inputs(b, dev, b, nhwc)
    x.requires_grad_(True)
    q = torch.zeros((), device=dev)
    state = {}

    def call(clear=False):
        x.grad = None
        if clear:
            return None
        loss = lf(q, t, x)
        loss.backward()
        state["loss"] = loss
        return loss

    ms, peak, last = _alternate(("torch", "hip"), call, a.seconds, a.rounds)
    n = x.numel()
    print(f"(a) loss alone, fwd + bwd, [{b}, 159, 256, 256] fp32 {'NHWC' if nhwc else 'NCHW'} prediction, fp32 NCHW target: {n / 1e6:.1f} M elements, "
          f"{4 * n / 1e9:.2f} GB per tensor, algorithmic {20 * n / 1e9:.2f} GB (8 + 12 B / element)")
    print(f"    {'path':6} {'ms':>8} {'min..max':>17} {'peak MB':>9} {'alg GB/s':>9} {'of 6.3 TB/s':>11} {'loss':>10}")
    for name in ("torch", "hip"):
        med = statistics.median(ms[name])
        rate = 20 * n / med / 1e6
        print(f"    {name:6} {med:8.3f} {min(ms[name]):8.3f}..{max(ms[name]):<8.3f} {peak[name] / 2 ** 20:9.1f} {rate:9.1f} "
              f"{100 * rate / ACHIEVABLE_HBM_GBS:10.1f}% {last[name]:10.6f}")
    print(f"    torch / hip = {statistics.median(ms['torch']) / statistics.median(ms['hip']):.2f}x;  "
          f"the gradient alone is {4 * n / 2 ** 20:.1f} MB")
    # the two kernels apart (call time between device events, the reduce launch with the forward)
    w = lf.weight
    with torch.no_grad():
        for _ in range(3):
            ops.seg_loss(x, t, w, mse=True)
        reps = max(3, int(0.3 / (statistics.median(ms["hip"]) * 1e-3)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.seg_loss(x, t, w, mse=True)
        e1.record()
        torch.cuda.synchronize()
    fwd = e0.elapsed_time(e1) / reps
    bwd = statistics.median(ms["hip"]) - fwd
    print(f"    hip forward alone {fwd:.3f} ms = {8 * n / fwd / 1e6:.0f} GB/s ({100 * 8 * n / fwd / 1e6 / ACHIEVABLE_HBM_GBS:.0f}% of 6.3 TB/s); "
          f"the rest (backward, autograd) {bwd:.3f} ms = {12 * n / bwd / 1e6:.0f} GB/s ({100 * 12 * n / bwd / 1e6 / ACHIEVABLE_HBM_GBS:.0f}%)")
    x.grad = None


def train_step(lf, dev, a):
    from mas_hip import ops
    from mas_hip.optim import Adam
    from models import VQBASE
    ops.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    m = VQBASE(**SEG_CFG).to(dev).train()
    m.quantize.q_counter = m.quantize.q_re_end               # steady state: VQ active, no k-means
    opt = Adam(m.parameters(), lr=1e-5, betas=(0.5, 0.9))
    gen = torch.Generator(device=dev).manual_seed(1)
    seg = (torch.rand((8, 159, 256, 256), device=dev, generator=gen) < 0.3).float()
    info = {}

    def call(clear=False):
        opt.zero_grad(set_to_none=True)
        if clear:
            return None
        rec, q_loss = m(seg)
        info["rec"] = (rec.dtype, rec.is_contiguous(memory_format=torch.channels_last))
        loss = lf(q_loss, seg, rec)
        loss.backward()
        opt.step()
        return loss

    ms, peak, last = _alternate(("torch", "hip"), call, a.seconds * 3, a.rounds)
    print(f"(b) one VQ-SEG training step, B = 8, 256 x 256, bf16 compute, VQBASE at conf/seg_config.yaml's widths, VQVAEWithBCELoss, "
          f"mas_hip.optim.Adam; the decoder's output is {info['rec'][0]}, channels_last: {info['rec'][1]}")
    print(f"    {'loss path':9} {'ms':>9} {'min..max':>19} {'peak MB':>9} {'loss':>10}")
    for name in ("torch", "hip"):
        print(f"    {name:9} {statistics.median(ms[name]):9.2f} {min(ms[name]):9.2f}..{max(ms[name]):<9.2f} {peak[name] / 2 ** 20:9.1f} "
              f"{last[name]:10.6f}")
    print(f"    torch / hip = {statistics.median(ms['torch']) / statistics.median(ms['hip']):.3f}x")
    del m, opt


def big_batch(lf, dev):
    from mas_hip import ops
    x, t = _inputs(64, dev, 64)
    w = lf.weight
    x.requires_grad_(True)
    loss = ops.seg_loss(x, t, w, mse=True)
    loss.backward()
    halves = []
    for k in range(2):
        xh = x.detach()[32 * k:32 * k + 32].requires_grad_(True)
        lh = ops.seg_loss(xh, t[32 * k:32 * k + 32], w, mse=True)
        lh.backward()
        same = bool(torch.equal(x.grad[32 * k:32 * k + 32], 0.5 * xh.grad))
        halves.append((float(lh.detach()), same, bool(torch.isfinite(xh.grad).all())))
        del xh
    mean = 0.5 * (halves[0][0] + halves[1][0])
    ok = abs(float(loss.detach()) - mean) <= 4 * 2.0 ** -23 * max(1.0, abs(mean)) and all(h[1] and h[2] for h in halves)
    print(f"(c) B = 64, {x.numel() / 1e6:.0f} M elements, {4 * x.numel() / 1e9:.2f} GB per tensor: loss {float(loss.detach()):.7f}, halves "
          f"{halves[0][0]:.7f} {halves[1][0]:.7f} (mean {mean:.7f}); gradient == half of each half's, bit for bit: {halves[0][1]} {halves[1][1]}"
          f" -> {'OK' if ok else 'MISMATCH'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per path and configuration (at least)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_seg_loss: no GPU found (there is no CPU path to time)")
    import losses
    dev = torch.device("cuda:0")
    lf = losses.VQVAEWithBCELoss(image_channels=159, codebook_weight=1.0).to(dev)
    print(f"VQ-SEG objective, torch expression against csrc/seg_loss.hip; >= {a.seconds:g} s per path in {a.rounds} alternating rounds; "
          f"{torch.cuda.get_device_name(0)}")
    ok = True
    if "a" in a.parts:
        for b in (8, 32):
            loss_alone(b, lf, dev, a)
            torch.cuda.empty_cache()
        loss_alone(32, lf, dev, a, nhwc=False)                   # what this repository's decoder hands back: the same-layout kernel
        torch.cuda.empty_cache()
    if "b" in a.parts:
        train_step(lf, dev, a)
        torch.cuda.empty_cache()
    if "c" in a.parts:
        ok = big_batch(lf, dev)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
