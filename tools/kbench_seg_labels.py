#!/usr/bin/env python3
"""The VQ-SEG input as label planes (csrc/seg_labels.hip) measured on one GPU against the dense-map paths it stands beside,
both in ONE process, alternating in rounds after a warm-up, each round a window of calls between two device events.

  dense  : the one-hot fp32 NCHW map (what the reference's dataloader delivers) through the paths that existed before: ops.seg_loss,
           the cast + transpose + pad glue in front of the encoder's first convolution, a 1.33 GB / 32 host -> device copy per sample
  labels : mas_hip.seglabels.SegLabels -- 4 uint8 planes per sample -- through ops.seg_loss_labels, ops.seg_expand and VQBASE

 (a) the loss alone, forward + backward, [32, 159, 256, 256] fp32, NCHW and NHWC prediction; the dense path has an fp32 NCHW target.
     ms per call (median, min..max over the rounds = the spread of repeated runs of the same code), peak memory above the inputs, and
     the labels path's 12 algorithmic bytes per element (read x forward; read x, write dx backward) per second;
 (b) the input map of the encoder's first convolution, [32, 160, 256, 256] NHWC bf16: ops.seg_expand against the glue it replaces
     (``ops.nhwc(x, bf16)`` then ``F.pad`` of the channel axis, as ops.norm_act_conv runs them on a dense input);
 (c) one VQ-SEG training step at B = 8, bf16 compute, the batch starting in PINNED host memory: the host -> device copy and the step
     (forward, VQVAEWithBCELoss, backward, mas_hip.optim.Adam) timed apart between device events, the peak device memory of copy + step,
     and the step once more with the batch already on the device.

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


def _labels(b, device, seed):
    """random planes of the reference layout: every class and "none" in each group, edge values 0 .. 2"""
    from mas_hip.seglabels import SegLabels
    gen = torch.Generator().manual_seed(seed)
    planes = torch.stack([torch.randint(0, g + 1, (b, 256, 256), generator=gen, dtype=torch.uint8) for g in (133, 20, 5, 2)], 1)
    return SegLabels(planes.contiguous()).to(device)


def _alternate(paths, seconds, rounds, clear=None):
    """paths: {name: call}.  -> {name: [ms per call, one per round]}, {name: peak bytes of one call above what was allocated before it}"""
    calls, peak = {}, {}
    for name, call in paths.items():
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
        if clear is not None:
            clear()
        torch.cuda.synchronize()
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
    return f"    {name:8} {med:9.3f} {min(v):9.3f}..{max(v):<9.3f} spread {100 * (max(v) - min(v)) / med:5.1f}% {extra}"


def loss_alone(dev, a, nhwc):
    from mas_hip import ops
    b = 32
    lab = _labels(b, dev, 3)
    t = lab.dense()                                              # fp32 NCHW on the device: the dense path's target
    gen = torch.Generator(device=dev).manual_seed(5)
    x = (2.0 * torch.randn((b, 256, 256, 159), device=dev, generator=gen)).permute(0, 3, 1, 2)
    if not nhwc:
        x = x.contiguous()
    x.requires_grad_(True)
    w = torch.ones(159, device=dev)
    w[153:158] = 20.0
    out = {}

    def dense():
        x.grad = None
        loss = ops.seg_loss(x, t, w, mse=True)
        loss.backward()
        out["dense"] = loss

    def labels():
        x.grad = None
        loss = ops.seg_loss_labels(x, lab, w, mse=True)
        loss.backward()
        out["labels"] = loss

    ms, peak = _alternate({"dense": dense, "labels": labels}, a.seconds, a.rounds, clear=lambda: setattr(x, "grad", None))
    n = x.numel()
    dense()
    gd = x.grad.clone()
    labels()
    same = bool(torch.equal(gd, x.grad))
    print(f"(a) loss alone, fwd + bwd, [{b}, 159, 256, 256] fp32 {'NHWC' if nhwc else 'NCHW'} prediction: {n / 1e6:.1f} M elements; dense = "
          f"ops.seg_loss on an fp32 NCHW target (20 B / element), labels = ops.seg_loss_labels (12 B / element + 4 B / pixel)")
    print(f"    {'path':8} {'ms':>9} {'min..max':>20}")
    for name, bytes_per in (("dense", 20), ("labels", 12)):
        rate = bytes_per * n / statistics.median(ms[name]) / 1e6
        print(_row(name, ms[name], f"peak {peak[name] / 2 ** 20:8.1f} MB  {rate:7.1f} GB/s on {bytes_per} B / element = "
                                   f"{100 * rate / ACHIEVABLE_HBM_GBS:5.1f}% of 6.3 TB/s  loss {float(out[name].detach()):.7f}"))
    print(f"    dense / labels = {statistics.median(ms['dense']) / statistics.median(ms['labels']):.3f}x;  dx bit-identical: {same};  "
          f"resident beside the prediction: target {4 * n / 2 ** 20:.0f} MB against planes {lab.planes.numel() / 2 ** 20:.0f} MB")
    x.grad = None


def expand(dev, a):
    import torch.nn.functional as F
    from mas_hip import ops
    b = 32
    lab = _labels(b, dev, 7)
    x = lab.dense()                                              # fp32 NCHW: what arrives from the host on the dense path
    out = {}

    def dense():
        out["dense"] = F.pad(ops.nhwc(x, torch.bfloat16), (0, 0, 0, 0, 0, 1))

    def labels():
        out["labels"] = ops.seg_expand(lab, dtype=torch.bfloat16, channels_last=True, pad_to=160)

    ms, peak = _alternate({"dense": dense, "labels": labels}, a.seconds, a.rounds, clear=out.clear)
    same = bool(torch.equal(out["dense"], out["labels"])) and out["dense"].stride() == out["labels"].stride()
    nb = out["labels"].numel() * 2
    print(f"(b) the first convolution's input, [{b}, 160, 256, 256] NHWC bf16 ({nb / 1e9:.2f} GB): dense = cast + transpose + pad of the "
          f"fp32 NCHW map (ops.nhwc, F.pad), labels = ops.seg_expand; same bytes: {same}")
    print(f"    {'path':8} {'ms':>9} {'min..max':>20}")
    for name in ("dense", "labels"):
        print(_row(name, ms[name], f"peak {peak[name] / 2 ** 20:8.1f} MB  output written at {nb / statistics.median(ms[name]) / 1e6:7.1f} GB/s"))
    print(f"    dense / labels = {statistics.median(ms['dense']) / statistics.median(ms['labels']):.3f}x")
    out.clear()


def train_step(dev, a):
    import losses
    from mas_hip import ops
    from mas_hip.optim import Adam
    from models import VQBASE
    ops.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    lf = losses.VQVAEWithBCELoss(image_channels=159, codebook_weight=1.0).to(dev)
    m = VQBASE(**SEG_CFG).to(dev).train()
    m.quantize.q_counter = m.quantize.q_re_end               # steady state: VQ active, no k-means
    opt = Adam(m.parameters(), lr=1e-5, betas=(0.5, 0.9))
    host = {"labels": _labels(8, "cpu", 11).pin_memory()}
    host["dense"] = host["labels"].dense().pin_memory()
    assert host["dense"].is_pinned() and host["labels"].is_pinned()
    res = {}
    for name in ("dense", "labels"):                             # warm-up: kernels, allocator, weight images
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            seg = host[name].to(dev, non_blocking=True)
            rec, q = m(seg)
            lf(q, seg, rec).backward()
            opt.step()
        del seg, rec, q
    torch.cuda.synchronize()
    for name in ("dense", "labels"):
        res[name] = dict(copy=[], step=[], loss=None)
    for r in range(a.rounds):
        for name in ("dense", "labels"):
            for k in range(a.steps):
                opt.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                if r == 0 and k == 0:
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                seg = host[name].to(dev, non_blocking=True)
                e1.record()
                rec, q = m(seg)
                loss = lf(q, seg, rec)
                loss.backward()
                opt.step()
                e2.record()
                torch.cuda.synchronize()
                if r == 0 and k == 0:
                    res[name]["peak"] = (torch.cuda.max_memory_allocated(), base)
                res[name]["copy"].append(e0.elapsed_time(e1))
                res[name]["step"].append(e1.elapsed_time(e2))
                res[name]["loss"] = float(loss.detach())
                del seg, rec, q, loss
    # the step once more with the batch already ON the device: above, the host queues the step's launches while the copy runs, so a long copy
    # hides launch overhead that a short one leaves in the step's window; here both paths start from the same empty queue
    resident = {name: host[name].to(dev) for name in ("dense", "labels")}
    for r in range(a.rounds):
        for name in ("dense", "labels"):
            for k in range(a.steps):
                opt.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rec, q = m(resident[name])
                loss = lf(q, resident[name], rec)
                loss.backward()
                opt.step()
                e1.record()
                torch.cuda.synchronize()
                res[name].setdefault("resident", []).append(e0.elapsed_time(e1))
                del rec, q, loss
    nbytes = {"dense": host["dense"].numel() * 4, "labels": host["labels"].planes.numel()}
    print(f"(c) one VQ-SEG training step, B = 8, 256 x 256, bf16 compute, VQBASE at conf/seg_config.yaml's widths, VQVAEWithBCELoss, "
          f"mas_hip.optim.Adam; the batch starts in pinned host memory; {a.rounds} alternating rounds of {a.steps} steps")
    print(f"    {'input':8} {'host MB':>9} {'copy ms':>9} {'min..max':>19} {'GB/s':>7} {'step ms':>9} {'min..max':>19} {'copy+step':>10} {'peak MB':>9} {'loss':>10}")
    tot = {}
    for name in ("dense", "labels"):
        c, s = res[name]["copy"], res[name]["step"]
        cm, sm = statistics.median(c), statistics.median(s)
        tot[name] = cm + sm
        print(f"    {name:8} {nbytes[name] / 2 ** 20:9.1f} {cm:9.3f} {min(c):9.3f}..{max(c):<9.3f} {nbytes[name] / cm / 1e6:7.1f} {sm:9.2f} "
              f"{min(s):9.2f}..{max(s):<9.2f} {cm + sm:10.2f} {res[name]['peak'][0] / 2 ** 20:9.1f} {res[name]['loss']:10.6f}")
    print(f"    the step with the batch already on the device (no copy in front of it):")
    for name in ("dense", "labels"):
        print(_row(name, res[name]["resident"]))
    print(f"    dense / labels = {statistics.median(res['dense']['resident']) / statistics.median(res['labels']['resident']):.3f}x")
    print(f"    copy + step, dense / labels = {tot['dense'] / tot['labels']:.3f}x;  step alone = "
          f"{statistics.median(res['dense']['step']) / statistics.median(res['labels']['step']):.3f}x;  peak device memory "
          f"{(res['dense']['peak'][0] - res['labels']['peak'][0]) / 2 ** 20:.1f} MB lower with labels (model, optimizer state and step included in both)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed window per path and configuration (at least)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4, help="(c): steps per path and round")
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("kbench_seg_labels: medians of at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("kbench_seg_labels: no GPU found (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    print(f"VQ-SEG input as label planes (csrc/seg_labels.hip) against the dense-map paths; >= {a.seconds:g} s per path in {a.rounds} "
          f"alternating rounds; {torch.cuda.get_device_name(0)}")
    if "a" in a.parts:
        for nhwc in (False, True):
            loss_alone(dev, a, nhwc)
            torch.cuda.empty_cache()
    if "b" in a.parts:
        expand(dev, a)
        torch.cuda.empty_cache()
    if "c" in a.parts:
        train_step(dev, a)


if __name__ == "__main__":
    main()
