#!/usr/bin/env python3
"""GPU child of tests/test_gpu_wgrad_splits.py: every split-K weight-gradient kernel, run through ``ops.conv_wgrad_raw`` exactly as the
backward calls it, at the split count this process was started with (MAS_WGRAD_SPLITS / MAS_WGRAD_OVERSUB / unset: read once per
process by the library) and the CU budget ``ops`` gives its weight-gradient descriptors (MAS_WGRAD_CUS in the environment, or its default).

    wgrad_split_check.py OUT.pt

For every case of CASES: the kernel that ran is the one named (``set_launch_hook`` + ``last_kernel``); every ``ops._wgrad_partials``
workspace is filled with NaN before each call, so a slab element no launch writes reaches dW as NaN; two calls are bitwise equal.  dW,
db, the per-slice split counts the library reported, the budget and the case go to OUT.pt.  All numeric checks against fp64 are the parent's, on
the CPU.  Exits non-zero on a failed assertion."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402

ACT_NONE, ACT_AFFINE_SILU = 0, 2


def _case(name, kernel, n, cin, cout, h, w, ks=3, stride=1, pad=(1, 1), ho=None, wo=None, dtype="bf16", act=ACT_NONE, up=False,
          slice_imgs=None):
    if ho is None:
        hl, wl = (2 * h, 2 * w) if up else (h, w)
        ho, wo = (hl + pad[0] + pad[0] - ks) // stride + 1, (wl + pad[1] + pad[1] - ks) // stride + 1
    return dict(name=name, kernel=kernel, n=n, cin=cin, cout=cout, h=h, w=w, ks=ks, stride=stride, pt=pad[0], pl=pad[1], ho=ho, wo=wo,
                dtype=dtype, act=act, up=up, slice_imgs=slice_imgs)


# Small shapes (N <= 5, maps <= 48 x 80, N * Ho * Wo <= ~2 * 10^4) chosen so that the parent's split list reaches every walk regime of
# every family (tests/helpers/wgrad_walk.py restates the walks; the parent asserts the union of regimes).
CASES = [
    # LDS-DMA 3x3 (conv_wgrad_dma.hip KS = 3): ragged Ho % 8 and Wo % 16, 5 x 3 tiles per image, 60 tiles (31/32/33/47 unclamped)
    _case("dma_ragged", "conv_wgrad_dma", 4, 64, 128, 36, 44),
    # Cin = 192 (three 64-channel tiles: odd n_ci_t), Cout = 384
    _case("dma_c192_c384", "conv_wgrad_dma", 2, 192, 384, 20, 24),
    # the Upsample fold (W < 32: not the sub-pixel kernel): 24 x 28 output map, Cout = 128, Cin = 128
    _case("dma_upfold", "conv_wgrad_dma", 2, 128, 128, 12, 14, up=True),
    # the GroupNorm + SiLU prologue with a random scale / shift, 5 x 5 tiles per image, 50 tiles
    _case("dma_silu", "conv_wgrad_dma", 2, 64, 128, 38, 80, act=ACT_AFFINE_SILU),
    # the sub-pixel form of Upsample + conv (KS = 2): 2 x 3 low-resolution tiles per image
    _case("up2", "conv_wgrad_up2", 2, 64, 128, 12, 40, up=True),
    # Downsample: stride 2, pads (0, 1, 0, 1) -> 20 x 36 output, 5 x 3 tiles of 4 x 16 per image, 60 tiles
    _case("s2_down", "wgrad_s2", 4, 64, 128, 40, 72, stride=2, pad=(0, 0), ho=20, wo=36),
    # 1x1 bf16: M = 880 pixels, M % 64 = 48
    _case("pw_bf16", "wgrad1x1", 2, 128, 256, 20, 22, ks=1, pad=(0, 0)),
    # 1x1 fp32: Cin / Cout multiples of 4, not of 64
    _case("pw_f32", "wgrad1x1_f32", 2, 36, 20, 30, 34, ks=1, pad=(0, 0), dtype="f32"),
    # thin RGB-edge layers, 11 x 3 tiles of 4 x 16 per image
    _case("thin_8_128", "wgrad_thin", 2, 8, 128, 42, 44),
    _case("thin_128_8", "wgrad_thin", 2, 128, 8, 42, 44),
    # the general kernels in slab mode
    _case("tr_96_160", "conv_wgrad_tr", 2, 96, 160, 20, 36),
    _case("tr_4x4_s1", "conv_wgrad_tr", 2, 64, 64, 21, 21, ks=4),
    _case("tr_4x4_s2", "conv_wgrad_tr", 2, 32, 64, 24, 24, ks=4, stride=2),          # space-to-depth: ks = 2 over 128 channels
    _case("gen_f32_s1", "conv_wgrad", 2, 40, 24, 18, 20, dtype="f32"),
    _case("gen_f32_s2", "conv_wgrad", 2, 40, 24, 22, 34, stride=2, dtype="f32"),
    # N = 5 cut into batch slices 2 + 2 + 1 (ops._MAX_TENSOR_BYTES lowered): slabs appended per slice at offset `first`, one reduce over
    # `tot`; the sub-pixel path reduces per slice and adds
    _case("dma_sliced", "conv_wgrad_dma", 5, 64, 128, 21, 37, slice_imgs=2),
    _case("up2_sliced", "conv_wgrad_up2", 5, 64, 128, 12, 40, up=True, slice_imgs=2),
]


def make_inputs(c):
    """deterministic CPU operands of a case: x (bf16 or fp32), dy, ss ([N][Cin][2] fp32 scale / shift, prologue cases only)"""
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])))
    dt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
    x = torch.randn(c["n"], c["cin"], c["h"], c["w"], generator=g).to(dt)
    dy = (0.5 * torch.randn(c["n"], c["cout"], c["ho"], c["wo"], generator=g)).to(dt)
    ss = None
    if c["act"] != ACT_NONE:
        ss = torch.stack([1.0 + 0.3 * torch.randn(c["n"], c["cin"], generator=g), 0.5 * torch.randn(c["n"], c["cin"], generator=g)],
                         dim=-1).contiguous()
    return x, dy, ss


def descs_of(ops, c, slices):
    """the descriptors conv_wgrad_raw hands the library (after the 4x4 / stride-2 space-to-depth rewrite), one per batch slice"""
    dt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
    if c["ks"] == 4 and c["stride"] == 2:
        g = (c["ho"] + 1, c["wo"] + 1, 4 * c["cin"], c["ho"], c["wo"], c["cout"], 2, 1, 0, 0)
    else:
        g = (c["h"], c["w"], c["cin"], c["ho"], c["wo"], c["cout"], c["ks"], c["stride"], c["pt"], c["pl"])
    return [ops._wgrad_desc(n1 - n0, *g, dt, c["act"], c["up"]) for n0, n1 in slices]


def run(out_path):
    from mas_hip import ops, lib
    dev = torch.device("cuda:0")
    kernels = []

    def hook(kind, shape, launch):
        launch()
        if kind == "conv_wgrad":
            kernels.append(ops.last_kernel())

    ops.set_launch_hook(hook)
    results = {}
    max_bytes = ops._MAX_TENSOR_BYTES
    try:
        for c in CASES:
            x, dy, ss = make_inputs(c)
            cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
            xd, dyd, ssd = cl(x), cl(dy), (ss.to(dev) if ss is not None else None)
            esz = x.element_size()
            per_img = max(c["h"] * c["w"] * c["cin"] * esz, c["ho"] * c["wo"] * c["cout"] * esz)
            ops._MAX_TENSOR_BYTES = c["slice_imgs"] * per_img if c["slice_imgs"] else max_bytes
            slices = ops._batch_slices(c["n"], c["h"] * c["w"] * c["cin"] * esz, c["ho"] * c["wo"] * c["cout"] * esz)
            assert (len(slices) > 1) == bool(c["slice_imgs"]), (c["name"], slices)
            ds = descs_of(ops, c, slices)
            if c["kernel"] == "conv_wgrad_up2":
                splits = [int(lib().mas_conv_up2_wgrad_splits(C.byref(d))) for d in ds]
            else:
                splits = [int(lib().mas_conv_wgrad_splits(C.byref(d))) for d in ds]
            assert all(k > 0 for k in splits), (c["name"], splits)
            args = (c["n"], c["h"], c["w"], c["cin"], c["ho"], c["wo"], c["cout"], c["ks"], c["stride"], c["pt"], c["pl"], c["act"], c["up"], True)
            ops.conv_wgrad_raw(xd, ssd, dyd, *args)          # creates the workspace (torch.empty) for the NaN fill below
            outs = []
            for _ in range(2):
                torch.cuda.synchronize()
                for ws in ops._wgrad_partials.values():
                    ws.fill_(float("nan"))
                kernels.clear()
                dw, db = ops.conv_wgrad_raw(xd, ssd, dyd, *args)
                torch.cuda.synchronize()
                assert kernels and all(k == c["kernel"] for k in kernels), (c["name"], kernels)
                # (the sub-pixel path hooks every slice's launch, the others one launch over all slices)
                assert len(kernels) == (len(slices) if c["kernel"] == "conv_wgrad_up2" else 1), (c["name"], kernels, slices)
                outs.append((dw.cpu(), db.cpu()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"{c['name']}: dW / db not bitwise run to run"
            results[c["name"]] = dict(dw=outs[0][0], db=outs[0][1], splits=splits, slices=slices, kernel=kernels[0])
            print(f"{c['name']:14s} {kernels[0]:15s} splits {splits}", flush=True)
    finally:
        ops._MAX_TENSOR_BYTES = max_bytes
        ops.set_launch_hook(None)
    env = {k: os.environ.get(k) for k in ("MAS_WGRAD_SPLITS", "MAS_WGRAD_OVERSUB")}
    torch.save(dict(results=results, env=env, wgrad_cus=ops.wgrad_cus(), cus=torch.cuda.get_device_properties(0).multi_processor_count), out_path)


if __name__ == "__main__":
    run(sys.argv[1])
