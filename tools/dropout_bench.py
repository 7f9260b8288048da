#!/usr/bin/env python3
"""Dropout costs, one process, one GPU ("Dropout"):
  1. causal attention at B 8, H 16, S 1536, head 64, bf16: forward and backward (delta + dkv + dq) with p = 0.1 against p = 0;
  2. the same fwd + bwd against the ATen composition (materialised scores, softmax, torch.dropout, two matmuls);
  3. mas_dropout_apply on a 32x256x256x128 bf16 tensor against Tensor.copy_ (bytes moved / time);
  4. a 24-layer MakeAScene step with attention, output and MLP dropout at 0.1 against 0.
Prints one JSON line.   python tools/dropout_bench.py [--reps 20] [--no-step]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402

import mas_hip  # noqa: E402
from mas_hip import ops  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = mas_hip.lib()
    out = {}
    B, H, S, hd = 8, 16, 1536, 64
    d = H * hd
    torch.manual_seed(0)
    x = torch.randn(B, S, 3 * d, device=dev).bfloat16()
    o = torch.empty(B, S, d, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, S, device=dev)
    delta = torch.empty_like(lse)
    go = torch.randn(B, S, d, device=dev).bfloat16()
    dx = torch.empty_like(x)
    seed = ops.drop_seed(dev)
    base, esz, st = x.data_ptr(), 2, ops._stream
    qkv_p = [ops.C.c_void_p(base), ops.C.c_void_p(base + d * esz), ops.C.c_void_p(base + 2 * d * esz)]
    sc = hd ** -0.5

    def fwd(p):
        if p > 0:
            mas_hip.check(L.mas_attn_causal_fwd_drop(*qkv_p, ops._ptr(o), ops._ptr(lse), mas_hip.BF16, B, H, S, hd, 3 * d, 3 * d, 3 * d, S * 3 * d,
                                                     S * 3 * d, S * 3 * d, sc, p, ops._ptr(seed), st()))
        else:
            mas_hip.check(L.mas_attn_causal_fwd(*qkv_p, ops._ptr(o), ops._ptr(lse), mas_hip.BF16, B, H, S, hd, 3 * d, 3 * d, 3 * d, S * 3 * d,
                                                S * 3 * d, S * 3 * d, sc, st()))

    def bwd(p):
        args = (ops._ptr(x), ops._ptr(o), ops._ptr(go), ops._ptr(lse), ops._ptr(delta), ops._ptr(dx), mas_hip.BF16, B, H, S, hd, sc)
        if p > 0:
            mas_hip.check(L.mas_attn_causal_bwd_drop(*args, p, ops._ptr(seed), st()))
        else:
            mas_hip.check(L.mas_attn_causal_bwd(*args, st()))

    for p in (0.0, 0.1):
        fwd(p)
        out[f"attn_fwd_ms_p{p}"] = timed(lambda: fwd(p), a.reps)
        out[f"attn_bwd_ms_p{p}"] = timed(lambda: bwd(p), a.reps)
    t0 = out["attn_fwd_ms_p0.0"] + out["attn_bwd_ms_p0.0"]
    t1 = out["attn_fwd_ms_p0.1"] + out["attn_bwd_ms_p0.1"]
    out["attn_fwdbwd_ratio_p0.1_vs_p0"] = t1 / t0

    # ATen composition at the same shape (fp32 scores would need 1.2 GB per tensor; bf16 as autocast would run it)
    xa = x.clone().requires_grad_(True)
    mask = torch.ones(S, S, device=dev, dtype=torch.bool).tril()

    def aten():
        q, k, v = (t.view(B, S, H, hd).transpose(1, 2) for t in xa.split(d, dim=-1))
        s_ = torch.matmul(q, k.transpose(-1, -2)) * sc
        pr = torch.dropout(torch.softmax(s_.masked_fill(~mask, float("-inf")), dim=-1), 0.1, True)
        y = torch.matmul(pr, v).transpose(1, 2).reshape(B, S, d)
        y.backward(go)
    out["aten_fwdbwd_ms_p0.1"] = timed(aten, max(3, a.reps // 4), warm=1)
    out["hip_vs_aten_speedup"] = out["aten_fwdbwd_ms_p0.1"] / t1
    del xa

    # element-wise dropout against copy_
    t = torch.randn(32, 256, 256, 128, device=dev).bfloat16()
    y = torch.empty_like(t)
    nbytes = 2 * t.numel() * t.element_size()
    ms_drop = timed(lambda: mas_hip.check(L.mas_dropout_apply(ops._ptr(t), ops._ptr(y), t.numel(), mas_hip.BF16, 0.1, ops._ptr(seed), st())),
                    a.reps)
    ms_copy = timed(lambda: y.copy_(t), a.reps)
    out.update(dropout_apply_ms=ms_drop, dropout_apply_GBps=nbytes / ms_drop / 1e6, copy_ms=ms_copy, copy_GBps=nbytes / ms_copy / 1e6,
               dropout_vs_copy_rate=ms_copy / ms_drop)
    del t, y

    if not a.no_step:
        from models.transformer import MakeAScene
        for p in (0.0, 0.1):
            torch.manual_seed(0)
            m = MakeAScene(24, 1024, 16, 8192, 256, 49408 + 256, 32, 16, 256).to(dev).train()
            for mod in m.modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = p
            text = torch.randint(1, 49408, (8, 256), device=dev)
            text[:, 200:] = 0
            seg = torch.randint(0, 256, (8, 256), device=dev)
            img = torch.randint(0, 8192, (8, 1024), device=dev)

            def step():
                m.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    logits = m(text, seg, img)
                loss = torch.nn.functional.cross_entropy(logits.float().reshape(-1, 8192), img.reshape(-1))
                loss.backward()
                if not math.isfinite(float(loss)):
                    raise SystemExit("non-finite loss")
            out[f"step24_ms_p{p}"] = timed(step, 5, warm=2)
            del m
            torch.cuda.empty_cache()
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
