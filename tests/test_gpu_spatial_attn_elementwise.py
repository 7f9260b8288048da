"""The AttnBlock attention core (make-a-scene_amd/csrc/spatial_attn.hip, spatial_attn_flash.hip, spatial_attn_core.h), every element of o,
lse, delta, dQ, dK and dV against fp64, on both kernel sets.  Cases, inputs, reference, bounds and the GPU runner are
tests/helpers/spatial_attn_check.py (read its docstring first); tests/test_spatial_attn_elementwise_cpu.py shows on the CPU that these
bounds catch a dropped key, a dropped tile, a skipped rescale, a chunk visited twice, an lse that misses a key, swapped V rows, a truncated
P, a neighbour's delta, another image's K and a channel tile written where it should be dropped.

One test per family, so that a failure names its kernel: shipped forward (``mas_spatial_attn_fwd``), shipped backward
(``mas_spatial_attn_bwd``), chunked forward and backward (``mas_spatial_attn_flash_fwd / _bwd``).  Shapes: S on every edge of the 32-token
tile, the 8-wave work-group and the 256-key chunk (1 ... 256 shipped, 1 ... 769 chunked), C = 32 ... 512 (1 to 4 channel groups, partly
full ones), grids that are and are not a multiple of 8; five operand modes (gauss at q scales 1.5 and 0.05, hard, onehot, uniform).  The
backward entries are fed the reference's lse (and o), so each direction is judged on its own arithmetic.  Every output lies inside a
NaN-filled allocation with 8 KiB of sentinel on each side: every element must come back finite and inside its bound, every guard byte
unchanged.  REQUIRED lists the (launch name, feature) pairs the union of the cases has to reach.

Bounds (U = 2^-8, TAU = 2^-18; A, AD = the reference formula on absolute values; the casts are quoted in the helper's docstring):
  o, dV, dQ, dK   FLOOR + U |r| + c U A + TAU A (+ delta's error on AD for dQ, dK);  c = 1, and 2 for the chunked dK (dS is built from the P
                  read back from LDS already rounded, then cast again)
  delta           shipped: K_DELTA TAU A_D, A_D = rowsum(P o |dO||v|^T) (fp32 sum of P dP, no cast); chunked: (U + TAU) A_D,
                  A_D = rowsum(|dO| o |o|) (reads the rounded o)
  lse             K_LSE 2^-23 max(1, |lse|, max|s| of the row), per forward kernel
  exact           onehot: o == v[t(i)], dV == the integer sums of dO, bitwise; uniform: chunked |o - r| <= (U + 2^-22) |r|, shipped at S a
                  power of two o == bf16(mean v) bitwise
No bf16 bound needed a further rounding: every bf16 tensor stays below 1 with the counts as derived.

Measured on an MI355X, worst |y - r| / bound over all cases and modes of the family (1 = the bound; lse and the shipped delta with the
coefficients chosen below):
                     o      lse     delta   dV      dQ      dK
  shipped forward    0.823  0.361
  shipped backward                  0.439   0.901   0.762   0.854
  chunked forward    0.646  0.332
  chunked backward                  0.466   0.875   0.413   0.481
  per mode, worst tensor: shipped gauss 0.823 (o), gauss_flat 0.501 (dQ), hard 0.860 (dV), onehot 0.901 (dV), uniform 0.491 (dQ);
  chunked gauss 0.714 (dV), gauss_flat 0.502 (dV), hard 0.802 (dV), onehot 0.875 (dV), uniform 0.466 (delta).
  Every exact check of the onehot and uniform modes holds on both kernel sets, every guard byte came back unchanged, and the bf16 figures
  equal those of the CPU model of the helper to three digits (the same roundings in the same places).
Measured coefficients (they cover __expf, __logf and the accumulation order and cannot be derived).  Rule: the worst value seen on the MI355X,
doubled, then the next power of two above.
  K_LSE    worst |lse - r| / (2^-23 max(1, |lse|, max|s|)):
           spatial_attn_fwd        5.78 (hard mode, C = 384 and 512 only: the raw score near 60 / scale = 1358 is summed in fp32 over C / 16
                                   MFMA steps; gauss 2.19, gauss_flat 1.61, onehot 0.82, uniform 0.74)  -> 11.6 -> 16
           spatial_attn_flash_fwd  5.31 (hard mode, C = 384 and 512; gauss 1.65, gauss_flat 1.64, onehot 0.82, uniform 1.14) -> 10.6 -> 16
  K_DELTA  worst |delta - D| / (TAU A_D), shipped backward:  1.76 (hard mode: P = exp(s - lse) of two fp32 numbers near 60, each good to
           2^-19; gauss 0.07, onehot 0.62)  -> 3.5 -> K_DELTA = 4
The whole file takes about 7 s on an MI355X box: 1.8 s for the shipped kernel set (both directions share one pass and one reference),
2.9 s for the chunked one, 0.02 s per determinism case.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import spatial_attn_check as CHK  # noqa: E402

PARTS = {"fwd": ("o", "lse"), "bwd": ("delta", "dv", "dq", "dk")}
_done = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _kset(kset):
    """runs and judges every (case, mode) of a kernel set once, both directions on one reference:
    {part: (failures, worst ratio per tensor, [(case, launch name)])}"""
    if kset in _done:
        return _done[kset]
    t0 = time.time()
    res = {part: ([], {}, []) for part in PARTS}
    for c in CHK.CASES:
        if c["kset"] != kset:
            continue
        for mode in c["modes"]:
            ins = CHK.make_inputs(c, mode)
            ref = CHK.reference(ins, kset)
            if mode == "onehot":
                CHK.onehot_precondition(ins, ref)              # on the reference alone, before any kernel output exists
            for i, part in enumerate(("fwd", "bwd")):
                fails, worst, ran = res[part]
                got, _, kern, gf = CHK.run(c, ins, ref, part)
                fails += gf
                if kern != CHK.LAUNCH[kset][i]:
                    fails.append(f"{c['name']} {mode}: the {part} launch was {kern}, not {CHK.LAUNCH[kset][i]}")
                f, w = CHK.judge(c, mode, ins, ref, got)
                fails += f
                for k, v in w.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                    worst[(k, mode)] = max(worst.get((k, mode), 0.0), v)
                if mode == c["modes"][0]:
                    ran.append((c, kern))
    print(f"\n{kset}: {time.time() - t0:.1f} s for both directions")
    _done[kset] = res
    return res


def _check(kset, part):
    _dev()
    fails, worst, _ = _kset(kset)[part]
    print(f"\n{kset} {part}: worst |y - r| / bound  " + "  ".join(f"{k} {worst[k]:.3f}" for k in PARTS[part]))
    for mode in CHK.MODES:
        print(f"  {mode:10s} " + "  ".join(f"{k} {worst[(k, mode)]:.3f}" for k in PARTS[part]))
    # the measured coefficients in their own units (bound = coefficient * unit): what K_LSE and K_DELTA are chosen from
    if part == "fwd":
        print(f"{kset} fwd: measured  lse / (2^-23 max(1, |lse|, max|s|)) {worst['lse'] * CHK.K_LSE[CHK.LAUNCH[kset][0]]:.2f}")
    elif kset == "shipped":
        print(f"{kset} bwd: measured  delta / (TAU A_D) {worst['delta'] * CHK.K_DELTA:.2f}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


def test_shipped_forward():
    _check("shipped", "fwd")


def test_shipped_backward():
    _check("shipped", "bwd")


def test_chunked_forward():
    _check("flash", "fwd")


def test_chunked_backward():
    _check("flash", "bwd")


def test_every_required_launch_and_feature_was_reached():
    _dev()
    ran = []
    for kset in ("shipped", "flash"):
        for part in PARTS:
            ran += _kset(kset)[part][2]
    got = CHK.reached(ran)
    missing = {k: sorted(f - got.get(k, set())) for k, f in CHK.REQUIRED.items() if not f <= got.get(k, set())}
    assert not missing, missing


@pytest.mark.parametrize("name,part", [("shipped-N2S81C64", "fwd"), ("shipped-N2S81C64", "bwd"), ("flash-N2S600C64", "fwd"), ("flash-N2S600C64", "bwd")])
def test_second_run_gives_equal_bits(name, part):
    _dev()
    c = next(c for c in CHK.CASES if c["name"] == name)
    assert c["S"] % 32
    ins = CHK.make_inputs(c, "gauss")
    ref = CHK.reference(ins, c["kset"])
    (_, a, _, _), (_, b, _, _) = CHK.run(c, ins, ref, part), CHK.run(c, ins, ref, part)
    for k in PARTS[part]:
        assert np.array_equal(a[k], b[k]), k
