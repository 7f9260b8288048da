"""Stage-2 causal attention (make-a-scene_amd/csrc/attention.hip), every element of o, lse, delta, dQ, dK and dV against fp64, on every
kernel route.  Cases, inputs, reference, bounds and the GPU runner are tests/helpers/attn_rowwise_check.py (read its docstring first);
tests/test_attn_rowwise_cpu.py shows on the CPU that these bounds catch a dropped key tile, a diagonal off by one, a skipped rescale,
an lse that misses a key, swapped V rows, a truncated P and a head that reads its neighbour's K.

One test per route family, so that a failure names its kernel; every family runs B = 2, H = 3 (and one B = H = 1 case) at sequence
lengths on the edges of the 32-key wave tile, the 64-key tile of the fast kernels and the 128-query block (1 ... 321), in four operand
modes (gauss, hard, onehot, uniform; dropout cases gauss and hard).  The launch names tell the routes apart, and REQUIRED lists the
(launch name, feature) pairs the union of the cases has to reach: a dispatch change that makes a case vacuous fails here.
  generic fp32 fwd + bwd            hd 16 / 32 / 64 / 128
  generic bf16 fwd + bwd            hd 16 / 32; hd 64 through the designed fallbacks: forward from three buffers whose token strides are
                                    4 mod 8 elements (fa_aligned() fails), backward from fused buffers 8 bytes past a 16-byte boundary.
                                    Checked in the source first: the generic kernels touch global memory one element at a time (the Q / K / V
                                    fragment loops, the K / V staging loop, stage_tile, attn_bwd_delta_kernel, the d < HD store loops)
  v2 fwd + fast64 bwd               bf16 hd 64 aligned; v2 forward also from three separate aligned buffers with different strides
  fast fwd (hd 128) + generic bwd   bf16 hd 128
  dropout p = 0.25                  v2 / fast64, generic bf16 hd 32, generic fp32 hd 64; Z from mas_attn_dropout_mask
The backward entries are fed the reference's o (rounded to the kernel's dtype) and lse, so each direction is judged on its own arithmetic.

Bounds (U = 2^-8, TAU = 2^-18; A, AD = the reference formula on absolute values; derivation with the casts in the helper's docstring):
  bf16   o:       U |r| + 1 U A + TAU A      1 = the cast of the unnormalised P to the MFMA operand, ``pf[j] = (T)s[8 * t + j]`` (generic) /
                                             ``pf[j] = (T)s[sub][8 * t + j]`` (fast, v2); l, alpha and 1 / l stay fp32; U |r| = the store
                                             ``(T)(oacc[i][r] * inv)``; dropout zeroes P before the cast and scales the fp32 ``inv``
         dV:      U |r| + 1 U A + TAU A      1 = ``pf[j] = (T)s[8 * t + j]`` in both dkv kernels (P o keep mask); U |r| = ``(T)dv[i][r]``
         dQ, dK:  U |r| + 1 U A + TAU A + (U + TAU) AD      1 = ``sf[j] = (T)dp[8 * t + j]``, the one cast of dS (computed in fp32 from the
                                             fp32 P); AD = P o A_D scale times |k| / |q|: what D's own error, counted under delta,
                                             carries into dS -- A_dS is built on |D| and does not hold it when dO o o cancels
         delta:   U A_D + TAU A_D            attn_bwd_delta_kernel sums dO * o in fp32 over the already rounded bf16 o; no output cast
  fp32   o, dV, dQ, dK:  C_F32 TAU (A + AD);  delta: K_DELTA 2^-23 A_D
  lse    K_LSE 2^-23 max(1, |lse|, max|s| of the row), per forward kernel
  exact  onehot: o == v[t(i)] bitwise; bf16 dV == the integer sum of dO over the queries that chose the key, bitwise
No bf16 bound needed a further rounding: every bf16 family stays below 1 with the counts as derived.

Measured on an MI355X, worst |y - r| / bound over all cases and modes of the family (1 = the bound):
                       o      delta   dV      dQ      dK
  generic bf16         0.865  0.557   0.902   0.507   0.792
  generic bf16 hd 64   0.721  0.361   0.889   0.395   0.700
  v2 + fast64          0.784  0.304   0.910   0.376   0.753
  fast128 + generic    0.794  0.232   0.941   0.363   0.691
  dropout bf16         0.860  0.411   0.915   0.910   0.888
  generic fp32         0.225  0.468   0.404   0.019   0.078    (with the coefficients chosen below)
  dropout fp32         0.279  0.372   0.206   0.144   0.109
  every exact check of the onehot mode holds on every route.
Measured coefficients (they cover __expf / v_exp_f32, __logf and the accumulation order and cannot be derived).  Rule: the worst value seen
on the MI355X, doubled, then the next power of two above.
  C_F32    worst |y - r| / (TAU (A + AD)):  generic fp32 o 7.20, dV 12.92, dQ 0.62, dK 2.49; dropout fp32 o 8.91, dV 6.61, dQ 4.61,
           dK 3.49.  Worst 12.92 (hard mode, hd 128: 128 fp32 products of size ~5 summed to a raw score near 680) -> 25.8 -> C_F32 = 32
  K_DELTA  worst |delta - D| / (2^-23 A_D), fp32:  1.87, dropout 1.49 -> 3.74 -> K_DELTA = 4
  K_LSE    worst |lse - r| / (2^-23 max(1, |lse|, max|s|)):
           attn_causal_fwd_generic fp32   9.22 (dropout 3.93)            -> 18.4 -> 32
           attn_causal_fwd_generic bf16   1.64 (hd 16 / 32: 1.42, dropout 1.40) -> 3.3 -> 4
           attn_causal_fwd_v2 bf16        1.76 (dropout 1.68)            -> 3.5  -> 4
           attn_causal_fwd_fast bf16      3.46                           -> 6.9  -> 8
One thing the exact mode showed about the hardware, not a defect: where the dO of a key's queries cancel to zero, the bf16 kernels return
-2^-23 or -2^-22, never a positive value -- as if the MFMA's adder truncated the 1e-14-sized off-target terms toward minus infinity on
the grid of the cancelled terms (a supposition; only the values were observed).  That is inside TAU A_dV, which is why zero-sum elements
are held to 2^-30 sum|dO| + TAU A_dV and only non-zero sums bitwise.
The whole file takes about 6 s on an MI355X box, each test about a second.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import attn_rowwise_check as CHK  # noqa: E402

TENSORS = ("o", "lse", "delta", "dv", "dq", "dk")
_done = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _family(fam):
    """runs and judges every (case, mode) of a family once: (failures, worst ratio per (dtype, tensor), [(case, fwd kernel, bwd kernel)])"""
    if fam in _done:
        return _done[fam]
    fails, worst, ran = [], {}, []
    for c in CHK.CASES:
        if c["family"] != fam:
            continue
        for mode in c["modes"]:
            ins, ref, got, (kf, kb) = CHK.run(c, mode)
            if kf != c["fwd"]:
                fails.append(f"{c['name']} {mode}: the forward took {kf}, not {c['fwd']}")
            if c["bwd_layout"] is not None and kb != c["bwd"]:
                fails.append(f"{c['name']} {mode}: the backward took {kb}, not {c['bwd']}")
            f, w = CHK.judge(c, mode, ins, ref, got)
            fails += f
            for k, v in w.items():
                if k == "lse":                      # per forward kernel, in units of 2^-23 max(1, |lse|, max|s|): what K_LSE is chosen from
                    k, v = "lse " + c["fwd"], v * CHK.K_LSE[(c["fwd"], c["dtype"])]
                worst[(c["dtype"], k)] = max(worst.get((c["dtype"], k), 0.0), v)
        ran.append((c, kf, kb))
    _done[fam] = (fails, worst, ran)
    return _done[fam]


def _check(fam):
    _dev()
    fails, worst, _ = _family(fam)
    for dt in ("bf16", "f32"):
        if any(d == dt for d, _ in worst):
            print(f"\n{fam} {dt}: worst |y - r| / bound  " + "  ".join(f"{k} {worst[(dt, k)]:.3f}" for k in TENSORS if (dt, k) in worst))
            # the measured coefficients in units of their own scale (bound = coefficient * scale): what C_F32, K_DELTA and K_LSE are chosen from
            meas = [f"{k} / (2^-23 max(1, |lse|, max|s|)) {v:.2f}" for (d, k), v in sorted(worst.items()) if d == dt and k.startswith("lse")]
            if dt == "f32":
                meas += [f"{k} / (TAU (A + AD)) {worst[(dt, k)] * CHK.C_F32:.2f}" for k in ("o", "dv", "dq", "dk") if (dt, k) in worst]
                meas += [f"delta / (2^-23 A_D) {worst[(dt, 'delta')] * CHK.K_DELTA:.2f}"] if (dt, "delta") in worst else []
            print(f"{fam} {dt}: measured  " + ";  ".join(meas))
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


def test_generic_fp32():
    _check("f32_generic")


def test_generic_bf16_hd16_hd32():
    _check("bf16_generic")


def test_generic_bf16_hd64_unaligned():
    _check("bf16_generic64")


def test_v2_forward_fast64_backward():
    _check("v2_fast64")


def test_fast128_forward_generic_backward():
    _check("fast128")


def test_dropout_variants():
    _check("dropout")


def test_every_required_route_and_feature_was_reached():
    _dev()
    ran = []
    for fam in CHK.FAMILIES:
        ran += _family(fam)[2]
    got = CHK.reached(ran)
    missing = {k: sorted(f - got.get(k, set())) for k, f in CHK.REQUIRED.items() if not f <= got.get(k, set())}
    assert not missing, missing
