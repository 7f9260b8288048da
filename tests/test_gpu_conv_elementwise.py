"""Every bf16 convolution forward kernel and every data-gradient launch, element by element against fp64.

The rest of the suite judges a bf16-output convolution by one number, max|y - ref| / max|ref| < 1e-2 ... 3e-2.  One product dropped from
one output pixel moves that number by 6e-3 (Cin = 128), an output truncated instead of rounded by 4e-3: both pass.  Here
tests/helpers/conv_elementwise_check.py runs, in one child process per dispatch setting (the switches are read once per process),
``ops.conv_fwd_raw`` and the data gradient of ``ops.norm_act_conv`` (``requires_grad`` on x only: the transposed image, conv_s2_dgrad,
conv_up2_dgrad, or the zero_stuff2x / sumpool2x fallbacks) for conv1x1, conv_thin_fwd / _out, conv_s2_fwd / _dgrad, the general conv_fwd
instances (3x3, 1x1, 4x4 stride 1 and 2, stride 2, bf16 -> fp32, fp32 -> fp32), conv3x3_wide, conv3x3_stream (8- and 16-row tiles) and
conv_up2_fwd / _dgrad at few-tile shapes, and records the kernel each launch took.  All judging is here, on the CPU, in two operand modes:

  * gauss: x, dy, res = randn().bfloat16(), w = randn() / sqrt(K) rounded to bf16, fp32 bias.  r = the fp64 convolution of exactly those
    operands (Upsample and padding applied first), S = the same convolution of the absolute values + |b| + |res|.  EVERY element must
    satisfy |y - r| <= 2^-8 (|r| + TAU S) + TAU S: half a bf16 ulp under round-to-nearest-even (derived) on top of the fp32 accumulation
    of the products (TAU = 2^-18, the weight-gradient suite's value for the same MFMA accumulation); fp32 outputs: TAU S alone.  Affine
    prologues use power-of-two scales and shifts that are multiples of 1/4 (x * s + b is then the same fp32 number on both sides) and keep
    TAU; affine + SiLU (exp2 / rcp sigmoid in the kernel: a few operands round to the neighbouring bf16 value) uses TAU_ACT = 2^-13.
  * int: small integer operands with K max|x| max|w| + max|b| + max|res| < 2^24, so every partial sum is exact in fp32 in any order
    and the output must equal r.float().bfloat16() BITWISE (fp32 outputs: r itself).  Every tap carries its own offset, rotating with
    o and i.  Before a kernel's output is looked at, the reference alone must show teeth: at least 25 % of |r| above 256 and at least 5 %
    exact bf16 ties, for every prologue-free case (the ranges of the thin K = 72 and the other small-K cases are widened until they hold).

Two references follow the arithmetic the library documents instead of the plain formula (both restated in the helper and checked against
the plain one in tests/test_conv_elementwise_cpu.py):
  * the sub-pixel kernels (conv_up2_fwd / _dgrad) are handed phase filters = sums of up to four taps added in fp32 and rounded ONCE to
    bf16 (include/mas_hip.h, MAS_WLAYOUT_UP2).  In gauss mode their r and S are the fp64 convolution with those rounded phase filters: against
    the nine bf16 taps the outputs differ by the phase filters' own rounding, 2^-9 of each filter element, which TAU S cannot hold
    (PLAIN_UP2 below records it).  In int mode the sums are exact and the plain Upsample + conv reference is used bitwise.
  * the Upsample fold's fallback data gradient rounds twice: the 3x3 kernel writes the high-resolution gradient in bf16 and sumpool2x
    adds four of them in fp32 and rounds again.  Its bound is the composed one (``two_stage_bound``), its int-mode value the two roundings.

REQUIRED lists what the union of the children has to reach; a dispatch change that makes a case vacuous fails here.

Measured worst |y - r| / bound per family on an MI355X (1 = the bound), TAU = 2^-18, TAU_ACT = 2^-13:
  forward, TAU:      conv3x3_wide 0.991, conv3x3_stream 0.990, conv_up2_fwd 0.993, conv1x1 0.987, conv_thin_fwd 0.989, conv_thin_out 0.968,
                     conv_s2_fwd 0.983, conv_fwd 0.989 (fp32 outputs, TAU S alone: bf16 -> fp32 0.018, fp32 -> fp32 0.056)
  forward, TAU_ACT:  affine + SiLU conv3x3_wide 0.863, conv3x3_stream 0.869, conv_fwd 0.922
  data gradient:     conv3x3_wide 0.985, conv3x3_stream 0.986, conv_up2_dgrad 0.984, conv1x1 0.979, conv_thin_fwd 0.990, conv_thin_out 0.967,
                     conv_s2_dgrad 0.989, conv_fwd 0.986, zero_stuff2x + conv3x3_stream 0.986, zero_stuff2x + conv_fwd 0.979,
                     + sumpool2x (composed bound): conv3x3_wide 0.800, conv3x3_stream 0.831, conv_fwd 0.820
  The bf16 figures sit just under 1 because the bound IS the rounding: the worst element is a near-tie, at 0.99 of half an ulp, and what
  the accumulation adds is far below TAU S (the fp32-output figures show it alone: 2-6 % of TAU S).  Every int-mode case is bitwise equal.
  PLAIN_UP2, the sub-pixel kernels against the nine bf16 taps instead of the rounded phase filters: conv_up2_fwd 135, conv_up2_dgrad 44.
The whole file (7 children) takes ~30 s on an MI355X box, half of it the fp64 references on the CPU."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import conv_elementwise_check as CHK  # noqa: E402

CHILD = os.path.join(HERE, "helpers", "conv_elementwise_check.py")
CHILD_TIMEOUT = 240
TAU, TAU_ACT = 2.0 ** -18, 2.0 ** -13
SWITCHES = ("MAS_CONV_WIDE", "MAS_CONV_WIDE_MIN_TILES_PER_CU", "MAS_CONV_WIDE_ANY_WIDTH", "MAS_CONV_UP2", "MAS_CONV_S2", "MAS_CONV_STREAM",
            "MAS_CONV_STREAM_TH8", "MAS_CONV_STREAM_MIN_TILES_PER_CU", "MAS_CONV_WGS_PER_CU", "MAS_CONV1X1", "MAS_CONV_THIN", "MAS_CONV_THIN_OUT")

WIDE, STREAM, UP2F, UP2D, GEN = CHK.WIDE, CHK.STREAM, CHK.UP2F, CHK.UP2D, CHK.GEN
REQUIRED = {
    "conv1x1": {"ragged_m", "chunks3", "chunks7", "cout_tiles2", "res", "dgrad"},
    "conv_thin_fwd": {"fwd", "dgrad"},
    "conv_thin_out": {"fwd", "dgrad"},
    "conv_s2_fwd": {"even", "odd", "cout_tiles2"},
    "conv_s2_dgrad": {"even", "odd"},
    GEN: {"bc32", "bc128", "res", "affine", "silu", "k1", "k3s2", "k4s2", "k4s1", "bf16_f32", "f32_f32"},
    WIDE: {"one_tile", "ragged", "cin64", "cin128", "cin256", "cin512", "cout_tiles2", "cout_tiles4", "res", "pad2", "transposed", "affine",
           "silu", "upfold", "sumpool_dgrad", "multi_tile"},
    UP2F: {"ragged", "cin64", "cin128", "cout_tiles2", "pad8", "multi_tile"},
    UP2D: {"ragged", "cin64", "cin128", "cout_tiles2", "pad8"},
    STREAM: {"th8", "th16", "th16_plain", "ragged", "cin128", "cin256", "cout_tiles2", "res", "affine", "silu", "upfold"},
    "zero_stuff2x": {"pad2_dgrad"},
}
TEETH_ABOVE, TEETH_TIES = 0.25, 0.05


def _run_children(tmp_path):
    env0 = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    got = {}
    for label, extra, _ in CHK.SETTINGS:       # one at a time; the first failure ends the test (no further child, no retry)
        out = str(tmp_path / f"conv_{label}.pt")
        try:
            p = subprocess.run([sys.executable, CHILD, label, out], env={**env0, **extra}, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"child {label} timed out after {CHILD_TIMEOUT} s\n{e.stdout or ''}\n{e.stderr or ''}")
        if p.returncode != 0:
            pytest.fail(f"child {label} exited with {p.returncode}\n{p.stdout}\n{p.stderr[-6000:]}")
        got[label] = torch.load(out)
    return got


def _matches(want, names):
    """does the recorded launch list match a case's expectation ("*" = anything)"""
    want = (want,) if isinstance(want, str) else tuple(want)
    return want == ("*",) or (len(want) == len(names) and all(w in ("*", k) for w, k in zip(want, names)))


def _has_teeth(c):
    return c["act"] == CHK.ACT_NONE              # (an affine prologue makes r a multiple of 1/4: the tie count is defined for integers)


def judge(c, mode, rec, failures, worst, rows, plain_up2):
    """every check of one (case, mode) recording; returns the (kernel, feature) pairs it reached"""
    ins = CHK.make_inputs(c, mode)
    name, gauss = c["name"], mode == "gauss"
    silu = c["act"] == CHK.ACT_AFFINE_SILU
    tau = TAU_ACT if silu else TAU
    out_bf16 = c["out"] == "bf16"
    launches = [("y", rec["fwd_kernel"])] + ([("y_nac", rec["nac_fwd_kernel"])] if "y_nac" in rec else [])
    if not _matches(c["fwd"], [rec["fwd_kernel"]]):
        failures.append(f"{name} {mode}: forward took {rec['fwd_kernel']}, not {c['fwd']}")
    ran = {k for _, k in launches}
    cache = {}
    for key, kern in launches:
        phases = gauss and kern == UP2F
        if phases not in cache:
            cache[phases] = CHK.reference_fwd(c, ins, phases=phases, mags=gauss)
        r, s = cache[phases]
        fam = kern + (":silu" if silu else "")
        if gauss:
            ratio, bad = CHK.gauss_ratio(rec[key], r, s, tau, out_bf16)
            worst[fam] = max(worst.get(fam, 0.0), ratio)
            rows.append((name, key, kern, f"{ratio:.3f}", ""))
            if bad:
                failures.append(f"{name} gauss {key} ({kern}): {bad} of {r.numel()} elements outside the bound, worst |y - r| / bound = {ratio:.3f}")
            if kern == UP2F and key == "y":          # for the record: the same output against the nine bf16 taps
                rp, sp = CHK.reference_fwd(c, ins)
                plain_up2[UP2F] = max(plain_up2.get(UP2F, 0.0), CHK.gauss_ratio(rec[key], rp, sp, tau)[0])
        else:
            above, ties = CHK.int_teeth(r) if c["act"] == CHK.ACT_NONE else (float("nan"), float("nan"))
            if _has_teeth(c):     # on the reference alone, before the kernel's output is looked at
                assert above >= TEETH_ABOVE and ties >= TEETH_TIES, (name, "forward reference has no teeth", above, ties)
            eq, nd = CHK.int_equal(rec[key], r, out_bf16)
            rows.append((name, key, kern, f">256 {above:.2f} ties {ties:.2f}", "equal" if eq else f"{nd} DIFFER"))
            if not eq:
                failures.append(f"{name} int {key} ({kern}): {nd} of {r.numel()} elements differ from the exactly rounded reference")
    if c["dgrad"] is not None:
        names = rec["dgrad_kernels"]
        ran |= set(names)
        if not _matches(c["dgrad"], names):
            failures.append(f"{name} {mode}: data gradient took {names}, not {c['dgrad']}")
        two_stage, phases = names[-1] == "sumpool2x", gauss and UP2D in names
        kern = "+".join(names)
        r, s = CHK.reference_dgrad(c, ins, phases=phases, high_res=two_stage, mags=gauss)
        if gauss:
            if two_stage:
                r, bound = CHK.two_stage_bound(r, s, tau)
                ratio, bad = CHK.gauss_ratio(rec["dx"], r, None, tau, bound=bound)
            else:
                ratio, bad = CHK.gauss_ratio(rec["dx"], r, s, tau, out_bf16)
            worst[kern + " (dgrad)"] = max(worst.get(kern + " (dgrad)", 0.0), ratio)
            rows.append((name, "dx", kern, f"{ratio:.3f}", ""))
            if bad:
                failures.append(f"{name} gauss dx ({kern}): {bad} of {r.numel()} elements outside the bound, worst |dx - r| / bound = {ratio:.3f}")
            if UP2D in names:
                rp, sp = CHK.reference_dgrad(c, ins)
                plain_up2[UP2D] = max(plain_up2.get(UP2D, 0.0), CHK.gauss_ratio(rec["dx"], rp, sp, tau)[0])
        else:
            above, ties = CHK.int_teeth(r)
            if _has_teeth(c):
                assert above >= TEETH_ABOVE and ties >= TEETH_TIES, (name, "data-gradient reference has no teeth", above, ties)
            expected = CHK.int_expected_two_stage(r) if two_stage else None
            eq, nd = CHK.int_equal(rec["dx"], r, out_bf16, expected=expected)
            rows.append((name, "dx", kern, f">256 {above:.2f} ties {ties:.2f}", "equal" if eq else f"{nd} DIFFER"))
            if not eq:
                failures.append(f"{name} int dx ({kern}): {nd} of {rec['dx'].numel()} elements differ from the exactly rounded reference")
    reached = {(k, f) for k, f in c["want"] if k in ran}
    feats = rec["features"]
    if rec["fwd_kernel"] == STREAM:
        reached.add((STREAM, "th8" if "th8" in feats else ("th16" if c["act"] != CHK.ACT_NONE else "th16_plain")))
    if "tiles_gt_grid" in feats:
        reached.add((rec["fwd_kernel"], "multi_tile"))
    return reached


def test_every_conv_forward_and_data_gradient_element_by_element_vs_fp64(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    got = _run_children(tmp_path)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    failures, worst, plain_up2, reached = [], {}, {}, set()
    for label, _, cases in CHK.SETTINGS:
        rows = []
        for c in cases:
            for mode in CHK.MODES:
                rec = got[label]["results"].get((c["name"], mode))
                if rec is None:
                    assert mode == "int" and c["act"] == CHK.ACT_AFFINE_SILU, (label, c["name"], mode)     # SiLU: gauss mode only
                    continue
                reached |= judge(c, mode, rec, failures, worst, rows, plain_up2)
        for name, key, kern, fig, eq in rows:
            print(f"{label:12s} {name:18s} {key:6s} {kern:32s} {fig:24s} {eq}")
    print("worst |y - r| / bound per family (gauss mode):")
    for fam in sorted(worst):
        print(f"  {fam:40s} {worst[fam]:.3f}")
    print("sub-pixel kernels against the nine bf16 taps instead of the rounded phase filters: " +
          ", ".join(f"{k} {v:.1f}" for k, v in sorted(plain_up2.items())))
    for kern, want in REQUIRED.items():
        missing = sorted(f for f in want if (kern, f) not in reached)
        if missing:
            failures.append(f"{kern}: no child reached {missing}")
    assert not failures, "\n".join(failures[:60])
