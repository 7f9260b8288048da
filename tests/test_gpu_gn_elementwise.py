"""Every GroupNorm kernel, element by element against fp64.

The rest of the suite judges GroupNorm by one number per tensor, max|got - ref| / max|ref| against torch's fp32: a group that is wrong
beside a group with larger values passes, and so does one image whose rstd is 1 % off, or a ragged tile whose out-of-map pixel was
counted.  Here tests/helpers/gn_elementwise_check.py runs, in one child process per dispatch setting, every kernel of
csrc/groupnorm.hip (``gn_stats`` + ``gn_act`` in bf16 and fp32 through both branches of gn_stats_partial, the small-map forward at
every UNITS instance and both thread counts, the small-map backward + gn_param_reduce, the three-launch backward on the packed bf16
and the generic fp32 kernels) and the fused statistics of conv3x3_wide and conv_up2_fwd through ``gn_stats_from_partials`` at few-tile
shapes and at more tiles than work-groups, and records every output and the kernel each launch took.  All judging is on the CPU
(``judge`` in the helper; every bound is derived in the helper's docstring from the kernels' arithmetic), in two operand modes:

  * gauss: x = randn * sigma + mu with (mu, sigma) rotating over (image, group) through (0.3, 1.5), (8, 1), (-20, 0.5), so one tensor
    holds easy and 40-sigma groups side by side; EVERY element of mean_rstd, scale_shift (against the kernel's own mean_rstd), a (against
    the kernel's own scale_shift), dx, dgamma, dbeta and of the statistics tables must be inside its bound;
  * int: integers with an integer offset per group (up to +-100), every fp32 sum below 2^24: mean bitwise equal to float(mu), rstd within
    one fp32 ulp, table rows / column sums, dgamma, dbeta (synthetic power-of-two table) and gn_act on a power-of-two table bitwise.

REQUIRED lists the (kernel, feature) pairs the children have to reach; a dispatch change that leaves a case vacuous fails here.
The multi child's cases are 136 and 33 images of 16 x 32: the smallest counts whose tiles exceed one work-group per CU on 256 CUs, which
is what makes one tile's statistics flush overlap the next tile's first stage.

Measured worst |error| / bound per family on an MI355X (1 = the bound), gauss mode:
  mean / rstd:  gn_stats_partial fixed bf16 0.043 / 0.055, fixed fp32 0.114 / 0.078, atomic bf16 0.011 / 0.034, atomic fp32 0.025 / 0.024;
                gn_small_fwd UNITS 1 / 2 / 4 / 8 / 16: mean 0.000 / 0.006 / 0.026 / 0.018 / 0.012, rstd 0.026 / 0.059 / 0.085 / 0.036 / 0.038;
                gn_stats_from_partials fed by conv3x3_wide 0.000 / 0.002, by conv_up2_fwd 0.000 / 0.002 (the bound there is mostly the
                convolution's own TAU S per term); statistics tables: conv3x3_wide rows 0.005, columns 0.002, conv_up2_fwd columns 0.002
  scale_shift:  sc 0.91 ... 0.996 in every family (one fp32 rounding IS the bound), sh 0.43 ... 0.50 (an fma: half of the two roundings allowed)
  a:            gn_act bf16 affine 0.996, SiLU 0.995; fp32 affine 0.499, SiLU 0.442; gn_small_fwd 0.996 / 0.996 and bitwise mas_gn_act on its table
  dx:           gn_small_bwd UNITS 1 / 2 / 4 / 8: 0.496 / 0.993 / 0.993 / 0.995, gn_bwd_apply_pk 0.996, gn_bwd_apply<float> 0.257
  dgamma:       gn_small_bwd 0.344 / 0.060 / 0.028 / 0.036, gn_bwd_apply_pk 0.010, gn_bwd_apply<float> 0.025
  dbeta:        gn_small_bwd 0.017 / 0.014 / 0.004 / 0.006, gn_bwd_apply_pk 0.014, gn_bwd_apply<float> 0.011
  The bf16 a / dx figures sit just under 1 because their bound is the rounding itself (a near-tie at 0.99 of half an ulp); what the fp32
  arithmetic adds shows alone in the fp32 tensors and in the sums: a tenth of the worst-case chain bound or less.
int mode: every equality holds (mean, table rows and column sums, dgamma, dbeta, gn_act on the power-of-two table: all "equal"), every
rstd is bitwise the rounded fp64 value (0 ulp of the 1 allowed); dx under the bound without accumulation terms: 0.985 ... 0.996, fp32 0.543.
No kernel defect was found.  The three tests take ~15 s together on an MI355X box, most of it the fp64 convolutions of the multi child."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import gn_elementwise_check as CHK  # noqa: E402

CHILD = os.path.join(HERE, "helpers", "gn_elementwise_check.py")
CHILD_TIMEOUT = 240
SWITCHES = ("MAS_CONV_WIDE", "MAS_CONV_WIDE_MIN_TILES_PER_CU", "MAS_CONV_WIDE_ANY_WIDTH", "MAS_CONV_UP2", "MAS_CONV_WGS_PER_CU", "MAS_GN_SMALL",
            "MAS_FUSED_GN_STATS", "MAS_GN_ACT_BLOCKS", "MAS_GN_APPLY_BLOCKS", "MAS_GN_ACT_REV", "MAS_GN_ACT_NT")
WIDE, UP2F = CHK.WIDE, CHK.UP2F
REQUIRED = {
    "forward": {
        "gn_stats_finalize": {"fixed", "atomic"},
        "gn_act": {"bf16", "f32"},
        "gn_small_fwd": {"units1", "units2", "units4", "units8", "units16"},
    },
    "backward": {
        "gn_param_reduce": {"units1", "units2", "units4", "units8", "act1_res0", "act1_res1", "act2_res0", "act2_res1"},
        "gn_bwd_apply": {"packed", "generic"},
    },
    "fused": {
        "gn_stats_from_partials": {f"{WIDE}:one_tile", f"{WIDE}:ragged", f"{WIDE}:narrow_last_column", f"{WIDE}:cout_tiles2", f"{WIDE}:res",
                                   f"{WIDE}:tiles_gt_grid", f"{UP2F}:ragged", f"{UP2F}:cout_tiles2", f"{UP2F}:tiles_gt_grid"},
    },
}
_children = {}          # label -> loaded recording, or an error text: a child runs once per session, and after a failure none is started


def _child(label, tmp_path_factory):
    broken = [v for v in _children.values() if isinstance(v, str)]
    if broken:
        pytest.fail("an earlier child failed; no further child is started\n" + broken[0][:2000])
    if label not in _children:
        extra = next(e for s, e, _ in CHK.SETTINGS if s == label)
        env0 = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        out = str(tmp_path_factory.mktemp("gn") / f"gn_{label}.pt")
        try:
            p = subprocess.run([sys.executable, CHILD, label, out], env={**env0, **extra}, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            if p.returncode != 0:
                _children[label] = f"child {label} exited with {p.returncode}\n{p.stdout}\n{p.stderr[-6000:]}"
            else:
                _children[label] = torch.load(out)
        except subprocess.TimeoutExpired as e:
            _children[label] = f"child {label} timed out after {CHILD_TIMEOUT} s\n{e.stdout or ''}\n{e.stderr or ''}"
    if isinstance(_children[label], str):
        pytest.fail(_children[label])
    return _children[label]["results"]


def _judge_all(part, cases_by_label, tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    failures, worst, reached = [], {}, set()
    for label, cases in cases_by_label:
        got = _child(label, tmp_path_factory)
        for c in cases:
            for mode in CHK.MODES:
                rows, r, f = CHK.judge(c, mode, got[(c["name"], mode)])
                reached |= r
                failures += f
                for key, fam, fig, verdict in rows:
                    print(f"{label:8s} {c['name']:16s} {mode:5s} {key:22s} {fam:44s} {fig:>10s} {verdict}")
                    if verdict != "equal" and mode == "gauss":
                        worst[fam] = max(worst.get(fam, 0.0), float(fig))
    print(f"worst |error| / bound per family (gauss mode), {part}:")
    for fam in sorted(worst):
        print(f"  {fam:48s} {worst[fam]:.3f}")
    for kern, want in REQUIRED[part].items():
        missing = sorted(f for f in want if (kern, f) not in reached)
        if missing:
            failures.append(f"{kern}: no child reached {missing}")
    assert not failures, "\n".join(failures[:60])


def test_statistics_and_activation_element_by_element_vs_fp64(tmp_path_factory):
    _judge_all("forward", [("default", CHK.STATS_CASES + CHK.SMALL_CASES)], tmp_path_factory)


def test_backward_element_by_element_vs_fp64(tmp_path_factory):
    _judge_all("backward", [("default", CHK.BWD_CASES)], tmp_path_factory)


def test_fused_statistics_tables_vs_fp64(tmp_path_factory):
    _judge_all("fused", [("wide", CHK.FUSED_WIDE), ("multi", CHK.FUSED_MULTI)], tmp_path_factory)
