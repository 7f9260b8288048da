"""The CPU side of tests/test_gpu_bn_elementwise.py, checked without a GPU (tests/helpers/bn_elementwise_check.py):

  * the fp64 references equal ``F.batch_norm`` (+ LeakyReLU) and its autograd in float64 on the same operands, running statistics included;
  * the launch geometry the helper restates agrees with the constants in csrc/batchnorm.hip and gives what the cases were chosen for;
  * a model of every kernel's arithmetic in the kernel's own order stays inside EVERY bound for every case in both operand modes and
    meets every int-mode equality, the operand conditions hold (ambiguous share <= 1e-4, at least 5 % exact bf16 ties, u == 0 planted),
    and the models reach every (kernel, feature) pair the GPU test's REQUIRED table lists;
  * teeth: each planted error of TEETH drives the same judge outside a bound or breaks an int-mode equality.

What the bounds cannot resolve is said here instead of forced: ``eps_missing`` is caught in gauss mode only (the int-mode table is
synthetic and the integer variance ~2e4 hides 1e-5), ``ge_at_zero`` in int mode only (gauss mode has no u == 0), and a momentum taken as
the fp64 0.1 instead of the fp32 value differs by U / 4 of mom (mean - running_mean): below the one fp32 rounding of the result except
in the channels whose running_mean was seeded to cancel the update (c % 8 == 5), where it is caught."""
import importlib.util
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import bn_elementwise_check as CHK  # noqa: E402

DIRECT = CHK.direct_cases()
CASES = {c["name"]: c for c in DIRECT + CHK.WRAP_CASES}
_records = {}


def _judge_model(c, mode, plant=None):
    key = (c["name"], mode, plant)
    if plant is not None:
        return CHK.judge(c, mode, CHK.model_record(c, mode, plant))
    if key not in _records:
        _records[key] = CHK.judge(c, mode, CHK.model_record(c, mode))
    return _records[key]


def _modes(c):
    return CHK.MODES if c["kind"] == "direct" else ("gauss",)


@pytest.mark.parametrize("c", CHK.WRAP_CASES, ids=lambda c: c["name"])
def test_reference_is_batch_norm_in_float64(c):
    ins = CHK.make_inputs(c)
    ch, m = c["c"], c["m"]
    rm, rv = torch.zeros(ch, dtype=torch.float64), torch.ones(ch, dtype=torch.float64)
    zero = torch.zeros(ch, dtype=torch.float64)
    close = lambda a, b, what: (float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())) or pytest.fail(f"{what}: {float((a - b).abs().max())}"))
    for step in range(CHK.WRAP_STEPS + 1):
        ref = CHK.wrap_reference(c, ins, step, rm, rv, zero, zero, step + 1)
        x = ins["x"][step].double().requires_grad_(True)
        ga = ins["gamma"].double().requires_grad_(True) if c["affine"] else None
        be = ins["beta"].double().requires_grad_(True) if c["affine"] else None
        mom = (CHK.f32(c["momentum"]) if c["momentum"] is not None else 1.0 / (step + 1)) if step < CHK.WRAP_STEPS else 0.0
        trm, trv = rm.clone(), rv.clone()
        y = F.batch_norm(x, trm, trv, ga, be, training=step < CHK.WRAP_STEPS, momentum=mom, eps=CHK.f32(CHK.EPS))
        y = F.leaky_relu(y, CHK.f32(c["slope"])) if c["slope"] != 1.0 else y
        y.backward(ins["dy"][step].double())
        close(ref["y"][0], y.detach(), "y")
        close(ref["dx"][0][0], x.grad, "dx")
        if c["affine"]:
            close(ref["dgamma"][0], ga.grad, "dgamma")
            close(ref["dbeta"][0], be.grad, "dbeta")
        if step < CHK.WRAP_STEPS:
            close(ref["running_mean"][0], trm, "running_mean")
            close(ref["running_var"][0], trv, "running_var")
            rm, rv = trm, trv
        assert all(float(v[1].min()) > 0 for k, v in ref.items() if k in ("y", "dgamma", "dbeta", "running_mean", "running_var"))


def test_restated_geometry():
    src = open(os.path.join(os.path.dirname(HERE), "make-a-scene_amd", "csrc", "batchnorm.hip")).read()
    for pattern in (r"constexpr int NT = 256;", r"constexpr int BN_ROWS_PER_BLOCK = 128;", r"constexpr int BN_MAX_BLOCKS = 1024;",
                    r"quads = C / 4, R = NT / quads > 0 \? NT / quads : 1", r"q = tid % quads, rl = tid / quads", r"for \(; b \+ 8 <= nblk; b \+= 8\)",
                    r"rows_per_block = mas_cdiv\(M, nblk\)", r"cap = 8LL \* mas_num_cus\(\)", r"q = \(int\)\(i % quads\)", r"u > 0\.0f \? u : u \* slope",
                    r"> 0\.0f\) \? d : d \* slope", r"\(float\)\(sums\[c\] / n\), k2 = \(float\)\(sums\[C \+ c\] / n\)", r"var \* n / \(n - 1\.0\)"):
        assert re.search(pattern, src), pattern
    by = {c["name"]: c for c in DIRECT}
    geo = lambda n: (CHK.quads(by[n]["c"]), CHK.row_lanes(by[n]["c"]), CHK.bn_blocks(by[n]["m"]), CHK.rows_per_block(by[n]["m"]))
    assert geo("c4_m2") == (1, 256, 1, 2) and geo("c4_m129") == (1, 256, 2, 65)
    assert geo("c12_m129") == (3, 85, 2, 65) and 3 * 85 == 255                          # thread 255 idle
    assert geo("c256_m300")[:2] == (64, 4) and geo("c1024_m131_bf")[:2] == (256, 1)
    assert [geo(n)[2] for n in ("c64_m800", "c64_m1024_bf", "c64_m1100")] == [7, 8, 9]
    assert geo("c4_m131073")[2:] == (1024, 129) and CHK.empty_blocks(131073) == 7        # blocks 1017 .. 1023
    assert CHK.stride_rows(256) == 4099 and 4099 * 512 // 4 > 8 * 256 * 256 > 4096 * 512 // 4 - 1
    assert max(c["m"] * c["c"] for c in DIRECT) == 4099 * 512
    for c in DIRECT:                                                                       # the kernels' own limits
        assert c["c"] % 4 == 0 and c["c"] <= 4 * CHK.NT and CHK.row_lanes(c["c"]) * 2 * c["c"] * 8 <= 65536


@pytest.mark.parametrize("c", DIRECT + CHK.WRAP_CASES, ids=lambda c: c["name"])
def test_model_stays_inside_every_bound(c):
    worst = {}
    for mode in _modes(c):
        rows, reached, failures = _judge_model(c, mode)
        for key, fam, fig, verdict in rows:
            print(f"{c['name']:24s} {mode:5s} {key:20s} {fam:44s} {fig:>8s} {verdict}")
            if mode == "gauss":
                worst[fam] = max(worst.get(fam, 0.0), float(fig))
        assert not failures, "\n".join(failures)
        assert rows and reached
    assert all(v <= 1 for v in worst.values()), worst


def test_models_reach_every_required_feature():
    spec = importlib.util.spec_from_file_location("_bn_gpu_test", os.path.join(HERE, "test_gpu_bn_elementwise.py"))
    gpu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gpu)
    reached = set()
    for c in DIRECT + CHK.WRAP_CASES:
        for mode in _modes(c):
            reached |= _judge_model(c, mode)[1]
    for part, table in gpu.REQUIRED.items():
        for kern, want in table.items():
            assert not sorted(f for f in want if (kern, f) not in reached), (part, kern, sorted(f for f in want if (kern, f) not in reached))


def test_operand_conditions_on_the_references():
    """the ambiguous share and the int-mode teeth, printed (``judge`` asserts them before it looks at any output)"""
    for c in DIRECT:
        for mode in CHK.MODES:
            ins = CHK.make_inputs(c, mode)
            t = CHK.bwd_terms(ins["x"], ins["dy"], ins["mr"], ins["ss"], ins["slope"], exact=mode == "int")
            line = f"{c['name']:16s} {mode:5s} ambiguous {int(t['amb'].sum())} of {t['amb'].numel()}"
            assert CHK.ambiguous_share(t) <= CHK.AMBIGUOUS_SHARE
            if mode == "int":
                zeros = int((t["u"] == 0).sum())
                line += f", u == 0 at {zeros} ({zeros / t['amb'].numel():.2%})"
                if c["dt"] == "bf16":
                    ry, _ = CHK.apply_reference(ins["x"], ins["ss"], ins["slope"], "bf16")
                    r0, _ = CHK.apply_reference(ins["x"], ins["ss"], 0.0, "bf16")
                    rd = CHK.bwd_apply_reference(t, ins["gamma"], ins["mr"], ins["bsums"], "bf16")[0][0]
                    ties = [CHK.bf16_ties(r) for r in (ry, r0, rd)]
                    line += ", bf16 ties y %.3f, y at slope 0 %.3f, dx %.3f" % tuple(ties)
                    assert min(ties) >= CHK.TEETH_TIES
            print(line)


# planted error -> (the cases it is planted into, the modes that must catch it in EVERY one of them)
BOTH = CHK.MODES
TEETH = {
    "last_row_dropped": (["c12_m129", "c64_m800"], BOTH),
    "lane_twice": (["c4_m129", "c256_m300"], BOTH),
    "fold_remainder_skipped": (["c64_m800", "c64_m1100"], BOTH),
    "biased_running_var": (["c4_m2", "c256_m300"], BOTH),
    "local_count": (["c256_glob"], BOTH),
    "momentum_fp64": (["c256_m300"], ("gauss",)),
    "eps_missing": (["c64_m800", "sync_12"], ("gauss",)),
    "ge_at_zero": (["c64_m800", "c128_patch_bf"], ("int",)),
    "slope_on_positive": (["c64_m800", "c12_m129_bf", "leaky_f32_02"], BOTH),
    "k_swapped": (["c256_m300", "c12_m129_bf"], BOTH),
    "q_mask": (["c12_m129", "c12_m129_bf", "sync_12"], BOTH),
    "bf16_truncate": (["c12_m129_bf", "c128_patch_bf", "leaky_bf16_02"], BOTH),
    "rstd_off_one_channel": (["c64_m800", "sync_64_cumulative", "leaky_f32_02"], ("gauss",)),
    "dgamma_small_gamma": (["c64_m800", "sync_64_cumulative", "leaky_bf16_02"], BOTH),
}


@pytest.mark.parametrize("kind", sorted(TEETH))
def test_teeth_planted_error_is_caught(kind):
    names, modes = TEETH[kind]
    for name in names:
        c = CASES[name]
        for mode in (m for m in modes if m in _modes(c)):
            assert not _judge_model(c, mode)[2], (name, mode, "the unmutated model fails")
            _, _, failures = _judge_model(c, mode, kind)
            print(f"teeth {kind:24s} {name:20s} {mode:5s}: {len(failures)} checks fail" + (f" ({failures[0]})" if failures else ""))
            assert failures, (kind, name, mode, "not caught")
