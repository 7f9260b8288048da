"""The CPU side of tests/test_gpu_gn_elementwise.py, checked without a GPU (tests/helpers/gn_elementwise_check.py):

  * the fp64 references equal ``F.group_norm`` (+ SiLU) and its autograd in float64 on the same operands to 1e-12;
  * the launch geometry the helper restates (``pick_split``, ``rstep``, the small-map thread / unit counts) agrees with the constants
    in csrc/groupnorm.hip and gives what the cases were chosen for; no (N, HW) has an empty trailing split (searched, see below);
  * an fp32 model of every kernel's arithmetic -- the same summation tree in numpy float32, fp64 where the kernel uses fp64 -- stays
    inside EVERY bound for every case in both operand modes and meets every int-mode equality: the operands were chosen so that
    arithmetic of the documented kind passes, before any kernel is looked at;
  * teeth: each of eight planted errors drives the same judge outside a bound or breaks an int-mode equality, planted into the easy
    groups alone (mu = 0.3 sigma-ish) and into the far-mean groups alone (mu = -40 sigma), where the error has groups to live in."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import gn_elementwise_check as CHK  # noqa: E402

GN_CASES = CHK.STATS_CASES + CHK.SMALL_CASES + CHK.BWD_CASES
FUSED_CASES = CHK.FUSED_WIDE + CHK.FUSED_MULTI


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("name", ["st_128_41x55", "st_96_9x13", "sf_32_9x13", "sm_64_1x1", "sm_64_9x13", "sm_128_20x20"])
def test_forward_reference_is_group_norm_in_float64(name):
    c = CHK.CASES[name]
    ins = CHK.make_inputs(c, "gauss")
    x, ga, be = ins["x"].double(), ins["gamma"].double(), ins["beta"].double()
    ref = CHK.stats_reference(x, 1)
    gi = CHK.group_of(c, c["c"])
    sc = ref["rstd"][:, gi] * ga[None]
    ss = torch.stack([sc, be[None] - ref["mean"][:, gi] * sc], -1)
    want = F.group_norm(x, CHK.G, ga, be, eps=CHK.EPS)
    _close(CHK.act_reference(x, ss, CHK.ACT_AFFINE)[0], want, "affine")
    _close(CHK.act_reference(x, ss, CHK.ACT_SILU)[0], want * torch.sigmoid(want), "silu")
    xg = x.reshape(c["n"], CHK.G, -1)
    _close(ref["mean"], xg.mean(-1), "mean")
    _close(ref["rstd"], 1 / torch.sqrt(xg.var(-1, unbiased=False) + CHK.EPS), "rstd")


@pytest.mark.parametrize("name", ["bs_64_1x1", "bs_64_9x13", "b3_32_5x7", "b3_128_41x55", "b3f_128_20x12"])
@pytest.mark.parametrize("act,res", CHK.ACT_RES)
def test_backward_reference_is_autograd_in_float64(name, act, res):
    c = CHK.CASES[name]
    ins = CHK.make_inputs(c, "gauss")
    x = ins["x"].double().requires_grad_(True)
    ga, be = ins["gamma"].double().requires_grad_(True), ins["beta"].double().requires_grad_(True)
    a = F.group_norm(x, CHK.G, ga, be, eps=CHK.EPS)
    if act == CHK.ACT_SILU:
        a = a * torch.sigmoid(a)
    a.backward(ins["da"].double())
    # the exact table instead of the fp32 one the kernel is handed
    st = CHK.stats_reference(ins["x"].double(), 1)
    gi = CHK.group_of(c, c["c"])
    sc = st["rstd"][:, gi] * ins["gamma"].double()[None]
    exact = dict(ins, mr=torch.stack([st["mean"], st["rstd"]], -1), ss=torch.stack([sc, ins["beta"].double()[None] - st["mean"][:, gi] * sc], -1))
    ref = CHK.bwd_reference(c, exact, act, res)
    _close(ref["dx"], x.grad + (ins["dres"].double() if res else 0.0), "dx")
    _close(ref["dgamma"], ga.grad, "dgamma")
    _close(ref["dbeta"], be.grad, "dbeta")
    assert all(float(ref[k].min()) > 0 for k in ("bdx", "bdgamma", "bdbeta"))


def test_restated_geometry():
    src = open(os.path.join(os.path.dirname(HERE), "make-a-scene_amd", "csrc", "groupnorm.hip")).read()
    for pattern in (r"constexpr int NT = 256;", r"constexpr int MAX_SPLIT = 64;", r"constexpr int target = 1024;", r"HW / 64 > 0 \? HW / 64 : 1",
                    r"gn_small_threads\(int HW\) \{ return HW <= 256 \? 256 : 512; \}", r"\(HW \* \(cb / 8\) \+ t - 1\) / t",
                    r"HW <= 512 && gn_small_ok", r"HW <= 1024 && C % 64 == 0 && C % G == 0 && 64 % \(C / G\) == 0", r"if \(NT % upp == 0\)"):
        assert re.search(pattern, src), pattern
    assert (CHK.NT, CHK.MAX_SPLIT) == (256, 64)
    # what the cases were chosen for
    assert CHK.rstep(32, "bf16") == 64 > 5 * 7
    ns = CHK.pick_split(3, 41 * 55)
    rows = -(-41 * 55 // ns)
    assert (ns, rows, 41 * 55 - (ns - 1) * rows) == (35, 65, 45)
    assert [c["name"] for c in CHK.STATS_CASES if not CHK.stream_fixed(c["c"], c["dt"])] == ["st_96_9x13", "st_320_20x12", "sf_96_9x13"]
    assert [w for w in (32, 64, 96, 128, 192, 256, 320, 512) if not CHK.stream_fixed(w, "bf16")] == [96, 192, 320]
    assert all(CHK.stream_fixed(w, "f32") for w in (32, 64, 128, 256)) and not CHK.stream_fixed(96, "f32")
    assert {CHK.small_fwd_instance(h * w) for _, _, h, w in CHK.SMALL_SHAPES} == {1, 2, 4, 8, 16}
    assert {CHK.small_threads(h * w) for _, _, h, w in CHK.SMALL_SHAPES} == {256, 512}
    assert {CHK.small_bwd_instance(c["hw"]) for c in CHK.BWD_CASES if CHK.bwd_family(c)[0] == "small"} == {1, 2, 4, 8}
    assert {CHK.bwd_family(c)[0] for c in CHK.BWD_CASES} == {"small", "raw", "generic"}
    assert CHK.bwd_family(CHK.CASES["bd_128_31x33"])[0] == "raw"          # 1023 pixels: the default entry point takes the three launches
    # A trailing split is empty when (ns - 1) * ceil(HW / ns) >= HW, i.e. HW = ns q + r with q + r <= ns - 1.  pick_split keeps
    # ns <= HW / 64 and ns <= 64, so q >= 64 >= ns: no (N, HW) has one.  Searched as well:
    for n in range(1, 130):
        for hw in range(1, 6000):
            ns = CHK.pick_split(n, hw)
            assert (ns - 1) * -(-hw // ns) < hw, (n, hw, ns)


def _judge_model(c, mode, plant=None):
    return CHK.judge(c, mode, CHK.model_record(c, mode, plant))


@pytest.mark.parametrize("c", GN_CASES + FUSED_CASES, ids=lambda c: c["name"])
def test_fp32_model_stays_inside_every_bound(c):
    worst = {}
    for mode in CHK.MODES:
        rows, reached, failures = _judge_model(c, mode)
        for key, fam, fig, verdict in rows:
            print(f"{c['name']:16s} {mode:5s} {key:22s} {fam:44s} {fig:>8s} {verdict}")
            if mode == "gauss":
                worst[fam] = max(worst.get(fam, 0.0), float(fig))
        assert not failures, "\n".join(failures)
        assert rows and reached
    assert all(v < 1 for v in worst.values()), worst


# planted error -> the cases it is planted into (the smallest that have the feature it needs)
TEETH = {
    "pixel_dropped": ["st_128_41x55", "sm_64_9x13", "sf_128_20x12"],
    "var_m_minus_1": ["st_128_41x55", "sm_64_1x1"],
    "shift_from_unscaled_mean": ["st_512_9x13", "sm_64_9x13"],
    "k3_omitted": ["bs_64_9x13", "b3_32_5x7"],
    "dres_last_row": ["bs_64_9x13", "b3f_32_9x13"],
    "last_split_lost": ["b3_128_41x55", "bs_128_8x8"],
    "a_truncated": ["st_32_5x7", "sm_64_9x13"],
}


@pytest.mark.parametrize("kind", sorted(TEETH))
@pytest.mark.parametrize("cls", [0, 2], ids=["easy_groups", "far_mean_groups"])
def test_teeth_planted_error_is_caught(kind, cls):
    caught = []
    for name in TEETH[kind]:
        for mode in CHK.MODES:
            _, _, failures = _judge_model(CHK.CASES[name], mode, (kind, cls))
            caught += [(name, mode, f) for f in failures]
            print(f"teeth {kind:26s} groups {cls} {name:14s} {mode:5s}: {len(failures)} checks fail" + (f" ({failures[0]})" if failures else ""))
    assert any(m == "gauss" for _, m, _ in caught), (kind, cls, "no gauss-mode bound is broken")
    assert any(m == "int" for _, m, _ in caught), (kind, cls, "no int-mode check is broken")


@pytest.mark.parametrize("name", ["w_ragged_res", "g_narrow"])
def test_teeth_out_of_map_pixel_counted(name):
    """one pixel outside the map of every ragged tile counted with the value bias: in int mode the table rows are no longer equal; in
    gauss mode one pixel in a 40 x 72 map is inside the accumulation bound of the column sums, as the issue says of max-relative checks --
    that is what the int mode is for"""
    c = CHK.CASES[name]
    _, _, failures = _judge_model(c, "int", ("edge_pixel_counted", None))
    print(f"teeth edge_pixel_counted {name}: {len(failures)} checks fail ({failures[:1]})")
    assert any("row sum" in f for f in failures)


def test_int_mode_activation_reference_has_ties():
    for c in CHK.STATS_CASES:
        if c["dt"] == "bf16" and CHK.stream_fixed(c["c"], "bf16"):
            ins = CHK.make_inputs(c, "int")
            r, _ = CHK.int_act_expected(ins["x"], ins["ss_syn"], "bf16")
            ties = CHK.bf16_ties(r)
            print(f"{c['name']}: share of exact bf16 ties among the int-mode gn_act values {ties:.3f}")
            assert ties >= CHK.INT_ACT_TIES
