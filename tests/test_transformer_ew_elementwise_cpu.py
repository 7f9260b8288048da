"""The CPU side of tests/test_gpu_transformer_ew_elementwise.py, checked without a GPU (tests/helpers/transformer_ew_check.py):

  * the fp64 references equal ``F.layer_norm`` and its autograd in float64, and ``0.5 x (1 + tanh(...))`` and its autograd, to 1e-12;
  * the launch geometry the helper restates agrees with the constants of csrc/transformer_ew.hip (NT, LN_KMAX, CS_NT, CS_MAX_SLICES, the
    per-CU caps, the 128 / 32 steps of the fold), and every case reaches the feature it was chosen for on 256, 304 and 64 CUs;
  * a numpy float32 model of each kernel's summation order stays inside EVERY bound and meets every exact-mode equality, for every case
    in both modes: the operands were chosen so that arithmetic of the documented kind passes, before any kernel is looked at;
  * teeth: each of fourteen planted errors drives the same ``judge`` outside a bound or breaks an equality."""
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import transformer_ew_check as CHK  # noqa: E402

CUS = 64          # the models run the cases of the smallest device: the same paths, the shortest tensors


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), (what, err)


def _pick(family, **kw):
    return [c for c in CHK.FAMILIES[family](CUS) if all(c.get(k) == v for k, v in kw.items())]


def test_gelu_reference_is_the_tanh_formula_in_float64():
    g = torch.Generator().manual_seed(5)
    x = (3 * torch.randn(4096, generator=g)).double().requires_grad_(True)
    dy = torch.randn(4096, generator=g).double()
    y = 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    y.backward(dy)
    _close(CHK.gelu_reference(x.detach())[0], y.detach(), "y")
    dx, a = CHK.gelu_reference(x.detach(), dy)
    _close(dx, x.grad, "dx")
    assert float((a - dy.abs()).min()) >= 0
    # the sweep's ends: finite limits, no NaN
    big = torch.tensor([3e38, -3e38, 2.0 ** 64, -2.0 ** 64, 1e-40, 0.0], dtype=torch.float64)
    dxb, _ = CHK.gelu_reference(big, torch.ones(6, dtype=torch.float64))
    assert torch.equal(dxb, torch.tensor([1.0, 0.0, 1.0, 0.0, 0.5, 0.5], dtype=torch.float64))
    assert CHK.sweep_x().numel() == 65280 and bool(torch.isfinite(CHK.sweep_x().float()).all())


@pytest.mark.parametrize("ti,to,d,rows", [("bf16", "bf16", 520, 5), ("f32", "f32", 1024, 5), ("f32", "bf16", 200, 3), ("bf16", "f32", 4, 1)])
def test_layernorm_references_are_layer_norm_and_its_autograd_in_float64(ti, to, d, rows):
    (c,) = _pick("ln_bwd", ti=ti, to=to, d=d, rows=rows)
    ins = CHK.make_inputs(c, "gauss")
    x = ins["x"].double().requires_grad_(True)
    ga, be = ins["gamma"].double().requires_grad_(True), ins["beta"].double().requires_grad_(True)
    res = torch.randn(rows, d, dtype=torch.float64)
    y = F.layer_norm(x, (d,), ga, be, eps=CHK.EPS)
    y.backward(ins["dy"].double())
    ref = CHK.ln_reference(x.detach(), ga.detach(), be.detach(), res, CHK.EPS)
    _close(ref["y"], y.detach() + res, "y")
    _close(ref["mean"], x.detach().mean(-1), "mean")
    _close(ref["rstd"], 1 / torch.sqrt(x.detach().var(-1, unbiased=False) + CHK.EPS), "rstd")
    exact_mr = torch.stack([ref["mean"], ref["rstd"]], -1)                 # the exact table instead of the fp32 one the kernel is handed
    bw = CHK.ln_bwd_reference(x.detach(), ins["dy"].double(), ga.detach(), exact_mr, ins["add"].double())[1]
    _close(bw["dx"], x.grad + ins["add"].double(), "dx")
    _close(bw["dgamma"], ga.grad, "dgamma")
    _close(bw["dbeta"], be.grad, "dbeta")
    assert all(float(bw[k].min()) > 0 for k in ("e", "bdgamma", "bdbeta")) and float(ref["e"].min()) > 0


def test_restated_geometry():
    src = open(os.path.join(os.path.dirname(HERE), "make-a-scene_amd", "csrc", "transformer_ew.hip")).read()
    for pattern in (r"constexpr int NT = 256;", r"constexpr int LN_KMAX = 4;", r"constexpr int CS_NT = 64, CS_MAX_SLICES = 128;",
                    r"const long long cap = 16LL \* mas_num_cus\(\);", r'mas_env_int\("MAS_LN_FWD_BLOCKS_PER_CU", 8\)',
                    r'mas_env_int\("MAS_LN_PAIR_FWD_BLOCKS_PER_CU", 8\)', r"int ln_blocks\(int rows, int per_cu = 4\)",
                    r"ln_blocks\(rows, dx_colsum \? 3 : 4\)", r"mas_cdiv\(4 \* mas_num_cus\(\), col_blocks > 0 \? col_blocks : 1\)",
                    r"nsl > mas_cdiv\(rows, 8\)", r"long long want = 4LL \* mas_num_cus\(\);", r"for \(; k \+ 96 < nblk; k \+= 128\)",
                    r"for \(; k < nblk; k \+= 32\)", r"const int col = blockIdx\.x \* 32 \+ cq \* 4;", r"r \+ 7 \* nsl < rows; r \+= 8 \* nsl"):
        assert re.search(pattern, src), pattern
    assert (CHK.NT, CHK.LN_KMAX, CHK.CS_NT, CHK.CS_MAX_SLICES) == (256, 4, 64, 128)
    assert (CHK.GELU_PER_CU, CHK.LN_FWD_PER_CU, CHK.LN_BWD_PER_CU, CHK.LN_BWD_CS_PER_CU, CHK.CS_PER_CU, CHK.GELU_CS_PER_CU) == (16, 8, 4, 3, 4, 4)
    assert (CHK.FOLD_UNROLL, CHK.FOLD_STEP) == (128, 32)
    # what the issue says of the launch code
    assert CHK.GELU_PER_CU * 256 * CHK.NT * 8 == 8388608 and 4 * CHK.LN_FWD_PER_CU * 256 == 8192
    assert CHK.fold_features(201, 64) == {"fold_unrolled", "fold_remainder"} and CHK.fold_features(128, 520) == {"fold_unrolled", "fold_ragged_cols"}
    assert CHK.fold_features(96, 32) == set()
    assert CHK.gelu_cs_grid(257 * 8, 8, 256) == (771, 257) and CHK.gelu_cs_grid(4096, 8, 256) == (1024, 2) and CHK.gelu_cs_grid(257 * 4, 4, 64) == (257, 257)
    assert CHK.colsum_slices(5, 1024, 8, 256) == 1 and CHK.colsum_slices(1027, 520, 8, 256) == 128
    # every case reaches its feature (asserted as the cases are built) and the union reaches REQUIRED, whatever the device
    for cus in CHK.DEVICE_CUS:
        for part, make in CHK.FAMILIES.items():
            reached = set().union(*(CHK.features(c, cus) for c in make(cus)))
            for launch, want in CHK.REQUIRED[part].items():
                assert {(launch, f) for f in want} <= reached, (cus, part, launch, {f for f in want if (launch, f) not in reached})
        big = [c for c in CHK.ln_bwd_cases(cus) if c["rows"] == 4 * 4 * cus + 5]
        assert big and all(CHK.ln_blocks(c["rows"], 4, cus) != CHK.ln_blocks(c["rows"], 3, cus) for c in big)


@pytest.mark.parametrize("part", sorted(CHK.FAMILIES))
def test_fp32_model_stays_inside_every_bound(part):
    failures, worst, _ = CHK.judge_family(part, CUS, lambda c, mode, ins: CHK.model_record(c, mode, CUS))
    for fam in sorted(worst):
        print(f"{fam:52s} {worst[fam]:.3f}")
    assert not failures, "\n".join(failures[:40])
    assert worst and all(v < 1 for v in worst.values()), worst


def test_exact_mode_references_have_ties():
    """on the references alone: the bf16 outputs of the exact mode hold at least TIES exact round-to-even ties"""
    for c in _pick("ln_fwd", to="bf16", rows=5) + _pick("pair", to="bf16", rows=5):
        ins = CHK.make_inputs(c, "exact")
        if c["kind"] == "pair":
            amp2 = 2.0 ** (torch.arange(5) % 4).double()
            xn = CHK.ln_reference(ins["x"].double(), ins["gamma"].double(), ins["beta"].double(), ins["res"].double(), 0.0)["y"]
            assert torch.equal(xn.abs(), amp2[:, None].expand_as(xn)), c["name"]
            y = CHK.ln_reference(xn, ins["gamma2"].double(), ins["beta2"].double(), None, 0.0)["y"]
        else:
            y = CHK.ln_reference(ins["x"].double(), ins["gamma"].double(), ins["beta"].double(), ins["res"].double() if c["res"] else None, 0.0)["y"]
        ties = CHK.bf16_ties(y)
        print(f"{c['name']}: share of exact bf16 ties {ties:.3f} of {y.numel()}")
        assert ties >= CHK.TIES, (c["name"], ties)


# planted error -> the cases it is planted into (the smallest that have the feature it needs)
TEETH = {
    "var_d_minus_1": lambda: _pick("ln_fwd", ti="f32", to="f32", d=1024, rows=5, res=0) + _pick("pair", d=1024, rows=5),
    "one_pass": lambda: _pick("ln_fwd", ti="f32", to="bf16", d=1024, rows=5, res=0) + _pick("ln_fwd", ti="f32", to="f32", d=256, rows=5, res=1),
    # (fp32 inputs: the squares of bf16 values are exact in fp32 and so are their sums at these D)
    "eps_swapped": lambda: _pick("pair", d=256, rows=5),
    "lane_last_vec": lambda: _pick("ln_fwd", ti="bf16", to="bf16", d=520, rows=5, res=1) + _pick("ln_fwd", ti="f32", to="f32", d=260, rows=3, res=0),
    "res_after_rounding": lambda: _pick("ln_fwd", ti="bf16", to="bf16", d=200, rows=5, res=1),
    "truncating_store": lambda: _pick("ln_fwd", ti="f32", to="bf16", d=256, rows=3, res=0) + _pick("pair", to="bf16", d=260, rows=5),
    "xhat_m2_dropped": lambda: _pick("ln_bwd", ti="bf16", to="bf16", d=512, rows=5),
    "dgamma_from_g": lambda: _pick("ln_bwd", ti="f32", to="bf16", d=256, rows=5),
    "block_partial_lost": lambda: _pick("ln_bwd", ti="bf16", to="bf16", d=16, rows=801),
    "dx_add_last_k": lambda: _pick("ln_bwd", ti="bf16", to="bf16", d=2048, rows=3) + _pick("ln_bwd", ti="f32", to="f32", d=788, rows=3),
    "colsum_unrounded": lambda: _pick("ln_bwd", ti="bf16", to="bf16", d=520, rows=801),
    "gelu_no_3": lambda: _pick("gelu", dir="bwd", dt="bf16", n=6151) + _pick("gelu", dir="bwd", dt="f32", tag="sweep"),
    "gelu_tail_skipped": lambda: _pick("gelu", dir="fwd", dt="bf16", n=6151) + _pick("gelu", dir="bwd", dt="f32", n=3),
    "slice_last_row": lambda: _pick("colsum", dt="bf16", cols=520, rows=1027) + _pick("colsum", dt="f32", cols=4, rows=9),
}


@pytest.mark.parametrize("kind", sorted(TEETH))
def test_teeth_planted_error_is_caught(kind):
    cases = TEETH[kind]()
    assert cases, kind
    for c in cases:
        caught = []
        for mode in c["modes"]:
            _, _, failures = CHK.judge(c, mode, CHK.model_record(c, mode, CUS, kind), CUS)
            caught += failures
            print(f"teeth {kind:20s} {c['name']:40s} {mode:5s}: {len(failures)} checks fail" + (f" ({failures[0]})" if failures else ""))
        assert caught, (kind, c["name"], "no bound is broken and no equality fails")
