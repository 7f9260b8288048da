"""Every split-K weight-gradient kernel at many split counts against an fp64 reference.

The split count of a weight gradient is no property of the shape: it follows the CU count, the CU budget (MasConvDesc.wgrad_cus), MAS_WGRAD_OVERSUB
and a different clamp in each kernel, so the rest of the suite only sees the few counts its shapes give on one part.  Here it is an
input: tests/helpers/wgrad_split_check.py runs every family (LDS-DMA 3x3 with and without the Upsample fold and the GroupNorm+SiLU
prologue, its sub-pixel form, stride 2, bf16 / fp32 1x1, thin 8 <-> 128, the general kernels in slab mode) in one child process per
setting -- the production sizing, MAS_WGRAD_OVERSUB=2, and MAS_WGRAD_SPLITS = 1 ... 10^4 -- and the numbers are checked here, on the CPU:

  * against fp64: ``torch.nn.grad.conv2d_weight`` in float64 on the same bf16-rounded operands (Upsample and padding applied first),
    element by element |dW - ref| <= TAU * S with S = conv2d_weight(|a|, |dy|) in fp64, and the relative L2 error <= EPS.  A slab
    rounded through bf16 is ~1e-3 of S, a tile row (16 pixels) left out >= 8e-4 of S on average at these K, a single pixel left out
    moves the relative L2 by ~1/sqrt(K) >= 7e-3: all far above the bounds;
  * across split counts: every child's dW / db agree with every other's within the same fp32 bounds (the prologue cases included:
    their operand rounding is the same at every split count);
  * the knob is inert: two children that ran the same kernel with the same split counts return bitwise equal dW / db.

tests/helpers/wgrad_walk.py restates each kernel's walk; with it the split counts the library reported are checked against the
restated setups, every launch's walk is checked to visit each tile once, and the union over the children must reach every regime
listed in REQUIRED -- a shape change that silently drops one fails here instead of passing vacuously.

Bounds, set from the first MI355X run with >= 10x headroom (measured worst case over all cases and children in brackets; fp32
accumulation of bf16 products is expected near 1e-6):
  TAU = 2^-18 = 3.8e-6 (2.5e-7 against fp64, 2.7e-7 across split counts: 14x), EPS = 1e-5 (8.2e-7 / 8.5e-7: 12x).
  The prologue case rounds act(x * s + b) to bf16 in the kernel (exp2 / rcp approximations) and on the CPU (exact sigmoid): a few
  operands round to the neighbouring bf16 value, which no split count changes.  TAU_ACT = 2^-13 = 1.2e-4 (5.1e-6: 24x),
  EPS_ACT = 1e-4 (7.6e-6: 13x) -- still 10x below a slab rounded through bf16; across split counts it meets TAU / EPS.
The whole file (10 children) takes ~30 s on an MI355X."""
import itertools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import wgrad_split_check as CHK  # noqa: E402
import wgrad_walk as W  # noqa: E402

CHILD = os.path.join(HERE, "helpers", "wgrad_split_check.py")
SETTINGS = [("unset", {}), ("oversub2", {"MAS_WGRAD_OVERSUB": "2"})] + \
    [(f"splits={k}", {"MAS_WGRAD_SPLITS": str(k)}) for k in (1, 2, 5, 7, 32, 33, 47, 10 ** 4)]
CHILD_TIMEOUT = 300
TAU, EPS = 2.0 ** -18, 1e-5
TAU_ACT, EPS_ACT = 2.0 ** -13, 1e-4

COMMON = {"nsplit1", "uneven", "multi_per_wg", "at_ceiling"}
REQUIRED = {
    "conv_wgrad_dma": COMMON | {"one_per_wg", "col_carry", "row_carry", "image_cross", "G4", "G16", "G16_tail"},
    "conv_wgrad_up2": COMMON | {"one_per_wg", "col_carry", "row_carry", "image_cross", "up2"},
    "wgrad_s2": COMMON | {"one_per_wg", "image_cross", "G4", "G16", "G16_tail"},
    "wgrad_thin": COMMON | {"at_ceiling", "image_cross", "G4"},
    "wgrad1x1": COMMON | {"at_ceiling", "G4"},
    "wgrad1x1_f32": COMMON | {"G4"},
    "conv_wgrad_tr": COMMON | {"one_per_wg", "image_cross", "G4"},
    "conv_wgrad": COMMON | {"one_per_wg", "image_cross", "G4"},
}
REGIMES = ["nsplit1", "one_per_wg", "at_ceiling", "multi_per_wg", "uneven", "col_carry", "row_carry", "image_cross", "G4", "G16",
           "G16_tail", "up2"]


def _silu(u):
    return u * torch.sigmoid(u)


def _reference(c):
    """fp64 dW, db and their magnitudes S = conv2d_weight(|a|, |dy|), Sb = sum |dy|, on the operands the kernel reads"""
    x, dy, ss = CHK.make_inputs(c)
    if ss is not None:                     # the prologue: act(x * s + b) in fp32, rounded to bf16 as the kernel does (zero padding after)
        a = _silu(x.float() * ss[..., 0][:, :, None, None] + ss[..., 1][:, :, None, None]).bfloat16().double()
    else:
        a = x.double()
    if c["up"]:
        a = a.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    ks, s = c["ks"], c["stride"]
    need_h, need_w = (c["ho"] - 1) * s + ks, (c["wo"] - 1) * s + ks
    a = F.pad(a, (c["pl"], need_w - a.shape[3] - c["pl"], c["pt"], need_h - a.shape[2] - c["pt"]))    # (negative: crop)
    d = dy.double()
    shape = (c["cout"], c["cin"], ks, ks)
    ref = torch.nn.grad.conv2d_weight(a, shape, d, stride=s)
    mag = torch.nn.grad.conv2d_weight(a.abs(), shape, d.abs(), stride=s)
    return ref, mag, d.sum((0, 2, 3)), d.abs().sum((0, 2, 3))


def _errs(dw, db, ref, mag, rb, mb):
    """(max |dW - ref| / S over dW and db, relative L2 of dW); NaN anywhere -> inf"""
    dw, db = dw.double(), db.double()
    if not (torch.isfinite(dw).all() and torch.isfinite(db).all()):
        return float("inf"), float("inf")
    r = torch.cat([((dw - ref).abs() / mag.clamp_min(1e-300)).flatten(), ((db - rb).abs() / mb.clamp_min(1e-300)).flatten()])
    r = torch.where(torch.cat([(dw - ref).flatten(), (db - rb).flatten()]) == 0, torch.zeros_like(r), r)
    return float(r.max()), float((dw - ref).norm() / ref.norm())


def _walk_geo(c, n):
    """the descriptor geometry of one batch slice of n images, as wgrad_walk's dicts"""
    if c["ks"] == 4 and c["stride"] == 2:
        return dict(n=n, h=c["ho"] + 1, w=c["wo"] + 1, cin=4 * c["cin"], cout=c["cout"], ks=2, stride=1, ho=c["ho"], wo=c["wo"])
    return dict(n=n, h=c["h"], w=c["w"], cin=c["cin"], cout=c["cout"], ks=c["ks"], stride=c["stride"], ho=c["ho"], wo=c["wo"])


def _run_children(tmp_path):
    env0 = {k: v for k, v in os.environ.items() if k not in ("MAS_WGRAD_SPLITS", "MAS_WGRAD_OVERSUB")}
    got = {}
    for label, extra in SETTINGS:          # one at a time; the first failure ends the test (no further child, no retry)
        out = str(tmp_path / f"wgrad_{len(got)}.pt")
        try:
            p = subprocess.run([sys.executable, CHILD, out], env={**env0, **extra}, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"child {label} timed out after {CHILD_TIMEOUT} s\n{e.stdout or ''}\n{e.stderr or ''}")
        if p.returncode != 0:
            pytest.fail(f"child {label} exited with {p.returncode}\n{p.stdout}\n{p.stderr[-6000:]}")
        got[label] = torch.load(out)
    return got


def test_every_wgrad_kernel_at_every_split_count_vs_fp64(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    got = _run_children(tmp_path)
    refs = {c["name"]: _reference(c) for c in CHK.CASES}
    reached = {k: {} for k in REQUIRED}
    worst = {"fp64": (0.0, 0.0), "act": (0.0, 0.0), "cross": (0.0, 0.0)}
    failures = []
    for label, res in got.items():
        cus, env = res["cus"], res["env"]
        budget = cus * 3 // 4 if res["wgrad_cus"] == -1 else (res["wgrad_cus"] or cus)      # (ops.wgrad_cus() of the child)
        oversub, override = int(env["MAS_WGRAD_OVERSUB"] or 1), max(0, int(env["MAS_WGRAD_SPLITS"] or 0))
        for c in CHK.CASES:
            r = res["results"][c["name"]]
            kern = r["kernel"]
            # the restated setups give the split counts the library reported, and every launch's walk covers each tile once
            for (n0, n1), k in zip(r["slices"], r["splits"]):
                g = _walk_geo(c, n1 - n0)
                want = W.splits(kern, g, cus, oversub, budget, override)
                assert k == want, (label, c["name"], (n0, n1), k, want)
                per_wg, seen = W.walk(kern, g, k)
                assert W.covers_once(kern, g, per_wg), (label, c["name"], k)
                for reg, on in seen.items():
                    if on:
                        reached[kern].setdefault(reg, set()).add(label)
            red = W.reduce_variant(kern, _walk_geo(c, 1)["ks"], sum(r["splits"]))
            regs = [red] if kern == "conv_wgrad_up2" else [red] + (["G16_tail"] if red == "G16" and sum(r["splits"]) % 16 else [])
            for reg in regs:
                reached[kern].setdefault(reg, set()).add(label)
            # against fp64
            e_max, e_l2 = _errs(r["dw"], r["db"], *refs[c["name"]])
            act = c["act"] != CHK.ACT_NONE
            key = "act" if act else "fp64"
            worst[key] = (max(worst[key][0], e_max), max(worst[key][1], e_l2))
            print(f"{label:12s} {c['name']:14s} {kern:15s} splits {str(r['splits']):16s} max/S {e_max:.2e}  relL2 {e_l2:.2e}")
            if not act and (e_max > TAU or e_l2 > EPS):
                failures.append(f"{label} {c['name']}: max |dW - ref| / S = {e_max:.3e} (TAU {TAU:.3e}), rel L2 {e_l2:.3e} (EPS {EPS:.0e})")
            if act and (e_max > TAU_ACT or e_l2 > EPS_ACT):
                failures.append(f"{label} {c['name']}: max |dW - ref| / S = {e_max:.3e} (TAU_ACT {TAU_ACT:.3e}), rel L2 {e_l2:.3e} (EPS_ACT {EPS_ACT:.0e})")
    # across split counts (fp32 bounds for every case) and the knob's inertness (bitwise where kernel and split counts match)
    labels = list(got)
    for c in CHK.CASES:
        ref, mag, rb, mb = refs[c["name"]]
        for la, lb in itertools.combinations(labels, 2):
            ra, rb_ = got[la]["results"][c["name"]], got[lb]["results"][c["name"]]
            if ra["kernel"] == rb_["kernel"] and ra["splits"] == rb_["splits"]:
                if not (torch.equal(ra["dw"], rb_["dw"]) and torch.equal(ra["db"], rb_["db"])):
                    failures.append(f"{c['name']}: {la} and {lb} ran {ra['kernel']} with splits {ra['splits']} but differ")
                continue
            e_max, e_l2 = _errs(ra["dw"], ra["db"], rb_["dw"].double(), mag, rb_["db"].double(), mb)
            e_l2 = float((ra["dw"].double() - rb_["dw"].double()).norm() / ref.norm())
            worst["cross"] = (max(worst["cross"][0], e_max), max(worst["cross"][1], e_l2))
            if e_max > TAU or e_l2 > EPS:
                failures.append(f"{c['name']}: {la} vs {lb}: max diff / S {e_max:.3e}, rel L2 {e_l2:.3e}")
    print(f"worst: fp64 max/S {worst['fp64'][0]:.2e} relL2 {worst['fp64'][1]:.2e} | prologue max/S {worst['act'][0]:.2e} relL2 "
          f"{worst['act'][1]:.2e} | across splits max/S {worst['cross'][0]:.2e} relL2 {worst['cross'][1]:.2e}")
    # the regime table: which settings reached which walk of which family
    print(f"{'family':15s} " + " ".join(f"{r:>12s}" for r in REGIMES))
    for kern, regs in reached.items():
        print(f"{kern:15s} " + " ".join(f"{len(regs.get(r, ())):>12d}" if regs.get(r) else f"{'-':>12s}" for r in REGIMES))
    for kern, want in REQUIRED.items():
        missing = want - set(reached[kern])
        if missing:
            failures.append(f"{kern}: no child reached {sorted(missing)}")
    assert not failures, "\n".join(failures[:40])
