#!/usr/bin/env python3
"""GPU child of tests/test_gpu_gn_elementwise.py, and the CPU side that test and tests/test_gn_elementwise_cpu.py import.

    gn_elementwise_check.py SETTING OUT.pt

runs every case of SETTINGS[SETTING] in both operand modes and writes every output of every launch together with ``ops.last_kernel()``
right after it.  Nothing numeric is judged there.  The CPU side: seeded operands (``make_inputs``), fp64 references with their magnitude
sums, the bounds below, the kernels' launch geometry restated (``pick_split`` ... ``small_units``) and an fp32 model of each kernel's
arithmetic (``model_*``: the same summation tree in numpy float32, fp64 where the kernel uses fp64).

Notation: U = 2^-24 (one fp32 rounding, relative), G = 32 groups, m = (C / G) * H * W values per group, eps = 1e-6.

1. Statistics.  A producer forms per channel s = sum x and q = sum x^2 in fp32 and hands them to an fp64 combination (groups, mean,
   variance).  With L the longest chain of fp32 additions one value passes through, |ds| <= L U sum|x| and |dq| <= Lq U sum x^2:
     gn_stats_partial, fixed branch   L = ceil(rows_per / rstep) (a thread's loads) + rstep (the fold over the row groups)
     gn_stats_partial, atomic branch  L = rows_per: the terms one LDS cell receives, valid in any order
     gn_small_fwd_kernel              L = UNITS + TP
     conv3x3_wide / conv_up2 epilogue L = 32 (a lane's pixels) + 1 (the other half-wave) + 8 (the waves, in stats_flush) = 41
   Lq = L + 1: the square is rounded on its own where the compiler does not contract it into an fma (bf16 squares are exact).
   The fp64 part adds nothing that matters, the stores of mean and rstd one rounding each (the rsqrt in fp64, then one conversion):
     |dmean| <= L U E|x| + U |mu|,  |dv| <= Lq U E[x^2] + 2 |mu| L U E|x|,  |drstd| / rstd <= 1/2 |dv| / (v + eps) + 2 U
   For the fused table the summed values are the convolution's unrounded fp32 outputs y~, |y~ - r| <= TAU S (TAU = 2^-18, the conv
   suite's bound, S from ``reference_fwd``): sum|x| becomes sum(|r| + TAU S) and every term adds its own TAU S, resp.
   (2 |r| + TAU S) TAU S to the square.
2. scale_shift against the kernel's own mean_rstd: sc = fl(rstd * gamma): |sc - rstd gamma| <= U |rstd gamma|;
   sh = fl(beta - fl(mean * sc)): |sh - (beta - mean sc)| <= 2 U (|beta| + |mean sc|).
3. a against act(x sc + sh) in fp64 from the kernel's own scale_shift.  e = 2 U (|x sc| + |sh|) is the fp32 evaluation of the affine
   part (product and sum, or one fma).  SiLU (``silu2_f``: t = u * -log2(e); E = v_exp_f32(t); s = v_rcp_f32(1 + E); a = u * s) adds,
   with 1 ulp = 2 U relative for each of the two transcendental instructions (the accuracy AMD's public CDNA ISA manual gives for
   V_EXP_F32 and V_RCP_F32, and the comment at ``silu_f`` in mas_common.h): t carries 2 U |t| (the rounded constant and the product)
   = an error 2 U |u| ln2 log2(e) = 2 U |u| in the exponent, so E is relative (2 U + 2 U |u|) off, 1 + E one more rounding, the
   reciprocal 2 U:  rho_s = (1 - s) 2 U (1 + |u|) + U + 2 U on s, and the last product one U:
     e_silu = |silu'(u)| e + |silu(u)| (rho_s + U),   |silu'| <= 1.1
   bf16 tensors: |a - r| <= 2^-8 (|r| + e) + e; fp32 tensors: e alone.
4. Backward against fp64 from the same x, da, dres, gamma, mean_rstd, scale_shift the kernel is handed: du = da silu'(x sc + sh) (or
   da), xhat = (x - mean) rstd, S1 = sum du, S2 = sum du xhat per (n, c), A = sum_g gamma S1, B = sum_g gamma S2,
   dx = rstd gamma du - rstd / m (A + xhat B) + dres = c1 du + k2 x + k3 + dres.
     evaluation   2^-22 (|c1 du| + |k2 x| + |k3|): three rounded coefficients, two products, two sums.  ADDED to the issue's list:
                  U (|dres| + |dx|) for the residual's own addition, and |c1| ddu for the fp32 evaluation of silu' (below);
     accumulation dS1 <= L U sum|du| + sum ddu; generic and small-map kernels dS2 <= (L + 1) U sum|du xhat| + sum(ddu |xhat| + |du| dxhat);
                  the packed three-launch kernels keep q = sum du x raw and form S2 = rstd (q - mean S1) in fp64:
                  dS2 <= rstd ((L + 1) U sum|du x| + sum ddu |x| + |mean| dS1)   (the |mean| dS1 part is ADDED: the issue's list has
                  the first term only, and with a far mean the two are the same size);
                  dA = sum_g |gamma| dS1, dB = sum_g |gamma| dS2, and dx moves by rstd / m (dA + |xhat| dB);
     ADDED        dxhat, the fp32 evaluation of xhat, which the issue's list leaves out: generic kernels fl(fl(x - mean) rstd):
                  2 U |xhat|; the small-map kernel fl(x rstd + fl(-mean rstd)): U (|x rstd| + |mean rstd| + |xhat|) -- with a far mean
                  the two addends are 40 times the result;
                  ddu for SiLU: silu'(u) = s (1 + u (1 - s)) evaluated in fp32 from u with error e (above): with ds = s rho_s,
                  d(1 - s) = ds + U, dp = |u| d(1 - s) + 2 U (|u (1 - s)| + 1) for p = u (1 - s) + 1,
                  ddu = |da| (0.5 e + s dp + |p| ds + U |silu'|) + U |du|   (|silu''| <= 0.5).
   dx: |dx - r| <= 2^-8 (|r| + E) + E with E = evaluation + propagated accumulation (fp32 tensors: E alone).
   dgamma, dbeta per channel: sum over the images of (dS + U |S|) (the per-image fp32 value) + U |result| (the final store).
*int* mode: integers with a per-group integer offset; every fp32 sum a kernel forms stays below 2^24 (asserted in ``make_inputs``) and
is exact in any order.  mean must equal float(mu) bitwise, rstd within one fp32 ulp; with a synthetic table (integer mean, power-of-two
rstd and gamma) dbeta / dgamma must equal the fp64 result bitwise, ``gn_act`` on a power-of-two table must equal the exactly rounded
value bitwise (``bf16_ties``: the share of exact bf16 ties among them, at least INT_ACT_TIES), and dx takes the gauss bound with L = 0 and dxhat = 0 (dx divides by m, so it is no exact fp32 value and has no ties to count:
the tie share is defined, and asserted, for the activation alone)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import conv_elementwise_check as CONV  # noqa: E402
from conv_elementwise_check import WIDE, UP2F, WIDE_ENV, MODES, HALF_ULP  # noqa: E402

G, EPS = 32, 1e-6
U = 2.0 ** -24
TAU = 2.0 ** -18
NT, MAX_SPLIT = 256, 64
ACT_AFFINE, ACT_SILU = 1, 2
PAIRS = ((0.3, 1.5), (8.0, 1.0), (-20.0, 0.5))        # (mu, sigma) rotated over (n, g): easy, 8 sigma, 40 sigma
INT_OFFSETS = (0, 100, -100, 37, -63)
L_FUSED = 41


# ------------------------------------------------------------------------------------------------------- launch geometry, restated
def pick_split(n, hw, max_split=MAX_SPLIT):
    s = min(-(-1024 // n), max_split, max(hw // 64, 1))
    return max(s, 1)


def epu(dt):
    return 8 if dt == "bf16" else 4


def stream_fixed(c, dt):
    """does gn_stats_partial / gn_bwd_partial keep a thread on one channel unit (the fixed-order branch)?"""
    return NT % (c // epu(dt)) == 0


def rstep(c, dt):
    return NT // (c // epu(dt))


def small_threads(hw):
    return 256 if hw <= 256 else 512


def small_units(hw):
    t = small_threads(hw)
    return (hw * 8 + t - 1) // t


def small_fwd_instance(hw):
    u = small_units(hw)
    return 1 if u <= 1 else 2 if u <= 2 else 4 if u <= 4 else 8 if u <= 8 else 16


def small_bwd_instance(hw):
    u = small_units(hw)
    return 1 if u <= 1 else 2 if u <= 2 else 4 if u <= 4 else 8


def small_ok(dt, hw, c):
    return dt == "bf16" and 1 <= hw <= 1024 and c % 64 == 0 and c % G == 0 and 64 % (c // G) == 0


def stream_chain(n, hw, c, dt):
    """L of the streaming reductions (statistics and backward partial sums share the walk)"""
    rows_per = -(-hw // pick_split(n, hw))
    if not stream_fixed(c, dt):
        return rows_per
    rs = rstep(c, dt)
    return -(-rows_per // rs) + rs


def small_chain(hw, bwd=False):
    return (small_bwd_instance(hw) if bwd else small_fwd_instance(hw)) + small_threads(hw) // 8


# ----------------------------------------------------------------------------------------------------------------------------- cases
def _gn(name, kind, n, c, h, w, dt="bf16", path=None):
    """kind: "stats" (gn_stats [+ gn_act where it takes the width]), "small" (gn_stats_act), "bwd" (gn_bwd, path None / "three")"""
    return dict(name=name, kind=kind, n=n, c=c, h=h, w=w, hw=h * w, dt=dt, path=path)


# (No (N, HW) gives gn_stats_partial an EMPTY trailing split: pick_split keeps at least 64 rows per split and at most 64 splits, see
# test_restated_geometry in tests/test_gn_elementwise_cpu.py, which also searches.  The short trailing split of st_128_41x55 is the edge.)
STATS_CASES = [
    _gn("st_32_5x7", "stats", 2, 32, 5, 7),             # rstep = 64 > HW: whole row groups idle
    _gn("st_128_41x55", "stats", 3, 128, 41, 55),       # 35 splits of 65 rows, the last one short
    _gn("st_512_9x13", "stats", 2, 512, 9, 13),
    _gn("st_96_9x13", "stats", 2, 96, 9, 13),           # atomic branch (gn_act rejects the width: statistics only)
    _gn("st_320_20x12", "stats", 2, 320, 20, 12),
    _gn("sf_32_9x13", "stats", 2, 32, 9, 13, dt="f32"),
    _gn("sf_128_20x12", "stats", 2, 128, 20, 12, dt="f32"),
    _gn("sf_256_9x13", "stats", 2, 256, 9, 13, dt="f32"),
    _gn("sf_96_9x13", "stats", 2, 96, 9, 13, dt="f32"),  # atomic branch
]
SMALL_SHAPES = [(3, 64, 1, 1), (2, 128, 8, 8), (3, 64, 9, 13), (2, 256, 12, 20), (2, 128, 20, 20), (2, 64, 31, 33), (2, 512, 32, 32)]
SMALL_CASES = [_gn("sm_%d_%dx%d" % (c, h, w), "small", n, c, h, w) for n, c, h, w in SMALL_SHAPES]
BWD_CASES = (
    [_gn("bs_%d_%dx%d" % (c, h, w), "bwd", n, c, h, w) for n, c, h, w in SMALL_SHAPES if h * w <= 512] +
    [_gn("b3_%d_%dx%d" % (c, h, w), "bwd", n, c, h, w, path="three") for n, c, h, w in ((2, 32, 5, 7), (3, 128, 41, 55), (2, 512, 9, 13))] +
    [_gn("b3f_%d_%dx%d" % (c, h, w), "bwd", n, c, h, w, dt="f32", path="three") for n, c, h, w in ((2, 32, 9, 13), (2, 128, 20, 12))] +
    [_gn("b3_128_31x33", "bwd", 2, 128, 31, 33, path="three"), _gn("bd_128_31x33", "bwd", 2, 128, 31, 33)]     # 1023 pixels: both entry points take the three launches
)
ACT_RES = [(a, r) for a in (ACT_AFFINE, ACT_SILU) for r in (False, True)]


def _fused(name, feats, base=None, **kw):
    """a convolution case of the conv helper (same name: the kernel it takes is asserted there too) with *int* ranges narrowed until
    sum r^2 per (tile, channel) stays below 2^24 (asserted on the reference)"""
    c = dict(CONV.CASES[base or name]) if (base or name) in CONV.CASES else CONV._case(name, **kw)
    c.update(name=name, kind="fused", xr=1, wr=0, feats=tuple(feats))
    return c


FUSED_WIDE = [
    _fused("w_one_tile", ["one_tile"]),
    _fused("w_ragged_res", ["ragged", "res"]),
    _fused("w_cout256", ["ragged", "cout_tiles2", "res"]),
    _fused("g_narrow", ["ragged", "narrow_last_column"], n=2, cin=128, cout=128, h=19, w=52, fwd=WIDE),   # last tile column: 20 of 32 pixels
    _fused("u_128_256", ["ragged", "cout_tiles2"]),
]
# 136 and 33 images of 16 x 32: the smallest counts whose tiles (2 resp. 8 per image) exceed one work-group per CU on 256 CUs
FUSED_MULTI = [_fused("m_wide", ["tiles_gt_grid"]), _fused("m_up2", ["tiles_gt_grid"])]

SETTINGS = [
    ("default", {}, STATS_CASES + SMALL_CASES + BWD_CASES),
    ("wide", WIDE_ENV, FUSED_WIDE),
    ("multi", dict(WIDE_ENV, MAS_CONV_WGS_PER_CU="1"), FUSED_MULTI),
]
CASES = {c["name"]: c for _, _, cs in SETTINGS for c in cs}


# -------------------------------------------------------------------------------------------------------------------------- operands
def _tdt(s):
    return torch.bfloat16 if s == "bf16" else torch.float32


def group_of(c, channels):
    return torch.arange(channels) // (channels // G)


def _per_group(vals, n, c):
    """[n, c] tensor: vals[(image + group) % len] for every channel"""
    idx = (torch.arange(n)[:, None] + group_of(c, c)[None, :]) % len(vals)
    return torch.tensor(vals, dtype=torch.float64)[idx]


def synthetic_table(c, g):
    """*int* mode backward: integer mean, power-of-two rstd and gamma, beta a multiple of 1/4, scale_shift consistent with them"""
    n, ch = c["n"], c["c"]
    mean = _per_group(INT_OFFSETS, n, ch)[:, ::ch // G]                                            # [n, G]
    rstd = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n, G), generator=g)]
    gamma = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (ch,), generator=g)]
    beta = torch.randint(-4, 5, (ch,), generator=g).float() * 0.25
    mr = torch.stack([mean, rstd], -1).float()
    sc = rstd[:, group_of(c, ch)] * gamma.double()[None]
    sh = beta.double()[None] - mean[:, group_of(c, ch)] * sc
    return gamma, beta, mr.contiguous(), torch.stack([sc, sh], -1).float().contiguous()


def table_from(x, gamma, beta):
    """gauss mode backward: the table a forward would have left, from the exact statistics: fp32 mean_rstd, and scale_shift formed
    from those fp32 values the way the kernels form it"""
    n, ch = x.shape[:2]
    xg = x.double().reshape(n, G, -1)
    mean = xg.mean(-1)
    rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + EPS)
    mr = torch.stack([mean, rstd], -1).float()
    gi = torch.arange(ch) // (ch // G)
    sc = mr[..., 1][:, gi] * gamma[None]
    sh = beta[None] - mr[..., 0][:, gi] * sc
    return mr.contiguous(), torch.stack([sc, sh], -1).contiguous()


def block_sums_exact(c, t):
    """*int* mode: the largest sum of |t| any fp32 accumulator can hold = over a channel's pixels of one block (one split of the
    streaming kernels, the whole map of the small-map ones) must stay below 2^24"""
    n, ch = t.shape[:2]
    v = t.double().abs().reshape(n, ch, -1)
    small = c["kind"] == "small" or (c["kind"] == "bwd" and c["path"] is None and c["hw"] <= 512 and small_ok(c["dt"], c["hw"], ch))
    rows_per = c["hw"] if small else -(-c["hw"] // pick_split(n, c["hw"]))
    pad = -c["hw"] % rows_per
    return float(F.pad(v, (0, pad)).reshape(n, ch, -1, rows_per).sum(-1).max()) < 2 ** 24


def make_inputs(c, mode):
    """seeded CPU operands of a GroupNorm case: x, gamma, beta; backward cases: da, dres, mr, ss (the table handed to the kernel);
    *int* "stats" cases: ss_syn, a power-of-two table for gn_act.  Fused cases: the conv helper's operands + gamma, beta"""
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])) * 2 + (mode == "int") + 77)
    if c["kind"] == "fused":
        ins = CONV.make_inputs(c, mode)
        ins["gamma"], ins["beta"] = 1.0 + 0.1 * torch.randn(c["cout"], generator=g), 0.1 * torch.randn(c["cout"], generator=g)
        return ins
    n, ch, h, w, dt = c["n"], c["c"], c["h"], c["w"], _tdt(c["dt"])
    ins = {}
    if mode == "gauss":
        mu, sg = _per_group([p[0] for p in PAIRS], n, ch), _per_group([p[1] for p in PAIRS], n, ch)
        x = (torch.randn(n, ch, h, w, generator=g).double() * sg[:, :, None, None] + mu[:, :, None, None]).float().to(dt)
        gamma, beta = 1.0 + 0.1 * torch.randn(ch, generator=g), 0.1 * torch.randn(ch, generator=g)
        if c["kind"] == "bwd":
            ins["da"] = torch.randn(n, ch, h, w, generator=g).to(dt)
            ins["dres"] = torch.randn(n, ch, h, w, generator=g).to(dt)
            ins["mr"], ins["ss"] = table_from(x, gamma, beta)
    else:
        off = _per_group(INT_OFFSETS, n, ch)
        x = (torch.randint(-4, 5, (n, ch, h, w), generator=g).double() + off[:, :, None, None]).float().to(dt)
        assert torch.equal(x.double(), x.double().round()) and block_sums_exact(c, x.double() ** 2), c["name"]
        gamma, beta = 1.0 + 0.1 * torch.randn(ch, generator=g), 0.1 * torch.randn(ch, generator=g)
        if c["kind"] == "bwd":
            gamma, beta, ins["mr"], ins["ss"] = synthetic_table(c, g)
            ins["da"] = torch.randint(-4, 5, (n, ch, h, w), generator=g).to(dt)
            ins["dres"] = torch.randint(-16, 17, (n, ch, h, w), generator=g).to(dt)
            rs = ins["mr"][..., 1].double()[:, group_of(c, ch)][:, :, None, None]
            mu = ins["mr"][..., 0].double()[:, group_of(c, ch)][:, :, None, None]
            da = ins["da"].double()
            for t in (da, da * x.double(), da * (x.double() - mu) * rs):          # sum da, raw sum da x, sum da xhat
                assert block_sums_exact(c, t), c["name"]
        elif c["kind"] == "stats":
            sc = torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.randint(0, 4, (n, ch), generator=g)]
            sh = torch.randint(-8, 9, (n, ch), generator=g).float() * 0.25
            ins["ss_syn"] = torch.stack([sc, sh], -1).contiguous()
    ins.update(x=x, gamma=gamma, beta=beta)
    return ins


# ------------------------------------------------------------------------------------------------------------ references and bounds
def _ratio(got, ref, bound):
    """(worst |got - ref| / bound over EVERY element, number outside); a non-finite value is outside"""
    got, err = got.double(), (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max()), int((ratio > 1).sum())


def stats_reference(v, l_s, extra=None):
    """v [n, C, ...] fp64, the values a producer summed -> dict of per-(n, g) fp64 mean, var, rstd and the bounds of section 1.
    extra: per-element |error| of the summed values themselves (the fused table: TAU S)"""
    n, ch = v.shape[:2]
    vg = v.reshape(n, G, -1)
    m = vg.shape[-1]
    mean = vg.mean(-1)
    var = ((vg - mean[..., None]) ** 2).mean(-1)
    a1 = vg.abs() if extra is None else vg.abs() + extra.reshape(n, G, -1)
    ds = l_s * U * a1.sum(-1)
    dq = (l_s + 1) * U * (a1 ** 2).sum(-1)
    if extra is not None:
        eg = extra.reshape(n, G, -1)
        ds, dq = ds + eg.sum(-1), dq + ((2 * vg.abs() + eg) * eg).sum(-1)
    dmean = ds / m + U * mean.abs()
    dv = dq / m + 2 * mean.abs() * ds / m
    rstd = 1.0 / torch.sqrt(var + EPS)
    return dict(mean=mean, var=var, rstd=rstd, m=m, bmean=dmean, brstd=rstd * (0.5 * dv / (var + EPS) + 2 * U))


def ulp32(t):
    """one fp32 unit in the last place at |t| (t fp64 holding fp32 values)"""
    f = t.float().abs()
    return (torch.nextafter(f, torch.full_like(f, float("inf"))) - f).double()


def judge_stats(mr, ref, mode):
    """mean_rstd [n, G, 2] of a kernel against ``stats_reference`` -> {"mean": (figure, number outside), "rstd": ...}; *int* mode: mean
    bitwise float(mu), rstd within one fp32 ulp (figure 0 = equal)"""
    mean, rstd = mr[..., 0].double(), mr[..., 1].double()
    if mode == "int":
        want_m, want_r = ref["mean"].float().double(), ref["rstd"].float().double()
        bad_m = int((mean != want_m).sum()) + int((~torch.isfinite(mean)).sum())
        off = (rstd - want_r).abs() / ulp32(want_r)
        off = torch.where(torch.isfinite(off), off, torch.full_like(off, float("inf")))
        return {"mean": (float(bad_m > 0), bad_m), "rstd": (float(off.max()), int((off > 1).sum()))}
    return {"mean": _ratio(mean, ref["mean"], ref["bmean"]), "rstd": _ratio(rstd, ref["rstd"], ref["brstd"])}


def judge_table(ss, mr, gamma, beta):
    """section 2: scale_shift [n, C, 2] against the SAME kernel's mean_rstd"""
    ch = ss.shape[1]
    gi = torch.arange(ch) // (ch // G)
    mean, rstd = mr[..., 0].double()[:, gi], mr[..., 1].double()[:, gi]
    sc, sh = ss[..., 0].double(), ss[..., 1].double()
    want_sc = rstd * gamma.double()[None]
    want_sh = beta.double()[None] - mean * sc
    return {"sc": _ratio(sc, want_sc, U * want_sc.abs() * (1 + 2.0 ** -20)),
            "sh": _ratio(sh, want_sh, 2 * U * (beta.double().abs()[None] + (mean * sc).abs()))}


def _sig(u):
    return torch.sigmoid(u)


def silu_terms(u, e):
    """(silu(u), its fp32 evaluation error e_silu, silu'(u), the relative error ddsilu of silu' evaluated in fp32) -- section 3 / 4"""
    s = _sig(u)
    rho = (1 - s) * 2 * U * (1 + u.abs()) + 3 * U
    d1 = s * (1 + u * (1 - s))
    e_silu = 1.1 * e + (u * s).abs() * (rho + U)
    ds = s * rho
    dw = ds + U
    p = u * (1 - s) + 1
    dp = u.abs() * dw + 2 * U * ((u * (1 - s)).abs() + 1)
    dd = 0.5 * e + s * dp + p.abs() * ds + U * d1.abs()
    return u * s, e_silu, d1, dd


def act_reference(x, ss, act):
    """(r, bound) of a = act(x sc + sh), fp64, from the table handed in (section 3)"""
    x = x.double()
    sc, sh = ss[..., 0].double()[:, :, None, None], ss[..., 1].double()[:, :, None, None]
    u = x * sc + sh
    e = 2 * U * ((x * sc).abs() + sh.abs())
    if act == ACT_SILU:
        u, e, _, _ = silu_terms(u, e)
    return u, e


def act_bound(r, e, dt):
    return HALF_ULP * (r.abs() + e) + e if dt == "bf16" else e


def int_act_expected(x, ss_syn, dt):
    """*int* mode gn_act on a power-of-two table: x sc + sh is exact in fp32, the output that value rounded once"""
    r, _ = act_reference(x, ss_syn, ACT_AFFINE)
    assert torch.equal(r.float().double(), r)
    return r, r.float().to(_tdt(dt))


def bf16_ties(r):
    """share of the elements of r (fp64, exact in fp32) that lie exactly half way between two bf16 values: only round-to-nearest-EVEN
    gets them all right"""
    f = r.float()
    bits = f.view(torch.int32) & 0xFFFF
    return float((bits == 0x8000).double().mean())


def bwd_family(c):
    """(family, L): which kernels a backward case runs, from the restated dispatch"""
    if c["path"] is None and c["hw"] <= 512 and small_ok(c["dt"], c["hw"], c["c"]):
        return "small", small_chain(c["hw"], bwd=True)
    return ("raw" if c["dt"] == "bf16" else "generic"), stream_chain(c["n"], c["hw"], c["c"], c["dt"])


def bwd_reference(c, ins, act, res, exact=False):
    """fp64 backward and the bounds of section 4 -> dict(dx, bdx, dgamma, bdgamma, dbeta, bdbeta).  exact (*int* mode): L = 0, dxhat = 0"""
    fam, chain = bwd_family(c)
    n, ch = c["n"], c["c"]
    gi = group_of(c, ch)
    x, da = ins["x"].double(), ins["da"].double()
    gamma = ins["gamma"].double()
    e4 = lambda t: t[:, :, None, None]
    mean, rstd = e4(ins["mr"][..., 0].double()[:, gi]), e4(ins["mr"][..., 1].double()[:, gi])
    sc, sh = e4(ins["ss"][..., 0].double()), e4(ins["ss"][..., 1].double())
    u = x * sc + sh
    if act == ACT_SILU:
        _, _, d1, dd = silu_terms(u, 2 * U * ((x * sc).abs() + sh.abs()))
        du = da * d1
        ddu = da.abs() * dd + U * du.abs()
    else:
        du, ddu = da, torch.zeros_like(da)
    xhat = (x - mean) * rstd
    if exact or fam == "raw":
        dxhat = torch.zeros_like(x)
    elif fam == "generic":
        dxhat = 2 * U * xhat.abs()
    else:
        dxhat = U * ((x * rstd).abs() + (mean * rstd).abs() + xhat.abs())
    l1, l2 = (0.0, 0.0) if exact else (chain * U, (chain + 1) * U)
    sp = lambda t: t.sum((2, 3))                                                     # per (n, c)
    s1, s2 = sp(du), sp(du * xhat)
    ds1 = l1 * sp(du.abs()) + sp(ddu)
    if fam == "raw":
        ds2 = rstd[:, :, 0, 0] * (l2 * sp((du * x).abs()) + sp(ddu * x.abs()) + mean[:, :, 0, 0].abs() * ds1)
    else:
        ds2 = l2 * sp((du * xhat).abs()) + sp(ddu * xhat.abs() + du.abs() * dxhat)
    grp = lambda t: t.reshape(n, G, -1).sum(-1)[:, gi]                                # sum over the channels of a group, back per channel
    a_, b_ = e4(grp(gamma[None] * s1)), e4(grp(gamma[None] * s2))
    da_, db_ = e4(grp(gamma.abs()[None] * ds1)), e4(grp(gamma.abs()[None] * ds2))
    m = float(ch // G * c["hw"])
    c1 = rstd * gamma[None, :, None, None]
    k2 = -rstd * rstd * b_ / m
    k3 = rstd * (mean * rstd * b_ - a_) / m
    dx = c1 * du - rstd / m * (a_ + xhat * b_)
    ev = 4 * U * ((c1 * du).abs() + (k2 * x).abs() + k3.abs()) + c1.abs() * ddu
    if res:
        dres = ins["dres"].double()
        dx = dx + dres
        ev = ev + U * (dres.abs() + dx.abs())
    e_all = ev + rstd / m * (da_ + xhat.abs() * db_)
    out = dict(dx=dx, bdx=HALF_ULP * (dx.abs() + e_all) + e_all if c["dt"] == "bf16" else e_all)
    for key, s_, d_ in (("dbeta", s1, ds1), ("dgamma", s2, ds2)):
        tot = s_.sum(0)
        out[key], out["b" + key] = tot, (d_ + U * s_.abs()).sum(0) + U * tot.abs()
    return out


def fused_reference(c, ins, mode, kern):
    """(r, extra): the exact values the epilogue sums and the error each carries (gauss: TAU S; int: none, the sums are exact)"""
    gauss = mode == "gauss"
    key = (c["name"], mode, kern)
    if _fused_cache.get("key") != key:          # one slot: judge and model ask for the same reference in turn
        r, s = CONV.reference_fwd(c, ins, phases=gauss and kern == UP2F, mags=gauss)
        _fused_cache.update(key=key, val=(r, (TAU * s if gauss else None)))
    return _fused_cache["val"]


_fused_cache = {}


def tile_sums(r, th=16, tw=32):
    """[n, C, H, W] -> [n, tiles_h * tiles_w, C]: sums over the in-map pixels of each 16 x 32 tile, in the wide kernel's row order"""
    n, ch, h, w = r.shape
    rp = F.pad(r, (0, -w % tw, 0, -h % th))
    t = rp.reshape(n, ch, rp.shape[2] // th, th, rp.shape[3] // tw, tw).sum((3, 5))
    return t.reshape(n, ch, -1).permute(0, 2, 1).contiguous()


def fused_sums_reference(r, extra, rows):
    """-> (s, q, bound_s, bound_q) per table row ([n, rows, C]; rows = True) or per (n, c) column ([n, C])"""
    a1 = r.abs() if extra is None else r.abs() + extra
    red = tile_sums if rows else (lambda t: t.sum((2, 3)))
    s, q = red(r), red(r * r)
    bs, bq = L_FUSED * U * red(a1), (L_FUSED + 1) * U * red(a1 * a1)
    if extra is not None:
        bs, bq = bs + red(extra), bq + red((2 * r.abs() + extra) * extra)
    return s, q, bs, bq


# --------------------------------------------------------------------------------------------- fp32 models of the kernels' arithmetic
f32 = np.float32


def _nhwc(t):
    """[n, C, H, W] tensor -> [n, HW, C] float32 array"""
    n, ch = t.shape[:2]
    return t.float().reshape(n, ch, -1).permute(0, 2, 1).contiguous().numpy()


def tree_sum(v, step):
    """v [rows, C] float32: row group j adds rows j, j + step, ... in order, then the groups are added in order (the streaming
    kernels' thread walk + fold with step = rstep, the small-map kernels' with step = TP)"""
    rows, ch = v.shape
    k = -(-rows // step)
    vp = np.zeros((k * step, ch), f32)
    vp[:rows] = v
    vp = vp.reshape(k, step, ch)
    acc = np.zeros((step, ch), f32)
    for i in range(k):
        acc = acc + vp[i]
    out = np.zeros(ch, f32)
    for j in range(step):
        out = out + acc[j]
    return out


def chain_sum(v):
    """sequential fp32 sum over rows (one order of the atomic branch)"""
    out = np.zeros(v.shape[1], f32)
    for i in range(v.shape[0]):
        out = out + v[i]
    return out


def planted(plant, kind):
    return plant is not None and plant[0] == kind


def plant_mask(plant, n, ch):
    """[n, C] bool: the (image, channel) pairs a planted error touches.  plant = (kind, cls): cls None = everywhere, else the groups with
    (image + group) % 3 == cls, the ones gauss mode gives PAIRS[cls]"""
    gi = np.arange(ch) // (ch // G)
    cls = (np.arange(n)[:, None] + gi[None, :]) % 3
    return np.ones((n, ch), bool) if plant[1] is None else cls == plant[1]


def model_channel_sums(c, planes, plant=None, small=False):
    """per image and channel the fp64 total of the per-block fp32 sums of every plane in ``planes`` ([n, HW, C] float32 arrays)"""
    n, hw, ch = planes[0].shape
    if small:
        blocks, step = [(0, hw)], small_threads(hw) // 8
    else:
        ns = pick_split(n, hw)
        rows_per = -(-hw // ns)
        blocks = [(min(hw, i * rows_per), min(hw, (i + 1) * rows_per)) for i in range(ns)]
        step = rstep(ch, c["dt"]) if stream_fixed(ch, c["dt"]) else None
    out = [np.zeros((n, ch), np.float64) for _ in planes]
    for i in range(n):
        for bi, (r0, r1) in enumerate(blocks):
            for k, p in enumerate(planes):
                if r1 <= r0:
                    continue
                v = p[i, r0:r1]
                part = (tree_sum(v, step) if step else chain_sum(v)).astype(np.float64)
                if planted(plant, "last_split_lost") and k == 1 and bi == len(blocks) - 1:      # the second sum of the last split
                    part = np.where(plant_mask(plant, n, ch)[i], 0.0, part)
                out[k][i] += part
    return out


def model_finalize(hw, s, q, gamma, beta, plant=None):
    """gn_stats_finalize / the small kernel's channel threads: fp64 groups, fp32 stores, scale_shift in fp32"""
    n, ch = s.shape
    cpg = ch // G
    m = float(cpg * hw)
    sg, qg = s.reshape(n, G, cpg).sum(-1), q.reshape(n, G, cpg).sum(-1)
    mean = sg / m
    var = np.maximum(qg / m - mean * mean, 0.0)
    if planted(plant, "var_m_minus_1"):
        var = np.where(plant_mask(plant, n, ch)[:, ::cpg], var * m / max(m - 1, 0.5), var)
    rstd = (1.0 / np.sqrt(var + EPS)).astype(f32)
    mean32 = mean.astype(f32)
    gi = np.arange(ch) // cpg
    ga, be = gamma.numpy().astype(f32), beta.numpy().astype(f32)
    sc = rstd[:, gi] * ga[None]
    ms = (mean32[:, gi] * sc).astype(f32)
    if planted(plant, "shift_from_unscaled_mean"):
        ms = np.where(plant_mask(plant, n, ch), (mean32[:, gi] * ga[None]).astype(f32), ms)
    sh = be[None] - ms
    return np.stack([mean32, rstd], -1), np.stack([sc.astype(f32), sh.astype(f32)], -1)


def model_stats(c, ins, plant=None):
    """(mean_rstd, scale_shift) float32 arrays as gn_stats (streaming) or gn_stats_act (small) form them"""
    x = _nhwc(ins["x"])
    if planted(plant, "pixel_dropped"):                          # one pixel of the first channel of every touched group
        first = np.arange(c["c"]) % (c["c"] // G) == 0
        x = x.copy()
        x[:, c["hw"] // 2, :] = np.where(plant_mask(plant, c["n"], c["c"]) & first[None], f32(0), x[:, c["hw"] // 2, :])
    s, q = model_channel_sums(c, [x, x * x], small=c["kind"] == "small")
    return model_finalize(c["hw"], s, q, ins["gamma"], ins["beta"], plant)


def _bf16_round(a32, truncate=False):
    t = torch.from_numpy(np.ascontiguousarray(a32))
    if truncate:
        return (t.view(torch.int32) & -65536).view(torch.float32)
    return t.bfloat16().float()


def _silu32(u):
    t = u * f32(-1.4426950408889634)
    s = f32(1.0) / (np.exp2(t).astype(f32) + f32(1.0))
    return (u * s).astype(f32), s.astype(f32)


def model_act(x, ss, act, dt, plant=None):
    """a [n, C, H, W] in the tensor's type from fp32 arithmetic on ``ss`` ([n, C, 2] float32 array)"""
    xa = x.float().numpy()
    u = (xa * ss[:, :, None, None, 0]).astype(f32) + ss[:, :, None, None, 1]
    if act == ACT_SILU:
        u, _ = _silu32(u)
    if dt == "f32":
        return torch.from_numpy(u)
    a = _bf16_round(u)
    if planted(plant, "a_truncated"):
        a = torch.where(torch.from_numpy(plant_mask(plant, *u.shape[:2]))[:, :, None, None], _bf16_round(u, truncate=True), a)
    return a.bfloat16()


def model_bwd(c, ins, act, res, plant=None):
    """(dx, dgamma, dbeta) from fp32 arithmetic in the order of the kernels ``bwd_family`` names"""
    fam, _ = bwd_family(c)
    n, ch, hw = c["n"], c["c"], c["hw"]
    cpg = ch // G
    gi = np.arange(ch) // cpg
    x, da = _nhwc(ins["x"]), _nhwc(ins["da"])
    mr, ss = ins["mr"].numpy(), ins["ss"].numpy()
    mu, rs = mr[:, gi, 0][:, None, :], mr[:, gi, 1][:, None, :]            # [n, 1, C]
    sc, sh = ss[:, None, :, 0], ss[:, None, :, 1]
    if act == ACT_SILU:
        u = (x * sc).astype(f32) + sh
        _, s = _silu32(u)
        du = (da * (s * ((u * (f32(1.0) - s)).astype(f32) + f32(1.0))).astype(f32)).astype(f32)
    else:
        du = da
    if fam == "raw":
        second = (du * x).astype(f32)
    elif fam == "generic":
        second = ((du * (x - mu).astype(f32)).astype(f32) * rs).astype(f32)
    else:
        second = (du * ((x * rs).astype(f32) + (-mu * rs).astype(f32)).astype(f32)).astype(f32)
    s1, s2 = model_channel_sums(c, [du, second], plant=plant, small=fam == "small")
    mu64, rs64 = mr[:, gi, 0].astype(np.float64), mr[:, gi, 1].astype(np.float64)
    if fam == "raw":
        s2 = rs64 * (s2 - mu64 * s1)
    nsum1, nsum2 = s1.astype(f32), s2.astype(f32)
    ga = ins["gamma"].double().numpy()
    m = float(cpg * hw)
    a_ = (ga[None] * s1).reshape(n, G, cpg).sum(-1)[:, gi]
    b_ = (ga[None] * s2).reshape(n, G, cpg).sum(-1)[:, gi]
    k0 = (rs64 * ga[None]).astype(f32)[:, None, :]
    k1 = (-rs64 * rs64 * b_ / m).astype(f32)[:, None, :]
    k2 = (rs64 * (mu64 * rs64 * b_ - a_) / m).astype(f32)
    if planted(plant, "k3_omitted"):                             # for the first channel of every touched group
        k2 = np.where(plant_mask(plant, n, ch) & (np.arange(ch) % cpg == 0)[None], f32(0), k2)
    k2 = k2[:, None, :]
    v = (k0 * du).astype(f32) + ((k1 * x).astype(f32) + k2).astype(f32)
    if res:
        dr = _nhwc(ins["dres"]).copy()
        if planted(plant, "dres_last_row"):
            dr[:, hw - c["w"]:, :] = np.where(plant_mask(plant, n, ch)[:, None, :], f32(0), dr[:, hw - c["w"]:, :])
        v = v.astype(f32) + dr
    v = np.ascontiguousarray(v.astype(f32).transpose(0, 2, 1)).reshape(n, ch, c["h"], c["w"])
    dx = torch.from_numpy(v) if c["dt"] == "f32" else _bf16_round(v).bfloat16()
    dgamma = torch.from_numpy(nsum2.astype(np.float64).sum(0).astype(f32))
    dbeta = torch.from_numpy(nsum1.astype(np.float64).sum(0).astype(f32))
    return dx, dgamma, dbeta


def model_fused_table(r, bias=None, plant=None):
    """the wide kernel's statistics rows [n, tiles, C, 2] float32 from v = float32(r): wave w of a tile owns pixel rows 2 w, 2 w + 1,
    half-wave g the columns (i & 3) + 8 (i >> 2) + 4 g of register i = 0 .. 15; a lane adds its 32 pixels in (row, register) order,
    the half-waves are added, then the 8 waves in order.  plant "edge_pixel_counted": the first out-of-map pixel of every ragged tile
    counts with the value bias[c]"""
    n, ch, h, w = r.shape
    th, tw = -(-h // 16), -(-w // 32)
    v = np.zeros((n, ch, th * 16, tw * 32), f32)
    v[:, :, :h, :w] = r.float().numpy()
    if planted(plant, "edge_pixel_counted"):
        b = bias.numpy().astype(f32)[None, :]
        if w % 32:
            v[:, :, 0, w] = b
        elif h % 16:
            v[:, :, h, 0] = b
    v = v.reshape(n, ch, th, 8, 2, tw, 4, 2, 4)               # [n, C, tile row, wave, j, tile col, i >> 2, g, i & 3]
    v = v.transpose(0, 2, 5, 3, 7, 4, 6, 8, 1)               # [n, tile row, tile col, wave, g, j, i >> 2, i & 3, C]
    v = np.ascontiguousarray(v).reshape(n, th * tw, 8, 2, 32, ch)
    out = np.zeros((n, th * tw, ch, 2), f32)
    for k, vals in enumerate((v, v * v)):
        lane = np.zeros(vals.shape[:4] + (ch,), f32)
        for i in range(32):
            lane = lane + vals[:, :, :, :, i]
        wave = lane[:, :, :, 0] + lane[:, :, :, 1]
        tot = np.zeros((n, th * tw, ch), f32)
        for wv in range(8):
            tot = tot + wave[:, :, wv]
        out[..., k] = tot
    return torch.from_numpy(out)


def model_record(c, mode, plant=None):
    """what the GPU child would have written for (c, mode) had the kernels been these models: the same keys, so ``judge`` takes either"""
    ins = make_inputs(c, mode)
    out = {}
    t = torch.from_numpy
    if c["kind"] == "stats":
        mr, ss = model_stats(c, ins, plant)
        out.update(stats_kernel="gn_stats_finalize", mr=t(mr), ss=t(ss))
        if stream_fixed(c["c"], c["dt"]):
            for act in (ACT_AFFINE, ACT_SILU):
                out["a%d" % act], out["a%d_kernel" % act] = model_act(ins["x"], ss, act, c["dt"], plant), "gn_act"
            if mode == "int":
                out["a_syn"] = model_act(ins["x"], ins["ss_syn"].numpy(), ACT_AFFINE, c["dt"], plant)
    elif c["kind"] == "small":
        mr, ss = model_stats(c, ins, plant)
        for act in (ACT_AFFINE, ACT_SILU):
            a = model_act(ins["x"], ss, act, c["dt"], plant)
            out.update({"k%d" % act: "gn_small_fwd", "mr%d" % act: t(mr), "ss%d" % act: t(ss), "a%d" % act: a, "a%d_gn_act" % act: a.clone()})
    elif c["kind"] == "bwd":
        fam, _ = bwd_family(c)
        for act, res in ACT_RES:
            if mode == "int" and act == ACT_SILU:
                continue
            key = "%d%d" % (act, res)
            out["dx" + key], out["dg" + key], out["db" + key] = model_bwd(c, ins, act, res, plant)
            out["k" + key] = "gn_param_reduce" if fam == "small" else "gn_bwd_apply"
    else:
        kern = UP2F if c["up"] else WIDE
        r, _ = fused_reference(c, ins, mode, kern)
        if kern == WIDE:
            table = model_fused_table(r, ins["b"], plant)
        else:                                    # (the sub-pixel kernel's rows are not judged one by one: one row per image, same lane order)
            rr = r.float().numpy()
            if planted(plant, "edge_pixel_counted"):
                rr = rr.copy()
                rr[:, :, 0, 0] += ins["b"].numpy()[None]
            flat = np.ascontiguousarray(rr.reshape(rr.shape[0], rr.shape[1], -1).transpose(0, 2, 1))
            table = torch.from_numpy(np.stack([np.stack([tree_sum(p, 64) for p in v]) for v in (flat, flat * flat)], -1))[:, None]
        s64 = table.double().sum(1)
        mr, ss = model_finalize(c["ho"] * c["wo"], s64[..., 0].numpy(), s64[..., 1].numpy(), ins["gamma"], ins["beta"], plant)
        out.update(fwd_kernel=kern, stats_kernel="gn_stats_from_partials", table=table, rows=table.shape[1], mr=t(mr), ss=t(ss),
                   features=["tiles_gt_grid"] if "tiles_gt_grid" in c["feats"] else [])
    return out


# ---------------------------------------------------------------------------------------------------------------------------- judging
INT_ACT_TIES = 0.08           # *int* mode gn_act on the power-of-two table: at least this share of exact bf16 ties (bf16 cases)


def judge(c, mode, rec):
    """every check of one (case, mode) recording -> (rows, reached, failures): rows = (output, family, figure, verdict) with verdict
    "" (inside the bound), "equal" (an *int* mode equality that holds) or a complaint; reached = the (kernel, feature) pairs"""
    ins = make_inputs(c, mode)
    rows, reached, failures = [], set(), []
    gauss = mode == "gauss"
    name = c["name"]

    def put(key, fam, pair, equality=False):
        fig, bad = pair
        verdict = ("equal" if equality else "") if bad == 0 and fig <= 1 else f"{bad} OUTSIDE" if not equality else f"{bad} DIFFER"
        rows.append((key, fam, "%.3f" % fig, verdict))
        if verdict not in ("", "equal"):
            failures.append(f"{name} {mode} {key} ({fam}): {verdict}, worst figure {fig:.3f}")

    def equal(key, fam, got, want):
        nd = int((got.double() != want.double()).sum()) + int((~torch.isfinite(got.double())).sum())
        put(key, fam, (float(nd > 0), nd), equality=True)

    def stats_rows(tag, fam, mr, ss, ref):
        for k, pair in judge_stats(mr, ref, mode).items():
            put(tag + k, f"{fam} {k}", pair, equality=(mode == "int" and k == "mean"))
        for k, pair in judge_table(ss, mr, ins["gamma"], ins["beta"]).items():
            put(tag + k, f"{fam} {k}", pair)

    def act_rows(key, fam, a, ss, act, dt):
        r, e = act_reference(ins["x"], ss, act)
        put(key, fam, _ratio(a, r, act_bound(r, e, dt)))

    def expect(key, want):
        if rec[key] != want:
            failures.append(f"{name} {mode}: {key} is {rec[key]}, not {want}")
        return rec[key] == want

    if c["kind"] == "stats":
        dt, branch = c["dt"], "fixed" if stream_fixed(c["c"], c["dt"]) else "atomic"
        ref = stats_reference(ins["x"].double(), stream_chain(c["n"], c["hw"], c["c"], dt))
        if expect("stats_kernel", "gn_stats_finalize"):
            reached.add(("gn_stats_finalize", branch))
        stats_rows("", f"gn_stats_partial[{branch}] {dt}", rec["mr"], rec["ss"], ref)
        for act in (ACT_AFFINE, ACT_SILU):
            if "a%d" % act in rec:
                if expect("a%d_kernel" % act, "gn_act"):
                    reached.add(("gn_act", dt))
                act_rows("a%d" % act, f"gn_act act{act} {dt}", rec["a%d" % act], rec["ss"], act, dt)
        assert ("a1" in rec) == stream_fixed(c["c"], dt), name
        if "a_syn" in rec:
            r, want = int_act_expected(ins["x"], ins["ss_syn"], dt)
            if dt == "bf16":
                ties = bf16_ties(r)
                assert ties >= INT_ACT_TIES, (name, "the int-mode activation reference has no ties", ties)
            equal("a_syn", f"gn_act act1 {dt}", rec["a_syn"], want)
    elif c["kind"] == "small":
        units = small_fwd_instance(c["hw"])
        ref = stats_reference(ins["x"].double(), small_chain(c["hw"]))
        for act in (ACT_AFFINE, ACT_SILU):
            if expect("k%d" % act, "gn_small_fwd"):
                reached.add(("gn_small_fwd", "units%d" % units))
            fam = f"gn_small_fwd<{units}>"
            stats_rows("act%d " % act, fam, rec["mr%d" % act], rec["ss%d" % act], ref)
            act_rows("a%d" % act, f"gn_small_fwd act{act}", rec["a%d" % act], rec["ss%d" % act], act, "bf16")
            equal("a%d=gn_act" % act, "gn_small_fwd vs gn_act", rec["a%d" % act], rec["a%d_gn_act" % act])
    elif c["kind"] == "bwd":
        fam, _ = bwd_family(c)
        label = {"small": "gn_small_bwd<%d>" % small_bwd_instance(c["hw"]), "raw": "gn_bwd_apply_pk", "generic": "gn_bwd_apply<float>"}[fam]
        for act, res in ACT_RES:
            key = "%d%d" % (act, res)
            if "dx" + key not in rec:
                assert mode == "int" and act == ACT_SILU, (name, key)
                continue
            if expect("k" + key, "gn_param_reduce" if fam == "small" else "gn_bwd_apply"):
                if fam == "small":
                    reached.add(("gn_param_reduce", "units%d" % small_bwd_instance(c["hw"])))
                    reached.add(("gn_param_reduce", "act%d_res%d" % (act, res)))
                else:
                    reached.add(("gn_bwd_apply", "packed" if fam == "raw" else "generic"))
            ref = bwd_reference(c, ins, act, res, exact=not gauss)
            put("dx act%d res%d" % (act, res), label + " dx", _ratio(rec["dx" + key], ref["dx"], ref["bdx"]))
            for short, full in (("dg", "dgamma"), ("db", "dbeta")):
                if gauss:
                    put("%s act%d res%d" % (full, act, res), f"{label} {full}", _ratio(rec[short + key], ref[full], ref["b" + full]))
                else:           # representable on the reference alone, before the kernel's output is looked at
                    assert torch.equal(ref[full].float().double(), ref[full]), (name, full, "not representable in fp32")
                    equal("%s act%d res%d" % (full, act, res), f"{label} {full}", rec[short + key], ref[full].float())
    else:
        kern = rec["fwd_kernel"]
        want_kern = UP2F if c["up"] else WIDE
        if kern != want_kern:
            failures.append(f"{name} {mode}: forward took {kern}, not {want_kern}")
        if expect("stats_kernel", "gn_stats_from_partials") and kern == want_kern:
            reached |= {("gn_stats_from_partials", f"{kern}:{f}") for f in list(c["feats"]) + rec["features"]}
        r, extra = fused_reference(c, ins, mode, kern)
        table = rec["table"].double()
        n, cout = c["n"], c["cout"]
        if not gauss:           # on the reference alone: every sum of a table row exact in fp32
            worst = tile_sums(r * r).max() if kern == WIDE else (r * r).sum((2, 3)).max()
            assert float(worst) < 2 ** 24, (name, "int-mode sums are not exact", float(worst))
        for rows_, tag in ([(True, "row")] if kern == WIDE else []) + [(False, "column")]:
            s, q, bs, bq = fused_sums_reference(r, extra, rows_)
            got = table if rows_ else table.sum(1)
            if rows_ and got.shape[1] != s.shape[1]:
                failures.append(f"{name} {mode}: {got.shape[1]} table rows, {s.shape[1]} tiles")
                continue
            for k, (want, bound) in enumerate(((s, bs), (q, bq))):
                key = "%s sum%s" % (tag, " x^2" if k else " x")
                if gauss:
                    put(key, f"{kern} statistics {tag}s", _ratio(got[..., k], want, bound))
                else:
                    equal(key, f"{kern} statistics {tag}s", got[..., k], want)
        stats_rows("", f"gn_stats_from_partials <- {kern}", rec["mr"], rec["ss"], stats_reference(r, L_FUSED, extra))
    return rows, reached, failures


# ------------------------------------------------------------------------------------------------------------------------- GPU child
def run(setting, out_path):
    from mas_hip import ops
    label, env, cases = next(s for s in SETTINGS if s[0] == setting)
    for k, v in env.items():
        assert os.environ.get(k) == v, f"start this child with {k}={v}"
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ops.set_compute_dtype(torch.bfloat16)
    cl = lambda t: None if t is None else t.to(dev).contiguous(memory_format=torch.channels_last)
    back = lambda t: t.detach().cpu().contiguous()
    results = {}
    for c in cases:
        for mode in MODES:
            ins = make_inputs(c, mode)
            gd, bd = ins["gamma"].to(dev), ins["beta"].to(dev)
            out = {}
            if c["kind"] == "stats":
                xd = cl(ins["x"])
                mr, ss = ops.gn_stats(xd, gd, bd, G, EPS)
                out["stats_kernel"] = ops.last_kernel()
                out["mr"], out["ss"] = back(mr), back(ss)
                if ops._gn_act_ok(c["c"], xd.dtype):
                    for act in (ACT_AFFINE, ACT_SILU):
                        out["a%d" % act] = back(ops.gn_act(xd, ss, act))
                        out["a%d_kernel" % act] = ops.last_kernel()
                    if mode == "int":
                        out["a_syn"] = back(ops.gn_act(xd, ins["ss_syn"].to(dev), ACT_AFFINE))
            elif c["kind"] == "small":
                xd = cl(ins["x"])
                assert ops.gn_small_ok(xd, G), c["name"]
                for act in (ACT_AFFINE, ACT_SILU):
                    mr, ss, a = ops.gn_stats_act(xd, gd, bd, G, EPS, act)
                    out["k%d" % act] = ops.last_kernel()
                    out["mr%d" % act], out["ss%d" % act], out["a%d" % act] = back(mr), back(ss), back(a)
                    out["a%d_gn_act" % act] = back(ops.gn_act(xd, ss, act))      # mas_gn_act on the small kernel's table
            elif c["kind"] == "bwd":
                xd, dad, drd = cl(ins["x"]), cl(ins["da"]), cl(ins["dres"])
                mrd, ssd = ins["mr"].to(dev), ins["ss"].to(dev)
                for act, res in ACT_RES:
                    if mode == "int" and act == ACT_SILU:
                        continue
                    dx, dg, db = ops.gn_bwd(xd, dad, drd if res else None, G, act, gd, mrd, ssd, path=c["path"])
                    key = "%d%d" % (act, res)
                    out["k" + key] = ops.last_kernel()
                    out["dx" + key], out["dg" + key], out["db" + key] = back(dx), back(dg), back(db)
            else:
                n, cin, cout, h, w = c["n"], c["cin"], c["cout"], c["h"], c["w"]
                ho, wo, (pt, pb, pl, pr) = c["ho"], c["wo"], c["pad"]
                ops._stats_state["on"] = True
                wd, bsd = ins["w"].to(dev), (ins["b"].to(dev) if ins["b"] is not None else None)
                y, partial, rows = ops.conv_fwd_raw(cl(ins["x"]), None, ops.ConvWeight(wd, False), bsd, cl(ins["res"]), n, h, w, cin, ho, wo, cout,
                                                    c["ks"], c["stride"], pt, pl, c["act"], c["up"], torch.bfloat16, want_stats=True)
                out["fwd_kernel"] = ops.last_kernel()
                assert partial is not None and rows > 0, (c["name"], "the launch filled no statistics table")
                feats = set()
                if setting == "multi":                   # launch geometry: grid = min(tiles, MAS_CONV_WGS_PER_CU * CUs)
                    if out["fwd_kernel"] == WIDE:
                        tiles = n * ((ho + 15) // 16) * ((wo + 31) // 32) * (cout // 128)
                    else:
                        tiles = (n * ((h + 15) // 16) * ((w + 31) // 32) + 7) // 8 * 8 * 4 * (cout // 128)
                    assert int(os.environ["MAS_CONV_WGS_PER_CU"]) == 1 and tiles > cus, (c["name"], tiles, cus)
                    feats.add("tiles_gt_grid")
                mr, ss = ops.gn_stats(y, gd, bd, G, EPS, partial, rows)
                out["stats_kernel"] = ops.last_kernel()
                torch.cuda.synchronize()
                out["table"], out["rows"] = back(partial).view(n, rows, cout, 2), rows
                out["mr"], out["ss"] = back(mr), back(ss)
                out["features"] = sorted(feats)
            torch.cuda.synchronize()
            results[(c["name"], mode)] = out
            print(f"{label:8s} {c['name']:16s} {mode:5s} " + " ".join(f"{k}={v}" for k, v in sorted(out.items()) if "kernel" in k or k[0] == "k"), flush=True)
    torch.save(dict(results=results, cus=cus, env={k: os.environ.get(k) for k in env}), out_path)


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2])
