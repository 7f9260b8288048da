"""Causal attention (make-a-scene_amd/csrc/attention.hip) judged row by row: cases, input builders, the fp64 reference, the bounds, a CPU
model of the kernels' arithmetic with its mutations, and ``run`` (GPU only: the raw entries through ``ops.lib()``).  Importing this file
needs neither a GPU nor the library.  tests/test_attn_rowwise_cpu.py shows that the bounds have teeth, tests/test_gpu_attn_rowwise.py
judges the kernels.

Layout here is [B, H, S, hd] float64 throughout; ``run`` packs / unpacks the kernels' [B, S, H*hd] buffers.

Reference (``reference``; the plain formula on exactly the operands handed to the kernel, bf16 cases rounded to bf16 first):
  s = scale q k^T over keys <= query, lse = logsumexp(s), P = exp(s - lse), o = (P o Z) v, D = rowsum(dO o o), dV = (P o Z)^T dO,
  dP = dO v^T, dS = P o (dP o Z - D) scale, dQ = dS k, dK = dS^T q;  Z = keep mask * drop scale (1 without dropout).
Magnitudes, the same formula on absolute values:  A_o = (P o Z)|v|, A_D = rowsum(|dO| o |o|), A_dV = (P o Z)^T |dO|,
  A_dS = P o (|dP| o Z + |D|) scale, A_dQ = A_dS |k|, A_dK = A_dS^T |q|, and for the error D carries into dS (below)
  AD_dS = P o A_D scale, AD_dQ = AD_dS |k|, AD_dK = AD_dS^T |q|.

What the backward is fed.  ``run`` hands the backward entries the REFERENCE's o rounded to the kernel's dtype and the reference's lse
rounded to fp32, not the forward kernel's outputs: the forward is judged on its own, and the backward's bounds then depend on nothing
but the backward's own arithmetic.  (The chain forward -> backward is what the older norm tests run.)

Bounds, U = 2^-8 (half a bf16 ulp, round-to-nearest-even), TAU = 2^-18 (fp32 MFMA accumulation, the value of both other element-wise
suites).  bf16 kernels, every element:  |y - r| <= U |r| + c U A + TAU A  (+ (U + TAU) AD for dQ, dK).  The counts, from attention.hip:
  o      c = 1: the unnormalised probabilities exp(s - m) are cast to bf16 as the B operand of O^T += V^T P^T
                (generic ``pf[j] = (T)s[8 * t + j]``; fast / v2 ``pf[j] = (T)s[sub][8 * t + j]``); the running sum l, the rescale
                factors alpha and the final 1 / l stay fp32.  U |r| is the store ``(T)(oacc[i][r] * inv)``.  Dropout zeroes
                probabilities before that cast and its scale goes into the fp32 ``inv``: no further rounding.
  delta  no output rounding (fp32).  The kernel sums dO * o over the ALREADY ROUNDED o (attn_bwd_delta_kernel reads the bf16 o):
                |o_in - o| <= U |o| gives U A_D; TAU A_D for the fp32 sum.
  dV     c = 1: P (o keep mask) is cast to bf16 for dV^T += dO^T P (``pf[j] = (T)s[8 * t + j]`` in attn_bwd_dkv_kernel and
                attn_bwd_dkv_bf16_kernel); the dropout scale multiplies the fp32 accumulator.  U |r| is the store ``(T)dv[i][r]``.
  dQ, dK c = 1: dS = P (dP - D) scale is computed in fp32 from the fp32 P (the bf16 cast of P feeds dV only) and cast once,
                ``sf[j] = (T)dp[8 * t + j]``, for dQ^T += K^T dS^T (dq kernels) and dK^T += Q^T dS (dkv kernels).  U |r| is the store.
                D enters dS with the error counted under delta, (U + TAU) A_D per row, which A_dS (built on |D|, not A_D) does not
                hold when dO o o cancels: it is carried by its own magnitude, (U + TAU) AD.
fp32 kernels: no cast anywhere; |y - r| <= C_F32 TAU (A + AD), delta K_DELTA 2^-23 A_D.  lse (all kernels, fp32 in every one of them):
|lse - r| <= K_LSE 2^-23 max(1, |lse|, max|s| of the row).  C_F32, K_DELTA and K_LSE cover __expf / v_exp_f32, __logf and the accumulation
order and are MEASURED on an MI355X (next power of two above twice the worst seen; figures in tests/test_gpu_attn_rowwise.py).

Operand modes (``make_inputs``):
  gauss    randn q, k, v, dO.
  hard     gauss + a planted score structure: the first PLANT = 10 head dims of k carry the +-1 bit code of the key index, those of q
           a * (bit code of the target key t(i)), a = round(6 / scale) (an integer, exact in bf16), so the scaled score is about +60 at
           the target, 60 - 12 h at Hamming distance h from it, about 0 for the bulk and -60 at the complement.  t(i) follows
           ``target``; 2 rows in 13 keep their gauss q, so rescale and no-rescale rows share a wave.
  onehot   k_j = a +-1 code of key j over ALL head dims (pairwise Hamming distance >= DMIN[hd]), q_i = c * code(t(i)), v and dO integers
           in +-{1..4}; c is the smallest integer that puts every other key at least GAP = 32 below the target.  ``onehot_precondition``
           asserts on the reference alone: every row's off-target mass times max|v| is below 2^-30 (so is the second-largest probability)
           and every per-key integer sum of dO is exact in bf16.  Then o[i] == v[t(i)] and dV[j] == sum of dO over {i: t(i) = j} BITWISE
           (bf16 kernels; the fp32 kernels' dV takes the general bound: their P is exp(s - lse) of scores near 60, 1 + O(1e-5)),
           dV of a key whose integer sum is zero (no query chose it, or the dO of its queries cancel) is below 2^-30 sum|dO| + TAU A_dV
           (the MFMA's fp32 adder leaves up to an ulp of the cancelled terms behind), lse[i] is the target's score, dQ and dK obey the
           general bound.
  uniform  q = 0: every score is 0, P = 1 / (i + 1), lse[i] = log(i + 1); integer v and dO.
"""
import functools
import zlib

import numpy as np

U, TAU = 2.0 ** -8, 2.0 ** -18
# measured coefficients (procedure and figures: tests/test_gpu_attn_rowwise.py)
C_F32 = 32.0
K_DELTA = 4.0
K_LSE = {("attn_causal_fwd_generic", "f32"): 32.0, ("attn_causal_fwd_generic", "bf16"): 4.0, ("attn_causal_fwd_v2", "bf16"): 4.0,
         ("attn_causal_fwd_fast", "bf16"): 8.0}

# fp32 underflow: a product below the normal range (2^-126) may be flushed to zero or lose its low bits; an element sums at most
# S * hd <= 2^16 such terms with operands below 2^9, so what underflow can move stays below 2^-100, an absolute floor under every bound
FLOOR = 2.0 ** -100
PLANT = 10
GAP = 32.0
DMIN = {16: 4, 32: 8, 64: 20, 128: 48,
        96: 24, 160: 48, 384: 140, 512: 200}    # the channel widths of tests/helpers/spatial_attn_check.py (code books of up to 769 keys)
DROP_P, DROP_SEED = 0.25, (0x1234ABCD5678, 7)
N_RULES = 11

FWD_V2, FWD_FAST, FWD_GEN = "attn_causal_fwd_v2", "attn_causal_fwd_fast", "attn_causal_fwd_generic"
BWD_FAST, BWD_GEN = "attn_causal_bwd_fast64", "attn_causal_bwd_generic"
S_ALL = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 321)


# --------------------------------------------------------------------------- #
# cases
# --------------------------------------------------------------------------- #
def _case(family, dtype, hd, S, fwd, bwd, B=2, H=3, layout="fused", p=0.0, bwd_layout="fused"):
    """layout: how the FORWARD gets q, k, v ("fused" [B,S,3d]; "sep68": three buffers with token strides = 4 mod 8 elements, the
    fa_aligned() fallback; "sep_al": three buffers with different 16-byte aligned token and batch strides).  bwd_layout: "fused", or
    "fused_off8": the fused buffers start 8 bytes past a 16-byte boundary (the generic backward at head width 64); None: no backward."""
    name = f"{family}-{dtype}-hd{hd}-B{B}H{H}S{S}-{layout}" + ("-drop" if p else "")
    modes = ("gauss", "hard") if p else ("gauss", "hard", "onehot", "uniform")
    return dict(name=name, family=family, dtype=dtype, hd=hd, S=S, B=B, H=H, fwd=fwd, bwd=bwd, layout=layout, p=p, bwd_layout=bwd_layout,
                modes=modes, tile=64 if fwd in (FWD_V2, FWD_FAST) else 32)


def _cases():
    c = []
    # generic fp32 forward and backward
    c += [_case("f32_generic", "f32", 64, S, FWD_GEN, BWD_GEN) for S in S_ALL]
    c += [_case("f32_generic", "f32", hd, S, FWD_GEN, BWD_GEN) for hd in (16, 32, 128) for S in (33, 129, 257)]
    c += [_case("f32_generic", "f32", 32, 65, FWD_GEN, BWD_GEN, B=1, H=1)]
    # generic bf16: head widths 16 and 32; head width 64 through the unaligned forward layout and the offset fused backward
    c += [_case("bf16_generic", "bf16", 32, S, FWD_GEN, BWD_GEN) for S in S_ALL]
    c += [_case("bf16_generic", "bf16", 16, S, FWD_GEN, BWD_GEN) for S in (1, 33, 64, 129, 257, 321)]
    c += [_case("bf16_generic", "bf16", 16, 65, FWD_GEN, BWD_GEN, B=1, H=1)]
    c += [_case("bf16_generic64", "bf16", 64, S, FWD_GEN, BWD_GEN, layout="sep68", bwd_layout="fused_off8") for S in (1, 33, 64, 129, 257, 321)]
    c += [_case("bf16_generic64", "bf16", 64, 65, FWD_GEN, BWD_GEN, B=1, H=1, layout="sep68", bwd_layout="fused_off8")]
    # v2 forward + fast64 backward; v2 forward from three separate aligned buffers
    c += [_case("v2_fast64", "bf16", 64, S, FWD_V2, BWD_FAST) for S in S_ALL]
    c += [_case("v2_fast64", "bf16", 64, 129, FWD_V2, BWD_FAST, B=1, H=1)]
    c += [_case("v2_fast64", "bf16", 64, S, FWD_V2, None, layout="sep_al", bwd_layout=None) for S in (33, 129, 257, 321)]
    # head width 128: fast forward + generic backward
    c += [_case("fast128", "bf16", 128, S, FWD_FAST, BWD_GEN) for S in S_ALL]
    c += [_case("fast128", "bf16", 128, 65, FWD_FAST, BWD_GEN, B=1, H=1)]
    # dropout, p = 0.25
    c += [_case("dropout", "bf16", 64, S, FWD_V2, BWD_FAST, p=DROP_P) for S in (33, 64, 129, 257, 321)]
    c += [_case("dropout", "bf16", 32, S, FWD_GEN, BWD_GEN, p=DROP_P) for S in (33, 64, 129, 257)]
    c += [_case("dropout", "f32", 64, S, FWD_GEN, BWD_GEN, p=DROP_P) for S in (33, 64, 129, 257)]
    return c


CASES = _cases()
FAMILIES = ("f32_generic", "bf16_generic", "bf16_generic64", "v2_fast64", "fast128", "dropout")


def features(c):
    """what a case exercises in the kernel that serves it (tile = that kernel's key tile)"""
    t = c["tile"]
    n = -(-c["S"] // t)
    f = {c["dtype"], "hd%d" % c["hd"], "tiles_odd" if n % 2 else "tiles_even"}
    if c["S"] % t:
        f.add("ragged")
    if c["S"] < t:
        f.add("sub_tile")
    if c["S"] > 128:
        f.add("multi_block")
    if c["p"]:
        f.add("drop")
    if c["B"] == 1 and c["H"] == 1:
        f.add("bh1")
    if c["layout"] != "fused":
        f.add(c["layout"])
    return f


def bwd_features(c):
    f = features(c) - {"sep68", "sep_al"}
    if c["bwd_layout"] == "fused_off8":
        f.add("fused_off8")
    return f


_SHAPE = {"tiles_odd", "tiles_even", "ragged", "sub_tile", "multi_block", "bh1"}
REQUIRED = {
    FWD_V2: _SHAPE | {"bf16", "hd64", "drop", "sep_al"},
    FWD_FAST: _SHAPE | {"bf16", "hd128"},
    FWD_GEN: _SHAPE | {"f32", "bf16", "hd16", "hd32", "hd64", "hd128", "drop", "sep68"},
    BWD_FAST: _SHAPE | {"bf16", "hd64", "drop"},
    BWD_GEN: _SHAPE | {"f32", "bf16", "hd16", "hd32", "hd64", "hd128", "drop", "fused_off8"},
}


def reached(cases_and_kernels):
    """[(case, fwd kernel name, bwd kernel name or None)] -> {kernel: features}"""
    got = {}
    for c, kf, kb in cases_and_kernels:
        got.setdefault(kf, set()).update(features(c))
        if kb is not None:
            got.setdefault(kb, set()).update(bwd_features(c))
    return got


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def bf16_round(x):
    """float -> nearest bf16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def bf16_trunc(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def target(i, rule):
    """the key that holds query i's maximum.  Rules: 0 key 0; 1 the diagonal; 2 / 3 the last key of the first 32- / 64-key tile;
    4 / 5 the first key of the query's own (last) 32- / 64-key tile; 6..9 keys 31 / 32 / 63 / 64 counted from the start of the 64-key tile
    before the query's; 10 the key before the diagonal.  Always clipped to [0, i]."""
    if rule == 0:
        t = 0
    elif rule == 1:
        t = i
    elif rule == 2:
        t = 31
    elif rule == 3:
        t = 63
    elif rule == 4:
        t = (i // 32) * 32
    elif rule == 5:
        t = (i // 64) * 64
    elif rule in (6, 7, 8, 9):
        t = max((i // 64) * 64 - 64, 0) + (31, 32, 63, 64)[rule - 6]
    else:
        t = i - 1
    return min(max(t, 0), i)


def targets(S, cycle):
    """rule of row i = i mod cycle (cycle is odd, so every rule meets every lane of a wave); rules >= N_RULES mean 'no target' (-1)"""
    return np.array([target(i, i % cycle) if i % cycle < N_RULES else -1 for i in range(S)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def codes(hd, n):
    """n distinct +-1 codes of length hd with pairwise Hamming distance >= DMIN[hd] (greedy over seeded random draws)"""
    rs = np.random.RandomState(1000 + hd)
    out = np.zeros((0, hd), dtype=np.int64)
    while len(out) < n:
        cand = rs.randint(0, 2, size=(4096, hd)) * 2 - 1
        for v in cand:
            if len(out) == 0 or (hd - out @ v).min() >= 2 * DMIN[hd]:      # hd - <a, b> = 2 * Hamming distance
                out = np.vstack([out, v[None]])
                if len(out) == n:
                    break
    return out


def _ints(rs, shape):
    return (rs.randint(1, 5, size=shape) * (rs.randint(0, 2, size=shape) * 2 - 1)).astype(np.float64)


def make_inputs(c, mode):
    B, H, S, hd = c["B"], c["H"], c["S"], c["hd"]
    rs = np.random.RandomState(zlib.crc32((c["name"] + mode).encode()) & 0x7FFFFFFF)
    scale = float(np.float32(hd ** -0.5))
    shape = (B, H, S, hd)
    rnd = (lambda x: bf16_round(x).astype(np.float64)) if c["dtype"] == "bf16" else (lambda x: x.astype(np.float32).astype(np.float64))
    q, k, v, do = (rnd(rs.randn(*shape)) for _ in range(4))
    tg = None
    if mode == "hard":
        a = float(round(6.0 / scale))
        tg = targets(S, 13)
        bits = ((np.arange(S)[:, None] >> np.arange(PLANT)[None, :]) & 1) * 2.0 - 1.0         # [S, PLANT]
        k[..., :PLANT] = bits
        rows = tg >= 0
        q[:, :, rows, :PLANT] = a * bits[tg[rows]]
    elif mode == "onehot":
        tg = targets(S, N_RULES)
        # every (batch, head) draws its own key permutation of the code book: a head or batch mix-up reads foreign codes
        book = codes(hd, max(S, 2))
        k = np.empty(shape)
        q = np.empty(shape)
        for b in range(B):
            for h in range(H):
                kc = book[rs.permutation(len(book))[:S]].astype(np.float64)
                k[b, h] = kc
                q[b, h] = kc[tg]
        cq = float(np.ceil(GAP / (scale * 2 * DMIN[hd])))
        q *= cq
        v, do = _ints(rs, shape), _ints(rs, shape)
    elif mode == "uniform":
        q = np.zeros(shape)
        v, do = _ints(rs, shape), _ints(rs, shape)
    elif mode != "gauss":
        raise ValueError(mode)
    return dict(q=q, k=k, v=v, do=do, scale=scale, target=tg)


def drop_z(c, keep=None):
    """Z = keep * scale for a dropout case (keep: [B,H,S,S] 0/1 from mas_attn_dropout_mask; None: the Philox restatement), else None"""
    if not c["p"]:
        return None
    import philox_ref as R
    if keep is None:
        keep = R.attention_keep(DROP_SEED[0], DROP_SEED[1], c["B"], c["H"], c["S"], c["p"])
    return np.asarray(keep, dtype=np.float64) * R.scale(R.threshold(c["p"]))


# --------------------------------------------------------------------------- #
# fp64 reference and bounds
# --------------------------------------------------------------------------- #
def reference(ins, Z=None):
    q, k, v, do, scale = ins["q"], ins["k"], ins["v"], ins["do"], ins["scale"]
    S = q.shape[2]
    T = lambda x: np.swapaxes(x, -1, -2)
    causal = np.tril(np.ones((S, S), dtype=bool))
    s = scale * (q @ T(k))
    sm = np.where(causal, s, -np.inf)
    mx = sm.max(-1, keepdims=True)
    lse = mx[..., 0] + np.log(np.exp(sm - mx).sum(-1))
    P = np.exp(sm - lse[..., None])
    Z = np.ones_like(P) if Z is None else Z
    PZ = P * Z
    o, A_o = PZ @ v, PZ @ np.abs(v)
    D, A_D = (do * o).sum(-1), (np.abs(do) * np.abs(o)).sum(-1)
    dV, A_dV = T(PZ) @ do, T(PZ) @ np.abs(do)
    dP = do @ T(v)
    dS = P * (dP * Z - D[..., None]) * scale
    A_dS = P * (np.abs(dP) * Z + np.abs(D)[..., None]) * scale
    AD_dS = P * A_D[..., None] * scale
    return dict(P=P, lse=lse, smax=np.where(causal, np.abs(s), 0.0).max(-1), o=o, A_o=A_o, delta=D, A_delta=A_D, dv=dV, A_dv=A_dV,
                dq=dS @ k, dk=T(dS) @ q, A_dq=A_dS @ np.abs(k), A_dk=T(A_dS) @ np.abs(q), AD_dq=AD_dS @ np.abs(k), AD_dk=T(AD_dS) @ np.abs(q))


def bound(ref, key, dtype, fwd=None):
    r = ref[key]
    if key == "lse":
        return K_LSE[(fwd, dtype)] * 2.0 ** -23 * np.maximum(1.0, np.maximum(np.abs(r), ref["smax"]))
    A = ref["A_" + key]
    AD = ref["AD_" + key] if key in ("dq", "dk") else 0.0
    if dtype == "f32":
        return FLOOR + (K_DELTA * 2.0 ** -23 * A if key == "delta" else C_F32 * TAU * (A + AD))
    if key == "delta":
        return FLOOR + U * A + TAU * A
    return FLOOR + U * np.abs(r) + U * A + TAU * A + (U + TAU) * AD


def onehot_precondition(ins, ref):
    """asserted on the reference alone, before any kernel output is looked at"""
    tg, v, do = ins["target"], ins["v"], ins["do"]
    S = v.shape[2]
    off = 1.0 - ref["P"][:, :, np.arange(S), tg]
    assert (off * np.abs(v).max() < 2.0 ** -30).all(), float(off.max())
    P2 = ref["P"].copy()
    P2[:, :, np.arange(S), tg] = 0.0
    assert (P2.max(-1) < 2.0 ** -30).all()
    sums = np.zeros_like(do)
    np.add.at(sums, (slice(None), slice(None), tg), do)
    assert (np.abs(sums) <= 256).all()                  # integers up to 256 are exact in bf16
    asum = np.zeros_like(do)
    np.add.at(asum, (slice(None), slice(None), tg), np.abs(do))
    return sums, asum


def judge(c, mode, ins, ref, got):
    """-> (failures: [str], worst: {tensor: ratio}).  got: the tensors a kernel (or the model) produced, any subset of
    o, lse, delta, dq, dk, dv."""
    fails, worst = [], {}
    tag = f"{c['name']} {mode}"
    for key in ("o", "lse", "delta", "dv", "dq", "dk"):
        if key not in got:
            continue
        y, r = np.asarray(got[key], dtype=np.float64), ref[key]
        assert y.shape == r.shape, (tag, key, y.shape, r.shape)
        bd = bound(ref, key, c["dtype"], c["fwd"])
        err = np.abs(y - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bd > 0, err / bd, np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(y), ratio, np.inf)
        worst[key] = float(ratio.max())
        bad = ~(err <= bd) | ~np.isfinite(y)
        if bad.any():
            first = tuple(int(i) for i in np.argwhere(bad)[0])
            fails.append(f"{tag}, {key}: {int(bad.sum())} of {bad.size} elements outside, worst ratio {worst[key]:.3g}, first bad (b, h, row"
                         f"{', col' if y.ndim == 4 else ''}) = {first}: got {y[first]!r}, reference {r[first]!r}")
    if mode == "onehot":
        tg = ins["target"]
        sums, asum = onehot_precondition(ins, ref)
        if "o" in got:
            want = ins["v"][:, :, tg, :]
            bad = np.asarray(got["o"], dtype=np.float64) != want
            if bad.any():
                first = tuple(int(i) for i in np.argwhere(bad)[0])
                fails.append(f"{tag}, o exact: {int(bad.sum())} of {bad.size} elements differ from v[t(i)], first (b, h, row, col) = {first}: "
                             f"got {got['o'][first]!r}, v[t] {want[first]!r} (t = {int(tg[first[2]])})")
        if "dv" in got:
            y = np.asarray(got["dv"], dtype=np.float64)
            chosen = np.zeros(y.shape[2], dtype=bool)
            chosen[tg] = True
            # a non-zero integer sum absorbs the off-target terms (each below 2^-30 |dO|) when it is rounded; a zero sum -- a key that no query
            # chose, or whose queries' dO cancel -- leaves them standing
            exact = chosen[None, None, :, None] & (sums != 0)
            bad = (y != sums) & exact if c["dtype"] == "bf16" else np.zeros(y.shape, dtype=bool)
            # (what remains of them is the off-target mass and the fp32 accumulation: P = 1 on the target is exact in bf16, nothing is rounded)
            bad |= (np.abs(y) > 2.0 ** -30 * np.abs(ins["do"]).sum(2, keepdims=True) + TAU * ref["A_dv"]) & ~exact & (sums == 0)
            if bad.any():
                first = tuple(int(i) for i in np.argwhere(bad)[0])
                fails.append(f"{tag}, dv exact: {int(bad.sum())} of {bad.size} elements differ from the integer sums, first (b, h, key, col) = "
                             f"{first}: got {y[first]!r}, sum {sums[first]!r}")
    return fails, worst


def old_norm_passes(c, ref, got):
    """the criterion of test_causal_attention_vs_oracle, max|got - ref| / max|ref| < tol (twice that for the gradients): the tensors that pass"""
    tol = 3e-2 if c["dtype"] == "bf16" else 2e-4
    ok = []
    for key in ("o", "dq", "dk", "dv"):
        if key in got:
            e = np.abs(np.asarray(got[key], dtype=np.float64) - ref[key]).max() / (np.abs(ref[key]).max() + 1e-12)
            if e < (tol if key == "o" else 2 * tol):
                ok.append(key)
    return ok


# --------------------------------------------------------------------------- #
# CPU model of the kernels' arithmetic (fp32 online softmax over key tiles; bf16 casts where the kernels cast), with mutations
# --------------------------------------------------------------------------- #
MUTATIONS = ("drop_tile", "strict_diagonal", "skip_rescale", "lse_missing_key", "swap_v_rows", "truncate_p", "next_head_k")


def model(c, ins, ref, Z=None, mut=None):
    """what a correct kernel computes, in numpy float32; ``mut`` plants one defect.  The backward is fed what ``run`` feeds it."""
    f32 = np.float32
    bf = c["dtype"] == "bf16"
    rnd = (bf16_trunc if mut == "truncate_p" else bf16_round) if bf else (lambda x: x)
    rnd_out = bf16_round if bf else (lambda x: x)
    q, k, v, do = (ins[n].astype(f32) for n in ("q", "k", "v", "do"))
    scale = f32(ins["scale"])
    B, H, S, hd = q.shape
    tile = c["tile"]
    T = lambda x: np.swapaxes(x, -1, -2)
    if mut == "next_head_k":
        k = np.roll(k, -1, axis=1) if H > 1 else np.roll(k, -1, axis=0)
    vv = v
    if mut == "swap_v_rows" and S >= 2:
        a = min(40, S - 2)
        vv = v.copy()
        vv[:, :, [a, a + 1]] = v[:, :, [a + 1, a]]
    if Z is None:
        z01, zs = np.ones((B, H, S, S), dtype=f32), f32(1.0)
    else:
        zs = f32(Z.max()) if Z.max() > 0 else f32(1.0)
        z01 = (Z > 0).astype(f32)
    qi, kj = np.arange(S)[:, None], np.arange(S)[None, :]
    allowed = (kj < qi) | ((kj == qi) & (qi == 0)) if mut == "strict_diagonal" else (kj <= qi)
    if mut == "drop_tile" and S > tile:                 # rows past the second key tile never see it (first tile when there are only two)
        lo = tile if S > 2 * tile else 0
        allowed = allowed & ~((kj >= lo) & (kj < lo + tile) & (qi >= lo + tile))
    # bf16 operands: every product is exact in fp32 and the MFMA adds them all but exactly -- the raw score is the fp64 sum rounded once
    # (a BLAS fp32 dot product rounds after every term, in an order of its own); fp32 operands: fp32 throughout
    scores = (lambda a, b: (a.astype(np.float64) @ T(b.astype(np.float64))).astype(f32) * scale) if bf else (lambda a, b: (a @ T(b)) * scale)
    # ---- forward
    m = np.full((B, H, S), -1e30, dtype=f32)
    l = np.zeros((B, H, S), dtype=f32)
    acc = np.zeros((B, H, S, hd), dtype=f32)
    l_lse = np.zeros((B, H, S), dtype=f32)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        for it, k0 in enumerate(range(0, S, tile)):
            k1 = min(k0 + tile, S)
            s = scores(q, k[:, :, k0:k1])
            s = np.where(allowed[None, None, :, k0:k1], s, f32(-1e30))
            m_new = np.maximum(m, s.max(-1))
            alpha = np.exp(m - m_new)
            p = np.exp(s - m_new[..., None]).astype(f32)
            l = l * alpha + p.sum(-1, dtype=f32)
            l_lse = l_lse * alpha + p.sum(-1, dtype=f32)
            if mut == "lse_missing_key" and it == 0:    # the sum the lse is taken from misses key 0
                l_lse = l_lse - p[..., 0]
            if not (mut == "skip_rescale" and it == 1):
                acc = acc * alpha[..., None]
            acc = acc + rnd(p * z01[:, :, :, k0:k1]) @ vv[:, :, k0:k1]
            m = m_new
        out = dict(o=rnd_out(acc * (f32(1.0) / l * zs)[..., None]), lse=m + np.log(l_lse))
        # ---- backward, fed the reference's o (rounded) and lse
        o_in = rnd_out(ref["o"].astype(f32))
        lse = ref["lse"].astype(f32)
        delta = (o_in * do).sum(-1, dtype=f32)
        s = scores(q, k)
        P = np.where(allowed[None, None], np.exp(s - lse[..., None]), f32(0.0)).astype(f32)
        dv = T(rnd(P * z01)) @ do * zs
        dp = do @ T(vv)
        ds = P * (dp * z01 * zs - delta[..., None]) * scale
        dsr = rnd_out(ds) if mut != "truncate_p" else rnd(ds)
        out.update(delta=delta, dv=rnd_out(dv), dq=rnd_out(dsr @ k), dk=rnd_out(T(dsr) @ q))
    return out


# --------------------------------------------------------------------------- #
# GPU: the raw entries, the way _CausalAttention calls them
# --------------------------------------------------------------------------- #
def run(c, mode):
    """-> (ins, ref, got, kernels): got = o, lse (+ delta, dq, dk, dv) as float64 [B,H,S,(hd)]; kernels = (forward, backward or None) as
    ops.last_kernel() named them.  Buffers are NaN-filled first: an element no kernel wrote, or padding a kernel read, shows."""
    import ctypes as C
    import torch
    import mas_hip
    from mas_hip import ops
    dev = torch.device("cuda:0")
    L = mas_hip.lib()
    B, H, S, hd = c["B"], c["H"], c["S"], c["hd"]
    d = H * hd
    tdt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
    mdt = mas_hip.BF16 if c["dtype"] == "bf16" else mas_hip.F32
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ins = make_inputs(c, mode)
    pack = lambda x: torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1, 3).reshape(B, S, d))).to(tdt)      # exact: x is representable
    unpack = lambda t: t.double().cpu().numpy().reshape(B, S, H, hd).transpose(0, 2, 1, 3)
    nan = float("nan")

    keep, seed = None, None
    if c["p"]:
        seed = torch.tensor(list(DROP_SEED), dtype=torch.int64, device=dev)
        kd = torch.zeros((B, H, S, S), dtype=torch.uint8, device=dev)
        mas_hip.check(L.mas_attn_dropout_mask(ptr(seed), B, H, S, float(c["p"]), ptr(kd), ops._stream()), "attn_dropout_mask")
        keep = kd.cpu().numpy()
    ref = reference(ins, drop_z(c, keep))

    # ---- forward
    fused = torch.cat([pack(ins[n]) for n in ("q", "k", "v")], dim=-1).contiguous().to(dev)
    if c["layout"] == "fused":
        esz = fused.element_size()
        qp, kp, vp = (C.c_void_p(fused.data_ptr() + i * d * esz) for i in range(3))
        lds, bss = (3 * d,) * 3, (S * 3 * d,) * 3
        hold = [fused]
    else:
        pad = (4, 12, 20) if c["layout"] == "sep68" else (8, 16, 24)
        lds = tuple(d + x for x in pad)
        bss = tuple(S * ld + x for ld, x in zip(lds, pad))
        assert all((ld % 8 == 0) == (c["layout"] == "sep_al") for ld in lds)
        hold = []
        for n, ld, bs in zip(("q", "k", "v"), lds, bss):
            buf = torch.full((B * bs,), nan, dtype=tdt, device=dev)
            buf.as_strided((B, S, d), (bs, ld, 1)).copy_(pack(ins[n]).to(dev))
            hold.append(buf)
        qp, kp, vp = (ptr(t) for t in hold)
    o = torch.full((B, S, d), nan, dtype=tdt, device=dev)
    lse = torch.full((B, H, S), nan, dtype=torch.float32, device=dev)
    scale = float(ins["scale"])
    if c["p"]:
        mas_hip.check(L.mas_attn_causal_fwd_drop(qp, kp, vp, ptr(o), ptr(lse), mdt, B, H, S, hd, lds[0], lds[1], lds[2], bss[0], bss[1], bss[2],
                                                 scale, float(c["p"]), ptr(seed), ops._stream()), "attn_causal_fwd_drop")
    else:
        mas_hip.check(L.mas_attn_causal_fwd(qp, kp, vp, ptr(o), ptr(lse), mdt, B, H, S, hd, lds[0], lds[1], lds[2], bss[0], bss[1], bss[2],
                                            scale, ops._stream()), "attn_causal_fwd")
    k_fwd = ops.last_kernel()
    torch.cuda.synchronize()
    got = dict(o=unpack(o), lse=lse.double().cpu().numpy())
    if c["bwd_layout"] is None:
        return ins, ref, got, (k_fwd, None)

    # ---- backward on the fused layout, fed the reference's o and lse
    n3 = B * S * 3 * d
    off = 8 // fused.element_size() if c["bwd_layout"] == "fused_off8" else 0
    xbuf = torch.full((n3 + off,), nan, dtype=tdt, device=dev)
    gbuf = torch.full((n3 + off,), nan, dtype=tdt, device=dev)
    x, dx = xbuf[off:].view(B, S, 3 * d), gbuf[off:].view(B, S, 3 * d)
    x.copy_(fused)
    assert x.data_ptr() % 16 == (8 if off else 0) and dx.data_ptr() % 16 == (8 if off else 0)
    o_in = pack(ref["o"]).contiguous().to(dev)
    g = pack(ins["do"]).contiguous().to(dev)
    lse_in = torch.from_numpy(ref["lse"].astype(np.float32)).to(dev)
    delta = torch.full((B, H, S), nan, dtype=torch.float32, device=dev)
    if c["p"]:
        mas_hip.check(L.mas_attn_causal_bwd_drop(ptr(x), ptr(o_in), ptr(g), ptr(lse_in), ptr(delta), ptr(dx), mdt, B, H, S, hd, scale,
                                                 float(c["p"]), ptr(seed), ops._stream()), "attn_causal_bwd_drop")
    else:
        mas_hip.check(L.mas_attn_causal_bwd(ptr(x), ptr(o_in), ptr(g), ptr(lse_in), ptr(delta), ptr(dx), mdt, B, H, S, hd, scale,
                                            ops._stream()), "attn_causal_bwd")
    k_bwd = ops.last_kernel()
    torch.cuda.synchronize()
    dq, dk, dv = (unpack(t.contiguous()) for t in torch.split(dx, d, dim=-1))
    got.update(delta=delta.double().cpu().numpy(), dq=dq, dk=dk, dv=dv)
    del hold
    return ins, ref, got, (k_fwd, k_bwd)
