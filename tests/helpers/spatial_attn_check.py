"""The spatial self-attention core of AttnBlock (make-a-scene_amd/csrc/spatial_attn.hip, S <= 256: "shipped"; spatial_attn_flash.hip,
online softmax over 256-key chunks: "flash"; both on spatial_attn_core.h) judged element by element: cases, input builders, the fp64
reference, the bounds, a CPU model of each kernel set's arithmetic with its mutations, and ``run`` (GPU only: the raw entries through
``mas_hip.lib()``).  Importing this file needs neither a GPU nor the library.  tests/test_spatial_attn_elementwise_cpu.py shows that the
bounds have teeth, tests/test_gpu_spatial_attn_elementwise.py judges the kernels.  The pieces shared with the causal suite (bf16_round,
bf16_trunc, codes, U, TAU, FLOOR) come from tests/helpers/attn_rowwise_check.py.

Layout is [N, S, C] float64 throughout (lse, delta: [N, S]); one head, no mask.

Reference (``reference``; the plain formula on exactly the bf16 operands handed to the kernel):
  s = scale q k^T, scale = float32(C^-1/2);  lse = logsumexp(s), P = exp(s - lse), o = P v;  dP = dO v^T, D = rowsum(P o dP), dV = P^T dO,
  dS = P o (dP - D) scale, dQ = dS k, dK = dS^T q.
Magnitudes, the same formulas on absolute values:  A_o = P|v|, A_dP = |dO||v|^T, A_dV = P^T|dO|, A_dS = P o (|dP| + |D|) scale,
  A_dQ = A_dS|k|, A_dK = A_dS^T|q|;  what delta's own error carries into dS:  AD_dS = P o A_D scale, AD_dQ = AD_dS|k|, AD_dK = AD_dS^T|q|.
  A_D differs per kernel set, because the two compute delta differently:
    shipped  A_D = rowsum(P o A_dP): spatial_attn_bwd_kernel<false> sums P dP over the keys in fp32, ``part += pv[ti][r] * dp[ti][r]``;
    flash    A_D = rowsum(|dO| o |o|): spatial_attn_flash_bwd_dq_kernel sums dO o over the channels of the bf16 ``out`` it is handed,
             ``part += (float)a[e] * (float)b[e]``.

What the backward is fed.  ``run`` hands the backward entries the REFERENCE's lse rounded to fp32 and (flash) the reference's o rounded to
bf16, not the forward kernel's outputs: each direction is judged on its own arithmetic.  The chain forward -> backward is what
tests/test_gpu_spatial_attn.py and tests/test_gpu_spatial_attn_flash.py run.

Bounds, U = 2^-8 (half a bf16 ulp), TAU = 2^-18 (fp32 MFMA accumulation), every element:
  |y - r| <= FLOOR + U |r| + c U A + TAU A  (+ the delta term on AD for dQ, dK);  c = the bf16 casts on the element's path, U |r| = the
  store in sp_store, ``bf16x4 o = {(bf16_t)acc[i][4 * q], ...}``.  The counts (CASTS), from the sources:
  shipped (spatial_attn.hip)
    o      c = 1: the NORMALISED P, ``sc[ti][r] *= inv``, is cast by sp_put_rows, ``const bf16x4 o = {(bf16_t)v[ti][4 * q], ...}``; the
                  sum and 1 / sum stay fp32.
    dV     c = 1: P = __expf(s scale - lse), fp32, cast by ``if constexpr (KEYS) sp_put_rows(smem + L.o_p, L.SP, pv, ...)``.
    dQ, dK c = 1: ``dp[ti][r] = p.scale * pv[ti][r] * (dp[ti][r] - d)`` is built from the fp32 pv (the cast P feeds dV only) and cast once,
                  ``sp_put_rows(smem + L.o_p2, L.SP, dp, ...)``.
    delta  fp32, no cast anywhere: K_DELTA TAU A_D, K_DELTA measured; it enters dS with that error: K_DELTA TAU AD for dQ, dK.
  flash (spatial_attn_flash.hip)
    o      c = 1: the UNNORMALISED ``const float e = ... __expf(sc[ti][r] * p.scale - mn)`` is cast by ``sp_put_rows(smem + L.o_p, L.SP,
                  sc, ch.Sc, ...)``; l, alpha (``acc[i][r] *= alpha``) and ``inv = 1.0f / l`` stay fp32.
    dV     c = 1: ``sp_put_rows(smem + L.o_p, L.SP, pv, ch.Sc, mt, g, l31)`` in the dK/dV kernel.
    dQ     c = 1: ``dp[ti][r] = p.scale * pv[ti][r] * (dp[ti][r] - drow)`` from the fp32 pv, cast once by sp_put_rows.
    dK     c = 2: ``dp[ti][r] = p.scale * pb[ti][r] * (dp[ti][r] - dq)`` is built from pb, the P that sf_get_rows reads back from LDS
                  ALREADY ROUNDED to bf16 (``v[ti][4 * q + e] = mt < n_mt ? (float)o[e] : 0.0f``), and is cast again by sp_put_rows.
    delta  fp32 output over the already rounded o: U A_D + TAU A_D; (U + TAU) AD for dQ, dK (as in the causal suite).
  lse (fp32 in both):  |lse - r| <= K_LSE 2^-23 max(1, |lse|, max|s| of the row), one K_LSE per forward kernel.
K_DELTA and K_LSE cover __expf, __logf and the summation order and are MEASURED on an MI355X (the worst value seen, doubled, then the next
power of two above; figures in tests/test_gpu_spatial_attn_elementwise.py).

Operand modes (``make_inputs``):
  gauss       randn rounded to bf16: q, k, v times 1.5 (the scale of the norm tests), dO times 1.
  gauss_flat  the same with q times 0.05: the flat softmax of an untrained block.
  hard        gauss (q and k of unit scale) + a planted score structure: the first b = ceil(log2 S) channels of k carry the +-1 bit code
              of the key index, those of q a * (bit code of the target key t(i)), a = round(60 / (scale b)): about +60 at the target, -60
              at its complement (the complement of key S - 1 is always a key), 60 - 120 h / b at Hamming distance h (b <= 10: steps of
              12 or more).  t(i) follows ``target`` (N_RULES rules, cycling with period 13 over the rows: 2 rows in 13 keep their gauss
              q).  Blocks walk the chunks from different starts, so between the rules every block sees its maximum rise at a later chunk
              and sees later chunks vanish.
  onehot      k_j = a +-1 code of key j over ALL channels (pairwise Hamming distance >= DMIN[C]), q_i = c * code(t(i)), v and dO integers
              in +-{1..4}; every image draws its own key permutation of the code book, so a block that reads another image's K or V gets
              foreign codes.  ``onehot_precondition`` asserts on the reference alone: off-target mass times max|v| < 2^-30, every per-key
              integer sum of dO <= 256.  Then BITWISE o[i] == v[t(i)] and dV[j] == the integer sum of dO over {i: t(i) = j} wherever that
              sum is non-zero; zero sums are held to 2^-30 sum|dO| + TAU A_dV; lse[i] is the target's score under the lse bound.
  uniform     q = 0, integer v and dO: P = 1 / S, lse = log S.  The mode that catches a dropped key under a flat softmax.  Tight check on o:
              flash, every S: |o - r| <= U |r| + 2^-22 |r| (the unnormalised P is exactly 1, the fp32 sums of integers are exact, 1 / l and
              the product round once each); shipped, S a power of two: o == bf16(mean v) bitwise (bf16(1 / S) is exact).
"""
import zlib

import numpy as np

import attn_rowwise_check as ARC
from attn_rowwise_check import bf16_round, bf16_trunc, codes, U, TAU, FLOOR

# measured coefficients (procedure and figures: tests/test_gpu_spatial_attn_elementwise.py)
K_DELTA = 4.0
FWD_S, BWD_S = "spatial_attn_fwd", "spatial_attn_bwd(dkv)"
FWD_F, BWD_F = "spatial_attn_flash_fwd", "spatial_attn_flash_bwd(dkv)"
K_LSE = {FWD_S: 16.0, FWD_F: 16.0}
CASTS = {"shipped": dict(o=1, dv=1, dq=1, dk=1), "flash": dict(o=1, dv=1, dq=1, dk=2)}

GAP = 32.0
N_RULES = 11
KC = 256                                        # keys per chunk (spatial_attn_flash.hip), the whole problem of spatial_attn.hip
NW = 8                                          # waves per work-group = 32-column tiles a chunk can hold
MODES = ("gauss", "gauss_flat", "hard", "onehot", "uniform")
LAUNCH = {"shipped": (FWD_S, BWD_S), "flash": (FWD_F, BWD_F)}
FAMILIES = ("shipped_fwd", "shipped_bwd", "flash_fwd", "flash_bwd")


# --------------------------------------------------------------------------- #
# cases
# --------------------------------------------------------------------------- #
def _case(kset, S, C, N=2):
    return dict(name=f"{kset}-N{N}S{S}C{C}", kset=kset, N=N, S=S, C=C, modes=MODES)


def _cases():
    c = []
    # shipped kernel: every edge of the 32-token tile and of the 8-wave work-group at C = 64; N * ceil(S / 32) a multiple of 8 at
    # S = 128, 255, 256 (the XCD remap taken), not at the others
    c += [_case("shipped", S, 64) for S in (1, 16, 31, 32, 33, 35, 64, 81, 128, 129, 255, 256)]
    c += [_case("shipped", 33, 64, N=8), _case("shipped", 200, 64, N=3)]      # 16 blocks: remap with a ragged tile; 21: gr = 3 without it
    # 1..4 channel groups, groups partly full (sp_rows_zero_pad, the clamped C - 16 fragment)
    c += [_case("shipped", S, C) for C in (32, 96, 160, 384, 512) for S in (33, 129, 256)]
    # chunked kernel: one chunk (the direct entry), two, three and four; the last chunk of one key or ragged
    c += [_case("flash", S, 64) for S in (1, 33, 256, 257, 288, 400, 512, 513, 600, 769)]
    c += [_case("flash", 600, 64, N=8)]                                       # 152 blocks: the remap taken beyond one chunk
    c += [_case("flash", S, C) for C in (32, 160) for S in (33, 288, 600)]
    c += [_case("flash", 288, 384), _case("flash", 257, 512), _case("flash", 513, 512)]
    return c


CASES = _cases()


def chunks(S):
    """[(first key, keys)] of the 256-key chunks"""
    return [(c0, min(KC, S - c0)) for c0 in range(0, S, KC)]


def features(c):
    """what a case exercises in the launches that serve it (both directions run the same grid, tiles and chunk walk)"""
    N, S, C = c["N"], c["S"], c["C"]
    nb = -(-S // 32)
    f = {"groups%d" % (-(-C // 128)), "remap" if (N * nb) % 8 == 0 else "no_remap"}
    f |= {"gr%d" % ((rot >> 1) & 3) for rot in range(nb)}
    if S % 32:
        f.add("ragged")
    if S < 32:
        f.add("sub_tile")
    if any(-(-sc // 32) < NW for _, sc in chunks(S)):
        f.add("idle_waves")
    if C % 128:
        f.add("c_pad")
    if c["kset"] == "flash":
        ch = chunks(S)
        f.add("chunks%s" % (len(ch) if len(ch) < 3 else "3plus"))
        if len(ch) > 1 and ch[-1][1] == 1:
            f.add("last_chunk_one_key")
        if any(rot % len(ch) for rot in range(nb)):
            f.add("chunk_start_rotated")
        ntl = -(-ch[-1][1] // 32)
        if len(ch) > 1 and ch[-1][1] % 32 and any(rot % ntl for rot in range(nb)):
            f.add("rt_ragged_last")                                       # rt = rot % tiles-in-chunk non-zero in a ragged last chunk
    return f


_COMMON = {"ragged", "sub_tile", "idle_waves", "c_pad", "groups1", "groups2", "groups3", "groups4", "remap", "no_remap", "gr0", "gr1", "gr2", "gr3"}
_CHUNKED = {"chunks1", "chunks2", "chunks3plus", "last_chunk_one_key", "chunk_start_rotated", "rt_ragged_last"}
REQUIRED = {FWD_S: _COMMON, BWD_S: _COMMON, FWD_F: _COMMON | _CHUNKED, BWD_F: _COMMON | _CHUNKED}


def reached(cases_and_kernels):
    """[(case, launch name)] -> {launch name: features}"""
    got = {}
    for c, k in cases_and_kernels:
        got.setdefault(k, set()).update(features(c))
    return got


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def target(i, rule, S):
    """the key that holds query i's maximum.  Rules: 0 key 0; 1 key S - 1 (the last key of the last chunk); 2 the diagonal; 3 / 4 the
    first / last key of the row's own 32-tile; 5 the first key of the (ragged) last tile; 6 / 7 keys 255 / 256; 8 the first key of the
    last chunk; 9 (i + S / 2) mod S; 10 the key before the last chunk.  Clipped to [0, S - 1]."""
    c0 = ((S - 1) // KC) * KC
    t = (0, S - 1, i, (i // 32) * 32, (i // 32) * 32 + 31, ((S - 1) // 32) * 32, 255, 256, c0, (i + S // 2) % S, c0 - 1)[rule]
    return min(max(t, 0), S - 1)


def targets(S, cycle):
    """rule of row i = i mod cycle (odd, so every rule meets every lane of a wave); rules >= N_RULES mean 'no target' (-1)"""
    return np.array([target(i, i % cycle, S) if i % cycle < N_RULES else -1 for i in range(S)], dtype=np.int64)


def plant_bits(S):
    """the bits that tell S keys apart: with no more than these, the complement of key S - 1 (a target of every case) is a key too"""
    return max(1, int(S - 1).bit_length())


def _ints(rs, shape):
    return (rs.randint(1, 5, size=shape) * (rs.randint(0, 2, size=shape) * 2 - 1)).astype(np.float64)


def make_inputs(c, mode):
    N, S, C = c["N"], c["S"], c["C"]
    rs = np.random.RandomState(zlib.crc32((c["name"] + mode).encode()) & 0x7FFFFFFF)
    scale = float(np.float32(C ** -0.5))
    shape = (N, S, C)
    rnd = lambda x: bf16_round(x).astype(np.float64)
    g = [rs.randn(*shape) for _ in range(4)]
    # (hard: unit q and k, so that the unplanted channels move a score by about 1 and the planted key keeps the maximum)
    fq, fk = {"gauss_flat": (0.05, 1.5), "hard": (1.0, 1.0)}.get(mode, (1.5, 1.5))
    q, k, v, do = rnd(g[0] * fq), rnd(g[1] * fk), rnd(g[2] * 1.5), rnd(g[3])
    tg = None
    if mode == "hard":
        nbits = plant_bits(S)
        a = float(bf16_round(np.array([round(60.0 / (scale * nbits))]))[0])
        tg = targets(S, 13)
        bits = ((np.arange(S)[:, None] >> np.arange(nbits)[None, :]) & 1) * 2.0 - 1.0             # [S, nbits]
        k[..., :nbits] = bits
        rows = tg >= 0
        q[:, rows, :nbits] = a * bits[tg[rows]]
    elif mode == "onehot":
        tg = targets(S, N_RULES)
        book = codes(C, max(S, 2))
        k, q = np.empty(shape), np.empty(shape)
        for n in range(N):
            kc = book[rs.permutation(len(book))[:S]].astype(np.float64)
            k[n], q[n] = kc, kc[tg]
        q *= float(np.ceil(GAP / (scale * 2 * ARC.DMIN[C])))
        v, do = _ints(rs, shape), _ints(rs, shape)
    elif mode == "uniform":
        q = np.zeros(shape)
        v, do = _ints(rs, shape), _ints(rs, shape)
    elif mode not in ("gauss", "gauss_flat"):
        raise ValueError(mode)
    return dict(q=q, k=k, v=v, do=do, scale=scale, target=tg)


# --------------------------------------------------------------------------- #
# fp64 reference and bounds
# --------------------------------------------------------------------------- #
def reference(ins, kset):
    """everything ``judge`` needs, and nothing of size S x S (the cases are cached)"""
    q, k, v, do, scale = ins["q"], ins["k"], ins["v"], ins["do"], ins["scale"]
    S = q.shape[1]
    T = lambda x: np.swapaxes(x, -1, -2)
    s = scale * (q @ T(k))
    mx = s.max(-1, keepdims=True)
    lse = mx[..., 0] + np.log(np.exp(s - mx).sum(-1))
    P = np.exp(s - lse[..., None])
    o, A_o = P @ v, P @ np.abs(v)
    dP, A_dP = do @ T(v), np.abs(do) @ T(np.abs(v))
    D = (P * dP).sum(-1)
    A_D = (P * A_dP).sum(-1) if kset == "shipped" else (np.abs(do) * np.abs(o)).sum(-1)
    dS = P * (dP - D[..., None]) * scale
    A_dS = P * (np.abs(dP) + np.abs(D)[..., None]) * scale
    AD_dS = P * A_D[..., None] * scale
    ref = dict(lse=lse, smax=np.abs(s).max(-1), o=o, A_o=A_o, delta=D, A_delta=A_D, dv=T(P) @ do, A_dv=T(P) @ np.abs(do),
               dq=dS @ k, dk=T(dS) @ q, A_dq=A_dS @ np.abs(k), A_dk=T(A_dS) @ np.abs(q), AD_dq=AD_dS @ np.abs(k), AD_dk=T(AD_dS) @ np.abs(q),
               smin=s.min(), argmax=s.argmax(-1))
    tg = ins["target"]
    if tg is not None:
        rows = np.nonzero(tg >= 0)[0]
        ref["s_target"] = s[:, rows, tg[rows]]
        ref["p_target"] = P[:, rows, tg[rows]]
        if len(rows) == S:                          # onehot: the off-target mass and the second-largest probability
            P2 = P.copy()
            P2[:, np.arange(S), tg] = 0.0
            ref["off_mass"], ref["p_second"] = P2.sum(-1), P2.max(-1)
    return ref


def bound(ref, key, kset):
    r = ref[key]
    if key == "lse":
        return K_LSE[LAUNCH[kset][0]] * 2.0 ** -23 * np.maximum(1.0, np.maximum(np.abs(r), ref["smax"]))
    A = ref["A_" + key]
    d_err = K_DELTA * TAU if kset == "shipped" else U + TAU
    if key == "delta":
        return FLOOR + d_err * A
    AD = ref["AD_" + key] if key in ("dq", "dk") else 0.0
    return FLOOR + U * np.abs(r) + CASTS[kset][key] * U * A + TAU * A + d_err * AD


def onehot_precondition(ins, ref):
    """asserted on the reference alone, before any kernel output is looked at"""
    tg, v, do = ins["target"], ins["v"], ins["do"]
    assert (ref["off_mass"] * np.abs(v).max() < 2.0 ** -30).all(), float(ref["off_mass"].max())
    assert (ref["p_second"] < 2.0 ** -30).all()
    sums, asum = np.zeros_like(do), np.zeros_like(do)
    np.add.at(sums, (slice(None), tg), do)
    np.add.at(asum, (slice(None), tg), np.abs(do))
    assert (np.abs(sums) <= 256).all()                  # integers up to 256 are exact in bf16
    return sums, asum


def uniform_o_check(c, ins, ref, y):
    """the tight check of the uniform mode -> (bad mask or None when only the general bound applies, what it was held to)"""
    S = c["S"]
    if c["kset"] == "flash":
        r = ins["v"].sum(1, keepdims=True) / S      # (the integer sum is exact: a zero mean is 0 here, not the 1e-17 of exp(-log S))
        return ~(np.abs(y - r) <= (U + 2.0 ** -22) * np.abs(r)), "U |r| + 2^-22 |r|"
    if S & (S - 1) == 0:
        return y != bf16_round(ins["v"].sum(1, keepdims=True) / S).astype(np.float64), "bf16(mean v), bitwise"
    return None, ""


def judge(c, mode, ins, ref, got):
    """-> (failures: [str], worst: {tensor: ratio}).  got: the tensors a kernel (or the model) produced, any subset of
    o, lse, delta, dq, dk, dv."""
    fails, worst = [], {}
    tag = f"{c['name']} {mode}"

    def first_bad(bad, what, y, r, extra=""):
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        fails.append(f"{tag}, {what}: {int(bad.sum())} of {bad.size} elements outside{extra}, first bad (image, row{', channel' if y.ndim == 3 else ''})"
                     f" = {first}: got {y[first]!r}, reference {r[first]!r}")

    for key in ("o", "lse", "delta", "dv", "dq", "dk"):
        if key not in got:
            continue
        y, r = np.asarray(got[key], dtype=np.float64), ref[key]
        assert y.shape == r.shape, (tag, key, y.shape, r.shape)
        bd = bound(ref, key, c["kset"])
        err = np.abs(y - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bd > 0, err / bd, np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(y), ratio, np.inf)
        worst[key] = float(ratio.max())
        bad = ~(err <= bd) | ~np.isfinite(y)
        if bad.any():
            first_bad(bad, key, y, r, f", worst ratio {worst[key]:.3g}")
    if mode == "uniform" and "o" in got:
        y = np.asarray(got["o"], dtype=np.float64)
        bad, what = uniform_o_check(c, ins, ref, y)
        if bad is not None and bad.any():
            first_bad(np.broadcast_to(bad, y.shape), f"o tight ({what})", y, ref["o"])
    if mode == "onehot":
        tg = ins["target"]
        sums, asum = onehot_precondition(ins, ref)
        if "o" in got:
            y, want = np.asarray(got["o"], dtype=np.float64), ins["v"][:, tg, :]
            bad = y != want
            if bad.any():
                first_bad(bad, "o exact (v[t(i)])", y, want)
        if "lse" in got:
            y = np.asarray(got["lse"], dtype=np.float64)
            bad = ~(np.abs(y - ref["s_target"]) <= bound(ref, "lse", c["kset"]))
            if bad.any():
                first_bad(bad, "lse vs the target's score", y, ref["s_target"])
        if "dv" in got:
            y = np.asarray(got["dv"], dtype=np.float64)
            chosen = np.zeros(y.shape[1], dtype=bool)
            chosen[tg] = True
            # a non-zero integer sum absorbs the off-target terms (each below 2^-30 |dO|) when it is rounded; a zero sum -- a key that no
            # query chose, or whose queries' dO cancel -- leaves them standing
            exact = chosen[None, :, None] & (sums != 0)
            bad = (y != sums) & exact
            bad |= (np.abs(y) > 2.0 ** -30 * np.abs(ins["do"]).sum(1, keepdims=True) + TAU * ref["A_dv"]) & ~exact & (sums == 0)
            if bad.any():
                first_bad(bad, "dv exact (integer sums of dO)", y, sums)
    return fails, worst


def old_norm_passes(ref, got):
    """the criterion of test_spatial_attention_fwd_bwd_vs_torch on what ``got`` holds: relmax < 2e-2 and rel-L2 < 1e-2 on o, rel-L2 < 2e-2
    and relmax < 4e-2 on the gradient of the fused q|k|v"""
    def norms(y, r):
        return np.abs(y - r).max() / max(np.abs(r).max(), 1e-12), np.linalg.norm(y - r) / max(np.linalg.norm(r), 1e-12)
    ok = True
    if "o" in got:
        mx, l2 = norms(np.asarray(got["o"], dtype=np.float64), ref["o"])
        ok &= bool(mx < 2e-2 and l2 < 1e-2)
    if "dq" in got:
        mx, l2 = norms(np.concatenate([np.asarray(got[k], dtype=np.float64) for k in ("dq", "dk", "dv")], -1),
                       np.concatenate([ref[k] for k in ("dq", "dk", "dv")], -1))
        ok &= bool(mx < 4e-2 and l2 < 2e-2)
    return ok


# --------------------------------------------------------------------------- #
# CPU models of the two kernel sets' arithmetic (numpy float32; bf16 casts where the kernels cast), with mutations
# --------------------------------------------------------------------------- #
MUTATIONS = ("drop_key_last", "drop_tile_some_rows", "skip_rescale", "chunk_twice", "lse_missing_key", "swap_v_rows", "truncate_p",
             "delta_neighbour_row", "next_image_k", "stale_channel_tile")
FLASH_ONLY = ("skip_rescale", "chunk_twice")


def model(c, ins, ref, mut=None):
    """what a correct kernel of c's set computes, in numpy float32; ``mut`` plants one defect.  The backward is fed what ``run`` feeds it."""
    f32, f64 = np.float32, np.float64
    flash = c["kset"] == "flash"
    assert mut is None or mut in MUTATIONS and (flash or mut not in FLASH_ONLY)
    rnd = bf16_trunc if mut == "truncate_p" else bf16_round
    q, k, v, do = (ins[n].astype(f32) for n in ("q", "k", "v", "do"))
    scale = f32(ins["scale"])
    N, S, C = q.shape
    T = lambda x: np.swapaxes(x, -1, -2)
    # bf16 operands: every product is exact in fp32 and the MFMA adds them all but exactly -- a product is the fp64 sum rounded once
    mm = lambda a, b: (a.astype(f64) @ b.astype(f64)).astype(f32)
    if mut == "next_image_k":
        k = np.roll(k, -1, axis=0)
    vv = v
    if mut == "swap_v_rows" and S >= 2:
        a = min(40, S - 2)
        vv = v.copy()
        vv[:, [a, a + 1]] = v[:, [a + 1, a]]
    seen = np.ones((S, S), dtype=bool)              # [query, key]: the keys a query's block multiplies
    if mut == "drop_key_last" and S > 1:
        seen[:, S - 1] = False
    if mut == "drop_tile_some_rows" and S > 32:     # the second half of the query blocks never sees the second key tile
        seen[(np.arange(S) // 32 >= -(-S // 32) // 2)[:, None] & ((np.arange(S) // 32) == 1)[None, :]] = False
    ch = chunks(S) if flash else [(0, S)]
    nch = len(ch)
    start = (np.arange(S) // 32) % nch              # the chunk a row's block starts its walk on (rot % nch)

    def walk(st):
        if mut == "chunk_twice":                    # the walk does not wrap: it stays on the last chunk and never sees the first ones
            return [min(i + st, nch - 1) for i in range(nch)]
        return [(i + st) % nch for i in range(nch)]

    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        s = mm(q, T(k)) * scale
        neg = f32(-1e30)
        # ---- forward
        o, lse = np.empty((N, S, C), dtype=f32), np.empty((N, S), dtype=f32)
        for st in range(nch):
            rows = np.nonzero(start == st)[0]
            if not len(rows):
                continue
            m = np.full((N, len(rows)), neg, dtype=f32)
            l = np.zeros((N, len(rows)), dtype=f32)
            l_lse = np.zeros((N, len(rows)), dtype=f32)
            acc = np.zeros((N, len(rows), C), dtype=f32)
            for it, ci in enumerate(walk(st)):
                c0, sc = ch[ci]
                ok = seen[rows, c0:c0 + sc][None]
                sch = np.where(ok, s[:, rows, c0:c0 + sc], neg)
                mn = np.maximum(m, sch.max(-1))
                alpha = np.exp(m - mn)
                e = np.where(ok, np.exp(sch - mn[..., None]), f32(0.0)).astype(f32)
                l = l * alpha + e.sum(-1, dtype=f32)
                e_lse = e.copy()
                if mut == "lse_missing_key" and c0 == 0:
                    e_lse[..., 0] = 0.0             # the sum the lse is taken from misses key 0
                l_lse = l_lse * alpha + e_lse.sum(-1, dtype=f32)
                if not (mut == "skip_rescale" and it == 1):
                    acc = acc * alpha[..., None]
                if flash:
                    acc = acc + mm(rnd(e), vv[:, c0:c0 + sc])
                else:                               # one chunk: the normalised P is what is cast
                    acc = mm(rnd(e * (f32(1.0) / l)[..., None]), vv)
                m = mn
            o[:, rows] = acc * (f32(1.0) / l)[..., None] if flash else acc
            lse[:, rows] = m + np.log(l_lse)
        out = dict(o=bf16_round(o), lse=lse)
        # ---- backward, fed the reference's lse (and, flash, its o rounded to bf16)
        lse_in = ref["lse"].astype(f32)
        qseen = seen.copy()                         # what a block multiplies of the other side: by query block (dQ) ...
        if mut == "chunk_twice":
            for st in range(nch):
                gone = sorted(set(range(nch)) - set(walk(st)))
                for ci in gone:
                    qseen[np.ix_(start == st, np.arange(ch[ci][0], ch[ci][0] + ch[ci][1]))] = False
        kseen = T(qseen) if mut == "chunk_twice" else qseen       # ... and by key block (dK / dV; its chunks are chunks of queries)
        P = np.exp(s - lse_in[..., None]).astype(f32)
        dp = mm(do, T(vv))
        if flash:
            delta = (do * bf16_round(ref["o"].astype(f32))).sum(-1, dtype=f32)
        else:
            delta = (np.where(qseen[None], P, f32(0.0)) * dp).sum(-1, dtype=f32)
        Pq = np.where(qseen[None], P, f32(0.0))
        dsq = rnd(scale * Pq * (dp - delta[..., None]))
        Pk = np.where(kseen[None], P, f32(0.0))
        dk_delta = np.concatenate([delta[:, 1:], delta[:, -1:]], 1) if mut == "delta_neighbour_row" else delta
        Pb = rnd(Pk)
        dsk = rnd(scale * (Pb if flash else Pk) * (dp - dk_delta[..., None]))
        out.update(delta=delta, dq=bf16_round(mm(dsq, k)), dv=bf16_round(mm(T(Pb), do)), dk=bf16_round(mm(T(dsk), q)))
    if mut == "stale_channel_tile":
        # a channel tile past C written instead of dropped: it lands on the next row's first tile (out: row stride C) and, from dV at
        # the end of a fused row, on the next row's dQ
        out["o"] = out["o"].copy()
        out["o"][:, 1:, :32] = out["o"][:, :-1, C - 32:].copy()
        out["dq"][:, 1:, :32] = out["dv"][:, :-1, C - 32:]
    return out


# --------------------------------------------------------------------------- #
# GPU: the raw entries, the way _SpatialAttention / _SpatialAttentionFlash call them
# --------------------------------------------------------------------------- #
GUARD_BYTES = 8192


def run(c, ins, ref, part):
    """part "fwd" -> o, lse; "bwd" -> delta, dq, dk, dv (float64), fed the reference's lse / o.  -> (got, raw, launch name, failures).
    Every output lives inside a larger NaN-filled allocation with GUARD_BYTES of sentinel on each side: after the call every element
    inside must be finite (``judge``) and every guard byte unchanged (failures).  Inputs sit at the very start of their own allocations.
    raw: the outputs' bits, for the determinism test."""
    import ctypes as C_
    import torch
    import mas_hip
    from mas_hip import ops
    dev = torch.device("cuda:0")
    L = mas_hip.lib()
    N, S, C = c["N"], c["S"], c["C"]
    flash = c["kset"] == "flash"
    ptr = lambda t: C_.c_void_p(t.data_ptr())
    bf = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16)                 # exact: x is representable
    holds = []

    def guarded(shape, dtype):
        esz = torch.empty((), dtype=dtype).element_size()
        g, n = GUARD_BYTES // esz, int(np.prod(shape))
        buf = torch.full((g + n + g,), float("nan"), dtype=dtype, device=dev)
        holds.append((buf, g, n))
        return buf[g:g + n].view(shape)

    def guard_failures(tag):
        out = []
        for buf, g, n in holds:
            bits = buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32)
            nanbits = torch.full((1,), float("nan"), dtype=buf.dtype).view(bits.dtype).item()
            for side, part_ in (("before", bits[:g]), ("after", bits[g + n:])):
                bad = (part_ != nanbits).nonzero()
                if len(bad):
                    out.append(f"{tag}: {len(bad)} guard elements {side} a {tuple(buf.shape)} {buf.dtype} output were written, first at {int(bad[0])}")
        return out

    x = torch.cat([bf(ins[n]) for n in ("q", "k", "v")], dim=-1).contiguous().to(dev)
    if part == "fwd":
        o, lse = guarded((N, S, C), torch.bfloat16), guarded((N, S), torch.float32)
        fn = L.mas_spatial_attn_flash_fwd if flash else L.mas_spatial_attn_fwd
        mas_hip.check(fn(ptr(x), ptr(o), ptr(lse), mas_hip.BF16, N, S, C, ops._stream()), "spatial_attn fwd")
        kern = ops.last_kernel()
        torch.cuda.synchronize()
        outs = dict(o=o, lse=lse)
    else:
        g = bf(ins["do"]).contiguous().to(dev)
        lse_in = torch.from_numpy(ref["lse"].astype(np.float32)).to(dev)
        delta, dx = guarded((N, S), torch.float32), guarded((N, S, 3 * C), torch.bfloat16)
        if flash:
            o_in = bf(bf16_round(ref["o"])).contiguous().to(dev)
            mas_hip.check(L.mas_spatial_attn_flash_bwd(ptr(x), ptr(o_in), ptr(g), ptr(lse_in), ptr(delta), ptr(dx), mas_hip.BF16, N, S, C,
                                                       ops._stream()), "spatial_attn_flash_bwd")
        else:
            mas_hip.check(L.mas_spatial_attn_bwd(ptr(x), ptr(g), ptr(lse_in), ptr(delta), ptr(dx), mas_hip.BF16, N, S, C, ops._stream()),
                          "spatial_attn_bwd")
        kern = ops.last_kernel()
        torch.cuda.synchronize()
        outs = dict(delta=delta, dq=dx[..., :C], dk=dx[..., C:2 * C], dv=dx[..., 2 * C:])
    got = {k: t.double().cpu().numpy() for k, t in outs.items()}
    raw = {k: t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy() for k, t in outs.items()}
    return got, raw, kern, guard_failures(f"{c['name']} {part}")
