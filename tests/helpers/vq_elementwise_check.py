#!/usr/bin/env python3
"""GPU child of tests/test_gpu_vq_elementwise.py, and the CPU side that test and tests/test_vq_elementwise_cpu.py import.

    vq_elementwise_check.py SETTING OUT.pt

runs every case of SETTINGS[SETTING] in every operand mode through ``ops.vq_lookup`` (+ autograd, + one direct ``mas_vq_bwd`` call) and
writes every output together with ``ops.last_kernel()`` right after it.  Nothing numeric is judged there.  The CPU side: seeded operands
(``make_inputs``), fp64 references, the launch geometry restated (``geometry``: pick_ksplit, tiles_per, active and empty splits;
``ACC_ROW``: the accumulator row of (half-wave, register); ``quarters``: the codebook gradient's per = ceil(M / 4) wave ranges and their
64-wide ballots; VB_CODES = 8), an fp32 numpy model of every kernel with the split / tile / half-wave merge order written out
(``model_*``) and ``judge``.

Notation: U = 2^-24 (one fp32 rounding, relative); z [M, D] latent rows, e [K, D] codes, zz = |z|^2, ee = |e|^2, beta = 0.25.
SECOND = 1 + 2^-13 multiplies the forward bounds for the terms of second order (the longest chain is under 300 roundings, 300 U < 2^-15).

1. Distances.  The kernel forms d = fl(fl(zz + ee) - 2 dot) with
     zz, ee   row_sqnorm: a lane squares and adds ceil(D / 64) values, then 6 butterfly additions: with the square's own rounding
              |dzz| <= (ceil(D / 64) + 6 + 1) U zz, and the same for ee;
     zz + ee  one rounding: U (zz + ee);
     dot      a D-term fp32 FMA chain (v_mfma_f32_32x32x2_f32): |ddot| <= D U sum_i |z_i e_i| in any order, and it enters d twice;
     the final subtraction: U |d|.
   B(m, k) = SECOND U ((ceil(D / 64) + 8) (zz_m + ee_k) + 2 D sum_i |z_mi e_ki| + |d64(m, k)|).
   Per latent row, with d64 the fp64 distances of the same fp32 operands: ALWAYS d64[m, idx] - min_k d64[m, k] <= B(m, idx) + B(m, argmin)
   (figure "slack"); where the fp64 top-2 gap exceeds B(m, first) + B(m, second) the index must EQUAL the fp64 argmin.  Rows left to the
   first rule alone (``near_tie_rows``, from the reference alone) are at most NEAR_TIE_CAP of a *far* case and none of a *gauss* case.
2. z_q must be cb[idx] bitwise with the kernel's own idx.
3. Loss against (1 + beta) / (M D) sum (cb[idx] - z)^2 in fp64 with the kernel's idx.  vq_finalize: df = fl(e - z) (ADDED to the issue's
   list: one rounding, twice in the square), the square, a lane's ceil(D / 64) additions, 6 butterfly additions, 4 additions over the
   block's waves; vq_loss_reduce sums the blocks in fp64 and stores once; ``ops`` multiplies by the fp32-rounded constant in fp32 (2).
   Every term is positive, so the bound is relative: SECOND (ceil(D / 64) + 6 + 4 + 1 + 2 + 1 + 2) U loss.
   *int* mode: every sum is an exact integer below 2^24, only the two roundings of the scale remain: SECOND 2 U loss.
4. dz against g_zq + c (z - e), c = g_loss 2 / (M D): the rounded coefficient, the difference, the product and the sum (or one fma):
   U (|g_zq| + 3 |c (z - e)| + |dz|).
5. dcb[k, :] against sum_{m: idx = k} -c beta (z - e).  A term carries 4 roundings (the division, times beta, the difference, the
   product).  Fixed order (``default``): a wave adds its quarter's hits of code k in order into a zeroed LDS row (n_q - 1 rounded
   additions), the four rows are folded with 3 more: with L = max_q n_q + 3 the bound U ((L + 3) sum|term| + |result|) covers both.
   Atomics (``atomic``, MAS_VQ_BWD_DET=0): L = the code's total hit count, valid in any order.  A code nobody picked: exactly 0.
*int* mode: integers in [-4, 4]; every fp32 value the forward forms is an exact integer below 2^24 (asserted in ``make_inputs``), so idx
must equal np.argmin of the fp64 distances (the FIRST minimum) on every row; ties are planted (``tie_plan``): duplicate codebook rows
cb[j] = cb[i], i < j, in every relation the merge order has (TIE_RELATIONS), and latent rows equal to them (d = 0, shared by exactly
the duplicates).  Backward with M D, g_loss, beta powers of two: every term and partial sum is exact, dz and dcb bitwise the fp64 result."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -13
NT, ROWS_PER_BLOCK, CODES_PER_TILE, MAX_KSPLIT, VB_CODES = 256, 128, 32, 64, 8
WAVES = NT // 64
SENTINEL = 0x7FFFFFFF
BETA = 0.25
NEAR_TIE_CAP = 0.10
FWD_MODES = ("gauss", "far", "int")
f32, f64 = np.float32, np.float64
# accumulator row owned by (half-wave g, register r): mas_common.h acc_row
ACC_ROW = np.array([[(r & 3) + 8 * (r >> 2) + 4 * g for r in range(16)] for g in (0, 1)])


# ------------------------------------------------------------------------------------------------------- launch geometry, restated
def cdiv(a, b):
    return -(-a // b)


def pick_ksplit(m, k):
    rb, ntiles = cdiv(m, ROWS_PER_BLOCK), cdiv(k, CODES_PER_TILE)
    return max(1, min(cdiv(1024, rb), MAX_KSPLIT, ntiles))


def geometry(m, k):
    rb, ntiles = cdiv(m, ROWS_PER_BLOCK), cdiv(k, CODES_PER_TILE)
    ks = pick_ksplit(m, k)
    tiles_per = cdiv(ntiles, ks)
    active = cdiv(ntiles, tiles_per)
    return dict(rb=rb, ntiles=ntiles, ksplit=ks, tiles_per=tiles_per, active=active, empty=ks - active,
                last_codes=k - (ntiles - 1) * CODES_PER_TILE, capped=ks == cdiv(1024, rb) < min(MAX_KSPLIT, ntiles))


def split_of(code, geo):
    return code // CODES_PER_TILE // geo["tiles_per"]


def quarters(m):
    """the (lo, hi) row range of each wave of vq_bwd_codebook_kernel"""
    per = cdiv(m, WAVES)
    return [(min(m, w * per), min(m, (w + 1) * per)) for w in range(WAVES)]


def sqnorm_chain(d):
    return cdiv(d, 64) + 6


# ----------------------------------------------------------------------------------------------------------------------------- cases
def _fwd(m, k, d):
    return dict(name="f_%dx%dx%d" % (m, k, d), kind="fwd", M=m, K=k, D=d)


def _bwd(name, m, k, d, pattern, int_too=False, variants=False, direct=False):
    return dict(name=name, kind="bwd", M=m, K=k, D=d, pattern=pattern, int_too=int_too, variants=variants, direct=direct)


FWD_CASES = [_fwd(*s) for s in ((130, 2080, 32), (33, 2049, 256), (2049, 1985, 32), (161, 100, 64), (97, 161, 128), (129, 257, 256),
                                (1, 1, 32), (1, 33, 64), (3, 8, 32))]
NONFINITE = dict(name="nf_161x100x64", kind="nonfinite", M=161, K=100, D=64)
NF_ALL_NAN, NF_ONE_NAN, NF_PINF, NF_NINF = (5, 70, 160), 33, 100, 131
BWD_CASES = [
    _bwd("b_one_256_d128", 256, 45, 128, "one", int_too=True),          # chains of 64 additions into one LDS row, four waves
    _bwd("b_one_403_d256", 403, 45, 256, "one"),                        # per = 101: two ballots per wave, the last quarter short
    _bwd("b_edges_403_d128", 403, 45, 128, "edges"),
    _bwd("b_edges_403_d256", 403, 41, 256, "edges"),
    _bwd("b_edges_256_d64", 256, 45, 64, "edges", int_too=True),        # per = 64: lo + 64 is the next quarter's first row
    _bwd("b_edges_512_d32", 512, 45, 32, "edges", int_too=True),        # per = 128: two full ballots per wave, exact in int mode
    _bwd("b_ragged_k41_d32", 100, 41, 32, "ragged"),                    # K % 8 = 1: the last group is the last code alone
    _bwd("b_ragged_k45_d64", 100, 45, 64, "ragged"),                    # K % 8 = 5
    _bwd("b_small_1_d32", 1, 9, 32, "small"),                           # three waves with empty ranges
    _bwd("b_small_3_d64", 3, 13, 64, "small"),                          # one wave with an empty range
    _bwd("b_rand_147_d128", 147, 45, 128, "rand16", variants=True),     # the three argument shapes of _VQ.backward
    _bwd("b_rand_256_d32", 256, 45, 32, "rand16", int_too=True),
    _bwd("b_direct_147_d256", 147, 45, 256, "rand16", direct=True),     # mas_vq_bwd itself, dcb pre-filled
]
EDGE_GROUP = 1               # "edges": the boundary rows pick the codes of this 8-group, every other row a code of another group
ONE_CODE = 19
SETTINGS = [
    ("default", {}, FWD_CASES + [NONFINITE] + BWD_CASES),
    ("atomic", {"MAS_VQ_BWD_DET": "0"}, BWD_CASES),
]
CASES = {c["name"]: c for c in FWD_CASES + [NONFINITE] + BWD_CASES}


def modes_of(c):
    if c["kind"] == "fwd":
        return FWD_MODES
    if c["kind"] == "nonfinite":
        return ("gauss",)
    return ("gauss", "int") if c["int_too"] else ("gauss",)


def far_offset(d):
    return 3.0 if d == 256 else 8.0


# -------------------------------------------------------------------------------------------------------------------- planted ties
TIE_RELATIONS = ("adjacent_registers", "other_half_wave", "next_tile", "adjacent_splits", "first_last_split", "code0_last_code",
                 "triple_three_splits")


def relations_with_room(c):
    """the tie relations the geometry of a case has (a case with fewer than 33 rows plants what fits and promises nothing)"""
    geo, k = geometry(c["M"], c["K"]), c["K"]
    room = {"adjacent_registers": k >= 2, "other_half_wave": k >= 5, "next_tile": geo["tiles_per"] >= 2 and k > CODES_PER_TILE,
            "adjacent_splits": geo["active"] >= 2,
            "first_last_split": geo["active"] >= 2 and k - (geo["active"] - 1) * CODES_PER_TILE * geo["tiles_per"] >= 2,      # a code beside K - 1
            "code0_last_code": k >= 2, "triple_three_splits": geo["active"] >= 3}
    return [r for r in TIE_RELATIONS if room[r]]


def classify_ties(codes, c):
    """the relations a group of duplicate codes (ascending) stands in, from the restated geometry alone"""
    geo, out = geometry(c["M"], c["K"]), set()
    i, j = codes[0], codes[-1]
    tile = lambda k: k // CODES_PER_TILE
    if len(codes) == 3:
        if len({split_of(k, geo) for k in codes}) == 3:
            out.add("triple_three_splits")
        return out
    if tile(i) == tile(j) and j == i + 1 and i % 4 != 3:
        out.add("adjacent_registers")                  # same lane: acc_row(lane, r) and acc_row(lane, r + 1)
    if tile(i) == tile(j) and j == i + 4 and (i >> 2) & 1 == 0:
        out.add("other_half_wave")                     # same register, lanes l and l + 32
    if tile(j) == tile(i) + 1 and split_of(i, geo) == split_of(j, geo):
        out.add("next_tile")
    if split_of(j, geo) == split_of(i, geo) + 1:
        out.add("adjacent_splits")
    if split_of(i, geo) == 0 and split_of(j, geo) == geo["active"] - 1 and geo["active"] >= 2 and (i, j) != (0, c["K"] - 1):
        out.add("first_last_split")
    if (i, j) == (0, c["K"] - 1):
        out.add("code0_last_code")
    return out


def tie_plan(c, rs):
    """[(relation, codes)]: disjoint groups of codes to be made equal, two per relation where the codebook has room"""
    geo, k = geometry(c["M"], c["K"]), c["K"]
    stride = CODES_PER_TILE * geo["tiles_per"]
    used, plan = set(), []

    def take(rel, codes):
        if all(0 <= x < k for x in codes) and not used & set(codes) and len(set(codes)) == len(codes) and rel in classify_ties(sorted(codes), c):
            used.update(codes)
            plan.append((rel, tuple(sorted(codes))))
            return True
        return False

    order = [int(x) for x in rs.permutation(k)]
    last_split = [x for x in order if split_of(x, geo) == geo["active"] - 1]
    far = max(1, (geo["active"] - 2) // 2)
    for _ in range(2):
        for rel in sorted(relations_with_room(c), key=lambda r: r != "code0_last_code"):       # codes 0 and K - 1 first: nobody else takes them
            if rel == "code0_last_code":
                take(rel, (0, k - 1))
                continue
            for i in order:
                cand = {"adjacent_registers": [(i, i + 1)], "other_half_wave": [(i, i + 4)], "next_tile": [(i, i + CODES_PER_TILE)],
                        "adjacent_splits": [(i, i + stride)], "first_last_split": [(i, j) for j in last_split[:8]],
                        "triple_three_splits": [(i, i + far * stride, i + 2 * far * stride)]}[rel]
                if any(take(rel, cd) for cd in cand):
                    break
    return plan


# -------------------------------------------------------------------------------------------------------------------------- operands
def _seed(c, mode):
    return (sum(map(ord, c["name"])) * 7 + {"gauss": 0, "far": 1, "int": 2}[mode]) % (2 ** 31)


def bwd_pick(c, rs):
    m, k = c["M"], c["K"]
    if c["pattern"] == "one":
        return np.full(m, ONE_CODE, np.int64)
    if c["pattern"] == "edges":
        lo_g, hi_g = EDGE_GROUP * VB_CODES, (EDGE_GROUP + 1) * VB_CODES
        others = np.array([x for x in range(k) if not lo_g <= x < hi_g])
        pick = others[rs.randint(0, len(others), m)]
        for n, row in enumerate(edge_rows(m)):
            pick[row] = lo_g + n % VB_CODES
        return pick.astype(np.int64)
    if c["pattern"] == "ragged":
        pick = rs.randint(0, k, m)
        pick[0] = pick[m - 1] = k - 1
        pick[1] = k - k % VB_CODES                       # the first code of the ragged last group
        return pick.astype(np.int64)
    if c["pattern"] == "small":
        return np.array([k - 1, 0, k - 1][:m], np.int64)
    codes = rs.permutation(k)[:16]                      # rand16
    return codes[rs.randint(0, 16, m)].astype(np.int64)


def edge_rows(m):
    """the first and last row of every wave quarter and the rows on both sides of its 64-wide ballot boundary"""
    rows = set()
    for lo, hi in quarters(m):
        if hi > lo:
            rows |= {lo, hi - 1} | {r for r in (lo + 63, lo + 64) if r < hi}
    return sorted(rows)


def make_inputs(c, mode):
    """seeded CPU operands as float32 numpy arrays.  fwd: z [M, D], cb [K, D] (+ ties, tie_rows in *int* mode); nonfinite: z, z_finite,
    cb, bad_rows; bwd: z, cb, pick, g_zq, g_loss"""
    rs = np.random.RandomState(_seed(c, mode))
    m, k, d = c["M"], c["K"], c["D"]
    if c["kind"] == "bwd":
        pick = bwd_pick(c, rs)
        if mode == "int":
            cb = rs.randint(-4, 5, (k, d)).astype(f32)
            z = cb[pick] + rs.randint(-1, 2, (m, d)).astype(f32)
            g_zq, g_loss = rs.randint(-4, 5, (m, d)).astype(f32), 2.0
            assert (m * d) & (m * d - 1) == 0, c["name"]
        else:
            cb = rs.randn(k, d).astype(f32)
            z = (cb[pick] + 0.01 * rs.randn(m, d)).astype(f32)
            g_zq, g_loss = rs.randn(m, d).astype(f32), 0.7
        return dict(z=z, cb=cb, pick=pick, g_zq=g_zq, g_loss=g_loss)
    if mode == "int":
        z, cb = rs.randint(-4, 5, (m, d)).astype(f32), rs.randint(-4, 5, (k, d)).astype(f32)
        plan = tie_plan(c, rs)
        for _, codes in plan:
            cb[list(codes[1:])] = cb[codes[0]]
        rows = [int(x) for x in rs.permutation(m)]
        groups = {rel: [cd for r, cd in plan if r == rel] for rel, _ in plan}
        ties = []
        for n in range(4 if m >= 33 else 1):              # four rows per relation, shared among its groups
            for rel, cds in groups.items():
                if rows:
                    codes = cds[n % len(cds)]
                    row = rows.pop()
                    z[row] = cb[codes[0]]
                    ties.append((row, rel, codes))
        zero_rows = [rows.pop() for _ in range(2)] if m >= 33 else []      # |z|^2 = 0 < every real distance: a padded code would win
        z[zero_rows] = 0.0
        z64, c64 = z.astype(f64), cb.astype(f64)
        big = (z64 ** 2).sum(1)[:, None] + (c64 ** 2).sum(1)[None] + 2 * np.abs(z64) @ np.abs(c64).T
        assert float(big.max()) < 2 ** 24 and m * d * 64 < 2 ** 24, c["name"]
        return dict(z=z, cb=cb, ties=ties, zero_rows=zero_rows)
    off = far_offset(d) if mode == "far" else 0.0
    z, cb = (rs.randn(m, d) + off).astype(f32), (rs.randn(k, d) + off).astype(f32)
    if c["kind"] == "nonfinite":
        zf = z.copy()
        for r in NF_ALL_NAN:
            z[r] = np.nan
        z[NF_ONE_NAN, 17], z[NF_PINF, 3], z[NF_NINF, 40] = np.nan, np.inf, -np.inf
        return dict(z=z, z_finite=zf, cb=cb, bad_rows=sorted(NF_ALL_NAN + (NF_ONE_NAN, NF_PINF, NF_NINF)))
    return dict(z=z, cb=cb)


# ------------------------------------------------------------------------------------------------------------ references and bounds
_ref_cache = {}


def reference_fwd(c, mode):
    """fp64 distances of the fp32 operands and what the index rules need; one slot: judge, model and conditions ask in turn"""
    key = (c["name"], mode)
    if _ref_cache.get("key") != key:
        ins = make_inputs(c, mode)
        z, cb = (ins["z_finite"] if c["kind"] == "nonfinite" else ins["z"]).astype(f64), ins["cb"].astype(f64)
        zz, ee = (z * z).sum(1), (cb * cb).sum(1)
        d64 = zz[:, None] + ee[None] - 2.0 * (z @ cb.T)
        mag = np.abs(z) @ np.abs(cb).T
        bound = SECOND * U * ((sqnorm_chain(c["D"]) + 2) * (zz[:, None] + ee[None]) + 2 * c["D"] * mag + np.abs(d64))
        first = d64.argmin(1)
        rows = np.arange(c["M"])
        if c["K"] > 1:
            masked = d64.copy()
            masked[rows, first] = np.inf
            second = masked.argmin(1)
            gap = d64[rows, second] - d64[rows, first]
            wide = gap > bound[rows, first] + bound[rows, second]
        else:
            second, wide = first, np.ones(c["M"], bool)
        _ref_cache.update(key=key, val=dict(ins=ins, d64=d64, bound=bound, first=first, second=second, wide=wide))
    return _ref_cache["val"]


def near_tie_rows(c, mode):
    """rows whose fp64 top-2 gap is inside the bound: judged by the slack rule alone (from the reference alone)"""
    return int((~reference_fwd(c, mode)["wide"]).sum())


def loss_reference(c, ins, idx, mode):
    z, e = ins["z"].astype(f64), ins["cb"].astype(f64)[idx]
    ref = (1.0 + BETA) / (c["M"] * c["D"]) * ((e - z) ** 2).sum()
    chain = 2 if mode == "int" else sqnorm_chain(c["D"]) + 4 + 1 + 2 + 1 + 2
    return ref, SECOND * chain * U * abs(ref)


def bwd_reference(c, ins, idx, setting):
    """fp64 dz, dcb from the operands and the kernel's idx, with the bounds of sections 4 and 5"""
    m, k, d = c["M"], c["K"], c["D"]
    z, cb, g = ins["z"].astype(f64), ins["cb"].astype(f64), ins["g_zq"].astype(f64)
    coef = ins["g_loss"] * 2.0 / (m * d)
    diff = z - cb[idx]
    dz = g + coef * diff
    bdz = U * (np.abs(g) + 3 * np.abs(coef * diff) + np.abs(dz))
    term = -coef * BETA * diff
    dcb, mag = np.zeros((k, d)), np.zeros((k, d))
    np.add.at(dcb, idx, term)
    np.add.at(mag, idx, np.abs(term))
    hits = np.stack([np.bincount(idx[lo:hi], minlength=k) for lo, hi in quarters(m)])       # [4, K]
    chain = hits.max(0) + 3 if setting == "default" else hits.sum(0)
    bdcb = U * ((chain[:, None] + 3) * mag + np.abs(dcb))
    return dict(dz=dz, bdz=bdz, dcb=dcb, bdcb=bdcb, hits=hits)


# --------------------------------------------------------------------------------------------- fp32 models of the kernels' arithmetic
def planted(plant, kind):
    return plant == kind


def _butterfly_sum(lanes):
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(64) ^ o]
    return lanes[:, 0]


def _lane_squares(x):
    """row_sqnorm / vq_finalize: lane l adds x[l]^2, x[l + 64]^2, ... in order, then the 64-lane butterfly"""
    rows, d = x.shape
    xp = np.zeros((rows, cdiv(d, 64) * 64), f32)
    xp[:, :d] = x
    lanes = np.zeros((rows, 64), f32)
    for j in range(xp.shape[1] // 64):
        v = xp[:, j * 64:(j + 1) * 64]
        lanes = lanes + v * v
    return _butterfly_sum(lanes)


_dot_cache = {}


def model_dot(c, mode, z, cb, bf16=False):
    """dot(z_m, e_k) as a chain of fp32 FMAs: step s takes dimension s (lanes 0 .. 31) and then D / 2 + s (lanes 32 .. 63)"""
    key = (c["name"], mode, bf16)
    if key not in _dot_cache or "#" in c["name"]:         # (a second lookup's operand depends on the first one's result: never reused)
        if bf16:
            z, cb = (torch.from_numpy(a).bfloat16().float().numpy() for a in (z, cb))
        z64, c64 = z.astype(f64), cb.astype(f64)
        acc = np.zeros((z.shape[0], cb.shape[0]), f32)
        hd = c["D"] // 2
        for s in range(hd):
            for dim in (s, hd + s):
                acc = (z64[:, dim, None] * c64[None, :, dim] + acc).astype(f32)
        _dot_cache[key] = acc
    return _dot_cache[key]


def _take(bv, bi, ov, oi, rule):
    """take_min as a mask: where (ov, oi) replaces (bv, bi)"""
    if rule == "le":
        return ov <= bv
    if rule == "high":
        return (ov < bv) | ((ov == bv) & (oi > bi))
    return (ov < bv) | ((ov == bv) & (oi < bi))


def model_lookup(c, mode, z, cb, plant=None):
    """(idx, zq, loss) of mas_vq_argmin_fwd + the scale in ``ops``, in fp32 with the kernels' merge order"""
    m, k, d = c["M"], c["K"], c["D"]
    geo = geometry(m, k)
    ks, tp, nt = geo["ksplit"], geo["tiles_per"], geo["ntiles"]
    with np.errstate(all="ignore"):
        zz, ee = _lane_squares(z), _lane_squares(cb)
        if planted(plant, "ee_shifted"):
            ee = np.roll(ee, 1)
        dot = model_dot(c, mode, z, cb, bf16=planted(plant, "bf16_dot"))
        dist = (zz[:, None] + ee[None]) - f32(2.0) * dot
        tiles = ks * tp
        dp = np.full((m, tiles * CODES_PER_TILE), np.inf, f32)
        dp[:, :k] = dist
        if planted(plant, "padded_code"):                 # the staged tile holds zeros there; ee read as 0
            dp[:, k:nt * CODES_PER_TILE] = zz[:, None]
        if planted(plant, "last_tile_dropped"):
            for sp in range(geo["active"]):
                t1 = min(nt, (sp + 1) * tp)
                dp[:, (t1 - 1) * CODES_PER_TILE:t1 * CODES_PER_TILE] = np.inf
        # a lane: registers ascending, tiles ascending, strict <
        v = dp.reshape(m, ks, tp, CODES_PER_TILE)[:, :, :, ACC_ROW].transpose(0, 1, 3, 2, 4).reshape(m, ks, 2, tp * 16)
        ki = np.arange(tiles * CODES_PER_TILE).reshape(ks, tp, CODES_PER_TILE)[:, :, ACC_ROW].transpose(0, 2, 1, 3).reshape(ks, 2, tp * 16)
        v = np.where(np.isnan(v), np.inf, v)              # NaN < best is false
        pos = v.argmin(-1)
        if planted(plant, "lane_le"):                      # d <= best: a lane keeps its LAST minimum
            pos = v.shape[-1] - 1 - v[..., ::-1].argmin(-1)
        bv = np.take_along_axis(v, pos[..., None], -1)[..., 0]
        bi = np.take_along_axis(np.broadcast_to(ki, (m,) + ki.shape), pos[..., None], -1)[..., 0]
        bi = np.where(bv < np.inf, bi, SENTINEL)
        # the two half-waves of a row
        rule = "high" if planted(plant, "take_min_high") else "le" if planted(plant, "halfwave_le") else "low"
        t = _take(bv[:, :, 0], bi[:, :, 0], bv[:, :, 1], bi[:, :, 1], rule)
        pv, pi = np.where(t, bv[:, :, 1], bv[:, :, 0]), np.where(t, bi[:, :, 1], bi[:, :, 0])
        if planted(plant, "empty_zero"):
            pv[:, geo["active"]:], pi[:, geo["active"]:] = 0.0, 0
        # vq_finalize: lane sp, sp + 64, ...; then the butterfly
        rule = "high" if plant in ("take_min_high", "finalize_last") else "low"
        lv, li = np.full((m, 64), np.inf, f32), np.full((m, 64), SENTINEL, np.int64)
        for s0 in range(0, ks, 64):
            n = min(64, ks - s0)
            t = _take(lv[:, :n], li[:, :n], pv[:, s0:s0 + n], pi[:, s0:s0 + n], rule)
            lv[:, :n], li[:, :n] = np.where(t, pv[:, s0:s0 + n], lv[:, :n]), np.where(t, pi[:, s0:s0 + n], li[:, :n])
        for o in (32, 16, 8, 4, 2, 1):
            ov, oi = lv[:, np.arange(64) ^ o], li[:, np.arange(64) ^ o]
            t = _take(lv, li, ov, oi, rule)
            lv, li = np.where(t, ov, lv), np.where(t, oi, li)
        idx = np.where(li[:, 0] == SENTINEL, 0, li[:, 0]).astype(np.int64)
        gather = np.minimum(idx, k - 1)                    # (a planted padded code has no row to gather: the judge sees the index)
        if planted(plant, "zq_next"):
            gather = gather.copy()
            gather[m // 2] = (gather[m // 2] + 1) % k
        zq = cb[gather]
        df = cb[np.minimum(idx, k - 1)] - z
        wave = _lane_squares(df)
        blocks = np.zeros(cdiv(m, WAVES) * WAVES, f32)
        blocks[:m] = wave
        blocks = blocks.reshape(-1, WAVES)
        bsum = np.zeros(blocks.shape[0], f32)
        for w in range(WAVES):
            bsum = bsum + blocks[:, w]
        if planted(plant, "loss_last_block"):
            bsum = bsum[:-1]
        sq = f32(bsum.astype(f64).sum())
        loss = f32(sq * f32((1.0 + BETA) / (m * d)))
    return idx, zq, loss


def model_bwd(c, ins, idx, setting, plant=None, prefill=0.0):
    """(dz, dcb): vq_bwd_kernel's dz; dcb by the fixed-order kernel (``default``) or by one order of the atomics on ``prefill``"""
    m, k, d = c["M"], c["K"], c["D"]
    z, cb, g = ins["z"], ins["cb"], ins["g_zq"]
    coef = f32(f32(ins["g_loss"]) * f32(2.0)) / f32(m * d)
    diff = z - cb[idx]
    dz = (coef * diff).astype(f32) + (f32(0) if planted(plant, "dz_no_gzq") else g)
    beta = f32(BETA * BETA) if planted(plant, "beta_squared") else f32(BETA)
    if setting == "default":
        cbeta = f32(f32(-f32(ins["g_loss"]) * f32(2.0)) / f32(m * d)) * beta
        term = (cbeta * diff).astype(f32)
        acc = np.zeros((WAVES, k, d), f32)
        for w, (lo, hi) in enumerate(quarters(m)):
            if planted(plant, "fourth_quarter") and w == WAVES - 1:
                continue
            for row in range(lo, hi):
                if planted(plant, "hit_lo64") and row == lo + 64:
                    continue
                acc[w, idx[row]] = acc[w, idx[row]] + term[row]
        dcb = acc[0]
        for w in range(1, WAVES):
            dcb = dcb + acc[w]
        if planted(plant, "unstored_row") and prefill != 0.0:   # (else every row of the range is stored: the pre-fill is gone)
            last = [x for x in range((k - 1) // VB_CODES * VB_CODES, k) if x not in set(idx.tolist())]
            dcb[last[-1:]] = prefill
    else:
        term = ((-coef) * beta * diff).astype(f32)
        dcb = np.full((k, d), prefill, f32)
        for row in range(m):
            if planted(plant, "fourth_quarter") and row >= quarters(m)[-1][0]:
                continue
            if planted(plant, "hit_lo64") and any(row == lo + 64 < hi for lo, hi in quarters(m)):
                continue
            dcb[idx[row]] = dcb[idx[row]] + term[row]
    return dz.astype(f32), dcb.astype(f32)


def model_record(c, mode, plant=None, setting="default"):
    """what the GPU child would have written for (c, mode) had the kernels been these models: the same keys, so ``judge`` takes either"""
    ins = make_inputs(c, mode)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = {}
    if c["kind"] in ("fwd", "nonfinite"):
        idx, zq, loss = model_lookup(c, mode, ins["z"], ins["cb"], plant)
        out.update(idx=t(idx), zq=t(zq), loss=torch.tensor(float(loss), dtype=torch.float32), k_fwd="vq_finalize")
        if mode == "int":
            idx2, zq2, _ = model_lookup(dict(c, name=c["name"] + "#again"), mode, zq, ins["cb"], plant)
            out.update(idx2=t(idx2), zq2=t(zq2))
        if c["kind"] == "nonfinite":
            idx_f, zq_f, _ = model_lookup(dict(c, name=c["name"] + "#finite"), mode, ins["z_finite"], ins["cb"], plant)
            out.update(idx_f=t(idx_f), zq_f=t(zq_f))
        return out
    idx = ins["pick"]
    dz, dcb = model_bwd(c, ins, idx, setting, plant)
    kern = "vq_bwd_codebook" if setting == "default" else "vq_bwd"
    out.update(idx=t(idx), dz=t(dz), dcb=t(dcb), k_bwd=kern)
    if setting == "default":
        out.update(dz_again=t(dz.copy()), dcb_again=t(dcb.copy()))
    if c["variants"]:
        out.update(dz_only=t(dz.copy()), k_dz_only="vq_bwd", dcb_only=t(dcb.copy()), k_dcb_only=kern)
    if c["direct"]:
        if setting == "default":
            out["dcb_nan"] = t(model_bwd(c, ins, idx, setting, plant, prefill=float("nan"))[1])
        out["dcb_one"] = t(model_bwd(c, ins, idx, setting, plant, prefill=1.0)[1])
    return out


# ---------------------------------------------------------------------------------------------------------------------------- judging
def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _ratio(got, ref, bound):
    """(worst |got - ref| / bound over EVERY element, number outside); a non-finite value is outside, a zero bound asks for equality"""
    got = got.astype(f64)
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    return float(ratio.max()), int((ratio > 1).sum())


def judge(c, mode, rec, setting="default"):
    """every check of one (case, mode) recording -> (rows, reached, failures, notes): rows = (output, family, figure, verdict) with
    verdict "" (inside the bound), "equal" (an equality that holds) or a complaint; reached = the (kernel, feature) pairs; notes =
    {"slack_only": rows judged by the slack rule alone}"""
    rows, reached, failures, notes = [], set(), [], {}
    name, m, k, d = c["name"], c["M"], c["K"], c["D"]

    def put(key, fam, pair, equality=False):
        fig, bad = pair
        verdict = ("equal" if equality else "") if bad == 0 and fig <= 1 else f"{bad} OUTSIDE" if not equality else f"{bad} DIFFER"
        rows.append((key, fam, "%.3f" % fig, verdict))
        if verdict not in ("", "equal"):
            failures.append(f"{name} {mode} {key} ({fam}): {verdict}, worst figure {fig:.3f}")

    def equal(key, fam, got, want):
        nd = int((_bits(got) != _bits(want)).sum()) if got.shape == want.shape else max(got.size, 1)
        put(key, fam, (float(nd > 0), nd), equality=True)

    def same_idx(key, fam, got, want):
        nd = int((got != want).sum())
        put(key, fam, (float(nd > 0), nd), equality=True)

    def expect(key, want):
        if rec.get(key) != want:
            failures.append(f"{name} {mode}: {key} is {rec.get(key)}, not {want}")
        return rec.get(key) == want

    fam = "far" if mode == "far" else mode
    if c["kind"] in ("fwd", "nonfinite"):
        ref = reference_fwd(c, mode)
        ins, d64, bound, first, wide = ref["ins"], ref["d64"], ref["bound"], ref["first"], ref["wide"]
        geo = geometry(m, k)
        idx, zq = _np(rec["idx"]).astype(np.int64), _np(rec["zq"])
        inside = (idx >= 0) & (idx < k)
        put("idx in [0, K)", f"{fam} idx", (float((~inside).any()), int((~inside).sum())), equality=True)
        ok_kernel = expect("k_fwd", "vq_finalize")
        idc = np.clip(idx, 0, k - 1)
        r = np.arange(m)
        equal("zq = cb[idx]", f"{fam} zq", zq, ins["cb"][idc])
        if c["kind"] == "nonfinite":
            good = np.setdiff1d(r, ins["bad_rows"])
            same_idx("idx of the finite rows", "nonfinite idx", idx[good], _np(rec["idx_f"])[good])
            equal("zq of the finite rows", "nonfinite zq", zq[good], _np(rec["zq_f"])[good])
            lossv = float(_np(rec["loss"]))
            put("loss is non-finite", "nonfinite loss", (float(np.isfinite(lossv)), int(np.isfinite(lossv))), equality=True)
            if ok_kernel and not failures:
                reached.add(("vq_finalize", "nonfinite"))
            idx = _np(rec["idx_f"]).astype(np.int64)             # the index rules: on the finite call
            inside = (idx >= 0) & (idx < k)
            idc = np.clip(idx, 0, k - 1)
        slack = (d64[r, idc] - d64[r, first]) / (bound[r, idc] + bound[r, first])
        slack = np.where(inside, slack, np.inf)
        put("d64[idx] - min", f"{fam} slack", (float(slack.max()), int((slack > 1).sum())))
        if mode == "int":
            same_idx("idx = first fp64 minimum", "int idx", idx, first)
        else:
            notes["slack_only"] = int((~wide).sum())
            same_idx("idx = fp64 argmin (wide gap)", f"{fam} idx", idx[wide], first[wide])
        if c["kind"] == "fwd":
            want, bl = loss_reference(c, ins, idc, mode)
            put("loss", f"{fam} loss", _ratio(_np(rec["loss"]).reshape(1), np.array([want]), np.array([bl])))
        if mode == "int":
            same_idx("lookup of zq: idx", "int idempotence", _np(rec["idx2"]), idx)
            equal("lookup of zq: zq", "int idempotence", _np(rec["zq2"]), zq)
            tied = {}
            for row, rel, codes in ins["ties"]:
                tied.setdefault(rel, []).append(idx[row] == codes[0])
            if ok_kernel:
                reached |= {("vq_finalize", "tie:" + rel) for rel, hits in tied.items() if all(hits) and len(hits) >= 4}
                reached.add(("vq_finalize", "idempotent"))
        if ok_kernel and c["kind"] == "fwd":
            reached.add(("vq_partial", "D%d" % d))
            reached |= {("vq_partial", f) for f, on in (("empty_splits", geo["empty"] > 0), ("ksplit_capped", geo["capped"]),
                                                       ("two_tiles_ragged", geo["tiles_per"] >= 2 and geo["last_codes"] < CODES_PER_TILE),
                                                       ("one_split", geo["ksplit"] == 1), ("row_blocks_17", geo["rb"] == 17)) if on}
        return rows, reached, failures, notes

    ins = make_inputs(c, mode)
    idx = _np(rec["idx"]).astype(np.int64)
    same_idx("idx = pick", f"{fam} idx", idx, ins["pick"])
    idx = np.clip(idx, 0, k - 1)
    ref = bwd_reference(c, ins, idx, setting)
    kern = "vq_bwd_codebook" if setting == "default" else "vq_bwd"
    label = "fixed order" if setting == "default" else "atomics"

    def dz_rows(key, got):
        if mode == "int":
            equal(key, "int dz", got, ref["dz"].astype(f32))
        else:
            put(key, f"{fam} dz", _ratio(got, ref["dz"], ref["bdz"]))

    def dcb_rows(key, got):
        if mode == "int":
            assert np.array_equal(ref["dcb"].astype(f32).astype(f64), ref["dcb"]), (name, "dcb is not representable in fp32")
            equal(key, f"int dcb {label}", got, ref["dcb"].astype(f32) + f32(0))
        else:
            put(key, f"{fam} dcb {label}", _ratio(got, ref["dcb"], ref["bdcb"]))

    dz_rows("dz", _np(rec["dz"]))
    dcb_rows("dcb", _np(rec["dcb"]))
    ok = expect("k_bwd", kern)
    if setting == "default":
        equal("dz, second run", "repeat", _np(rec["dz_again"]), _np(rec["dz"]))
        equal("dcb, second run", "repeat", _np(rec["dcb_again"]), _np(rec["dcb"]))
    feats = {"D%d" % d, c["pattern"]} | ({"int_exact"} if mode == "int" else set())
    if c["variants"]:
        dz_rows("dz, z alone needs grad", _np(rec["dz_only"]))
        dcb_rows("dcb, codebook alone needs grad", _np(rec["dcb_only"]))
        if expect("k_dz_only", "vq_bwd") and expect("k_dcb_only", kern):
            feats |= {"need_z", "need_cb", "need_both"}
    if c["direct"]:
        unpicked = np.setdiff1d(np.arange(k), idx)
        assert len(unpicked) and any(x >= k - k % VB_CODES for x in unpicked), (name, "no unpicked code in the last group")
        one = _np(rec["dcb_one"])
        if setting == "default":
            nan = _np(rec["dcb_nan"])
            bad = int((~np.isfinite(nan)).sum())
            put("dcb over a NaN fill: finite", "direct call", (float(bad > 0), bad), equality=True)
            equal("dcb over a NaN fill: unpicked rows 0", "direct call", nan[unpicked], np.zeros_like(nan[unpicked]))
            dcb_rows("dcb over a NaN fill", nan)
            equal("dcb over a fill of ones", "direct call", one, nan)
            feats.add("prefill_overwritten")
        else:
            equal("dcb over a fill of ones: unpicked rows 1", "direct call", one[unpicked], np.ones_like(one[unpicked]))
            feats.add("prefill_added_to")
    if ok:
        reached |= {(kern, f) for f in feats}
    return rows, reached, failures, notes


# ------------------------------------------------------------------------------------------------------------------------- GPU child
def run(setting, out_path):
    from mas_hip import lib, check, _ptr, _stream, ops
    label, env, cases = next(s for s in SETTINGS if s[0] == setting)
    for key, v in env.items():
        assert os.environ.get(key) == v, f"start this child with {key}={v}"
    if setting == "default":
        assert os.environ.get("MAS_VQ_BWD_DET", "1") == "1", "start this child without MAS_VQ_BWD_DET"
    dev = torch.device("cuda:0")
    back = lambda t: t.detach().cpu().contiguous()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def as_map(rows):            # [M, D] rows -> the [1, D, 1, M]-logical tensor in channels-last memory
        return rows.view(1, 1, rows.shape[0], rows.shape[1]).permute(0, 3, 1, 2)

    def as_rows(t):
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])

    def lookup(z_rows, cb):
        zq, loss, idx = ops.vq_lookup(as_map(z_rows), cb, BETA)
        return zq, loss, idx, ops.last_kernel()

    results = {}
    for c in cases:
        for mode in modes_of(c):
            ins = make_inputs(c, mode)
            m, k, d = c["M"], c["K"], c["D"]
            out = {}
            cb = up(ins["cb"])
            if c["kind"] in ("fwd", "nonfinite"):
                with torch.no_grad():
                    zq, loss, idx, out["k_fwd"] = lookup(up(ins["z"]), cb)
                    out.update(idx=back(idx), zq=back(as_rows(zq)), loss=back(loss))
                    if mode == "int":
                        zq2, _, idx2, _ = lookup(as_rows(zq).contiguous(), cb)
                        out.update(idx2=back(idx2), zq2=back(as_rows(zq2)))
                    if c["kind"] == "nonfinite":
                        zq_f, _, idx_f, _ = lookup(up(ins["z_finite"]), cb)
                        out.update(idx_f=back(idx_f), zq_f=back(as_rows(zq_f)))
            else:
                g_zq, g_loss = as_map(up(ins["g_zq"])), torch.tensor(ins["g_loss"], dtype=torch.float32, device=dev)

                def grads(need_z, need_cb):
                    zr, cbr = up(ins["z"]).requires_grad_(need_z), up(ins["cb"]).requires_grad_(need_cb)
                    zq, loss, idx, _ = lookup(zr, cbr)
                    torch.autograd.backward([zq, loss], [g_zq, g_loss])
                    kern = ops.last_kernel()
                    return (back(zr.grad) if need_z else None), (back(cbr.grad) if need_cb else None), back(idx), kern

                out["dz"], out["dcb"], out["idx"], out["k_bwd"] = grads(True, True)
                if setting == "default":
                    out["dz_again"], out["dcb_again"], _, _ = grads(True, True)
                if c["variants"]:
                    out["dz_only"], _, _, out["k_dz_only"] = grads(True, False)
                    _, out["dcb_only"], _, out["k_dcb_only"] = grads(False, True)
                if c["direct"]:             # the call of ops._VQ.backward, on a dcb the caller did not zero
                    zr, idx_d, gz, gl = up(ins["z"]), out["idx"].to(dev), up(ins["g_zq"]), g_loss.reshape(1).contiguous()
                    for key, fill in (("dcb_nan", float("nan")), ("dcb_one", 1.0)):
                        if key == "dcb_nan" and setting != "default":
                            continue
                        dz, dcb = torch.empty_like(zr), torch.full((k, d), fill, dtype=torch.float32, device=dev)
                        check(lib().mas_vq_bwd(_ptr(zr), _ptr(cb), _ptr(idx_d), _ptr(gz), _ptr(gl), float(BETA), m, k, d,
                                               _ptr(dz), _ptr(dcb), _stream()), "vq_bwd")
                        torch.cuda.synchronize()
                        out[key] = back(dcb)
            torch.cuda.synchronize()
            results[(c["name"], mode)] = out
            print(f"{label:8s} {c['name']:20s} {mode:5s} " + " ".join(f"{key}={v}" for key, v in sorted(out.items()) if key.startswith("k_")), flush=True)
    torch.save(dict(results=results, env={key: os.environ.get(key) for key in env}), out_path)


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2])
