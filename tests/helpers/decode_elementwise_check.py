"""Decode attention (make-a-scene_amd/csrc/attn_decode.hip + attn_decode_core.h, attn_decode_split.hip, attn_decode_shared.hip +
attn_decode_tile.h; host-``past`` and device-``past`` forms) judged element by element: cases, inputs, the fp64 reference, the bounds, a
float32 model of the three key walks with its mutations, and ``run`` (GPU only).  Importing this file needs neither a GPU nor the library.
tests/test_decode_elementwise_cpu.py shows that the judgement has teeth, tests/test_gpu_decode_elementwise.py judges the kernels.

Inputs and reference are those of tests/helpers/attn_rowwise_check.py (``CHK``): a decode call with nq queries and ``past`` cached rows is
the last nq rows of causal attention over S = past + nq keys, so the operands are ``CHK.make_inputs`` (seeded by the case name) and the
truth is ``CHK.reference``: its ``o`` and ``A_o = P |v|`` on rows past .. past + nq - 1.  Layout [slices, H, S, hd] float64, a slice
being a batch element or, for the shared kernels, a candidate row.  What is added to those operands here (``make_inputs``):
  shared   every row of a group is a slice of its own (its own query and own keys / values); the first ``prompt_len`` keys and values are
           copied from the group's first slice into all of them before the reference is taken, and those are the prompt block.  In the
           onehot mode the own keys of the other rows are the codes the prompt block left over, in an order of the row's own, so no row
           meets a code twice.
  targets  the queries of the decode rows are planted again, one target key per (slice, head, query) (``decode_targets``): slice 0 always
           on the LAST visible key (the row the device-``past`` forms append), the others rotate through the last key of every split's
           range and the first key of the next, key 0, the key before the last, the first key and a middle key of the last (ragged) pass
           and keys 31 / 32 / 63 / 64 / KPP - 1 / KPP / pass - 1 / pass.
  cold     hard mode, split and shared routes (the ones that keep per-range states), S <= 64, last (slice, head): the query carries 5 a on plant bits 6 .. 9, which are -1 in every key below 64, and 0
           on bits 0 .. 5: EVERY visible key scores about -120.  A correct online softmax only sees differences; one that mixes in a state
           with m = 0 (an empty split taken as m = 0 instead of -1e30) multiplies everything by exp(-120) = 0 in fp32.  No other row can
           show that defect: wherever a target is visible the maximum is +60 and exp(0 - 60) only adds zeros.

Modes: gauss and hard take the general bound; onehot requires ``CHK.onehot_precondition`` on the reference alone (per slice) and then
o == v[target] BITWISE for bf16 and fp32 (the kernels keep q * scale, the scores, m, l, o, the merges and 1 / l in fp32 and cast once at
the store: l is exactly 1 and what the other keys add is absorbed below half an ulp of an integer v); uniform (q = 0, integer v) is
sum(v) / L exactly where L is a power of two -- bitwise for fp32, bitwise after the one rounding for bf16 -- and takes the general bound
elsewhere.  The code books serve 769 keys, at hd 16 (minimum distance 4 in 16 bits, a greedy search) 513: a longer case (the ones that give
every one of 32 splits a key need 993 keys; bf16 hd 16 beyond its 512-key pass) has no onehot mode.

Bounds (U, TAU, C_F32, FLOOR are CHK's, the project's measured values for this arithmetic: fp32 sums of at most 128 products, __expf, a
few hundred keys):   bf16  |y - r| <= U |r| + C_F32 TAU A_o + FLOOR      fp32  |y - r| <= C_F32 TAU A_o + FLOOR
Condition, checked on the CPU: the float32 model below (numpy float32, np.exp, the kernels' order) stays under a QUARTER of the fp32 bound
C_F32 TAU A_o + FLOOR in every case and mode -- for bf16 cases the model's value before the store (the store's own rounding reaches all of
U |r| by itself, so the rounded value is held to the whole bf16 bound); the factor 4 is left for __expf, as tests/test_gpu_token_loss.py
allows a fast exp.

The model (``model``): q * scale, a score per key (unsplit: the hd products added in order; split / tile: the EPU products of a 16-byte
unit added in order, then the G units by the butterfly), then per slot the online softmax over its keys in the order the kernel meets them
  unsplit  256 slots (lanes), slot t owns keys t, t + 256, ...
  split    chunk = ceil(L / nsplit) rounded up to 32, range s = [s chunk, min(L, (s + 1) chunk)), KPP = 256 / G slots, slot t owns keys
           begin + t, begin + t + KPP, ... (a pass is KPP * KU keys); the states are combined in split order
  shared   the prompt ranges (every row of the group against the group's prompt block), then the row's own ranges, one combine
the slots of a wave merged by the butterfly (halves added), the four waves in order, m = -1e30, l = 0, o = 0 for anything without keys.
"""
import zlib

import numpy as np

import attn_rowwise_check as CHK

QT, GRAN, KU, NT, MAX_SPLITS = 4, 32, 4, 256, 32
S_ONEHOT_MAX = {16: 513, 32: 769, 64: 769, 128: 769}
COLD = -2
ROUTES = ("unsplit", "split", "shared")
HOST = {"unsplit": "attn_decode", "split": "attn_decode_split", "shared": "attn_decode_shared"}
DEV = {r: k + "_dev" for r, k in HOST.items()}
L_CATEGORIES = ("1", "31", "32", "33", "kpp-1", "kpp", "kpp+1", "pass-1", "pass", "pass+1", "ragged2")
COMBOS = [(dt, hd) for dt in ("bf16", "f32") for hd in (16, 32, 64, 128)]


# --------------------------------------------------------------------------- #
# geometry
# --------------------------------------------------------------------------- #
def geom(route, dtype, hd):
    """epu: elements of a 16-byte unit; G: lanes per key row; slots: key slots of the work-group; kpp: the slot edge the lengths are chosen
    around (a wave for the unsplit kernel); keys per pass"""
    epu = 8 if dtype == "bf16" else 4
    if route == "unsplit":
        return dict(epu=epu, G=1, slots=NT, kpp=64, keys_per_pass=NT)
    G = hd // epu
    return dict(epu=epu, G=G, slots=NT // G, kpp=NT // G, keys_per_pass=NT // G * KU)


def split_ranges(L, nsplit):
    chunk = -(-(-(-L // nsplit)) // GRAN) * GRAN
    return [(s * chunk, min(L, (s + 1) * chunk)) for s in range(nsplit)]            # end <= begin: no key


def walks(c):
    """[(begin, end)] of every key range a work-group walks, in key indices of the S keys (own ranges after the prompt)"""
    if c["route"] == "unsplit":
        return [(0, c["past"] + i + 1) for i in range(c["nq"])]
    if c["route"] == "split":
        return split_ranges(c["S"], c["nsplit"])
    p = c["plen"]
    return split_ranges(p, c["nsp"]) + [(p + b, p + e) for b, e in split_ranges(c["own"], c["nso"])]


# --------------------------------------------------------------------------- #
# cases
# --------------------------------------------------------------------------- #
def _modes(S, hd):
    return ("gauss", "hard", "onehot", "uniform") if S <= S_ONEHOT_MAX[hd] else ("gauss", "hard", "uniform")


def _unsplit(dtype, hd, L, nq=1, layout="plain", B=2, H=3, cat=None):
    """L: the keys the FIRST query sees (past + 1); query i sees L + i"""
    S = L - 1 + nq
    return dict(name=f"dec_unsplit-{dtype}-hd{hd}-B{B}H{H}L{L}nq{nq}-{layout}", route="unsplit", dtype=dtype, hd=hd, nsl=B, H=H, S=S,
                past=L - 1, nq=nq, layout=layout, modes=_modes(S, hd), cat=cat)


def _split(dtype, hd, L, nsplit, B=2, H=3, cat=None):
    return dict(name=f"dec_split-{dtype}-hd{hd}-B{B}H{H}L{L}-n{nsplit}", route="split", dtype=dtype, hd=hd, nsl=B, H=H, S=L, past=L - 1,
                nq=1, nsplit=nsplit, modes=_modes(L, hd), cat=cat)


def _shared(dtype, hd, group, plen, own, nsp, nso, groups=2, H=3, cat=None):
    S = plen + own
    return dict(name=f"dec_shared-{dtype}-hd{hd}-g{groups}x{group}H{H}-p{plen}o{own}-n{nsp}_{nso}", route="shared", dtype=dtype, hd=hd,
                nsl=groups * group, H=H, S=S, past=S - 1, nq=1, group=group, groups=groups, plen=plen, own=own, nsp=nsp, nso=nso,
                modes=_modes(S, hd), cat=cat)


def lengths(route, dtype, hd):
    """{category: L} of a (route, dtype, hd): the edges of the 32-key granule, of the slots and of a pass, and a second ragged pass"""
    g = geom(route, dtype, hd)
    K, P = g["kpp"], g["keys_per_pass"]
    return {"1": 1, "31": 31, "32": 32, "33": 33, "kpp-1": K - 1, "kpp": K, "kpp+1": K + 1, "pass-1": P - 1, "pass": P, "pass+1": P + 1,
            "ragged2": P + K + 3}


def _thinned(ci):
    """the categories combination ci of 8 takes: a window of four that moves by three, and a length beyond a pass.  The union over the
    eight (dtype, hd) of a route is every category (tests/test_decode_elementwise_cpu.py asserts it)"""
    idx = {(3 * ci + j) % 11 for j in range(4)} | {10 if ci % 2 == 0 else 9}
    return [L_CATEGORIES[i] for i in sorted(idx)]


def _cases():
    c = []
    NQ = (1, 2, 1, 5, 1)
    NSPLIT = (2, 3, 8, 1, 32)
    n = 0
    for ci, (dt, hd) in enumerate(COMBOS):
        # ---- unsplit: nq in {1, 2, 5}, q a strided view / k, v with strides of their own on every other case
        for cat in _thinned(ci):
            L = lengths("unsplit", dt, hd)[cat]
            c.append(_unsplit(dt, hd, L, nq=NQ[n % 5], layout=("plain", "strided")[n % 2], cat=cat))
            n += 1
        # ---- split: nsplit in {1, 2, 3, 8, 32}
        for cat in _thinned(ci):
            L = lengths("split", dt, hd)[cat]
            c.append(_split(dt, hd, L, NSPLIT[n % 5], cat=cat))
            n += 1
        c.append(_split(dt, hd, 33, (32, 2)[ci % 2], cat="33"))          # 31 neutral states / the last split with keys holds one key
        # ---- shared: group x prompt_len x own length x split counts, thinned; the long prompts go with small groups (the reference is
        #      slices * S^2)
        g = geom("shared", dt, hd)
        K, P = g["kpp"], g["keys_per_pass"]
        ecat = ("kpp-1", "kpp", "kpp+1", "pass-1", "pass")[ci % 5]
        edge = lengths("shared", dt, hd)[ecat]
        c += [_shared(dt, hd, 5 if P + 1 <= 160 else 1, P + 1, 33, 2, 3, cat="pass+1"),
              _shared(dt, hd, 3, 33, 1, 1, 1, cat="33"),
              _shared(dt, hd, 4, 31, 32, 5, 1, cat="31"),
              _shared(dt, hd, 5, 1, 33, 2, 3, cat="1"),
              _shared(dt, hd, 9, 33, 32, 2, 3, cat="33"),
              _shared(dt, hd, 4 if edge <= 160 else 1, edge, 1, 5, 1, cat=ecat)]
        if hd in (16, 128):                                              # nst = 64: the combine block has 64 (hd 16) and 128 (hd 128) lanes
            c.append(_shared(dt, hd, 5, 33, 33, 32, 32, cat="33"))
    # every one of 32 splits holds keys from 993 keys on (31 * 32 + 1: the last split holds exactly one); no onehot mode at that length
    c += [_split("bf16", 128, 993, 32, cat="all32"), _split("f32", 16, 993, 32, cat="all32"),
          _shared("bf16", 16, 1, 31, 993, 32, 32, cat="all32"), _shared("f32", 128, 1, 31, 993, 32, 32, cat="all32")]
    # B = H = 1, one per route
    c += [_unsplit("bf16", 64, 65, B=1, H=1, cat="kpp+1"), _split("f32", 32, 129, 3, B=1, H=1, cat="pass+1"),
          _shared("bf16", 32, 1, 33, 33, 2, 3, groups=1, H=1, cat="33")]
    seen, out = set(), []
    for x in c:                                      # two categories can name one length (KPP = 32)
        if x["name"] not in seen:
            seen.add(x["name"])
            out.append(x)
    return out


CASES = _cases()


def features(c):
    g = geom(c["route"], c["dtype"], c["hd"])
    f = {c["dtype"], "hd%d" % c["hd"]}
    for b, e in walks(c):
        n = e - b
        if n <= 0:
            f.add("empty_splits")
            continue
        if n % g["keys_per_pass"]:
            f.add("ragged_pass")
        if n > g["keys_per_pass"]:
            f.add("multi_pass")
        if n < GRAN:
            f.add("sub_granule")
    if c["route"] == "shared":
        if c["nsp"] + c["nso"] == 64:
            f.add("nst64")
        if MAX_SPLITS in (c["nsp"], c["nso"]):
            f.add("nsplit32")
        if c["group"] % QT:
            f.add("ragged_group")
        f.add("strided_q")
    if c["route"] == "split":
        if c["nsplit"] == MAX_SPLITS:
            f.add("nsplit32")
        f.add("strided_q")
    if c["route"] == "unsplit" and c["layout"] == "strided":
        f.add("strided_q")
    if c["nq"] > 1:
        f.add("nq_gt1")
    if c["nsl"] == 1 and c["H"] == 1:
        f.add("bh1")
    return f


_SHAPE = {"bf16", "f32", "hd16", "hd32", "hd64", "hd128", "ragged_pass", "multi_pass", "sub_granule", "bh1"}
_SPLIT = _SHAPE | {"empty_splits", "nsplit32"}
REQUIRED = {
    "attn_decode": _SHAPE | {"nq_gt1", "strided_q"},
    "attn_decode_dev": _SHAPE | {"dev_append"},
    "attn_decode_split": _SPLIT | {"strided_q"},
    "attn_decode_split_dev": _SPLIT | {"dev_append"},
    "attn_decode_shared": _SPLIT | {"nst64", "ragged_group", "strided_q"},
    "attn_decode_shared_dev": _SPLIT | {"nst64", "ragged_group", "dev_append"},
}


def has_dev(c):
    return c["nq"] == 1


def reached(cases_and_kernels):
    """[(case, {form: kernel name})] -> {kernel: features}"""
    got = {}
    for c, kern in cases_and_kernels:
        f = features(c)
        if "host" in kern:
            got.setdefault(kern["host"], set()).update(f)
        if "dev" in kern:
            got.setdefault(kern["dev"], set()).update((f - {"strided_q", "nq_gt1"}) | {"dev_append"})
    return got


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def target_candidates(c, iq):
    """the keys worth holding query iq's maximum, the last visible key first"""
    L = c["past"] + iq + 1
    g = geom(c["route"], c["dtype"], c["hd"])
    K, P = g["kpp"], g["keys_per_pass"]
    cand = [L - 1]
    for b, e in walks(c):
        if e > b and c["route"] != "unsplit":
            cand += [e - 1, e]                       # the last key of a split's range, the first key of the next
    p0 = (L - 1) // P * P
    cand += [0, L - 2, p0, (p0 + L - 1) // 2, 31, 32, 63, 64, K - 1, K, P - 1, P]
    out = []
    for t in cand:
        if 0 <= t < L and t not in out:
            out.append(t)
    return out


def decode_targets(c, mode):
    """[slices, H, nq] target keys; COLD: the cold query (hard mode only)"""
    nsl, H, nq = c["nsl"], c["H"], c["nq"]
    off = zlib.crc32(c["name"].encode()) % 97
    tg = np.zeros((nsl, H, nq), dtype=np.int64)
    for iq in range(nq):
        cand = target_candidates(c, iq)
        rest = cand[1:] or cand
        for b in range(nsl):
            for h in range(H):
                sl = b * H + h
                tg[b, h, iq] = cand[0] if sl == 0 else rest[(off + sl - 1 + 5 * iq) % len(rest)]
    if mode == "hard" and c["route"] != "unsplit" and c["S"] <= 64 and nsl * H > 1:
        tg[nsl - 1, H - 1, :] = COLD
    return tg


def make_inputs(c, mode):
    nsl, H, S, hd = c["nsl"], c["H"], c["S"], c["hd"]
    ins = CHK.make_inputs(dict(name=c["name"], B=nsl, H=H, S=S, hd=hd, dtype=c["dtype"]), mode)
    q, k, v, scale = ins["q"], ins["k"], ins["v"], ins["scale"]
    rs = np.random.RandomState(zlib.crc32((c["name"] + mode + "/decode").encode()) & 0x7FFFFFFF)
    cq = float(np.ceil(CHK.GAP / (scale * 2 * CHK.DMIN[hd])))
    if c["route"] == "shared":
        plen, own = c["plen"], c["own"]
        first = np.arange(nsl) // c["group"] * c["group"]
        k0 = k.copy()
        k[:, :, :plen] = k0[first][:, :, :plen]
        v[:, :, :plen] = v[first][:, :, :plen].copy()
        if mode == "onehot":
            for r in range(nsl):
                for h in range(H):
                    if r != first[r]:
                        k[r, h, plen:] = k0[first[r], h, plen:][rs.permutation(own)]
            q[:] = cq * k[:, :, ins["target"]]       # every row's query follows its keys again
    tg = decode_targets(c, mode)
    if mode == "hard":
        a = float(round(6.0 / scale))
        bits = ((np.arange(1 << CHK.PLANT)[:, None] >> np.arange(CHK.PLANT)[None, :]) & 1) * 2.0 - 1.0
    for b in range(nsl):
        for h in range(H):
            for iq in range(c["nq"]):
                row, t = c["past"] + iq, int(tg[b, h, iq])
                if mode == "hard":
                    if t == COLD:
                        q[b, h, row, :6] = 0.0
                        q[b, h, row, 6:CHK.PLANT] = 5.0 * a
                    else:
                        q[b, h, row, :CHK.PLANT] = a * bits[t % (1 << CHK.PLANT)]
                elif mode == "onehot":
                    q[b, h, row] = cq * k[b, h, t]
    ins["dtarget"] = tg
    return ins


def onehot_precondition(c, ins, ref):
    """``CHK.onehot_precondition`` slice by slice, on the reference alone: the decode rows with their targets, the others with the rule
    their queries were built by (dO plays no part in decoding: zero)"""
    S = c["S"]
    for b in range(c["nsl"]):
        for h in range(c["H"]):
            tg = ins["target"].copy()
            tg[c["past"]:c["past"] + c["nq"]] = ins["dtarget"][b, h]
            vv = ins["v"][b:b + 1, h:h + 1]
            CHK.onehot_precondition(dict(target=tg, v=vv, do=np.zeros_like(vv)), dict(P=ref["P"][b:b + 1, h:h + 1]))
    assert S <= S_ONEHOT_MAX[c["hd"]]


# --------------------------------------------------------------------------- #
# judgement
# --------------------------------------------------------------------------- #
def rows_of(c, x):
    return x[:, :, c["past"]:c["past"] + c["nq"]]


def prepare(c, mode):
    """-> (ins, ref): the operands and the fp64 truth of the decode rows, ref = {o, A_o} [slices, H, nq, hd].  The onehot precondition is
    asserted here, on the reference alone, before any output exists"""
    ins = make_inputs(c, mode)
    full = CHK.reference(ins)
    if mode == "onehot":
        onehot_precondition(c, ins, full)
    del ins["do"]
    return ins, dict(o=rows_of(c, full["o"]).copy(), A_o=rows_of(c, full["A_o"]).copy())


def bound(c, ref, f32_part=False):
    r, A = ref["o"], ref["A_o"]
    bd = CHK.FLOOR + CHK.C_F32 * CHK.TAU * A
    return bd + CHK.U * np.abs(r) if c["dtype"] == "bf16" and not f32_part else bd


def exact_want(c, mode, ins):
    """(want [slices, H, nq, hd], mask of the queries it holds for) of the exact modes, else None"""
    if mode == "onehot":
        tg = ins["dtarget"]
        b, h = np.arange(c["nsl"])[:, None, None], np.arange(c["H"])[None, :, None]
        return ins["v"][b, h, tg], np.ones(c["nq"], dtype=bool)
    if mode == "uniform":
        L = c["past"] + 1 + np.arange(c["nq"])
        want = rows_of(c, np.cumsum(ins["v"], axis=2)) / L[:, None]
        if c["dtype"] == "bf16":
            want = CHK.bf16_round(want).astype(np.float64)
        return want, (L & (L - 1)) == 0
    return None


def judge(c, mode, ins, ref, y, tag=""):
    """y [slices, H, nq, hd] -> (failures: [str], worst |y - r| / bound)"""
    y = np.asarray(y, dtype=np.float64)
    r, bd = ref["o"], bound(c, ref)
    assert y.shape == r.shape, (c["name"], y.shape, r.shape)
    tag = f"{c['name']} {mode}{' ' + tag if tag else ''}"
    err = np.abs(y - r)
    with np.errstate(invalid="ignore"):
        ratio = np.where(np.isfinite(y), err / bd, np.inf)
    worst = float(ratio.max())
    fails = []
    bad = ~(err <= bd) | ~np.isfinite(y)
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        fails.append(f"{tag}: {int(bad.sum())} of {bad.size} elements outside, worst ratio {worst:.3g}, first bad (slice, h, query, col) = "
                     f"{first}: got {y[first]!r}, reference {r[first]!r}")
    ex = exact_want(c, mode, ins)
    if ex is not None:
        want, qmask = ex
        bad = (y != want) & qmask[None, None, :, None]
        if bad.any():
            first = tuple(int(i) for i in np.argwhere(bad)[0])
            fails.append(f"{tag} exact: {int(bad.sum())} of {bad.size} elements differ bitwise, first (slice, h, query, col) = {first}: got "
                         f"{y[first]!r}, want {want[first]!r}")
    return fails, worst


def old_criterion_passes(c, ref, y):
    """what the three older decode test files ask: max|y - ref| / max|ref| < 1e-2 (bf16), 2e-5 (fp32)"""
    r = ref["o"]
    e = np.abs(np.asarray(y, dtype=np.float64) - r).max() / max(np.abs(r).max(), 1e-12)
    return bool(e < (1e-2 if c["dtype"] == "bf16" else 2e-5)), float(e)


# --------------------------------------------------------------------------- #
# float32 model of the three walks, with mutations
# --------------------------------------------------------------------------- #
MUTATIONS = {                                        # name: the routes it applies to
    "drop_split_end": ("split", "shared"),           # one key dropped at the end of a split's range
    "drop_last_key": ROUTES,                         # key `past` dropped
    "range_start_off_by_one": ("split", "shared"),   # a split's range starts one early: a key is counted twice
    "skip_rescale": ROUTES,                          # o not multiplied by a = exp(m - m_new) when a slot's maximum rises
    "empty_m0": ("split", "shared"),                 # an empty split's state taken as m = 0 instead of -1e30
    "combine_skips_state63": ("shared",),            # the combine ignores the last state when nst = 64
    "next_head_k_unit": ROUTES,                      # a head reads its neighbour's first 16-byte unit of K
    "swap_v_rows": ROUTES,                           # the V rows of two adjacent keys swapped
    "truncate_out": ROUTES,                          # bf16 output truncated instead of rounded
    "swap_query_slots": ("shared",),                 # query slots 1 and 2 of a prompt tile exchanged
    "ragged_store_last_row": ("shared",),            # the query past the end of a ragged group lands on the group's last row
}
F32 = np.float32


def _tree(x, axis=-1):
    """the butterfly: x[i] + x[i ^ off] for off = n / 2 ... 1 -- the upper half added to the lower until one is left"""
    x = np.moveaxis(x, axis, -1)
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def _scores(c, qf, K):
    """qf [..., hd] (pre-scaled), K [..., n, hd] -> [..., n], float32 in the kernel's order"""
    g = geom(c["route"], c["dtype"], c["hd"])
    if c["route"] == "unsplit":
        s = np.zeros(K.shape[:-1], dtype=F32)
        for d in range(c["hd"]):
            s = s + qf[..., None, d] * K[..., d]
        return s
    G, epu = g["G"], g["epu"]
    Kr, qr = K.reshape(K.shape[:-1] + (G, epu)), qf.reshape(qf.shape[:-1] + (G, epu))
    part = np.zeros(Kr.shape[:-1], dtype=F32)
    for j in range(epu):
        part = part + qr[..., None, :, j] * Kr[..., j]
    return _tree(part)


def _walk(s, V, begin, end, nslot, skip_rescale):
    """slot t meets keys begin + t, begin + t + nslot, ...: (m, l, o) per slot"""
    lead, hd = s.shape[:-1], V.shape[-1]
    m = np.full(lead + (nslot,), -1e30, dtype=F32)
    l = np.zeros(lead + (nslot,), dtype=F32)
    o = np.zeros(lead + (nslot, hd), dtype=F32)
    for k0 in range(begin, end, nslot):
        n = min(nslot, end - k0)
        sk, mo = s[..., k0:k0 + n], m[..., :n]
        mn = np.maximum(mo, sk)
        a, pv = np.exp(mo - mn), np.exp(sk - mn)
        l[..., :n] = l[..., :n] * a + pv
        ao = np.ones_like(a) if skip_rescale else a
        o[..., :n, :] = o[..., :n, :] * ao[..., None] + pv[..., None] * V[..., k0:k0 + n, :]
        m[..., :n] = mn
    return m, l, o


def _merge(m, l, o):
    """the slots of a wave by the butterfly, then the four waves in order -> (o [..., hd], m, l), un-normalised"""
    lead, ns, hd = m.shape[:-1], m.shape[-1], o.shape[-1]
    w = ns // 4
    m, l, o = m.reshape(lead + (4, w)), l.reshape(lead + (4, w)), o.reshape(lead + (4, w, hd))
    mw = m.max(-1)
    f = np.exp(m - mw[..., None])
    lw, ow = _tree(l * f), _tree(o * f[..., None], axis=-2)
    mt = mw.max(-1)
    fw = np.exp(mw - mt[..., None])
    lt = ((lw[..., 0] * fw[..., 0] + lw[..., 1] * fw[..., 1]) + lw[..., 2] * fw[..., 2]) + lw[..., 3] * fw[..., 3]
    ot = ((ow[..., 0, :] * fw[..., 0, None] + ow[..., 1, :] * fw[..., 1, None]) + ow[..., 2, :] * fw[..., 2, None]) + \
        ow[..., 3, :] * fw[..., 3, None]
    return ot, mt, lt


def _state(s, V, begin, end, nslot, mut):
    o, m, l = _merge(*_walk(s, V, begin, max(begin, end), nslot, mut == "skip_rescale"))
    if mut == "empty_m0" and end <= begin:
        m = np.zeros_like(m)
    return o, m, l


def _combine(states, mut):
    mt = states[0][1]
    for _, m, _ in states[1:]:
        mt = np.maximum(mt, m)
    if mut == "combine_skips_state63" and len(states) == 64:
        states = states[:63]
    lt, acc = np.zeros_like(mt), np.zeros_like(states[0][0])
    for o, m, l in states:
        f = np.exp(m - mt)
        lt = lt + l * f
        acc = acc + o * f[..., None]
    return acc * (F32(1.0) / lt)[..., None]


def _mutate_ranges(ranges, mut):
    """ranges: [(begin, end)] of one walk over keys 0 .. L - 1, in split order"""
    full = [i for i, (b, e) in enumerate(ranges) if e > b]
    out = list(ranges)
    if mut == "drop_split_end" and len(full) > 1:
        b, e = out[full[0]]
        out[full[0]] = (b, e - 1)
    if mut == "range_start_off_by_one" and len(full) > 1:
        b, e = out[full[1]]
        out[full[1]] = (b - 1, e)
    return out


def applies(c, mut):
    """whether the mutation changes anything the case computes"""
    if mut is None:
        return True
    if c["route"] not in MUTATIONS[mut]:
        return False
    if mut == "truncate_out":
        return c["dtype"] == "bf16"
    if mut == "combine_skips_state63":
        return c["nsp"] + c["nso"] == 64
    if mut == "swap_query_slots":
        return c["group"] >= 3
    if mut == "ragged_store_last_row":
        return c["group"] % QT != 0 and c["groups"] > 1
    if mut == "empty_m0":
        return "empty_splits" in features(c)
    if mut in ("drop_split_end", "range_start_off_by_one"):
        if c["route"] == "split":
            return sum(e > b for b, e in split_ranges(c["S"], c["nsplit"])) > 1
        return sum(e > b for b, e in split_ranges(c["plen"], c["nsp"])) > 1 or sum(e > b for b, e in split_ranges(c["own"], c["nso"])) > 1
    if mut == "swap_v_rows":
        return c["past"] + 1 >= 2
    if mut == "next_head_k_unit":
        return c["nsl"] * c["H"] > 1
    return True


def model(c, ins, mut=None, cast=True):
    """what a correct kernel computes, in numpy float32 -> [slices, H, nq, hd] float32; ``mut`` plants one defect; cast=False: the fp32
    value before the store's rounding to bf16"""
    bf = c["dtype"] == "bf16"
    g = geom(c["route"], c["dtype"], c["hd"])
    q, K, V = (ins[n].astype(F32) for n in ("q", "k", "v"))
    scale = F32(ins["scale"])
    nsl, H, S, hd = q.shape
    if mut == "next_head_k_unit":
        K = K.copy()
        K[..., :g["epu"]] = np.roll(K[..., :g["epu"]], -1, axis=1 if H > 1 else 0)
    if mut == "swap_v_rows" and c["past"] + 1 >= 2:
        a = min(40, c["past"] - 1)
        V = V.copy()
        V[:, :, [a, a + 1]] = V[:, :, [a + 1, a]]
    out = np.zeros((nsl, H, c["nq"], hd), dtype=F32)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        for iq in range(c["nq"]):
            row = c["past"] + iq
            L = row + 1
            Lm = L - 1 if mut == "drop_last_key" else L
            qf = q[:, :, row] * scale
            if c["route"] == "unsplit":
                o, _, l = _state(_scores(c, qf, K[:, :, :L]), V, 0, Lm, NT, mut)
                y = o * (F32(1.0) / l)[..., None]
            elif c["route"] == "split":
                s = _scores(c, qf, K[:, :, :L])
                rng = _mutate_ranges(split_ranges(L, c["nsplit"]), mut)
                rng = [(b, min(e, Lm)) for b, e in rng]
                y = _combine([_state(s, V, b, e, g["slots"], mut) for b, e in rng], mut)
            else:
                plen, own, group = c["plen"], c["own"], c["group"]
                src = np.arange(nsl)                 # the row whose query a row's prompt states are computed with
                for gi in range(c["groups"]):
                    if mut == "swap_query_slots":
                        for t in range(0, group, QT):
                            if t + 2 < group:
                                src[gi * group + t + 1], src[gi * group + t + 2] = gi * group + t + 2, gi * group + t + 1
                    if mut == "ragged_store_last_row" and group % QT:
                        src[gi * group + group - 1] = (gi * group + group) % nsl
                sp = _scores(c, qf[src], K[:, :, :plen])
                so = _scores(c, qf, K[:, :, plen:L])
                rp = _mutate_ranges(split_ranges(plen, c["nsp"]), mut)
                ro = _mutate_ranges(split_ranges(own, c["nso"]), mut)
                ro = [(b, min(e, Lm - plen)) for b, e in ro]
                st = [_state(sp, V[:, :, :plen], b, e, g["slots"], mut) for b, e in rp]
                st += [_state(so, V[:, :, plen:L], b, e, g["slots"], mut) for b, e in ro]
                y = _combine(st, mut)
            out[:, :, iq] = y
    if bf and cast:
        out = CHK.bf16_trunc(out) if mut == "truncate_out" else CHK.bf16_round(out)
    return out


# --------------------------------------------------------------------------- #
# GPU: every form of a case
# --------------------------------------------------------------------------- #
def run(c, ins):
    """-> ({form: y [slices, H, nq, hd] float64}, {form: kernel name as mas_last_kernel gave it}); forms: "host", and "dev" where the
    case has one query.  Every cache row past the valid length, the memory around strided rows and around the prompt blocks, the
    outputs and the workspaces hold NaN before the call; so does the cache row the device form appends."""
    import torch
    from mas_hip import _DT, _ptr, _stream, check, decode, lib, ops
    dev = torch.device("cuda:0")
    nsl, H, S, hd, past, nq = c["nsl"], c["H"], c["S"], c["hd"], c["past"], c["nq"]
    d = H * hd
    tdt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
    nan = float("nan")
    scale = float(ins["scale"])
    pack = lambda x: torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1, 3).reshape(nsl, x.shape[2], d))).to(tdt)   # exact
    unpack = lambda t: t.double().cpu().numpy().reshape(nsl, nq, H, hd).transpose(0, 2, 1, 3)
    past_t = torch.tensor([past], dtype=torch.int32, device=dev)
    kf, vf = pack(ins["k"]).to(dev), pack(ins["v"]).to(dev)                              # [slices, S, d]
    qkv = torch.cat([pack(ins["q"][:, :, past:past + nq]).to(dev), kf[:, past:past + nq], vf[:, past:past + nq]], dim=-1).contiguous()
    qs = qkv[..., :d]                                                                    # a strided view of the fused row
    got, kern = {}, {}

    def cache(x, valid, cap):
        t = torch.full((nsl, cap, d), nan, dtype=tdt, device=dev)
        t[:, :valid] = x[:, :valid]
        return t

    if c["route"] in ("unsplit", "split"):
        cap = S + 3
        kc, vc = cache(kf, S, cap), cache(vf, S, cap)
        o = torch.full((nsl, nq, d), nan, dtype=tdt, device=dev)
        if c["route"] == "split":
            n = c["nsplit"]
            ws = torch.full((nsl * H * n * (hd + 2),), nan, dtype=torch.float32, device=dev)
            check(lib().mas_attn_decode_split(_ptr(qs), _ptr(kc), _ptr(vc), _ptr(o), _DT[tdt], nsl, H, 1, past, hd, qs.stride(1), kc.stride(1),
                                              vc.stride(1), o.stride(1), qs.stride(0), kc.stride(0), vc.stride(0), o.stride(0), scale, n,
                                              _ptr(ws), ws.numel(), _stream()), "attn_decode_split")
        elif c["layout"] == "strided":
            # q inside the fused row; k and v rows with token and batch strides of their own, NaN in between
            lds, bss = (d + 8, d + 16), (cap * (d + 8) + 16, cap * (d + 16) + 8)
            bufs = []
            for x, ld, bs in zip((kf, vf), lds, bss):
                buf = torch.full((nsl * bs,), nan, dtype=tdt, device=dev)
                buf.as_strided((nsl, S, d), (bs, ld, 1)).copy_(x)
                bufs.append(buf)
            check(lib().mas_attn_decode(_ptr(qs), _ptr(bufs[0]), _ptr(bufs[1]), _ptr(o), _DT[tdt], nsl, H, nq, past, hd, qs.stride(1), lds[0],
                                        lds[1], o.stride(1), qs.stride(0), bss[0], bss[1], o.stride(0), scale, _stream()), "attn_decode")
        else:
            o = ops.attention_decode(qs.contiguous(), kc, vc, past, H)
        kern["host"] = ops.last_kernel()
        got["host"] = unpack(o)
        if has_dev(c):
            kd, vd = cache(kf, past, cap), cache(vf, past, cap)                          # row `past` is NaN: the kernel appends it
            od = torch.full((nsl, 1, d), nan, dtype=tdt, device=dev)
            if c["route"] == "split" and c["nsplit"] == 1:                               # the wrapper sends one split to the unsplit kernel
                ws = torch.full((nsl * H * (hd + 2),), nan, dtype=torch.float32, device=dev)
                check(lib().mas_attn_decode_split_dev(_ptr(qs), _ptr(qkv[..., d:2 * d]), _ptr(qkv[..., 2 * d:]), qkv.stride(0), _ptr(kd),
                                                      _ptr(vd), kd.stride(1), kd.stride(0), cap, _ptr(od), od.stride(0), _DT[tdt], nsl, H, hd,
                                                      _ptr(past_t), scale, 1, _ptr(ws), ws.numel(), _stream()), "attn_decode_split_dev")
            else:
                decode.attention_decode_dev(qkv, kd, vd, past_t, H, out=od, kv_splits=c.get("nsplit"))
            kern["dev"] = ops.last_kernel()
            got["dev"] = unpack(od)
    else:
        plen, own, group, groups = c["plen"], c["own"], c["group"], c["groups"]
        cap = own + 3
        first = torch.arange(groups, device=dev) * group
        blocks = []
        for x in (kf, vf):                           # the prompt blocks: views into a larger NaN-filled buffer
            big = torch.full((groups, plen + 4, d), nan, dtype=tdt, device=dev)
            big[:, 2:2 + plen] = x[first, :plen]
            blocks.append(big[:, 2:2 + plen])
        pk, pv = blocks
        ko, vo = kf[:, plen:], vf[:, plen:]
        o = ops.attention_decode_shared(qs, pk, pv, cache(ko, own, cap), cache(vo, own, cap), past, H, group=group, prompt_splits=c["nsp"],
                                        kv_splits=c["nso"])
        kern["host"] = ops.last_kernel()
        got["host"] = unpack(o)
        od = torch.full((nsl, 1, d), nan, dtype=tdt, device=dev)
        decode.attention_decode_shared_dev(qkv, pk, pv, cache(ko, own - 1, cap), cache(vo, own - 1, cap), past_t, H, group=group,
                                           prompt_splits=c["nsp"], kv_splits=c["nso"], out=od)
        kern["dev"] = ops.last_kernel()
        got["dev"] = unpack(od)
    torch.cuda.synchronize()
    return got, kern
