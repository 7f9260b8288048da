"""float64 numpy restatement of the stage-2 read-out (``mas_token_readout`` / ``mas_token_readout_accumulate``) and the case
list that tests/test_gpu_token_readout.py runs on the GPU and tests/test_token_readout_cpu.py checks against torch on the CPU first.

The reference works on exactly the values the kernel reads: ``make_case`` rounds the inputs to the case's dtype before widening them.
The shapes and layouts are the ones tests/helpers/token_ce_ref.py established for this row walk."""
import numpy as np
import torch

IGNORE = -100
VS = (1, 7, 8, 255, 2048, 2049, 8192, 8200)     # no unit | tail only | one unit | units + tail | one unit per lane | +1 | resident limit | past it
ROWS = (1, 3, 257)
HARD = ("max_last", "const", "dominant", "big1e4", "wide3e3", "neginf", "neginf_target", "all_neginf", "nan_row", "posinf_row", "ignored",
        "all_ignored", "bad_targets", "ties")
MAX_KS = 8
RANK_BINS = 33


def readout_ref(x, target, ignore_index=IGNORE):
    """x float64 [rows, V], target int64 [rows] -> (nll f64, entropy f64, argmax i64, rank i64), each [rows], by the rules of the header:
    ignored rows 0, 0, -1, -1; invalid rows (another target outside [0, V), a NaN or +inf in the row, a row of -inf alone) NaN, NaN, -1, V"""
    x = np.asarray(x, dtype=np.float64)
    rows, v = x.shape
    t = np.asarray(target, dtype=np.int64)
    nll, ent = np.zeros(rows), np.zeros(rows)
    arg, rank = np.full(rows, -1, dtype=np.int64), np.full(rows, -1, dtype=np.int64)
    for r in range(rows):
        if t[r] == ignore_index:
            continue
        xr = x[r]
        if t[r] < 0 or t[r] >= v or np.isnan(xr).any() or (xr == np.inf).any() or (xr == -np.inf).all():
            nll[r] = ent[r] = np.nan
            rank[r] = v
            continue
        m = xr.max()
        d = xr - m
        e = np.exp(d)
        l = e.sum()
        logl = np.log(l)
        xt = xr[t[r]]
        nll[r] = (m - xt) + logl                                 # x_t = -inf: +inf
        fin = d != -np.inf
        ent[r] = logl - (e[fin] * d[fin]).sum() / l              # an entry of -inf adds 0
        arg[r] = int(np.argmax(xr))                              # numpy: the first index of the maximum
        rank[r] = int((xr > xt).sum() + (xr[:t[r]] == xt).sum())
    return nll, ent, arg, rank


def rank_bin(rank):
    """bin 0 = rank 0, bin b >= 1 = rank in [2^(b-1), 2^b)"""
    return 0 if rank <= 0 else int(rank).bit_length()


def accumulate_ref(nll, entropy, argmax, rank, target, positions, ks, ignore_index=IGNORE, into=None):
    """the per-row arrays (``nll`` / ``entropy`` as the float32 values a kernel produced, or float64) -> dict of nll_sum f64 [L],
    entropy_sum f64 [L], count i64 [L], hits i64 [L, nk], rank_hist i64 [33], invalid i64 [1]: per position a local fp64 sum from 0 over
    r = p, p + L, ... in increasing r (counted rows), added ONCE to what ``into`` holds"""
    rows, L, nk = len(target), int(positions), len(ks)
    assert rows % L == 0 and 1 <= nk <= MAX_KS and all(k >= 1 for k in ks)
    acc = into if into is not None else dict(nll_sum=np.zeros(L), entropy_sum=np.zeros(L), count=np.zeros(L, dtype=np.int64),
                                             hits=np.zeros((L, nk), dtype=np.int64), rank_hist=np.zeros(RANK_BINS, dtype=np.int64),
                                             invalid=np.zeros(1, dtype=np.int64))
    for p in range(L):
        sn, se = np.float64(0.0), np.float64(0.0)
        for r in range(p, rows, L):
            if target[r] == ignore_index:
                continue
            if argmax[r] < 0:
                acc["invalid"][0] += 1
                continue
            with np.errstate(invalid="ignore"):
                sn = sn + np.float64(nll[r])
                se = se + np.float64(entropy[r])
            acc["count"][p] += 1
            for i, k in enumerate(ks):
                acc["hits"][p, i] += int(rank[r] < k)
            acc["rank_hist"][rank_bin(rank[r])] += 1
        with np.errstate(invalid="ignore"):
            acc["nll_sum"][p] = acc["nll_sum"][p] + sn
            acc["entropy_sum"][p] = acc["entropy_sum"][p] + se
    return acc


def _cases():
    out = []
    for v in VS:                                 # every path x every row count; ignored rows in every other case with more than one row
        for k, rows in enumerate(ROWS):
            out.append(dict(kind="randn", v=v, rows=rows, layout="contig", ignore=rows > 1 and (k + v) % 2 == 0))
    for v in (7, 2049, 8192):                    # the [2, 3, V] slice of [2, 5, V], read in place
        out.append(dict(kind="randn", v=v, rows=6, layout="slice", ignore=True))
    for v in (255, 2048, 8200):                  # 4 bytes off a 16-byte boundary: the element-wise path
        out.append(dict(kind="randn", v=v, rows=3, layout="offset", ignore=False))
    for kind in HARD:
        for v in (255, 2049, 8200):
            out.append(dict(kind=kind, v=v, rows=5, layout="contig", ignore=kind in ("ignored", "all_ignored")))
    for c in out:
        c["id"] = "{kind}-V{v}-r{rows}-{layout}{ig}".format(ig="-ign" if c["ignore"] else "", **c)
    return out


CASES = _cases()


def make_case(case, dtype, seed=0):
    """-> (x32 [rows, V] float32 numpy holding values exactly representable in ``dtype``, target int64 [rows]): the inputs of one case,
    the same on every machine.  ``dtype`` torch.float32 or torch.bfloat16."""
    rows, v, kind = case["rows"], case["v"], case["kind"]
    rng = np.random.default_rng(1000 * seed + 7 * v + rows + (13 * (1 + HARD.index(kind)) if kind in HARD else 0))
    x = rng.standard_normal((rows, v)).astype(np.float32)
    t = rng.integers(0, v, size=rows).astype(np.int64)
    if kind == "max_last":                       # the maximum AND the target in the last element (the tail, where V has one)
        x[:, -1] = 9.0
        t[:] = v - 1
        x[0, -1] = -9.0                          # ... and one row whose target is last but far from the maximum
        x[1, -2] = 9.0                           # ... and one where the maximum occurs twice: argmax is the first
    elif kind == "const":                        # rank must equal t, argmax 0
        x[:] = 3.25
        x[1] = -1e4
        x[2] = 0.0
    elif kind == "dominant":                     # target = argmax by a wide margin: nll ~ 0, entropy ~ 0
        x[np.arange(rows), t] += 60.0
    elif kind == "big1e4":                       # m + log l would round to 1e-3 here
        x += 1e4
    elif kind == "wide3e3":                      # every exp but one underflows
        x *= 3e3
    elif kind in ("neginf", "neginf_target"):
        mask = rng.random((rows, v)) < 0.3
        mask[np.arange(rows), t] = kind == "neginf_target"       # x_t = -inf: valid, nll = +inf
        mask[np.arange(rows), (t + 1) % v] = False               # (one finite entry stays in every row; the hard cases have V >= 255)
        x[mask] = -np.inf
    elif kind == "all_neginf":                   # rows 1 and 3: invalid
        x[1] = -np.inf
        x[3] = -np.inf
    elif kind == "nan_row":                      # a NaN in a unit (row 0), in the last element (row 2), at the target (row 4)
        x[0, v // 3] = np.nan
        x[2, -1] = np.nan
        x[4, t[4]] = np.nan
    elif kind == "posinf_row":
        x[0, v // 3] = np.inf
        x[2, -1] = np.inf
        x[4, t[4]] = np.inf
    elif kind == "bad_targets":
        t[1], t[3] = -5, v
    elif kind == "ties":                         # the target's value at least 8 times on either side of t, and above the rest or not
        for r in range(rows):
            t[r] = v // 2 + r
            val = np.float32((-0.5, 0.0, 0.25, 1.0, 5.0)[r])
            left = rng.choice(t[r], size=min(8 + r, t[r]), replace=False)
            right = t[r] + 1 + rng.choice(v - t[r] - 1, size=min(9 + r, v - t[r] - 1), replace=False)
            x[r, left] = val
            x[r, right] = val
            x[r, t[r]] = val
    if case["ignore"]:
        t[::3] = IGNORE
    if kind == "all_ignored":
        t[:] = IGNORE
    x = torch.from_numpy(x).to(dtype).float().numpy()
    return x, t
