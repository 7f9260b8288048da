"""numpy restatement of the nucleus (top-p) rule of the sampler (include/mas_hip.h "Top-p"; ``MakeAScene.generate(top_p=p)``), on top of
``sample_ref``: with K the set top-k keeps and q the float64 softmax of lg over K, entry j stays iff j is in K and the q-mass of the
entries of K with a strictly larger value is <= top_p."""
import numpy as np

import sample_ref as S


def cumulative(lg, top_k=None):
    """(K, values, excl, incl): the top-k mask, the distinct values of lg over K in descending order, and for each of them the float64
    softmax mass over K of the strictly larger values and of the values at or above it"""
    lg = np.asarray(lg, dtype=np.float32)
    in_k = S.kept(lg, top_k)
    x = lg[in_k].astype(np.float64)
    top = x.max()
    w = np.exp(x - top) if np.isfinite(top) else np.where(x == top, 1.0, 0.0)
    vals, inverse = np.unique(x, return_inverse=True)
    mass = np.bincount(inverse, weights=w, minlength=len(vals))[::-1] / w.sum()
    incl = np.cumsum(mass)
    return in_k, vals[::-1], incl - mass, incl


def kept_p(lg, top_k, top_p):
    """(mask, p-margin).  mask: the entries the rule keeps (top_p None or >= 1: what top-k keeps).  p-margin: the smallest |c - top_p|
    over all exclusive and inclusive cumulative masses c at distinct values -- how far top_p is from a place where the set changes (the
    sampler's own summation may land on the other side of top_p when this is within its rounding error)."""
    lg = np.asarray(lg, dtype=np.float32)
    in_k, vals, excl, incl = cumulative(lg, top_k)
    if top_p is None or not top_p < 1:
        return in_k, np.inf
    t = vals[excl <= top_p].min()                    # excl[0] = 0: never empty for top_p >= 0; upward closed, so a threshold value
    margin = float(np.abs(np.concatenate([excl, incl]) - float(top_p)).min())
    return in_k & (lg.astype(np.float64) >= t), margin


def midpoint_p(lg, top_k, n):
    """the float32 midway between the (n-1)-th and the n-th inclusive cumulative mass of the sorted entries (tie-free rows): the
    top_p that keeps exactly n entries, as far from both neighbours as it can be"""
    _, _, _, incl = cumulative(lg, top_k)
    lo = incl[n - 2] if n >= 2 else 0.0
    return float(np.float32(0.5 * (lo + incl[n - 1])))


def select_p(lc, lu=None, cond_scale=None, temperature=1.0, top_k=None, top_p=None, u=None):
    """``sample_ref.select`` with the top-p mask: the token of one row and the gap between its two best perturbed scores"""
    lmix = S.mix(lc, lu, cond_scale)
    if temperature == 0:
        return int(np.argmax(lmix)), np.inf
    lg = (lmix / np.float32(temperature)).astype(np.float32)
    s = S.gumbel_scores(lg, kept_p(lg, top_k, top_p)[0], u)
    order = np.argsort(-s, kind="stable")
    return int(order[0]), float(s[order[0]] - s[order[1]]) if s.shape[-1] > 1 else np.inf


def select_rows_p(lc, lu, cond_scale, temperature, top_k, top_p, seed, offset, rows, step):
    """``sample_ref.select_rows`` with the top-p mask -> (tokens, gaps)"""
    lmix = S.mix(lc, lu, cond_scale)
    lg = (lmix / np.float32(temperature)).astype(np.float32)
    keep = kept_p(lg, top_k, top_p)[0]
    v = lg.shape[-1]
    toks, gaps = np.empty(rows, dtype=np.int64), np.empty(rows)
    j = np.arange(v, dtype=np.uint64)
    for r in range(rows):
        s = S.gumbel_scores(lg, keep, S.uniform(S.sample_bits(seed, offset, r, step, j)))
        order = np.argsort(-s, kind="stable")
        toks[r] = order[0]
        gaps[r] = s[order[0]] - s[order[1]] if v > 1 else np.inf
    return toks, gaps
