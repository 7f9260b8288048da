"""numpy restatement of the on-device sampler (``mas_sample_tokens``, make-a-scene_amd/csrc/decode_step.hip) and of its random mapping
(include/mas_hip.h, "Sampling"; make-a-scene_amd/csrc/mas_philox.h ``mas_sample_bits4`` / ``mas_sample_uniform``)."""
import numpy as np

import philox_ref as R


def sample_bits(seed, offset, row, step, j):
    """the 32-bit word behind u_j of output row ``row`` at decode step ``step`` (arrays broadcast together)"""
    k0, k1, off = R.split_seed(seed, offset)
    row, step, j = (np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(row, step, j))
    words = R.philox4x32_10(j >> np.uint64(2), step, row, off, k0, k1)
    slot = (j & np.uint64(3)).astype(np.int64)
    return np.choose(slot, words).astype(np.uint32)


def uniform(bits):
    """u = ((bits >> 9) + 0.5) * 2^-23: exact in float32 and float64 alike (at most 24 significant bits), in [2^-24, 1 - 2^-24]"""
    return ((np.asarray(bits, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def mix(lc, lu=None, cond_scale=None):
    """the guidance mix in the eager code's fp32 operations: lu + s * (lc - lu), each rounded to float32"""
    lc = np.asarray(lc, dtype=np.float32)
    if lu is None or cond_scale is None:
        return lc
    lu = np.asarray(lu, dtype=np.float32)
    return (lu + np.float32(cond_scale) * (lc - lu)).astype(np.float32)


def kept(lg, top_k):
    """the entries ``lg.masked_fill(lg < kth, -inf)`` leaves finite: lg >= the top_k-th largest value (ties at it are kept)"""
    lg = np.asarray(lg, dtype=np.float32)
    if not top_k or top_k >= lg.shape[-1]:
        return np.ones(lg.shape, dtype=bool)
    kth = np.sort(lg)[::-1][top_k - 1]
    return lg >= kth


def gumbel_scores(lg, keep, u):
    """float64 perturbed scores lg_j - log(-log u_j) over the kept entries (-inf elsewhere)"""
    s = np.asarray(lg, dtype=np.float64) - np.log(-np.log(np.asarray(u, dtype=np.float64)))
    return np.where(keep, s, -np.inf)


def select(lc, lu=None, cond_scale=None, temperature=1.0, top_k=None, u=None):
    """the token of one row and the margin between its two best perturbed scores (inf for greedy).  temperature 0: the first index of
    the maximum of the mixed logits (torch.argmax); else Gumbel-max over lg = l / T restricted to the top-k with uniforms ``u``."""
    lmix = mix(lc, lu, cond_scale)
    if temperature == 0:
        return int(np.argmax(lmix)), np.inf
    lg = (lmix / np.float32(temperature)).astype(np.float32)
    s = gumbel_scores(lg, kept(lg, top_k), u)
    order = np.argsort(-s, kind="stable")
    return int(order[0]), float(s[order[0]] - s[order[1]]) if s.shape[-1] > 1 else np.inf


def select_rows(lc, lu, cond_scale, temperature, top_k, seed, offset, rows, step):
    """``select`` for output rows 0 .. rows-1 sharing one logits row pair, uniforms from the Sampling mapping -> (tokens, margins)"""
    v = np.asarray(lc).shape[-1]
    toks, gaps = np.empty(rows, dtype=np.int64), np.empty(rows)
    j = np.arange(v, dtype=np.uint64)
    for r in range(rows):
        toks[r], gaps[r] = select(lc, lu, cond_scale, temperature, top_k, uniform(sample_bits(seed, offset, r, step, j)))
    return toks, gaps
