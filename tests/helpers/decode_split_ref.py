"""float64 numpy restatement of the split-key decode attention (make-a-scene_amd/csrc/attn_decode_split.hip): the key ranges the partial
kernel computes from L and nsplit, the un-normalised online-softmax state of a range, and the merge in split order -- the algebra the
kernel pair implements, and the GPU tests' second reference."""
import numpy as np

GRAN = 32          # a split's key range is a multiple of this many keys
NEUTRAL_M = -1e30  # the running maximum of a split without keys


def split_ranges(L, nsplit):
    """[(begin, end)] of every split for L visible keys: equal chunks of ceil(L / nsplit) keys rounded up to GRAN; empty when begin >= L"""
    chunk = (-(-L // nsplit) + GRAN - 1) // GRAN * GRAN
    return [(s * chunk, max(s * chunk, min(L, (s + 1) * chunk))) for s in range(nsplit)]


def partial_state(q, k, v, begin, end):
    """(m, l, o) of keys begin .. end-1: m the maximum score, l = sum exp(s - m), o = sum exp(s - m) v; the neutral state when empty.
    q [hd] (already scaled), k / v [L, hd]."""
    hd = q.shape[0]
    if end <= begin:
        return NEUTRAL_M, 0.0, np.zeros(hd)
    s = k[begin:end].astype(np.float64) @ q.astype(np.float64)
    m = float(s.max())
    p = np.exp(s - m)
    return m, float(p.sum()), p @ v[begin:end].astype(np.float64)


def combine(states):
    """the context row from the states, merged in split order"""
    mt = max(m for m, _, _ in states)
    lt, acc = 0.0, np.zeros_like(states[0][2])
    for m, l, o in states:
        f = np.exp(m - mt)
        lt += l * f
        acc = acc + o * f
    return acc / lt


def split_attention(q, k, v, nsplit):
    """q [hd] (scaled), k / v [L, hd] float -> softmax(k q) v computed split by split (float64)"""
    return combine([partial_state(q, k, v, b, e) for b, e in split_ranges(k.shape[0], nsplit)])


def plain_attention(q, k, v):
    s = k.astype(np.float64) @ q.astype(np.float64)
    p = np.exp(s - s.max())
    return (p / p.sum()) @ v.astype(np.float64)
