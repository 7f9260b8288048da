"""numpy restatement of make-a-scene_amd/csrc/mas_philox.h: Philox4x32-10 and the dropout masks the kernels draw from it (the mapping
of include/mas_hip.h, "Dropout").  Vectorised over any number of counters; uint64 arithmetic, so no overflow warnings."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counters (arrays or scalars, broadcast together) and a key -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _MASK, p1 & _MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _MASK, p0 & _MASK]
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """t = round(p * 65536) on the float32 p the kernels receive; kept iff a 16-bit value >= t"""
    t = np.floor(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    return int(min(max(t, 0.0), 65536.0))


def scale(t):
    return 0.0 if t >= 65536 else float(np.float32(65536.0) / np.float32(65536 - t))


def split_seed(seed, offset):
    """the two int64 of the device seed tensor -> (key0, key1, counter word 3)"""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32, int(offset) & 0xFFFFFFFF


def attention_keep(seed, offset, B, H, S, p):
    """[B, H, S(query), S(key)] bool keep mask of the fused attention kernels (and of mas_attn_dropout_mask)"""
    k0, k1, off = split_seed(seed, offset)
    t = threshold(p)
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    q = np.arange(S, dtype=np.uint64)[None, :, None]
    k = np.arange(S, dtype=np.uint64)[None, None, :]
    r = philox4x32_10(k >> np.uint64(2), q >> np.uint64(1), bh, off, k0, k1)
    slot = (np.uint64(4) * (q & np.uint64(1)) + (k & np.uint64(3))) * np.ones_like(bh)
    word = np.choose((slot >> np.uint64(1)).astype(np.int64), r)
    u16 = (word >> ((slot & np.uint64(1)) * np.uint64(16)).astype(np.uint32)) & np.uint32(0xFFFF)
    return (u16 >= t).reshape(B, H, S, S)


def elementwise_keep(seed, offset, n, p):
    """[n] bool keep mask of mas_dropout_apply over a flat tensor of n elements (memory order)"""
    k0, k1, off = split_seed(seed, offset)
    t = threshold(p)
    i = np.arange(n, dtype=np.uint64)
    g = i >> np.uint64(3)
    r = philox4x32_10(g & _MASK, g >> np.uint64(32), 0, off, k0, k1)
    slot = i & np.uint64(7)
    word = np.choose((slot >> np.uint64(1)).astype(np.int64), r)
    u16 = (word >> ((slot & np.uint64(1)) * np.uint64(16)).astype(np.uint32)) & np.uint32(0xFFFF)
    return u16 >= t
