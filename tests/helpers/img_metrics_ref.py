"""numpy restatement of the VQ-IMG read-out (csrc/img_metrics.hip): the byte rule emulated exactly in ``np.float32``, the
integer squared error, SSIM in float64 by the definition, and the codebook counts.  Nothing here imports the package under test."""
import numpy as np

WINDOW, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def window():
    """g[i] = exp(-(i - 5)^2 / (2 1.5^2)), i = 0 .. 10, normalised to sum 1 (float64)"""
    g = np.exp(-((np.arange(WINDOW, dtype=np.float64) - WINDOW // 2) ** 2) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def to_bytes(x, lo=-1.0, hi=1.0):
    """float image [N, C, H, W] (float32; a bf16 image widened exactly) -> uint8 [N, H, W, C].  s = float32(255 / (hi - lo)) formed in double
    and rounded once; t = (x - lo) * s as two fp32 operations; clamp to [0, 255] with NaN -> 0 (np.fmax / np.fmin return the operand that
    is not a NaN); np.rint rounds half to even."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4
    s = np.float32(255.0 / (float(hi) - float(lo)))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - np.float32(lo)).astype(np.float32) * s
        assert t.dtype == np.float32
        t = np.fmin(np.fmax(t, np.float32(0.0)), np.float32(255.0))
    return np.ascontiguousarray(np.rint(t).astype(np.uint8).transpose(0, 2, 3, 1))


def sse(a, b):
    """uint8 [N, H, W, C] x 2 -> int64 [N]"""
    d = a.astype(np.int64) - b.astype(np.int64)
    return (d * d).reshape(d.shape[0], -1).sum(axis=1)


def _windowed(v, g):
    """[N, H, W, C] float64 -> the "valid" separable sums [N, H - 10, W - 10, C]: horizontal taps, then vertical"""
    n, h, w, c = v.shape
    hs = np.zeros((n, h, w - WINDOW + 1, c))
    for i in range(WINDOW):
        hs += g[i] * v[:, :, i:i + w - WINDOW + 1]
    out = np.zeros((n, h - WINDOW + 1, w - WINDOW + 1, c))
    for j in range(WINDOW):
        out += g[j] * hs[:, j:j + h - WINDOW + 1]
    return out


def ssim_map(a, b):
    a, b, g = a.astype(np.float64), b.astype(np.float64), window()
    ma, mb = _windowed(a, g), _windowed(b, g)
    va, vb, vab = _windowed(a * a, g) - ma * ma, _windowed(b * b, g) - mb * mb, _windowed(a * b, g) - ma * mb
    return ((2.0 * ma * mb + C1) * (2.0 * vab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))


def ssim(a, b):
    """uint8 [N, H, W, C] x 2 -> float64 [N]: the mean of the map over channels and window positions; NaN when H or W is below 11"""
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
    n, h, w, _ = a.shape
    if h < WINDOW or w < WINDOW:
        return np.full(n, np.nan)
    return ssim_map(a, b).reshape(n, -1).mean(axis=1)


def psnr(sse_, elements):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(255.0 ** 2 / (sse_.astype(np.float64) / elements))


def code_usage(indices, n_embed):
    """-> int64 [K + 1]: np.bincount of the indices inside [0, K), and in the last slot the number outside"""
    idx = np.asarray(indices).reshape(-1).astype(np.int64)
    ok = (idx >= 0) & (idx < n_embed)
    return np.concatenate([np.bincount(idx[ok], minlength=n_embed), [np.count_nonzero(~ok)]]).astype(np.int64)


def perplexity(counts):
    p = counts[:-1].astype(np.float64) / counts[:-1].sum()
    p = p[p > 0]
    return float(np.exp(-(p * np.log(p)).sum()))


def tie_grid(shape, seed):
    """float32 multiples of 0.5 in [-2, 257.5]: with (lo, hi) = (0, 255) the scale is 1 and every second value is a rounding tie"""
    rs = np.random.RandomState(seed)
    return (rs.randint(-4, 516, shape) * 0.5).astype(np.float32)


def hard_values(shape, seed):
    """uniform values with NaN, +-inf and +-1e30 strewn in"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1.5, 1.5, shape).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], dtype=np.float32)
    pos = rs.randint(0, flat.size, max(5, flat.size // 7))
    flat[pos] = special[np.arange(pos.size) % special.size]
    return x


def fp32_probe(size=64, seed=0):
    """Why the kernel sums in fp64 -- not run by the suite; call it by hand.  The same separable sums with float32 weights, products and
    accumulators against float64, on flat bright pictures: the image's SSIM is off by up to 7e-5 (constant 255 against 254; 250 +- 1
    noise), with or without centring the bytes, because float32 weights do not sum to 1 and the variance of a constant is then not 0.
    Random noise and sharp edges stay below 2e-6.  -> {case: |ssim32 - ssim64|}"""
    rs = np.random.RandomState(seed)
    cases = {"255 vs 254": (np.full((1, size, size, 1), 255, np.uint8), np.full((1, size, size, 1), 254, np.uint8)),
             "250 +- 1": tuple((250 + rs.randint(-1, 2, (1, size, size, 1))).astype(np.uint8) for _ in range(2)),
             "noise": tuple(rs.randint(0, 256, (1, size, size, 1)).astype(np.uint8) for _ in range(2))}
    g32 = window().astype(np.float32)

    def win32(v):
        n, h, w, c = v.shape
        hs = np.zeros((n, h, w - WINDOW + 1, c), np.float32)
        for i in range(WINDOW):
            hs += g32[i] * v[:, :, i:i + w - WINDOW + 1]
        out = np.zeros((n, h - WINDOW + 1, w - WINDOW + 1, c), np.float32)
        for j in range(WINDOW):
            out += g32[j] * hs[:, j:j + h - WINDOW + 1]
        return out

    report = {}
    for name, (a, b) in cases.items():
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        ma, mb = win32(a32), win32(b32)
        va, vb, vab = win32(a32 * a32) - ma * ma, win32(b32 * b32) - mb * mb, win32(a32 * b32) - ma * mb
        c1, c2 = np.float32(C1), np.float32(C2)
        m32 = ((2 * ma * mb + c1) * (2 * vab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
        report[name] = abs(float(m32.astype(np.float64).mean()) - float(ssim(a, b)[0]))
    return report
