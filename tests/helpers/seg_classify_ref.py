"""The rule that turns VQ-SEG logits into label planes, restated in numpy as a channel-by-channel scan, the reference
Visualizer's own expression (log_utils.py:55-67) restated in torch, the inputs the tests of the rule share, and brute-force agreement counts.

For a layout with planes k = 0 .. P-1 and per-plane thresholds t_k (None, or a probability in (0, 1)):
    tau_k = float32(log(t_k / (1 - t_k))) computed in double and rounded once; -inf for None
    class plane (S channels from `base`): m = the largest logit, a = the FIRST channel that holds it (a scan in channel order with a
        strict `>`: torch.argmax's rule); byte = a - base + 1 if m > tau_k else 0
    value plane (one channel): byte = 1 if x > tau_k else 0
Logits are compared as float32; bfloat16 widens exactly, so nothing is rounded anywhere and an implementation must give these bytes
exactly on every input without NaN (+-inf order as values)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

REFERENCE_THRESHOLDS = (None, None, 0.2, 0.2)


def taus(thresholds):
    return [np.float32(-np.inf) if t is None else np.float32(math.log(t / (1.0 - t))) for t in thresholds]


def classify(x: np.ndarray, groups, value_channels, thresholds) -> np.ndarray:
    """x float32 [N, C, H, W] -> uint8 [N, P, H, W]"""
    assert x.dtype == np.float32 and x.ndim == 4
    tau = taus(thresholds)
    n, c, h, w = x.shape
    assert c == sum(groups) + value_channels and len(tau) == len(groups) + value_channels
    out = np.zeros((n, len(tau), h, w), dtype=np.uint8)
    base = 0
    for k, size in enumerate(groups):
        m = x[:, base].copy()
        a = np.zeros((n, h, w), dtype=np.int64)
        for j in range(1, size):
            better = x[:, base + j] > m
            m = np.where(better, x[:, base + j], m)
            a = np.where(better, j, a)
        out[:, k] = np.where(m > tau[k], a + 1, 0).astype(np.uint8)
        base += size
    for v in range(value_channels):
        out[:, len(groups) + v] = (x[:, base + v] > tau[len(groups) + v]).astype(np.uint8)
    return out


def visualizer_labels(x: torch.Tensor) -> np.ndarray:
    """What reference log_utils.py:55-67 computes for logits of the reference layout, read back as a label byte: per group the one-hot of
    the slice argmax, for the face and edge groups multiplied by `sigmoid(slice) > 0.2`; the byte is the one-hot's channel + 1, or 0 where
    the product left it all zero.  x: float32 or bfloat16 [N, 159, H, W]; argmax and sigmoid run in x's dtype, as they would there."""
    bounds = ((0, 133, False), (133, 153, False), (153, 158, True), (158, 159, True))      # panoptic, human parts, face, edges
    planes = []
    for lo, hi, gated in bounds:
        part = x[:, lo:hi]
        hot = F.one_hot(part.argmax(dim=1), num_classes=hi - lo).movedim(-1, 1).float()
        if gated:
            hot = hot * (torch.sigmoid(part) > 0.2)
        assert float(hot.sum(1).max()) <= 1.0
        classes = torch.arange(1, hi - lo + 1, dtype=torch.float32).view(1, -1, 1, 1)
        planes.append((hot * classes).sum(1).to(torch.uint8))
    return torch.stack(planes, 1).numpy()


def tie_rich_logits(shape, groups, value_channels, thresholds, scale, seed, bf16=False, shift_group=None, clear=0.0):
    """logits quantised to multiples of 0.5 (ties are frequent): scale * randn rounded to the grid; `shift_group`: that group moved by -3 so
    that "none" and every class occur under a gate; `clear` > 0: entries within `clear` of a plane's tau are moved to tau + 0.5 (the
    comparison with the sigmoid form is only made away from tau).  -> float32 numpy (a bfloat16-representable one with bf16)"""
    n, c, h, w = shape
    rs = np.random.RandomState(seed)
    x = (np.round(scale * rs.randn(n, c, h, w) * 2.0) / 2.0).astype(np.float32)
    bases = np.concatenate([[0], np.cumsum(list(groups) + [1] * value_channels)])
    if shift_group is not None:
        x[:, bases[shift_group]:bases[shift_group + 1]] -= 3.0
    if clear > 0.0:
        for k, tau in enumerate(taus(thresholds)):
            if np.isfinite(tau):
                s = x[:, bases[k]:bases[k + 1]]
                s[np.abs(s - tau) < clear] = np.float32(tau) + np.float32(0.5)
    if bf16:
        x = torch.from_numpy(x).bfloat16().float().numpy()
    return x


def hard_logits(shape, seed):
    """logits to +-150 with +inf and -inf sprinkled in (no NaN)"""
    rs = np.random.RandomState(seed)
    x = (2.0 * rs.randn(*shape)).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] *= 40.0
    flat[3::13] = np.inf
    flat[5::17] = -np.inf
    return x


def agreement_counts(pred: np.ndarray, target: np.ndarray, groups, value_channels) -> np.ndarray:
    """uint8 [N, P, H, W] twice -> int64 [3 C + P + 1] = inter[C], pred[C], target[C], agree[P], pixels"""
    c = sum(groups) + value_channels
    p = len(groups) + value_channels
    out = np.zeros(3 * c + p + 1, dtype=np.int64)
    base = 0
    for k, size in enumerate(groups):
        pv = np.where((pred[:, k] >= 1) & (pred[:, k] <= size), pred[:, k], 0)
        tv = np.where((target[:, k] >= 1) & (target[:, k] <= size), target[:, k], 0)
        for v in range(1, size + 1):
            out[base + v - 1] = np.count_nonzero((pv == v) & (tv == v))
            out[c + base + v - 1] = np.count_nonzero(pv == v)
            out[2 * c + base + v - 1] = np.count_nonzero(tv == v)
        out[3 * c + k] = np.count_nonzero(pv == tv)
        base += size
    for v in range(value_channels):
        k = len(groups) + v
        pb, tb = pred[:, k] > 0, target[:, k] > 0
        out[base + v], out[c + base + v], out[2 * c + base + v] = np.count_nonzero(pb & tb), np.count_nonzero(pb), np.count_nonzero(tb)
        out[3 * c + k] = np.count_nonzero(pb == tb)
    out[-1] = pred.shape[0] * pred.shape[2] * pred.shape[3]
    return out
