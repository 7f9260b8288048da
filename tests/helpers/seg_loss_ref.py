"""The VQ-SEG objective in float64 numpy -- what ``mas_hip.ops.seg_loss`` (csrc/seg_loss.hip) is checked against.  For x = prediction
logits [N, C, H, W], t = target, w = pos_weight [C], n = x.size and an upstream gradient g:

    lw   = 1 + (w[c] - 1) t
    bce  = (1 - t) x + lw softplus(-x)          softplus(-x) = max(-x, 0) + log1p(exp(-|x|))
    mse  = (sigmoid(x) - t)^2                   sigmoid from the same e = exp(-|x|): no overflow either side
    loss = mean(bce) + mse_on mean(mse)
    dx   = g / n [ (1 - t) - lw (1 - sigmoid(x)) + mse_on 2 (sigmoid(x) - t) sigmoid(x) (1 - sigmoid(x)) ]

tests/test_seg_loss_cpu.py pins this to tests/golden/loss_seg.npz, which the reference's own classes made."""
import numpy as np

HEAVY = (153, 158)            # the module's vector: 20 on channels 153..157, 1 elsewhere
HEAVY_WEIGHT = 20.0


def module_weight(c=159):
    w = np.ones(c, dtype=np.float64)
    w[HEAVY[0]:HEAVY[1]] = HEAVY_WEIGHT
    return w


def seg_loss_ref(x, t, w, mse, g=1.0):
    """-> (loss, bce_mean, mse_mean, dx), all float64; x, t [N, C, H, W] in logical order (any memory layout), w [C]"""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(1, -1, 1, 1)
    assert x.ndim == 4 and x.shape == t.shape and w.shape[1] == x.shape[1]
    e = np.exp(-np.abs(x))
    sig = np.where(x >= 0, 1.0, e) / (1.0 + e)
    oms = np.where(x >= 0, e, 1.0) / (1.0 + e)               # 1 - sigmoid, without the cancellation
    lw = 1.0 + (w - 1.0) * t
    bce = (1.0 - t) * x + lw * (np.maximum(-x, 0.0) + np.log1p(e))
    sq = (sig - t) ** 2
    bce_mean, mse_mean = float(bce.mean()), float(sq.mean()) if mse else 0.0
    d = (1.0 - t) - lw * oms
    if mse:
        d = d + 2.0 * (sig - t) * sig * oms
    return bce_mean + mse_mean, bce_mean, mse_mean, float(g) / x.size * d
