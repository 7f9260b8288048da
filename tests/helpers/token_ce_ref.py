"""float64 numpy reference of the token cross-entropy (``mas_hip.ops.cross_entropy``) and the case list that
tests/test_gpu_token_loss.py runs on the GPU and tests/test_token_loss_cpu.py checks against ``F.cross_entropy`` in float64 first.

The reference works on exactly the values the kernel reads: ``make_case`` rounds the inputs to the case's dtype before widening them."""
import numpy as np
import torch

IGNORE = -100
VS = (1, 7, 8, 255, 2048, 2049, 8192, 8200)     # no unit | tail only | one unit | units + tail | one unit per lane | +1 | resident limit | past it
ROWS = (1, 3, 257)
REDUCTIONS = ("mean", "sum", "none")
HARD = ("max_last", "const", "dominant", "big1e4", "wide3e3", "neginf", "ignored", "all_ignored", "bad_targets")


def ce_ref(x, target, reduction="mean", ignore_index=IGNORE, eps=0.0, grad_out=1.0):
    """x float64 [rows, V], target int64 [rows], grad_out a scalar (mean / sum) or [rows] (none) -> (loss, dx [rows, V], w [rows]):
    the loss of ``F.cross_entropy``, its gradient for the incoming ``grad_out`` and the per-row weight w_r of the gradient formula.
    target == ignore_index: loss 0, zero gradient row; any other target outside [0, V): NaN in that row's loss and gradient."""
    x = np.asarray(x, dtype=np.float64)
    rows, v = x.shape
    t = np.asarray(target, dtype=np.int64)
    ign = t == ignore_index
    bad = ~ign & ((t < 0) | (t >= v))
    tc = np.where(ign | bad, 0, t)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=1, keepdims=True)
        logl = np.log(np.exp(x - m).sum(axis=1, keepdims=True))
        logp = (x - m) - logl
        row = -(1.0 - eps) * logp[np.arange(rows), tc]
        if eps > 0.0:
            row = row + eps * -logp.mean(axis=1)
        row = np.where(ign, 0.0, np.where(bad, np.nan, row))
        count = float((~ign).sum())
        if reduction == "none":
            loss, w = row, np.broadcast_to(np.asarray(grad_out, dtype=np.float64), (rows,)).copy()
        elif reduction == "sum":
            loss, w = row.sum(), np.full(rows, float(grad_out))
        else:
            loss, w = row.sum() / count if count else np.nan, np.full(rows, float(grad_out) / count if count else np.inf)
        onehot = np.zeros_like(x)
        onehot[np.arange(rows), tc] = 1.0
        dx = w[:, None] * (np.exp(logp) - (1.0 - eps) * onehot - eps / v)
    dx[ign] = 0.0
    dx[bad] = np.nan
    w = np.where(ign, 0.0, w)
    return loss, dx, w


def _cases():
    out, k = [], 0
    for v in VS:                                 # every path x every row count; reduction, smoothing and ignored rows rotate through them
        for rows in ROWS:
            out.append(dict(kind="randn", v=v, rows=rows, layout="contig", reduction=REDUCTIONS[k % 3], eps=(0.0, 0.1)[(k // 3) % 2],
                            ignore=rows > 1 and k % 2 == 0))
            k += 1
    for v in (7, 2049, 8192):                    # the [2, 5, V] slice of [2, 9, V], read in place
        out.append(dict(kind="randn", v=v, rows=10, layout="slice", reduction=REDUCTIONS[k % 3], eps=0.1, ignore=True))
        k += 1
    for v in (255, 2048, 8200):                  # 4 bytes off a 16-byte boundary: the element-wise path
        out.append(dict(kind="randn", v=v, rows=3, layout="offset", reduction=REDUCTIONS[k % 3], eps=0.1, ignore=False))
        k += 1
    for kind in HARD:
        for v in (255, 2049, 8200):
            eps = 0.0 if kind == "neginf" else (0.0, 0.1)[k % 2]
            red = "none" if kind == "bad_targets" else REDUCTIONS[k % 3]
            out.append(dict(kind=kind, v=v, rows=5, layout="contig", reduction=red, eps=eps, ignore=kind in ("ignored", "all_ignored")))
            k += 1
    for c in out:
        c["id"] = "{kind}-V{v}-r{rows}-{layout}-{reduction}-eps{eps}{ig}".format(ig="-ign" if c["ignore"] else "", **c)
    return out


CASES = _cases()


def make_case(case, dtype, seed=0):
    """-> (x32 [rows, V] float32 numpy holding values exactly representable in ``dtype``, target int64 [rows], grad_out): the inputs of
    one case, the same on every machine.  ``dtype`` torch.float32 or torch.bfloat16."""
    rows, v, kind = case["rows"], case["v"], case["kind"]
    rng = np.random.default_rng(1000 * seed + 7 * v + rows + 13 * HARD.index(kind) if kind in HARD else 1000 * seed + 7 * v + rows)
    x = rng.standard_normal((rows, v)).astype(np.float32)
    t = rng.integers(0, v, size=rows).astype(np.int64)
    if kind == "max_last":                       # the maximum AND the target in the last element (the tail, where V has one)
        x[:, -1] = 9.0
        t[:] = v - 1
        x[0, -1] = -9.0                          # ... and one row whose target is last but far from the maximum
    elif kind == "const":
        x[:] = 3.25
        x[1] = -1e4
        x[2] = 0.0
    elif kind == "dominant":                     # target = argmax by a wide margin: loss ~ 0
        x[np.arange(rows), t] += 60.0
    elif kind == "big1e4":                       # m + log l would round to 1e-3 here
        x += 1e4
    elif kind == "wide3e3":                      # every exp but one underflows
        x *= 3e3
    elif kind == "neginf":
        mask = rng.random((rows, v)) < 0.3
        mask[np.arange(rows), t] = False
        x[mask] = -np.inf
    elif kind == "bad_targets":
        t[1], t[3] = -5, v
    if case["ignore"]:
        t[::3] = IGNORE
    if kind == "all_ignored":
        t[:] = IGNORE
    x = torch.from_numpy(x).to(dtype).float().numpy()
    g = rng.standard_normal(rows).astype(np.float32) if case["reduction"] == "none" else np.float32(1.75)
    return x, t, g
