"""float64 numpy restatement of ``mas_hip.optim`` with ``device_step=True``: the per-step scalars the device forms from its own step
count (``mas_adam_multi_dev``: ``step_size``, ``sqrt(bc2)``, the EMA weight from ``t, lr, beta1, beta2, d, k``), one Adam / AdamW update
with them, and a run over several steps that returns parameters, both moments, the averages and the step counts.  Constants the kernel
holds in fp32 (``beta``, ``1 - beta``, ``eps``, ``weight_decay``, ``lr``) enter the fp64 recurrences as those fp32 values
(``moment_weights`` says why that matters for beta2 = 0.999); everything the kernel computes is computed here in fp64.  The norm and the clip
coefficient are ``adam_clip_ref``'s, the EMA recurrence ``adam_ema_ref``'s (imported, not restated).
tests/test_adam_dev_host.py checks it against torch on the CPU; tests/test_gpu_adam_dev.py checks the kernels against it."""
import numpy as np

import adam_clip_ref as R
import adam_ema_ref as E

F32 = np.float32


def step_scalars(t, lr, beta1, beta2):
    """(step_size, sqrt(bc2)) of a parameter's t-th step (t = 1, 2, ...): the learning rate as the fp32 value the device scalar holds, the
    powers, the division and the root in fp64, each result rounded to fp32 once"""
    lr32 = float(F32(lr))
    return float(F32(lr32 / (1.0 - beta1 ** t))), float(F32(np.sqrt(1.0 - beta2 ** t)))


def ema_weight(d, k=None):
    """``1 - decay`` of the optimizer's k-th step (k = 0, 1, ...; None: no warm-up, the fixed decay): the decay in fp64, rounded to fp32,
    subtracted from 1 in fp32"""
    decay = float(d) if k is None else min(float(d), (1.0 + k) / (10.0 + k))
    return float(F32(1.0) - F32(decay))


def moment_weights(beta):
    """(beta, 1 - beta) as the Adam kernel holds them: beta rounded to fp32, the difference formed in fp32.  These are constants of the
    kernel, not results it computes: they enter the fp64 recurrences as the values it uses, like the clip coefficient and the EMA weight.
    (The bias corrections above are formed from the fp64 betas, as the host forms them.)  For beta = 0.999 the fp32 ``1 - beta`` is
    1.3e-5 away from the fp64 one -- ``beta_rounding`` bounds that."""
    return float(F32(beta)), float(F32(1.0) - F32(beta))


def beta_rounding(beta):
    """bound on the relative distance between the kernel's ``1 - beta`` and the exact one: beta moves by at most half an ulp (2^-24
    relative) when rounded to fp32, the subtraction from 1 is exact for beta >= 0.5, so the difference moves by 2^-24 beta / (1 - beta)"""
    return 2.0 ** -24 * beta / (1.0 - beta)


def adam_update(p, g, m, v, t, lr, betas, eps, weight_decay, decoupled=False, coef=1.0):
    """one update of one tensor in fp64 with the scalars above -> (p, m, v); ``coef``: the clip coefficient the gradient is multiplied by"""
    step_size, bc2_sqrt = step_scalars(t, lr, *betas)
    (_, omb1), (b2, omb2) = moment_weights(betas[0]), moment_weights(betas[1])
    lr32, eps, weight_decay = float(F32(lr)), float(F32(eps)), float(F32(weight_decay))
    p, m, v = (np.asarray(x, dtype=np.float64) for x in (p, m, v))
    g = np.asarray(g, dtype=np.float64) * coef
    if weight_decay != 0.0:
        if decoupled:
            p = p - lr32 * weight_decay * p
        else:
            g = g + weight_decay * p
    m = m + omb1 * (g - m)
    v = b2 * v + omb2 * g * g
    return p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps), m, v


def adam_dev_steps(params, grads_per_step, lrs, betas, eps, weight_decay, decoupled=False, max_grad_norm=None, ema_decay=None,
                   ema_warmup=False, skip_nonfinite=False):
    """params: list of arrays; grads_per_step: per step one array or None per parameter; lrs: one learning rate per step (or one for all).
    Returns dict(p, m, v, ema, t, k, skipped, norms).  A parameter without a gradient takes no part in a step and its count stays; a step
    whose norm is not finite (``skip_nonfinite``) leaves every array alone and still advances the counts of the parameters that had a
    gradient, and the EMA counter k advances at every step."""
    if np.isscalar(lrs):
        lrs = [lrs] * len(grads_per_step)
    p = [np.asarray(x, dtype=np.float64).copy() for x in params]
    m, v = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p]
    ema = [x.copy() for x in p] if ema_decay is not None else None
    t, k, skipped, norms = [0] * len(p), 0, [], []
    for grads, lr in zip(grads_per_step, lrs):
        coef, skip = 1.0, False
        if max_grad_norm is not None or skip_nonfinite:
            norm = R.grad_norm([g for g in grads if g is not None and np.size(g)])
            norms.append(norm)
            skip = bool(skip_nonfinite and not np.isfinite(norm))
            if max_grad_norm is not None:
                coef = float(R.clip_coef(norm, max_grad_norm)[1])
        skipped.append(skip)
        w = None if ema_decay is None else ema_weight(ema_decay, k if ema_warmup else None)
        for i, g in enumerate(grads):
            if g is None:
                continue
            t[i] += 1
            if skip:
                continue
            p[i], m[i], v[i] = adam_update(p[i], g, m[i], v[i], t[i], lr, betas, eps, weight_decay, decoupled, coef)
            if ema is not None:
                ema[i] = ema[i] + w * (p[i] - ema[i])
        k += 1
    return dict(p=p, m=m, v=v, ema=ema, t=t, k=k, skipped=skipped, norms=norms)


__all__ = ["step_scalars", "ema_weight", "moment_weights", "beta_rounding", "adam_update", "adam_dev_steps", "E", "R"]
