"""float64 numpy restatement of what ``mas_hip.optim`` computes with ``max_grad_norm``: the global L2 norm of a list of gradients, the
clip coefficient of torch.nn.utils.clip_grad_norm_ (its two fp32 roundings are part of the definition), and Adam / AdamW over several
steps.  tests/test_adam_clip_host.py checks it against torch on the CPU; tests/test_gpu_adam_clip.py checks the kernels against it."""
import numpy as np

F32 = np.float32


def grad_norm(grads):
    """the fp64 L2 norm over all arrays (None entries are skipped); squares of fp32 values are exact in fp64"""
    total = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for g in grads:
            if g is not None:
                g = np.asarray(g, dtype=np.float64).ravel()
                total += float(np.dot(g, g))
        return float(np.sqrt(total))


def clip_coef(norm, max_norm):
    """(out[0], out[1]) of ``mas_grad_clip_coef``: the norm rounded to fp32, then ``min(max_norm / (out[0] + 1e-6), 1)`` in fp32 with
    one rounding per operation.  A NaN norm gives a NaN coefficient."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n32 = F32(norm)
        c = F32(max_norm) / (n32 + F32(1e-6))
    return n32, (F32(1.0) if c > F32(1.0) else c)


def adam_steps(params, grads_per_step, lr, betas, eps, weight_decay, max_grad_norm=None, decoupled=False, steps_done=None):
    """params: list of arrays (any shape); grads_per_step: per step a list with one array or None per parameter.  Returns
    (final parameters in float64, [(fp32 norm, fp32 coefficient) per step]).  A parameter without a gradient takes no part in that step and
    its own step count does not advance.  The coefficient enters as the fp32 value the kernels use."""
    b1, b2 = betas
    p = [np.asarray(x, dtype=np.float64).copy() for x in params]
    m = [np.zeros_like(x) for x in p]
    v = [np.zeros_like(x) for x in p]
    t = [0] * len(p) if steps_done is None else list(steps_done)
    log = []
    for grads in grads_per_step:
        coef = 1.0
        if max_grad_norm is not None:
            n32, c32 = clip_coef(grad_norm([g for g in grads if g is not None and np.size(g)]), max_grad_norm)
            log.append((n32, c32))
            coef = float(c32)
        for i, g in enumerate(grads):
            if g is None:
                continue
            t[i] += 1
            g = np.asarray(g, dtype=np.float64) * coef
            if weight_decay != 0.0:
                if decoupled:
                    p[i] -= lr * weight_decay * p[i]
                else:
                    g = g + weight_decay * p[i]
            m[i] = b1 * m[i] + (1.0 - b1) * g
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            denom = np.sqrt(v[i]) / np.sqrt(1.0 - b2 ** t[i]) + eps
            p[i] -= (lr / (1.0 - b1 ** t[i])) * m[i] / denom
    return p, log
