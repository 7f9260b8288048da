"""float64 numpy restatement of what ``mas_hip.optim`` adds with ``ema_decay`` / ``ema_warmup`` / ``skip_nonfinite``: the EMA recurrence,
the warm-up schedule, and the guard.  The Adam / AdamW step itself is ``adam_clip_ref.adam_steps`` (imported, not restated).
tests/test_adam_ema_host.py and tests/test_gpu_adam_ema.py check the optimizer against it."""
import numpy as np

import adam_clip_ref as R

F32 = np.float32


def ema_weight(decay):
    """``1 - decay`` as the kernel forms it: both rounded to fp32 (the weight enters the fp64 recurrence as the value the kernel uses, as
    the clip coefficient does in adam_clip_ref)"""
    return float(F32(1.0) - F32(decay))


def warmup_decay(decay, k):
    """the decay of the optimizer's k-th step (k = 0, 1, ...) under ``ema_warmup``"""
    return min(float(decay), (1.0 + k) / (10.0 + k))


def ema_update(ema, p_new, decay):
    """one step of the recurrence in fp64: ``ema + (1 - decay) (p_new - ema)``"""
    ema, p_new = np.asarray(ema, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    return ema + ema_weight(decay) * (p_new - ema)


def ema_bound(k, p, ema):
    """elementwise bound on |ema - ref64| after k steps when ref64 is driven by the optimizer's own fp32 ``p``: each step rounds twice in
    fp32 (the difference, the fused multiply-add), each by at most half an ulp of a value no larger than 2 max(|p|, |ema|): 2^-23 max per
    step, taken with a factor 2"""
    return k * 2.0 ** -22 * np.maximum(np.abs(np.asarray(p, dtype=np.float64)), np.abs(np.asarray(ema, dtype=np.float64)))


def step_is_skipped(grads):
    """the guard: the fp64 global norm of this step's gradients (None entries and empty arrays take no part) is NaN or infinite"""
    return not np.isfinite(R.grad_norm([g for g in grads if g is not None and np.size(g)]))


def adam_ema_steps(params, grads_per_step, lr, betas, eps, weight_decay, decays, max_grad_norm=None, decoupled=False, skip_nonfinite=False):
    """Adam / AdamW with an EMA of the weights over several steps, all in float64.  ``decays``: one decay per step.  Returns
    (parameters, EMAs, [skipped per step]).  A parameter without a gradient at a step keeps its EMA.  With ``skip_nonfinite`` a step
    whose norm is not finite leaves every array unchanged while every step count advances; ``adam_steps`` starts from zero moments, so
    such steps can only be expressed where they lead the run (they become its ``steps_done``) -- anything else raises."""
    p0 = [np.asarray(x, dtype=np.float64).copy() for x in params]
    skipped = [bool(skip_nonfinite and step_is_skipped(gs)) for gs in grads_per_step]
    lead = 0
    while lead < len(skipped) and skipped[lead]:
        lead += 1
    if any(skipped[lead:]):
        raise ValueError("adam_ema_steps: a skipped step after an applied one cannot be expressed through adam_clip_ref.adam_steps")
    done = [sum(1 for gs in grads_per_step[:lead] if gs[i] is not None) for i in range(len(p0))]
    p, ema = p0, [x.copy() for x in p0]
    for j in range(lead, len(grads_per_step)):
        p, _ = R.adam_steps(p0, grads_per_step[lead:j + 1], lr, betas, eps, weight_decay, max_grad_norm=max_grad_norm, decoupled=decoupled,
                            steps_done=done)
        ema = [e if g is None else ema_update(e, x, decays[j]) for e, x, g in zip(ema, p, grads_per_step[j])]
    return p, ema, skipped
