"""``device_step=True`` of ``mas_hip.optim`` without a GPU: the float64 helper of the device-side scalars and update
(tests/helpers/adam_dev_ref.py) against torch.optim.Adam / AdamW and against adam_ema_ref, the refusals, the no-op rule of
``sync_hyperparameters()``, and the argument checks of the two C entries.  The kernels are tests/test_gpu_adam_dev.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import adam_dev_ref as D  # noqa: E402
import adam_ema_ref as E  # noqa: E402

SHAPES = ((5,), (3, 4), (2, 3, 3, 3))


def _arrays(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]


def _grads(seed, steps, absent=()):
    g = torch.Generator().manual_seed(seed)
    return [[None if (k, i) in absent else torch.randn(*s, generator=g, dtype=torch.float64) * (0.1 + k) for i, s in enumerate(SHAPES)]
            for k in range(steps)]


def _np(ts):
    return [None if t is None else t.detach().double().numpy() for t in ts]


@pytest.mark.parametrize("betas", [(0.5, 0.9), (0.9, 0.999)])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_float64_helper_matches_torch_over_six_steps(decoupled, wd, betas):
    """torch's single-tensor implementation on float64 CPU parameters.  The helper differs from it by the fp32 rounding of lr, step_size,
    sqrt(bc2), eps and weight_decay (2^-24 relative each: 6 steps x 5 x 2^-24 = 1.8e-6 of what the updates moved, asserted as 2e-6 of the
    largest parameter -- the bound the GPU tests use for the same arithmetic), and by the kernel's fp32 ``beta`` and ``1 - beta``
    (``moment_weights``): a moment's weight is off by at most ``beta_rounding(beta)`` relative -- 6e-5 for 0.999, 5e-7 for 0.9 -- which
    reaches the moment itself in full and the parameter only through ``sqrt(v)`` in an update of size lr."""
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    ps = [torch.nn.Parameter(x.clone()) for x in _arrays(1)]
    opt = cls(ps, lr=3e-3, betas=betas, eps=1e-8, weight_decay=wd, foreach=False, fused=False)
    grads = _grads(2, 6, absent={(3, 1)})
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.clone()
        opt.step()
    got = D.adam_dev_steps(_np(_arrays(1)), [_np(gs) for gs in grads], 3e-3, betas, 1e-8, wd, decoupled=decoupled)
    assert got["t"] == [6, 5, 6] and got["k"] == 6 and got["skipped"] == [False] * 6
    for i, (p, gp, gm, gv) in enumerate(zip(ps, got["p"], got["m"], got["v"])):
        st = opt.state[p]
        for a, b, tol in ((gp, p.detach().numpy(), 2e-6), (gm, st["exp_avg"].numpy(), 2e-6 + D.beta_rounding(betas[0])),
                          (gv, st["exp_avg_sq"].numpy(), 2e-6 + D.beta_rounding(betas[1]))):
            assert np.abs(a - b).max() <= tol * np.abs(b).max()
        assert int(st["step"]) == got["t"][i]


def test_scalars_are_the_host_formulas():
    """what ``adam_launch`` forms on the host today from the same numbers, and ``_ema_weight`` / adam_ema_ref for the EMA weight"""
    from mas_hip.optim import _ema_weight
    for b1, b2 in ((0.5, 0.9), (0.9, 0.999)):
        for t in (1, 2, 7, 1000, 100000):
            for lr in (1e-3, 4.5e-4, 0.0):
                lr32 = C.c_float(lr).value
                want = (C.c_float(lr32 / (1.0 - b1 ** t)).value, C.c_float(np.sqrt(1.0 - b2 ** t)).value)
                assert D.step_scalars(t, lr, b1, b2) == want
    for beta in (0.5, 0.9, 0.95, 0.999):
        b32, omb = D.moment_weights(beta)
        assert b32 == C.c_float(beta).value and omb == C.c_float(1.0 - C.c_float(beta).value).value       # `1.0f - b` of the kernel
        assert abs(omb - (1.0 - beta)) <= D.beta_rounding(beta) * (1.0 - beta)
    for d in (0.0, 0.5, 0.9, 0.999, 0.9999):
        assert D.ema_weight(d) == _ema_weight(d) == E.ema_weight(d)
        for k in (0, 1, 8, 9, 10, 89, 90, 91, 5000, 2 ** 24):
            decay = E.warmup_decay(d, k)
            assert D.ema_weight(d, k) == _ema_weight(decay) == E.ema_weight(decay)


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
def test_ema_of_the_helper_is_adam_ema_ref(warmup):
    grads = [_np(gs) for gs in _grads(3, 5, absent={(2, 1)})]
    got = D.adam_dev_steps(_np(_arrays(1)), grads, 2e-3, (0.5, 0.9), 1e-8, 0.02, ema_decay=0.9, ema_warmup=warmup)
    ema = _np(_arrays(1))
    for k in range(5):
        part = D.adam_dev_steps(_np(_arrays(1)), grads[:k + 1], 2e-3, (0.5, 0.9), 1e-8, 0.02)["p"]
        decay = E.warmup_decay(0.9, k) if warmup else 0.9
        ema = [e if g is None else E.ema_update(e, x, decay) for e, x, g in zip(ema, part, grads[k])]
    for a, b in zip(got["ema"], ema):
        assert np.array_equal(a, b)
    # and the whole run against the existing float64 run (host bias corrections, unrounded): the same 2e-6
    decays = [E.warmup_decay(0.9, k) if warmup else 0.9 for k in range(5)]
    want_p, want_e, _ = E.adam_ema_steps(_np(_arrays(1)), grads, 2e-3, (0.5, 0.9), 1e-8, 0.02, decays)
    for a, b in list(zip(got["p"], want_p)) + list(zip(got["ema"], want_e)):
        assert np.abs(a - b).max() <= 2e-6 * np.abs(b).max()


def test_guard_of_the_helper():
    grads = [_np(gs) for gs in _grads(4, 4)]
    grads[2][1][2, 1] = np.inf
    got = D.adam_dev_steps(_np(_arrays(1)), grads, 2e-3, (0.5, 0.9), 1e-8, 0.0, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True, max_grad_norm=1.0)
    assert got["skipped"] == [False, False, True, False] and got["t"] == [4, 4, 4] and got["k"] == 4
    two = D.adam_dev_steps(_np(_arrays(1)), grads[:2], 2e-3, (0.5, 0.9), 1e-8, 0.0, ema_decay=0.9, ema_warmup=True, max_grad_norm=1.0)
    three = D.adam_dev_steps(_np(_arrays(1)), grads[:3], 2e-3, (0.5, 0.9), 1e-8, 0.0, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True, max_grad_norm=1.0)
    for key in ("p", "m", "v", "ema"):
        assert all(np.array_equal(a, b) for a, b in zip(two[key], three[key]))


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_device_step_on_cpu_parameters_raises_at_step(decoupled):
    from mas_hip.optim import Adam, AdamW
    ps = [torch.nn.Parameter(x.float()) for x in _arrays(1)]
    opt = (AdamW if decoupled else Adam)(ps, lr=1e-3, device_step=True)            # (constructing is fine: nothing is touched yet)
    assert opt.device_step is True and "device_step" not in opt.defaults and all("device_step" not in g for g in opt.param_groups)
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match=r"parameter 0 of shape \(5,\)"):
        opt.step()
    with pytest.raises(RuntimeError, match=r"parameter 0 of shape \(5,\)"):
        opt.init_state()
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before)) and all(len(opt.state[p]) == 0 for p in ps)
    with pytest.raises(RuntimeError, match="device_step=True"):
        Adam(ps, lr=1e-3).init_state()
    assert Adam(ps, lr=1e-3).device_step is False


def test_capturable_still_raises_and_points_at_device_step():
    from mas_hip.optim import Adam, AdamW
    ps = [torch.nn.Parameter(torch.zeros(4))]
    for cls in (Adam, AdamW):
        with pytest.raises(NotImplementedError, match="device_step"):
            cls(ps, capturable=True)
        with pytest.raises(NotImplementedError):
            cls(ps, capturable=True, device_step=True)
    import mas_hip.optim
    assert "device_step" in mas_hip.optim.__doc__.split("raise")[1][:200]


def test_sync_hyperparameters_is_a_no_op_when_nothing_changed():
    from mas_hip.optim import Adam
    ps = [torch.nn.Parameter(x.float()) for x in _arrays(1)]
    opt = Adam([dict(params=ps[:2]), dict(params=ps[2:], lr=5e-4)], lr=1e-3, device_step=True)
    pushed = []
    opt._push_lr = lambda vals: pushed.append(vals)                 # the one place a copy is issued
    assert opt.sync_hyperparameters() is True and pushed == [(1e-3, 5e-4)]
    assert opt.sync_hyperparameters() is False and opt.sync_hyperparameters() is False and len(pushed) == 1
    opt.param_groups[1]["lr"] = 5e-4                                 # written again with the same value: nothing to push
    assert opt.sync_hyperparameters() is False and len(pushed) == 1
    opt.param_groups[0]["lr"] = torch.tensor(2e-3)                   # a 0-dim tensor, as some schedulers leave one
    assert opt.sync_hyperparameters() is True and pushed[-1] == (float(torch.tensor(2e-3)), 5e-4) and len(pushed) == 2
    assert torch.is_tensor(opt.param_groups[0]["lr"])               # the group keeps what the caller put there
    assert opt.sync_hyperparameters() is False and len(pushed) == 2
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)        # a scheduler drives it unchanged
    n = len(pushed)
    assert opt.sync_hyperparameters() in (True, False)
    opt.param_groups[0]["lr"] = 7e-4
    assert opt.sync_hyperparameters() is True and pushed[-1][0] == 7e-4 and len(pushed) >= n + 1
    assert sched is not None
    # without device_step there is nothing to push
    plain = Adam(ps, lr=1e-3)
    plain._push_lr = lambda vals: pushed.append("plain")
    assert plain.sync_hyperparameters() is False and "plain" not in pushed


def test_state_generation_counts_loads_and_new_groups():
    from mas_hip.optim import Adam
    ps = [torch.nn.Parameter(x.float()) for x in _arrays(1)]
    opt = Adam(ps[:2], lr=1e-3)
    g0 = opt.state_generation
    opt.add_param_group(dict(params=ps[2:]))
    assert opt.state_generation == g0 + 1
    opt.load_state_dict(opt.state_dict())
    assert opt.state_generation == g0 + 2


def test_header_declares_the_entries_and_they_validate_arguments_without_gpu():
    import mas_hip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mas_hip.h")).read(), flags=re.S)
    for name in ("mas_adam_multi_dev", "mas_adam_advance_dev"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in mas_hip.EXPORTS
    L = mas_hip.lib()
    assert L.mas_abi_version() == mas_hip.ABI_VERSION == 10
    f = L.mas_adam_multi_dev
    assert f.argtypes[1] == f.argtypes[2] == C.POINTER(C.c_void_p) and f.argtypes[6] == f.argtypes[7] == f.argtypes[12] == C.c_double
    one = C.cast(C.c_void_p(16), C.POINTER(C.c_void_p))             # non-null pointers that no branch below follows
    call = lambda items=16, steps=one, n=1, blocks=1, lr=16, b1=0.9, b2=0.999, decay=0.9, rec=16: f(
        items, one, steps, n, blocks, lr, b1, b2, 1e-8, 0.0, None, 0, decay, None, None, rec, None)
    for rc in (call(items=None), call(steps=None), call(n=0), call(blocks=0), call(lr=None), call(rec=None)):
        assert rc == -1 and b"adam_multi_dev" in L.mas_last_error()
    for bad in (1.0, -0.1, float("nan")):
        assert call(b1=bad) == -1 and b"betas" in L.mas_last_error()
        assert call(b2=bad) == -1 and b"betas" in L.mas_last_error()
        assert call(decay=bad) == -1 and b"ema_decay" in L.mas_last_error()
    assert call(rec=20) == -1 and b"aligned" in L.mas_last_error()
    for rc in (L.mas_adam_advance_dev(None, 1, None), L.mas_adam_advance_dev(16, 0, None), L.mas_adam_advance_dev(16, -3, None)):
        assert rc == -1 and b"adam_advance_dev" in L.mas_last_error()
