"""``ema_decay`` / ``ema_warmup`` / ``skip_nonfinite`` / ``swap_ema()`` of ``mas_hip.optim`` on CPU tensors (the torch-expression path: the
same formulas as the kernel), the state-dict interchange with torch.optim.Adam, and the argument checks of the two C entries
``mas_adam_multi_ema`` / ``mas_swap_multi``.  The kernels are tests/test_gpu_adam_ema.py; the float64 helper is tests/helpers/adam_ema_ref.py."""
import copy
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

import adam_ema_ref as E  # noqa: E402

NEW_ENTRIES = ("mas_adam_multi_ema", "mas_swap_multi")
KW = dict(lr=2e-3, betas=(0.5, 0.9), eps=1e-8)
STATE = ("exp_avg", "exp_avg_sq")


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in ((5,), (3, 4), (2, 3, 3, 3))]


def _grads(seed, steps, absent=()):
    """per step one gradient per parameter of _params; `absent`: (step, parameter) pairs without one"""
    g = torch.Generator().manual_seed(seed)
    return [[None if (k, i) in absent else torch.randn(*s, generator=g) for i, s in enumerate(((5,), (3, 4), (2, 3, 3, 3)))] for k in range(steps)]


def _step(opt, ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.clone()
    opt.step()


def _bits(opt, ps, keys=STATE + ("ema",)):
    """clones of p and of the state tensors, in one flat list"""
    return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in keys if k in opt.state[p]]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _np(ts):
    return [None if t is None else t.detach().double().numpy() for t in ts]


def test_header_declares_the_entries_and_they_validate_arguments_without_gpu():
    import mas_hip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mas_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in mas_hip.EXPORTS
    L = mas_hip.lib()
    assert L.mas_abi_version() == mas_hip.ABI_VERSION == 10
    assert L.mas_adam_multi_ema.argtypes[1] == C.POINTER(C.c_void_p) and L.mas_swap_multi.argtypes[1] == C.POINTER(C.c_void_p)   # float* const*
    one = C.cast(C.c_void_p(16), C.POINTER(C.c_void_p))        # a non-null pointer that no branch below follows
    adam = lambda items, ema, n, blocks, bc1, decay, norm: L.mas_adam_multi_ema(items, ema, n, blocks, 1e-3, 0.9, 0.999, 1e-8, 0.0, bc1, 0.001, None, 0,
                                                                                decay, norm, None)
    for rc in (adam(None, None, 0, 0, 0.1, 0.9, None), adam(None, one, 1, 1, 0.1, 0.9, 16), adam(16, one, 0, 1, 0.1, 0.9, None),
               adam(16, one, 1, 0, 0.1, 0.9, None)):
        assert rc == -1 and b"adam_multi_ema" in L.mas_last_error()
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert adam(16, one, 1, 1, 0.1, bad, None) == -1 and b"ema_decay" in L.mas_last_error() and b"adam_multi_ema" in L.mas_last_error()
    # step 0 (no bias correction): refused with either new argument, and through the forward to mas_adam_multi_ex with neither
    for ema, norm in ((one, None), (None, 16), (one, 16), (None, None)):
        assert adam(16, ema, 1, 1, 0.0, 0.9, norm) == -1 and b"bias corrections" in L.mas_last_error()
    for rc in (L.mas_swap_multi(None, None, 0, 0, None), L.mas_swap_multi(None, one, 1, 1, None), L.mas_swap_multi(16, None, 1, 1, None),
               L.mas_swap_multi(16, one, 0, 1, None), L.mas_swap_multi(16, one, 1, 0, None)):
        assert rc == -1 and b"swap_multi" in L.mas_last_error()


def test_constructor_validation():
    from mas_hip.optim import Adam, AdamW
    p = _params(3)
    for cls in (Adam, AdamW):
        for bad in (1.0, -0.1, 2.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="ema_decay"):
                cls(p, ema_decay=bad)
        o = cls(p)
        assert o.ema_decay is None and o.ema_warmup is False and o.skip_nonfinite is False and o.step_skipped is None
        assert "ema_step" not in o.param_groups[0]
        o = cls(p, ema_decay=0, ema_warmup=True, skip_nonfinite=True, max_grad_norm=2)
        assert o.ema_decay == 0.0 and o.ema_warmup is True and o.skip_nonfinite is True and o.max_grad_norm == 2.0
        for key in ("ema_decay", "ema_warmup", "skip_nonfinite"):       # attributes, not keys of `defaults` / the groups
            assert key not in o.defaults and all(key not in g for g in o.param_groups)
        with pytest.raises(RuntimeError, match="ema_decay"):
            with cls(p).swap_ema():
                pass


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
@pytest.mark.parametrize("m", [None, 2.0], ids=["plain", "clipped"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_ema_on_cpu_leaves_the_update_alone_and_matches_float64(decoupled, m, warmup):
    from mas_hip.optim import Adam, AdamW
    cls = AdamW if decoupled else Adam
    a, b = _params(1), _params(1)
    kw = dict(weight_decay=0.02, max_grad_norm=m, **KW)
    oa = cls([dict(params=a[:2]), dict(params=a[2:])], ema_decay=0.9, ema_warmup=warmup, **kw)
    ob = cls([dict(params=b[:2]), dict(params=b[2:])], **kw)
    grads = _grads(2, 5, absent={(2, 1)})
    decays = [E.warmup_decay(0.9, k) if warmup else 0.9 for k in range(5)]
    assert decays[0] == (0.1 if warmup else 0.9) and decays[-1] == (5.0 / 14.0 if warmup else 0.9)
    ref = _np(a)
    for k, gs in enumerate(grads):
        kept = [oa.state[p]["ema"].clone() if "ema" in oa.state[p] else p.detach().clone() for p in a]
        _step(oa, a, gs)
        _step(ob, b, gs)
        assert _same(_bits(oa, a, STATE), _bits(ob, b, STATE))                   # p, exp_avg, exp_avg_sq: bitwise the optimizer without EMA
        for i, (p, g) in enumerate(zip(a, gs)):
            ema = oa.state[p]["ema"]
            if g is None:
                assert torch.equal(ema, kept[i])                                 # no gradient at this step: the average stays
                continue
            ref[i] = E.ema_update(ref[i], p.detach().numpy(), decays[k])
            assert ema.dtype == torch.float32 and ema.shape == p.shape
            assert (np.abs(ema.double().numpy() - ref[i]) <= E.ema_bound(k + 1, p.detach().numpy(), ema.numpy())).all()
            assert not torch.equal(ema, p.detach())
    assert oa.param_groups[0]["ema_step"] == 5 and "ema_step" not in oa.param_groups[1]
    # the all-float64 restatement (Adam itself from adam_clip_ref) agrees: fp32 against fp64 over five steps
    want_p, want_e, _ = E.adam_ema_steps(_np(_params(1)), [_np(gs) for gs in grads], KW["lr"], KW["betas"], KW["eps"], 0.02, decays,
                                         max_grad_norm=m, decoupled=decoupled)
    for p, wp, we in zip(a, want_p, want_e):
        assert np.allclose(p.detach().numpy(), wp, rtol=1e-5, atol=1e-6) and np.allclose(oa.state[p]["ema"].numpy(), we, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("m", [None, 2.0], ids=["plain", "clipped"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_skip_nonfinite_on_cpu(bad, m):
    from mas_hip.optim import Adam
    kw = dict(weight_decay=0.02, max_grad_norm=m, ema_decay=0.9, **KW)
    a, b = _params(1), _params(1)
    oa, ob = Adam(a, skip_nonfinite=True, **kw), Adam(b, **kw)
    grads = _grads(3, 4)
    for gs in grads[:2]:
        _step(oa, a, gs)
        _step(ob, b, gs)
        assert bool(oa.step_skipped) is False
    assert _same(_bits(oa, a), _bits(ob, b))         # finite norms: the guard changes nothing
    before = _bits(oa, a)
    poisoned = [g.clone() for g in grads[2]]
    poisoned[1][2, 1] = bad
    _step(oa, a, poisoned)
    assert _same(_bits(oa, a), before)               # p, exp_avg, exp_avg_sq and ema of every parameter: their old bits
    assert oa.step_skipped.dtype == torch.bool and oa.step_skipped.dim() == 0 and bool(oa.step_skipped) is True
    assert not bool(torch.isfinite(oa.grad_norm)) and all(int(oa.state[p]["step"]) == 3 for p in a)
    # the next finite step is the step of an optimizer whose step counts are one ahead
    for p in b:
        ob.state[p]["step"] += 1
    ob.param_groups[0]["ema_step"] += 1
    _step(oa, a, grads[3])
    _step(ob, b, grads[3])
    assert bool(oa.step_skipped) is False and _same(_bits(oa, a), _bits(ob, b))
    # without the guard the same gradient ends the run
    c = _params(1)
    oc = Adam(c, **kw)
    _step(oc, c, poisoned)
    assert not bool(torch.isfinite(c[1]).all())


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_skipped_first_steps_then_float64_reference(decoupled):
    """two poisoned steps lead the run: nothing moves, then three applied steps match the float64 run whose step counts start at 2"""
    from mas_hip.optim import Adam, AdamW
    a = _params(1)
    opt = (AdamW if decoupled else Adam)(a, weight_decay=0.02, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True, **KW)
    grads = _grads(4, 5)
    grads[0][0][3], grads[1][2][0, 0, 0, 0] = float("nan"), float("-inf")
    start = [p.detach().clone() for p in a]
    for k, gs in enumerate(grads):
        _step(opt, a, gs)
        assert bool(opt.step_skipped) is (k < 2)
        if k < 2:
            assert all(torch.equal(p, s) and torch.equal(opt.state[p]["ema"], s) for p, s in zip(a, start))
            assert all(not opt.state[p][key].any() for p in a for key in STATE)
    decays = [E.warmup_decay(0.9, k) for k in range(5)]
    want_p, want_e, skipped = E.adam_ema_steps(_np(start), [_np(gs) for gs in grads], KW["lr"], KW["betas"], KW["eps"], 0.02, decays,
                                               decoupled=decoupled, skip_nonfinite=True)
    assert skipped == [True, True, False, False, False] and all(int(opt.state[p]["step"]) == 5 for p in a)
    for p, wp, we in zip(a, want_p, want_e):
        assert np.allclose(p.detach().numpy(), wp, rtol=1e-5, atol=1e-6) and np.allclose(opt.state[p]["ema"].numpy(), we, rtol=1e-5, atol=1e-6)


def test_state_dict_interchange():
    from mas_hip.optim import Adam
    grads = _grads(5, 5)
    a = _params(1)
    oa = Adam([dict(params=a[:2]), dict(params=a[2:])], ema_decay=0.9, ema_warmup=True, **KW)
    for gs in grads[:3]:
        _step(oa, a, gs)
    sd = oa.state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq", "ema"} for s in sd["state"].values()) and sd["param_groups"][0]["ema_step"] == 3
    # ours -> torch.optim.Adam, which carries the unknown keys along, then a step there
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = torch.optim.Adam([dict(params=b[:2]), dict(params=b[2:])], **KW)
    ob.load_state_dict(copy.deepcopy(sd))
    assert all(torch.equal(ob.state[pb]["ema"], oa.state[pa]["ema"]) for pa, pb in zip(a, b))
    # ours -> ours: the run continues bit for bit, warm-up step included
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oc = Adam([dict(params=c[:2]), dict(params=c[2:])], ema_decay=0.9, ema_warmup=True, **KW)
    oc.load_state_dict(copy.deepcopy(sd))
    assert oc.param_groups[0]["ema_step"] == 3
    for gs in grads[3:]:
        _step(oa, a, gs)
        _step(oc, c, gs)
    _step(ob, b, grads[3])
    _step(ob, b, grads[4])
    assert _same(_bits(oa, a), _bits(oc, c)) and oc.param_groups[0]["ema_step"] == 5
    assert all(torch.allclose(pa, pb, rtol=1e-6, atol=1e-7) for pa, pb in zip(a, b))
    # torch's state (no "ema", no "ema_step") -> ours: the average starts from the weights as they are at the next step
    d = [torch.nn.Parameter(p.detach().clone()) for p in b]
    od = Adam([dict(params=d[:2]), dict(params=d[2:])], ema_decay=0.5, ema_warmup=True, **KW)
    tsd = copy.deepcopy(ob.state_dict())
    for s in tsd["state"].values():
        del s["ema"]
    tsd["param_groups"][0].pop("ema_step", None)
    od.load_state_dict(tsd)
    assert all("ema" not in od.state[p] for p in d)
    now = [p.detach().clone() for p in d]
    g = _grads(6, 1)[0]
    _step(od, d, g)
    decay = E.warmup_decay(0.5, 0)                   # its own first EMA step
    for p, w in zip(d, now):
        assert int(od.state[p]["step"]) == 6
        want = E.ema_update(w.numpy(), p.detach().numpy(), decay)
        assert (np.abs(od.state[p]["ema"].double().numpy() - want) <= E.ema_bound(1, p.detach().numpy(), w.numpy())).all()
    # and this optimizer's own state without an average
    e = _params(1)
    oe = Adam(e, **KW)
    _step(oe, e, grads[0])
    f = [torch.nn.Parameter(p.detach().clone()) for p in e]
    of = Adam(f, ema_decay=0.5, **KW)
    of.load_state_dict(copy.deepcopy(oe.state_dict()))
    now = [p.detach().clone() for p in f]
    _step(of, f, grads[1])
    for p, w in zip(f, now):
        assert torch.equal(of.state[p]["ema"], torch.lerp(w, p.detach(), 0.5))


def test_swap_ema_and_ema_state_dict_on_cpu():
    from mas_hip.optim import Adam
    lin = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3), torch.nn.Linear(3, 2))
    frozen = lin[2].bias                              # not handed to the optimizer: no average
    ps = [p for p in lin.parameters() if p is not frozen]
    opt = Adam(ps, ema_decay=0.5, **KW)
    x = torch.randn(8, 4, generator=torch.Generator().manual_seed(0))
    for _ in range(3):
        opt.zero_grad()
        lin(x).square().mean().backward()
        opt.step()
    live, ema = [p.detach().clone() for p in ps], [opt.state[p]["ema"].clone() for p in ps]
    assert not any(torch.equal(a, b) for a, b in zip(live, ema))
    esd = opt.ema_state_dict(lin)
    sd = lin.state_dict()
    assert list(esd) == list(sd)
    names = {id(p): n for n, p in lin.named_parameters()}
    for n in sd:
        mine = [i for i, p in enumerate(ps) if names[id(p)] == n]
        assert torch.equal(esd[n], ema[mine[0]] if mine else sd[n])              # buffers and the parameter without an average: unchanged
        assert esd[n].data_ptr() != (opt.state[ps[mine[0]]]["ema"].data_ptr() if mine else -1)     # a clone
    with opt.swap_ema() as inside:
        assert inside is opt
        assert all(torch.equal(p.detach(), e) for p, e in zip(ps, ema))
        assert all(torch.equal(opt.state[p]["ema"], w) for p, w in zip(ps, live))
        assert all(torch.equal(v, esd[n]) for n, v in opt.ema_state_dict(lin).items())
        with pytest.raises(RuntimeError, match="already active"):
            with opt.swap_ema():
                pass
        with pytest.raises(RuntimeError, match="inside swap_ema"):
            opt.step()
        assert all(torch.equal(p.detach(), e) for p, e in zip(ps, ema))            # neither refusal touched anything
    assert all(torch.equal(p.detach(), w) for p, w in zip(ps, live))
    assert all(torch.equal(opt.state[p]["ema"], e) for p, e in zip(ps, ema))
    with pytest.raises(ZeroDivisionError):           # an exception inside still restores
        with opt.swap_ema():
            1 / 0
    assert all(torch.equal(p.detach(), w) for p, w in zip(ps, live))
    opt.step()                                       # and the optimizer steps again
