"""Global-norm clipping and AdamW in ``mas_hip.optim`` on CPU tensors: the host logic of ``max_grad_norm`` (one norm over all groups,
the coefficient formula, parameters without a gradient, the state layout that stays torch.optim.Adam's), ``AdamW`` against
torch.optim.AdamW, ``clip_grad_norm_``, and the argument checks of the four C entries.  The kernels are tests/test_gpu_adam_clip.py."""
import copy
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import adam_clip_ref as R  # noqa: E402

NEW_ENTRIES = ("mas_grad_sqnorm_multi", "mas_grad_clip_coef", "mas_adam_multi_ex", "mas_grad_scale_multi")
KW = dict(lr=2e-3, betas=(0.5, 0.9), eps=1e-8)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in ((5,), (3, 4), (2, 3, 3, 3))]


def _run(ours_cls, torch_cls, wd, m, steps=5):
    """`steps` steps of ours(max_grad_norm=m) beside torch's clip_grad_norm_ + optimizer on the same gradients (two groups; parameter 1 sits
    step 2 out); returns both parameter lists, both optimizers and the per-step (gradients, our norm, our coefficient)"""
    a, b = _params(1), _params(1)
    oa = ours_cls([dict(params=a[:2]), dict(params=a[2:])], weight_decay=wd, max_grad_norm=m, **KW)
    ob = torch_cls([dict(params=b[:2]), dict(params=b[2:])], weight_decay=wd, **KW)
    g = torch.Generator().manual_seed(2)
    seen = []
    for step in range(steps):
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g)
            pa.grad, pb.grad = gr.clone(), gr.clone()
        if step == 2:
            a[1].grad = None
            b[1].grad = None
        grads = [None if p.grad is None else p.grad.clone() for p in a]
        oa.step()
        if m is not None:
            torch.nn.utils.clip_grad_norm_(b, m)
            assert all(p.grad is None or torch.equal(p.grad, gr) for p, gr in zip(a, grads))      # ours leaves the gradients alone
            seen.append((grads, oa.grad_norm.clone(), oa.clip_coef.clone()))
        ob.step()
    return a, b, oa, ob, seen


@pytest.mark.parametrize("wd", [0.0, 0.02])
@pytest.mark.parametrize("m", [2.0, 100.0])          # the norm of the 71 unit-normal elements is about 8.4: 2 clips, 100 does not
def test_clipped_adam_matches_clip_grad_norm_and_torch_adam(wd, m):
    from mas_hip.optim import Adam
    a, b, oa, ob, seen = _run(Adam, torch.optim.Adam, wd, m)
    for pa, pb in zip(a, b):
        assert torch.allclose(pa, pb, rtol=1e-6, atol=1e-7)
        assert int(oa.state[pa]["step"]) == int(ob.state[pb]["step"])
    for grads, norm, coef in seen:
        n32, c32 = R.clip_coef(R.grad_norm([None if g is None else g.numpy() for g in grads]), m)
        assert norm.dtype == torch.float32 and norm.dim() == 0 and coef.dtype == torch.float32 and coef.dim() == 0
        assert float(norm) == float(n32) and float(coef) == float(c32)
        assert (float(coef) < 1.0) == (m == 2.0)
    # the float64 helper agrees with both (it is the reference of the GPU tests)
    p0 = [p.detach().numpy() for p in _params(1)]
    ref, _ = R.adam_steps(p0, [[None if g is None else g.numpy() for g in grads] for grads, _, _ in seen], KW["lr"], KW["betas"], KW["eps"],
                          wd, max_grad_norm=m)
    for pa, r in zip(a, ref):
        assert np.allclose(pa.detach().numpy(), r, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("m", [None, 2.0])
def test_adamw_matches_torch_adamw(m):
    from mas_hip.optim import Adam, AdamW
    a, b, oa, ob, seen = _run(AdamW, torch.optim.AdamW, 0.05, m)
    for pa, pb in zip(a, b):
        assert torch.allclose(pa, pb, rtol=1e-6, atol=1e-7)
    assert isinstance(oa, Adam) and oa.defaults["weight_decay"] == 0.05 and AdamW(_params(3)).defaults["weight_decay"] == 1e-2
    # decoupled and coupled decay differ by far more than the tolerance: the comparison above can tell them apart
    c, _, _, _, _ = _run(Adam, torch.optim.Adam, 0.05, m)
    assert not torch.allclose(a[0], c[0], rtol=1e-4, atol=1e-5)
    if m is not None:
        p0 = [p.detach().numpy() for p in _params(1)]
        ref, _ = R.adam_steps(p0, [[None if g is None else g.numpy() for g in grads] for grads, _, _ in seen], KW["lr"], KW["betas"],
                              KW["eps"], 0.05, max_grad_norm=m, decoupled=True)
        for pa, r in zip(a, ref):
            assert np.allclose(pa.detach().numpy(), r, rtol=1e-6, atol=1e-7)
    # state_dict interchange with torch.optim.AdamW, both directions, then one more step everywhere
    c, d = [torch.nn.Parameter(p.detach().clone()) for p in a], [torch.nn.Parameter(p.detach().clone()) for p in b]
    oc = torch.optim.AdamW([dict(params=c[:2]), dict(params=c[2:])], weight_decay=0.05, **KW)
    od = AdamW([dict(params=d[:2]), dict(params=d[2:])], weight_decay=0.05, max_grad_norm=m, **KW)
    oc.load_state_dict(copy.deepcopy(oa.state_dict()))
    od.load_state_dict(copy.deepcopy(ob.state_dict()))
    g = torch.Generator().manual_seed(4)
    for pa, pb, pc, pd in zip(a, b, c, d):
        gr = torch.randn(pa.shape, generator=g)
        pa.grad, pb.grad, pc.grad, pd.grad = gr.clone(), gr.clone(), gr.clone(), gr.clone()
    oa.step(); od.step()
    if m is not None:
        torch.nn.utils.clip_grad_norm_(b, m)
        torch.nn.utils.clip_grad_norm_(c, m)
    ob.step(); oc.step()
    for pa, pb, pc, pd in zip(a, b, c, d):
        assert torch.allclose(pc, pa, rtol=1e-6, atol=1e-7) and torch.allclose(pd, pb, rtol=1e-6, atol=1e-7)


def test_state_layout_is_torch_adams_with_a_clip():
    from mas_hip.optim import Adam
    a, b, oa, ob, _ = _run(Adam, torch.optim.Adam, 0.02, 2.0, steps=3)
    sd = oa.state_dict()
    assert all("max_grad_norm" not in g for g in sd["param_groups"]) and all("max_grad_norm" not in g for g in oa.param_groups)
    assert "max_grad_norm" not in oa.defaults and oa.max_grad_norm == 2.0
    assert set(sd["param_groups"][0]) == set(Adam(_params(3)).state_dict()["param_groups"][0])      # the same keys as without a clip
    for p in a:
        assert set(oa.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
    # ours -> torch's and back -> ours, then one clipped step on each side
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oc = torch.optim.Adam([dict(params=c[:2]), dict(params=c[2:])], weight_decay=0.02, **KW)
    oc.load_state_dict(copy.deepcopy(sd))
    d = [torch.nn.Parameter(p.detach().clone()) for p in a]
    od = Adam([dict(params=d[:2]), dict(params=d[2:])], weight_decay=0.02, max_grad_norm=2.0, **KW)
    od.load_state_dict(copy.deepcopy(oc.state_dict()))
    g = torch.Generator().manual_seed(6)
    for pa, pc, pd in zip(a, c, d):
        gr = torch.randn(pa.shape, generator=g)
        pa.grad, pc.grad, pd.grad = gr.clone(), gr.clone(), gr.clone()
    oa.step(); od.step()
    torch.nn.utils.clip_grad_norm_(c, 2.0)
    oc.step()
    for pa, pc, pd in zip(a, c, d):
        assert torch.equal(pa, pd) and torch.allclose(pc, pa, rtol=1e-6, atol=1e-7)


def test_constructor_and_argument_checks():
    from mas_hip.optim import Adam, AdamW, clip_grad_norm_
    p = _params(3)
    for cls in (Adam, AdamW):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                cls(p, max_grad_norm=bad)
        for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
            with pytest.raises(NotImplementedError):
                cls(p, max_grad_norm=1.0, **kw)
        assert cls(p).max_grad_norm is None and cls(p, max_grad_norm=3).max_grad_norm == 3.0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            clip_grad_norm_(p, bad)
    o = Adam(p, max_grad_norm=1.0)
    assert o.step() is None and all(len(o.state[q]) == 0 for q in p) and o.grad_norm is None       # no gradients: nothing happens
    # gradients on two devices (a meta tensor stands in for the second one): refused before any state is created or advanced
    two = [torch.nn.Parameter(torch.ones(2)), torch.nn.Parameter(torch.ones(2, device="meta"))]
    two[0].grad, two[1].grad = torch.ones(2), torch.ones(2, device="meta")
    o = Adam(two, max_grad_norm=1.0)
    with pytest.raises(NotImplementedError):
        o.step()
    with pytest.raises(NotImplementedError):
        clip_grad_norm_(two, 1.0)
    assert all(len(o.state[q]) == 0 for q in two) and torch.equal(two[0].grad, torch.ones(2))
    # a zero-numel parameter and a parameter without a gradient take no part; all-zero gradients give norm 0 and coefficient exactly 1
    q = [torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.zeros(0)), torch.nn.Parameter(torch.ones(2))]
    q[0].grad, q[1].grad = torch.zeros(4), torch.zeros(0)
    o = Adam(q, max_grad_norm=1.0)
    o.step()
    assert float(o.grad_norm) == 0.0 and float(o.clip_coef) == 1.0 and torch.equal(q[0], torch.ones(4)) and len(o.state[q[2]]) == 0
    # NaN stays NaN in the norm, in the coefficient and in every updated parameter (torch's error_if_nonfinite=False)
    q[0].grad, q[2].grad = torch.tensor([1.0, float("nan"), 0.0, 0.0]), torch.ones(2)
    o.step()
    assert torch.isnan(o.grad_norm) and torch.isnan(o.clip_coef) and torch.isnan(q[0]).all() and torch.isnan(q[2]).all()


def test_standalone_clip_grad_norm_on_cpu():
    from mas_hip.optim import clip_grad_norm_
    for m in (2.0, 100.0):
        a, b = _params(5), _params(5)
        g = torch.Generator().manual_seed(7)
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g)
            pa.grad, pb.grad = gr.clone(), gr.clone()
        a[1].grad = b[1].grad = None
        want = R.clip_coef(R.grad_norm([p.grad.numpy() for p in b if p.grad is not None]), m)
        got, ref = clip_grad_norm_(a, m), torch.nn.utils.clip_grad_norm_(b, m)
        assert got.dim() == 0 and got.dtype == torch.float32 and float(got) == float(want[0]) and abs(float(got) - float(ref)) <= 1e-6 * float(ref)
        for pa, pb in zip(a, b):
            assert (pa.grad is None and pb.grad is None) or torch.allclose(pa.grad, pb.grad, rtol=3e-7, atol=0)
    single = torch.nn.Parameter(torch.ones(4))
    single.grad = torch.full((4,), 3.0)
    assert float(clip_grad_norm_(single, 3.0)) == 6.0 and torch.allclose(single.grad, torch.full((4,), 1.5), rtol=1e-6)
    assert float(clip_grad_norm_([torch.nn.Parameter(torch.ones(2))], 1.0)) == 0.0           # no gradient at all


def test_header_declares_the_entries_and_they_validate_arguments_without_gpu():
    import mas_hip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mas_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in mas_hip.EXPORTS
    L = mas_hip.lib()
    assert L.mas_abi_version() == mas_hip.ABI_VERSION == 10
    for rc in (L.mas_grad_sqnorm_multi(None, 0, 0, None, None), L.mas_grad_sqnorm_multi(1, 1, 1, None, None),
               L.mas_grad_clip_coef(None, 0, None, 0, 1.0, None, None), L.mas_grad_clip_coef(None, 4, None, 0, 1.0, 1, None),
               L.mas_grad_clip_coef(1, 4, None, 2, 1.0, 1, None), L.mas_grad_clip_coef(1, 0, None, 0, 1.0, 1, None),
               L.mas_adam_multi_ex(None, 0, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, None, 1, None),
               L.mas_adam_multi_ex(None, 0, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, None, 0, None),
               L.mas_adam_multi_ex(1, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.001, 1, 1, None),      # step 0: no bias correction
               L.mas_grad_scale_multi(None, 0, 0, None, None), L.mas_grad_scale_multi(1, 1, 1, None, None)):
        assert rc == -1 and L.mas_last_error()
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert L.mas_grad_clip_coef(1, 4, None, 0, bad, 1, None) == -1 and b"max_norm" in L.mas_last_error()
