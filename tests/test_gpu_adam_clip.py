"""Global-norm clipping and AdamW of ``mas_hip.optim`` on the GPU (csrc/optim.hip: grad_sqnorm_multi, grad_clip_coef, adam_multi_ex,
grad_scale_multi) against the float64 helper tests/helpers/adam_clip_ref.py.

Bounds.  The norm: squares are exact in fp64, a sum of N <= 2^27 terms errs by at most N * 2^-53 ~ 1.5e-8 relative, the fp32 rounding of
the result adds 6e-8: relative error <= 5e-7 (NORM_TOL).  The update: torch's own fp32 GPU path (clip_grad_norm_ + fused Adam / AdamW) runs on
the same inputs against the same helper, and ours may err at most twice what that path errs over the whole parameter set (two fp32 paths
that round one coefficient differently), with the project's existing Adam bound 2e-6 as the floor."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import adam_clip_ref as R  # noqa: E402

# the smallest set at which the walk can go wrong: around the 4096-element block, two full blocks, a partial last block, 576 blocks (the
# coefficient kernel loops past one round of its 256 threads); plus, appended by _params: an unaligned view (element-wise path), a
# zero-numel parameter, a parameter that never has a gradient
SIZES = [(1,), (7,), (4095,), (4096,), (4097,), (8191,), (2, 4096), (100003,), (512, 512, 3, 3)]
NORM_TOL = 5e-7
KW = dict(lr=3e-3, betas=(0.5, 0.9), eps=1e-8)
STEPS = 6


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data():
    """initial values and the gradients of every step, once, on the host (the schedule of test_gpu_adam.py: the gradient scale grows with
    the step; parameter 2 sits step 3 out); entry -3 is the view, -2 the empty parameter, -1 never has a gradient"""
    g = torch.Generator().manual_seed(3)
    shapes = SIZES + [(1000,), (0,), (33,)]
    p0 = [torch.randn(*s, generator=g) for s in shapes]
    grads = []
    for step in range(STEPS):
        gs = [torch.randn(*s, generator=g) * (0.1 + step) for s in shapes]
        gs[-1] = None
        if step == 3:
            gs[2] = None
        grads.append(gs)
    return dict(p0=p0, grads=grads)


def _params(data, dev):
    ps = [torch.nn.Parameter(t.clone().to(dev)) for t in data["p0"]]
    base = torch.zeros(1001, device=dev)
    base[1:] = data["p0"][-3].to(dev)
    ps[-3] = torch.nn.Parameter(base[1:])            # storage offset 4 bytes: not 16-byte aligned
    assert ps[-3].data_ptr() % 16 == 4
    return ps


def _set_grads(ps, gs, dev, scale=1.0):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else (g * scale).to(dev)


def _np(ts):
    return [None if t is None else t.detach().double().cpu().numpy() for t in ts]


def _rel(a, b):
    """max |a - b| / max |b| of one tensor against its float64 reference"""
    b = torch.as_tensor(b)
    if b.numel() == 0:
        return 0.0
    return float((a.detach().double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _worst(ps, ref):
    return max(_rel(p, r) for p, r in zip(ps, ref))


@pytest.mark.parametrize("scale", [1.0, 1e20, 1e-30])
def test_norm_against_float64_at_three_scales(data, scale):
    """x1e20: an fp32 sum of squares overflows, the fp64 sum and the fp32 norm do not; x1e-30: fp32 squares underflow to zero"""
    from mas_hip import ops
    from mas_hip.optim import clip_grad_norm_
    dev = _dev()
    ps = _params(data, dev)
    _set_grads(ps, data["grads"][1], dev, scale)
    before = [None if p.grad is None else p.grad.clone() for p in ps]
    want = R.grad_norm(_np(before))
    got = clip_grad_norm_(ps, 1e30)                  # far above every norm here: the coefficient is exactly 1
    assert ops.last_kernel() == "grad_scale_multi"
    again = clip_grad_norm_(ps, 1e30)
    err = abs(float(got.double()) - want) / want
    print(f"scale {scale:g}: norm {float(got):.9g}, float64 {want:.17g}, relative error {err:.3g} (bound {NORM_TOL:g})")
    assert got.dtype == torch.float32 and got.dim() == 0 and got.device == dev
    assert err <= NORM_TOL
    assert torch.equal(got, again)                   # fixed summation order: the same bits
    assert all(b is None or torch.equal(p.grad, b) for p, b in zip(ps, before))     # multiplied by exactly 1


def test_norm_of_zero_gradients_and_of_one_element(data):
    from mas_hip.optim import Adam, clip_grad_norm_
    dev = _dev()
    ps = _params(data, dev)
    start = [p.detach().clone() for p in ps]
    _set_grads(ps, [None if g is None else torch.zeros_like(g) for g in data["grads"][0]], dev)
    opt = Adam(ps, max_grad_norm=1.0, **KW)
    opt.step()
    assert float(opt.grad_norm) == 0.0 and float(opt.clip_coef) == 1.0
    assert all(torch.equal(p, s) for p, s in zip(ps, start))
    one = torch.nn.Parameter(torch.ones(1, device=dev))
    one.grad = torch.full((1,), -3.0, device=dev)
    n = clip_grad_norm_(one, 1.5)
    want_n, want_c = R.clip_coef(3.0, 1.5)
    assert float(n) == float(want_n) == 3.0 and float(one.grad) == float(np.float32(-3.0) * want_c)


def test_nan_gradient_stays_nan(data):
    """one NaN element: NaN norm, NaN coefficient (the clamp must not turn it into 1), every updated parameter NaN -- as with torch"""
    from mas_hip.optim import Adam
    dev = _dev()
    ours, theirs = _params(data, dev), _params(data, dev)
    _set_grads(ours, data["grads"][0], dev)
    ours[4].grad[1234] = float("nan")
    for po, pt in zip(ours, theirs):
        pt.grad = None if po.grad is None else po.grad.clone()
    opt = Adam(ours, max_grad_norm=1.0, **KW)
    opt.step()
    real = [p for p in theirs if p.numel()]          # (the yardstick needs no empty parameter)
    torch.nn.utils.clip_grad_norm_(real, 1.0)
    torch.optim.Adam(real, fused=True, **KW).step()
    assert bool(torch.isnan(opt.grad_norm)) and bool(torch.isnan(opt.clip_coef))
    for po, pt in zip(ours, theirs):
        if po.grad is None:
            assert torch.equal(po, pt)
        else:
            assert bool(torch.isnan(po).all()) and bool(torch.isnan(pt).all())


# the norms of the six steps are about 158, 1.7e3, 3.3e3, 4.9e3, 6.5e3, 8.0e3 (2.49 M unit-normal elements x (0.1 + step))
@pytest.mark.parametrize("m", [1e5, 4000.0, 1.0], ids=["never", "from_step_3", "always"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_clipped_steps_against_float64(data, decoupled, wd, m):
    from mas_hip import ops
    from mas_hip.optim import Adam, AdamW
    dev = _dev()
    ours, theirs = _params(data, dev), _params(data, dev)
    opt = (AdamW if decoupled else Adam)(ours, weight_decay=wd, max_grad_norm=m, **KW)
    ref_params = [p for p in theirs if p.numel()]                          # (the yardstick needs no empty parameter)
    ref_opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ref_params, weight_decay=wd, fused=True, **KW)
    coefs = []
    for gs in data["grads"]:
        _set_grads(ours, gs, dev)
        _set_grads(theirs, gs, dev)
        kept = [None if p.grad is None else p.grad.clone() for p in ours]
        opt.step()
        assert ops.last_kernel() == "adam_multi_ex"
        assert all(k is None or torch.equal(p.grad, k) for p, k in zip(ours, kept))     # gradients are not modified
        coefs.append((opt.grad_norm.clone(), opt.clip_coef.clone()))
        torch.nn.utils.clip_grad_norm_(ref_params, m)
        ref_opt.step()
    want, log = R.adam_steps(_np(data["p0"]), [_np(gs) for gs in data["grads"]], KW["lr"], KW["betas"], KW["eps"], wd, max_grad_norm=m,
                             decoupled=decoupled)
    clipped = [float(c) < 1.0 for _, c in coefs]
    assert clipped == {1e5: [False] * 6, 4000.0: [False] * 3 + [True] * 3, 1.0: [True] * 6}[m], coefs
    for (n, c), (n32, c32) in zip(coefs, log):
        assert abs(float(n) - float(n32)) <= NORM_TOL * float(n32)
        assert abs(float(c) - float(c32)) <= 2 * NORM_TOL * float(c32)     # the coefficient of a norm within NORM_TOL, one more rounding
    e_ours, e_torch = _worst(ours, want), _worst(theirs, want)
    bound = max(2.0 * e_torch, 2e-6)
    print(f"{'AdamW' if decoupled else 'Adam'} wd {wd} max_grad_norm {m:g}: ours {e_ours:.3g}, torch fused {e_torch:.3g}, bound {bound:.3g}")
    assert e_ours <= bound
    for p in ours:
        if p.grad is not None and p.numel():
            assert int(opt.state[p]["step"]) == (5 if p is ours[2] else 6)


def test_unclipped_step_still_ends_in_adam_multi(data):
    from mas_hip import ops
    from mas_hip.optim import Adam, AdamW
    dev = _dev()
    for cls, kernel in ((Adam, "adam_multi"), (AdamW, "adam_multi_ex")):
        ps = _params(data, dev)
        _set_grads(ps, data["grads"][0], dev)
        opt = cls(ps, **KW)
        opt.step()
        assert ops.last_kernel() == kernel and opt.grad_norm is None and opt.clip_coef is None


def test_mixed_step_counts_share_one_global_norm():
    """b joins after a has taken two steps: two Adam launches (own bias corrections each), ONE norm over both"""
    from mas_hip.optim import Adam
    dev = _dev()
    g = torch.Generator().manual_seed(0)
    a0, b0, ga, gb = (torch.randn(n, generator=g) for n in (5000, 777, 5000, 777))
    m = 60.0                                         # |ga| ~ 71, |gb| ~ 28: clips from the first step on
    ours, theirs = [[torch.nn.Parameter(t.clone().to(dev)) for t in (a0, b0)] for _ in range(2)]
    opt, ref = Adam(ours, lr=1e-2, max_grad_norm=m), torch.optim.Adam(theirs, lr=1e-2, fused=True)
    sched = []
    for k in range(5):
        gs = [ga * (k + 1), gb * (k + 1) if k >= 2 else None]
        sched.append(gs)
        for ps in (ours, theirs):
            for p, x in zip(ps, gs):
                p.grad = None if x is None else x.clone().to(dev)
        opt.step()
        torch.nn.utils.clip_grad_norm_(theirs, m)
        ref.step()
        want_n = R.grad_norm(_np(gs))
        assert abs(float(opt.grad_norm) - want_n) <= NORM_TOL * want_n
    want, _ = R.adam_steps(_np([a0, b0]), [_np(gs) for gs in sched], 1e-2, (0.9, 0.999), 1e-8, 0.0, max_grad_norm=m)
    e_ours, e_torch = _worst(ours, want), _worst(theirs, want)
    print(f"mixed step counts: ours {e_ours:.3g}, torch fused {e_torch:.3g}")
    assert e_ours <= max(2.0 * e_torch, 2e-6)
    assert int(opt.state[ours[0]]["step"]) == 5 and int(opt.state[ours[1]]["step"]) == 3


def test_parameter_the_table_cannot_hold_enters_through_extra():
    """a non-contiguous CUDA parameter: its squared norm reaches the coefficient launch through `extra`, and the torch expression that
    updates it multiplies its gradient by the same device coefficient"""
    from mas_hip.optim import Adam
    dev = _dev()
    g = torch.Generator().manual_seed(1)
    w0, t0 = torch.randn(5000, generator=g), torch.randn(40, 30, generator=g)
    gw, gt = torch.randn(5000, generator=g), torch.randn(40, 30, generator=g)
    w, t = torch.nn.Parameter(w0.clone().to(dev)), torch.nn.Parameter(t0.clone().to(dev).t())
    assert not t.is_contiguous()
    w.grad, t.grad = gw.clone().to(dev), gt.clone().to(dev).t()
    opt = Adam([w, t], lr=1e-2, weight_decay=0.01, max_grad_norm=5.0)
    opt.step()
    want, log = R.adam_steps(_np([w0, t0.t()]), [_np([gw, gt.t()])], 1e-2, (0.9, 0.999), 1e-8, 0.01, max_grad_norm=5.0)
    assert abs(float(opt.grad_norm) - float(log[0][0])) <= NORM_TOL * float(log[0][0]) and float(opt.clip_coef) < 0.1
    assert _rel(w, want[0]) <= 2e-6 and _rel(t, want[1]) <= 2e-6
    # only such parameters: no table at all, the coefficient launch runs on `extra` alone
    t.grad = gt.clone().to(dev).t()
    only = Adam([t], lr=1e-2, max_grad_norm=5.0)
    only.step()
    want_n = R.grad_norm(_np([gt]))
    assert abs(float(only.grad_norm) - want_n) <= NORM_TOL * want_n


@pytest.mark.parametrize("m", [1000.0, 1e5], ids=["clips", "does_not_clip"])
def test_standalone_clip_grad_norm(data, m):
    from mas_hip.optim import clip_grad_norm_
    dev = _dev()
    ours, theirs = _params(data, dev), _params(data, dev)
    _set_grads(ours, data["grads"][1], dev)
    _set_grads(theirs, data["grads"][1], dev)
    before = _np([p.grad for p in ours])
    got = clip_grad_norm_(ours, m)
    ref = torch.nn.utils.clip_grad_norm_([p for p in theirs if p.numel()], m)
    want_n, want_c = R.clip_coef(R.grad_norm(before), m)
    err = abs(float(got.double()) - R.grad_norm(before)) / R.grad_norm(before)
    ulps = 0
    for po, pt, b in zip(ours, theirs, before):
        if b is None or b.size == 0:
            assert (po.grad is None and pt.grad is None) or po.grad.numel() == 0
            continue
        ulps = max(ulps, int((po.grad.view(torch.int32) - pt.grad.view(torch.int32)).abs().max()))
        # in place, by the helper's coefficient: a norm within one fp32 ulp of the helper's (1.2e-7), the sum and the quotient of the
        # coefficient and the product rounded once on either side (6e-8 each)
        assert _rel(po.grad, b * float(want_c)) <= 5e-7
    print(f"max_norm {m:g}: norm error {err:.3g}; torch's norm {float(ref):.9g} vs {float(got):.9g}; gradients within {ulps} ulp of torch's")
    assert err <= NORM_TOL and (float(want_c) < 1.0) == (m == 1000.0)
    assert ulps <= 2


def test_clipped_steps_do_not_synchronise_the_host(data):
    from mas_hip.optim import AdamW
    dev = _dev()
    ps = _params(data, dev)
    fresh = [[None if g is None else g.to(dev) for g in gs] for gs in data["grads"][:3]]
    opt = AdamW(ps, max_grad_norm=1.0, **KW)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gs in fresh:                             # three table changes: inside the ring of four, whose own event wait does not come up
            for p, g in zip(ps, gs):
                p.grad = g
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert opt.grad_norm.is_cuda and opt.grad_norm.dim() == 0 and float(opt.clip_coef) < 1.0


def test_model_level_token_loss_then_clipped_adamw():
    """one token_loss(...).backward() under bf16 autocast on the tiny MakeAScene of the transformer tests, then AdamW(max_grad_norm=1).step():
    against the float64 helper, with torch's clip + fused AdamW on cloned parameters as the yardstick; the post-step hook saw the step"""
    from mas_hip import ops
    from mas_hip.optim import AdamW
    from models.transformer import MakeAScene
    from oracle import transformer_oracle as TO
    dev = _dev()
    cfg = dict(num_layers=2, hidden_dim=64, num_attn_heads=4, image_vocab_size=128, seg_vocab_size=40, text_vocab_size=58,
               image_tokens_per_dim=4, seg_tokens_per_dim=2, text_length=8)
    model = MakeAScene(**cfg)
    model.load_state_dict(TO.synth_transformer_state_dict(cfg, seed=7), strict=True)
    model = model.to(dev)
    text, seg, img = (t.to(dev) for t in TO.synth_tokens(cfg, batch=2, seed=7))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = model.token_loss(text, seg, img)
    loss.backward()
    ps = [p for p in model.parameters() if p.grad is not None]
    assert len(ps) > 10 and all(p.grad.dtype == torch.float32 for p in ps)
    p0, g0 = _np(ps), _np([p.grad for p in ps])
    clones = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for c, p in zip(clones, ps):
        c.grad = p.grad.clone()
    stamps = [ops._param_stamp(p) for p in ps]
    kw = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    opt = AdamW(ps, max_grad_norm=1.0, **kw)
    opt.step()
    torch.nn.utils.clip_grad_norm_(clones, 1.0)
    torch.optim.AdamW(clones, fused=True, **kw).step()
    want, log = R.adam_steps(p0, [g0], kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"], max_grad_norm=1.0, decoupled=True)
    assert abs(float(opt.grad_norm) - float(log[0][0])) <= NORM_TOL * float(log[0][0])
    e_ours, e_torch = _worst(ps, want), _worst(clones, want)
    print(f"model level: norm {float(opt.grad_norm):.6g}, coefficient {float(opt.clip_coef):.6g}; ours {e_ours:.3g}, torch fused {e_torch:.3g}")
    assert e_ours <= max(2.0 * e_torch, 2e-6)
    assert all(ops._param_stamp(p)[2] == s[2] + 1 for p, s in zip(ps, stamps))
