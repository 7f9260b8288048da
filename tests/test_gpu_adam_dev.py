"""``mas_hip.optim.Adam / AdamW(device_step=True)`` on the GPU (optim.hip: ``mas_adam_multi_dev`` + ``mas_adam_advance_dev``): against the
float64 helper (tests/helpers/adam_dev_ref.py) and against the host-step optimizer on the same inputs within the 2e-6 of
tests/test_gpu_adam.py, step counts on the device, state_dict interchange with torch.optim.Adam(fused=True), clipping, EMA warm-up, the
non-finite guard, learning-rate changes, no host synchronisation, and ``step()`` captured into a graph."""
import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import adam_dev_ref as D  # noqa: E402

SIZES = [(1,), (7,), (128,), (4096,), (4097,), (3, 5, 7), (100003,), (512, 512, 3, 3), (8191,), (2, 4096)]      # tests/test_gpu_adam.py's
SMALL = [(1,), (7,), (4096,), (4097,), (3, 5, 7), (8191,), (2, 4096)]
TOL = 2e-6
KEYS = ("exp_avg", "exp_avg_sq", "ema")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _params(dev, seed, sizes=SIZES, unaligned=True):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in sizes]
    if unaligned:                        # storage offset 4 bytes -> the element-wise path of the kernel
        ps.append(torch.nn.Parameter(torch.randn(1001, generator=g).to(dev)[1:]))
    return ps


def _grad_steps(ps, seed, steps, absent=()):
    g = torch.Generator().manual_seed(seed)
    return [[None if (k, i) in absent else torch.randn(p.shape, generator=g) * (0.1 + k) for i, p in enumerate(ps)] for k in range(steps)]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.to(p.device).clone()


def _rel(a, b):
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a.detach().double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _np(ts):
    return [None if t is None else t.detach().double().cpu().numpy() for t in ts]


def _bits(opt, ps):
    return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in KEYS if k in opt.state[p]]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _worst_vs(ref, opt, ps):
    """largest relative error of p, both moments and the average against the helper's dict"""
    worst = 0.0
    for i, p in enumerate(ps):
        st = opt.state[p]
        worst = max(worst, _rel(p, ref["p"][i]), _rel(st["exp_avg"], ref["m"][i]), _rel(st["exp_avg_sq"], ref["v"][i]))
        if ref["ema"] is not None:
            worst = max(worst, _rel(st["ema"], ref["ema"][i]))
    return worst


@pytest.mark.parametrize("betas", [(0.5, 0.9), (0.9, 0.999)])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_matches_float64_and_the_host_step(decoupled, wd, betas):
    from mas_hip import ops
    from mas_hip.optim import Adam, AdamW
    dev = _dev()
    cls = AdamW if decoupled else Adam
    ours, host = _params(dev, 3), _params(dev, 3)
    kw = dict(lr=3e-3, betas=betas, eps=1e-8, weight_decay=wd, ema_decay=0.9)
    o, h = cls(ours, device_step=True, **kw), cls(host, **kw)
    grads = _grad_steps(ours, 5, 6, absent={(3, 2)})                 # a parameter that sits a step out
    start = _np(ours)
    for gs in grads:
        _set(ours, gs), _set(host, gs)
        h.step()
        assert ops.last_kernel() == "adam_multi_ema"
        o.step()
        assert ops.last_kernel() == "adam_advance_dev"
    ref = D.adam_dev_steps(start, [_np(gs) for gs in grads], 3e-3, betas, 1e-8, wd, decoupled=decoupled, ema_decay=0.9)
    worst = _worst_vs(ref, o, ours)
    print(f"device_step vs float64, worst error / 2e-6: {worst / TOL:.3f}")
    assert worst < TOL, worst
    # against the host-step optimizer on the same inputs, directly
    ratio = 0.0
    for po, ph in zip(ours, host):
        so, sh = o.state[po], h.state[ph]
        assert so["step"].is_cuda and so["step"].dim() == 0 and so["step"].dtype == torch.float32
        assert int(so["step"]) == int(sh["step"])
        for a, b in ((po, ph), (so["exp_avg"], sh["exp_avg"]), (so["exp_avg_sq"], sh["exp_avg_sq"]), (so["ema"], sh["ema"])):
            ratio = max(ratio, _rel(a, b.detach().double().cpu()) / TOL)
    print(f"device_step vs host step, worst error / 2e-6: {ratio:.3f}")
    assert ratio < 1.0, ratio
    # one vector behind all the counts
    vec = o._dev["vec"]
    assert all(o.state[p]["step"].data_ptr() == vec.data_ptr() + 4 * (1 + i) for i, p in enumerate(ours))


def test_state_dict_interchange_with_torch_fused_adam():
    from mas_hip.optim import Adam
    dev = _dev()
    a, b = _params(dev, 9, SMALL), _params(dev, 9, SMALL)
    oa = Adam(a, lr=1e-3, betas=(0.5, 0.9), device_step=True)
    ob = torch.optim.Adam(b, lr=1e-3, betas=(0.5, 0.9), fused=True)
    grads = _grad_steps(a, 1, 4)
    for gs in grads[:2]:
        _set(a, gs), _set(b, gs)
        oa.step(), ob.step()
    sd = oa.state_dict()
    assert all(s["step"].is_cuda and s["step"].dim() == 0 and s["step"].dtype == torch.float32 for s in sd["state"].values())
    assert all(s["step"].data_ptr() != oa.state[p]["step"].data_ptr() for s, p in zip(sd["state"].values(), a))        # copies, not views
    # ours -> torch's fused, torch's fused -> ours, then one more step everywhere
    c, d = [torch.nn.Parameter(p.detach().clone()) for p in a], [torch.nn.Parameter(p.detach().clone()) for p in b]
    oc = torch.optim.Adam(c, lr=1e-3, betas=(0.5, 0.9), fused=True)
    od = Adam(d, lr=1e-3, betas=(0.5, 0.9), device_step=True)
    to_torch = copy.deepcopy(sd)
    for g in to_torch["param_groups"]:
        g["fused"] = True                                             # (the groups travel with the state: the target stays the fused one)
    oc.load_state_dict(to_torch)
    od.load_state_dict(copy.deepcopy(ob.state_dict()))
    for ps in (a, b, c, d):
        _set(ps, grads[2])
    oa.step(), ob.step(), oc.step(), od.step()
    for pa, pb, pc, pd in zip(a, b, c, d):
        assert _rel(pc, pa.detach().double().cpu()) < TOL and _rel(pd, pb.detach().double().cpu()) < TOL and _rel(pa, pb.detach().double().cpu()) < TOL
        assert int(od.state[pd]["step"]) == int(oa.state[pa]["step"]) == 3
    # and back into itself IN PLACE: the storage of the state does not move, the generation does
    before = {p: {k: v.data_ptr() for k, v in oa.state[p].items()} for p in a}
    gen = oa.state_generation
    oa.load_state_dict(copy.deepcopy(oc.state_dict()))
    assert oa.state_generation == gen + 1
    assert all(oa.state[p][k].data_ptr() == ptr for p in a for k, ptr in before[p].items())
    for ps in (a, c):
        _set(ps, grads[3])
    oa.step(), oc.step()
    for pa, pc in zip(a, c):
        assert _rel(pa, pc.detach().double().cpu()) < TOL and int(oa.state[pa]["step"]) == 4


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_clipping_and_ema_warmup(decoupled):
    from mas_hip.optim import Adam, AdamW
    dev = _dev()
    ps = _params(dev, 4, SMALL)
    opt = (AdamW if decoupled else Adam)(ps, lr=2e-3, betas=(0.9, 0.999), weight_decay=0.01, max_grad_norm=1.5, ema_decay=0.9, ema_warmup=True,
                                         device_step=True)
    grads = _grad_steps(ps, 6, 5, absent={(1, 0)})
    start = _np(ps)
    for gs in grads:
        _set(ps, gs)
        opt.step()
        assert float(opt.clip_coef) < 1.0                             # the clip is active at every step
    ref = D.adam_dev_steps(start, [_np(gs) for gs in grads], 2e-3, (0.9, 0.999), 1e-8, 0.01, decoupled=decoupled, max_grad_norm=1.5,
                           ema_decay=0.9, ema_warmup=True)
    assert abs(float(opt.grad_norm) - ref["norms"][-1]) <= 1e-6 * ref["norms"][-1]
    worst = _worst_vs(ref, opt, ps)
    assert worst < TOL, worst
    sd = opt.state_dict()
    assert sd["param_groups"][0]["ema_step"] == 5 == ref["k"] and [int(opt.state[p]["step"]) for p in ps] == ref["t"]


def test_skip_nonfinite_keeps_every_bit_and_advances_the_count():
    from mas_hip.optim import Adam
    dev = _dev()
    ps = _params(dev, 4, SMALL)
    opt = Adam(ps, lr=2e-3, betas=(0.5, 0.9), weight_decay=0.01, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True, device_step=True)
    grads = _grad_steps(ps, 7, 4)
    for gs in grads[:2]:
        _set(ps, gs)
        opt.step()
        assert bool(opt.step_skipped) is False
    before = _bits(opt, ps)
    poisoned = [g.clone() for g in grads[2]]
    poisoned[3][17] = float("nan")
    _set(ps, poisoned)
    opt.step()
    assert _same(_bits(opt, ps), before)
    assert bool(opt.step_skipped) is True and all(int(opt.state[p]["step"]) == 3 for p in ps)
    _set(ps, grads[3])
    opt.step()
    assert bool(opt.step_skipped) is False and not _same(_bits(opt, ps), before)
    start = _np(_params(dev, 4, SMALL))
    ref = D.adam_dev_steps(start, [_np(gs) for gs in grads[:2]] + [_np(poisoned), _np(grads[3])], 2e-3, (0.5, 0.9), 1e-8, 0.01, ema_decay=0.9,
                           ema_warmup=True, skip_nonfinite=True)
    assert ref["skipped"] == [False, False, True, False]
    assert _worst_vs(ref, opt, ps) < TOL and opt.state_dict()["param_groups"][0]["ema_step"] == 4


def test_lr_change_takes_effect_at_the_next_step():
    from mas_hip.optim import Adam
    dev = _dev()
    ps = _params(dev, 4, SMALL)
    opt = Adam(ps, lr=2e-3, betas=(0.5, 0.9), device_step=True)
    grads = _grad_steps(ps, 8, 4)
    lrs = [2e-3, 5e-4, 5e-4, 1e-3]
    start = _np(ps)
    for k, gs in enumerate(grads):
        if k == 1:
            opt.param_groups[0]["lr"] = 5e-4                          # a float
        if k == 3:
            opt.param_groups[0]["lr"] = torch.tensor(1e-3)            # a 0-dim tensor
        _set(ps, gs)
        opt.step()
    ref = D.adam_dev_steps(start, [_np(gs) for gs in grads], lrs, (0.5, 0.9), 1e-8, 0.0)
    assert _worst_vs(ref, opt, ps) < TOL
    stale = D.adam_dev_steps(start, [_np(gs) for gs in grads], 2e-3, (0.5, 0.9), 1e-8, 0.0)      # (the test can tell: the old lr is far off)
    assert _rel(ps[2], stale["p"][2]) > 1e-4
    assert torch.is_tensor(opt.param_groups[0]["lr"])


def test_no_host_synchronisation_in_a_step_loop():
    from mas_hip.optim import AdamW
    dev = _dev()
    ps = _params(dev, 4, SMALL)
    opt = AdamW(ps, lr=2e-3, max_grad_norm=1.0, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True, device_step=True)
    grads = [[g.to(dev) for g in gs] for gs in _grad_steps(ps, 9, 4)]
    opt.init_state()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k, gs in enumerate(grads):
            for p, g in zip(ps, gs):
                p.grad = g
            if k == 2:
                opt.param_groups[0]["lr"] = 1e-3
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(int(opt.state[p]["step"]) == 4 for p in ps)


def test_step_under_capture_needs_init_state_and_replays_bit_for_bit():
    """step() alone captured on a side stream, three replays against three eager device_step steps, the gradients written into static
    ``.grad`` tensors: the same kernel on the same inputs, so every bit of the state agrees"""
    from mas_hip.optim import AdamW
    dev = _dev()
    kw = dict(lr=2e-3, betas=(0.9, 0.999), weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True, device_step=True)
    a, b = _params(dev, 4, SMALL), _params(dev, 4, SMALL)
    oa, ob = AdamW(a, **kw), AdamW(b, **kw)
    grads = [[g.to(dev) for g in gs] for gs in _grad_steps(a, 10, 4)]
    for ps in (a, b):
        for p, g in zip(ps, grads[0]):
            p.grad = g.clone()
    ob.step()                                                         # eager: step 1 of 4
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=dev)
    fresh = AdamW(_params(dev, 4, SMALL), **kw)
    for p, g in zip(fresh.param_groups[0]["params"], grads[0]):
        p.grad = g.clone()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        scratch = torch.zeros(8, device=dev)
        with pytest.raises(RuntimeError, match="init_state"):
            with torch.cuda.graph(graph, stream=side):
                scratch.add_(1.0)
                fresh.step()                                          # no state yet: refused instead of allocated inside the capture
        oa.step()                                                     # warm-up on the capture stream: step 1 of 4
        oa.init_state()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            oa.step()
    main.wait_stream(side)
    assert _same(_bits(oa, a), _bits(ob, b))                          # the capture executed nothing
    for k in (1, 2, 3):
        for ps in (a, b):
            for p, g in zip(ps, grads[k]):
                p.grad.copy_(g)
        if k == 2:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 1e-3
            oa.sync_hyperparameters()
        graph.replay()
        ob.step()
        torch.cuda.synchronize()
        assert _same(_bits(oa, a), _bits(ob, b)), k
        assert torch.equal(oa._dev["vec"], ob._dev["vec"]) and int(oa.state[a[0]]["step"]) == k + 1
    assert oa.state_dict()["param_groups"][0]["ema_step"] == 4
