"""The EMA of the weights inside the one-launch Adam, the non-finite guard and the swap (csrc/optim.hip: adam_multi_kernel<*, *, true>,
swap_multi_kernel; ``mas_hip.optim`` ``ema_decay`` / ``skip_nonfinite`` / ``swap_ema()``) on the GPU.

Bounds.  p, exp_avg, exp_avg_sq with ``ema_decay`` are BITWISE those of the same optimizer without it.  The EMA after k steps:
|ema - ref64| <= k * 2^-22 * max(|p|, |ema|) elementwise, ref64 the float64 recurrence of tests/helpers/adam_ema_ref.py driven by the GPU's
own p after each step -- each step rounds twice in fp32 (the difference, the fused multiply-add), each by at most half an ulp of a value no
larger than 2 max(|p|, |e|): 2^-23 max per step, taken with a factor 2.  Against the all-float64 run (Adam from adam_clip_ref.py) p keeps the
project's Adam bound 2e-6 (max |dp| / max |p| per tensor), and the EMA that bound plus k * 2^-22: it averages those p."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import adam_ema_ref as E  # noqa: E402

# around the 4096-element block, two full blocks and a tail; then, appended by _params: storage offset by one element with a full block
# (element-wise path on a full block), an empty parameter, a parameter that never has a gradient
SIZES = [1, 3, 4095, 4096, 4097, 2 * 4096 + 5]
OFFSET_N = 4096 + 9
POISONED = 4                                         # index of the 4097-element tensor
KW = dict(lr=3e-3, betas=(0.5, 0.9), eps=1e-8)
STEPS = 5
STATE = ("exp_avg", "exp_avg_sq")
CONFIGS = {"plain": (False, None), "clipped": (False, 20.0), "adamw": (True, None), "adamw_clipped": (True, 20.0)}    # norms: about 157 x (0.1 + step) -- 20 clips from the second step on


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    sizes = SIZES + [OFFSET_N, 0, 33]
    p0 = [torch.randn(n, generator=g) for n in sizes]
    grads = []
    for step in range(STEPS):
        gs = [torch.randn(n, generator=g) * (0.1 + step) for n in sizes]
        gs[-1] = None
        if step == 2:
            gs[1] = None
        grads.append(gs)
    return dict(p0=p0, grads=grads)


def _params(data, dev):
    ps = [torch.nn.Parameter(t.clone().to(dev)) for t in data["p0"]]
    base = torch.empty(OFFSET_N + 1, device=dev)
    base[1:] = data["p0"][-3].to(dev)
    ps[-3] = torch.nn.Parameter(base[1:])            # storage offset 4 bytes: not 16-byte aligned
    assert ps[-3].data_ptr() % 16 == 4
    return ps


def _set_grads(ps, gs, dev):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.to(dev)


def _opt(ps, decoupled, m, **kw):
    from mas_hip.optim import Adam, AdamW
    return (AdamW if decoupled else Adam)(ps, weight_decay=0.01, max_grad_norm=m, **KW, **kw)


def _bits(opt, ps, keys=STATE + ("ema",)):
    return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in keys if k in opt.state[p]]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _rel(a, b):
    b = torch.as_tensor(b)
    return 0.0 if b.numel() == 0 else float((a.detach().double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("config", list(CONFIGS))
def test_ema_in_the_launch_leaves_the_update_alone_and_is_within_its_bound(data, config):
    from mas_hip import ops
    dev = _dev()
    decoupled, m = CONFIGS[config]
    a, b = _params(data, dev), _params(data, dev)
    oa, ob = _opt(a, decoupled, m, ema_decay=0.9), _opt(b, decoupled, m)
    ref = [_np(p) for p in a]
    worst = 0.0
    for k, gs in enumerate(data["grads"]):
        _set_grads(a, gs, dev)
        _set_grads(b, gs, dev)
        kept = [oa.state[p]["ema"].clone() if "ema" in oa.state[p] else None for p in a]
        oa.step()
        assert ops.last_kernel() == "adam_multi_ema"
        ob.step()
        assert _same(_bits(oa, a, STATE), _bits(ob, b, STATE))                     # the EMA does not disturb p, exp_avg, exp_avg_sq
        for i, (p, g) in enumerate(zip(a, gs)):
            if g is None:
                assert ("ema" not in oa.state[p]) if kept[i] is None else torch.equal(oa.state[p]["ema"], kept[i])     # no gradient: kept
                continue
            ema = oa.state[p]["ema"]
            assert ema.dtype == torch.float32 and ema.shape == p.shape and ema.device == p.device
            if p.numel() == 0:
                continue
            ref[i] = E.ema_update(ref[i], _np(p), 0.9)
            err, bound = np.abs(_np(ema) - ref[i]), E.ema_bound(k + 1, _np(p), _np(ema))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (config, k, i, float((err / np.maximum(bound, 1e-300)).max()))
            assert p.numel() < 3 or not torch.equal(ema, p.detach())
    print(f"{config}: worst |ema - ref64| / bound over {STEPS} steps {worst:.3g}")
    assert "ema" not in oa.state[a[-1]] and len(oa.state[a[-1]]) == 0                # never had a gradient: no state at all
    assert oa.param_groups[0]["ema_step"] == STEPS


def test_unaligned_ema_alone_takes_the_element_path(data):
    """p, g and both moments 16-byte aligned and the EMA not (a state loaded into a view): the kernel must not take float4 accesses on it.
    The EMA is checked against the recurrence driven by the kernel's own p; p itself is on the element-wise path of the other tests."""
    dev = _dev()
    p = torch.nn.Parameter(data["p0"][5].clone().to(dev))                            # two full blocks and a tail
    opt = _opt([p], False, 20.0, ema_decay=0.9)
    ref = _np(p)
    for k, gs in enumerate(data["grads"][:3]):
        p.grad = gs[5].to(dev)
        if k == 1:
            st = opt.state[p]
            st["ema"] = torch.empty(p.numel() + 1, device=dev)[1:].copy_(st["ema"])
            assert st["ema"].data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0
        opt.step()
        ref = E.ema_update(ref, _np(p), 0.9)
        ema = opt.state[p]["ema"]
        assert (np.abs(_np(ema) - ref) <= E.ema_bound(k + 1, _np(p), _np(ema))).all()
    assert ema.data_ptr() % 16 == 4 and bool(torch.isfinite(p).all())


def test_ema_warmup_uses_the_schedule(data):
    dev = _dev()
    a = _params(data, dev)
    opt = _opt(a, False, None, ema_decay=0.999, ema_warmup=True)
    ref = [_np(p) for p in a]
    for k, gs in enumerate(data["grads"][:3]):
        _set_grads(a, gs, dev)
        opt.step()
        for i, (p, g) in enumerate(zip(a, gs)):
            if g is not None and p.numel():
                ref[i] = E.ema_update(ref[i], _np(p), E.warmup_decay(0.999, k))      # 0.1, 2/11, 3/12: far from 0.999
                assert (np.abs(_np(opt.state[p]["ema"]) - ref[i]) <= E.ema_bound(k + 1, _np(p), _np(opt.state[p]["ema"]))).all()


@pytest.mark.parametrize("m", [None, 20.0], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_guard_keeps_every_bit_and_the_next_step_is_the_step_one_count_ahead(data, bad, m):
    from mas_hip import ops
    dev = _dev()
    a, b, c = _params(data, dev), _params(data, dev), _params(data, dev)
    oa, ob = _opt(a, False, m, ema_decay=0.9, skip_nonfinite=True), _opt(b, False, m, ema_decay=0.9)
    for gs in data["grads"][:2]:
        _set_grads(a, gs, dev)
        _set_grads(b, gs, dev)
        oa.step()
        assert ops.last_kernel() == "adam_multi_ema" and bool(oa.step_skipped) is False
        ob.step()
    assert _same(_bits(oa, a), _bits(ob, b))         # a finite norm: the guarded step keeps the bits of the unguarded one
    before = _bits(oa, a)
    poisoned = [None if g is None else g.clone() for g in data["grads"][2]]
    poisoned[POISONED][1234] = bad
    _set_grads(a, poisoned, dev)
    oa.step()
    skipped = oa.step_skipped
    assert skipped.dtype == torch.bool and skipped.dim() == 0 and skipped.device == dev and bool(skipped) is True
    assert _same(_bits(oa, a), before)               # p, exp_avg, exp_avg_sq, ema of EVERY tensor
    assert not bool(torch.isfinite(oa.grad_norm))
    # the following finite step: the unguarded optimizer with every count one ahead (the parameters that had a gradient at the skipped step)
    for p, g in zip(b, poisoned):
        if g is not None:
            ob.state[p]["step"] += 1
    _set_grads(a, data["grads"][3], dev)
    _set_grads(b, data["grads"][3], dev)
    oa.step()
    ob.step()
    assert bool(oa.step_skipped) is False and _same(_bits(oa, a), _bits(ob, b)) and not _same(_bits(oa, a), before)
    # the same gradient without the guard behaves as before: the weights are gone
    oc = _opt(c, False, m, ema_decay=0.9)
    _set_grads(c, poisoned, dev)
    oc.step()
    assert not bool(torch.isfinite(c[POISONED]).all()) and not bool(torch.isfinite(oc.state[c[POISONED]]["ema"]).all())
    if m is not None and bad != bad:                 # a NaN norm is a NaN coefficient: every updated tensor
        assert not any(bool(torch.isfinite(p).all()) for p, g in zip(c, poisoned) if g is not None and p.numel())


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_skipped_first_step_then_the_float64_run(data, decoupled):
    dev = _dev()
    a = _params(data, dev)
    opt = _opt(a, decoupled, 20.0, ema_decay=0.9, skip_nonfinite=True)
    grads = [[None if g is None else g.clone() for g in gs] for gs in data["grads"][:4]]
    grads[0][POISONED][7] = float("nan")
    for k, gs in enumerate(grads):
        _set_grads(a, gs, dev)
        opt.step()
        assert bool(opt.step_skipped) is (k == 0)
    want_p, want_e, _ = E.adam_ema_steps([_np(t) for t in data["p0"]], [[_np(g) for g in gs] for gs in grads], KW["lr"], KW["betas"], KW["eps"],
                                         0.01, [0.9] * 4, max_grad_norm=20.0, decoupled=decoupled, skip_nonfinite=True)
    for i, p in enumerate(a):
        if p.numel() and grads[1][i] is not None:
            ep, ee = _rel(p, want_p[i]), _rel(opt.state[p]["ema"], want_e[i])
            assert ep <= 2e-6 and ee <= 2e-6 + 3 * 2.0 ** -22, (i, ep, ee)
            assert int(opt.state[p]["step"]) == (3 if i == 1 else 4)


def test_two_runs_give_the_same_bits(data):
    dev = _dev()
    runs = []
    for _ in range(2):
        ps = _params(data, dev)
        opt = _opt(ps, True, 20.0, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True)
        for gs in data["grads"]:
            _set_grads(ps, gs, dev)
            opt.step()
        runs.append(_bits(opt, ps))
    assert _same(*runs)


def test_steps_with_ema_and_guard_do_not_synchronise_the_host(data):
    dev = _dev()
    ps = _params(data, dev)
    fresh = [[None if g is None else g.to(dev) for g in gs] for gs in data["grads"][:3]]
    opt = _opt(ps, True, None, ema_decay=0.9, skip_nonfinite=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for gs in fresh:
            for p, g in zip(ps, gs):
                p.grad = g
            opt.step()
        skipped = opt.step_skipped                   # a device expression
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert skipped.is_cuda and bool(skipped) is False and float(opt.clip_coef) == 1.0


def test_swap_multi_exchanges_and_restores(data):
    from mas_hip import ops
    dev = _dev()
    ps = _params(data, dev)
    opt = _opt(ps, False, None, ema_decay=0.5)
    for gs in data["grads"][:2]:
        _set_grads(ps, gs, dev)
        opt.step()
    st = opt.state[ps[3]]
    st["ema"] = torch.empty(4097, device=dev)[1:].copy_(st["ema"])                   # one pair with an unaligned side on a full block
    live, ema = [p.detach().clone() for p in ps], [opt.state[p]["ema"].clone() if "ema" in opt.state[p] else None for p in ps]
    ptrs = [p.data_ptr() for p in ps]
    with opt.swap_ema():
        assert ops.last_kernel() == "swap_multi"
        for p, w, e in zip(ps, live, ema):
            assert torch.equal(p.detach(), w if e is None else e) and (e is None or torch.equal(opt.state[p]["ema"], w))
        with pytest.raises(RuntimeError, match="already active"):
            with opt.swap_ema():
                pass
        with pytest.raises(RuntimeError, match="inside swap_ema"):
            opt.step()
    for p, w, e in zip(ps, live, ema):
        assert torch.equal(p.detach(), w) and (e is None or torch.equal(opt.state[p]["ema"], e))
    assert [p.data_ptr() for p in ps] == ptrs


def _swap_checks(model, opt, fresh_model, forward):
    """`forward(model)` in eval mode: live, under swap_ema(), from a second model loaded with ema_state_dict(), and live again"""
    from mas_hip import ops
    model.eval()
    with torch.no_grad():
        y_live = forward(model).clone()              # the caches now hold images of the live weights
        with opt.swap_ema():
            assert ops.last_kernel() == "swap_multi"
            y_ema = forward(model).clone()
        y_after = forward(model).clone()
        other = fresh_model()
        other.load_state_dict(opt.ema_state_dict(model), strict=True)
        other = other.to(y_live.device).eval()
        y_other = forward(other).clone()
    assert torch.isfinite(y_ema.float()).all()
    assert torch.equal(y_ema, y_other)               # the kernels saw the averaged weights
    assert not torch.equal(y_ema, y_live)
    assert torch.equal(y_after, y_live)              # and the live ones again afterwards
    return y_live, y_ema


def test_swap_ema_through_the_vq_model():
    from mas_hip import ops
    from mas_hip.optim import Adam
    from models import VQBASE
    from oracle import vq_oracle as O
    dev = _dev()
    cfg = dict(ddconfig=dict(z_channels=32, in_channels=3, out_channels=3, channels=[32, 32, 64], num_res_blocks=1,
                             resolution=16, attn_resolutions=[8], dropout=0.0), n_embed=64, embed_dim=32, init_steps=10, reservoir_size=100)

    def fresh():
        m = VQBASE(**cfg)
        m.quantize.q_counter = m.quantize.q_re_end   # steady state: VQ active, no k-means
        return m
    model = fresh()
    model.load_state_dict(O.synth_state_dict(cfg["ddconfig"], cfg["n_embed"], cfg["embed_dim"], seed=0), strict=True)
    model = model.to(dev).train()
    x = O.synth_image_batch(2, 3, 16, seed=0).to(dev)
    opt = Adam(model.parameters(), lr=1e-3, ema_decay=0.5)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        rec, q = model(x)
        ((x - rec).abs().mean() + q).backward()
        opt.step()
    assert ops.last_kernel() == "adam_multi_ema"
    _swap_checks(model, opt, fresh, lambda m: m(x)[0])


def test_swap_ema_through_the_transformer():
    from mas_hip.optim import AdamW
    from models.transformer import MakeAScene
    from oracle import transformer_oracle as TO
    dev = _dev()
    cfg = dict(num_layers=2, hidden_dim=64, num_attn_heads=4, image_vocab_size=128, seg_vocab_size=40, text_vocab_size=58,
               image_tokens_per_dim=4, seg_tokens_per_dim=2, text_length=8)
    model = MakeAScene(**cfg)
    model.load_state_dict(TO.synth_transformer_state_dict(cfg, seed=7), strict=True)
    model = model.to(dev).train()
    text, seg, img = (t.to(dev) for t in TO.synth_tokens(cfg, batch=2, seed=7))
    opt = AdamW(model.parameters(), lr=1e-3, max_grad_norm=1.0, ema_decay=0.5, skip_nonfinite=True)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model.token_loss(text, seg, img)
        loss.backward()
        opt.step()
    assert bool(opt.step_skipped) is False

    def forward(m):
        with torch.autocast("cuda", dtype=torch.bfloat16):          # the bf16 Linear shadows
            return m(text, seg, img)
    _swap_checks(model, opt, lambda: MakeAScene(**cfg), forward)
