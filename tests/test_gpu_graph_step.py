"""``mas_hip.graphs.GraphedTrainStep``: the stage-2 training step of a tiny ``MakeAScene`` (2 layers, hidden 64, 4 heads, vocabularies
96 / 40 / 58, 4x4 image, 2x2 seg, text 8; B = 2) captured into one graph, against a twin model trained eagerly with the same
``device_step=True`` optimizer on the same batches.  Both paths issue the same kernels on the same data, so losses, parameters, moments
and step counts agree bit for bit -- in fp32 and under bf16 autocast."""
import contextlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
sys.path.insert(0, ROOT)

CFG = dict(num_layers=2, hidden_dim=64, num_attn_heads=4, image_vocab_size=96, seg_vocab_size=40, text_vocab_size=58,
           image_tokens_per_dim=4, seg_tokens_per_dim=2, text_length=8)
MODES = [pytest.param(None, id="fp32"), pytest.param(torch.bfloat16, id="bf16-autocast")]
KEYS = ("exp_avg", "exp_avg_sq", "ema")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _mode(amp):
    from mas_hip import ops
    if amp is None:
        ops.set_compute_dtype(torch.float32)             # (restored by the suite's autouse fixture)


def _ctx(amp):
    return torch.autocast("cuda", dtype=amp) if amp is not None else contextlib.nullcontext()


def _model(dev, drop=0.0):
    from models.transformer import MakeAScene
    from oracle import transformer_oracle as TO
    m = MakeAScene(**CFG)
    m.load_state_dict(TO.synth_transformer_state_dict(CFG, seed=5), strict=True)
    m = m.to(dev).train()
    for layer in m.transformer.layers:
        layer.attn.attn_drop.p = layer.attn.out_drop.p = drop
    return m


def _batches(dev, n, first=0):
    from oracle import transformer_oracle as TO
    return [tuple(t.to(dev) for t in TO.synth_tokens(CFG, batch=2, seed=40 + first + i)) for i in range(n)]


def _eager_step(model, opt, batch, amp, scale=None):
    opt.zero_grad(set_to_none=True)
    with _ctx(amp):
        loss = model.token_loss(*batch)
        if scale is not None:
            loss = loss * scale
        loss.backward()
        opt.step()
    return loss.detach().clone()


def _bits(model, opt):
    ps = list(model.parameters())
    return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in KEYS if k in opt.state[p]] + \
           [opt.state[p]["step"].clone() for p in ps]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _pair(dev, amp, opt_kw, warmup=1, drop=0.0, extra=None):
    """(graphed model, its optimizer, the step, twin model, its optimizer) with the twin already past the warm-up steps"""
    from mas_hip import graphs, ops
    from mas_hip.optim import AdamW
    mg, mt = _model(dev, drop), _model(dev, drop)
    og, ot = AdamW(mg.parameters(), device_step=True, **opt_kw), AdamW(mt.parameters(), device_step=True, **opt_kw)
    first = _batches(dev, 1)[0] + (() if extra is None else (extra,))
    # fresh caches at capture time: invalidated, then filled by one eager forward -- a capture that leaves the refresh out would compute
    # every replay with the weights of the capture
    ops.invalidate_weight_cache()
    with torch.no_grad(), _ctx(amp):
        mg.token_loss(*first[:3])
    fn = (lambda t, s, i: mg.token_loss(t, s, i)) if extra is None else (lambda t, s, i, c: mg.token_loss(t, s, i) * c)
    step = graphs.GraphedTrainStep(fn, og, first, amp_dtype=amp, warmup=warmup, modules=[mg])
    for _ in range(warmup):                                   # construction trains: the twin takes the same steps
        _eager_step(mt, ot, first[:3], amp, extra)
    return mg, og, step, mt, ot


@pytest.mark.parametrize("amp", MODES)
def test_twin_run_bit_for_bit_and_fresh_weights_afterwards(amp):
    dev = _dev()
    _mode(amp)
    mg, og, step, mt, ot = _pair(dev, amp, dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01), warmup=2)
    assert step.captures == 1 and _same(_bits(mg, og), _bits(mt, ot))                  # the capture itself executed nothing
    for k, batch in enumerate(_batches(dev, 5, first=1)):
        lg = step(*batch).clone()
        lt = _eager_step(mt, ot, batch, amp)
        assert lg.dim() == 0 and torch.equal(lg, lt), (k, float(lg), float(lt))
    assert _same(_bits(mg, og), _bits(mt, ot))
    assert all(int(og.state[p]["step"]) == 7 for p in mg.parameters()) and step.captures == 1
    # an eager forward between replays sees the weights of now (stale bf16 shadows / images would give the loss of an earlier step)
    fresh = _batches(dev, 1, first=20)[0]
    with torch.no_grad(), _ctx(amp):
        assert torch.equal(mg.token_loss(*fresh), mt.token_loss(*fresh))
    lg = step(*fresh).clone()                                                           # and the graph goes on from there
    assert torch.equal(lg, _eager_step(mt, ot, fresh, amp)) and _same(_bits(mg, og), _bits(mt, ot))


@pytest.mark.parametrize("amp", MODES)
def test_settings_that_move(amp):
    dev = _dev()
    _mode(amp)
    mg, og, step, mt, ot = _pair(dev, amp, dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01))
    batches = _batches(dev, 5, first=1)
    for k, batch in enumerate(batches):
        if k == 2:                                            # a learning rate through param_groups: no new capture
            og.param_groups[0]["lr"] = ot.param_groups[0]["lr"] = 3e-4
        if k == 3:                                            # betas are launch arguments: recaptured lazily
            og.param_groups[0]["betas"] = ot.param_groups[0]["betas"] = (0.8, 0.9)
        if k == 4:                                            # the state reloaded in place: recaptured, nothing moved
            ptrs = [og.state[p]["exp_avg"].data_ptr() for p in mg.parameters()]
            og.load_state_dict(og.state_dict())
            assert ptrs == [og.state[p]["exp_avg"].data_ptr() for p in mg.parameters()]
        lg = step(*batch).clone()
        assert torch.equal(lg, _eager_step(mt, ot, batch, amp)), k
        assert _same(_bits(mg, og), _bits(mt, ot)), k
        assert step.captures == (1, 1, 1, 2, 3)[k], (k, step.captures)


@pytest.mark.parametrize("amp", MODES)
def test_guard_clip_and_ema_inside_the_graph(amp):
    dev = _dev()
    _mode(amp)
    one, inf = torch.ones((), device=dev), torch.full((), float("inf"), device=dev)
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01, max_grad_norm=0.01, ema_decay=0.9, ema_warmup=True, skip_nonfinite=True)
    mg, og, step, mt, ot = _pair(dev, amp, kw, extra=one)
    for k, batch in enumerate(_batches(dev, 5, first=1)):
        before = _bits(mg, og)[:-len(list(mg.parameters()))]                           # everything but the step counts
        c = inf if k == 3 else one
        lg = step(*batch, c).clone()
        lt = _eager_step(mt, ot, batch, amp, c)
        assert torch.equal(lg, lt) and _same(_bits(mg, og), _bits(mt, ot)), k
        assert bool(og.step_skipped) is (k == 3) and bool(ot.step_skipped) is (k == 3)
        if k == 3:
            assert not bool(torch.isfinite(lg)) and _same(_bits(mg, og)[:len(before)], before)
        else:
            assert float(og.clip_coef) < 1.0 and not _same(_bits(mg, og)[:len(before)], before)      # the clip is active
    assert all(int(og.state[p]["step"]) == 6 for p in mg.parameters()) and step.captures == 1
    eg, et = og.ema_state_dict(mg), ot.ema_state_dict(mt)
    assert list(eg) == list(et) and all(torch.equal(eg[n], et[n]) for n in eg)
    assert not torch.equal(eg["to_logits.1.weight"], mg.to_logits[1].weight)
    # the averaged weights in front of the kernels between replays, and back
    fresh = _batches(dev, 1, first=20)[0]
    with og.swap_ema(), ot.swap_ema(), torch.no_grad(), _ctx(amp):
        assert torch.equal(mg.token_loss(*fresh), mt.token_loss(*fresh))
    assert torch.equal(step(*fresh, one).clone(), _eager_step(mt, ot, fresh, amp, one)) and _same(_bits(mg, og), _bits(mt, ot))


@pytest.mark.parametrize("amp", MODES)
def test_dropout_draws_new_masks_at_every_replay(amp):
    dev = _dev()
    _mode(amp)
    from mas_hip import graphs
    from mas_hip.optim import Adam
    batch = _batches(dev, 1)[0]
    losses = {}
    for drop in (0.1, 0.0):
        m = _model(dev, drop)
        opt = Adam(m.parameters(), lr=0.0, device_step=True)
        step = graphs.GraphedTrainStep(lambda t, s, i, m=m: m.token_loss(t, s, i), opt, batch, amp_dtype=amp, modules=[m])
        losses[drop] = [step(*batch).clone(), step(*batch).clone()]
    assert not torch.equal(*losses[0.1])
    assert torch.equal(*losses[0.0])


def test_embedding_lookups_beyond_atens_fast_backward_are_captured_in_slices():
    """B = 256: 4096 image-token indices, above ``graphs.EMBEDDING_GRAD_CHUNK``.  ATen's backward for that many sorts the indices and hands a
    count to the host, which a capture cannot hold; ``graphs.embedding`` sums ATen's dense backward over slices instead.  The twin takes
    the same slices eagerly (``embedding_grad_in_chunks``): bit for bit again."""
    dev = _dev()
    from mas_hip import graphs
    from mas_hip.optim import AdamW
    from oracle import transformer_oracle as TO
    amp = torch.bfloat16
    batches = [tuple(t.to(dev) for t in TO.synth_tokens(CFG, batch=256, seed=60 + i)) for i in range(4)]
    assert batches[0][2].numel() == 4096 > graphs.EMBEDDING_GRAD_CHUNK
    mg, mt = _model(dev), _model(dev)
    og, ot = (AdamW(m.parameters(), lr=1e-3, max_grad_norm=1.0, device_step=True) for m in (mg, mt))
    step = graphs.GraphedTrainStep(lambda t, s, i: mg.token_loss(t, s, i), og, batches[0], amp_dtype=amp, modules=[mg])
    _eager_step(mt, ot, batches[0], amp)                                                # the warm-up step: eager on both sides
    for k, batch in enumerate(batches[1:]):
        lg = step(*batch).clone()
        with graphs.embedding_grad_in_chunks():
            lt = _eager_step(mt, ot, batch, amp)
        assert torch.equal(lg, lt) and _same(_bits(mg, og), _bits(mt, ot)), k
    assert bool(torch.isfinite(lg)) and step.captures == 1
    # and the slices' sum is the eager gradient up to the order of the additions: 4096 fp32 terms per row at most, 2^-24 relative each
    w, grad = mg.image_token_embedding.weight, {}
    for chunks in (False, True):
        w.grad = None
        with (graphs.embedding_grad_in_chunks() if chunks else contextlib.nullcontext()), _ctx(amp):
            mg.token_loss(*batches[0]).backward()
        grad[chunks] = w.grad.clone()
    assert float((grad[True] - grad[False]).abs().max()) <= 4096 * 2.0 ** -24 * float(grad[False].abs().max())


def test_no_host_synchronisation_and_refusals():
    dev = _dev()
    from mas_hip import graphs
    from mas_hip.optim import Adam, AdamW
    amp = torch.bfloat16
    mg, og, step, mt, ot = _pair(dev, amp, dict(lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True))
    batches = _batches(dev, 4, first=1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k, batch in enumerate(batches):
            if k == 2:
                og.param_groups[0]["lr"] = 5e-4
            loss = step(*batch)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss)) and step.captures == 1 and int(og.state[next(mg.parameters())]["step"]) == 5
    fn = lambda t, s, i: mg.token_loss(t, s, i)
    with pytest.raises(TypeError, match="device_step"):
        graphs.GraphedTrainStep(fn, AdamW(mg.parameters(), lr=1e-3), batches[0])
    with pytest.raises(TypeError, match="device_step"):
        graphs.GraphedTrainStep(fn, torch.optim.AdamW(mg.parameters(), lr=1e-3), batches[0])
    with pytest.raises(NotImplementedError, match="reducer"):
        graphs.GraphedTrainStep(fn, Adam(mg.parameters(), lr=1e-3, device_step=True), batches[0], reducer=object())
    with pytest.raises(ValueError, match="warmup"):
        graphs.GraphedTrainStep(fn, Adam(mg.parameters(), lr=1e-3, device_step=True), batches[0], warmup=0)
