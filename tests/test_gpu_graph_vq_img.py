"""``GraphedGanStep`` over the VQ-IMG training step: a tiny 3-channel ``VQBASE`` (channels [32, 32, 64], a 64 x 64 input, B = 2,
``init_steps=2``: 16 x 16 latents, a reservoir of 70 rows that call 6 takes past its capacity) with ``VQLPIPSWithDiscriminator`` and two
``device_step=True`` Adams, captured -- one graph per codebook phase, or a micro-step and a closing step per phase under ``accumulate=3``
-- against a twin trained eagerly: the same calls in the same order with the HIP tail on, the same device counter and the
weight-gradient side stream off.  Twelve calls cross the three phases (calls 1-2 no collect, 3-5 collect, 6-12 collect + lookup) and seven
re-initialisations; the discriminator's gate (``disc_start=6`` on a counter that starts at 0) opens at call 7.  Both paths issue the same
kernels on the same data: everything agrees bit for bit.

The codebook has 48 codes, not 64: the first re-initialisation (call 6) clusters the 60 rows that calls 3-5 collected at B = 2, and k-means
refuses more clusters than points."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "make-a-scene_amd"), ROOT):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

pytestmark = pytest.mark.gpu
CFG = dict(ddconfig=dict(z_channels=32, in_channels=3, out_channels=3, channels=[32, 32, 64], num_res_blocks=1, resolution=64,
                         attn_resolutions=[16], dropout=0.0), n_embed=48, embed_dim=32, init_steps=2, reservoir_size=70)
KEYS = ("exp_avg", "exp_avg_sq")
CALLS, DISC_START = 12, 6
OUT = ("loss", "d_loss", "nll_loss", "g_loss", "d_weight")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(dev, device_reservoir=True, perceptual=None, loss_kw=None, **over):
    from losses.loss_img import VQLPIPSWithDiscriminator
    from models import VQBASE
    from oracle.vq_oracle import synth_state_dict
    cfg = dict(CFG, **over)
    m = VQBASE(**cfg)
    m.load_state_dict(synth_state_dict(cfg["ddconfig"], cfg["n_embed"], cfg["embed_dim"], seed=3), strict=True)
    m = m.to(dev).train()
    if device_reservoir:
        m.quantize.enable_device_reservoir(seed=77)
    crit = VQLPIPSWithDiscriminator(**dict(dict(disc_start=DISC_START, perceptual_loss=perceptual, face_loss=None), **(loss_kw or {})))
    if perceptual == "lpips":
        from oracle.lpips_oracle import synth_lpips_state_dict
        crit.perceptual_loss.load_state_dict(synth_lpips_state_dict(3), strict=True)
    return m, crit.to(dev)


_images = {}


def _batches(dev, n):
    from oracle.vq_oracle import synth_image_batch
    for k in range(n):
        if k not in _images:
            _images[k] = synth_image_batch(2, 3, 64, seed=500 + k)
    return [_images[k].to(dev) for k in range(n)]


def _optimizers(model, crit, **kw):
    from mas_hip.optim import Adam
    kw = dict(dict(lr=1e-3, betas=(0.5, 0.9), device_step=True), **kw)
    return Adam(model.parameters(), **kw), Adam(crit.discriminator.parameters(), **kw)


def _eager_call(model, crit, gopt, dopt, counter, images, closing):
    """one call of the eager twin, in the order of the reference's loop: backward adds into the gradients, both optimizers step on a closing call"""
    from losses.loss_img import hip_tail
    from mas_hip import ops
    disc = list(crit.discriminator.parameters())
    with ops.wgrad_stream_off(), hip_tail(True):
        rec, q = model(images)
        d_loss = crit(1, counter, images, rec)
        d_loss.backward()
        for p in disc:
            p.requires_grad_(False)
        crit.advance_global_step = True
        try:
            loss, (nll, _, _) = crit(0, counter, images, rec, q, last_layer=model.decoder.model[-1])
            loss.backward()
        finally:
            crit.advance_global_step = False
            for p in disc:
                p.requires_grad_(True)
        if closing:
            dopt.step()
            dopt.zero_grad(set_to_none=True)
            gopt.step()
            gopt.zero_grad(set_to_none=True)
    return [t.detach().clone() for t in (loss, d_loss, nll, crit.last_terms["g_loss"], crit.last_terms["d_weight"])]


def _bits(model, crit, gopt, dopt, counter):
    out = []
    for mod, opt in ((model, gopt), (crit.discriminator, dopt)):
        ps = list(mod.parameters())
        out += [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in KEYS if k in opt.state[p]] + \
               [opt.state[p]["step"].clone() for p in ps if "step" in opt.state[p]]
    out += [b.clone() if b.is_floating_point() else b.float() for b in crit.discriminator.buffers()]      # BatchNorm running statistics
    dev = model.quantize._dev
    return out + [dev["buf"].clone(), dev["state"].clone(), counter.to(torch.int32)]


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("accumulate", [1, 3])
def test_twin_run_bit_for_bit_across_phases_gate_and_reinitialisations(accumulate):
    dev = _dev()
    from mas_hip import graphs
    batches = _batches(dev, CALLS)
    # the runs one after the other, each from the same seeds (k-means draws its initial points from torch's generator)
    torch.manual_seed(11)
    mt, ct = _model(dev)
    gt, dt = _optimizers(mt, ct)
    counter = torch.zeros((), dtype=torch.int64, device=dev)
    eager = [_eager_call(mt, ct, gt, dt, counter, x, (k + 1) % accumulate == 0) for k, x in enumerate(batches)]
    torch.manual_seed(11)
    mg, cg = _model(dev)
    gg, dg = _optimizers(mg, cg)
    step = graphs.GraphedGanStep(mg, cg, gg, dg, batches[0], accumulate=accumulate, global_step=0)           # call 1 is the warm-up call
    assert step.captures == 0 and step.calls == 1 and step.codebooks == [mg.quantize] and mg.quantize.q_counter == 1
    assert int(step.global_step) == 1 and not cg.advance_global_step
    for k, x in enumerate(batches[1:], start=2):
        out = step(x)
        assert out._fields == OUT
        for name, got, want in zip(OUT, out, eager[k - 1]):
            assert got.dim() == 0 and torch.equal(got, want), (k, name, float(got), float(want))
        assert (float(out.d_loss) == 0.0) == (k < 7), (k, float(out.d_loss))          # the gate opens at call 7 ...
        if k % accumulate == 0 and accumulate > 1:            # after a closing call every gradient is zero or None
            assert all(p.grad is None or not bool(p.grad.any()) for m_ in (mg, cg.discriminator) for p in m_.parameters()), k
    assert all(float(e[1]) == 0.0 for e in eager[:6]) and all(float(e[1]) != 0.0 for e in eager[6:])
    assert _same(_bits(mg, cg, gg, dg, step.global_step), _bits(mt, ct, gt, dt, counter))
    assert step.captures == (3 if accumulate == 1 else 6) and step.calls == CALLS                          # ... without a capture of its own
    assert int(step.global_step) == int(counter) == CALLS
    qg, qt = mg.quantize, mt.quantize
    assert qg.q_counter == qt.q_counter == CALLS and qg._dev["c"] == qt._dev["c"] == 70 and qg._dev["state"].tolist() == [70, CALLS - 2]
    assert all(p.requires_grad for p in cg.discriminator.parameters()) and bool(torch.isfinite(out.loss))
    bn = [m_ for m_ in cg.discriminator.modules() if isinstance(m_, torch.nn.BatchNorm2d)]
    assert bn and all(not torch.equal(m_.running_mean, torch.zeros_like(m_.running_mean)) for m_ in bn)
    for opt, mod in ((gg, mg), (dg, cg.discriminator)):
        steps = {int(opt.state[p]["step"]) for p in mod.parameters() if p is not qg.embedding.weight}
        assert steps == {CALLS // accumulate}, steps


def test_replays_without_host_synchronisation_lpips_inside():
    """far from a re-initialisation (its k-means reads a scalar on the host by design): init_steps = 1000, the counter in the middle of the
    collect phase; the perceptual term is LPIPS on its HIP path; ``accumulate=2``: a micro-step and a closing step"""
    dev = _dev()
    from losses.lpips import hip_path
    from mas_hip import graphs
    batches = _batches(dev, 6)
    m, crit = _model(dev, perceptual="lpips", init_steps=1000)
    m.quantize.q_counter = 1500
    gopt, dopt = _optimizers(m, crit, max_grad_norm=1.0)
    with hip_path(True):
        step = graphs.GraphedGanStep(m, crit, gopt, dopt, batches[0], accumulate=2, global_step=DISC_START - 3)
        step(batches[1])                                      # the captures
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for x in batches[2:]:
                out = step(x)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(t)) for t in out) and step.captures == 2 and m.quantize.q_counter == 1506
    assert float(out.d_loss) != 0.0 and float(out.d_weight) > 0.0 and int(step.global_step) == DISC_START + 3
    assert int(gopt.state[next(m.parameters())]["step"]) == 3 and int(dopt.state[next(crit.discriminator.parameters())]["step"]) == 3
    step.set_global_step(0)
    assert float(step(batches[0]).d_loss) == 0.0 and step.captures == 2 and int(step.global_step) == 1


def test_learning_rates_reach_the_replay_and_betas_recapture_once():
    dev = _dev()
    from mas_hip import graphs
    batches = _batches(dev, 4)
    m, crit = _model(dev, init_steps=1000)
    m.quantize.q_counter = 1500
    gopt, dopt = _optimizers(m, crit)
    step = graphs.GraphedGanStep(m, crit, gopt, dopt, batches[0], global_step=DISC_START)
    step(batches[1])
    assert step.captures == 1
    snap = lambda mod: [p.detach().clone() for p in mod.parameters()]
    moved = lambda mod, old: any(not torch.equal(a, b) for a, b in zip(mod.parameters(), old))
    for opt, mine, other in ((gopt, m, crit.discriminator), (dopt, crit.discriminator, m)):
        opt.param_groups[0]["lr"] = 0.0                       # a changed learning rate on either optimizer: the next replay has it
        a, b = snap(mine), snap(other)
        step(batches[2])
        assert not moved(mine, a) and moved(other, b) and step.captures == 1
        opt.param_groups[0]["lr"] = 1e-3
    a, b = snap(m), snap(crit.discriminator)
    step(batches[3])
    assert moved(m, a) and moved(crit.discriminator, b) and step.captures == 1
    dopt.param_groups[0]["betas"] = (0.6, 0.9)                # baked into the launch: one new capture
    step(batches[0])
    assert step.captures == 2
    step(batches[1])
    assert step.captures == 2 and step.calls == 7


def test_refusals():
    dev = _dev()
    from mas_hip import graphs
    from mas_hip.optim import Adam
    x = _batches(dev, 1)[0]
    m, crit = _model(dev)
    gopt, dopt = _optimizers(m, crit)
    host = lambda mod: Adam(mod.parameters(), lr=1e-3)
    with pytest.raises(TypeError, match="generator's optimizer.*device_step"):
        graphs.GraphedGanStep(m, crit, host(m), dopt, x)
    with pytest.raises(TypeError, match="discriminator's optimizer.*device_step"):
        graphs.GraphedGanStep(m, crit, gopt, host(crit.discriminator), x)
    with pytest.raises(TypeError, match="device_step"):
        graphs.GraphedGanStep(m, crit, torch.optim.Adam(m.parameters()), dopt, x)
    with pytest.raises(NotImplementedError, match="reducer"):
        graphs.GraphedGanStep(m, crit, gopt, dopt, x, reducer=object())
    m2, crit2 = _model(dev, device_reservoir=False)
    with pytest.raises(RuntimeError, match="enable_device_reservoir"):
        graphs.GraphedGanStep(m2, crit2, *_optimizers(m2, crit2), x)
    term = lambda images, rec, boxes: (images - rec).square().mean()
    for name in ("face_loss", "object_loss"):
        m3, crit3 = _model(dev, loss_kw={name: term})
        with pytest.raises(NotImplementedError, match=f"{name}.*host box lists"):
            graphs.GraphedGanStep(m3, crit3, *_optimizers(m3, crit3), x)
    assert m.quantize.q_counter == 0 and m2.quantize.q_counter == 0
