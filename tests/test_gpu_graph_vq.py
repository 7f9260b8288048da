"""``GraphedTrainStep`` over the VQ-SEG training step: a tiny ``VQBASE`` (the channel widths of the ``vq_seg_tiny`` fixture, 159 label
channels, a 32 x 32 label-plane input, B = 2, ``init_steps=2``: 8 x 8 latents, a reservoir of 70 rows that call 6 takes past its
capacity) with ``VQVAEWithBCELoss`` over ``SegLabels``, captured -- one graph per codebook phase, or a micro-step and a closing step per
phase under ``accumulate=3`` -- against a twin trained eagerly with the device reservoir and the same ``device_step=True`` optimizer.
Twelve calls cross the three phases (calls 1-2 no collect, 3-5 collect, 6-12 collect + lookup) and seven re-initialisations.  Both
paths issue the same kernels on the same data: losses, parameters, moments, reservoir and counters agree bit for bit."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "make-a-scene_amd"), ROOT):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import seg_labels_ref as LR  # noqa: E402
import seg_data  # noqa: E402

pytestmark = pytest.mark.gpu
CFG = dict(ddconfig=dict(z_channels=32, in_channels=159, out_channels=159, channels=[32, 32, 64, 64], num_res_blocks=1, resolution=32,
                         attn_resolutions=[8], dropout=0.0), n_embed=48, embed_dim=32, init_steps=2, reservoir_size=70)
KEYS = ("exp_avg", "exp_avg_sq")
CALLS = 12


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(dev, device_reservoir=True, **over):
    from losses.loss_seg import VQVAEWithBCELoss
    from models import VQBASE
    from oracle.vq_oracle import synth_state_dict
    cfg = dict(CFG, **over)
    m = VQBASE(**cfg)
    m.load_state_dict(synth_state_dict(cfg["ddconfig"], cfg["n_embed"], cfg["embed_dim"], seed=3), strict=True)
    m = m.to(dev).train()
    if device_reservoir:
        m.quantize.enable_device_reservoir(seed=77)
    return m, VQVAEWithBCELoss().to(dev)


_planes = {}


def _batches(dev, n):
    """n batches of uint8 label planes [2, 4, 32, 32], made once"""
    for k in range(n):
        if k not in _planes:
            _planes[k] = torch.stack([seg_data.planes_from_arrays(*LR.sample_arrays(32, 32, seed=300 + 2 * k + s)) for s in range(2)])
    return [_planes[k].to(dev) for k in range(n)]


def _loss_fn(model, crit):
    from mas_hip.seglabels import SegLabels

    def fn(planes):
        lab = SegLabels(planes)
        rec, qloss = model(lab)
        return crit(qloss, lab, rec)
    return fn


def _eager_call(fn, opt, planes, closing):
    """one call of the eager twin: backward adds into the gradients, the optimizer steps on a closing call"""
    from mas_hip import ops
    with ops.wgrad_stream_off():
        loss = fn(planes)
        loss.backward()
        if closing:
            opt.step()
            opt.zero_grad(set_to_none=True)
    return loss.detach().clone()


def _bits(model, opt):
    ps = list(model.parameters())
    dev = model.quantize._dev
    return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in KEYS if k in opt.state[p]] + \
           [opt.state[p]["step"].clone() for p in ps if "step" in opt.state[p]] + [dev["buf"].clone(), dev["state"].clone()]


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _twin_run(dev, accumulate):
    from mas_hip import graphs
    from mas_hip.optim import AdamW
    batches = _batches(dev, CALLS)
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01, device_step=True)
    # the runs one after the other, each from the same seeds (k-means draws its initial points from torch's generator)
    torch.manual_seed(11)
    mt, ct = _model(dev)
    ot, ft = AdamW(mt.parameters(), **kw), _loss_fn(mt, ct)
    eager = [_eager_call(ft, ot, planes, (k + 1) % accumulate == 0) for k, planes in enumerate(batches)]
    torch.manual_seed(11)
    mg, cg = _model(dev)
    og = AdamW(mg.parameters(), **kw)
    step = graphs.GraphedTrainStep(_loss_fn(mg, cg), og, batches[0], modules=[mg], accumulate=accumulate)     # call 1 is the warm-up call
    assert step.captures == 0 and step.calls == 1 and step.codebooks == [mg.quantize] and mg.quantize.q_counter == 1
    graphed = []
    for k, planes in enumerate(batches[1:], start=2):
        graphed.append(step(planes).clone())
        if k % accumulate == 0 and accumulate > 1:            # after a closing call every gradient is zero or None
            assert all(p.grad is None or not bool(p.grad.any()) for p in mg.parameters()), k
    return step, (mg, og), (mt, ot), eager, graphed


@pytest.mark.parametrize("accumulate", [1, 3])
def test_twin_run_bit_for_bit_across_phases_and_reinitialisations(accumulate):
    dev = _dev()
    step, (mg, og), (mt, ot), eager, graphed = _twin_run(dev, accumulate)
    for k, (lg, lt) in enumerate(zip(graphed, eager[1:]), start=2):
        assert lg.dim() == 0 and torch.equal(lg, lt), (k, float(lg), float(lt))
    assert _same(_bits(mg, og), _bits(mt, ot))
    assert step.captures == (3 if accumulate == 1 else 6) and step.calls == CALLS
    qg, qt = mg.quantize, mt.quantize
    assert qg.q_counter == qt.q_counter == CALLS and qg._dev["c"] == qt._dev["c"] == 70 and qg._dev["state"].tolist() == [70, CALLS - 2]
    assert not torch.equal(qg.embedding.weight, torch.zeros_like(qg.embedding.weight)) and bool(torch.isfinite(graphed[-1]))
    steps = {int(og.state[p]["step"]) for p in mg.parameters() if p is not qg.embedding.weight}
    assert steps == {CALLS // accumulate}
    # the embedding has had a gradient since the lookup began (call 6) and none before: AdamW never touched it until then
    assert int(og.state[qg.embedding.weight]["step"]) == int(ot.state[qt.embedding.weight]["step"]) == len(
        [k for k in range(1, CALLS + 1) if k % accumulate == 0 and k >= 6])


def test_replays_without_host_synchronisation_and_refusals():
    dev = _dev()
    from mas_hip import graphs
    from mas_hip.optim import AdamW
    batches = _batches(dev, 6)
    # far from a re-initialisation (its k-means reads a scalar on the host by design): init_steps = 1000, and the counter in the middle
    # of the collect phase
    m, crit = _model(dev, init_steps=1000)
    m.quantize.q_counter = 1500
    opt = AdamW(m.parameters(), lr=1e-3, max_grad_norm=1.0, device_step=True)
    step = graphs.GraphedTrainStep(_loss_fn(m, crit), opt, batches[0], modules=[m], accumulate=2)
    step(batches[1])                                          # the captures: a micro-step and a closing step
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for planes in batches[2:]:
            loss = step(planes)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss)) and step.captures == 2 and m.quantize.q_counter == 1506
    assert m.quantize._dev["state"].tolist() == [70, 6] and int(opt.state[next(m.parameters())]["step"]) == 3
    # a Codebook that keeps its reservoir on the host cannot be captured
    m2, crit2 = _model(dev, device_reservoir=False)
    with pytest.raises(RuntimeError, match="enable_device_reservoir"):
        graphs.GraphedTrainStep(_loss_fn(m2, crit2), AdamW(m2.parameters(), lr=1e-3, device_step=True), batches[0], modules=[m2])
    with pytest.raises(RuntimeError, match="enable_device_reservoir"):
        graphs.GraphedTrainStep(_loss_fn(m2, crit2), AdamW(m2.parameters(), lr=1e-3, device_step=True), batches[0], codebooks=[m2.quantize])
    assert m2.quantize.q_counter == 0


def test_accumulate_one_without_a_codebook_is_the_unchanged_path():
    """a model that holds no Codebook (the decoder half, fed latents), ``accumulate=1``: captured at construction, one capture, and the
    replays equal the eager twin bit for bit, as tests/test_gpu_graph_step.py holds the stage-2 step to"""
    dev = _dev()
    from mas_hip import graphs, ops
    from mas_hip.optim import AdamW
    from models.modules import Decoder
    torch.manual_seed(5)
    dg = Decoder(**CFG["ddconfig"]).to(dev).train()
    dt = Decoder(**CFG["ddconfig"]).to(dev).train()
    dt.load_state_dict(dg.state_dict())
    og, ot = (AdamW(d.parameters(), lr=1e-3, device_step=True) for d in (dg, dt))
    zs = [torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(70 + k)).to(dev) for k in range(4)]
    fn = lambda d: (lambda z: d(z).float().square().mean())
    step = graphs.GraphedTrainStep(fn(dg), og, zs[0], modules=[dg], accumulate=1)
    assert step.captures == 1 and step.codebooks == [] and step.graph is not None
    for k, z in enumerate(zs):
        ot.zero_grad(set_to_none=True)
        with ops.wgrad_stream_off():
            lt = fn(dt)(z)
            lt.backward()
            ot.step()
        if k:
            assert torch.equal(step(z), lt.detach()), k
    assert step.captures == 1 and all(torch.equal(a, b) for a, b in zip(dg.parameters(), dt.parameters()))
    assert all(torch.equal(og.state[a]["exp_avg"], ot.state[b]["exp_avg"]) for a, b in zip(dg.parameters(), dt.parameters()))
