"""``GraphedGanStep`` with the face term inside the replayed VQ-IMG step: the tiny ``VQBASE`` of test_gpu_graph_vq_img.py (channels
[32, 32, 64], 64 x 64, B = 2, ``init_steps=2``, ``perceptual=None``) with a synthetic-weight ``FaceLoss`` on the loss, per-call face boxes
through the step's ``FaceTable``, against a twin trained eagerly through the same table path (HIP tail on, weight-gradient side stream
off).  The boxes cycle through one face, none, four faces over both images, none, seven faces (no rec row survives); nine calls cross the
three codebook phases (calls 1-2, 3-5, 6-9) and the discriminator's gate (``disc_start=6``: open from call 7).  Both paths issue the same
kernels on the same data: everything agrees bit for bit."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "make-a-scene_amd"), ROOT):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import face_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
CFG = dict(ddconfig=dict(z_channels=32, in_channels=3, out_channels=3, channels=[32, 32, 64], num_res_blocks=1, resolution=64,
                         attn_resolutions=[16], dropout=0.0), n_embed=48, embed_dim=32, init_steps=2, reservoir_size=70)
KEYS = ("exp_avg", "exp_avg_sq")
CALLS, DISC_START = 9, 6
OUT = ("loss", "d_loss", "nll_loss", "g_loss", "d_weight")
ONE = [[[8, 6, 40, 46]], []]
FOUR = [[[5, 5, 35, 40], [15, 10, 45, 45]], [[0, 0, 30, 20], [20, 15, 56, 48]]]
SEVEN = [[[0, 0, 20, 20], [5, 5, 30, 25], [10, 2, 38, 36], [2, 3, 22, 33]], [[12, 0, 40, 24], [0, 10, 40, 30], [-6, 30, 20, 60]]]
CYCLE = (ONE, None, FOUR, None, SEVEN)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("face") / "face_synth.pt"
    torch.save(R.synth_face_state_dict(0), p)
    return str(p)


@pytest.fixture
def face(ckpt, monkeypatch):
    """-> a function that builds one synthetic-weight FaceLoss per call (evaluation mode, on the host)"""
    monkeypatch.setenv("MAS_FACE_CKPT", ckpt)
    from losses.face_loss import FaceLoss
    return FaceLoss


def _model(dev, device_reservoir=True, loss_kw=None, **over):
    from losses.loss_img import VQLPIPSWithDiscriminator
    from models import VQBASE
    from oracle.vq_oracle import synth_state_dict
    cfg = dict(CFG, **over)
    m = VQBASE(**cfg)
    m.load_state_dict(synth_state_dict(cfg["ddconfig"], cfg["n_embed"], cfg["embed_dim"], seed=3), strict=True)
    m = m.to(dev).train()
    if device_reservoir:
        m.quantize.enable_device_reservoir(seed=77)
    crit = VQLPIPSWithDiscriminator(**dict(dict(disc_start=DISC_START, perceptual_loss=None, face_loss=None), **(loss_kw or {})))
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


def _eager_call(model, crit, gopt, dopt, counter, images, closing, table, boxes):
    """one call of the eager twin, in the order of the reference's loop; the boxes go through the same table, and a call without faces
    leaves the term out, as the step's variant without faces does"""
    from losses.loss_img import hip_tail
    from mas_hip import ops
    disc = list(crit.discriminator.parameters())
    faces = table.write(boxes, images.shape[0]) > 0
    with ops.wgrad_stream_off(), hip_tail(True):
        rec, q = model(images)
        d_loss = crit(1, counter, images, rec)
        d_loss.backward()
        for p in disc:
            p.requires_grad_(False)
        crit.advance_global_step = True
        try:
            loss, (nll, _, _) = crit(0, counter, images, rec, q, bbox_face=table if faces else None, last_layer=model.decoder.model[-1])
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
def test_twin_run_bit_for_bit_with_per_call_faces(face, accumulate):
    dev = _dev()
    from mas_hip import face as FH
    from mas_hip import graphs
    batches = _batches(dev, CALLS)
    boxes = [CYCLE[k % len(CYCLE)] for k in range(CALLS)]
    torch.manual_seed(11)
    mt, ct = _model(dev, loss_kw=dict(face_loss=face()))
    gt, dt = _optimizers(mt, ct)
    gt.init_state()                                             # (the step creates every moment at construction: the twin has them from
    dt.init_state()                                             # call 1 too, so that the state can be compared before the first step)
    counter = torch.zeros((), dtype=torch.int64, device=dev)
    table = FH.FaceTable(dev)
    eager, after = [], []
    for k, x in enumerate(batches):
        eager.append(_eager_call(mt, ct, gt, dt, counter, x, (k + 1) % accumulate == 0, table, boxes[k]))
        after.append(_bits(mt, ct, gt, dt, counter))
    torch.manual_seed(11)
    mg, cg = _model(dev, loss_kw=dict(face_loss=face()))
    gg, dg = _optimizers(mg, cg)
    step = graphs.GraphedGanStep(mg, cg, gg, dg, batches[0], accumulate=accumulate, global_step=0, example_bbox_face=boxes[0])   # call 1
    assert step.captures == 0 and step.calls == 1 and step.face_table.n_faces == 1
    assert _same(_bits(mg, cg, gg, dg, step.global_step), after[0])
    per_phase = 2 if accumulate == 1 else 4                     # (closing, faces) graphs
    seen = []
    for k, x in enumerate(batches[1:], start=2):
        out = step(x, boxes[k - 1])
        seen.append(step.captures)
        for name, got, want in zip(OUT, out, eager[k - 1]):
            assert got.dim() == 0 and torch.equal(got, want), (k, name, float(got), float(want))
        assert _same(_bits(mg, cg, gg, dg, step.global_step), after[k - 1]), k            # parameters, both Adams' state, BatchNorm buffers,
        assert (float(out.d_loss) == 0.0) == (k < 7), (k, float(out.d_loss))              # the reservoir and the counter after EVERY call
    # calls 2 | 3-5 | 6-9: one set of graphs at the first call of each phase, none when faces come and go inside it
    assert seen == [per_phase] + [2 * per_phase] * 3 + [3 * per_phase] * 4, seen
    assert set(step._graphs) == {(c, f) for c in ((True,) if accumulate == 1 else (False, True)) for f in (False, True)}
    assert int(step.global_step) == int(counter) == CALLS and mg.quantize.q_counter == mt.quantize.q_counter == CALLS
    assert all(p.requires_grad for p in cg.discriminator.parameters()) and bool(torch.isfinite(out.loss))
    assert all(not p.requires_grad and p.grad is None for p in cg.face_loss.parameters())


def test_faces_come_and_go_without_a_capture_or_a_host_read(face):
    """far from a re-initialisation (its k-means reads a scalar on the host by design); ``accumulate=2``: four graphs, taken at call 2"""
    dev = _dev()
    from mas_hip import graphs
    batches = _batches(dev, 6)
    m, crit = _model(dev, loss_kw=dict(face_loss=face()), init_steps=1000)
    m.quantize.q_counter = 1500
    gopt, dopt = _optimizers(m, crit)
    step = graphs.GraphedGanStep(m, crit, gopt, dopt, batches[0], accumulate=2, global_step=DISC_START)
    assert step.captures == 0
    step(batches[1], ONE)                                         # the captures: micro-step and closing step, without and with the term
    assert step.captures == 4
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for x, b in zip(batches[2:], (None, FOUR, [[], []], SEVEN)):
            out = step(x, b)
            assert step.captures == 4
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(t)) for t in out) and step.calls == 6 and step.face_table.n_faces == 7
    assert float(out.d_loss) != 0.0 and int(step.global_step) == DISC_START + 6
    with pytest.raises(ValueError, match="no area"):
        step(batches[0], [[[5, 5, 5, 9]], []])
    assert step.calls == 6 and int(step.global_step) == DISC_START + 6 and m.quantize.q_counter == 1506      # refused before the tick


def test_the_face_term_is_in_the_graph(face):
    """identical weights and images: one closing call with a face moves the generator elsewhere than one without; and the call without
    faces replays what a step built with face_loss=None replays"""
    dev = _dev()
    from mas_hip import graphs
    x0, x1 = _batches(dev, 2)
    params = []
    for kw, boxes in ((dict(face_loss=face()), ONE), (dict(face_loss=face()), None), (None, None)):
        torch.manual_seed(5)
        m, crit = _model(dev, loss_kw=kw, init_steps=1000)
        m.quantize.q_counter = 1500
        gopt, dopt = _optimizers(m, crit)
        step = graphs.GraphedGanStep(m, crit, gopt, dopt, x0, global_step=DISC_START)
        out = step(x1, boxes)
        assert step.captures == (2 if kw else 1) and bool(torch.isfinite(out.loss))
        params.append([p.detach().clone() for p in m.parameters()])
    assert any(not torch.equal(a, b) for a, b in zip(params[0], params[1]))
    assert all(torch.equal(a, b) for a, b in zip(params[1], params[2]))


def test_refusals(face):
    dev = _dev()
    from mas_hip import graphs
    x = _batches(dev, 1)[0]
    term = lambda images, rec, boxes: (images - rec).square().mean()
    for name, value in (("face_loss", term), ("face_loss", face().train()), ("object_loss", term)):
        m, crit = _model(dev, loss_kw={name: value})
        with pytest.raises(NotImplementedError, match=f"{name}.*host box lists"):
            graphs.GraphedGanStep(m, crit, *_optimizers(m, crit), x)
        assert m.quantize.q_counter == 0
    m, crit = _model(dev, loss_kw=dict(face_loss=face(), object_loss=term))             # the face term alone does not open the door
    with pytest.raises(NotImplementedError, match="object_loss.*host box lists"):
        graphs.GraphedGanStep(m, crit, *_optimizers(m, crit), x)
