"""``GraphedGanStep`` with the object term inside the replayed VQ-IMG step: the tiny ``VQBASE`` of test_gpu_graph_vq_img_face.py (channels
[32, 32, 64], 64 x 64, B = 2, ``init_steps=2``, ``perceptual=None``) with a synthetic-weight ``ObjectLoss`` on the loss, per-call object
boxes through the step's ``ObjectAtlas`` (one 96 x 160 canvas, eight cells), against a twin trained eagerly through the static node on
its own atlas (HIP tail on, weight-gradient side stream off).  Both paths issue the same kernels on the same data: everything agrees
bit for bit, after every call.  A call whose boxes do not fit the atlas runs eagerly on the list path, in the step and in the twin."""
import os
import sys
import warnings

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
CALLS, DISC_START = 8, 5
OUT = ("loss", "d_loss", "nll_loss", "g_loss", "d_weight")
ATLAS = dict(height=96, width=160, canvases=1, max_cells=8)
SOME = [[[4, 6, 40, 50], [10, 2, 30, 32]], [[20, 20, 48, 50]]]
LOPSIDED = [[], [[0, 0, 30, 30], [10, 20, 40, 60], [33, 3, 60, 28]]]
UNUSED = [[[0, 0, 10, 40]], [[5, 5, 60, 12]]]                       # both boxes under 16 px on a side: no used crop
OVERFLOW = [[[0, 0, 64, 64], [0, 0, 60, 60]], [[0, 0, 64, 60]]]     # three 80-px footprints: the canvas holds two
FACE_ONE = [[[8, 6, 40, 46]], []]
FACE_FOUR = [[[5, 5, 35, 40], [15, 10, 45, 45]], [[0, 0, 30, 20], [20, 15, 56, 48]]]
# (object boxes, face boxes) per call: none, some, some with faces as well, faces alone, ...
CYCLE = ((SOME, None), (None, None), (LOPSIDED, FACE_ONE), (None, FACE_FOUR), (UNUSED, None), (SOME, FACE_FOUR), (LOPSIDED, None), (None, None))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lpips_net():
    from losses.lpips import LPIPS
    from oracle.lpips_oracle import synth_lpips_state_dict
    m = LPIPS().eval()
    m.load_state_dict(synth_lpips_state_dict(3), strict=True)
    return m.to(_dev())


@pytest.fixture
def obj(lpips_net):
    """-> a function that builds one ObjectLoss on the shared synthetic LPIPS weights"""
    from losses.object_loss import ObjectLoss
    return lambda: ObjectLoss(lpips_net)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("face") / "face_synth.pt"
    torch.save(R.synth_face_state_dict(0), p)
    return str(p)


@pytest.fixture
def face(ckpt, monkeypatch):
    monkeypatch.setenv("MAS_FACE_CKPT", ckpt)
    from losses.face_loss import FaceLoss
    return FaceLoss


def _model(dev, loss_kw=None, q_counter=None, **over):
    from losses.loss_img import VQLPIPSWithDiscriminator
    from models import VQBASE
    from oracle.vq_oracle import synth_state_dict
    cfg = dict(CFG, **over)
    m = VQBASE(**cfg)
    m.load_state_dict(synth_state_dict(cfg["ddconfig"], cfg["n_embed"], cfg["embed_dim"], seed=3), strict=True)
    m = m.to(dev).train()
    m.quantize.enable_device_reservoir(seed=77)
    if q_counter is not None:
        m.quantize.q_counter = q_counter                      # far from a re-initialisation: one phase for the whole run
    crit = VQLPIPSWithDiscriminator(**dict(dict(disc_start=DISC_START, perceptual_loss=None, face_loss=None), **(loss_kw or {})))
    return m, crit.to(dev)


_images = {}


def _batches(dev, n):
    from oracle.vq_oracle import synth_image_batch
    for k in range(n):
        if k not in _images:
            _images[k] = synth_image_batch(2, 3, 64, seed=700 + k)
    return [_images[k].to(dev) for k in range(n)]


def _optimizers(model, crit, **kw):
    from mas_hip.optim import Adam
    kw = dict(dict(lr=1e-3, betas=(0.5, 0.9), device_step=True), **kw)
    return Adam(model.parameters(), **kw), Adam(crit.discriminator.parameters(), **kw)


def _eager_call(model, crit, gopt, dopt, counter, images, closing, atlas, obj_boxes, table=None, face_boxes=None):
    """one call of the eager twin, in the order of the reference's loop.  The object boxes go through the twin's own atlas and the
    static node; a call without a used crop leaves the term out, as the step's variant without it does; boxes that do not fit go to
    the list path."""
    from losses.loss_img import hip_tail
    from mas_hip import objects as O
    from mas_hip import ops
    disc = list(crit.discriminator.parameters())
    faces = table is not None and table.write(face_boxes, images.shape[0]) > 0
    try:
        bbox_obj = atlas if atlas.write(obj_boxes) > 0 else None
    except O.AtlasOverflow:
        bbox_obj = obj_boxes
    term = crit.object_loss
    with ops.wgrad_stream_off(), hip_tail(True):
        rec, q = model(images)
        d_loss = crit(1, counter, images, rec)
        d_loss.backward()
        for p in disc:
            p.requires_grad_(False)
        crit.advance_global_step = True
        if bbox_obj is None:
            crit.object_loss = None
        try:
            loss, (nll, _, _) = crit(0, counter, images, rec, q, bbox_obj=bbox_obj, bbox_face=table if faces else None,
                                     last_layer=model.decoder.model[-1])
            loss.backward()
        finally:
            crit.object_loss = term
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


def _twin(dev, loss_kw, batches, boxes, accumulate, with_faces=False, **over):
    """the eager run: -> (outputs per call, state after every call, the counter)"""
    from mas_hip import face as FH
    from mas_hip import objects as O
    torch.manual_seed(11)
    mt, ct = _model(dev, loss_kw=loss_kw(), **over)
    gt, dt = _optimizers(mt, ct)
    gt.init_state()
    dt.init_state()
    counter = torch.zeros((), dtype=torch.int64, device=dev)
    atlas, table = O.ObjectAtlas(dev, 2, **ATLAS), FH.FaceTable(dev) if with_faces else None
    eager, after = [], []
    for k, x in enumerate(batches):
        eager.append(_eager_call(mt, ct, gt, dt, counter, x, (k + 1) % accumulate == 0, atlas, boxes[k][0], table, boxes[k][1]))
        after.append(_bits(mt, ct, gt, dt, counter))
    return eager, after, counter


@pytest.mark.parametrize("accumulate", [1, 2])
def test_twin_run_bit_for_bit_with_per_call_objects_and_faces(obj, face, accumulate):
    dev = _dev()
    from mas_hip import graphs
    batches = _batches(dev, CALLS)
    boxes = [CYCLE[k % len(CYCLE)] for k in range(CALLS)]
    loss_kw = lambda: dict(object_loss=obj(), face_loss=face())
    eager, after, counter = _twin(dev, loss_kw, batches, boxes, accumulate, with_faces=True)
    torch.manual_seed(11)
    mg, cg = _model(dev, loss_kw=loss_kw())
    gg, dg = _optimizers(mg, cg)
    step = graphs.GraphedGanStep(mg, cg, gg, dg, batches[0], accumulate=accumulate, global_step=0, example_bbox_obj=boxes[0][0],
                                 example_bbox_face=boxes[0][1], object_atlas=ATLAS)                                         # call 1
    assert step.captures == 0 and step.calls == 1 and step.object_atlas.n_cells == 3 and step.eager_calls == 0
    assert (step.object_atlas.H, step.object_atlas.W, step.object_atlas.max_cells, step.object_atlas.n_images) == (96, 160, 8, 2)
    assert _same(_bits(mg, cg, gg, dg, step.global_step), after[0])
    per_phase = 4 * (1 if accumulate == 1 else 2)               # (closing, faces, objects) graphs
    seen = []
    for k, x in enumerate(batches[1:], start=2):
        out = step(x, boxes[k - 1][1], boxes[k - 1][0])
        seen.append(step.captures)
        for name, got, want in zip(OUT, out, eager[k - 1]):
            assert got.dim() == 0 and torch.equal(got, want), (k, name, float(got), float(want))
        assert _same(_bits(mg, cg, gg, dg, step.global_step), after[k - 1]), k            # parameters, both Adams' state, BatchNorm buffers,
        assert (float(out.d_loss) == 0.0) == (k < DISC_START + 1), (k, float(out.d_loss))  # the reservoir and the counter after EVERY call
    # calls 2 | 3-5 | 6-8: one set of graphs at the first call of each phase, none when boxes come and go inside it
    assert seen == [per_phase] + [2 * per_phase] * 3 + [3 * per_phase] * 3, seen
    assert set(step._graphs) == {(c, f, o) for c in ((True,) if accumulate == 1 else (False, True)) for f in (False, True) for o in (False, True)}
    assert int(step.global_step) == int(counter) == CALLS and step.eager_calls == 0
    assert cg.object_loss is not None and cg.object_loss.last_values.shape == (8,)
    assert all(p.requires_grad for p in cg.discriminator.parameters()) and bool(torch.isfinite(out.loss))


def test_objects_come_and_go_without_a_capture_or_a_host_read(obj):
    """far from a re-initialisation; ``accumulate=2``: micro-step and closing step, without and with the term -- four graphs at call 2"""
    dev = _dev()
    from mas_hip import graphs
    batches = _batches(dev, 6)
    m, crit = _model(dev, loss_kw=dict(object_loss=obj()), init_steps=1000)
    m.quantize.q_counter = 1500
    step = graphs.GraphedGanStep(m, crit, *_optimizers(m, crit), batches[0], accumulate=2, global_step=DISC_START, object_atlas=ATLAS)
    assert step.captures == 0 and step.face_table is None
    step(batches[1], None, SOME)
    assert step.captures == 4 and set(step._graphs) == {(c, False, o) for c in (False, True) for o in (False, True)}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for x, b in zip(batches[2:], (None, LOPSIDED, UNUSED, SOME)):
            out = step(x, bbox_obj=b)
            assert step.captures == 4
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(t)) for t in out) and step.calls == 6 and step.object_atlas.n_cells == 3 and step.eager_calls == 0
    assert float(out.d_loss) != 0.0 and int(step.global_step) == DISC_START + 6


def test_the_object_term_is_in_the_graph(obj):
    """identical weights and images: one closing call with boxes moves the generator elsewhere than one without; and the call without
    a used crop replays what a step built with object_loss=None replays"""
    dev = _dev()
    from mas_hip import graphs
    x0, x1 = _batches(dev, 2)
    params = []
    for kw, boxes in ((dict(object_loss=obj()), SOME), (dict(object_loss=obj()), UNUSED), (None, None)):
        torch.manual_seed(5)
        m, crit = _model(dev, loss_kw=kw, init_steps=1000)
        m.quantize.q_counter = 1500
        step = graphs.GraphedGanStep(m, crit, *_optimizers(m, crit), x0, global_step=DISC_START, object_atlas=ATLAS if kw else None)
        out = step(x1, bbox_obj=boxes)
        assert step.captures == (2 if kw else 1) and bool(torch.isfinite(out.loss))
        assert (step.object_atlas is not None) == bool(kw)
        params.append([p.detach().clone() for p in m.parameters()])
    assert any(not torch.equal(a, b) for a, b in zip(params[0], params[1]))
    assert all(torch.equal(a, b) for a, b in zip(params[1], params[2]))


@pytest.mark.parametrize("accumulate", [1, 2])
def test_an_overflowing_call_runs_eagerly_on_the_list_path(obj, accumulate):
    """call 3 of 5 does not fit the atlas: the step runs it eagerly (a micro-step under accumulate=2, a closing step under 1), the twin
    takes the list path for it, and the runs stay bit-equal; the graphs of call 2 serve calls 4 and 5"""
    dev = _dev()
    from mas_hip import graphs
    batches = _batches(dev, 5)
    boxes = [(b, None) for b in (SOME, LOPSIDED, OVERFLOW, None, SOME)]
    loss_kw = lambda: dict(object_loss=obj())
    eager, after, counter = _twin(dev, loss_kw, batches, boxes, accumulate, init_steps=1000, q_counter=1500)
    torch.manual_seed(11)
    mg, cg = _model(dev, loss_kw=loss_kw(), init_steps=1000, q_counter=1500)
    gg, dg = _optimizers(mg, cg)
    step = graphs.GraphedGanStep(mg, cg, gg, dg, batches[0], accumulate=accumulate, global_step=0, example_bbox_obj=SOME, object_atlas=ATLAS)
    graphs_per_phase = 2 * accumulate
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for k, x in enumerate(batches[1:], start=2):
            out = step(x, None, boxes[k - 1][0])
            for name, got, want in zip(OUT, out, eager[k - 1]):
                assert got.dim() == 0 and torch.equal(got, want), (k, name, float(got), float(want))
            assert _same(_bits(mg, cg, gg, dg, step.global_step), after[k - 1]), k
            assert step.eager_calls == (1 if k >= 3 else 0) and step.captures == graphs_per_phase, (k, step.captures)
    assert [w.category for w in caught if "ObjectAtlas" in str(w.message)] == [RuntimeWarning]
    assert step.calls == 5 and int(step.global_step) == int(counter) == 5 and step.object_atlas.n_cells == 3


def test_overflow_raises_before_the_tick_and_refusals(obj):
    dev = _dev()
    from mas_hip import graphs
    from mas_hip.objects import AtlasOverflow, ObjectAtlas
    x0, x1 = _batches(dev, 2)
    m, crit = _model(dev, loss_kw=dict(object_loss=obj()), init_steps=1000, q_counter=1500)
    atlas = ObjectAtlas(dev, 2, **ATLAS)
    step = graphs.GraphedGanStep(m, crit, *_optimizers(m, crit), x0, global_step=3, object_atlas=atlas, on_overflow="raise")
    assert step.object_atlas is atlas
    step(x1, bbox_obj=SOME)
    before = (step.calls, int(step.global_step), m.quantize.q_counter, step.captures, step.eager_calls)
    with pytest.raises(AtlasOverflow, match="1 of 3 used crops"):
        step(x0, bbox_obj=OVERFLOW)
    assert (step.calls, int(step.global_step), m.quantize.q_counter, step.captures, step.eager_calls) == before == (2, 5, 1502, 2, 0)
    assert atlas.n_cells == 3                                            # the table keeps the boxes of the last good call
    assert bool(torch.isfinite(step(x0, bbox_obj=LOPSIDED).loss)) and step.calls == 3
    # refused at construction: any object term that is not an ObjectLoss, a policy that does not exist, an atlas for a larger batch
    term = lambda images, rec, boxes: (images - rec).square().mean()
    m2, crit2 = _model(dev, loss_kw=dict(object_loss=term))
    with pytest.raises(NotImplementedError, match="object_loss.*host box lists"):
        graphs.GraphedGanStep(m2, crit2, *_optimizers(m2, crit2), x0)
    m3, crit3 = _model(dev, loss_kw=dict(object_loss=obj()))
    with pytest.raises(ValueError, match="on_overflow"):
        graphs.GraphedGanStep(m3, crit3, *_optimizers(m3, crit3), x0, on_overflow="skip")
    with pytest.raises(ValueError, match="object atlas"):
        graphs.GraphedGanStep(m3, crit3, *_optimizers(m3, crit3), x0, object_atlas=ObjectAtlas(dev, 4, **ATLAS))
    assert m2.quantize.q_counter == 0 and m3.quantize.q_counter == 0
