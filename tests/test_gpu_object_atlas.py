"""The object term at fixed capacity on the MI355X: ``mas_hip.objects.object_loss_static`` on an ``ObjectAtlas`` (csrc/object.hip's
``mas_obj_*_dev`` entry points) against the list path (``objects.object_loss``) on the same boxes.  Two images of 64 x 64, an atlas of one
96 x 160 canvas with eight cells, synthetic LPIPS weights.

Bounds: both sides run the same kernel bodies on the same data (only the canvas around the crops differs), so the fp32 comparison uses
the one-kernel fp32 yardsticks of tests/test_gpu_object_loss.py: values within 1e-5 relative, d rec within 1e-4 of its maximum.  The
bf16 case uses that file's bf16 bounds against the list path's own bf16 result: loss and d rec within 1.2x the deviation of the CPU
restatement under ``torch.autocast(bfloat16)`` from itself in fp32, d rec cosine >= 0.98.  Each case prints whether it was bit-equal."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import object_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W, MAX, SIZE = 96, 160, 8, 64

SOME = [[[4, 6, 40, 50], [10, 2, 30, 32]], [[20, 20, 48, 50]]]
# the largest crop the atlas takes: its footprint (the crop and its gutter) ends at the canvas's last tile row and column, the crop itself
# fills tile rows 0..4 and columns 0..8 up to their last pixel; the box leaves the image on all four sides
EDGE = [[[-40, -8, 104, 72]], []]
SIXTEENS = [[[4 * k, 3 * k, 4 * k + 16, 3 * k + 16] for k in range(4)], [[40 - 5 * k, 7 * k, 56 - 5 * k, 7 * k + 16] for k in range(4)]]   # max_cells crops of 16 x 16
OUTSIDE = [[[-10, 30, 20, 70]], [[50, -6, 80, 24]]]
OVERLAP = [[[5, 5, 45, 40], [20, 10, 60, 50]], []]
LOPSIDED = [[], [[0, 0, 30, 30], [10, 20, 40, 60], [33, 3, 60, 28]]]
GEOMETRIES = dict(some=SOME, edge=EDGE, sixteens=SIXTEENS, outside=OUTSIDE, overlap=OVERLAP, lopsided=LOPSIDED)


@pytest.fixture(scope="module")
def sd():
    from oracle.lpips_oracle import synth_lpips_state_dict
    return synth_lpips_state_dict(3)


@pytest.fixture(scope="module")
def net(sd):
    from losses.lpips import LPIPS
    m = LPIPS().eval()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.fixture(scope="module")
def images():
    img, rec = R.synth_images(2, SIZE, SIZE)
    return img.to(DEV), rec.to(DEV)


@pytest.fixture
def dtype_restored():
    from mas_hip import ops
    old = ops.compute_dtype()
    yield
    ops.set_compute_dtype(old)


def _dout():
    return (0.5 + torch.rand(1 + MAX, generator=torch.Generator().manual_seed(9))).to(DEV)


def _atlas():
    from mas_hip import objects as O
    return O.ObjectAtlas(DEV, 2, height=H, width=W, canvases=1, max_cells=MAX)


def _static(net, images, atlas, dtype):
    """-> (out [1 + MAX], d rec) for the weights ``_dout()`` on every output"""
    from mas_hip import objects as O
    img, rec = images
    r = rec.clone().requires_grad_(True)
    out = O.object_loss_static(net, img, r, atlas, dtype)
    (out * _dout()).sum().backward()
    return out.detach(), r.grad


def _list(net, images, boxes, dtype):
    from mas_hip import objects as O
    img, rec = images
    r = rec.clone().requires_grad_(True)
    out = O.object_loss(net, img, r, boxes, dtype)
    (out * _dout()[:out.numel()]).sum().backward()
    return out.detach(), r.grad


def _rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30))


def _check_fp32(name, got, want):
    (out, d), (lout, ld) = got, want
    n = lout.numel() - 1
    print(f"[object atlas] {name}: {n} crops, out bit-equal {torch.equal(out[:1 + n], lout)}, d rec bit-equal {torch.equal(d, ld)}, "
          f"out rel {_rel(out[:1 + n], lout):.3g}, d rec rel {_rel(d, ld):.3g}")
    assert out.shape == (1 + MAX,) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all())
    assert float((out[:1 + n] - lout).abs().div(lout.abs()).max()) <= 1e-5, (out, lout)
    assert float(out[1 + n:].abs().sum()) == 0.0
    assert float((d - ld).abs().max()) <= 1e-4 * float(ld.abs().max())
    assert float(ld.abs().max()) > 0


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_static_node_matches_the_list_path_fp32(net, images, name):
    boxes = GEOMETRIES[name]
    atlas = _atlas()
    n = atlas.write(boxes)
    assert n == sum(len(R.used(b)) for b in boxes)
    if name == "edge":
        (c, oy, ox, h, w, *_r), = atlas.last_plan.cells
        assert (oy, ox, h, w) == (0, 0, 80, 144) and oy + h + 16 == H and ox + w + 16 == W
    if name == "sixteens":
        assert n == MAX
    _check_fp32(name, _static(net, images, atlas, torch.float32), _list(net, images, boxes, torch.float32))


def test_static_node_bf16_within_autocast_deviation(sd, net, images):
    img, rec = (t.cpu() for t in images)
    grads, losses = [], []
    for autocast in (False, True):
        rr = rec.clone().requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            loss, _ = R.object_loss(sd, img, rr, SOME, net=R.lpips_fp32_head)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append(rr.grad)
    dev_loss, dev_drec = abs(losses[1] - losses[0]), float((grads[1] - grads[0]).abs().max())
    atlas = _atlas()
    atlas.write(SOME)
    from mas_hip import objects as O
    got, want = [], []
    for fn, what, res in ((O.object_loss_static, atlas, got), (O.object_loss, SOME, want)):
        r = images[1].clone().requires_grad_(True)
        out = fn(net, images[0], r, what, torch.bfloat16)
        out[0].backward()
        res += [float(out[0].detach()), r.grad]
    print(f"[object atlas] bf16: loss {got[0]} vs list {want[0]} (autocast deviation {dev_loss}), d rec max diff "
          f"{float((got[1] - want[1]).abs().max())} (autocast deviation {dev_drec}), bit-equal {torch.equal(got[1], want[1])}")
    assert abs(got[0] - want[0]) <= 1.2 * dev_loss + 1e-6 * abs(want[0])
    assert float((got[1] - want[1]).abs().max()) <= 1.2 * dev_drec
    a, b = got[1].flatten().double(), want[1].flatten().double()
    assert float(torch.dot(a, b) / (a.norm() * b.norm())) >= 0.98


def test_empty_table_and_slots_beyond_n_cells(net, images):
    atlas = _atlas()
    assert atlas.write(SIXTEENS) == MAX
    full, _ = _static(net, images, atlas, torch.float32)
    assert bool((full[1:] > 0).all())
    assert atlas.write(SOME) == 3
    out, d = _static(net, images, atlas, torch.float32)                  # after a fuller call: slots >= n_cells are 0
    assert bool((out[:4] > 0).all()) and float(out[4:].abs().sum()) == 0.0 and float(d.abs().max()) > 0
    for empty in ([[], []], None, [[[0, 0, 10, 40]], []]):
        assert atlas.write(empty) == 0
        out, d = _static(net, images, atlas, torch.float32)
        assert out.shape == (1 + MAX,) and torch.count_nonzero(out) == 0 and torch.count_nonzero(d) == 0
        assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(d).any())
        atlas.write(SOME)


def test_an_out_of_range_header_runs_nothing(net, images):
    """n_cells outside [0, max_cells]: every work-group returns; ``out`` keeps what it held"""
    from mas_hip import objects as O
    atlas = _atlas()
    atlas.write(SOME)
    partial = torch.zeros(atlas.n_partial, device=DEV)
    for bad in (-1, MAX + 1):
        atlas.dev[0] = bad
        out = torch.full((1 + MAX,), 7.0, device=DEV)
        O.check(O.lib().mas_obj_finalize_dev(O._p(partial), *atlas._args(), O._p(out), O._stream()), "obj_finalize_dev")
        assert bool((out == 7.0).all())
        y = torch.full((2, 64, H, W), -3.0, device=DEV).contiguous(memory_format=torch.channels_last)
        O.relu_fwd(y, atlas, 0)
        assert bool((y == -3.0).all())


def test_two_runs_are_bit_equal(net, images):
    atlas = _atlas()
    atlas.write(OVERLAP)
    a, b = _static(net, images, atlas, torch.bfloat16), _static(net, images, atlas, torch.bfloat16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0][0]) > 0


def test_the_node_captures_and_a_replay_follows_the_table(net, images, dtype_restored):
    from losses.object_loss import ObjectLoss
    from mas_hip import ops
    ops.set_compute_dtype(torch.bfloat16)
    img, rec = images
    term = ObjectLoss(net)
    atlas = _atlas()
    atlas.write(SOME)
    static_rec = rec.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), ops.wgrad_stream_off():
        for _ in range(2):                                              # the convolutions' choices and packed weights settle eagerly
            static_rec.grad = None
            term(img, static_rec, atlas).backward()
        static_rec.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            loss = term(img, static_rec, atlas)
            loss.backward()
        values, grad = term.last_values, static_rec.grad
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    replayed = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for boxes in (OVERLAP, [[], []], SIXTEENS, EDGE):
            atlas.write(boxes)
            graph.replay()
            replayed.append((loss.detach().clone(), values.clone(), grad.clone()))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for boxes, (l, v, g) in zip((OVERLAP, [[], []], SIXTEENS, EDGE), replayed):
        atlas.write(boxes)
        r = rec.clone().requires_grad_(True)
        want = term(img, r, atlas)
        want.backward()
        assert torch.equal(l, want.detach()) and torch.equal(v, term.last_values) and torch.equal(g, r.grad), boxes
        assert v.shape == (MAX,) and (float(l) > 0) == (atlas.n_cells > 0)
