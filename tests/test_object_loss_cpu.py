"""The object-aware VQ-IMG term without a GPU: the atlas packer (mas_hip/objects.py), the CPU restatement (tests/helpers/object_ref.py)
against the golden the reference's own LPIPS wrote (tests/golden/object_tiny.npz), and the wiring into VQLPIPSWithDiscriminator."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import object_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "object_tiny.npz")


def _seeded_boxes(seed, n_images=32, per_image=4, size=256, lo=8, hi=160):
    rng = random.Random(seed)
    out = []
    for _ in range(n_images):
        boxes = []
        for _ in range(rng.randint(0, per_image)):
            h, w = rng.randint(lo, hi), rng.randint(lo, hi)
            y0, x0 = rng.randint(-h // 2, size - h // 2), rng.randint(-w // 2, size - w // 2)
            boxes.append([x0, y0, x0 + w, y0 + h])
        out.append(boxes)
    return out


def _check_plan(plan, bbox, n_images):
    from mas_hip import objects as O
    a = O.ALIGN
    assert plan.H % a == 0 and plan.W % a == 0
    want = [(b, box) for b, boxes in enumerate(bbox[:n_images]) for box in boxes if R.used([box])]
    assert len(plan.cells) == len(want)
    occ = np.zeros((plan.n_canvas, plan.H, plan.W), dtype=np.int32)
    for (n, oy, ox, h, w, b, top, left), (wb, box) in zip(plan.cells, want):
        assert (b, left, top, left + w, top + h) == (wb,) + tuple(box)          # (image, box) order, every used box placed
        assert oy % a == 0 and ox % a == 0 and 0 <= n < plan.n_canvas
        assert oy + h + O.GUTTER <= plan.H and ox + w + O.GUTTER <= plan.W     # room for the gutter inside the canvas
        cell = occ[n, oy:oy + h + O.GUTTER, ox:ox + w + O.GUTTER]
        assert not cell.any(), "a crop or its gutter overlaps another crop's"
        cell[...] = 1
    for b in range(len(plan.img_cell0) - 1):
        assert all(plan.cells[k][5] == b for k in range(plan.img_cell0[b], plan.img_cell0[b + 1]))


def test_filter_rule():
    from mas_hip import objects as O
    assert O.is_used([0, 0, 16, 16]) and O.is_used([-5, 3, 11, 40])
    assert not O.is_used([0, 0, 15, 40]) and not O.is_used([0, 0, 40, 15]) and not O.is_used([10, 10, 0, 40])
    cells, img0 = O.used_boxes(R.BOXES, 3)
    assert [b for b, _ in cells] == [0, 0, 0, 0, 2, 2] and img0 == [0, 4, 4, 6]
    # zip stops at the shorter of images and box lists
    assert O.used_boxes(R.BOXES, 1)[1] == [0, 4] and O.used_boxes(R.BOXES[:2], 3)[1] == [0, 4, 4]


def test_box_tensor_is_converted_like_the_collate():
    from mas_hip import objects as O
    t = torch.tensor([[[1.7, 2.2, 30.9, 40.0], [0, 0, 5, 5]], [[3, 4, 40, 50], [-2.5, 1, 20, 30]]])
    assert O.box_lists(t) == [[[1, 2, 30, 40], [0, 0, 5, 5]], [[3, 4, 40, 50], [-2, 1, 20, 30]]]
    with pytest.raises(ValueError):
        O.box_lists(torch.zeros(2, 4))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_packer_invariants_and_efficiency(seed):
    from mas_hip import objects as O
    bbox = _seeded_boxes(seed)
    plan = O.make_plan(bbox, 32)
    _check_plan(plan, bbox, 32)
    # the tile map names exactly the cell of every 16 x 16 tile a crop touches
    for k, (n, oy, ox, h, w, *_r) in enumerate(plan.cells):
        t = plan.tiles[n, oy // 16:(oy + h + 15) // 16, ox // 16:(ox + w + 15) // 16]
        assert (t == k).all()
    assert (plan.tiles >= 0).sum() == sum(((h + 15) // 16) * ((w + 15) // 16) for (_, _, _, h, w, *_r) in plan.cells)
    for l, c in enumerate(O.CHANNELS):
        per = [(h >> l) * (w >> l) for (_, _, _, h, w, *_r) in plan.cells]
        assert [plan.blk0[l][k + 1] - plan.blk0[l][k] for k in range(len(per))] == [-(-p // O.head_pixels(c)) for p in per]
    eff = plan.efficiency()
    print(f"seed {seed}: {plan.n_cells} crops on {plan.n_canvas} canvas(es) of {plan.H} x {plan.W}: area efficiency {eff:.2f}")
    assert 0.2 < eff <= 1.0


def test_packer_splits_into_canvases_and_widens_for_a_wide_crop():
    from mas_hip import objects as O
    bbox = [[[0, 0, 200, 200]] * 3 for _ in range(40)]
    plan = O.make_plan(bbox, 40, width=512, max_height=512)
    _check_plan(plan, bbox, 40)
    assert plan.n_canvas > 1 and plan.H <= 512
    bbox = [[[0, 0, 1500, 20], [0, 0, 20, 20]]]
    plan = O.make_plan(bbox, 1)
    _check_plan(plan, bbox, 1)
    assert plan.W >= 1516


def test_no_used_box_is_no_plan():
    from mas_hip import objects as O
    assert O.make_plan([[[0, 0, 10, 10]], []], 2) is None
    assert O.make_plan([], 4) is None


def test_plan_table_layout():
    from mas_hip import objects as O
    plan = O.make_plan(R.BOXES, 3)
    arr, offs = plan.table()
    assert arr.dtype == np.int32
    assert arr[offs[0]:offs[0] + 8].tolist() == list(plan.cells[0])
    assert arr[offs[1]:offs[2]].tolist() == plan.img_cell0
    assert arr[offs[2]:offs[3]].tolist() == [v for row in plan.blk0 for v in row]
    assert arr[offs[3]:].tolist() == plan.tiles.reshape(-1).tolist()


def test_restatement_reproduces_the_golden():
    from oracle.lpips_oracle import synth_lpips_state_dict
    z = np.load(GOLD)
    case = json.loads(str(z["case"]))
    assert case["boxes"] == R.BOXES and (case["H"], case["W"], case["seed"]) == (R.H, R.W, R.SEED)
    sd = synth_lpips_state_dict(case["lpips_seed"])
    img, rec = R.synth_images()
    rec.requires_grad_(True)
    loss, values = R.object_loss(sd, img, rec, R.BOXES)
    loss.backward()
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    assert np.allclose([float(v) for v in values], z["values"], rtol=1e-5)
    g = torch.from_numpy(z["drec"])
    assert float((rec.grad - g).abs().max()) <= 1e-4 * float(g.abs().max())
    assert torch.count_nonzero(g[1]) == 0                   # the image without boxes


def test_vq_img_loss_default_keeps_a_constant_zero_object_term():
    from losses.loss_img import VQLPIPSWithDiscriminator
    lf = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None)
    assert lf.object_loss is None
    keys = set(lf.state_dict().keys())
    assert all(k.startswith("discriminator.") for k in keys)


def test_vq_img_loss_object_term_shares_the_perceptual_weights():
    from losses.loss_img import VQLPIPSWithDiscriminator
    from losses.lpips import LPIPS
    from losses.object_loss import ObjectLoss
    plain = VQLPIPSWithDiscriminator(disc_start=0, face_loss=None)
    lf = VQLPIPSWithDiscriminator(disc_start=0, face_loss=None, object_loss="lpips")
    assert isinstance(lf.object_loss, ObjectLoss) and isinstance(lf.perceptual_loss, LPIPS)
    assert lf.object_loss.net is lf.perceptual_loss                 # one network, one set of weights
    assert set(lf.state_dict().keys()) == set(plain.state_dict().keys())
    own = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None, object_loss="lpips")
    assert isinstance(own.object_loss.net, LPIPS)
    marker = object()
    assert VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None, object_loss=marker).object_loss is marker
    with pytest.raises(ValueError):
        VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None, object_loss="vgg")


def test_vq_img_loss_uses_a_given_object_term():
    """the callable's value lands in the object slot of the returned tuple and in the sum"""
    from losses.loss_img import VQLPIPSWithDiscriminator
    seen = []

    def term(images, reconstructions, bbox_obj):
        seen.append(bbox_obj)
        return images.new_tensor(0.25)

    lf = VQLPIPSWithDiscriminator(disc_start=10, perceptual_loss=None, face_loss=None, object_loss=term)
    ref = VQLPIPSWithDiscriminator(disc_start=10, perceptual_loss=None, face_loss=None)
    last = torch.nn.Conv2d(4, 3, 3, padding=1)
    z = torch.randn(2, 4, 8, 8)
    img = torch.rand(2, 3, 8, 8)
    bbox = [[[0, 0, 8, 8]], []]
    rec = last(z)
    lf.discriminator = ref.discriminator = torch.nn.Sequential(torch.nn.Conv2d(3, 1, 1))
    loss, (nll, obj, face) = lf(0, 0, img, rec, torch.zeros(()), bbox_obj=bbox, last_layer=last)
    loss0, (_, obj0, _) = ref(0, 0, img, rec, torch.zeros(()), bbox_obj=bbox, last_layer=last)
    assert seen == [bbox] and float(obj) == 0.25 and float(obj0) == 0.0
    assert abs(float(loss) - float(loss0) - 0.25) < 1e-6
    with pytest.raises(ValueError):
        lf(0, 0, img, rec, torch.zeros(()), bbox_obj=None, last_layer=last)


def test_forward_without_gpu_refuses():
    from losses.object_loss import ObjectLoss
    m = ObjectLoss()
    img, rec = R.synth_images()
    with pytest.raises(RuntimeError):
        m(img, rec, R.BOXES)


def test_object_abi_entries_reject_bad_arguments_without_gpu():
    import ctypes
    import mas_hip
    L = mas_hip.lib()
    assert L.mas_obj_canvas_fwd(None, None, None, None, None, None, 0, None) == -1
    p = mas_hip.ObjPlan(8, 8, 8, 8, 1, 1, 1, 20, 16, 0)                    # H not a multiple of 16
    assert L.mas_obj_relu_fwd(8, ctypes.byref(p), 0, 2, 64, 0, None) == -1 and b"plan" in L.mas_last_error()
    p.H = 32
    assert L.mas_obj_relu_fwd(8, ctypes.byref(p), 5, 2, 64, 0, None) == -1         # level out of range
    assert L.mas_obj_pool_fwd(8, 8, ctypes.byref(p), 4, 2, 64, 0, None) == -1      # no pool after level 4
    assert L.mas_obj_relu_bwd(8, 8, 8, 12, 0, None) == -1                          # n % 8
    assert L.mas_obj_head_fwd(8, 8, ctypes.byref(p), 0, 96, 0, 1, 8, None) == -1   # C not a power of two in 64..512
    assert L.mas_obj_finalize(None, ctypes.byref(p), None, None) == -1
