"""FaceLoss on the MI355X (losses/face_loss.py, mas_hip/face.py, csrc/face.hip) against the CPU restatement of the reference
(tests/helpers/face_ref.py) and the golden the reference's own module wrote (tests/golden/face_tiny.npz).

Tolerances:
- one kernel in fp32: 3e-2 * max|ref| (the library's per-kernel bound; these kernels are fp32 arithmetic and land far inside it);
- the whole loss in fp32 parity mode: 1e-3 relative -- 53 convolutions in exact fp32 MFMA, only the summation order differs;
- the whole loss in bf16: loss and d rec within 1.2x the deviation of the restatement itself under torch.autocast(bfloat16) on the
  CPU (the same storage precision: the yardstick is what bf16 does to this network, not an absolute number), d rec cosine >= 0.98.
  The restatement's features are taken to fp32 for the L1 distances, as here: under autocast the reference's loss is itself a bf16
  scalar, whose final rounding (up to 2^-9 of the loss: 6e-4 on the n = 4 case) would otherwise be the whole yardstick."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import face_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "face_tiny.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLD)
    return z, json.loads(str(z["cases"]))


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("face") / "face_synth.pt"
    torch.save(R.synth_face_state_dict(0), p)
    return str(p)


@pytest.fixture
def face_module(ckpt, monkeypatch):
    monkeypatch.setenv("MAS_FACE_CKPT", ckpt)
    from losses.face_loss import FaceLoss
    return FaceLoss().to(DEV)


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _cos(a, b):
    a, b = a.detach().float().cpu().flatten(), b.detach().float().cpu().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30))


BOXES = [[[-6, 30, 20, 60], [10, 4, 50, 24], [12, 8, 40, 44]], [[-130, -120, 170, 180], [3, 5, 33, 30]]]   # edge, landscape, overlap, down, portrait


def test_crop_forward_backward_fp32():
    from mas_hip import face as FH
    img, rec = R.synth_images(2, 56, 64, 3)
    rows = []
    for b, boxes in enumerate(BOXES):
        for box in boxes:
            g = FH.face_geometry(box)
            rows.append(FH.FaceRow(1, b, g["top"], g["left"], g["h"], g["w"], g["rh"], g["rw"], g["ct"], g["cl"]))
    got = FH.crop_faces(img.to(DEV), rec.to(DEV).contiguous(memory_format=torch.channels_last), rows, torch.float32)
    ref = torch.stack([R.face_crop(rec[b], box) for b, boxes in enumerate(BOXES) for box in boxes])
    assert _rel(got, ref) < 3e-2 and _rel(got, ref) < 1e-4, _rel(got, ref)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(0))
    rr = rec.clone().requires_grad_(True)
    (torch.stack([R.face_crop(rr[b], box) for b, boxes in enumerate(BOXES) for box in boxes]) * g).sum().backward()
    d = FH.crop_faces_bwd(g.permute(0, 2, 3, 1).contiguous().to(DEV), rows, rec.to(DEV))
    assert _rel(d, rr.grad) < 3e-2 and _rel(d, rr.grad) < 1e-4, _rel(d, rr.grad)
    d2 = FH.crop_faces_bwd(g.permute(0, 2, 3, 1).contiguous().to(DEV), rows, rec.to(DEV))
    assert torch.equal(d, d2)                               # a gather in a fixed order: bitwise repeatable


def test_stem_forward_and_data_gradient_fp32():
    import ctypes as C
    from mas_hip import face as FH
    from mas_hip import check, lib, ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 3, 254, 254, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    y = torch.empty((3, 64, 127, 127), device=DEV, memory_format=torch.channels_last)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    wd = w.to(DEV)
    check(lib().mas_face_stem_fwd(C.c_void_p(xd.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(y.data_ptr()), 0, 3, ops._stream()), "stem")
    xr = x.clone().requires_grad_(True)
    ref = F.conv2d(xr, w, stride=2, padding=3)
    assert _rel(y, ref) < 3e-2 and _rel(y, ref) < 1e-4
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy)
    dyd = dy.to(DEV).contiguous(memory_format=torch.channels_last)
    dx = torch.empty((3, 254, 254, 3), device=DEV)
    check(lib().mas_face_stem_dgrad(C.c_void_p(dyd.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(dx.data_ptr()), 0, 3, ops._stream()), "stem")
    assert _rel(dx.permute(0, 3, 1, 2), xr.grad) < 3e-2 and _rel(dx.permute(0, 3, 1, 2), xr.grad) < 1e-4
    assert FH.FACE == 254


def test_bn_relu_pool_pass_against_torch():
    import ctypes as C
    from mas_hip import check, lib, ops
    g = torch.Generator().manual_seed(2)
    y = torch.randn(2, 64, 127, 127, generator=g)
    y[:, :, 10:20, 10:20] = 0.5                             # ties: the first maximum in row-major window order takes the gradient
    scale, shift = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
    ss = torch.stack([scale, shift], 1).contiguous().to(DEV)
    yd = y.to(DEV).contiguous(memory_format=torch.channels_last)
    z = torch.empty((2, 64, 63, 63), device=DEV, memory_format=torch.channels_last)
    idx = torch.empty(2 * 63 * 63 * 64, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(lib().mas_face_pool_fwd(p(yd), p(ss), p(z), p(idx), 0, 2, 127, 127, 64, ops._stream()), "pool")
    yr = y.clone().requires_grad_(True)
    ref = F.max_pool2d(F.relu(yr * scale[:, None, None] + shift[:, None, None]), 3, 2, 0, ceil_mode=True)
    assert _rel(z, ref) < 1e-6
    dz = torch.randn(ref.shape, generator=g)
    ref.backward(dz)
    seed = torch.randn(y.shape, generator=g)
    dzd = dz.to(DEV).contiguous(memory_format=torch.channels_last)
    sd_ = seed.to(DEV).contiguous(memory_format=torch.channels_last)
    dy = torch.empty_like(yd)
    check(lib().mas_face_pool_bwd(p(yd), p(ss), p(dzd), p(idx), p(sd_), p(dy), 0, 2, 127, 127, 64, ops._stream()), "pool")
    assert _rel(dy, yr.grad + seed) < 1e-5


def _case(golden, name):
    z, cases = golden
    c = next(c for c in cases if c["name"] == name)
    img, rec = R.synth_images(c["images"], c["H"], c["W"], c["seed"])
    return c, img, rec, z[name + "/loss"], z[name + "/diffs"], z[name + "/drec"]


@pytest.mark.parametrize("name", ["n1_portrait", "n3_edge_land_down", "n4_overlap", "n7_all_gt"])
def test_face_loss_fp32_matches_golden(golden, face_module, name):
    from mas_hip import ops
    ops.set_compute_dtype(torch.float32)
    c, img, rec, loss_g, diffs_g, drec_g = _case(golden, name)
    r = rec.to(DEV).requires_grad_(True)
    loss = face_module(img.to(DEV), r, c["boxes"])
    loss.backward()
    assert abs(float(loss) - float(loss_g)) <= 1e-3 * abs(float(loss_g))
    assert _rel(face_module.last_diffs, torch.from_numpy(diffs_g)) < 1e-3
    dg = torch.from_numpy(drec_g)
    if name == "n7_all_gt":
        assert torch.count_nonzero(r.grad) == 0
    else:
        assert _rel(r.grad, dg) < 1e-3, _rel(r.grad, dg)


@pytest.mark.parametrize("name", ["n1_portrait", "n3_edge_land_down", "n4_overlap"])
def test_face_loss_bf16_within_autocast_deviation(golden, face_module, name):
    from mas_hip import ops
    ops.set_compute_dtype(torch.bfloat16)
    c, img, rec, loss_g, _, drec_g = _case(golden, name)
    sd = R.synth_face_state_dict(0)
    rr = rec.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        la = R.face_loss(sd, img, rr, c["boxes"], l1_fp32=True)
    la.backward()
    dg = torch.from_numpy(drec_g)
    dev_loss = abs(float(la) - float(loss_g))
    dev_drec = float((rr.grad - dg).abs().max())
    r = rec.to(DEV).requires_grad_(True)
    loss = face_module(img.to(DEV), r, c["boxes"])
    loss.backward()
    assert abs(float(loss) - float(loss_g)) <= 1.2 * dev_loss + 1e-6 * abs(float(loss_g)), (float(loss), float(loss_g), dev_loss)
    assert float((r.grad.cpu() - dg).abs().max()) <= 1.2 * dev_drec, (float((r.grad.cpu() - dg).abs().max()), dev_drec)
    assert _cos(r.grad, dg) >= 0.98


def test_no_faces_launches_nothing(face_module):
    from mas_hip import ops
    img, rec = R.synth_images(2, 32, 32, 5)
    ops.upsample2x(torch.zeros(1, 8, 2, 2, dtype=torch.bfloat16, device=DEV).contiguous(memory_format=torch.channels_last))
    before = ops.last_kernel()
    r = rec.to(DEV).requires_grad_(True)
    out = face_module(img.to(DEV), r, [[], []])
    assert float(out) == 0.0 and not out.requires_grad
    assert ops.last_kernel() == before
    assert r.grad is None


def test_forward_backward_bitwise_repeatable(golden, face_module):
    c, img, rec, *_ = _case(golden, "n3_edge_land_down")
    outs = []
    for _ in range(2):
        r = rec.to(DEV).requires_grad_(True)
        loss = face_module(img.to(DEV), r, c["boxes"])
        loss.backward()
        outs.append((loss.detach().clone(), r.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_eval_path_touches_no_aten_activation_op(golden, face_module, monkeypatch):
    c, img, rec, *_ = _case(golden, "n4_overlap")
    imgd, r = img.to(DEV), rec.to(DEV).requires_grad_(True)

    def boom(*a, **k):
        raise AssertionError("ATen op on an activation map")

    for name in ("conv2d", "max_pool2d", "relu", "interpolate", "batch_norm"):
        monkeypatch.setattr(F, name, boom)
    loss = face_module(imgd, r, c["boxes"])
    loss.backward()
    assert torch.isfinite(r.grad).all() and r.grad.abs().max() > 0


def test_train_mode_matches_restatement(golden, face_module):
    c, img, rec, *_ = _case(golden, "n3_edge_land_down")
    sd = R.synth_face_state_dict(0)
    rr = rec.clone().requires_grad_(True)
    ref = R.face_loss(copy.deepcopy(sd), img, rr, c["boxes"], training=True)
    ref.backward()
    face_module.train()
    r = rec.to(DEV).requires_grad_(True)
    loss = face_module(img.to(DEV), r, c["boxes"])
    loss.backward()
    assert abs(float(loss) - float(ref)) <= 2e-3 * abs(float(ref))
    assert _rel(r.grad, rr.grad) < 2e-2 and _cos(r.grad, rr.grad) > 0.999


def test_vq_img_generator_step_with_face_term(golden, face_module):
    """d(decoder input) with the face term minus without it == the face term's own gradient (restatement) through the decoder"""
    from losses.loss_img import VQLPIPSWithDiscriminator
    from mas_hip import ops
    from models.modules import Conv2d
    ops.set_compute_dtype(torch.float32)
    torch.manual_seed(0)
    c, img, _, *_ = _case(golden, "n3_edge_land_down")
    h, w = c["H"], c["W"]
    last = Conv2d(8, 3, 3, 1, 1).to(DEV)
    zin = torch.randn(img.shape[0], 8, h, w, generator=torch.Generator().manual_seed(3))
    lf_on = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=face_module).to(DEV)
    lf_off = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None).to(DEV)
    lf_off.discriminator.load_state_dict(lf_on.discriminator.state_dict())
    grads = []
    for lf in (lf_on, lf_off):
        z = zin.to(DEV).requires_grad_(True)
        rec = last(z)
        q = torch.zeros((), device=DEV)
        loss, _ = lf(0, 1, img.to(DEV), rec, q, bbox_face=c["boxes"], last_layer=last)
        (gz,) = torch.autograd.grad(loss, z)
        grads.append(gz)
    diff = grads[0] - grads[1]
    z = zin.to(DEV).requires_grad_(True)
    rec = last(z)
    rec_cpu = rec.detach().cpu().requires_grad_(True)
    R.face_loss(R.synth_face_state_dict(0), img, rec_cpu, c["boxes"]).backward()
    (want,) = torch.autograd.grad(rec, z, grad_outputs=rec_cpu.grad.to(DEV))
    assert _rel(diff, want) < 2e-2 and _cos(diff, want) > 0.999
