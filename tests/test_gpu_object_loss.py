"""The object-aware VQ-IMG term on the MI355X (losses/object_loss.py, mas_hip/objects.py, csrc/object.hip) against torch, the CPU
restatement (tests/helpers/object_ref.py), the golden the reference's own LPIPS wrote (tests/golden/object_tiny.npz) and a per-crop
loop through the existing GPU LPIPS.

Tolerances (the FaceLoss yardsticks):
- one kernel in fp32: 1e-4 of max|ref| (fp32 arithmetic; only summation orders differ);
- the whole term in fp32 parity mode: 1e-3 relative (thirteen convolutions in exact fp32 MFMA);
- the whole term in bf16: loss and d rec within 1.2x the deviation of the restatement itself under torch.autocast(bfloat16) on the
  CPU (its head in fp32, as here), d rec cosine >= 0.98."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import object_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "object_tiny.npz")


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _cos(a, b):
    a, b = a.detach().float().cpu().flatten(), b.detach().float().cpu().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30))


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLD)
    return z, json.loads(str(z["case"]))


@pytest.fixture(scope="module")
def sd():
    from oracle.lpips_oracle import synth_lpips_state_dict
    return synth_lpips_state_dict(3)


@pytest.fixture(scope="module")
def lpips_net(sd):
    from losses.lpips import LPIPS
    m = LPIPS().eval()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _seeded_boxes(seed, n_images, size, lo, hi, per_image=4):
    rng = random.Random(seed)
    out = []
    for _ in range(n_images):
        boxes = []
        for _ in range(per_image):
            h, w = rng.randint(lo, hi), rng.randint(lo, hi)
            y0, x0 = rng.randint(-h // 4, size - 3 * h // 4), rng.randint(-w // 4, size - 3 * w // 4)
            boxes.append([x0, y0, x0 + w, y0 + h])
        out.append(boxes)
    return out


# ---- the atlas, restated in torch -------------------------------------------------------------------------------------------
def _masks(plan):
    """[5] bool [n_canvas, H >> l, W >> l]: the cells' valid rectangles per level"""
    out = []
    for l in range(5):
        m = torch.zeros(plan.n_canvas, plan.H >> l, plan.W >> l, dtype=torch.bool)
        for (n, oy, ox, h, w, *_r) in plan.cells:
            m[n, oy >> l:(oy >> l) + (h >> l), ox >> l:(ox >> l) + (w >> l)] = True
        out.append(m)
    return out


def _mask_nchw(mask, sides=2):
    return mask.repeat(sides, 1, 1)[:, None].float()


def _torch_canvas(plan, img, rec, shift, scale):
    can = torch.zeros(2 * plan.n_canvas, 8, plan.H, plan.W)
    for side, src in enumerate((img, rec)):
        for (n, oy, ox, h, w, b, top, left) in plan.cells:
            c = R.tv_crop(src[b], top, left, h, w)
            can[side * plan.n_canvas + n, :3, oy:oy + h, ox:ox + w] = (c - shift.view(3, 1, 1)) / scale.view(3, 1, 1)
    return can


def _plan_and_table(bbox, n_images):
    from mas_hip import objects as O
    plan = O.make_plan(bbox, n_images)
    table, p = O.upload(plan, DEV)
    return plan, table, p


def test_canvas_forward_and_adjoint_fp32():
    from mas_hip import objects as O
    img, rec = R.synth_images()
    plan, table, p = _plan_and_table(R.BOXES, 3)
    shift, scale = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])
    got = O.canvas_fwd(img.to(DEV), rec.to(DEV), p, shift.to(DEV), scale.to(DEV), torch.float32)
    want = _torch_canvas(plan, img, rec, shift, scale)
    assert _rel(got, want) < 1e-6
    # adjoint: d rec from a random rec-side canvas gradient, against torch's autograd of the crop + scaling
    g = torch.randn(plan.n_canvas, 8, plan.H, plan.W, generator=torch.Generator().manual_seed(1))
    rr = rec.clone().requires_grad_(True)
    (_torch_canvas(plan, img, rr, shift, scale)[plan.n_canvas:] * g).sum().backward()
    gd = g.to(DEV).contiguous(memory_format=torch.channels_last)
    d = O.canvas_bwd(gd, p, scale.to(DEV), rec.to(DEV))
    assert _rel(d, rr.grad) < 1e-5
    assert torch.equal(d, O.canvas_bwd(gd, p, scale.to(DEV), rec.to(DEV)))        # a gather in a fixed order


@pytest.mark.parametrize("level", [0, 2, 4])
def test_masked_relu_and_backward_fp32(level):
    from mas_hip import objects as O
    plan, table, p = _plan_and_table(R.BOXES, 3)
    m = _mask_nchw(_masks(plan)[level])
    c = 64
    y = torch.randn(2 * plan.n_canvas, c, plan.H >> level, plan.W >> level, generator=torch.Generator().manual_seed(level))
    yd = y.to(DEV).contiguous(memory_format=torch.channels_last)
    O.relu_fwd(yd, p, level)
    want = F.relu(y) * m
    assert torch.equal(yd.cpu(), want)
    da = torch.randn(y.shape, generator=torch.Generator().manual_seed(7)).to(DEV).contiguous(memory_format=torch.channels_last)
    dy = O.relu_bwd(da.clone(), yd)
    assert torch.equal(dy.cpu(), da.cpu() * (want > 0))


@pytest.mark.parametrize("level", [0, 3])
def test_masked_pool_and_backward_fp32(level):
    from mas_hip import objects as O
    plan, table, p = _plan_and_table(R.BOXES, 3)
    masks = _masks(plan)
    c, nc = 128, plan.n_canvas
    x = F.relu(torch.randn(2 * nc, c, plan.H >> level, plan.W >> level, generator=torch.Generator().manual_seed(3))) * _mask_nchw(masks[level])
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    got = O.pool_fwd(xd, p, level)
    want = F.max_pool2d(x, 2, 2) * _mask_nchw(masks[level + 1])
    assert torch.equal(got.cpu(), want)
    # backward on the rec side: a > 0 ? seed + routed dz : 0
    a = x[nc:].clone().requires_grad_(True)
    dz = torch.randn(nc, c, plan.H >> (level + 1), plan.W >> (level + 1), generator=torch.Generator().manual_seed(4))
    seed = torch.randn(a.shape, generator=torch.Generator().manual_seed(5))
    (F.max_pool2d(a, 2, 2) * _mask_nchw(masks[level + 1], 1) * dz).sum().backward()
    want_d = (a.detach() > 0) * (seed + a.grad)
    cl = torch.channels_last
    dy = O.pool_bwd(xd[nc:], seed.to(DEV).contiguous(memory_format=cl), dz.to(DEV).contiguous(memory_format=cl), p, level)
    assert _rel(dy, want_d) < 1e-6


def test_head_finalize_and_head_backward_fp32():
    """random masked features at all five levels: the crops' LPIPS heads, the loss and the rec-side seeds against torch"""
    from mas_hip import objects as O
    plan, table, p = _plan_and_table(R.BOXES, 3)
    masks = _masks(plan)
    nc, gen = plan.n_canvas, torch.Generator().manual_seed(11)
    feats = [F.relu(torch.randn(2 * nc, c, plan.H >> l, plan.W >> l, generator=gen)) * _mask_nchw(masks[l]) for l, c in enumerate(O.CHANNELS)]
    ws = [torch.rand(c, generator=gen) * (2.0 / c) for c in O.CHANNELS]
    fd = [f.to(DEV).contiguous(memory_format=torch.channels_last) for f in feats]
    wd = [w.to(DEV) for w in ws]
    partial = torch.empty(sum(plan.level_blocks(l) for l in range(5)), device=DEV)
    off = 0
    for l in range(5):
        O.head_fwd(fd[l], wd[l], p, plan, l, partial[off:])
        off += plan.level_blocks(l)
    out = O.finalize(partial, p, DEV)
    recf = [f[nc:].clone().requires_grad_(True) for f in feats]
    vals = []
    for (n, oy, ox, h, w, *_r) in plan.cells:
        v = 0
        for l in range(5):
            sl = (slice(None), slice(oy >> l, (oy >> l) + (h >> l)), slice(ox >> l, (ox >> l) + (w >> l)))
            fr, ff = feats[l][n][sl], recf[l][n][sl]
            d = (fr / (fr.norm(dim=0, keepdim=True) + 1e-10) - ff / (ff.norm(dim=0, keepdim=True) + 1e-10)) ** 2
            v = v + (d * ws[l].view(-1, 1, 1)).sum(0).mean()
        vals.append(v)
    loss = 0
    for b in range(plan.n_images):
        k0, k1 = plan.img_cell0[b], plan.img_cell0[b + 1]
        loss = loss + sum(vals[k0:k1], torch.zeros(())) / (k1 - k0 + 1)
    want = torch.stack([loss] + vals)
    assert _rel(out, want.detach()) < 1e-5
    dout = torch.randn(want.shape, generator=gen)
    (want * dout).sum().backward()
    dd = dout.to(DEV)
    for l in range(5):
        seed = O.head_bwd(fd[l], wd[l], p, l, dd)
        assert _rel(seed, recf[l].grad) < 1e-4, (l, _rel(seed, recf[l].grad))


# ---- the whole term ---------------------------------------------------------------------------------------------------------
def test_object_loss_fp32_matches_golden_and_restatement(golden, sd, lpips_net):
    from losses.object_loss import ObjectLoss
    from mas_hip import ops
    ops.set_compute_dtype(torch.float32)
    z, case = golden
    img, rec = R.synth_images()
    r = rec.to(DEV).requires_grad_(True)
    m = ObjectLoss(lpips_net)
    loss = m(img.to(DEV), r, case["boxes"])
    loss.backward()
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-3 * abs(float(z["loss"])), (float(loss.detach()), float(z["loss"]))
    assert _rel(m.last_values, torch.from_numpy(z["values"])) < 1e-3
    assert _rel(r.grad, torch.from_numpy(z["drec"])) < 1e-3, _rel(r.grad, torch.from_numpy(z["drec"]))
    assert torch.count_nonzero(r.grad[1]) == 0
    rr = rec.clone().requires_grad_(True)
    ref, _ = R.object_loss(sd, img, rr, R.BOXES)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-3 * abs(float(ref.detach()))
    # (the restatement's own fp32 CPU gradient may differ from the golden by a few 1e-4 of its maximum on another CPU)
    assert _rel(r.grad, rr.grad) < 1e-3 + _rel(rr.grad, torch.from_numpy(z["drec"]))


def test_object_loss_bf16_within_autocast_deviation(golden, sd, lpips_net):
    from losses.object_loss import ObjectLoss
    from mas_hip import ops
    ops.set_compute_dtype(torch.bfloat16)
    z, case = golden
    img, rec = R.synth_images()
    rr = rec.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        la, _ = R.object_loss(sd, img, rr, R.BOXES, net=R.lpips_fp32_head)
    la.backward()
    loss_g, dg = float(z["loss"]), torch.from_numpy(z["drec"])
    dev_loss = abs(float(la.detach()) - loss_g)
    dev_drec = float((rr.grad - dg).abs().max())
    r = rec.to(DEV).requires_grad_(True)
    loss = ObjectLoss(lpips_net)(img.to(DEV), r, case["boxes"])
    loss.backward()
    assert abs(float(loss.detach()) - loss_g) <= 1.2 * dev_loss + 1e-6 * abs(loss_g), (float(loss.detach()), loss_g, dev_loss)
    assert float((r.grad.cpu() - dg).abs().max()) <= 1.2 * dev_drec, (float((r.grad.cpu() - dg).abs().max()), dev_drec)
    assert _cos(r.grad, dg) >= 0.98


def test_no_used_box_launches_nothing(lpips_net):
    from losses.object_loss import ObjectLoss
    from mas_hip import ops
    img, rec = R.synth_images()
    ops.upsample2x(torch.zeros(1, 8, 2, 2, dtype=torch.bfloat16, device=DEV).contiguous(memory_format=torch.channels_last))
    before = ops.last_kernel()
    r = rec.to(DEV).requires_grad_(True)
    out = ObjectLoss(lpips_net)(img.to(DEV), r, [[[0, 0, 10, 40]], [], [[5, 5, 60, 12]]])
    assert float(out) == 0.0 and not out.requires_grad
    assert ops.last_kernel() == before


def test_forward_backward_bitwise_repeatable(lpips_net):
    from losses.object_loss import ObjectLoss
    img, rec = R.synth_images()
    m = ObjectLoss(lpips_net)
    outs = []
    for _ in range(2):
        r = rec.to(DEV).requires_grad_(True)
        loss = m(img.to(DEV), r, R.BOXES)
        loss.backward()
        outs.append((loss.detach().clone(), r.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_atlas_matches_a_per_crop_lpips_loop_at_b32(lpips_net):
    """B = 32, four seeded boxes per image (some crossing the edges, some under 16 px): the atlas against one GPU LPIPS call per
    crop (losses.lpips.LPIPS: bf16 convolutions, as the atlas in bf16)"""
    from losses.object_loss import ObjectLoss
    from mas_hip import ops
    ops.set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(32, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
    rec = (img + 0.2 * torch.randn(img.shape, generator=g).to(DEV)).clamp(-1, 1)
    bbox = _seeded_boxes(7, 32, 128, 10, 100)
    r = rec.clone().requires_grad_(True)
    m = ObjectLoss(lpips_net)
    loss = m(img, r, bbox)
    loss.backward()
    rr = rec.clone().requires_grad_(True)
    ref, vals = R.object_loss(None, img, rr, bbox, net=lambda _sd, a, b: lpips_net(a.contiguous(), b.contiguous()))
    ref.backward()
    assert len(vals) == m.last_values.numel() > 64
    assert _rel(m.last_values, torch.stack([v.detach() for v in vals])) < 2e-2
    assert abs(float(loss) - float(ref)) <= 1e-2 * abs(float(ref)), (float(loss), float(ref))
    assert _cos(r.grad, rr.grad) >= 0.99, _cos(r.grad, rr.grad)


def test_vq_img_generator_step_with_object_term(lpips_net, sd):
    """d(decoder input) with the object term minus without it == the term's own gradient (restatement) through the decoder"""
    from losses.loss_img import VQLPIPSWithDiscriminator
    from losses.object_loss import ObjectLoss
    from mas_hip import ops
    from models.modules import Conv2d
    ops.set_compute_dtype(torch.float32)
    torch.manual_seed(0)
    img, _ = R.synth_images()
    last = Conv2d(8, 3, 3, 1, 1).to(DEV)
    zin = torch.randn(img.shape[0], 8, R.H, R.W, generator=torch.Generator().manual_seed(3))
    lf_on = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None, object_loss=ObjectLoss(lpips_net)).to(DEV)
    lf_off = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None, face_loss=None).to(DEV)
    lf_off.discriminator.load_state_dict(lf_on.discriminator.state_dict())
    grads, objs = [], []
    for lf in (lf_on, lf_off):
        z = zin.to(DEV).requires_grad_(True)
        rec = last(z)
        q = torch.zeros((), device=DEV)
        loss, (_, obj, _) = lf(0, 1, img.to(DEV), rec, q, bbox_obj=R.BOXES, last_layer=last)
        (gz,) = torch.autograd.grad(loss, z)
        grads.append(gz)
        objs.append(float(obj))
    assert objs[0] > 0 and objs[1] == 0.0
    diff = grads[0] - grads[1]
    z = zin.to(DEV).requires_grad_(True)
    rec = last(z)
    rec_cpu = rec.detach().cpu().requires_grad_(True)
    R.object_loss(sd, img, rec_cpu, R.BOXES)[0].backward()
    (want,) = torch.autograd.grad(rec, z, grad_outputs=rec_cpu.grad.to(DEV))
    assert _rel(diff, want) < 2e-2 and _cos(diff, want) > 0.999


def test_vq_img_loss_lpips_option_runs_on_the_gpu(sd):
    """``object_loss="lpips"``: the term shares the perceptual LPIPS and the generator loss backpropagates through it"""
    from losses.loss_img import VQLPIPSWithDiscriminator
    from models.modules import Conv2d
    lf = VQLPIPSWithDiscriminator(disc_start=0, face_loss=None, object_loss="lpips")
    lf.perceptual_loss.load_state_dict(sd, strict=True)
    lf = lf.to(DEV)
    img, _ = R.synth_images()
    last = Conv2d(8, 3, 3, 1, 1).to(DEV)
    z = torch.randn(img.shape[0], 8, R.H, R.W, generator=torch.Generator().manual_seed(4)).to(DEV).requires_grad_(True)
    rec = last(z)
    loss, (_, obj, _) = lf(0, 1, img.to(DEV), rec, torch.zeros((), device=DEV), bbox_obj=R.BOXES, last_layer=last)
    loss.backward()
    assert float(obj) > 0 and torch.isfinite(z.grad).all() and z.grad.abs().max() > 0
