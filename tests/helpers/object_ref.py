"""CPU fp32 restatement of the object-aware VQ-IMG term (the reference's commented block, losses/loss_img.py:91-106, with the two
documented differences: boxes with a side under 16 px are skipped and not counted, and only ``reconstructions`` is differentiated)
on ``oracle.lpips_oracle``: torchvision's zero-padding ``crop`` and one LPIPS per box.  Pinned by tests/golden/object_tiny.npz, which
the reference's own LPIPS class wrote (tests/golden/make_object_golden.py)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import lpips_oracle as L  # noqa: E402

MIN_SIDE = 16

# the golden's case: three 48 x 64 images; image 0: an odd-sized box, a box overlapping it, a box crossing the left and bottom edges,
# an exactly 16 px box, and two boxes under 16 px (skipped); image 1: no boxes; image 2: a landscape box and one crossing the right edge
H, W, SEED = 48, 64, 21
BOXES = [[[4, 6, 31, 41], [20, 15, 52, 47], [-8, 30, 20, 58], [44, 2, 60, 18], [10, 40, 22, 47], [50, 20, 60, 44]],
         [],
         [[3, 5, 40, 26], [30, 20, 70, 47]]]


def synth_images(n=3, h=H, w=W, seed=SEED):
    """seeded img / rec pair in [-1, 1] (rec = img + a small perturbation, as a reconstruction)"""
    rs = np.random.RandomState(seed)
    img = rs.uniform(-1.0, 1.0, (n, 3, h, w)).astype(np.float32)
    rec = np.clip(img + 0.3 * rs.standard_normal((n, 3, h, w)).astype(np.float32), -1.0, 1.0)
    return torch.from_numpy(img), torch.from_numpy(rec)


def tv_crop(img, top, left, height, width):
    """torchvision.transforms.functional.crop on a tensor: zero padding where the box leaves the image"""
    h, w = img.shape[-2:]
    right, bottom = left + width, top + height
    if left < 0 or top < 0 or right > w or bottom > h:
        pad_ltrb = [max(-left + min(0, right), 0), max(-top + min(0, bottom), 0), max(right - w, 0), max(bottom - h, 0)]
        sub = img[..., max(top, 0):bottom, max(left, 0):right]
        return F.pad(sub, [pad_ltrb[0], pad_ltrb[2], pad_ltrb[1], pad_ltrb[3]], value=0.0)
    return img[..., top:bottom, left:right]


def used(boxes):
    return [b for b in boxes if (b[3] - b[1]) >= MIN_SIDE and (b[2] - b[0]) >= MIN_SIDE]


def lpips_fp32_head(sd, real_x, fake_x):
    """oracle LPIPS with the head in fp32 (the features are taken to fp32 first, as the HIP path does): under CPU autocast the
    convolutions run in bf16 and the head's own bf16 rounding does not become the yardstick"""
    shift, scale = sd["scaling_layer.shift"], sd["scaling_layer.scale"]
    fr = L.vgg_features(sd, (real_x - shift) / scale)
    ff = L.vgg_features(sd, (fake_x - shift) / scale)
    total = 0
    for i in range(5):
        d = (L.norm_tensor(fr[i].float()) - L.norm_tensor(ff[i].float())) ** 2
        total = total + F.conv2d(d, sd[f"lin{i}.model.1.weight"].float()).mean([2, 3], keepdim=True)
    return total


def object_loss(sd, images, recs, bbox, net=None):
    """-> (loss, [every used crop's LPIPS in (image, box) order]); ``net(sd, a, b)``: the LPIPS (default: the oracle's)"""
    net = net or L.lpips
    loss, values = 0, []
    for img, rec, boxes in zip(images, recs, bbox):
        u = used(boxes)
        s = 0
        for x0, y0, x1, y1 in u:
            a = tv_crop(img, y0, x0, y1 - y0, x1 - x0)[None]
            b = tv_crop(rec, y0, x0, y1 - y0, x1 - x0)[None]
            v = net(sd, a, b).mean()
            values.append(v)
            s = s + v
        loss = loss + s / (len(u) + 1)
    return loss, values
