"""CPU restatement of the reference's FaceLoss (losses/face_loss.py) for the tests: torchvision's tensor ``crop`` / ``Resize(256)`` /
``CenterCrop(254)`` rules written with ``F.pad`` / ``F.interpolate`` (bilinear, align_corners=False, antialias=True), the caffe-style
ResNet-50 on a state_dict, and the loss with the reference's ``faces[:6]`` row selection.  Plus ``synth_face_state_dict``: seeded
weights (numpy) under which every layer sees both ReLU signs and feature standard deviations stay between 0.05 and 20 at 254 x 254."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

ALPHAS = [0.1, 0.25 * 0.01, 0.25 * 0.1, 0.25 * 0.2, 0.25 * 0.02]
LAYERS = [(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)]      # (planes, blocks, stride of the first block)


# ---- torchvision (tensor) transforms ------------------------------------------------------------------------------------------
def tv_crop(img, top, left, height, width):
    """torchvision.transforms.functional.crop on a tensor: zero padding where the box leaves the image"""
    h, w = img.shape[-2:]
    right, bottom = left + width, top + height
    if left < 0 or top < 0 or right > w or bottom > h:
        pad_ltrb = [max(-left + min(0, right), 0), max(-top + min(0, bottom), 0), max(right - w, 0), max(bottom - h, 0)]
        sub = img[..., max(top, 0):bottom, max(left, 0):right]
        return F.pad(sub, [pad_ltrb[0], pad_ltrb[2], pad_ltrb[1], pad_ltrb[3]], value=0.0)
    return img[..., top:bottom, left:right]


def resized_size(h, w, size=256):
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def tv_resize(img, size=256):
    h, w = img.shape[-2:]
    oh, ow = resized_size(h, w, size)
    if (oh, ow) == (h, w):
        return img
    x = img[None] if img.dim() == 3 else img
    y = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=True)
    return y[0] if img.dim() == 3 else y


def tv_center_crop(img, size=254):
    h, w = img.shape[-2:]
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return tv_crop(img, top, left, size, size)


def face_crop(img, box):
    """one [3,H,W] image, one [x_min, y_min, x_max, y_max] box -> [3, 254, 254]"""
    x0, y0, x1, y1 = (int(v) for v in box)
    return tv_center_crop(tv_resize(tv_crop(img, y0, x0, y1 - y0, x1 - x0)))


def prepare_faces(imgs, recs, bboxes):
    gt, gen = [], []
    for img, rec, boxes in zip(imgs, recs, bboxes):
        for box in boxes:
            gt.append(face_crop(img, box))
            gen.append(face_crop(rec, box))
    if not gt:
        return None
    return torch.cat([torch.stack(gt), torch.stack(gen)], dim=0)


# ---- the network ---------------------------------------------------------------------------------------------------------------
def _bn(sd, p, x, training=False):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], training, 0.1, 1e-5)


def features(sd, x, training=False):
    """reference FaceLoss._forward on a state_dict: [conv1 output, layer1, layer2, layer3, layer4].  training: batch statistics
    (the running statistics in ``sd`` are updated in place, as the modules do)."""
    feats = []
    x = F.conv2d(x, sd["conv1.weight"], stride=2, padding=3)
    feats.append(x)
    x = F.max_pool2d(F.relu(_bn(sd, "bn1", x, training)), 3, 2, 0, ceil_mode=True)
    for li, (planes, blocks, stride) in enumerate(LAYERS, start=1):
        for b in range(blocks):
            p = f"layer{li}.{b}."
            s = stride if b == 0 else 1
            out = F.relu(_bn(sd, p + "bn1", F.conv2d(x, sd[p + "conv1.weight"], stride=s), training))
            out = F.relu(_bn(sd, p + "bn2", F.conv2d(out, sd[p + "conv2.weight"], padding=1), training))
            out = _bn(sd, p + "bn3", F.conv2d(out, sd[p + "conv3.weight"]), training)
            res = x
            if p + "downsample.0.weight" in sd:
                res = _bn(sd, p + "downsample.1", F.conv2d(x, sd[p + "downsample.0.weight"], stride=s), training)
            x = F.relu(out + res)
        feats.append(x)
    return feats


def face_loss(sd, img, rec, bbox, training=False, return_diffs=False, l1_fp32=False):
    """reference FaceLoss.forward: -> loss (and the five weighted terms).  l1_fp32: the features are taken to fp32 before the L1
    distances (under autocast the reference's own L1 and the loss would be bf16 tensors: a final rounding of up to 2^-9 of the loss
    that measures the scalar's storage, not the network)"""
    faces = prepare_faces(img, rec, bbox)
    if faces is None:
        z = img.new_tensor(0)
        return (z, None) if return_diffs else z
    faces = faces[:6]
    feats = [(f.float() if l1_fp32 else f).chunk(2) for f in features(sd, faces, training)]
    diffs = [a * torch.abs(p[0] - p[1]).sum(dim=0).mean() for a, p in zip(ALPHAS, feats)]
    loss = sum(diffs)
    return (loss, torch.stack(diffs)) if return_diffs else loss


# ---- seeded synthetic weights --------------------------------------------------------------------------------------------------
def expected_shapes():
    """the reference module's state_dict keys and shapes, in its order"""
    out = OrderedDict()

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{p}.{k}"] = (c,)
        out[f"{p}.num_batches_tracked"] = ()

    out["conv1.weight"] = (64, 3, 7, 7)
    bn("bn1", 64)
    inplanes = 64
    for li, (planes, blocks, stride) in enumerate(LAYERS, start=1):
        for b in range(blocks):
            p = f"layer{li}.{b}"
            out[p + ".conv1.weight"] = (planes, inplanes, 1, 1)
            bn(p + ".bn1", planes)
            out[p + ".conv2.weight"] = (planes, planes, 3, 3)
            bn(p + ".bn2", planes)
            out[p + ".conv3.weight"] = (planes * 4, planes, 1, 1)
            bn(p + ".bn3", planes * 4)
            if b == 0:
                out[p + ".downsample.0.weight"] = (planes * 4, inplanes, 1, 1)
                bn(p + ".downsample.1", planes * 4)
            inplanes = planes * 4
    return out


def synth_face_state_dict(seed=0):
    """He-scaled convolutions; BatchNorm running statistics that centre each layer only roughly (random means and variances), so
    both ReLU signs occur everywhere; the residual branch's bn3 and the downsample's BatchNorm scaled down so that 16 residual
    additions keep the features between 0.05 and 20 in standard deviation."""
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    for k, shape in expected_shapes().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
            continue
        if k.endswith(".weight") and len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            v = rs.standard_normal(shape) * np.sqrt(2.0 / fan_in)
        elif k.endswith("running_var"):
            v = rs.uniform(0.5, 2.0, shape)
        elif k.endswith("running_mean"):
            v = rs.standard_normal(shape) * 0.2
        elif k.endswith(".bias"):
            v = rs.standard_normal(shape) * 0.2
        else:                                                      # BatchNorm weight
            lo, hi = (0.2, 0.5) if (".bn3." in k or "downsample.1" in k) else (0.6, 1.4)
            v = rs.uniform(lo, hi, shape)
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return sd


def synth_images(n, h, w, seed):
    """seeded img / rec pair in [-1, 1] (rec = img + a small perturbation, as a reconstruction)"""
    rs = np.random.RandomState(seed)
    img = rs.uniform(-1.0, 1.0, (n, 3, h, w)).astype(np.float32)
    rec = np.clip(img + 0.3 * rs.standard_normal((n, 3, h, w)).astype(np.float32), -1.0, 1.0)
    return torch.from_numpy(img), torch.from_numpy(rec)
