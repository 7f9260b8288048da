#!/usr/bin/env python3
"""Generates tests/golden/object_tiny.npz by driving the REFERENCE's own LPIPS class (losses/lpips.py, loaded by file path) through the
arithmetic of the reference's commented object-loss block (losses/loss_img.py:91-106) on CPU
(``MAS_REFERENCE_ROOT=<reference checkout> python tests/golden/make_object_golden.py``).  What the reference needs and cannot have
offline is stubbed, nothing else: ``torchvision.models.vgg16`` (the published VGG16 'D' ``features`` stack, as in
make_lpips_golden.py), the checkpoint download of ``load_from_pretrained`` (skipped; weights: ``synth_lpips_state_dict(3)``, loaded
with ``strict=True``) and torchvision's ``crop`` (zero padding outside the image: tests/helpers/object_ref.py).  The block runs with the
two documented differences (boxes with a side under 16 px skipped and not counted; the gradient taken for ``reconstructions``).
Inputs are regenerated from the seed stored in the file."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import object_ref as R  # noqa: E402
from oracle.lpips_oracle import VGG_CFG, synth_lpips_state_dict  # noqa: E402

REF = os.environ.get("MAS_REFERENCE_ROOT", "")          # a checkout of the reference


def _vgg16(pretrained=False):
    layers, cin = [], 3
    for v in VGG_CFG + ["M"]:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    m = nn.Module()
    m.features = nn.Sequential(*layers)
    return m


def _load_reference_lpips():
    path = os.path.join(REF, "losses", "lpips.py")
    if not os.path.exists(path):
        sys.exit("set MAS_REFERENCE_ROOT to a checkout of the reference Make-A-Scene")
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    tvm.vgg16, tvf.crop = _vgg16, R.tv_crop
    tv.models, tv.transforms, tvt.functional = tvm, tvt, tvf
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    for name in ("requests", "tqdm"):                      # imported by lpips.py for the download it does not do here
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                stub = types.ModuleType(name)
                stub.tqdm = None
                sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("ref_lpips", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
    return mod


def main():
    torch.manual_seed(0)
    ref = _load_reference_lpips()
    from torchvision.transforms.functional import crop   # the stub above
    m = ref.LPIPS().eval()
    m.load_state_dict(synth_lpips_state_dict(seed=3), strict=True)
    images, recs = R.synth_images()
    recs.requires_grad_(True)
    # the reference's block (loss_img.py:91-106), restated with the used boxes
    object_loss = images.new_tensor(0)
    values = []
    for img, rec, bboxes in zip(images, recs, R.BOXES):
        bboxes = R.used(bboxes)
        img_object_loss = img.new_tensor(0)
        for bbox in bboxes:
            top, left, height, width = bbox[1], bbox[0], bbox[3] - bbox[1], bbox[2] - bbox[0]
            crop_img = crop(img, top, left, height, width).unsqueeze(0)
            crop_rec = crop(rec, top, left, height, width).unsqueeze(0)
            v = m(crop_img.contiguous(), crop_rec.contiguous()).mean()
            values.append(float(v.detach()))
            img_object_loss = img_object_loss + v
        object_loss = object_loss + img_object_loss / (len(bboxes) + 1)
    object_loss.backward()
    assert torch.isfinite(recs.grad).all()
    path = os.path.join(HERE, "object_tiny.npz")
    np.savez_compressed(path, loss=object_loss.detach().numpy().astype(np.float32), values=np.array(values, dtype=np.float32),
                        drec=recs.grad.numpy().astype(np.float32),
                        case=np.array(json.dumps(dict(H=R.H, W=R.W, seed=R.SEED, boxes=R.BOXES, lpips_seed=3))))
    print("loss", float(object_loss), "values", values, "|drec|", float(recs.grad.abs().max()), "torch", torch.__version__)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
