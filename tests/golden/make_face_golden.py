#!/usr/bin/env python3
"""Generates tests/golden/face_tiny.npz by running the REFERENCE's own FaceLoss (losses/face_loss.py, loaded by file path) on CPU
(``MAS_REFERENCE_ROOT=<reference checkout> python tests/golden/make_face_golden.py``).  Two things it needs are not available offline and are stubbed, nothing else:
``torchvision.transforms`` (``Resize``, ``CenterCrop`` and ``functional.crop``: the restatement in tests/helpers/face_ref.py) and the
checkpoint ``torch.load`` of the constructor, which returns ``face_ref.synth_face_state_dict(0)``; ``load_state_dict(strict=True)``
is asserted afterwards (= proof of the key layout and shapes).  Inputs are regenerated from the seeds stored in the file."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import face_ref as R  # noqa: E402

REF = os.environ.get("MAS_REFERENCE_ROOT", "")          # a checkout of the reference

# (name, images, H, W, seed, boxes per image)
CASES = [
    ("n1_portrait", 1, 48, 64, 11, [[[8, 6, 40, 46]]]),
    # an edge-crossing box (left and bottom), a landscape box, and a 300 x 300 box: Resize(256) DOWNscales it (antialias matters)
    ("n3_edge_land_down", 2, 56, 64, 12, [[[-6, 30, 20, 60], [10, 4, 50, 24]], [[-130, -120, 170, 180]]]),
    # overlapping boxes in image 0 (their rec crops are the two rows that reach rec); rows [gt0, gt1, gt2, gt3, rec0, rec1]
    ("n4_overlap", 2, 48, 56, 13, [[[5, 5, 35, 40], [15, 10, 45, 45]], [[0, 0, 30, 20], [20, 15, 56, 48]]]),
    # seven faces: faces[:6] keeps gt faces only, nothing reaches rec
    ("n7_all_gt", 3, 40, 40, 14, [[[0, 0, 20, 20], [5, 5, 30, 25], [10, 2, 38, 36]], [[2, 3, 22, 33], [12, 0, 40, 24]],
                                  [[0, 10, 40, 30], [6, 6, 26, 26]]]),
]


class _Resize(nn.Module):
    def __init__(self, size):
        super().__init__()
        self.size = size

    def forward(self, x):
        return R.tv_resize(x, self.size)


class _CenterCrop(nn.Module):
    def __init__(self, size):
        super().__init__()
        self.size = size

    def forward(self, x):
        return R.tv_center_crop(x, self.size)


def _load_reference():
    if not os.path.exists(os.path.join(REF, "losses", "face_loss.py")):
        sys.exit("set MAS_REFERENCE_ROOT to a checkout of the reference Make-A-Scene")
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    tvt.Resize, tvt.CenterCrop, tvf.crop = _Resize, _CenterCrop, R.tv_crop
    tvt.functional, tv.transforms = tvf, tvt
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    spec = importlib.util.spec_from_file_location("ref_face_loss", os.path.join(REF, "losses", "face_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    torch.manual_seed(0)
    ref = _load_reference()
    sd = R.synth_face_state_dict(0)
    real_load = torch.load
    torch.load = lambda *a, **k: sd                  # the constructor's checkpoint (face_loss.py:76)
    try:
        m = ref.FaceLoss()
    finally:
        torch.load = real_load
    m.load_state_dict(sd, strict=True)
    assert not m.training
    keys = list(m.state_dict().keys())
    assert keys == list(R.expected_shapes().keys())
    n_params = sum(p.numel() for p in m.parameters())
    out = {"keys": np.array(keys), "n_params": np.array(n_params)}
    meta = []
    for name, n_img, h, w, seed, boxes in CASES:
        img, rec = R.synth_images(n_img, h, w, seed)
        rec.requires_grad_(True)
        loss = m(img, rec, boxes)
        loss.backward()
        faces = m.prepare_faces(img, rec.detach(), boxes)
        with torch.no_grad():
            feats = [f.chunk(2) for f in m._forward(faces[:6])]
            diffs = torch.stack([a * torch.abs(p[0] - p[1]).sum(dim=0).mean() for a, p in zip(m.alphas, feats)])
        assert torch.allclose(diffs.sum(), loss.detach(), rtol=1e-5)
        out[name + "/loss"] = loss.detach().numpy().astype(np.float32)
        out[name + "/diffs"] = diffs.numpy().astype(np.float32)
        out[name + "/drec"] = rec.grad.numpy().astype(np.float32)
        meta.append(dict(name=name, images=n_img, H=h, W=w, seed=seed, boxes=boxes))
        print(f"{name}: loss {loss.item():.6f} diffs {diffs.numpy()} |drec| {rec.grad.abs().max().item():.3e}")
    out["cases"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "face_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
