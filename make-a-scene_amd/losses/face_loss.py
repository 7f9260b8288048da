"""Face-embedding loss (reference losses/face_loss.py): the face-aware term of the VQ-IMG objective ("face-aware vector quantisation").

Same import path, constructor (no arguments), attributes (``alphas``, ``channels``), methods (``_forward``, ``prepare_faces``,
``forward``) and ``state_dict`` keys as the reference: a frozen VGGFace2 ResNet-50 (caffe-style Bottlenecks: the stride on the first
1x1) built from ``nn.Conv2d`` / ``nn.BatchNorm2d`` children, so a checkpoint saved from the reference loads.

``forward(img, rec, bbox)`` in evaluation mode (the reference's constructor calls ``self.eval()``) is ONE autograd node on libmas_hip
(``mas_hip.face``): the face crops, the stem, bn1 + ReLU + max-pool, the Bottleneck joins and the feature L1 distances on
csrc/face.hip, the 52 1x1 / 3x3 convolutions on the library's convolution kernels, forward and data gradient -- bitwise reproducible,
no ATen kernel on an activation map.  Its backward reaches ``rec`` only (the parameters are frozen and ``img`` is data).
The reference's row selection is reproduced exactly: ``cat([gt faces], [rec faces])[:6]``, pairs (q, half + q) -- with n = 4 faces
the pairs are (gt0, gt3), (gt1, rec0), (gt2, rec1), and with n >= 6 no rec face takes part.

``forward(img, rec, table)`` with a ``mas_hip.face.FaceTable`` instead of the box lists is the same term at fixed capacity (six rows,
whatever the table holds): the node a captured graph replays (``mas_hip.graphs.GraphedGanStep``).  Evaluation mode only.

``train()`` (training-mode BatchNorm, outside the envelope): the reference's arithmetic on the torch modules, fed by the HIP crop.

Weights: ``MAS_FACE_CKPT``, or the reference's path if that file exists; loaded with ``strict=False`` as the reference does (extra
``fc.*`` keys are fine).  Tensors still at their random initialisation afterwards are named in a ``RuntimeError``
(``MAS_FACE_STRICT=0``: a warning)."""
import os
import warnings

import torch
import torch.nn as nn

REFERENCE_CKPT = "/home/ubuntu/Make-A-Scene/losses/face_loss_weights.pt"      # face_loss.py:76


def ckpt_path():
    """The checkpoint FaceLoss() loads: ``MAS_FACE_CKPT`` if set and present, else the reference's path if present, else None."""
    for p in (os.environ.get("MAS_FACE_CKPT", ""), REFERENCE_CKPT):
        if p and os.path.exists(p):
            return p
    return None


def conv3x3(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=stride, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        residual = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            residual = self.downsample(x)
        out += residual
        return self.relu(out)


class FaceLoss(nn.Module):
    _warned = False

    def __init__(self):
        super().__init__()
        layers = [3, 4, 6, 3]
        self.inplanes = 64
        self.alphas = [0.1, 0.25 * 0.01, 0.25 * 0.1, 0.25 * 0.2, 0.25 * 0.02]
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=0, ceil_mode=True)
        self.layer1 = self._make_layer(Bottleneck, 64, layers[0])
        self.layer2 = self._make_layer(Bottleneck, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(Bottleneck, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(Bottleneck, 512, layers[3], stride=2)
        self.channels = [64, 256, 512, 1024, 2048]
        self.load_from_pretrained()
        for param in self.parameters():
            param.requires_grad = False
        self.eval()

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def load_from_pretrained(self):
        """``MAS_FACE_CKPT`` (or the reference's ``face_loss_weights.pt``), ``strict=False`` as the reference loads it.  Every
        tensor it leaves at its initialisation is listed in ``self.unloaded`` and reported: an error by default (the reference's
        constructor cannot run without the file), a warning with ``MAS_FACE_STRICT=0``."""
        want = [k for k in self.state_dict().keys() if not k.endswith("num_batches_tracked")]
        loaded = set()
        path = ckpt_path()
        if path is not None:
            res = self.load_state_dict(torch.load(path, map_location="cpu"), strict=False)
            loaded = set(want) - set(res.missing_keys)
        self.unloaded = [k for k in want if k not in loaded]
        if not self.unloaded:
            return
        msg = ("FaceLoss: %d of %d tensors keep their RANDOM initialisation (no face-embedding weights: set MAS_FACE_CKPT to a state_dict "
               "of the reference's FaceLoss, e.g. face_loss_weights.pt); the face term is NOT a face distance until they are loaded.  "
               "Missing: %s" % (len(self.unloaded), len(want), ", ".join(self.unloaded[:6]) + (" ..." if len(self.unloaded) > 6 else "")))
        if os.environ.get("MAS_FACE_STRICT", "1") == "1":
            raise RuntimeError(msg + "  (MAS_FACE_STRICT=0 downgrades this to a warning: tests, arithmetic checks with synthetic weights)")
        if loaded or not FaceLoss._warned:
            FaceLoss._warned = True
            warnings.warn(msg)

    def _forward(self, x):
        """The reference's network arithmetic on the torch modules (face_loss.py:95-113): the training-mode path, and a readable
        statement of what the HIP path computes."""
        features = []
        x = self.conv1(x)
        features.append(x)
        x = self.maxpool(self.relu(self.bn1(x)))
        x = self.layer1(x)
        features.append(x)
        x = self.layer2(x)
        features.append(x)
        x = self.layer3(x)
        features.append(x)
        x = self.layer4(x)
        features.append(x)
        return features

    def forward(self, img, rec, bbox):
        """sum_i alpha_i * |f_i(p0) - f_i(p1)|.sum(0).mean() over the reference's row pairs; ``img.new_tensor(0)`` without faces.
        ``self.last_diffs``: the five weighted terms of the last evaluation-mode call (None without faces)."""
        from mas_hip import face as F
        if isinstance(bbox, F.FaceTable):
            # the boxes in a device table: the fixed-capacity node, which runs whatever the table holds and reads nothing on the host
            if self.training:
                raise RuntimeError("FaceLoss: a FaceTable belongs to the evaluation-mode HIP path (training-mode BatchNorm runs on the torch "
                                   "modules, from host box lists)")
            out = F.face_loss_static(self, img, rec, bbox)
            self.last_diffs = out[:5]
            return out[5]
        if self.training:
            return self._forward_train(img, rec, bbox)
        out = F.face_loss(self, img, rec, bbox)
        self.last_diffs = out[:5] if out is not None else None
        if out is None:
            return img.new_tensor(0)
        return out[5]

    def _forward_train(self, img, rec, bbox):
        from mas_hip import face as F
        from mas_hip import ops
        ops._require_cuda(img, "FaceLoss")
        n, rows = F.plan(bbox, min(img.shape[0], rec.shape[0]))
        if n == 0:
            return img.new_tensor(0)
        faces = F.FaceCrop.apply(img, rec, rows, torch.float32)
        features = [f.chunk(2) for f in self._forward(faces)]
        diffs = [a * torch.abs(p[0] - p[1]).sum(dim=0).mean() for a, p in zip(self.alphas, features)]
        return sum(diffs)

    def prepare_faces(self, imgs, recs, bboxes):
        """``cat([gt faces], [rec faces])`` [2n, 3, 254, 254] (channels_last, the compute dtype; differentiable), or None without faces
        -- every face, as the reference returns them before its ``[:6]``."""
        from mas_hip import face as F
        from mas_hip import ops
        ops._require_cuda(imgs, "FaceLoss")
        faces = F.face_list(bboxes, min(imgs.shape[0], recs.shape[0]))
        if not faces:
            return None
        rows = []
        for src in (0, 1):
            for b, box in faces:
                g = F.face_geometry(box)
                rows.append(F.FaceRow(src, b, g["top"], g["left"], g["h"], g["w"], g["rh"], g["rw"], g["ct"], g["cl"]))
        chunks = [F.FaceCrop.apply(imgs, recs, rows[i:i + F.MAX_ROWS], ops.compute_dtype()) for i in range(0, len(rows), F.MAX_ROWS)]
        return torch.cat(chunks, dim=0) if len(chunks) > 1 else chunks[0]
