"""The reference's one-hot construction of the VQ-SEG map, restated (Data/dataset_preprocessor.py:62-86; its dataset class needs cv2,
albumentations and hydra to import).  Per image it holds: ``seg_panoptic`` and ``seg_human`` integer label images with -1 for "none",
``seg_face`` with 0 for "none", and an edge image beside the first two.

    :62-64  panoptic: one_hot(seg_panoptic + 1, 134) without its first channel  -> 133 channels
    :69-71  human:    one_hot(seg_human + 1, 21) without its first channel      -> 20 channels
    :75     edges:    (edges_panoptic + edges_human) as float                   -> 1 channel
    :78-80  face:     one_hot(seg_face, 6) without its first channel            -> 5 channels
    :84-86  the map:  cat([panoptic, human, face, edges], -1)                   -> [H, W, 159]

What ``seg_data.planes_from_arrays`` + ``SegLabels.dense()`` are checked against, and the sample the tests share."""
import numpy as np
import torch
import torch.nn.functional as F


def reference_seg_map(seg_panoptic, edges_panoptic, seg_human, edges_human, seg_face):
    """-> float32 [H, W, 159], channels last as the reference's dataset returns it"""
    lab = lambda a: torch.from_numpy(np.asarray(a)).to(torch.long)
    pan = F.one_hot(lab(seg_panoptic) + 1, num_classes=134)[..., 1:]
    hum = F.one_hot(lab(seg_human) + 1, num_classes=21)[..., 1:]
    edges = (torch.from_numpy(np.asarray(edges_panoptic)).unsqueeze(-1) + torch.from_numpy(np.asarray(edges_human)).unsqueeze(-1)).float()
    face = F.one_hot(lab(seg_face), num_classes=6)[..., 1:]
    return torch.cat([pan, hum, face, edges], dim=-1).float()


def sample_arrays(h, w, seed=0, empty_plane=None):
    """seeded random arrays as the reference stores them; holds "none" pixels, each group's largest class and edge value 2 (from 2 x 2
    pixels on); ``empty_plane`` in {"panoptic", "human", "face"}: that plane is "none" everywhere"""
    rs = np.random.RandomState(seed)
    pan = rs.randint(-1, 133, (h, w)).astype(np.int64)
    hum = np.where(rs.rand(h, w) < 0.5, -1, rs.randint(0, 20, (h, w))).astype(np.int64)
    face = np.where(rs.rand(h, w) < 0.7, 0, rs.randint(1, 6, (h, w))).astype(np.int64)
    ep = (rs.rand(h, w) < 0.3).astype(np.uint8)
    eh = (rs.rand(h, w) < 0.3).astype(np.uint8)
    flat = lambda a: a.reshape(-1)
    if h * w >= 4:
        flat(pan)[0], flat(hum)[1], flat(face)[2] = 132, 19, 5
        flat(pan)[3], flat(hum)[3], flat(face)[3] = -1, -1, 0
        flat(ep)[1] = flat(eh)[1] = 1
    if empty_plane == "panoptic":
        pan[:] = -1
    elif empty_plane == "human":
        hum[:] = -1
    elif empty_plane == "face":
        face[:] = 0
    return pan, ep, hum, eh, face
