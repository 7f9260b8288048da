"""CPU side of the compact VQ-SEG input (``mas_hip.seglabels``, ``seg_data``, csrc/seg_labels.hip's entry points): the label planes stand
for exactly the map the reference's dataset builds (tests/helpers/seg_labels_ref.py restates Data/dataset_preprocessor.py:62-86), the
wrapper behaves like the tensor train.py moves around, and header, exports and binding agree on the four new entry points at ABI 10."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"),):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import seg_labels_ref as LR  # noqa: E402
import seg_data  # noqa: E402
from mas_hip.seglabels import SegLabels, SegLayout  # noqa: E402

ENTRY_POINTS = ("mas_seg_expand", "mas_seg_loss_labels_blocks", "mas_seg_loss_labels_fwd", "mas_seg_loss_labels_bwd")


def test_default_layout_is_the_reference_channel_order():
    lay = SegLayout()
    assert lay.groups == (133, 20, 5) and lay.value_channels == 1 and lay.planes == 4 and lay.channels == 159
    assert lay.bases == (0, 133, 153, 158)
    assert SegLayout(groups=(3, 2)).channels == 6 and SegLayout(groups=(5, 2)).bases == (0, 5, 7)
    for bad in (dict(groups=(1,) * 8), dict(groups=(256,)), dict(groups=(0, 3)), dict(groups=(), value_channels=0)):
        with pytest.raises(ValueError, match="SegLayout"):
            SegLayout(**bad)


@pytest.mark.parametrize("empty", [None, "panoptic", "human", "face"])
def test_planes_densify_to_the_reference_map(empty):
    arrays = LR.sample_arrays(9, 13, seed=11, empty_plane=empty)
    pan, ep, hum, eh, face = arrays
    if empty is None:                                            # the sample holds what it is meant to hold
        assert pan.max() == 132 and hum.max() == 19 and face.max() == 5 and (ep + eh).max() == 2
        assert (pan == -1).any() and (hum == -1).any() and (face == 0).any()
    ref = LR.reference_seg_map(*arrays)                          # [H, W, 159]
    planes = seg_data.planes_from_arrays(*arrays)
    assert planes.dtype == torch.uint8 and tuple(planes.shape) == (4, 9, 13)
    labels = seg_data.collate([planes])
    dense = labels.dense()
    assert dense.dtype == torch.float32 and tuple(dense.shape) == (1, 159, 9, 13) and dense.is_contiguous()
    assert torch.equal(dense[0].permute(1, 2, 0), ref)
    assert set(np.unique(dense.numpy())) <= {0.0, 1.0, 2.0} and float(dense[0, 158].max()) == 2.0
    cl = labels.dense(torch.bfloat16, memory_format=torch.channels_last)
    assert cl.dtype == torch.bfloat16 and cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(cl.float(), dense)
    if empty is not None:
        k = {"panoptic": (0, 133), "human": (133, 153), "face": (153, 158)}[empty]
        assert float(dense[0, k[0]:k[1]].abs().sum()) == 0.0


def test_labels_above_the_group_size_set_nothing():
    planes = torch.zeros(1, 4, 2, 2, dtype=torch.uint8)
    planes[0, 2, 0, 0] = 200                                     # face plane: 5 classes
    planes[0, 0, 1, 1] = 134                                     # panoptic plane: 133 classes
    planes[0, 1, 0, 1] = 20                                      # the largest human class
    dense = SegLabels(planes).dense()
    assert float(dense.sum()) == 1.0 and float(dense[0, 152, 0, 1]) == 1.0


def test_planes_from_arrays_refuses_what_it_cannot_represent():
    pan, ep, hum, eh, face = LR.sample_arrays(4, 5, seed=2)
    bad = pan.copy()
    bad[1, 1] = 133
    with pytest.raises(ValueError, match="seg_panoptic"):
        seg_data.planes_from_arrays(bad, ep, hum, eh, face)
    with pytest.raises(ValueError, match="edges_panoptic"):
        seg_data.planes_from_arrays(pan, ep.astype(np.float32) + 0.5, hum, eh, face)
    with pytest.raises(ValueError, match="seg_human"):
        seg_data.planes_from_arrays(pan, ep, np.where(hum < 0, -2, hum), eh, face)
    with pytest.raises(ValueError, match="seg_face"):
        seg_data.planes_from_arrays(pan, ep, hum, eh, face + 6)
    ok = seg_data.planes_from_arrays(pan.astype(np.float64), torch.from_numpy(ep), hum.astype(np.int16), eh, face)   # integer-valued floats pass
    assert torch.equal(ok, seg_data.planes_from_arrays(pan, ep, hum, eh, face))


def test_collate_to_indexing_and_shape():
    samples = [seg_data.planes_from_arrays(*LR.sample_arrays(6, 8, seed=s)) for s in range(3)]
    batch = seg_data.collate(samples)
    assert isinstance(batch, SegLabels) and len(batch) == 3 and batch.shape == torch.Size((3, 159, 6, 8)) and batch.dim() == 4
    assert batch.size(1) == 159 and tuple(batch.planes.shape) == (3, 4, 6, 8) and batch.planes.dtype == torch.uint8
    assert batch.device == torch.device("cpu") and not batch.is_cuda
    one = batch[1]
    assert isinstance(one, SegLabels) and len(one) == 1 and torch.equal(one.planes[0], samples[1])
    assert torch.equal(batch[-1].planes[0], samples[2]) and len(batch[1:]) == 2 and torch.equal(batch[1:].planes, batch.planes[1:])
    assert torch.equal(batch[1:].dense(), batch.dense()[1:])
    with pytest.raises(IndexError):
        batch[3]
    moved = batch.to(torch.device("cpu"))
    assert isinstance(moved, SegLabels) and moved.layout == batch.layout and torch.equal(moved.planes, batch.planes)
    assert isinstance(batch.to("cpu", non_blocking=True), SegLabels)
    with pytest.raises(TypeError, match="uint8"):
        batch.to(torch.float32)
    assert seg_data.collate([batch[0], batch[1]]).shape[0] == 2
    with pytest.raises(ValueError, match="collate"):
        seg_data.collate([samples[0].float()])
    with pytest.raises(ValueError, match="SegLabels"):
        SegLabels(torch.zeros(1, 3, 2, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="SegLabels"):
        SegLabels(torch.zeros(1, 4, 2, 2))


def test_ops_refuse_cpu_labels_and_name_themselves():
    from mas_hip import ops
    labels = seg_data.collate([seg_data.planes_from_arrays(*LR.sample_arrays(4, 4, seed=1))])
    with pytest.raises(RuntimeError, match="seg_expand"):
        ops.seg_expand(labels, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="seg_loss_labels"):
        ops.seg_loss_labels(torch.zeros(1, 159, 4, 4), labels, torch.ones(159))
    with pytest.raises(ValueError, match="seg_loss_labels"):
        ops.seg_loss_labels(torch.zeros(1, 158, 4, 4), labels, torch.ones(158))      # the layout's C does not match the prediction
    with pytest.raises(TypeError, match="seg_loss_labels"):
        ops.seg_loss_labels(torch.zeros(1, 159, 4, 4), labels.dense(), torch.ones(159))


def test_loss_classes_on_cpu_labels_run_the_torch_expression(monkeypatch):
    import losses
    from mas_hip import ops
    monkeypatch.delenv("MAS_SEG_LOSS", raising=False)
    monkeypatch.setattr(ops, "seg_loss_labels", lambda *a, **k: pytest.fail("ops.seg_loss_labels called for CPU labels"))
    labels = seg_data.collate([seg_data.planes_from_arrays(*LR.sample_arrays(5, 6, seed=s)) for s in (4, 5)])
    pred = torch.randn(2, 159, 5, 6, generator=torch.Generator().manual_seed(0))
    q = torch.tensor(0.25)
    for name in ("BCELossWithQuant", "VQVAEWithBCELoss"):
        m = getattr(losses, name)(image_channels=159, codebook_weight=0.5)
        assert list(m.state_dict()) == ["weight"]
        assert torch.equal(m(q, labels, pred), m(q, labels.dense(), pred))
    with pytest.raises(ValueError, match="SegLabels"):
        losses.BCELossWithQuant(image_channels=159)(q, labels, pred[:, :158])


def test_entry_points_in_header_exports_and_binding():
    import mas_hip
    txt = open(os.path.join(ROOT, "include", "mas_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in mas_hip.EXPORTS
    assert re.search(r"MAS_SEG_LABELS_TILE\s*=\s*%d\b" % mas_hip.SEG_LABELS_TILE, code)
    assert re.search(r"MAS_SEG_MAX_PLANES\s*=\s*%d\b" % mas_hip.SEG_MAX_PLANES, code)
    L = mas_hip.lib()
    assert L.mas_abi_version() == mas_hip.ABI_VERSION == 10
    raw = ctypes.CDLL(mas_hip.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), name


def test_entry_points_validate_arguments_without_gpu():
    import mas_hip
    L = mas_hip.lib()
    g = (ctypes.c_int * 3)(133, 20, 5)
    tile = mas_hip.SEG_LABELS_TILE
    # the grid: one work-group per tile of `tile` pixels of one image, up to eight per CU
    assert L.mas_seg_loss_labels_blocks(g, 3, 1, 2, 8, 8, mas_hip.F32, mas_hip.SEG_NCHW) == 2
    assert L.mas_seg_loss_labels_blocks(g, 3, 1, 3, 1, tile + 1, mas_hip.BF16, mas_hip.SEG_NHWC) == 6
    assert L.mas_seg_loss_labels_blocks(g, 3, 1, 0, 8, 8, mas_hip.F32, mas_hip.SEG_NCHW) == -1 and b"seg_loss_labels" in L.mas_last_error()
    assert L.mas_seg_loss_labels_blocks(g, 3, 6, 1, 8, 8, mas_hip.F32, mas_hip.SEG_NCHW) == -1      # nine planes
    assert L.mas_seg_loss_labels_blocks((ctypes.c_int * 1)(256), 1, 0, 1, 8, 8, mas_hip.F32, mas_hip.SEG_NCHW) == -1
    assert L.mas_seg_loss_labels_blocks(g, 3, 1, 1, 8, 8, 7, mas_hip.SEG_NCHW) == -2
    assert L.mas_seg_loss_labels_blocks(g, 3, 1, 1, 8, 8, mas_hip.F32, 5) == -1
    assert L.mas_seg_loss_labels_fwd(None, mas_hip.F32, 0, None, g, 3, 1, None, 2, 8, 8, 1, None, 0, None) == -1 and b"null" in L.mas_last_error()
    assert L.mas_seg_loss_labels_bwd(None, mas_hip.F32, 0, None, g, 3, 1, None, 2, 8, 8, 1, None, None, None) == -1
    assert L.mas_seg_expand(None, g, 3, 1, 2, 8, 8, None, mas_hip.BF16, mas_hip.SEG_NHWC, 160, None) == -1 and b"null" in L.mas_last_error()
    assert L.mas_seg_expand(None, g, 3, 1, 2, 8, 8, None, mas_hip.BF16, mas_hip.SEG_NHWC, 158, None) == -1 and b"C_pad" in L.mas_last_error()
