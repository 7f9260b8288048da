"""The face rows as six fixed slots of a device table (mas_hip.face.slots / pack_slots / FaceTable), without a GPU: the planner against a
direct restatement of the reference's ``cat([gt], [rec])[:6]`` + ``chunk(2)``, the host checks, the packed bytes, and the argument
checks of the four ``*_dev`` entry points."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import face_ref as R  # noqa: E402

BOX = [2, 3, 22, 33]


def _boxes(n, images):
    """n faces spread over ``images`` images (round robin), every box different"""
    out = [[] for _ in range(images)]
    for i in range(n):
        out[i % images].append([i, 2 * i, 20 + 3 * i, 30 + i])
    return out


def _restated(n):
    """cat([gt faces], [rec faces])[:6], chunk(2): -> (pairs [(row, row)], rows) with rows as (src, face)"""
    rows = ([(0, i) for i in range(n)] + [(1, i) for i in range(n)])[:6]
    half = len(rows) // 2
    return [(rows[q], rows[half + q]) for q in range(half)], rows


@pytest.mark.parametrize("images", [2, 3])
@pytest.mark.parametrize("n", range(9))
def test_slots_agree_with_the_reference_pairing(n, images):
    from mas_hip import face as F
    boxes = _boxes(n, images)
    order = F.face_list(boxes, images)                          # (image, box) per face, the reference's order
    got_n, recs = F.slots(boxes, images)
    pairs, rows = _restated(n)
    assert got_n == n and len(recs) == 6
    want = [None] * 6
    for q, (a, b) in enumerate(pairs):
        want[q], want[3 + q] = a, b
    ident = lambda r: None if r is None else (r.src, next(i for i, (b, box) in enumerate(order) if b == r.b and box[1] == r.top and box[0] == r.left))
    assert [ident(r) for r in recs] == want                     # which (src, face) sits in which slot
    t = F.pack_slots(recs, images)
    assert t.n_pairs == len(pairs) == min(n, 3)
    assert [bool(v) for v in t.valid] == [w is not None for w in want]
    rec_slots = [s for s, r in enumerate(recs) if r is not None and r.src == 1]
    assert rec_slots == [3 + q for q, (_, b) in enumerate(pairs) if b[0] == 1] and all(s >= 3 for s in rec_slots)
    assert len(rec_slots) == sum(r[0] == 1 for r in rows)       # every surviving rec row, and only in slots 3..5
    if n == 4:
        assert want == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1)]          # (gt0, gt3), (gt1, rec0), (gt2, rec1)
    if n >= 6:
        assert rec_slots == [] and t.n_pairs == 3
    # the geometry is plan()'s
    _, planned = F.plan(boxes, images)
    half = len(planned) // 2
    for q in range(half):
        assert bytes(recs[q]) == bytes(planned[q]) and bytes(recs[3 + q]) == bytes(planned[half + q])


def test_bad_boxes_raise_before_anything_is_written():
    from mas_hip import face as F
    table = F.FaceTable("cpu")
    assert table.write([[BOX], []], 2) == 1
    before = table.dev.clone()
    with pytest.raises(ValueError, match="no area"):
        table.write([[BOX, [5, 5, 5, 20]], []], 2)              # a box without area, as face_geometry refuses it
    with pytest.raises(ValueError, match="no area"):
        F.slots([[], [[9, 9, 3, 12]]], 2)
    assert torch.equal(table.dev, before) and table.n_faces == 1
    _, recs = F.slots([[BOX], [BOX]], 2)
    with pytest.raises(ValueError, match="image 1 of a batch of 1"):
        F.pack_slots(recs, 1)                                   # b >= N
    bad = list(recs)
    bad[3] = F.FaceRow(1, 0, 0, 0, 10, 10, 256, 256, 3, 1)      # centre crop leaves the resized image
    with pytest.raises(ValueError, match="geometry"):
        F.pack_slots(bad, 2)
    with pytest.raises(ValueError, match="pairs"):
        F.pack_slots([recs[0], None, None, None, None, None], 2)
    assert torch.equal(table.dev, before)
    assert table.write(None, 2) == 0 and not table.dev.any()    # no faces: every slot empty, all bytes zero


def test_packed_bytes_round_trip_through_the_struct():
    import mas_hip
    from mas_hip import face as F
    assert ctypes.sizeof(F.FaceSlots) == 6 * 40 + 6 * 4 + 8 == 4 * mas_hip.FACE_TABLE_INTS == F.FaceTable.NBYTES and mas_hip.FACE_SLOTS == F.SLOTS == 6
    boxes = _boxes(4, 2)
    table = F.FaceTable("cpu")
    assert table.write(boxes, 2) == 4 and table.n_images == 2
    back = F.FaceSlots.from_buffer_copy(bytes(table.dev.numpy().tobytes()))
    _, recs = F.slots(boxes, 2)
    assert back.n_pairs == 3 and list(back.valid) == [1] * 6 and back.pad_ == 0
    fields = [n for n, _ in mas_hip.FaceRow._fields_]
    for s in range(6):
        assert [getattr(back.row[s], f) for f in fields] == [getattr(recs[s], f) for f in fields]
    assert table.write(_boxes(1, 2), 2) == 1                    # the second pinned buffer; nothing of the four faces survives
    back = F.FaceSlots.from_buffer_copy(bytes(table.dev.numpy().tobytes()))
    assert back.n_pairs == 1 and list(back.valid) == [1, 0, 0, 1, 0, 0]
    assert all(getattr(back.row[s], f) == 0 for s in (1, 2, 4, 5) for f in fields)
    assert (back.row[0].src, back.row[3].src) == (0, 1)


def test_header_declares_the_dev_entries_inside_the_abi():
    import mas_hip
    V, I, FP, IP = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(mas_hip.FaceFeats), ctypes.POINTER(mas_hip.FaceImage)
    sig = mas_hip._SIGNATURES
    assert sig["mas_face_crop_fwd_dev"] == (I, [IP, IP, V, V, I, V])
    assert sig["mas_face_l1_fwd_dev"] == (I, [FP, V, V, V, V])
    assert sig["mas_face_l1_bwd_dev"] == (I, [FP, V, V, ctypes.POINTER(V), V])
    assert sig["mas_face_crop_bwd_dev"] == (I, [V, V, IP, V])
    assert mas_hip.lib().mas_abi_version() == mas_hip.ABI_VERSION


def test_dev_entries_reject_bad_arguments_without_gpu():
    import mas_hip
    L = mas_hip.lib()
    P = ctypes.c_void_p
    img = mas_hip.FaceImage(1, 0, 1, 3, 32, 32, 0, 3072, 1024, 32, 1)
    assert L.mas_face_crop_fwd_dev(ctypes.byref(img), ctypes.byref(img), None, P(1), 0, None) == -1 and b"null" in L.mas_last_error()
    assert L.mas_face_crop_fwd_dev(ctypes.byref(img), ctypes.byref(img), P(1), P(1), 7, None) == -1
    assert L.mas_face_crop_bwd_dev(P(1), None, ctypes.byref(img), None) == -1
    assert L.mas_face_crop_bwd_dev(None, P(1), ctypes.byref(img), None) == -1
    f = mas_hip.FaceFeats()
    for i, chw in enumerate((64 * 127 * 127, 256 * 63 * 63, 512 * 32 * 32, 1024 * 16 * 16, 2048 * 8 * 8)):
        f.p[i], f.chw[i] = 1, chw
    f.half, f.dtype = 2, 1
    seeds = (ctypes.c_void_p * 5)(*([1] * 5))
    assert L.mas_face_l1_fwd_dev(ctypes.byref(f), P(1), P(1), P(1), None) == -1 and b"capacity" in L.mas_last_error()     # half must be 3
    assert L.mas_face_l1_bwd_dev(ctypes.byref(f), P(1), P(1), seeds, None) == -1
    f.half = 3
    assert L.mas_face_l1_fwd_dev(ctypes.byref(f), None, P(1), P(1), None) == -1
    assert L.mas_face_l1_bwd_dev(ctypes.byref(f), P(1), None, seeds, None) == -1
    seeds[2] = None
    assert L.mas_face_l1_bwd_dev(ctypes.byref(f), P(1), P(1), seeds, None) == -1 and b"seed 2" in L.mas_last_error()


def test_table_path_refuses_training_mode_and_cpu(tmp_path, monkeypatch):
    from mas_hip import face as F
    p = tmp_path / "face_synth.pt"
    torch.save(R.synth_face_state_dict(0), p)
    monkeypatch.setenv("MAS_FACE_CKPT", str(p))
    from losses.face_loss import FaceLoss
    m = FaceLoss()
    img, rec = R.synth_images(1, 32, 32, 0)
    table = F.FaceTable("cpu")
    table.write([[[0, 0, 20, 20]]], 1)
    with pytest.raises(RuntimeError, match="GPU"):
        m(img, rec, table)                                      # no CPU fallback
    with pytest.raises(RuntimeError, match="evaluation-mode"):
        m.train()(img, rec, table)
