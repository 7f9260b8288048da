"""The fixed-capacity FaceLoss node (mas_hip.face._FaceLossStatic: the rows in a device table, six rows forward, the slice [3:6]
backward; csrc/face.hip ``*_dev``) on the MI355X, against the golden the reference's own module wrote (tests/golden/face_tiny.npz), and
against the list path of the same module.

Tolerances are test_gpu_face_loss.py's: the whole loss in fp32 parity mode within 1e-3 relative; in bf16 within 1.2x
the deviation of the CPU restatement under autocast(bfloat16), d rec cosine >= 0.98.  The reference is the golden, not the list path;
against the list path the same 1e-3 is asserted and whether the bits were equal is printed."""
import json
import os
import sys

import numpy as np
import pytest
import torch

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


def _case(golden, name):
    z, cases = golden
    c = next(c for c in cases if c["name"] == name)
    img, rec = R.synth_images(c["images"], c["H"], c["W"], c["seed"])
    return c, img, rec, z[name + "/loss"], z[name + "/diffs"], z[name + "/drec"]


def _run(mod, img, rec, bbox):
    """forward + backward on lists or on a table -> (loss, last_diffs, d rec), detached copies"""
    r = rec.to(DEV).requires_grad_(True)
    loss = mod(img.to(DEV), r, bbox)
    loss.backward()
    return loss.detach().clone(), mod.last_diffs.detach().clone(), r.grad.clone()


def _table(c):
    from mas_hip import face as FH
    t = FH.FaceTable(DEV)
    assert t.write(c["boxes"], c["images"]) == sum(len(b) for b in c["boxes"][:c["images"]])
    return t


@pytest.mark.parametrize("name", ["n1_portrait", "n3_edge_land_down", "n4_overlap", "n7_all_gt"])
def test_static_node_fp32_matches_golden_and_the_list_path(golden, face_module, name):
    from mas_hip import ops
    ops.set_compute_dtype(torch.float32)                          # (conftest puts the process's dtype back after every test)
    c, img, rec, loss_g, diffs_g, drec_g = _case(golden, name)
    loss, diffs, drec = _run(face_module, img, rec, _table(c))
    dg = torch.from_numpy(drec_g)
    print(f"{name}: loss {float(loss):.8g} (golden {float(loss_g):.8g}), diffs rel {_rel(diffs, torch.from_numpy(diffs_g)):.3g}, "
          f"d rec rel {_rel(drec, dg) if name != 'n7_all_gt' else 0.0:.3g}")
    assert abs(float(loss) - float(loss_g)) <= 1e-3 * abs(float(loss_g))
    assert _rel(diffs, torch.from_numpy(diffs_g)) < 1e-3
    if name == "n7_all_gt":
        assert torch.count_nonzero(drec) == 0
    else:
        assert _rel(drec, dg) < 1e-3, _rel(drec, dg)
    l2, d2, g2 = _run(face_module, img, rec, c["boxes"])          # the list path: 2 * min(n, 3) rows forward, the rec rows backward
    equal = torch.equal(loss, l2) and torch.equal(diffs, d2) and torch.equal(drec, g2)
    print(f"{name}: static node against the list path, fp32: bits {'EQUAL' if equal else 'DIFFER'} "
          f"(loss {abs(float(loss) - float(l2)):.3g}, d rec max {float((drec - g2).abs().max()):.3g})")
    assert abs(float(loss) - float(l2)) <= 1e-3 * abs(float(l2)) and _rel(diffs, d2) < 1e-3
    assert torch.count_nonzero(g2) == 0 if name == "n7_all_gt" else _rel(drec, g2) < 1e-3


@pytest.mark.parametrize("name", ["n1_portrait", "n3_edge_land_down", "n4_overlap"])
def test_static_node_bf16_within_autocast_deviation(golden, face_module, name):
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
    loss, diffs, drec = _run(face_module, img, rec, _table(c))
    print(f"{name} bf16: |loss - golden| {abs(float(loss) - float(loss_g)):.4g} (restatement {dev_loss:.4g}), "
          f"max |d rec - golden| {float((drec.cpu() - dg).abs().max()):.4g} (restatement {dev_drec:.4g}), cosine {_cos(drec, dg):.5f}")
    assert abs(float(loss) - float(loss_g)) <= 1.2 * dev_loss + 1e-6 * abs(float(loss_g)), (float(loss), float(loss_g), dev_loss)
    assert float((drec.cpu() - dg).abs().max()) <= 1.2 * dev_drec, (float((drec.cpu() - dg).abs().max()), dev_drec)
    assert _cos(drec, dg) >= 0.98
    l2, d2, g2 = _run(face_module, img, rec, c["boxes"])
    equal = torch.equal(loss, l2) and torch.equal(diffs, d2) and torch.equal(drec, g2)
    print(f"{name}: static node against the list path, bf16: bits {'EQUAL' if equal else 'DIFFER'}")


def test_nothing_of_an_earlier_table_survives(golden, face_module):
    """n4_overlap then n1_portrait on ONE table == n1_portrait on a fresh table, bit for bit: rows, valid flags and seeds are rewritten in full"""
    from mas_hip import face as FH
    c4, img4, rec4, *_ = _case(golden, "n4_overlap")
    c1, img1, rec1, *_ = _case(golden, "n1_portrait")
    table = FH.FaceTable(DEV)
    assert table.write(c4["boxes"], c4["images"]) == 4
    first = _run(face_module, img4, rec4, table)
    assert table.write(c1["boxes"], c1["images"]) == 1
    second = _run(face_module, img1, rec1, table)
    fresh = _run(face_module, img1, rec1, _table(c1))
    assert all(torch.equal(a, b) for a, b in zip(second, fresh))
    assert float(second[0]) != float(first[0]) and float(second[0]) > 0.0
    again = _run(face_module, img1, rec1, table)                  # and two runs of one table give equal bits
    assert all(torch.equal(a, b) for a, b in zip(second, again))


def test_zero_faces_run_anyway_is_exactly_zero(golden, face_module):
    from mas_hip import face as FH
    c, img, rec, *_ = _case(golden, "n3_edge_land_down")
    table = FH.FaceTable(DEV)
    assert table.write(c["boxes"], c["images"]) == 3
    _run(face_module, img, rec, table)
    assert table.write([[] for _ in range(c["images"])], c["images"]) == 0
    loss, diffs, drec = _run(face_module, img, rec, table)
    assert float(loss) == 0.0 and torch.count_nonzero(diffs) == 0 and torch.count_nonzero(drec) == 0
    assert torch.isfinite(drec).all()
    loss, _, drec = _run(face_module, img, rec, FH.FaceTable(DEV))        # a table that was never written
    assert float(loss) == 0.0 and torch.count_nonzero(drec) == 0


def test_no_host_synchronisation(golden, face_module):
    from mas_hip import face as FH
    c, img, rec, *_ = _case(golden, "n4_overlap")
    table = FH.FaceTable(DEV)
    imgd, recd = img.to(DEV), rec.to(DEV)
    table.write(c["boxes"], c["images"])
    face_module(imgd, recd.clone().requires_grad_(True), table).backward()          # first use: the weights' images, the BatchNorm table
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for boxes in (c["boxes"], [[], []], c["boxes"][:1] + [[]], c["boxes"]):       # four writes: both pinned buffers come round again
            n = table.write(boxes, c["images"])
            r = recd.clone().requires_grad_(True)
            loss = face_module(imgd, r, table)
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert n == 4 and bool(torch.isfinite(loss)) and float(loss) > 0.0 and float(r.grad.abs().max()) > 0.0


def test_training_mode_and_foreign_tables_raise(golden, face_module):
    from mas_hip import face as FH
    c, img, rec, *_ = _case(golden, "n3_edge_land_down")
    table = FH.FaceTable(DEV)
    table.write(c["boxes"], c["images"])
    with pytest.raises(ValueError, match="written for"):
        face_module(img[:1].to(DEV), rec[:1].to(DEV), table)                         # a row names image 1 of a batch of 1
    with pytest.raises(RuntimeError, match="face table is on"):
        face_module(img.to(DEV), rec.to(DEV), FH.FaceTable("cpu"))
    face_module.train()
    with pytest.raises(RuntimeError, match="evaluation-mode"):
        face_module(img.to(DEV), rec.to(DEV), table)
