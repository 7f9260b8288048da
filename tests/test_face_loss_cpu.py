"""FaceLoss without a GPU: the module's surface against the golden the reference's own class wrote (tests/golden/face_tiny.npz,
tests/golden/make_face_golden.py), weight loading and its errors, the wiring into VQLPIPSWithDiscriminator, the host geometry
(torchvision's Resize / CenterCrop rules, the reference's faces[:6] row selection), the CPU restatement against the golden, and the
new C entry points' argument checks."""
import ctypes
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import face_ref as R  # noqa: E402

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
def module(ckpt, monkeypatch):
    monkeypatch.setenv("MAS_FACE_CKPT", ckpt)
    from losses.face_loss import FaceLoss
    return FaceLoss()


def test_keys_shapes_and_parameter_count_match_the_reference(golden, module):
    z, _ = golden
    sd = module.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    assert len(sd) == 318
    assert sum(p.numel() for p in module.parameters()) == int(z["n_params"]) == 23508032
    for k, shape in R.expected_shapes().items():
        assert tuple(sd[k].shape) == shape, k
    assert module.alphas == R.ALPHAS and module.channels == [64, 256, 512, 1024, 2048]
    # weights came from the file
    ref = R.synth_face_state_dict(0)
    assert torch.equal(sd["layer3.5.conv2.weight"], ref["layer3.5.conv2.weight"]) and module.unloaded == []


def test_frozen_and_in_evaluation_mode(module):
    assert not module.training
    assert all(not m.training for m in module.modules())
    assert all(not p.requires_grad for p in module.parameters())


def test_reference_checkpoint_with_extra_keys_loads(tmp_path, monkeypatch):
    sd = R.synth_face_state_dict(1)
    sd["fc.weight"] = torch.zeros(8631, 2048)                 # the VGGFace2 classifier head the loss never uses: strict=False
    p = tmp_path / "w.pt"
    torch.save(sd, p)
    monkeypatch.setenv("MAS_FACE_CKPT", str(p))
    from losses.face_loss import FaceLoss
    m = FaceLoss()
    assert torch.equal(m.conv1.weight, sd["conv1.weight"]) and m.unloaded == []


def test_missing_weights_are_an_error_naming_the_variable(monkeypatch):
    from losses import face_loss
    monkeypatch.delenv("MAS_FACE_CKPT", raising=False)
    monkeypatch.delenv("MAS_FACE_STRICT", raising=False)
    monkeypatch.setattr(face_loss, "REFERENCE_CKPT", "/nonexistent/face_loss_weights.pt")
    with pytest.raises(RuntimeError, match="MAS_FACE_CKPT"):
        face_loss.FaceLoss()
    monkeypatch.setenv("MAS_FACE_STRICT", "0")
    face_loss.FaceLoss._warned = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        m = face_loss.FaceLoss()
    assert any("MAS_FACE_CKPT" in str(w.message) and "RANDOM" in str(w.message) for w in rec)
    assert len(m.unloaded) == 265


def test_vq_img_loss_builds_face_loss_from_the_checkpoint(ckpt, monkeypatch):
    from losses.face_loss import FaceLoss
    from losses.loss_img import VQLPIPSWithDiscriminator
    monkeypatch.setenv("MAS_FACE_CKPT", ckpt)
    lf = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None)
    assert isinstance(lf.face_loss, FaceLoss) and not lf.face_loss.training
    monkeypatch.delenv("MAS_FACE_CKPT")
    from losses import face_loss
    monkeypatch.setattr(face_loss, "REFERENCE_CKPT", "/nonexistent/face_loss_weights.pt")
    VQLPIPSWithDiscriminator._face_warned = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        l0 = VQLPIPSWithDiscriminator(disc_start=0, perceptual_loss=None)
    assert l0.face_loss is None
    assert any("FaceLoss" in str(w.message) and "ABSENT" in str(w.message) and "MAS_FACE_CKPT" in str(w.message) for w in rec)


def test_resize_and_center_crop_geometry():
    from mas_hip import face as F
    assert F.resized_size(256, 256) == (256, 256)
    assert F.resized_size(40, 32) == (320, 256)                 # portrait: width is the short side
    assert F.resized_size(20, 40) == (256, 512)
    assert F.resized_size(30, 70) == (256, int(256 * 70 / 30))  # int() truncates: 597
    assert F.resized_size(300, 300) == (256, 256)               # a downscaled crop
    # banker's rounding: (rh - 254) / 2 = 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert F.center_offsets(255, 256) == (0, 1)
    assert F.center_offsets(257, 259) == (2, 2)
    assert F.center_offsets(256, 597) == (1, 172)
    g = F.face_geometry([-6, 30, 20, 60])
    assert g == dict(top=30, left=-6, h=30, w=26, rh=int(256 * 30 / 26), rw=256, ct=int(round((int(256 * 30 / 26) - 254) / 2)), cl=1)
    for box in ([5, 5, 5, 20], [5, 5, 20, 5], [10, 10, 4, 20]):
        with pytest.raises(ValueError):
            F.face_geometry(box)


def test_restated_geometry_matches_torchvision_rules():
    """the restatement's crop sizes follow the same rules (it is what the golden's stub of torchvision ran)"""
    from mas_hip import face as F
    img = torch.randn(3, 48, 64)
    for box in ([8, 6, 40, 46], [-6, 30, 20, 60], [-130, -120, 170, 180], [10, 4, 50, 24]):
        g = F.face_geometry(box)
        c = R.tv_crop(img, g["top"], g["left"], g["h"], g["w"])
        assert tuple(c.shape[-2:]) == (g["h"], g["w"])
        assert tuple(R.tv_resize(c).shape[-2:]) == (g["rh"], g["rw"])
        assert tuple(R.face_crop(img, box).shape) == (3, 254, 254)


@pytest.mark.parametrize("n", range(8))
def test_surviving_rows_and_pairing(n):
    """faces[:6] of cat([gt], [rec]); pairs (q, half + q); rec rows are the tail [n, len)"""
    from mas_hip import face as F
    rows = F.surviving_rows(n)
    full = [(0, i) for i in range(n)] + [(1, i) for i in range(n)]
    assert rows == full[:6]
    assert len(rows) == min(2 * n, 6) and len(rows) % 2 == 0
    half = len(rows) // 2
    pairs = [(rows[q], rows[half + q]) for q in range(half)]
    rec_rows = [i for i, r in enumerate(rows) if r[0] == 1]
    assert rec_rows == list(range(n, len(rows)))                  # the backward's tail slice
    if n <= 3:
        assert pairs == [((0, q), (1, q)) for q in range(n)]
    if n == 4:
        assert pairs == [((0, 0), (0, 3)), ((0, 1), (1, 0)), ((0, 2), (1, 1))]
    if n >= 6:
        assert rec_rows == []
    faces = [[[0, 0, 10, 10]] * 2, [[0, 0, 10, 10]] * (n - 2)] if n >= 2 else [[[0, 0, 10, 10]] * n]
    nn_, table = F.plan(faces, len(faces))
    assert nn_ == n and [(r.src, r.b) for r in table] == [(s, 0 if i < 2 else 1) for s, i in rows]


def test_plan_stops_at_the_shorter_of_images_and_boxes():
    from mas_hip import face as F
    n, rows = F.plan([[[0, 0, 10, 10]], [[0, 0, 12, 12]], [[0, 0, 14, 14]]], 2)
    assert n == 2 and [r.h for r in rows] == [10, 12, 10, 12]


@pytest.mark.parametrize("name", ["n1_portrait", "n4_overlap"])
def test_restatement_reproduces_the_golden(golden, name):
    z, cases = golden
    c = next(c for c in cases if c["name"] == name)
    img, rec = R.synth_images(c["images"], c["H"], c["W"], c["seed"])
    rec.requires_grad_(True)
    loss, diffs = R.face_loss(R.synth_face_state_dict(0), img, rec, c["boxes"], return_diffs=True)
    loss.backward()
    np.testing.assert_allclose(loss.detach().numpy(), z[name + "/loss"], rtol=1e-5)
    np.testing.assert_allclose(diffs.detach().numpy(), z[name + "/diffs"], rtol=1e-5)
    d = z[name + "/drec"]
    np.testing.assert_allclose(rec.grad.numpy(), d, rtol=0, atol=1e-5 * np.abs(d).max())


def test_forward_without_gpu_refuses(ckpt, monkeypatch):
    """the product path has no CPU fallback"""
    from losses.face_loss import FaceLoss
    monkeypatch.setenv("MAS_FACE_CKPT", ckpt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = FaceLoss()
    img, rec = R.synth_images(1, 32, 32, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        m(img, rec, [[[0, 0, 20, 20]]])


def test_face_abi_entries_reject_bad_arguments_without_gpu():
    import mas_hip
    L = mas_hip.lib()
    P = ctypes.c_void_p
    assert L.mas_face_crop_fwd(None, None, None, 1, None, 0, None) == -1 and b"null" in L.mas_last_error()
    img = mas_hip.FaceImage(1, 0, 1, 3, 32, 32, 0, 3072, 1024, 32, 1)
    row = mas_hip.FaceRow(0, 0, 0, 0, 10, 10, 256, 256, 1, 1)
    rows = (mas_hip.FaceRow * 1)(row)
    assert L.mas_face_crop_fwd(ctypes.byref(img), ctypes.byref(img), rows, 9, P(1), 0, None) == -1        # more than 8 rows
    bad = (mas_hip.FaceRow * 1)(mas_hip.FaceRow(0, 0, 0, 0, 10, 10, 256, 256, 3, 1))                      # centre crop leaves the image
    assert L.mas_face_crop_fwd(ctypes.byref(img), ctypes.byref(img), bad, 1, P(1), 0, None) == -1 and b"geometry" in L.mas_last_error()
    img4 = mas_hip.FaceImage(1, 0, 1, 4, 32, 32, 0, 4096, 1024, 32, 1)
    assert L.mas_face_crop_fwd(ctypes.byref(img4), ctypes.byref(img), rows, 1, P(1), 0, None) == -1       # not RGB
    assert L.mas_face_crop_bwd(None, rows, 1, ctypes.byref(img), None) == -1
    assert L.mas_face_stem_fwd(None, None, None, 1, 1, None) == -1
    assert L.mas_face_stem_dgrad(P(1), P(1), P(1), 7, 1, None) == -1
    assert L.mas_face_bn_fold(None, 53, None, None) == -1
    assert L.mas_face_bn_fold(P(1), 0, P(1), None) == -1
    assert L.mas_face_pool_fwd(P(1), P(1), P(1), P(1), 0, 1, 127, 127, 62, None) == -1                    # C % 4
    assert L.mas_face_pool_bwd(P(1), P(1), P(1), None, None, P(1), 0, 1, 127, 127, 64, None) == -1
    assert L.mas_face_join_fwd(None, P(1), P(1), None, P(1), 0, 1, 4, None) == -1
    assert L.mas_face_join_bwd(None, None, P(1), P(1), None, P(1), None, 0, 1, 4, None) == -1
    assert L.mas_face_relu_bn_bwd(None, P(1), P(1), P(1), 0, 1, 4, None) == -1
    assert L.mas_face_subsample2x(P(1), P(1), 1, 1, 4, 4, 4, None) == -1                                  # bf16 needs C % 8
    f = mas_hip.FaceFeats()
    assert L.mas_face_l1_workspace(None) == -1 and L.mas_face_l1_workspace(ctypes.byref(f)) == -1
    for i, chw in enumerate((64 * 127 * 127, 256 * 63 * 63, 512 * 32 * 32, 1024 * 16 * 16, 2048 * 8 * 8)):
        f.p[i], f.chw[i] = 1, chw
    f.half, f.dtype = 3, 1
    assert L.mas_face_l1_workspace(ctypes.byref(f)) > 0
    assert L.mas_face_l1_fwd(ctypes.byref(f), None, None, None) == -1
    seeds = (ctypes.c_void_p * 5)(*([1] * 5))
    assert L.mas_face_l1_bwd(ctypes.byref(f), 2, 1, P(1), seeds, None) == -1                              # a gt row
    assert L.mas_face_l1_bwd(ctypes.byref(f), 3, 4, P(1), seeds, None) == -1                              # past the last row
