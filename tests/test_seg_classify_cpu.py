"""CPU side of reading VQ-SEG logits back as label planes: the rule as tests/helpers/seg_classify_ref.py states it against the
reference Visualizer's own expression (log_utils.py:55-67), ``SegLabels.from_logits`` on the CPU against the helper, hand-built ties,
``SegAgreement``'s arithmetic on counts typed in by hand, ``colorize``, argument validation, and the two new entry points' null-argument
convention."""
import ctypes
import math
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
import seg_classify_ref as CR  # noqa: E402
from mas_hip.seglabels import SegAgreement, SegLabels, SegLayout  # noqa: E402

REF = SegLayout()
REF_T = CR.REFERENCE_THRESHOLDS


@pytest.mark.parametrize("scale", [1.0, 4.0, 30.0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_rule_equals_the_visualizer_expression(dtype, scale):
    """reference log_utils.py:55-67 (argmax, one_hot, `*= sigmoid > 0.2` for face and edge) against the restated rule, on tie-rich logits;
    entries within 1e-2 of tau -- the only place `sigmoid(x) > 0.2` in fp32 and `x > tau` can differ -- are first moved to tau + 0.5"""
    x = CR.tie_rich_logits((2, 159, 16, 17), REF.groups, 1, REF_T, scale, seed=int(scale), bf16=dtype == torch.bfloat16, shift_group=2, clear=1e-2)
    for k, tau in enumerate(CR.taus(REF_T)):
        if np.isfinite(tau):
            assert not (np.abs(x[:, REF.bases[k]:REF.bases[k] + max(1, (REF.groups + (1,))[k])] - tau) < 1e-2).any()
    want = CR.visualizer_labels(torch.from_numpy(x).to(dtype))
    got = CR.classify(x, REF.groups, 1, REF_T)
    assert np.array_equal(got, want)
    face = got[:, 2]
    assert set(np.unique(face)) == set(range(6)), "none and every face class occur"
    assert set(np.unique(got[:, 3])) == {0, 1}
    if scale <= 4.0:
        ties = np.sort(x[:, :133], axis=1)
        assert (ties[:, -1] == ties[:, -2]).mean() > 0.01                               # the largest value is often held twice
    lab = SegLabels.from_logits(torch.from_numpy(x).to(dtype))
    assert lab.layout == REF and lab.planes.dtype == torch.uint8 and np.array_equal(lab.planes.numpy(), got)


def _one_pixel(values, layout, thresholds):
    x = torch.tensor(values, dtype=torch.float32).view(1, -1, 1, 1)
    ref = CR.classify(x.numpy(), layout.groups, layout.value_channels, thresholds)
    got = SegLabels.from_logits(x, layout, thresholds).planes.numpy()
    assert np.array_equal(got, ref)
    return [int(v) for v in got.reshape(-1)]


def test_hand_built_ties():
    lay = SegLayout(groups=(3, 2), value_channels=1)
    none = (None, None, None)
    assert _one_pixel([5, 1, 1, 0, 0, 0], lay, none)[:2] == [1, 1]                     # the maximum in a group's first channel
    assert _one_pixel([1, 1, 5, 0, 7, 0], lay, none)[:2] == [3, 2]                     # in its last channel
    assert _one_pixel([1, 5, 5, 2, 2, 0], lay, none)[:2] == [2, 1]                     # held twice: the lower channel
    assert _one_pixel([5, 1, 5, 0, 0, 0], lay, none)[:2] == [1, 1]
    assert _one_pixel([1, 2, 3, 9, 0, 0], lay, none)[:2] == [3, 1]                     # the neighbour's adjacent channel is larger: no leak
    assert _one_pixel([9, 1, 1, 0, 3, 8], lay, none)[:2] == [1, 2]
    assert _one_pixel([2, 2, 2, 2, 2, 2], lay, none) == [1, 1, 1]                      # all equal: label 1
    assert _one_pixel([-2, -2, -2, -2, -2, -2], lay, (0.2, 0.2, 0.2)) == [0, 0, 0]     # ... or 0 when gated (sigmoid(-2) = 0.12)
    assert _one_pixel([-1, -1, -1, -1, -1, -1], lay, (0.2, 0.2, 0.2)) == [1, 1, 1]     # (sigmoid(-1) = 0.27)
    assert _one_pixel([-2, -2, -1, -2, -2, -2], lay, (0.2, None, 0.9)) == [3, 1, 0]
    inf = float("inf")
    assert _one_pixel([-inf, inf, inf, -inf, -inf, inf], lay, (0.5, None, 0.5)) == [2, 0, 1]     # all -inf: nothing is above -inf


def test_logit_threshold_is_rounded_once_from_double():
    from mas_hip.seglabels import logit_thresholds
    taus = logit_thresholds(REF)
    assert taus[0] == taus[1] == -math.inf
    assert taus[2] == taus[3] == float(np.float32(math.log(0.2 / 0.8))) == float(CR.taus(REF_T)[2])
    assert logit_thresholds(SegLayout(groups=(2,), value_channels=0), 0.5) == (0.0,)


def test_agreement_arithmetic_on_counts_typed_in_by_hand():
    lay = SegLayout(groups=(3,), value_channels=1)                                       # C = 4, P = 2
    inter, pred, target = [2, 0, 0, 1], [4, 3, 0, 2], [2, 1, 0, 5]
    a = SegAgreement(lay, torch.tensor(inter + pred + target + [6, 4] + [8]))
    assert a.inter.tolist() == inter and a.pred.tolist() == pred and a.target.tolist() == target
    assert a.agree.tolist() == [6, 4] and int(a.pixels) == 8
    want = []
    for i, p, t in zip(inter, pred, target):                                             # brute force
        union = p + t - i
        want.append(i / union if union else float("nan"))
    iou = a.iou.numpy()
    assert iou.dtype == np.float64 and np.array_equal(np.isnan(iou), np.isnan(want))
    assert math.isnan(iou[2]) and np.array_equal(iou[[0, 1, 3]], np.array(want)[[0, 1, 3]])
    assert np.array_equal(a.pixel_accuracy.numpy(), np.array([6 / 8, 4 / 8]))
    assert np.array_equal(a.miou.numpy(), np.array([np.nanmean(np.array(want[:3])), want[3]]))
    b = SegAgreement(lay)
    assert b.counts.tolist() == [0] * 15 and bool(torch.isnan(b.iou).all()) and bool(torch.isnan(b.miou).all())
    c = a + a
    assert c.counts.tolist() == [2 * v for v in a.counts.tolist()] and a.counts[-1] == 8
    held = b.counts
    b += a
    b += a
    assert b.counts is held and torch.equal(b.counts, c.counts)
    assert torch.equal(c.iou[[0, 1, 3]], a.iou[[0, 1, 3]])
    with pytest.raises(ValueError, match="SegAgreement"):
        a + SegAgreement(SegLayout(groups=(2,), value_channels=2))
    with pytest.raises(ValueError, match="SegAgreement"):
        SegAgreement(lay, torch.zeros(14, dtype=torch.int64))


def test_colorize():
    lay = SegLayout(groups=(3, 2), value_channels=1)
    planes = torch.tensor([[0, 1, 2], [3, 255, 7]], dtype=torch.uint8).view(1, 1, 2, 3).repeat(2, 3, 1, 1)
    planes[1, 2] = 0
    lab = SegLabels(planes, lay)
    pal = torch.randint(0, 256, (3, 256, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    pic = lab.colorize(pal)
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (2, 3, 3, 2, 3)
    for b in range(2):
        for k in range(3):
            for y in range(2):
                for x in range(3):
                    assert torch.equal(pic[b, k, :, y, x], pal[k, int(planes[b, k, y, x])])
    dflt = lab.colorize()
    assert tuple(dflt.shape) == (2, 3, 3, 2, 3) and torch.equal(dflt, lab.colorize())     # seeded
    assert int(dflt[:, :, :, 0, 0].max()) == 0 and int(dflt[1, 2].max()) == 0            # label 0 is black
    assert int(dflt[0, 0, :, 0, 1].max()) > 0
    with pytest.raises(ValueError, match="colorize"):
        lab.colorize(pal[:2])


def test_validation():
    from mas_hip import ops
    x = torch.zeros(1, 159, 2, 2)
    small = SegLayout(groups=(3, 2), value_channels=1)
    for f in (SegLabels.from_logits, ops.seg_classify):
        with pytest.raises(ValueError, match="channels"):
            f(x[:, :158])                                                                # a wrong shape for the layout
        with pytest.raises(ValueError, match="channels"):
            f(x, small, 0.5)
        with pytest.raises(ValueError):
            f(x[0])
        for bad in (0.0, 1.0, (None, None, 0.2, 1.0), (None, 0.0, 0.2, 0.2)):
            with pytest.raises(ValueError, match="threshold"):
                f(x, None, bad)
        with pytest.raises(ValueError, match="thresholds"):
            f(x, None, (None, None, 0.2))                                                # the wrong length
        with pytest.raises(ValueError, match="thresholds"):
            f(torch.zeros(1, 6, 2, 2), small)                                            # no default for another layout
        with pytest.raises(RuntimeError, match="dtype"):
            f(x.half())
    assert SegLabels.from_logits(torch.zeros(1, 6, 2, 2), small, (None, 0.5, None)).planes[0, :, 0, 0].tolist() == [1, 0, 1]
    with pytest.raises(RuntimeError, match="seg_classify"):                              # the op itself has no CPU path
        ops.seg_classify(x)
    lab = SegLabels(torch.zeros(1, 4, 2, 2, dtype=torch.uint8))
    with pytest.raises((RuntimeError, ValueError), match="seg_agreement"):
        ops.seg_agreement(lab, lab)
    with pytest.raises(TypeError, match="seg_agreement"):
        ops.seg_agreement(lab.planes, lab)


def test_model_methods_need_eval_mode():
    from models import VQBASE
    cfg = dict(ddconfig=dict(z_channels=32, in_channels=159, out_channels=159, channels=[32, 32, 64], num_res_blocks=1,
                             resolution=16, attn_resolutions=[8], dropout=0.0), n_embed=64, embed_dim=32, init_steps=10, reservoir_size=100)
    m = VQBASE(**cfg)
    with pytest.raises(RuntimeError, match="eval"):
        m.decode_to_labels(torch.zeros(1, 16, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="eval"):
        m.reconstruct_labels(SegLabels(torch.zeros(1, 4, 16, 16, dtype=torch.uint8)))


def test_entry_points_in_header_exports_and_binding():
    import mas_hip
    txt = open(os.path.join(ROOT, "include", "mas_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    raw = ctypes.CDLL(mas_hip.LIB_PATH)
    for name in ("mas_seg_classify", "mas_seg_agreement"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in mas_hip.EXPORTS and hasattr(raw, name), name
    assert mas_hip.lib().mas_abi_version() == mas_hip.ABI_VERSION == 10


def test_entry_points_validate_arguments_without_gpu():
    import mas_hip
    L = mas_hip.lib()
    g = (ctypes.c_int * 3)(133, 20, 5)
    tau = (ctypes.c_float * 4)(-math.inf, -math.inf, -1.0, -1.0)
    assert L.mas_seg_classify(None, mas_hip.F32, mas_hip.SEG_NCHW, g, 3, 1, tau, 2, 8, 8, None, None) == -1
    assert b"seg_classify" in L.mas_last_error() and b"null" in L.mas_last_error()
    assert L.mas_seg_classify(None, mas_hip.F32, mas_hip.SEG_NCHW, g, 3, 1, None, 2, 8, 8, None, None) == -1 and b"null" in L.mas_last_error()
    assert L.mas_seg_agreement(None, None, g, 3, 1, 2, 8, 8, None, None) == -1
    assert b"seg_agreement" in L.mas_last_error() and b"null" in L.mas_last_error()
    # the envelope, checked before anything is launched (the pointers are never read on the host)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.mas_seg_classify(p, mas_hip.F32, mas_hip.SEG_NCHW, g, 3, 6, tau, 1, 8, 8, p, None) == -2                 # nine planes
    assert L.mas_seg_classify(p, mas_hip.F32, mas_hip.SEG_NCHW, (ctypes.c_int * 1)(256), 1, 0, tau, 1, 8, 8, p, None) == -2
    assert L.mas_seg_classify(p, mas_hip.F32, mas_hip.SEG_NCHW, g, 3, 1, tau, 1, 1 << 16, 1 << 15, p, None) == -2 and b"2^30" in L.mas_last_error()
    assert L.mas_seg_classify(p, 7, mas_hip.SEG_NCHW, g, 3, 1, tau, 1, 8, 8, p, None) == -2
    assert L.mas_seg_classify(p, mas_hip.F32, 5, g, 3, 1, tau, 1, 8, 8, p, None) == -1
    assert L.mas_seg_classify(p, mas_hip.F32, mas_hip.SEG_NCHW, g, 3, 1, (ctypes.c_float * 4)(0, 0, math.nan, 0), 1, 8, 8, p, None) == -1
    assert L.mas_seg_classify(p, mas_hip.F32, mas_hip.SEG_NCHW, g, 3, 1, tau, 0, 8, 8, p, None) == -1
    assert L.mas_seg_agreement(p, p, g, 3, 6, 1, 8, 8, p, None) == -2
    assert L.mas_seg_agreement(p, p, g, 3, 1, 1 << 20, 1 << 10, 1 << 10, p, None) == -2 and b"2^32" in L.mas_last_error()
