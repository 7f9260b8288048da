"""The VQ-IMG read-out without a GPU: the numpy helper (tests/helpers/img_metrics_ref.py) against closed forms, the
``ImageAgreement`` / ``CodeUsage`` arithmetic on hand-made CPU tensors, and every argument error of ``ops.image_bytes`` /
``image_agreement`` / ``code_usage`` and of ``VQBASE.decode_to_images`` / ``reconstruction_metrics`` -- raised before any device call."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"),):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import img_metrics_ref as R  # noqa: E402


def _const(v, h=16, w=19, c=3, n=1):
    return np.full((n, h, w, c), v, dtype=np.uint8)


# ---- the helper against closed forms ------------------------------------------------------------------------------------------------
def test_window_is_the_normalised_gaussian_and_the_package_hands_the_kernel_the_same():
    from mas_hip import imgmetrics
    g = R.window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and g.argmax() == 5 and np.allclose(g, g[::-1], rtol=0, atol=0)
    assert abs(g[4] / g[5] - math.exp(-1.0 / 4.5)) < 1e-15
    assert np.allclose(np.array(imgmetrics.ssim_window()), g, rtol=0, atol=1e-16)
    assert imgmetrics.WINDOW == R.WINDOW and imgmetrics.SIGMA == R.SIGMA


def test_ssim_of_identical_pictures_is_one():
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, (2, 14, 23, 3)).astype(np.uint8)
    assert np.array_equal(R.ssim(a, a), np.ones(2))
    assert np.array_equal(R.sse(a, a), np.zeros(2, np.int64))


@pytest.mark.parametrize("va,vb", [(255, 254), (0, 255), (10, 200), (128, 128)])
def test_ssim_of_constant_pictures(va, vb):
    want = (2.0 * va * vb + R.C1) / (va * va + vb * vb + R.C1)
    got = R.ssim(_const(va), _const(vb))
    assert abs(got[0] - want) < 1e-12, (got, want)
    if (va, vb) == (0, 255):
        assert abs(got[0] - R.C1 / (255.0 ** 2 + R.C1)) < 1e-15                    # black against white
    assert R.sse(_const(va), _const(vb))[0] == (va - vb) ** 2 * 16 * 19 * 3


def test_ssim_below_the_window_is_nan_and_one_window_is_the_plain_weighted_form():
    a, b = _const(3, h=10, w=40), _const(9, h=10, w=40)
    assert np.isnan(R.ssim(a, b)).all() and np.isnan(R.ssim(a.transpose(0, 2, 1, 3), b.transpose(0, 2, 1, 3))).all()
    rs = np.random.RandomState(1)
    a, b = (rs.randint(0, 256, (1, 11, 11, 1)).astype(np.uint8) for _ in range(2))
    w2 = np.outer(R.window(), R.window())
    fa, fb = a[0, :, :, 0].astype(np.float64), b[0, :, :, 0].astype(np.float64)
    ma, mb = (w2 * fa).sum(), (w2 * fb).sum()
    va, vb, vab = (w2 * fa * fa).sum() - ma * ma, (w2 * fb * fb).sum() - mb * mb, (w2 * fa * fb).sum() - ma * mb
    want = (2 * ma * mb + R.C1) * (2 * vab + R.C2) / ((ma * ma + mb * mb + R.C1) * (va + vb + R.C2))
    assert abs(R.ssim(a, b)[0] - want) < 1e-12


def test_byte_ties_round_to_even_and_the_edges_clamp():
    x = (np.arange(-4, 516) * 0.5).astype(np.float32).reshape(1, 1, 1, -1)        # -2, -1.5, ... 257.5
    got = R.to_bytes(x, 0.0, 255.0)[0, 0, :, 0]
    v = x.reshape(-1).astype(np.float64)
    want = np.clip(np.where(v % 1 == 0.5, 2 * np.round(v / 2), np.round(v)), 0, 255)
    assert np.array_equal(got, want.astype(np.uint8))
    assert got[4 + 1] == 0 and got[4 + 3] == 2 and got[4 + 5] == 2 and got[4 + 509] == 254      # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254
    hard = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -1.0, 1.0, 0.0], dtype=np.float32).reshape(1, 1, 1, -1)
    assert R.to_bytes(hard)[0, 0, :, 0].tolist() == [0, 255, 0, 255, 0, 0, 255, 128]            # 127.5 -> 128 (even)
    pic = R.to_bytes(np.zeros((2, 3, 4, 5), np.float32))
    assert pic.shape == (2, 4, 5, 3) and pic.flags["C_CONTIGUOUS"]


def test_code_usage_helper():
    idx = np.array([0, 3, 3, -1, 7, 8, 2 ** 40, 6], dtype=np.int64)
    c = R.code_usage(idx, 8)
    assert c.tolist() == [1, 0, 0, 2, 0, 0, 1, 1, 3] and c.dtype == np.int64
    assert abs(R.perplexity(np.array([5, 5, 5, 5, 9])) - 4.0) < 1e-12 and R.perplexity(np.array([0, 7, 0, 1])) == 1.0


# ---- the holders ----------------------------------------------------------------------------------------------------------------------
def test_image_agreement_arithmetic():
    from mas_hip.imgmetrics import ImageAgreement
    a = ImageAgreement(torch.tensor([0, 300]), torch.tensor([1.0, 0.5], dtype=torch.float64), torch.tensor([300, 300]))
    b = ImageAgreement(torch.tensor([1200]), torch.tensor([0.25], dtype=torch.float64), torch.tensor([1200]))
    c = a + b
    assert len(c) == 3 and c.sse.tolist() == [0, 300, 1200] and c.elements.tolist() == [300, 300, 1200] and c.ssim.tolist() == [1.0, 0.5, 0.25]
    assert c.mse.tolist() == [0.0, 1.0, 1.0] and c.mse.dtype == torch.float64
    psnr = c.psnr
    assert math.isinf(float(psnr[0])) and float(psnr[0]) > 0 and abs(float(psnr[1]) - 20 * math.log10(255.0)) < 1e-12
    assert math.isinf(float(c.mean_psnr)) and math.isfinite(float(c.pooled_psnr))
    assert abs(float(c.pooled_psnr) - 10 * math.log10(255.0 ** 2 / (1500 / 1800))) < 1e-12
    assert abs(float(c.mean_ssim) - 1.75 / 3) < 1e-15
    held = a
    a += b
    assert a is held and len(a) == 3 and a.sse.tolist() == [0, 300, 1200] and len(b) == 1
    with pytest.raises(ValueError, match="ImageAgreement"):
        a + 3
    with pytest.raises(ValueError, match="ImageAgreement"):
        ImageAgreement(torch.tensor([1]), torch.tensor([1.0]), torch.tensor([1]))              # ssim not float64
    with pytest.raises(ValueError, match="ImageAgreement"):
        ImageAgreement(torch.tensor([1, 2]), torch.tensor([1.0], dtype=torch.float64), torch.tensor([1, 2]))


def test_code_usage_arithmetic():
    from mas_hip.imgmetrics import CodeUsage
    k = 16
    uni = CodeUsage(k, torch.cat([torch.full((k,), 5), torch.tensor([2])]))
    assert int(uni.total) == 80 and int(uni.out_of_range) == 2 and int(uni.used) == k and int(uni.dead) == 0
    assert abs(float(uni.perplexity) - k) < 1e-12 and uni.perplexity.dtype == torch.float64
    hot = CodeUsage(k)
    hot.counts[3] = 9
    assert float(hot.perplexity) == 1.0 and int(hot.used) == 1 and int(hot.dead) == k - 1 and int(hot.out_of_range) == 0
    both = uni + hot
    assert both.counts.tolist() == [5, 5, 5, 14] + [5] * 12 + [2] and uni.counts[3] == 5
    held = hot.counts
    hot += uni
    assert hot.counts is held and hot.counts.tolist() == both.counts.tolist()
    with pytest.raises(ValueError, match="CodeUsage"):
        uni + CodeUsage(k + 1)
    with pytest.raises(ValueError, match="CodeUsage"):
        CodeUsage(k, torch.zeros(k, dtype=torch.int64))
    with pytest.raises(ValueError, match="CodeUsage"):
        CodeUsage(0)


def test_the_package_exports_the_new_constants():
    import mas_hip
    assert mas_hip.IMG_SSIM_TILE >= 1 and mas_hip.IMG_SSIM_WINDOW == 11 and mas_hip.IMG_MAX_CHANNELS == 4
    assert mas_hip.CODE_USAGE_LDS_BINS > 8192 and mas_hip.ABI_VERSION == 10
    for name in ("mas_img_bytes", "mas_img_agreement_blocks", "mas_img_agreement", "mas_img_agreement_reduce", "mas_code_usage"):
        assert name in mas_hip.EXPORTS


# ---- argument errors, before any device call ----------------------------------------------------------------------------------------
def test_ops_raise_on_bad_arguments_before_the_device_is_touched():
    from mas_hip import ops
    from mas_hip.imgmetrics import CodeUsage
    x = torch.zeros(2, 3, 12, 12)
    pic = torch.zeros(2, 12, 12, 3, dtype=torch.uint8)
    for lo, hi in ((1.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (-1.0, float("inf")), ("a", 1.0)):
        with pytest.raises(ValueError, match="range"):
            ops.image_bytes(x, lo, hi)
        with pytest.raises(ValueError, match="range"):
            ops.image_agreement(x, x, lo, hi)
    with pytest.raises(ValueError, match="channels"):
        ops.image_bytes(torch.zeros(1, 5, 12, 12))
    with pytest.raises(ValueError, match="channels"):
        ops.image_agreement(torch.zeros(1, 5, 12, 12), torch.zeros(1, 5, 12, 12))
    with pytest.raises(ValueError, match="channels"):
        ops.image_agreement(torch.zeros(1, 12, 12, 5, dtype=torch.uint8), torch.zeros(1, 12, 12, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\[N, C, H, W\]"):
        ops.image_bytes(torch.zeros(3, 12, 12))
    with pytest.raises(ValueError, match=r"\[N, C, H, W\]"):
        ops.image_bytes(torch.zeros(0, 3, 12, 12))
    with pytest.raises(RuntimeError, match="dtype"):
        ops.image_bytes(x.double())
    with pytest.raises(RuntimeError, match="dtype"):
        ops.image_agreement(x, x.half())
    with pytest.raises(ValueError, match="differ"):
        ops.image_agreement(x, torch.zeros(2, 3, 12, 13))                                      # shapes
    with pytest.raises(ValueError, match="differ"):
        ops.image_agreement(x, pic[:1])
    with pytest.raises(ValueError, match="differ"):
        ops.image_agreement(x, torch.zeros(2, 3, 12, 12, device="meta"))                       # devices
    for call in (lambda: ops.image_bytes(x), lambda: ops.image_agreement(x, x), lambda: ops.image_agreement(x, pic),
                 lambda: ops.code_usage(torch.zeros(4, dtype=torch.int64), 8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    idx = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="indices"):
        ops.code_usage(idx.float(), 8)
    with pytest.raises(ValueError, match="indices"):
        ops.code_usage(idx[:0], 8)
    with pytest.raises(ValueError, match="n_embed"):
        ops.code_usage(idx, 0)
    with pytest.raises(ValueError, match="out must be"):
        ops.code_usage(idx, 8, out=CodeUsage(9))
    with pytest.raises(ValueError, match="out must be"):
        ops.code_usage(idx, 8, out=torch.zeros(9, dtype=torch.int64))
    with pytest.raises(ValueError, match="out must be"):
        ops.code_usage(idx, 8, out=CodeUsage(8, device="meta"))


def test_model_methods_raise_on_bad_arguments_before_the_device_is_touched():
    from mas_hip.imgmetrics import CodeUsage
    from mas_hip.seglabels import SegLabels, SegLayout
    from models import VQBASE
    cfg = dict(ddconfig=dict(z_channels=32, in_channels=3, out_channels=3, channels=[32, 32, 64], num_res_blocks=1,
                             resolution=16, attn_resolutions=[8], dropout=0.0), n_embed=64, embed_dim=32, init_steps=10, reservoir_size=100)
    m = VQBASE(**cfg)
    x, tokens = torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, dtype=torch.int64)
    assert m.training
    with pytest.raises(RuntimeError, match="eval"):
        m.decode_to_images(tokens)
    with pytest.raises(RuntimeError, match="eval"):
        m.reconstruction_metrics(x)
    m.eval()
    with pytest.raises(ValueError, match="range"):
        m.decode_to_images(tokens, 1.0, 0.0)
    with pytest.raises(ValueError, match="range"):
        m.reconstruction_metrics(x, 0.0, float("inf"))
    with pytest.raises(TypeError, match="reconstruct_labels"):
        m.reconstruction_metrics(SegLabels(torch.zeros(1, 1, 16, 16, dtype=torch.uint8), SegLayout(groups=(3,), value_channels=0)))
    with pytest.raises(ValueError, match="usage"):
        m.reconstruction_metrics(x, usage=CodeUsage(65))
    with pytest.raises(ValueError, match="usage"):
        m.reconstruction_metrics(x, usage=torch.zeros(65, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.reconstruction_metrics(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.decode_to_images(tokens)
