"""The four NHWC data-movement kernels of misc.hip, bit for bit against torch on the CPU, in bf16 and fp32: ``upsample2x`` (nearest x2),
``sumpool2x`` (the adjoint: the data-gradient fallback of the Upsample fold), ``zero_stuff2x`` (the adjoint of a stride-2 read: the
Downsample data-gradient fallback) and ``space_to_depth2x`` (feeds every weight gradient of the discriminator's 4x4 stride-2 convolutions).
One thread moves one 16-byte unit (8 bf16 / 4 fp32 channels) and walks a grid-stride loop; the grid is capped at GRID_CAP blocks of NT
threads (``grid_for`` in misc.hip), so each kernel also runs one shape with more units than that: the loop's second trip."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))

GRID_CAP, NT = 8192, 256                    # misc.hip: grid_for() / NT
DTYPES = [torch.bfloat16, torch.float32]


def _units(numel, dtype):
    return numel // (8 if dtype == torch.bfloat16 else 4)


def _ints(shape, dtype, seed, lo=-100, hi=100):
    """integers (exact in bf16 up to 256, and every sum of four of them exact in fp32), none of them zero-heavy"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def _gpu(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mas_hip import ops
    return ops


def _check(y, want, name):
    from mas_hip import ops
    assert ops.last_kernel() == name
    assert y.shape == want.shape and y.dtype == want.dtype, (y.shape, want.shape, y.dtype)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y.cpu(), want), f"{int((y.cpu().float() != want.float()).sum())} of {want.numel()} elements differ"


# n, c, h, w: C = 8 (one bf16 unit), C = 24, odd maps
SMALL = [(2, 8, 5, 7), (1, 24, 9, 3), (3, 16, 1, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_upsample2x_equals_repeat_interleave(dtype):
    ops = _ops()
    big = (1, 24, 419, 421) if dtype == torch.bfloat16 else (1, 8, 513, 513)
    assert _units(4 * big[0] * big[1] * big[2] * big[3], dtype) > GRID_CAP * NT      # second trip of the grid-stride loop
    for i, shape in enumerate(SMALL + [big]):
        x = _ints(shape, dtype, 10 + i)
        want = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        _check(ops.upsample2x(_gpu(x)), want, "upsample2x")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_sumpool2x_equals_the_fp32_sum_rounded_once(dtype):
    ops = _ops()
    big = (1, 64, 513, 513) if dtype == torch.bfloat16 else (1, 32, 513, 513)          # OUTPUT shapes
    assert _units(big[0] * big[1] * big[2] * big[3], dtype) > GRID_CAP * NT
    for i, (n, c, ho, wo) in enumerate(SMALL + [big]):
        # int operands: the four-pixel sum is exact in fp32 whatever the order, so only the final rounding is left (|sum| <= 400 > 256:
        # bf16 does round, ties included)
        x = _ints((n, c, 2 * ho, 2 * wo), dtype, 20 + i)
        xf = x.float()
        want = (xf[:, :, 0::2, 0::2] + xf[:, :, 0::2, 1::2] + xf[:, :, 1::2, 0::2] + xf[:, :, 1::2, 1::2]).to(dtype)
        _check(ops.sumpool2x(_gpu(x)), want, "sumpool2x")
    # gauss operands: the fp32 sum in the kernel's order, dh outer, dw inner: ((x00 + x01) + x10) + x11
    g = torch.Generator().manual_seed(29)
    x = torch.randn(2, 24, 18, 14, generator=g).to(dtype)
    xf = x.float()
    want = (((xf[:, :, 0::2, 0::2] + xf[:, :, 0::2, 1::2]) + xf[:, :, 1::2, 0::2]) + xf[:, :, 1::2, 1::2]).to(dtype)
    _check(ops.sumpool2x(_gpu(x)), want, "sumpool2x")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_zero_stuff2x_places_every_pixel_and_zeroes_the_rest(dtype):
    ops = _ops()
    big = (1, 24, 419, 421) if dtype == torch.bfloat16 else (1, 8, 513, 513)
    assert _units(big[0] * big[1] * (2 * big[2] - 1) * (2 * big[3] - 1), dtype) > GRID_CAP * NT
    grow = [(0, 0), (2, 1), (1, 4)]         # (2H - 1, 2W - 1) is what the data gradient passes; larger maps get zero rows / columns
    for i, (n, c, h, w) in enumerate(SMALL + [big]):
        x = _ints((n, c, h, w), dtype, 30 + i, lo=1, hi=100)          # no zero in x: a pixel dropped or misplaced cannot hide among the zeros
        for dh, dw in (grow if i < len(SMALL) else grow[:1]):
            hout, wout = 2 * h - 1 + dh, 2 * w - 1 + dw
            want = torch.zeros(n, c, hout, wout, dtype=dtype)
            want[:, :, 0:2 * h - 1:2, 0:2 * w - 1:2] = x
            _check(ops.zero_stuff2x(_gpu(x), hout, wout), want, "zero_stuff2x")


def _s2d_ref(x, ho, wo, pad):
    """channel (dy * 2 + dx) * C + c of output pixel (h', w') = x[c, 2 h' + dy - pad, 2 w' + dx - pad], zero outside"""
    n, c, h, w = x.shape
    xp = F.pad(x, (pad, max(0, 2 * wo - w - pad), pad, max(0, 2 * ho - h - pad)))[:, :, :2 * ho, :2 * wo]
    return torch.cat([xp[:, :, dy::2, dx::2] for dy in range(2) for dx in range(2)], dim=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_space_to_depth2x_equals_the_strided_gather(dtype):
    ops = _ops()
    big = (1, 32, 725, 727) if dtype == torch.bfloat16 else (1, 16, 725, 727)
    shapes = [(2, 8, 5, 7), (1, 24, 9, 5), (2, 16, 8, 6), big]
    for i, (n, c, h, w) in enumerate(shapes):
        x = _ints((n, c, h, w), dtype, 40 + i, lo=1, hi=100)
        for pad in (0, 1):
            # the 4x4 / stride-2 convolution's output map, and the (ho + 1) x (wo + 1) image conv_wgrad_raw asks for
            ho, wo = (h + 2 * pad - 4) // 2 + 1, (w + 2 * pad - 4) // 2 + 1
            if (n, c, h, w) == big:
                assert _units(n * 4 * c * (ho + 1) * (wo + 1), dtype) > GRID_CAP * NT
            want = _s2d_ref(x, ho + 1, wo + 1, pad)
            assert want.shape == (n, 4 * c, ho + 1, wo + 1)
            _check(ops.space_to_depth2x(_gpu(x), ho + 1, wo + 1, pad), want, "space_to_depth2x")
