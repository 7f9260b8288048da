"""The VQ-IMG read-out on the GPU (csrc/img_metrics.hip) against the numpy restatement (tests/helpers/img_metrics_ref.py):
``ops.image_bytes`` and the squared error bit for bit, SSIM within 1e-9 absolute, ``ops.code_usage`` exactly, and the ``VQBASE`` methods.

The SSIM bound is derived, not tuned: byte products are exact integers <= 65025; a separable windowed sum is 22 fp64 FMAs, error
<= 22 * 2^-53 * 65025 = 1.6e-10; the variance terms combine at most four such sums over denominators >= C2 = 58.5, the means are >= 250 x
more accurate over C1 = 6.5: kernel and helper each stay within about 3e-11 per map value, and 1e-9 leaves more than 10 x.

Shapes, with T = ``mas_hip.IMG_SSIM_TILE``: below the window in one and in both directions (SSIM NaN, the squared error still counted),
exactly one window, T + 9 / T + 10 / T + 11 (one window position short of a tile, exactly one tile, one over, in both directions), odd sizes
with 1, 3 and 4 channels, and 2048 x 2048 x 1: more tiles than the largest grid has work-groups (8 per CU), so a work-group walks several.
H W a multiple of 4 (8) takes the 16-byte NCHW byte kernel for fp32 (bf16) when the base pointer allows; the others go pixel by pixel."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import img_metrics_ref as R  # noqa: E402
import mas_hip  # noqa: E402
from mas_hip.imgmetrics import CodeUsage, ImageAgreement  # noqa: E402

pytestmark = pytest.mark.gpu

T = mas_hip.IMG_SSIM_TILE
SHAPES = [(1, 3, 1, 1), (1, 3, 10, 40), (1, 3, 11, 11), (2, 3, 12, 13), (1, 1, 11, 64), (3, 4, 21, 43),
          (1, 3, T + 9, T + 9), (1, 3, T + 10, T + 10), (1, 3, T + 11, T + 11), (1, 2, 16, 24)]
BIG = (1, 1, 2048, 2048)
KINDS = {"uniform": (-1.0, 1.0), "ties": (0.0, 255.0), "hard": (-1.0, 1.0)}           # kind -> (lo, hi)
PDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
SSIM_TOL = 1e-9
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _image(shape, kind, which, bf16):
    """-> (x float32 numpy NCHW, the helper's bytes); computed once.  ``which``: 0 / 1, the two pictures of a pair.  ``bf16``: the values
    are rounded to bf16 first, so that an fp32 and a bf16 tensor hold the same numbers."""
    key = (shape, kind, which, bf16)
    if key not in _cache:
        seed = 97 * which + 13 * shape[0] + 7 * shape[1] + shape[2] * shape[3]
        if kind == "uniform":
            x = np.random.RandomState(seed).uniform(-1.3, 1.3, shape).astype(np.float32)      # wider than [lo, hi]: both clamps occur
        elif kind == "ties":
            x = R.tie_grid(shape, seed)
        else:
            x = R.hard_values(shape, seed)
        if bf16:
            x = torch.from_numpy(x).bfloat16().float().numpy()
        _cache[key] = (x, R.to_bytes(x, *KINDS[kind]))
    return _cache[key]


def _pair_ref(shape, kind, bf16):
    """the helper's (sse, ssim) of the pair; computed once"""
    key = ("pair", shape, kind, bf16)
    if key not in _cache:
        a, b = _image(shape, kind, 0, bf16)[1], _image(shape, kind, 1, bf16)[1]
        _cache[key] = (R.sse(a, b), R.ssim(a, b))
    return _cache[key]


def _place(a, fmt, dtype, dev, offset=0):
    """logical NCHW numpy -> device tensor of `dtype`, dense in `fmt`; offset: that many elements past an allocation's start"""
    n, c, h, w = a.shape
    src = torch.from_numpy(a).to(dev).to(dtype)
    buf = torch.zeros(a.size + offset + 64, dtype=dtype, device=dev)
    if fmt == "nhwc":
        v = buf[offset:offset + a.size].view(n, h, w, c).permute(0, 3, 1, 2)
    else:
        v = buf[offset:offset + a.size].view(n, c, h, w)
    v.copy_(src)
    assert v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


class _no_sync:
    """the calls inside must not synchronise with the host"""

    def __enter__(self):
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


def _same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


# ---- bytes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
@pytest.mark.parametrize("pdt", list(PDT))
@pytest.mark.parametrize("kind", list(KINDS))
def test_image_bytes_are_bit_exact(kind, pdt, fmt):
    from mas_hip import ops
    dev = _dev()
    lo, hi = KINDS[kind]
    seen = set()
    for shape in SHAPES:
        x, want = _image(shape, kind, 0, pdt == "bf16")
        for offset in (0, 1):
            xv = _place(x, fmt, PDT[pdt], dev, offset)
            before = xv.clone()
            with _no_sync():
                got = ops.image_bytes(xv, lo, hi)
            assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (shape[0], shape[2], shape[3], shape[1])
            g = got.cpu().numpy()
            assert np.array_equal(g, want), (shape, kind, pdt, fmt, offset, int((g != want).sum()))
            assert torch.equal(xv.view(torch.int16 if pdt == "bf16" else torch.int32), before.view(torch.int16 if pdt == "bf16" else torch.int32))
            seen |= set(np.unique(g).tolist())
    assert {0, 255} <= seen and len(seen) > 100
    if kind == "ties":
        x, want = _image((3, 4, 21, 43), kind, 0, pdt == "bf16")
        v = x.transpose(0, 2, 3, 1)
        tie = (v % 1 == 0.5) & (v > 0) & (v < 255)
        assert tie.sum() > 100 and (want[tie] % 2 == 0).all()                         # the ties are there, and the helper sent them to even


def test_image_bytes_default_range_and_a_slice():
    from mas_hip import ops
    dev = _dev()
    x, want = _image((3, 4, 21, 43), "uniform", 0, False)
    assert np.array_equal(ops.image_bytes(torch.from_numpy(x).to(dev)).cpu().numpy(), want)                  # (-1, 1)
    wide = torch.zeros(3, 7, 21, 50, device=dev)
    wide[:, 2:6, :, 3:46] = torch.from_numpy(x).to(dev)
    with _no_sync():
        got = ops.image_bytes(wide[:, 2:6, :, 3:46])                                                         # neither dense layout
    assert np.array_equal(got.cpu().numpy(), want)
    lo, hi = -0.73, 2.11                                                                                     # a scale that is not a power of two
    assert np.array_equal(ops.image_bytes(torch.from_numpy(x).to(dev), lo, hi).cpu().numpy(), R.to_bytes(x, lo, hi))


# ---- squared error and SSIM -----------------------------------------------------------------------------------------------------------
def _check_agreement(got, shape, kind, bf16, tag):
    want_sse, want_ssim = _pair_ref(shape, kind, bf16)
    n, c, h, w = shape
    assert isinstance(got, ImageAgreement) and len(got) == n and got.sse.is_cuda
    assert got.sse.dtype == torch.int64 and got.ssim.dtype == torch.float64 and got.elements.tolist() == [c * h * w] * n
    sse, ssim = got.sse.cpu().numpy(), got.ssim.cpu().numpy()
    err = float(np.nanmax(np.abs(ssim - want_ssim))) if not np.isnan(want_ssim).all() else 0.0
    print(f"{tag}: sse {sse.tolist()} ssim {ssim.tolist()} |ssim - helper| max {err:.3e}")
    assert np.array_equal(sse, want_sse), tag
    assert np.array_equal(np.isnan(ssim), np.isnan(want_ssim)), tag
    assert np.isnan(want_ssim).all() == (h < 11 or w < 11)
    assert err <= SSIM_TOL, (tag, err)
    psnr, want_psnr = got.psnr.cpu().numpy(), R.psnr(want_sse, c * h * w)
    assert np.array_equal(np.isinf(psnr), np.isinf(want_psnr)) and np.allclose(psnr[np.isfinite(psnr)], want_psnr[np.isfinite(psnr)], rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind", list(KINDS))
def test_image_agreement_against_the_helper(kind):
    """every shape; a and b in different dtype and memory layout, both ways round, aligned and one element past alignment"""
    from mas_hip import ops
    dev = _dev()
    lo, hi = KINDS[kind]
    for shape in SHAPES:
        xa, xb = _image(shape, kind, 0, True)[0], _image(shape, kind, 1, True)[0]
        first = None
        for (da, fa, oa), (db, fb, ob) in ((("fp32", "nchw", 0), ("bf16", "nhwc", 0)), (("bf16", "nchw", 1), ("fp32", "nhwc", 1)),
                                           (("bf16", "nhwc", 0), ("bf16", "nchw", 0)), (("fp32", "nhwc", 0), ("fp32", "nchw", 1))):
            a, b = _place(xa, fa, PDT[da], dev, oa), _place(xb, fb, PDT[db], dev, ob)
            with _no_sync():
                got = ops.image_agreement(a, b, lo, hi)
                again = ops.image_agreement(a, b, lo, hi)
            _check_agreement(got, shape, kind, True, f"{shape} {kind} a {da}/{fa}+{oa} b {db}/{fb}+{ob}")
            assert _same_bits(got.ssim, again.ssim) and torch.equal(got.sse, again.sse)                       # two runs
            if first is None:
                first = got
            assert _same_bits(got.ssim, first.ssim) and torch.equal(got.sse, first.sse)                       # the same bytes: the same bits
        # fp32 values that bf16 does not hold: the pair in fp32 alone
        x32a, x32b = _image(shape, kind, 0, False)[0], _image(shape, kind, 1, False)[0]
        got = ops.image_agreement(_place(x32a, "nchw", torch.float32, dev), _place(x32b, "nhwc", torch.float32, dev), lo, hi)
        _check_agreement(got, shape, kind, False, f"{shape} {kind} fp32")


def test_image_agreement_takes_pictures_slices_and_itself():
    from mas_hip import ops
    dev = _dev()
    shape = (3, 4, 21, 43)
    xa, xb = _image(shape, "uniform", 0, True)[0], _image(shape, "uniform", 1, True)[0]
    a, b = _place(xa, "nchw", torch.float32, dev), _place(xb, "nhwc", torch.bfloat16, dev)
    ref = ops.image_agreement(a, b)
    with _no_sync():
        pa, pb = ops.image_bytes(a), ops.image_bytes(b)
        from_pics = ops.image_agreement(pa, pb)
        mixed = ops.image_agreement(a, pb)
        wide = torch.zeros(3, 6, 21, 43, device=dev)
        wide[:, 1:5] = a
        sliced = ops.image_agreement(wide[:, 1:5], b)
        same = ops.image_agreement(a, pa)
    for other in (from_pics, mixed, sliced):
        assert _same_bits(other.ssim, ref.ssim) and torch.equal(other.sse, ref.sse)
    assert same.sse.tolist() == [0, 0, 0] and same.ssim.tolist() == [1.0, 1.0, 1.0]
    assert bool(torch.isinf(same.psnr).all()) and bool(torch.isinf(same.pooled_psnr))
    both = ref + same
    assert len(both) == 6 and bool(torch.isfinite(both.pooled_psnr)) and bool(torch.isinf(both.mean_psnr))
    _check_agreement(ref, shape, "uniform", True, "defaults")
    with pytest.raises(ValueError, match="differ"):
        ops.image_agreement(a, b[:2])


def test_image_agreement_closed_forms():
    """constant pictures: (2ab + C1) / (a^2 + b^2 + C1), and fp64 keeps the flat bright case that fp32 sums lose (7e-5)"""
    from mas_hip import ops
    dev = _dev()
    for va, vb in ((255, 254), (0, 255), (250, 251)):
        a = torch.full((2, 40, 37, 3), va, dtype=torch.uint8, device=dev)
        b = torch.full((2, 40, 37, 3), vb, dtype=torch.uint8, device=dev)
        got = ops.image_agreement(a, b)
        want = (2.0 * va * vb + R.C1) / (va * va + vb * vb + R.C1)
        assert float((got.ssim - want).abs().max()) < 1e-12 and got.sse.tolist() == [(va - vb) ** 2 * 40 * 37 * 3] * 2


def test_image_agreement_more_tiles_than_work_groups():
    from mas_hip import ops
    dev = _dev()
    xa, xb = _image(BIG, "uniform", 0, True)[0], _image(BIG, "uniform", 1, True)[0]
    a, b = _place(xa, "nchw", torch.float32, dev), _place(xb, "nhwc", torch.bfloat16, dev, 1)
    assert mas_hip.lib().mas_img_agreement_blocks(*BIG) > 8 * torch.cuda.get_device_properties(dev).multi_processor_count
    with _no_sync():
        got = ops.image_agreement(a, b)
        again = ops.image_agreement(a, b)
    assert np.array_equal(ops.image_bytes(a).cpu().numpy(), _image(BIG, "uniform", 0, True)[1])
    _check_agreement(got, BIG, "uniform", True, "2048 x 2048")
    assert _same_bits(got.ssim, again.ssim) and torch.equal(got.sse, again.sse)


def test_a_graph_replay_gives_the_eager_bits():
    from mas_hip import ops
    dev = _dev()
    shape = (3, 4, 21, 43)
    a = _place(_image(shape, "uniform", 0, True)[0], "nhwc", torch.bfloat16, dev)
    b = _place(_image(shape, "uniform", 1, False)[0], "nchw", torch.float32, dev)
    idx = torch.randint(-2, 70, (3, 64), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def step():
        g = ops.image_agreement(a, b)
        return g.sse, g.ssim, ops.code_usage(idx, 64).counts

    eager = step()
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        step()                                                       # warm-up on the capture stream
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        held = step()
    main.wait_stream(side)
    for _ in range(2):
        held[0].fill_(-1)
        held[1].fill_(7.0)
        held[2].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(held[0], eager[0]) and _same_bits(held[1], eager[1]) and torch.equal(held[2], eager[2])
    assert np.array_equal(eager[2].cpu().numpy(), R.code_usage(idx.cpu().numpy(), 64))


# ---- codebook usage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idt", ["int64", "int32"])
@pytest.mark.parametrize("k", [1, 7, 8192, mas_hip.CODE_USAGE_LDS_BINS - 1, mas_hip.CODE_USAGE_LDS_BINS, mas_hip.CODE_USAGE_LDS_BINS + 5])
def test_code_usage_counts(k, idt):
    from mas_hip import ops
    dev = _dev()
    dt = torch.int64 if idt == "int64" else torch.int32
    outside = [-1, k, 2 ** 40, -2 ** 40, k + 1] if idt == "int64" else [-1, k, 2 ** 31 - 1, -2 ** 31, k + 1]
    for n in (1, 255, 256, 257, 2 ** 20):
        rs = np.random.RandomState(k % 1000 + n % 1000)
        idx = rs.randint(0, k, n).astype(np.int64)
        if n > 1:
            idx[rs.randint(0, n, max(1, n // 50))] = k - 1                            # the last code is used
            pos = rs.randint(0, n, max(5, n // 20))
            idx[pos] = np.array(outside, dtype=np.int64)[np.arange(pos.size) % len(outside)]
        else:
            idx[0] = outside[2]
        want = R.code_usage(idx, k)
        assert want[-1] > 0 and want.sum() == n
        t = torch.from_numpy(idx).to(dev).to(dt) if idt == "int64" else torch.from_numpy(idx.astype(np.int32)).to(dev)
        t = t.view(-1, 1) if n % 2 else t.view(2, -1)                                 # any shape
        with _no_sync():
            got = ops.code_usage(t, k)
            held = got.counts
            twice = ops.code_usage(t, k, out=got)
        assert isinstance(got, CodeUsage) and twice is got and got.counts is held and got.counts.dtype == torch.int64
        assert tuple(got.counts.shape) == (k + 1,)
        assert np.array_equal(got.counts.cpu().numpy(), 2 * want), (k, n, idt)
        once = ops.code_usage(t, k)
        assert np.array_equal(once.counts.cpu().numpy(), want), (k, n, idt)
        assert int(once.total) == want[:-1].sum() and int(once.out_of_range) == want[-1]
        assert int(once.used) == np.count_nonzero(want[:-1]) and int(once.dead) == k - np.count_nonzero(want[:-1])
        if want[:-1].sum() > 0:
            p, wp = float(once.perplexity), R.perplexity(want)
            assert abs(p - wp) <= 1e-12 * wp, (k, n, p, wp)


# ---- model ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(PDT))
def test_model_pictures_and_reconstruction_metrics(mode):
    from mas_hip import ops
    from oracle.vq_oracle import synth_image_batch
    from test_gpu_model import TINY, _build
    dev = _dev()
    old = ops.compute_dtype()
    try:
        m = _build(TINY, 3, PDT[mode], train=False)
        x = synth_image_batch(3, 3, 32, seed=5).to(dev)
        tokens = m.encode_to_indices(x)
        with torch.no_grad():
            dec = m.decode_code(tokens)
            rec = m(x)[0]
        pics = m.decode_to_images(tokens)
        assert pics.dtype == torch.uint8 and tuple(pics.shape) == (3, 32, 32, 3) and pics.is_contiguous()
        assert np.array_equal(pics.cpu().numpy(), R.to_bytes(dec.float().cpu().numpy()))
        assert np.array_equal(m.decode_to_images(tokens, -2.0, 2.0).cpu().numpy(), R.to_bytes(dec.float().cpu().numpy(), -2.0, 2.0))
        with _no_sync():
            agree, usage = m.reconstruction_metrics(x)
        ra, rb = R.to_bytes(rec.float().cpu().numpy()), R.to_bytes(x.float().cpu().numpy())
        assert np.array_equal(agree.sse.cpu().numpy(), R.sse(ra, rb))
        err = float(np.abs(agree.ssim.cpu().numpy() - R.ssim(ra, rb)).max())
        print(f"{mode}: ssim {agree.ssim.tolist()} psnr {agree.psnr.tolist()} |ssim - helper| {err:.3e}")
        assert err <= SSIM_TOL and agree.elements.tolist() == [3 * 32 * 32] * 3
        want_counts = R.code_usage(tokens.cpu().numpy(), TINY["n_embed"])
        assert isinstance(usage, CodeUsage) and np.array_equal(usage.counts.cpu().numpy(), want_counts) and int(usage.out_of_range) == 0
        assert int(usage.total) == tokens.numel() and abs(float(usage.perplexity) - R.perplexity(want_counts)) <= 1e-12 * R.perplexity(want_counts)
        _, usage2 = m.reconstruction_metrics(x, usage=usage)
        assert usage2 is usage and np.array_equal(usage.counts.cpu().numpy(), 2 * want_counts)
        m.train()
        with pytest.raises(RuntimeError, match="eval"):
            m.decode_to_images(tokens)
        with pytest.raises(RuntimeError, match="eval"):
            m.reconstruction_metrics(x)
    finally:
        ops.set_compute_dtype(old)
