"""VQ-SEG logits back to label planes on the GPU (csrc/seg_classify.hip): ``ops.seg_classify`` bit for bit against the numpy
restatement of the rule (tests/helpers/seg_classify_ref.py) -- no exclusions, the rule is exact --, ``ops.seg_agreement`` against
brute-force numpy counts, repeatability and graph capture, and ``VQBASE.decode_to_labels`` / ``reconstruct_labels``.

Shapes: the issue's eight, among them ``mas_hip.SEG_LABELS_TILE`` minus one, exactly, plus one, and two for this kernel's own steps:
(1, 40, 52) = 2080 pixels is more than one work-group of 16-byte lanes (256 lanes x 4 fp32 / x 8 bf16 pixels), and several NHWC tiles plus
a part; (1, 725, 725), with the six-channel layout only, is more pixels than the largest grid has lanes (8 work-groups per CU x 256 CUs x
256 one-pixel lanes; H W odd takes the one-pixel kernels), so lanes and NHWC work-groups go round their loops more than once, in
``seg_agreement`` as well.  H W a multiple of 4 (8) takes the 16-byte NCHW kernel for fp32 (bf16) when the base pointer allows."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import seg_classify_ref as CR  # noqa: E402
import seg_labels_ref as LR  # noqa: E402
import mas_hip  # noqa: E402
import seg_data  # noqa: E402
from mas_hip.seglabels import SegAgreement, SegLabels, SegLayout  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = mas_hip.SEG_LABELS_TILE
LAYOUTS = {"reference": (SegLayout(), (None, None, 0.2, 0.2)),
           "c6": (SegLayout(groups=(3, 2), value_channels=1), (0.5, None, 0.2)),                  # 0.5: tau = 0 lies ON the logits' grid
           "wide": (SegLayout(groups=(4, 3, 2, 2, 2), value_channels=2), (None, 0.2, 0.5, None, 0.7, 0.5, None)),
           "g255": (SegLayout(groups=(255,), value_channels=0), (0.5,)),
           "values": (SegLayout(groups=(), value_channels=2), (0.5, None))}
SHAPES = [(1, 1, 1), (2, 3, 5), (3, 7, 33), (1, 16, 16), (2, 24, 24), (1, 1, TILE - 1), (1, 1, TILE), (1, 1, TILE + 1), (1, 40, 52)]
BIG = (1, 725, 725)
PDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _logits(lname, bhw, kind, bf16):
    """-> (x float32 numpy NCHW, the helper's planes); computed once.  ties: multiples of 0.5 at scale 4, the reference layout's face group
    moved by -3; hard: to +-150 with +-inf"""
    key = (lname, bhw, kind, bf16)
    if key not in _cache:
        lay, thr = LAYOUTS[lname]
        shape = (bhw[0], lay.channels, bhw[1], bhw[2])
        seed = 11 + 7 * bhw[0] + bhw[1] * bhw[2] + lay.channels
        if kind == "ties":
            x = CR.tie_rich_logits(shape, lay.groups, lay.value_channels, thr, 4.0, seed, bf16=bf16, shift_group=2 if lname == "reference" else None)
        else:
            x = CR.hard_logits(shape, seed)
            assert np.isinf(x).any() or x.size < 13
            if bf16:
                x = torch.from_numpy(x).bfloat16().float().numpy()
        _cache[key] = (x, CR.classify(x, lay.groups, lay.value_channels, thr))
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


def _classify_check(lname, bhw, kind, fmt, dtype, offset=0):
    from mas_hip import ops
    dev = _dev()
    lay, thr = LAYOUTS[lname]
    x, want = _logits(lname, bhw, kind, dtype == torch.bfloat16)
    xv = _place(x, fmt, dtype, dev, offset)
    before = xv.clone()
    guard = torch.full((64,), 7, dtype=torch.uint8, device=dev)
    got = ops.seg_classify(xv, lay, thr)
    torch.cuda.synchronize()
    assert isinstance(got, SegLabels) and got.layout == lay and got.planes.dtype == torch.uint8 and got.planes.is_contiguous()
    assert tuple(got.planes.shape) == (bhw[0], lay.planes, bhw[1], bhw[2]) and tuple(got.shape) == tuple(xv.shape)
    g = got.planes.cpu().numpy()
    tag = f"{lname} {bhw} {kind} {fmt}/{str(dtype)[6:]} off={offset}"
    assert np.array_equal(g, want), (tag, int((g != want).sum()))
    for k, size in enumerate(lay.groups + (1,) * lay.value_channels):
        assert int(g[:, k].max()) <= size, tag
    assert torch.equal(xv, before) and int(guard.min()) == 7 and int(guard.max()) == 7
    return g


@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
@pytest.mark.parametrize("pdt", list(PDT))
@pytest.mark.parametrize("lname", list(LAYOUTS))
def test_seg_classify_is_bit_exact(lname, pdt, fmt):
    seen = set()
    for bhw in SHAPES:
        for kind in ("ties", "hard"):
            seen |= set(np.unique(_classify_check(lname, bhw, kind, fmt, PDT[pdt])[:, 0]))
    lay = LAYOUTS[lname][0]
    if lay.groups:
        assert {1, lay.groups[0]} <= seen, "the first and the last class of the first group occur"
    if lname == "c6":
        assert 0 in seen                                             # gated at 0.5


@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
def test_seg_classify_more_pixels_than_the_grid_has_lanes(fmt):
    _classify_check("c6", BIG, "ties", fmt, torch.float32)


@pytest.mark.parametrize("pdt", list(PDT))
def test_seg_classify_base_pointer_aligned_to_one_element_only(pdt):
    """the prediction starts one element past a 16-byte boundary, with H W = 35 and with H W = 64 and 2080 (which would take 16-byte lanes)"""
    for fmt in ("nchw", "nhwc"):
        for bhw in ((3, 5, 7), (1, 8, 8), (1, 40, 52)):
            _classify_check("reference", bhw, "ties", fmt, PDT[pdt], offset=1)
    _classify_check("reference", (3, 5, 7), "hard", "nhwc", PDT[pdt], offset=3)


def test_seg_classify_takes_the_reference_defaults_a_slice_and_from_logits():
    from mas_hip import ops
    dev = _dev()
    x, want = _logits("reference", (2, 24, 24), "ties", False)
    xv = torch.from_numpy(x).to(dev)
    assert np.array_equal(ops.seg_classify(xv).planes.cpu().numpy(), want)                   # (None, None, 0.2, 0.2)
    assert np.array_equal(SegLabels.from_logits(xv).planes.cpu().numpy(), want)
    assert np.array_equal(SegLabels.from_logits(xv.cpu()).planes.numpy(), want)
    wide = torch.zeros(2, 170, 24, 24, device=dev)
    wide[:, 5:164] = xv
    assert np.array_equal(ops.seg_classify(wide[:, 5:164]).planes.cpu().numpy(), want)       # neither dense layout: made dense first
    one = ops.seg_classify(xv, None, 0.2).planes.cpu().numpy()
    assert np.array_equal(one, CR.classify(x, (133, 20, 5), 1, (0.2,) * 4))


def test_seg_classify_with_nan_stays_in_range():
    """the byte of a group that holds a NaN is unspecified, but within 0 .. S; groups without one are exact"""
    from mas_hip import ops
    dev = _dev()
    lay, thr = LAYOUTS["c6"]
    x, _ = _logits("c6", (2, 24, 24), "ties", False)
    x = x.copy()
    x[:, 1][..., ::3] = np.nan                                       # only the first group
    x[0, 0, 0, :5] = np.nan
    want = CR.classify(x, lay.groups, lay.value_channels, thr)
    for fmt in ("nchw", "nhwc"):
        g = ops.seg_classify(_place(x, fmt, torch.float32, dev), lay, thr).planes.cpu().numpy()
        assert int(g[:, 0].max()) <= 3 and np.array_equal(g[:, 1:], want[:, 1:])


# ---- agreement ------------------------------------------------------------------------------------------------------------------------
def _planes(lname, bhw, seed):
    """seeded label planes: every class, "none", bytes above the group's size, edge values 0 .. 2"""
    key = ("planes", lname, bhw, seed)
    if key not in _cache:
        lay = LAYOUTS[lname][0]
        b, h, w = bhw
        rs = np.random.RandomState(500 * seed + 31 * b + 7 * h + w + lay.channels)
        planes = np.zeros((b, lay.planes, h, w), dtype=np.uint8)
        for k, g in enumerate(lay.groups):
            v = rs.randint(0, min(g, 6) + 1, (b, h, w))             # few classes: intersections are frequent
            v = np.where(rs.rand(b, h, w) < 0.1, rs.randint(0, g + 1, (b, h, w)), v)
            if g < 255:
                v = np.where(rs.rand(b, h, w) < 0.05, rs.randint(g + 1, 256, (b, h, w)), v)
            planes[:, k] = v
        for k in range(lay.value_channels):
            planes[:, len(lay.groups) + k] = rs.randint(0, 3, (b, h, w))
        _cache[key] = planes
    return _cache[key]


def _agreement_check(lname, bhw):
    from mas_hip import ops
    dev = _dev()
    lay = LAYOUTS[lname][0]
    p, t = _planes(lname, bhw, 1), _planes(lname, bhw, 2)
    want = CR.agreement_counts(p, t, lay.groups, lay.value_channels)
    pl, tl = SegLabels(torch.from_numpy(p), lay).to(dev), SegLabels(torch.from_numpy(t), lay).to(dev)
    a = ops.seg_agreement(pl, tl)
    assert isinstance(a, SegAgreement) and a.counts.dtype == torch.int64 and a.counts.is_cuda
    assert np.array_equal(a.counts.cpu().numpy(), want), (lname, bhw)
    assert int(a.pixels) == bhw[0] * bhw[1] * bhw[2] and int(a.counts.max()) <= int(a.pixels)
    return a, want, pl, tl


@pytest.mark.parametrize("lname", list(LAYOUTS))
def test_seg_agreement_counts(lname):
    for bhw in SHAPES:
        _agreement_check(lname, bhw)
    p, t = _planes(lname, (2, 24, 24), 1), _planes(lname, (2, 24, 24), 2)
    lay = LAYOUTS[lname][0]
    if lay.groups and lay.groups[0] < 255:
        assert (p[:, 0] > lay.groups[0]).any() and (t[:, 0] > lay.groups[0]).any()           # bytes above the group's size are present
    if lay.value_channels:
        assert (t[:, -1] == 2).any()                                                         # and the edge value 2


def test_seg_agreement_more_pixels_than_the_grid_has_lanes():
    a, want, _, _ = _agreement_check("c6", BIG)
    iou = a.iou.cpu().numpy()
    c = 6
    assert np.allclose(iou, want[:c] / (want[c:2 * c] + want[2 * c:3 * c] - want[:c]), rtol=0, atol=0)


def test_seg_agreement_accumulates_and_derives_the_metrics():
    """two batches into one buffer = the counts of their concatenation; a prediction against itself agrees everywhere"""
    from mas_hip import ops
    dev = _dev()
    lay = LAYOUTS["reference"][0]
    a1, w1, p1, t1 = _agreement_check("reference", (2, 24, 24))
    _, w2, p2, t2 = _agreement_check("reference", (3, 7, 33))
    acc = SegAgreement(lay, device=dev)
    held = acc.counts
    assert ops.seg_agreement(p1, t1, out=acc) is acc
    ops.seg_agreement(p2, t2, out=acc)
    assert acc.counts is held and np.array_equal(acc.counts.cpu().numpy(), w1 + w2)
    both = (a1 + ops.seg_agreement(p2, t2)).counts.cpu().numpy()
    assert np.array_equal(both, w1 + w2)
    same = ops.seg_agreement(p1, p1)
    assert bool((same.pixel_accuracy == 1.0).all())
    iou = same.iou.cpu().numpy()
    assert np.all((iou == 1.0) | np.isnan(iou)) and np.isnan(iou).any() and bool((same.miou == 1.0).all())
    acc2 = a1.pixel_accuracy.cpu().numpy()
    assert np.array_equal(acc2, w1[3 * 159:3 * 159 + 4] / w1[-1])
    with pytest.raises(ValueError, match="seg_agreement"):
        ops.seg_agreement(p1, t2)
    with pytest.raises(ValueError, match="seg_agreement"):
        ops.seg_agreement(p1, t1, out=SegAgreement(LAYOUTS["c6"][0], device=dev))


def test_seg_agreement_of_one_concatenated_batch():
    """the same H W: accumulating two batches equals counting the concatenated batch in one call"""
    from mas_hip import ops
    dev = _dev()
    lay = LAYOUTS["wide"][0]
    pa, ta = _planes("wide", (2, 24, 24), 1), _planes("wide", (2, 24, 24), 2)
    pb, tb = _planes("wide", (2, 24, 24), 3), _planes("wide", (2, 24, 24), 4)
    mk = lambda a: SegLabels(torch.from_numpy(a), lay).to(dev)
    acc = ops.seg_agreement(mk(pb), mk(tb), out=ops.seg_agreement(mk(pa), mk(ta)))
    whole = ops.seg_agreement(mk(np.concatenate([pa, pb])), mk(np.concatenate([ta, tb])))
    assert torch.equal(acc.counts, whole.counts) and int(whole.pixels) == 4 * 576
    assert np.array_equal(whole.counts.cpu().numpy(), CR.agreement_counts(np.concatenate([pa, pb]), np.concatenate([ta, tb]), lay.groups, 2))


# ---- repeatability ------------------------------------------------------------------------------------------------------------------
def test_two_evaluations_and_a_graph_replay_give_identical_bytes_and_counts():
    from mas_hip import ops
    dev = _dev()
    lay, thr = LAYOUTS["reference"]
    x, want = _logits("reference", (2, 24, 24), "ties", False)
    target = SegLabels(torch.from_numpy(_planes("reference", (2, 24, 24), 2)), lay).to(dev)
    for fmt in ("nchw", "nhwc"):
        xv = _place(x, fmt, torch.float32, dev)

        def step():
            lab = ops.seg_classify(xv, lay, thr)
            return lab.planes, ops.seg_agreement(lab, target).counts

        e_planes, e_counts = step()
        r_planes, r_counts = step()
        assert torch.equal(e_planes, r_planes) and torch.equal(e_counts, r_counts)
        assert np.array_equal(e_planes.cpu().numpy(), want)
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            step()                                                   # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            g_planes, g_counts = step()
        main.wait_stream(side)
        for _ in range(2):
            g_planes.fill_(9)
            g_counts.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(g_planes, e_planes) and torch.equal(g_counts, e_counts)


# ---- model ------------------------------------------------------------------------------------------------------------------------------
def _tiny_seg(dtype):
    from test_gpu_model import TINY, _build
    cfg = dict(TINY, ddconfig=dict(TINY["ddconfig"], in_channels=159, out_channels=159))
    return _build(cfg, 3, dtype, train=False)


@pytest.mark.parametrize("mode", list(PDT))
def test_model_decodes_and_reconstructs_labels(mode):
    from mas_hip import ops
    dev = _dev()
    old = ops.compute_dtype()
    try:
        m = _tiny_seg(PDT[mode])
        labels = SegLabels(torch.stack([seg_data.planes_from_arrays(*LR.sample_arrays(16, 16, seed=20 + s)) for s in range(2)])).to(dev)
        idx = m.encode_to_indices(labels)
        got = m.decode_to_labels(idx)
        with torch.no_grad():
            logits = m.decode_code(idx)
        assert isinstance(got, SegLabels) and got.planes.is_cuda and tuple(got.planes.shape) == (2, 4, 16, 16)
        want = CR.classify(logits.float().cpu().numpy(), (133, 20, 5), 1, CR.REFERENCE_THRESHOLDS)
        assert np.array_equal(got.planes.cpu().numpy(), want)
        rec = m.reconstruct_labels(labels)
        assert isinstance(rec, SegLabels) and rec.planes.is_cuda and tuple(rec.planes.shape) == (2, 4, 16, 16)
        a = ops.seg_agreement(rec, labels)
        assert int(a.pixels) == 2 * 16 * 16 and int(a.counts.max()) <= int(a.pixels) and int(a.counts.min()) >= 0
        assert tuple(rec.colorize().shape) == (2, 4, 3, 16, 16) and rec.colorize().is_cuda
        m.train()
        with pytest.raises(RuntimeError, match="eval"):
            m.decode_to_labels(idx)
    finally:
        ops.set_compute_dtype(old)


def test_nothing_of_the_logits_size_is_allocated():
    """[4, 159, 64, 64] fp32: the peak rises by the planes and a small workspace; asserted below one quarter of the logits' bytes"""
    from mas_hip import ops
    dev = _dev()
    for fmt in ("nchw", "nhwc"):
        x = torch.randn(4, 159, 64, 64, device=dev)
        if fmt == "nhwc":
            x = x.contiguous(memory_format=torch.channels_last)
        ops.seg_classify(x)                                          # (library load, first launch)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        lab = ops.seg_classify(x)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        print(f"x {fmt}: peak rise {rise} bytes, planes {lab.planes.numel()} bytes, logits {x.numel() * 4} bytes")
        assert lab.planes.numel() <= rise < x.numel() * 4 // 4, (rise, x.numel() * 4)
