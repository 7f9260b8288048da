"""The compact VQ-SEG input on the GPU (csrc/seg_labels.hip): ``ops.seg_expand`` bit for bit against ``SegLabels.dense()`` on the CPU,
``ops.seg_loss_labels`` on the yardstick of tests/test_gpu_seg_loss.py, and ``VQBASE`` / the loss classes / ``tokenize_batch`` fed
labels against the same objects fed the dense map.

Loss bounds (DESIGN 2.10's table, restated).  The reference is the float64 restatement tests/helpers/seg_loss_ref.py fed the densified
labels; y = the deviation of torch's own fp32 CPU evaluation of the same expression from it; S = max(pos_weight) |g| / n:
  loss and each returned term   |error| <= max(4 y_loss, 4 * 2^-23 * max(1, |ref|))
  fp32 gradient, per element    |error| <= max(4 y_dx, 8 * 2^-24 * S)
  bf16 gradient, per element    |error| <= 2^-8 |ref| + 8 * 2^-24 * S
Shapes: the issue's five, and the kernel's own pixel tile (``mas_hip.SEG_LABELS_TILE``) minus one, exactly, plus one.  H W a multiple of
4 (8) takes the 16-byte NCHW kernels for fp32 (bf16), anything else the one-pixel-per-lane ones; an NHWC prediction always walks 16-byte
units with head and tail."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import seg_loss_ref as R  # noqa: E402
import seg_labels_ref as LR  # noqa: E402
import mas_hip  # noqa: E402
import seg_data  # noqa: E402
from mas_hip.seglabels import SegLabels, SegLayout  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = mas_hip.SEG_LABELS_TILE
DEFAULT = SegLayout()
C6 = SegLayout(groups=(3, 2), value_channels=1)                  # C = 6: padded to 8
C8 = SegLayout(groups=(5, 2), value_channels=1)                  # C = 8: no padding
WIDE = SegLayout(groups=(4, 3, 2, 2, 2), value_channels=2)       # seven planes, C = 15: the kernels' eight-entry instances
PDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _labels(b, h, w, layout=DEFAULT, seed=0) -> SegLabels:
    """seeded CPU labels: every class of every group, "none", values above the group's size (they set nothing), edge values 0 .. 2"""
    key = ("lab", b, h, w, layout, seed)
    if key not in _cache:
        rs = np.random.RandomState(1000 * seed + 31 * b + 7 * h + w + layout.channels)
        planes = np.zeros((b, layout.planes, h, w), dtype=np.uint8)
        for k, g in enumerate(layout.groups):
            v = rs.randint(0, g + 1, (b, h, w))
            v = np.where(rs.rand(b, h, w) < 0.05, rs.randint(g + 1, 256, (b, h, w)), v)      # above the group's size
            planes[:, k] = v
            planes[0, k].reshape(-1)[k % (h * w)] = g                                        # the group's largest class (a view: written in place)
        for k in range(layout.value_channels):
            planes[:, len(layout.groups) + k] = rs.randint(0, 3, (b, h, w))
        _cache[key] = SegLabels(torch.from_numpy(planes), layout)
    return _cache[key]


# ---- expand ---------------------------------------------------------------------------------------------------------------------------
EXPAND_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 7, 33), (1, 16, 16)]
EXPAND_CASES = [("default-nhwc-bf16-160", DEFAULT, torch.bfloat16, True, 160), ("default-nhwc-fp32-160", DEFAULT, torch.float32, True, 160),
                ("default-nchw-fp32-159", DEFAULT, torch.float32, False, None), ("c6-nhwc-bf16-8", C6, torch.bfloat16, True, 8),
                ("c6-nhwc-fp32-8", C6, torch.float32, True, 8), ("c8-nhwc-bf16-8", C8, torch.bfloat16, True, None),
                ("c8-nchw-fp32-8", C8, torch.float32, False, None), ("default-nhwc-fp32-159", DEFAULT, torch.float32, True, None),
                ("default-nchw-bf16-159", DEFAULT, torch.bfloat16, False, None), ("wide-nhwc-bf16-24", WIDE, torch.bfloat16, True, 24),
                ("wide-nchw-fp32-15", WIDE, torch.float32, False, None)]


@pytest.mark.parametrize("name,layout,dtype,cl,pad_to", EXPAND_CASES, ids=[c[0] for c in EXPAND_CASES])
@pytest.mark.parametrize("bhw", EXPAND_SHAPES, ids=["x".join(map(str, s)) for s in EXPAND_SHAPES])
def test_seg_expand_is_bit_exact(bhw, name, layout, dtype, cl, pad_to):
    from mas_hip import ops
    dev = _dev()
    lab = _labels(*bhw, layout=layout)
    ref = lab.dense()                                            # CPU, fp32 NCHW
    c = layout.channels
    assert set(np.unique(ref.numpy())) <= {0.0, 1.0, 2.0}
    guard = torch.full((64,), 7.0, device=dev)                   # (allocated around the output: a stray write would land near here)
    out = ops.seg_expand(lab.to(dev), dtype=dtype, channels_last=cl, pad_to=pad_to)
    torch.cuda.synchronize()
    cp = pad_to or c
    assert out.dtype == dtype and tuple(out.shape) == (bhw[0], cp, bhw[1], bhw[2])
    assert out.is_contiguous(memory_format=torch.channels_last) if cl else out.is_contiguous()
    got = out.float().cpu()
    assert torch.equal(got[:, :c], ref), name
    assert cp == c or float(got[:, c:].abs().max()) == 0.0       # pad channels: exact zeros
    assert float(guard.min()) == 7.0 and float(guard.max()) == 7.0


def test_seg_expand_dense_on_gpu_labels_and_label_above_group_size():
    dev = _dev()
    planes = torch.zeros(1, 4, 2, 3, dtype=torch.uint8)
    planes[0, 2, 0, 0] = 200                                     # face plane, five classes: sets nothing
    planes[0, 0, 1, 2] = 255
    planes[0, 2, 1, 1] = 5
    planes[0, 3, 0, 2] = 2
    lab = SegLabels(planes)
    for dtype in (torch.float32, torch.bfloat16):
        for mf in (torch.contiguous_format, torch.channels_last):
            got = lab.to(dev).dense(dtype, memory_format=mf)
            assert got.is_cuda and got.dtype == dtype and got.is_contiguous(memory_format=mf) and tuple(got.shape) == (1, 159, 2, 3)
            assert torch.equal(got.float().cpu(), lab.dense())
    d = lab.to(dev).dense().cpu()
    assert float(d.sum()) == 3.0 and float(d[0, 157, 1, 1]) == 1.0 and float(d[0, 158, 0, 2]) == 2.0


def test_seg_expand_errors_name_the_op():
    from mas_hip import ops
    dev = _dev()
    lab = _labels(1, 2, 2).to(dev)
    with pytest.raises((ValueError, RuntimeError), match="seg_expand"):
        ops.seg_expand(lab, dtype=torch.float16)
    with pytest.raises((ValueError, RuntimeError), match="seg_expand"):
        ops.seg_expand(lab, dtype=torch.float32, pad_to=158)
    with pytest.raises((ValueError, RuntimeError), match="seg_expand"):
        ops.seg_expand(lab.cpu(), dtype=torch.float32)
    with pytest.raises(TypeError, match="seg_expand"):
        ops.seg_expand(lab.dense(), dtype=torch.float32)


# ---- loss -----------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(2, 159, 8, 8), (3, 159, 5, 7), (1, 159, 1, 1), (1, 8, 9, 9), (2, 159, 64, 64),
               (1, 159, 1, TILE - 1), (1, 159, 1, TILE), (2, 159, 1, TILE + 1)]


def _layout_of(c):
    return {159: DEFAULT, 8: C8, 6: C6, 15: WIDE}[c]


def _weight(c):
    if c == 159:
        return R.module_weight().astype(np.float32)
    return np.random.RandomState(100 + c).uniform(0.5, 3.0, c).astype(np.float32)


def _inputs(shape, kind):
    """-> (x float32 numpy NCHW, labels on the CPU, their dense map as numpy).  plain: logits 2 randn; bf16: those rounded to bf16; hard:
    every 7th element x 20 (|x| up to about 150) and exact zeros, as the dense op's hard case; hardbf16: that rounded to bf16"""
    key = ("in", shape, kind)
    if key not in _cache:
        n, c, h, w = shape
        lab = _labels(n, h, w, layout=_layout_of(c), seed=1)
        rs = np.random.RandomState(7 + n + c + h * w)
        x = (2.0 * rs.randn(n, c, h, w)).astype(np.float32)
        if kind in ("hard", "hardbf16"):
            flat = x.reshape(-1)
            flat[::7] *= 20.0
            flat[3::11] = 0.0
            assert np.abs(x).max() > 100.0
        if kind in ("bf16", "hardbf16"):
            x = torch.from_numpy(x).bfloat16().float().numpy()
        _cache[key] = (x, lab, lab.dense().numpy())
    return _cache[key]


def _reference(shape, kind, mse, g=1.0):
    """-> fp64 (loss, bce_mean, mse_mean, dx), the yardsticks (y_loss, y_dx) of torch's fp32 CPU evaluation, and S; computed once"""
    key = ("ref", shape, kind, mse, g)
    if key not in _cache:
        x, _, t = _inputs(shape, kind)
        w = _weight(shape[1])
        ref = R.seg_loss_ref(x, t, w, mse, g)
        xt = torch.from_numpy(x).requires_grad_(True)
        tt = torch.from_numpy(t)
        loss = F.binary_cross_entropy_with_logits(xt.movedim(1, -1), tt.movedim(1, -1), pos_weight=torch.from_numpy(w))
        if mse:
            loss = F.mse_loss(torch.sigmoid(xt), tt) + loss
        loss.backward(torch.tensor(float(g)))
        y_loss = abs(float(loss.detach()) - ref[0])
        y_dx = float(np.abs(xt.grad.double().numpy() - ref[3]).max())
        _cache[key] = (ref, y_loss, y_dx, float(w.max()) * abs(g) / x.size)
    return _cache[key]


def _place(a, layout, dtype, dev, offset=0):
    """logical NCHW numpy -> device tensor of `dtype`, dense in `layout`; offset: that many elements past an allocation's start"""
    n, c, h, w = a.shape
    src = torch.from_numpy(a).to(dev).to(dtype)
    buf = torch.zeros(a.size + offset + 64, dtype=dtype, device=dev)
    if layout == "nhwc":
        v = buf[offset:offset + a.size].view(n, h, w, c).permute(0, 3, 1, 2)
    else:
        v = buf[offset:offset + a.size].view(n, c, h, w)
    v.copy_(src)
    assert v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


def _is_layout(v, layout):
    return v.is_contiguous(memory_format=torch.channels_last) if layout == "nhwc" else v.is_contiguous()


def _loss_bound(y_loss, ref):
    return max(4 * y_loss, 4 * 2.0 ** -23 * max(1.0, abs(ref)))


def _check(shape, kind, mse, xl, pdt=torch.float32, offset=0, g=1.0):
    from mas_hip import ops
    dev = _dev()
    x, lab, _ = _inputs(shape, kind)
    (ref_loss, ref_bce, ref_mse, ref_dx), y_loss, y_dx, S = _reference(shape, kind, mse, g)
    xv = _place(x, xl, pdt, dev, offset).requires_grad_(True)
    w = torch.from_numpy(_weight(shape[1])).to(dev)
    before = xv.detach().clone()
    loss, terms = ops.seg_loss_labels(xv, lab.to(dev), w, mse=mse, return_terms=True)
    (g * loss).backward()
    assert loss.dtype == torch.float32 and loss.shape == () and not terms["bce_mean"].requires_grad
    dx = xv.grad
    assert dx.dtype == pdt and dx.shape == xv.shape and dx.stride() == xv.stride() and _is_layout(dx, xl)
    assert torch.equal(xv.detach(), before)
    e_loss = abs(float(loss.detach()) - ref_loss)
    e_bce, e_mse = abs(float(terms["bce_mean"]) - ref_bce), abs(float(terms["mse_mean"]) - ref_mse)
    d = np.abs(dx.double().cpu().numpy() - ref_dx)
    tag = f"{shape} {kind} mse={int(mse)} x:{xl}/{str(pdt)[6:]} off={offset} g={g}"
    print(f"{tag}: loss err {e_loss:.2e} (torch fp32 {y_loss:.2e}), grad err {d.max():.2e} (torch fp32 {y_dx:.2e}; S {S:.2e})")
    assert np.isfinite(float(loss.detach())) and np.isfinite(d).all(), tag
    assert e_loss <= _loss_bound(y_loss, ref_loss), (tag, e_loss, y_loss)
    assert e_bce <= _loss_bound(y_loss, ref_bce) and e_mse <= _loss_bound(y_loss, ref_mse), (tag, e_bce, e_mse)
    if pdt == torch.float32:
        assert (d <= max(4 * y_dx, 8 * 2.0 ** -24 * S)).all(), (tag, float(d.max()), y_dx, S)
    else:
        assert (d <= 2.0 ** -8 * np.abs(ref_dx) + 8 * 2.0 ** -24 * S).all(), (tag, float(d.max()))


@pytest.mark.parametrize("mse", [False, True], ids=["bce", "bce+mse"])
@pytest.mark.parametrize("pdt", list(PDT), ids=["x_%s" % k for k in PDT])
@pytest.mark.parametrize("xl", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["x".join(map(str, s)) for s in LOSS_SHAPES])
def test_seg_loss_labels_vs_fp64(shape, xl, pdt, mse):
    _check(shape, "bf16" if pdt == "bf16" else "plain", mse, xl, PDT[pdt])


@pytest.mark.parametrize("xl", ["nchw", "nhwc"])
def test_seg_loss_labels_seven_planes(xl):
    """more than four planes: the kernels' eight-entry instances"""
    for pdt, kind in ((torch.float32, "plain"), (torch.bfloat16, "bf16")):
        _check((2, 15, 8, 8), kind, True, xl, pdt)
        _check((1, 15, 5, 7), kind, True, xl, pdt)


@pytest.mark.parametrize("xl", ["nchw", "nhwc"])
def test_seg_loss_labels_hard_inputs_stay_finite(xl):
    """|x| up to about 150 and exact zeros: loss and every gradient element finite (asserted in _check), and within the bounds"""
    for mse in (False, True):
        _check(LOSS_SHAPES[0], "hard", mse, xl)
    _check(LOSS_SHAPES[0], "hardbf16", True, xl, torch.bfloat16)


@pytest.mark.parametrize("pdt", list(PDT), ids=["x_%s" % k for k in PDT])
def test_seg_loss_labels_base_pointer_aligned_to_one_element_only(pdt):
    """the prediction starts one element past a 16-byte boundary (4 bytes for fp32, 2 for bf16), with H W = 35 and with H W = 64"""
    for xl in ("nchw", "nhwc"):
        _check((3, 159, 5, 7), "bf16", True, xl, PDT[pdt], offset=1)
        _check((2, 159, 8, 8), "bf16", True, xl, PDT[pdt], offset=1)
    _check((3, 159, 5, 7), "bf16", True, "nhwc", PDT[pdt], offset=3)


@pytest.mark.parametrize("xl", ["nchw", "nhwc"])
def test_upstream_gradient_scales_dx(xl):
    _check(LOSS_SHAPES[1], "plain", True, xl, g=3.0)
    _check(LOSS_SHAPES[0], "plain", True, xl, g=-0.5)


@pytest.mark.parametrize("xl", ["nchw", "nhwc"])
def test_two_evaluations_give_identical_bits_and_match_the_dense_op(xl):
    """the bits repeat (asserted); and, printed for DESIGN 2.11 and not asserted, whether dx equals the dense op's bit for bit"""
    from mas_hip import ops
    dev = _dev()
    shape = LOSS_SHAPES[4]
    x, lab, t = _inputs(shape, "plain")
    w = torch.from_numpy(_weight(159)).to(dev)
    outs = []
    for _ in range(2):
        xv = _place(x, xl, torch.float32, dev).requires_grad_(True)          # fresh copies
        loss = ops.seg_loss_labels(xv, lab.to(dev), w, mse=True)
        loss.backward()
        outs.append((loss.detach().clone(), xv.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][0])) and outs[0][1].abs().sum() > 0
    xv = _place(x, xl, torch.float32, dev).requires_grad_(True)
    dense_loss = ops.seg_loss(xv, torch.from_numpy(t).to(dev), w, mse=True)
    dense_loss.backward()
    print(f"x {xl}: dx bit-identical to ops.seg_loss on the dense target: {torch.equal(xv.grad, outs[0][1])}; "
          f"loss {float(outs[0][0]):.9g} against {float(dense_loss.detach()):.9g}")


def test_forward_and_backward_capture_into_a_graph():
    """forward + backward captured once on a side stream, replayed twice: the eager bits each time (no host synchronisation anywhere)"""
    from mas_hip import ops
    dev = _dev()
    x, lab, _ = _inputs(LOSS_SHAPES[1], "plain")
    w = torch.from_numpy(_weight(159)).to(dev)
    labd = lab.to(dev)
    for xl in ("nchw", "nhwc"):
        xv = _place(x, xl, torch.float32, dev).requires_grad_(True)

        def step():
            loss = ops.seg_loss_labels(xv, labd, w, mse=True)
            (gx,) = torch.autograd.grad(3.0 * loss, xv)
            return loss, gx

        e_loss, e_gx = step()
        e_loss, e_gx = e_loss.detach().clone(), e_gx.clone()
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            step()                                               # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            g_loss, g_gx = step()
        main.wait_stream(side)
        for _ in range(2):
            g_loss.detach().zero_()
            g_gx.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(g_loss.detach(), e_loss) and torch.equal(g_gx, e_gx)
        assert bool(torch.isfinite(e_loss)) and e_gx.abs().sum() > 0


def test_no_dense_target_is_allocated():
    """[4, 159, 64, 64] fp32, forward + backward: the peak rises by the gradient and at most 1 MiB (a dense target alone would be 10 MB more)"""
    from mas_hip import ops
    dev = _dev()
    shape = (4, 159, 64, 64)
    labd = _labels(4, 64, 64, seed=2).to(dev)
    w = torch.from_numpy(_weight(159)).to(dev)
    for xl in ("nchw", "nhwc"):
        x = torch.randn(shape, device=dev)
        xv = (x.contiguous(memory_format=torch.channels_last) if xl == "nhwc" else x).requires_grad_(True)
        del x
        ops.seg_loss_labels(xv, labd, w, mse=True).backward()    # (library load, first launches)
        xv.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ops.seg_loss_labels(xv, labd, w, mse=True).backward()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        grad_bytes = xv.numel() * 4
        print(f"x {xl}: peak rise {rise} bytes, gradient {grad_bytes} bytes")
        assert xv.grad is not None and rise <= grad_bytes + (1 << 20), (rise, grad_bytes)


def test_errors_name_the_op():
    from mas_hip import ops
    dev = _dev()
    lab = _labels(1, 4, 4, layout=C8).to(dev)
    x = torch.zeros(1, 8, 4, 4, device=dev)
    w = torch.ones(8, device=dev)
    bad = [lambda: ops.seg_loss_labels(x.cpu(), lab, w),
           lambda: ops.seg_loss_labels(x, lab.cpu(), w),
           lambda: ops.seg_loss_labels(x.half(), lab, w),
           lambda: ops.seg_loss_labels(x, lab, torch.ones(7, device=dev)),
           lambda: ops.seg_loss_labels(x, lab.dense(), w)]
    for f in bad:
        with pytest.raises((ValueError, RuntimeError, TypeError), match="seg_loss_labels"):
            f()
    with pytest.raises(ValueError, match="seg_loss_labels"):     # the layout's C (8) against a prediction of 6 channels
        ops.seg_loss_labels(torch.zeros(1, 6, 4, 4, device=dev), lab, torch.ones(6, device=dev))
    with pytest.raises(ValueError, match="seg_loss_labels"):
        ops.seg_loss_labels(torch.zeros(1, 8, 4, 5, device=dev), lab, w)


# ---- model, loss classes, tokenizer ---------------------------------------------------------------------------------------------------
def _tiny_seg(dtype, train=True):
    from test_gpu_model import TINY, _build
    cfg = dict(TINY, ddconfig=dict(TINY["ddconfig"], in_channels=159, out_channels=159))
    return _build(cfg, 3, dtype, train=train)


def _model_batch():
    planes = torch.stack([seg_data.planes_from_arrays(*LR.sample_arrays(16, 16, seed=20 + s)) for s in range(2)])
    return SegLabels(planes)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_model_on_labels_is_bit_identical_to_the_dense_map(mode):
    """the first convolution sees the same bytes either way, and every path here repeats bit for bit"""
    dev = _dev()
    m = _tiny_seg(PDT[mode])
    lab = _model_batch().to(dev)
    dense = lab.cpu().dense().float().to(dev)
    with torch.no_grad():
        rec_d, q_d = m(dense)
        rec_l, q_l = m(lab)
        (quant_l, _), (quant_d, _) = m.encode(lab), m.encode(dense)
    assert rec_l.shape == rec_d.shape == (2, 159, 16, 16)
    assert torch.equal(rec_l, rec_d) and torch.equal(q_l, q_d) and torch.equal(quant_l, quant_d)
    assert bool(torch.isfinite(rec_l).all())
    m.eval()
    idx_l, idx_d = m.encode_to_indices(lab), m.encode_to_indices(dense)
    assert idx_l.dtype == torch.int64 and idx_l.shape[0] == 2 and torch.equal(idx_l, idx_d)


def test_model_refuses_labels_of_another_channel_count():
    dev = _dev()
    m = _tiny_seg(torch.float32)
    with pytest.raises(ValueError, match="SegLabels"):
        m(_labels(1, 16, 16, layout=C8).to(dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(_model_batch())


def test_model_on_labels_peaks_lower_than_on_the_dense_map():
    dev = _dev()
    m = _tiny_seg(torch.bfloat16)
    lab = _model_batch().to(dev)
    peaks = {}
    for name in ("warm", "dense", "labels"):
        inp = lab if name == "labels" else lab.dense().float()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        rec, q = m(inp)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated()
        del rec, q, inp
    print(f"VQBASE forward peak: dense input {peaks['dense']} bytes, labels {peaks['labels']} bytes")
    assert peaks["labels"] < peaks["dense"]


def _exact_zero_biases(m, keys):
    """the thirteen biases of the tiny configuration whose exact gradient is ZERO (what a run holds for them is summation noise, and a
    relative error of noise says nothing): the rules of tests/test_gpu_seg_loss.py's model-level test, restated"""
    mods = dict(m.named_modules())
    zero = {k for k in keys if k.endswith(".k.bias")}            # a constant added to every attention key moves no softmax row
    for blk in ("encoder.model.1", "decoder.model.12", "decoder.model.13"):
        assert mods[blk].norm2.num_channels == mods[blk].norm2.num_groups == 32
        zero.add(blk + ".conv1.bias")                            # a per-channel constant in front of a one-channel-per-group GroupNorm
    assert mods["decoder.model.14"].num_channels == mods["decoder.model.14"].num_groups == 32
    zero |= {"decoder.model.12.conv2.bias", "decoder.model.12.nin_shortcut.bias", "decoder.model.13.conv2.bias"}   # the same, through the skips
    zero |= {"encoder.model.12.bias", "quant_conv.0.bias"}       # a per-channel constant in front of the batch norm
    assert zero <= set(keys) and len(zero) == 13
    return zero


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_loss_class_on_labels_against_the_dense_target(mode, monkeypatch):
    """VQVAEWithBCELoss fed labels (model input and target) against the same class fed the dense map: the loss within the loss bound of
    the float64 helper, every parameter gradient within 5e-4 relative L2 (the gate of DESIGN 2.10's model-level test; tensors whose
    gradient is exactly zero in the dense run's arithmetic -- noise in both -- are left out as that test leaves them out)"""
    import losses
    from mas_hip import ops
    dev = _dev()
    monkeypatch.delenv("MAS_SEG_LOSS", raising=False)
    m = _tiny_seg(PDT[mode])
    lf = losses.VQVAEWithBCELoss(image_channels=159, codebook_weight=1.0).to(dev)
    assert list(lf.state_dict()) == ["weight"]
    lab = _model_batch().to(dev)
    dense = lab.cpu().dense().float().to(dev)
    calls = []
    real = ops.seg_loss_labels
    monkeypatch.setattr(ops, "seg_loss_labels", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    runs = {}
    for name, inp in (("labels", lab), ("dense", dense)):
        m.zero_grad(set_to_none=True)
        rec, q_loss = m(inp)
        loss = lf(q_loss, inp, rec)
        loss.backward()
        runs[name] = (float(loss.detach()), float(q_loss.detach()), rec.detach().double().cpu().numpy(),
                      {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None})
    assert len(calls) == 1
    t = dense.cpu().numpy()
    ref = R.seg_loss_ref(runs["labels"][2], t, R.module_weight(), True)[0] + runs["labels"][1]
    xt, tt = torch.from_numpy(runs["labels"][2]).float(), torch.from_numpy(t)
    y = float(F.mse_loss(torch.sigmoid(xt), tt) + F.binary_cross_entropy_with_logits(
        xt.movedim(1, -1), tt.movedim(1, -1), pos_weight=torch.from_numpy(R.module_weight()).float())) + runs["labels"][1]
    y_loss = abs(y - ref)
    e_loss = abs(runs["labels"][0] - ref)
    print(f"{mode}: loss labels {runs['labels'][0]:.7f} dense {runs['dense'][0]:.7f}: err {e_loss:.2e} (torch fp32 {y_loss:.2e})")
    assert e_loss <= _loss_bound(y_loss, ref)
    assert abs(runs["labels"][0] - runs["dense"][0]) <= 2 * _loss_bound(y_loss, ref)         # (two evaluations, each within the bound)
    gl, gd = runs["labels"][3], runs["dense"][3]
    assert set(gl) == set(gd) and len(gl) > 20
    zero = _exact_zero_biases(m, gd)
    worst, failures = 0.0, []
    for k in sorted(gd):
        diff, ref_n = float((gl[k] - gd[k]).norm()), float(gd[k].norm())
        if k in zero:                                            # noise in both runs: held to the layer's own gradient scale instead
            scale = float(gd[k[:-len("bias")] + "weight"].norm())
            if not diff <= 5e-4 * scale:
                failures.append((k, diff, scale))
            continue
        e = diff / (ref_n + 1e-30)
        worst = max(worst, e)
        if not e <= 5e-4:
            failures.append((k, e))
    print(f"{mode}: parameter gradients: worst relative L2 {worst:.2e} over {len(gd) - len(zero)} tensors; {len(zero)} with an exact gradient of zero")
    assert not failures, failures


def test_loss_classes_with_the_switch_thrown_run_the_torch_expression(monkeypatch):
    import losses
    from mas_hip import ops
    dev = _dev()
    lab = _labels(2, 6, 6, seed=3).to(dev)
    pred = torch.randn(2, 159, 6, 6, generator=torch.Generator().manual_seed(1)).to(dev)
    q = torch.tensor(0.125, device=dev)
    monkeypatch.setenv("MAS_SEG_LOSS", "0")
    monkeypatch.setattr(ops, "seg_loss_labels", lambda *a, **k: pytest.fail("ops.seg_loss_labels called with MAS_SEG_LOSS=0"))
    monkeypatch.setattr(ops, "seg_loss", lambda *a, **k: pytest.fail("ops.seg_loss called with MAS_SEG_LOSS=0"))
    t = lab.cpu().dense().to(dev)
    w = torch.from_numpy(R.module_weight()).float().to(dev)
    bce = F.binary_cross_entropy_with_logits(pred.movedim(1, -1), t.movedim(1, -1), pos_weight=w)
    got = losses.BCELossWithQuant(image_channels=159, codebook_weight=0.5).to(dev)(q, lab, pred)
    assert torch.equal(got, bce + 0.5 * q)
    got = losses.VQVAEWithBCELoss(image_channels=159, codebook_weight=0.5).to(dev)(q, lab, pred)
    assert torch.equal(got, F.mse_loss(torch.sigmoid(pred), t) + bce + 0.5 * q)


def test_tokenize_batch_takes_labels():
    import token_data
    from test_gpu_model import TINY, _build
    dev = _dev()
    vq_seg = _tiny_seg(torch.bfloat16, train=False)
    vq_img = _build(TINY, 0, torch.bfloat16, train=False)
    lab = _model_batch().to(dev)
    images = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(dev)
    img_l, seg_l = token_data.tokenize_batch(vq_img, vq_seg, images, lab)
    img_d, seg_d = token_data.tokenize_batch(vq_img, vq_seg, images, lab.cpu().dense().to(dev))
    assert seg_l.shape[0] == 2 and seg_l.dtype == torch.int64 and torch.equal(seg_l, seg_d) and torch.equal(img_l, img_d)
