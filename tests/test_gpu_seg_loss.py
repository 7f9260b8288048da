"""``mas_hip.ops.seg_loss`` (csrc/seg_loss.hip) on the GPU against the float64 restatement of tests/helpers/seg_loss_ref.py, which
tests/test_seg_loss_cpu.py pins to the reference's own classes (tests/golden/loss_seg.npz).

Bounds (as tests/test_gpu_token_loss.py:101-108).  y = the deviation of torch's own fp32 CPU evaluation of the same expression from the
float64 helper on the same inputs; S = max(pos_weight) |g| / n, the largest weight an element's gradient carries:
  loss and each returned term   |error| <= max(4 y_loss, 4 * 2^-23 * max(1, |ref|))
  fp32 gradient, per element    |error| <= max(4 y_dx, 8 * 2^-24 * S)
  bf16 gradient, per element    |error| <= 2^-8 |ref| + 8 * 2^-24 * S          (one rounding of the gradient to bf16)
Shapes are the smallest at which the kernels can go wrong: one tile, a partial tile with unaligned rows in both layouts, one element rows,
an even channel count (padded LDS pitch), several tiles plus a tail, several work-groups per image; offsets past 2^31 are exercised by
tools/kbench_seg_loss.py, not here."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import seg_loss_ref as R  # noqa: E402
from make_golden_r6 import loss_seg_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 159, 8, 8), (3, 159, 5, 7), (1, 1, 3, 3), (2, 32, 9, 9), (1, 160, 16, 20), (2, 159, 64, 64)]
LAYOUTS = [("nchw", "nchw"), ("nchw", "nhwc"), ("nhwc", "nchw"), ("nhwc", "nhwc")]
PDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "uint8": torch.uint8}
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _weight(c):
    if c == 159:
        return R.module_weight().astype(np.float32)          # the module's vector: 20 on channels 153..157
    return np.random.RandomState(100 + c).uniform(0.5, 3.0, c).astype(np.float32)


def _inputs(shape, kind="hard01"):
    """-> (x, t) float32 numpy in logical NCHW order.  hard01: {0, 1} targets; soft: targets in (0, 1); bf16: hard01 with logits that bf16
    holds exactly; hard: the fixture's logits with every 7th element x 20 (|x| up to about 150) and exact zeros (hardbf16: then rounded to bf16)"""
    key = ("in", shape, kind)
    if key not in _cache:
        n, c, h, w = shape
        if shape == (2, 159, 8, 8):
            x, t, _ = loss_seg_inputs()                          # the fixture
        else:
            rs = np.random.RandomState(7 + n + c + h * w)
            x = (2.0 * rs.randn(n, c, h, w)).astype(np.float32)
            t = (rs.rand(n, c, h, w) < 0.3).astype(np.float32)
        if kind == "soft":
            t = np.random.RandomState(5).uniform(0.02, 0.98, shape).astype(np.float32)
        if kind == "bf16":
            x = torch.from_numpy(x).bfloat16().float().numpy()
        if kind in ("hard", "hardbf16"):
            x = x.copy()
            flat = x.reshape(-1)
            flat[::7] *= 20.0
            flat[3::11] = 0.0
            assert np.abs(x).max() > 100.0
            if kind == "hardbf16":
                x = torch.from_numpy(x).bfloat16().float().numpy()
        _cache[key] = (x, t)
    return _cache[key]


def _reference(shape, kind, mse, g=1.0):
    """-> fp64 (loss, bce_mean, mse_mean, dx), the yardsticks (y_loss, y_dx) of torch's fp32 CPU evaluation, and S; computed once"""
    key = ("ref", shape, kind, mse, g)
    if key not in _cache:
        x, t = _inputs(shape, kind)
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
    if layout == "nhwc":
        buf = torch.zeros(a.size + offset + 64, dtype=dtype, device=dev)
        v = buf[offset:offset + a.size].view(n, h, w, c).permute(0, 3, 1, 2)
    else:
        buf = torch.zeros(a.size + offset + 64, dtype=dtype, device=dev)
        v = buf[offset:offset + a.size].view(n, c, h, w)
    v.copy_(src)
    assert v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return v


def _is_layout(v, layout):
    return v.is_contiguous(memory_format=torch.channels_last) if layout == "nhwc" else v.is_contiguous()


def _loss_bound(y_loss, ref):
    return max(4 * y_loss, 4 * 2.0 ** -23 * max(1.0, abs(ref)))


def _check(shape, kind, mse, xl, tl, pdt=torch.float32, tdt=torch.float32, offset=0):
    from mas_hip import ops
    dev = _dev()
    x, t = _inputs(shape, kind)
    (ref_loss, ref_bce, ref_mse, ref_dx), y_loss, y_dx, S = _reference(shape, kind, mse)
    xv = _place(x, xl, pdt, dev, offset).requires_grad_(True)
    tv = _place(t, tl, tdt, dev, offset)
    w = torch.from_numpy(_weight(shape[1])).to(dev)
    before = xv.detach().clone()
    loss, terms = ops.seg_loss(xv, tv, w, mse=mse, return_terms=True)
    loss.backward()
    assert loss.dtype == torch.float32 and loss.shape == () and not terms["bce_mean"].requires_grad
    dx = xv.grad
    assert dx.dtype == pdt and dx.shape == xv.shape and dx.stride() == xv.stride() and _is_layout(dx, xl)
    assert torch.equal(xv.detach(), before)
    e_loss = abs(float(loss.detach()) - ref_loss)
    e_bce, e_mse = abs(float(terms["bce_mean"]) - ref_bce), abs(float(terms["mse_mean"]) - ref_mse)
    d = np.abs(dx.double().cpu().numpy() - ref_dx)
    tag = f"{shape} {kind} mse={int(mse)} x:{xl}/{str(pdt)[6:]} t:{tl}/{str(tdt)[6:]} off={offset}"
    print(f"{tag}: loss err {e_loss:.2e} (torch fp32 {y_loss:.2e}), grad err {d.max():.2e} (torch fp32 {y_dx:.2e}; S {S:.2e})")
    assert np.isfinite(float(loss.detach())) and np.isfinite(d).all(), tag
    assert e_loss <= _loss_bound(y_loss, ref_loss), (tag, e_loss, y_loss)
    assert e_bce <= _loss_bound(y_loss, ref_bce) and e_mse <= _loss_bound(y_loss, ref_mse), (tag, e_bce, e_mse)
    if pdt == torch.float32:
        assert (d <= max(4 * y_dx, 8 * 2.0 ** -24 * S)).all(), (tag, float(d.max()), y_dx, S)
    else:
        assert (d <= 2.0 ** -8 * np.abs(ref_dx) + 8 * 2.0 ** -24 * S).all(), (tag, float(d.max()))


@pytest.mark.parametrize("mse", [False, True], ids=["bce", "bce+mse"])
@pytest.mark.parametrize("xl,tl", LAYOUTS, ids=["x_%s-t_%s" % p for p in LAYOUTS])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_seg_loss_vs_fp64(shape, xl, tl, mse):
    _check(shape, "hard01", mse, xl, tl)


@pytest.mark.parametrize("tdt", list(TDT), ids=["t_%s" % k for k in TDT])
@pytest.mark.parametrize("pdt", list(PDT), ids=["x_%s" % k for k in PDT])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=["x".join(map(str, s)) for s in SHAPES[:2]])
def test_seg_loss_dtypes(shape, pdt, tdt):
    """logits that bf16 holds exactly and {0, 1} targets, so every storage type carries the same values; all four layout pairs"""
    for xl, tl in LAYOUTS:
        for mse in (False, True):
            _check(shape, "bf16", mse, xl, tl, PDT[pdt], TDT[tdt])


@pytest.mark.parametrize("pdt", list(PDT), ids=["x_%s" % k for k in PDT])
def test_seg_loss_base_pointer_aligned_to_one_element_only(pdt):
    """both tensors start one element past a 16-byte boundary (4 bytes for fp32, 2 for bf16); HW = 35 leaves no row aligned either"""
    for xl, tl in LAYOUTS:
        _check((3, 159, 5, 7), "bf16", True, xl, tl, PDT[pdt], PDT[pdt], offset=1)
    _check((3, 159, 5, 7), "bf16", True, "nhwc", "nchw", PDT[pdt], torch.uint8, offset=3)


def test_seg_loss_bool_target_is_uint8():
    from mas_hip import ops
    dev = _dev()
    x, t = _inputs(SHAPES[0], "hard01")
    w = torch.from_numpy(_weight(159)).to(dev)
    xv = _place(x, "nhwc", torch.float32, dev)
    a = ops.seg_loss(xv, torch.from_numpy(t).to(dev).bool(), w, mse=True)
    b = ops.seg_loss(xv, torch.from_numpy(t).to(dev).to(torch.uint8), w, mse=True)
    assert torch.equal(a, b) and bool(torch.isfinite(a))


@pytest.mark.parametrize("xl,tl", LAYOUTS, ids=["x_%s-t_%s" % p for p in LAYOUTS])
def test_seg_loss_soft_targets(xl, tl):
    for shape in SHAPES[:2]:
        _check(shape, "soft", True, xl, tl)


@pytest.mark.parametrize("xl,tl", LAYOUTS, ids=["x_%s-t_%s" % p for p in LAYOUTS])
def test_seg_loss_hard_inputs_stay_finite(xl, tl):
    """|x| up to about 150 and exact zeros: loss and every gradient element finite (asserted in _check), and within the bounds"""
    for mse in (False, True):
        _check(SHAPES[0], "hard", mse, xl, tl)
    _check(SHAPES[0], "hardbf16", True, xl, tl, torch.bfloat16, torch.uint8)


@pytest.mark.parametrize("cw", [1.0, 0.25])
@pytest.mark.parametrize("name,mse", [("BCELossWithQuant", False), ("VQVAEWithBCELoss", True)])
def test_loss_classes_reproduce_the_reference_fixture_on_the_gpu(name, mse, cw, monkeypatch):
    """the module (not the op) on GPU tensors against tests/golden/loss_seg.npz, which the reference's classes made: the bounds above with the
    fixture as the reference and its own deviation from the float64 helper as y"""
    import losses
    from mas_hip import ops
    dev = _dev()
    monkeypatch.delenv("MAS_SEG_LOSS", raising=False)
    calls = []
    real = ops.seg_loss
    monkeypatch.setattr(ops, "seg_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = np.load(os.path.join(ROOT, "tests", "golden", "loss_seg.npz"))
    pred, target, qloss = loss_seg_inputs()
    ref_loss, ref_dx = float(g[f"{name}:{cw}:loss"]), g[f"{name}:{cw}:grad"].astype(np.float64)
    h_loss, _, _, h_dx = R.seg_loss_ref(pred, target, g[f"{name}:weight"], mse)
    y_loss, y_dx = abs(h_loss + cw * float(qloss) - ref_loss), float(np.abs(h_dx - ref_dx).max())
    S = 20.0 / pred.size
    m = getattr(losses, name)(image_channels=159, codebook_weight=cw).to(dev)
    for layout in ("nchw", "nhwc"):
        p = _place(pred, layout, torch.float32, dev).requires_grad_(True)
        loss = m(torch.tensor(float(qloss), device=dev), torch.from_numpy(target).to(dev), p)
        loss.backward()
        e_loss = abs(float(loss.detach()) - ref_loss)
        d = np.abs(p.grad.double().cpu().numpy() - ref_dx)
        print(f"{name} cw={cw} {layout}: loss err {e_loss:.2e} (fixture vs fp64 {y_loss:.2e}), grad err {d.max():.2e} (fixture vs fp64 {y_dx:.2e})")
        assert e_loss <= _loss_bound(y_loss, ref_loss)
        assert (d <= max(4 * y_dx, 8 * 2.0 ** -24 * S)).all(), float(d.max())
    assert len(calls) == 2                                       # the HIP path, both times
    monkeypatch.setenv("MAS_SEG_LOSS", "0")                      # the switch: the torch expression on the same GPU tensors
    p = _place(pred, "nhwc", torch.float32, dev).requires_grad_(True)
    loss = m(torch.tensor(float(qloss), device=dev), torch.from_numpy(target).to(dev), p)
    assert len(calls) == 2 and abs(float(loss.detach()) - ref_loss) < 1e-5


def test_upstream_gradient_scales_and_accumulates():
    from mas_hip import ops
    dev = _dev()
    shape = SHAPES[1]
    x, t = _inputs(shape, "hard01")
    (_, _, _, ref1), _, y1, S1 = _reference(shape, "hard01", True)
    (_, _, _, ref3), _, y3, S3 = _reference(shape, "hard01", True, 3.0)            # torch's own backward under g = 3; S carries |g|
    b1, b3 = max(4 * y1, 8 * 2.0 ** -24 * S1), max(4 * y3, 8 * 2.0 ** -24 * S3)
    w = torch.from_numpy(_weight(159)).to(dev)
    xv = _place(x, "nhwc", torch.float32, dev).requires_grad_(True)
    tv = _place(t, "nchw", torch.float32, dev)
    (3.0 * ops.seg_loss(xv, tv, w, mse=True)).backward()
    d = np.abs(xv.grad.double().cpu().numpy() - ref3)
    assert np.abs(ref3 - 3.0 * ref1).max() == 0.0 or np.allclose(ref3, 3.0 * ref1, rtol=1e-15, atol=0.0)
    assert (d <= b3).all(), (float(d.max()), b3)
    ops.seg_loss(xv, tv, w, mse=True).backward()                                     # a second backward into the same .grad: 3 + 1
    d = np.abs(xv.grad.double().cpu().numpy() - (ref3 + ref1))
    assert (d <= b3 + b1 + 2.0 ** -24 * np.abs(ref3 + ref1)).all(), float(d.max())   # (each term's bound + the fp32 add)


def test_no_full_size_temporaries():
    """fp32 NHWC prediction, fp32 NCHW target, forward + backward: the peak rises by the gradient and at most 1 MiB of workspace.  A condition:
    the torch expression fails it by construction, and so would a hidden .contiguous() of either tensor"""
    from mas_hip import ops
    dev = _dev()
    shape = SHAPES[5]
    x, t = _inputs(shape, "hard01")
    w = torch.from_numpy(_weight(159)).to(dev)
    xv = _place(x, "nhwc", torch.float32, dev).requires_grad_(True)
    tv = _place(t, "nchw", torch.float32, dev)
    ops.seg_loss(xv, tv, w, mse=True).backward()                 # (library load, first launches)
    xv.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.seg_loss(xv, tv, w, mse=True).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    grad_bytes = xv.numel() * 4
    print(f"peak rise {rise} bytes, gradient {grad_bytes} bytes")
    assert xv.grad is not None and rise <= grad_bytes + (1 << 20), (rise, grad_bytes)


@pytest.mark.parametrize("xl,tl", [("nhwc", "nchw"), ("nchw", "nchw")], ids=["mixed", "flat"])
def test_two_evaluations_give_identical_bits(xl, tl):
    from mas_hip import ops
    dev = _dev()
    x, t = _inputs(SHAPES[5], "hard01")
    w = torch.from_numpy(_weight(159)).to(dev)
    outs = []
    for _ in range(2):
        xv = _place(x, xl, torch.float32, dev).requires_grad_(True)          # fresh copies
        tv = _place(t, tl, torch.float32, dev)
        loss = ops.seg_loss(xv, tv, w, mse=True)
        loss.backward()
        outs.append((loss.detach().clone(), xv.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][0])) and outs[0][1].abs().sum() > 0


def test_non_dense_prediction_goes_through_a_dense_copy():
    """a prediction sliced along W is neither dense layout: the op makes it dense first, and the gradient comes back in the slice's shape"""
    from mas_hip import ops
    dev = _dev()
    shape = SHAPES[1]
    x, t = _inputs(shape, "hard01")
    (ref_loss, _, _, ref_dx), y_loss, y_dx, S = _reference(shape, "hard01", True)
    n, c, h, wd = shape
    big = torch.full((n, c, h, wd + 3), 55.0, device=dev, requires_grad=True)
    with torch.no_grad():
        big[..., 1:1 + wd] = torch.from_numpy(x).to(dev)
    view = big[..., 1:1 + wd]
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    w = torch.from_numpy(_weight(159)).to(dev)
    loss = ops.seg_loss(view, torch.from_numpy(t).to(dev), w, mse=True)
    loss.backward()
    assert abs(float(loss.detach()) - ref_loss) <= _loss_bound(y_loss, ref_loss)
    gb = big.grad.double().cpu().numpy()
    assert (np.abs(gb[..., 1:1 + wd] - ref_dx) <= max(4 * y_dx, 8 * 2.0 ** -24 * S)).all()
    assert (gb[..., :1] == 0).all() and (gb[..., 1 + wd:] == 0).all()


def test_forward_and_backward_capture_into_a_graph():
    """forward + backward captured once on a side stream, replayed twice: the eager bits each time (no host synchronisation anywhere)"""
    from mas_hip import ops
    dev = _dev()
    x, t = _inputs(SHAPES[1], "hard01")
    w = torch.from_numpy(_weight(159)).to(dev)
    xv = _place(x, "nhwc", torch.float32, dev).requires_grad_(True)
    tv = _place(t, "nchw", torch.float32, dev)

    def step():
        loss = ops.seg_loss(xv, tv, w, mse=True)
        (gx,) = torch.autograd.grad(3.0 * loss, xv)
        return loss, gx

    e_loss, e_gx = step()
    e_loss, e_gx = e_loss.detach().clone(), e_gx.clone()
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        step()                                                   # warm-up on the capture stream
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


def test_loss_classes_fall_back_beyond_the_channel_limit(monkeypatch):
    """more channels than the kernels keep weights for in LDS: the op says so by name, the loss classes run the torch expression"""
    import losses
    from losses import loss_seg
    from mas_hip import ops
    dev = _dev()
    c = loss_seg._HIP_MAX_CHANNELS + 1
    x = torch.zeros(1, c, 1, 2, device=dev).contiguous(memory_format=torch.channels_last)
    t = torch.zeros(1, c, 1, 2, device=dev)
    with pytest.raises(RuntimeError, match="seg_loss"):
        ops.seg_loss(x, t, torch.ones(c, device=dev))
    monkeypatch.delenv("MAS_SEG_LOSS", raising=False)
    monkeypatch.setattr(ops, "seg_loss", lambda *a, **k: pytest.fail("ops.seg_loss called beyond its channel limit"))
    m = losses.BCELossWithQuant(image_channels=c).to(dev)
    loss = m(torch.zeros((), device=dev), t, x)
    assert abs(float(loss) - float(np.log(2.0))) < 1e-6          # softplus(0) on every element


def test_errors_name_the_op():
    from mas_hip import ops
    dev = _dev()
    x = torch.zeros(1, 3, 4, 4, device=dev)
    w = torch.ones(3, device=dev)
    bad = [lambda: ops.seg_loss(x.cpu(), x.cpu(), w.cpu()),                          # CPU tensors
           lambda: ops.seg_loss(x, x.cpu(), w),
           lambda: ops.seg_loss(x, torch.zeros(1, 3, 4, 5, device=dev), w),          # shape mismatch
           lambda: ops.seg_loss(x, torch.zeros(1, 3, 4, 4, dtype=torch.int32, device=dev), w),      # unsupported target dtype
           lambda: ops.seg_loss(x.half(), x, w),                                     # unsupported prediction dtype
           lambda: ops.seg_loss(x, x, torch.ones(4, device=dev)),                    # pos_weight not [C]
           lambda: ops.seg_loss(x[:0], x[:0], w),                                    # empty
           lambda: ops.seg_loss(x, x.clone().requires_grad_(True), w)]               # a target that requires grad
    for f in bad:
        with pytest.raises((ValueError, RuntimeError), match="seg_loss"):
            f()


def test_model_level_hip_loss_against_torch_loss(monkeypatch):
    """the tiny VQ-SEG configuration of tests/test_gpu_model.py:87-93 (TINY with 159 channels in and out, B = 2, 16 x 16, fp32 mode): one forward
    + backward with VQVAEWithBCELoss through the HIP loss and through MAS_SEG_LOSS=0 on the same weights and input.  The loss to the loss
    bound above (against the float64 helper on the decoder's output); every parameter gradient within 5e-4 relative L2 of the torch run --
    the fp32-mode gate of tests/test_gpu_parity_r5.py:174 (DESIGN 5 measures 6e-6 ... 9e-6 for the encoder and decoder backward).  Measured: 2.2e-6 at the worst over 172 tensors; the
    thirteen named biases whose exact gradient is zero are checked to be noise in both runs instead."""
    import losses
    from mas_hip import ops
    from test_gpu_model import TINY, _build
    dev = _dev()
    old = ops.compute_dtype()
    try:
        cfg = dict(TINY, ddconfig=dict(TINY["ddconfig"], in_channels=159, out_channels=159))
        m = _build(cfg, 3, torch.float32)
        lf = losses.VQVAEWithBCELoss(image_channels=159, codebook_weight=1.0).to(dev)
        seg = (torch.rand(2, 159, 16, 16, generator=torch.Generator().manual_seed(3)) < 0.3).float().to(dev)
        runs = {}
        for mode in ("hip", "torch"):
            if mode == "torch":
                monkeypatch.setenv("MAS_SEG_LOSS", "0")
            else:
                monkeypatch.delenv("MAS_SEG_LOSS", raising=False)
            m.zero_grad(set_to_none=True)
            rec, q_loss = m(seg)
            loss = lf(q_loss, seg, rec)
            loss.backward()
            runs[mode] = (float(loss.detach()), float(q_loss.detach()), rec.detach().double().cpu().numpy(),
                          {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None})
        ref = R.seg_loss_ref(runs["torch"][2], seg.cpu().numpy(), R.module_weight(), True)[0] + runs["torch"][1]
        y_loss = abs(runs["torch"][0] - ref)
        ref_h = R.seg_loss_ref(runs["hip"][2], seg.cpu().numpy(), R.module_weight(), True)[0] + runs["hip"][1]
        e_loss = abs(runs["hip"][0] - ref_h)
        print(f"loss hip {runs['hip'][0]:.7f} torch {runs['torch'][0]:.7f}: err {e_loss:.2e} (torch path {y_loss:.2e})")
        assert e_loss <= _loss_bound(y_loss, ref_h)
        assert abs(runs["hip"][0] - runs["torch"][0]) <= 2 * _loss_bound(y_loss, ref)       # (two evaluations, each within the bound)
        gh, gt = runs["hip"][3], runs["torch"][3]
        assert set(gh) == set(gt) and len(gh) > 20
        # Thirteen biases of this configuration have an exact gradient of ZERO: what both runs hold for them is summation noise, and a
        # relative error of noise says nothing (tests/test_gpu_parity_r5.py:91-92 leaves the first kind out for the same reason).  They
        # are named here, each kind with its reason; every other tensor, every other bias included, is held to the plain 5e-4.
        mods = dict(m.named_modules())
        zero = {}
        for k in gt:
            if k.endswith(".k.bias"):
                zero[k] = "a constant added to every attention key moves no softmax row"
        for blk in ("encoder.model.1", "decoder.model.12", "decoder.model.13"):
            assert mods[blk].norm2.num_channels == mods[blk].norm2.num_groups == 32
            zero[blk + ".conv1.bias"] = "a per-channel constant in front of norm2 with one channel per group"
        # decoder blocks 12 and 13 are the 32-channel tail: their outputs reach only one-channel-per-group GroupNorms (13's norm1, and
        # through the skips the final Normalize(32), decoder.model.14), which remove a per-channel constant
        assert mods["decoder.model.14"].num_channels == mods["decoder.model.14"].num_groups == 32
        for k in ("decoder.model.12.conv2.bias", "decoder.model.12.nin_shortcut.bias", "decoder.model.13.conv2.bias"):
            zero[k] = "a per-channel constant that only one-channel-per-group GroupNorms consume"
        # the encoder's last convolution feeds the 1x1 quant_conv.0, whose output the batch norm quant_conv.1 centres per channel
        for k in ("encoder.model.12.bias", "quant_conv.0.bias"):
            zero[k] = "a per-channel constant in front of the batch norm"
        assert set(zero) <= set(gt) and len(zero) == 13
        worst, failures = 0.0, []
        for k in sorted(gt):
            diff, ref_n, hip_n = float((gh[k] - gt[k]).norm()), float(gt[k].norm()), float(gh[k].norm())
            if k in zero:
                # noise in both runs: far below the layer's own gradient scale (fp32 summation noise of a bias gradient is about
                # 2^-24 sqrt(positions / fan-in) |dW| <= 2^-22 |dW| at these shapes; measured <= 1.2e-7 |dW|)
                scale = float(gt[k[:-len("bias")] + "weight"].norm())
                print(f"  {k:44s} exact gradient 0 ({zero[k]}): |hip| {hip_n:.2e} |torch| {ref_n:.2e} |dW| {scale:.2e}")
                if not (hip_n <= 2.0 ** -20 * scale and ref_n <= 2.0 ** -20 * scale):
                    failures.append((k, hip_n, ref_n, scale))
                continue
            e = diff / (ref_n + 1e-30)
            print(f"  {k:44s} rel-L2 {e:.2e}   |torch| {ref_n:.2e}")
            worst = max(worst, e)
            if not e <= 5e-4:
                failures.append((k, e))
        print(f"parameter gradients: worst relative L2 {worst:.2e} over {len(gt) - len(zero)} tensors; {len(zero)} with an exact gradient of zero")
        assert not failures, failures
    finally:
        ops.set_compute_dtype(old)
