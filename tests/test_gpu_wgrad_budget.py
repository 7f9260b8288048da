"""The CU budget of the weight-gradient grid travels in ``MasConvDesc.wgrad_cus`` (no environment variable), and the side-stream
section of the backward joins its streams in a ``finally`` and returns gradients that were allocated on the current stream."""
import ctypes as C
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "helpers")):
    if p not in sys.path:
        sys.path.insert(0, p)
import test_gpu_wgrad_splits as SPL  # noqa: E402  (its fp64 reference, error measure and bounds)
import wgrad_split_check as CHK  # noqa: E402
import wgrad_walk as W  # noqa: E402


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_the_budget_travels_in_the_descriptor(monkeypatch):
    """``mas_conv_wgrad_splits`` / ``mas_conv_wgrad_partial`` called directly with wgrad_cus = 0, -1 and 64: the split counts are what
    tests/helpers/wgrad_walk.py restates for budgets cus, 3 cus / 4 and 64, MAS_WGRAD_CUS in the environment changes none of them, and
    partial + reduce over a NaN-filled table meets the fp64 bounds of tests/test_gpu_wgrad_splits.py (TAU, EPS: no prologue here).
    Geometries: ``dma_ragged`` (N=4, 64 -> 128, 36 x 44: one output tile, 60 position tiles -- its count is clamped to 60 at all three
    budgets on any part with more than 60 CUs, so it cannot show that the field is read) and ``dma_c192_c384`` (nine output tiles, 12
    position tiles: 12, 12 and cdiv(64, 9) = 8 on a 256-CU part), over which at least two distinct counts are required."""
    import mas_hip
    from mas_hip import ops
    dev = _dev()
    lib = mas_hip.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    oversub, override = int(os.environ.get("MAS_WGRAD_OVERSUB") or 1), max(0, int(os.environ.get("MAS_WGRAD_SPLITS") or 0))
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
    counts = {}
    for c in (c for c in CHK.CASES if c["name"] in ("dma_ragged", "dma_c192_c384")):
        x, dy, _ = CHK.make_inputs(c)
        xd, dyd = cl(x), cl(dy)
        ref = SPL._reference(c)
        geo = SPL._walk_geo(c, c["n"])
        cin, cout, nw = c["cin"], c["cout"], c["cout"] * 9 * c["cin"]
        for b, budget in ((0, cus), (-1, cus * 3 // 4), (64, min(64, cus))):
            d = ops._desc(c["n"], c["h"], c["w"], cin, c["ho"], c["wo"], cout, 3, 1, 1, 1, torch.bfloat16, torch.bfloat16, ops.ACT_NONE, False)
            d.wgrad_cus = b
            k = int(lib.mas_conv_wgrad_splits(C.byref(d)))
            assert k == W.splits("conv_wgrad_dma", geo, cus, oversub, budget, override), (c["name"], b, k)
            with monkeypatch.context() as mp:
                mp.setenv("MAS_WGRAD_CUS", "7")
                assert int(lib.mas_conv_wgrad_splits(C.byref(d))) == k
                ws = torch.full((k * (nw + cout),), float("nan"), dtype=torch.float32, device=dev)
                pb = C.c_void_p(ws.data_ptr() + 4 * k * nw)
                dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=dev)
                db = torch.empty(cout, dtype=torch.float32, device=dev)
                mas_hip.check(lib.mas_conv_wgrad_partial(C.byref(d), ops._ptr(xd), ops._ptr(None), ops._ptr(dyd), ops._ptr(ws), pb, ops._stream()),
                              "conv_wgrad_partial")
                assert ops.last_kernel() == "conv_wgrad_dma"
                mas_hip.check(lib.mas_wgrad_reduce(ops._ptr(ws), pb, k, ops._ptr(dw), ops._ptr(db), cout, cin, 3, ops._stream()), "wgrad_reduce")
                torch.cuda.synchronize()
            e_max, e_l2 = SPL._errs(dw.cpu(), db.cpu(), *ref)
            print(f"{c['name']:14s} wgrad_cus {b:3d}: splits {k:3d}  max/S {e_max:.2e}  relL2 {e_l2:.2e}")
            assert e_max <= SPL.TAU and e_l2 <= SPL.EPS, (c["name"], b, k, e_max, e_l2)
            counts[c["name"], b] = k
    print("split counts:", counts)
    if override == 0 and oversub == 1 and cus >= 128:          # (the production sizing; an override or a small part clamps them all)
        assert len({k for (name, _), k in counts.items() if name == "dma_c192_c384"}) >= 2, counts


def _layer(dev):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 16, 16, generator=g).bfloat16().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    par = [(0.05 * torch.randn(128, 64, 3, 3, generator=g)), 0.1 * torch.randn(128, generator=g), 1.0 + 0.1 * torch.randn(64, generator=g),
           0.1 * torch.randn(64, generator=g)]
    par = [p.to(dev).requires_grad_(True) for p in par]
    dy = torch.randn(2, 128, 16, 16, generator=g).bfloat16().to(dev).contiguous(memory_format=torch.channels_last)
    return x, par, dy


def _backward(ops, x, par, dy):
    for t in [x] + par:
        t.grad = None
    y = ops.norm_act_conv(x, par[0], par[1], par[2], par[3], act=ops.ACT_AFFINE_SILU, in_dtype=torch.bfloat16)
    y.backward(dy)
    torch.cuda.synchronize()
    return [t.grad.clone() for t in [x] + par]


@pytest.fixture
def side(monkeypatch):
    """(ops, device, main stream) with the side stream switched on for the device without a probe"""
    from mas_hip import ops
    dev = _dev()
    monkeypatch.setattr(ops, "_WGRAD_STREAM", True)
    monkeypatch.setattr(ops, "_side_ok", {dev.index: False})
    yield ops, dev, torch.cuda.current_stream()
    ops.set_launch_hook(None)


def test_a_host_exception_inside_the_deferred_section_leaves_the_streams_usable(side):
    """A launch hook raises a Python exception at the "conv_wgrad" launch of a GroupNorm+SiLU conv layer (N=2, 64 -> 128, 16 x 16), i.e.
    on the side stream, before anything is launched there: a host exception, nothing faults on the GPU.  It propagates out of
    ``backward``; the current stream is what it was (here and, in the next backward, on the autograd thread: the data gradient is
    launched on it, the weight gradient on the side stream); with the hook removed the side-stream gradients are the one-stream
    gradients bit for bit.  That the join ran after the exception is not observable from here: it is the ``finally`` of
    ``ops._side_section``, which runs on the way out of the ``with`` block of ``_NormActConv.backward`` whether or not the body raised."""
    ops, dev, main = side
    x, par, dy = _layer(dev)
    one = _backward(ops, x, par, dy)                     # _side_ok False: everything on one stream
    ops._side_ok[dev.index] = True

    class Boom(Exception):
        pass

    def raising(kind, shape, launch):
        if kind == "conv_wgrad":
            assert torch.cuda.current_stream() == ops._side_stream()
            raise Boom("host exception before the weight-gradient launch")
        launch()

    ops.set_launch_hook(raising)
    with pytest.raises(Boom):
        _backward(ops, x, par, dy)
    assert torch.cuda.current_stream() == main
    seen = []

    def recording(kind, shape, launch):
        seen.append((kind, torch.cuda.current_stream()))
        launch()

    ops.set_launch_hook(recording)
    two = _backward(ops, x, par, dy)
    ops.set_launch_hook(None)
    kinds = dict(seen)
    assert kinds["conv_wgrad"] == ops._side_stream() != main and all(s == main for k, s in seen if k != "conv_wgrad"), seen
    again = _backward(ops, x, par, dy)
    assert torch.cuda.current_stream() == main
    for a, b, c in zip(one, two, again):
        assert torch.equal(a, b) and torch.equal(b, c)


def test_side_stream_gradients_are_allocated_on_the_current_stream(side, monkeypatch):
    """After a side-stream backward of the same layer, what the node returned as dW / db was allocated by ``ops._wgrad_outputs`` on the
    current stream, outside the side-stream section, and ``conv_wgrad_raw`` wrote into those very tensors."""
    ops, dev, main = side
    ops._side_ok[dev.index] = True
    x, par, dy = _layer(dev)
    made, returned = [], []
    alloc, raw = ops._wgrad_outputs, ops.conv_wgrad_raw

    def outputs(*a):
        outs = alloc(*a)
        made.append((torch.cuda.current_stream(), [t.data_ptr() for t in outs]))
        return outs

    def wgrad(*a):
        res = raw(*a)
        returned.append((torch.cuda.current_stream(), [t.data_ptr() for t in res], [t.data_ptr() for t in a[-2:]]))
        return res

    monkeypatch.setattr(ops, "_wgrad_outputs", outputs)
    monkeypatch.setattr(ops, "conv_wgrad_raw", wgrad)
    grads = _backward(ops, x, par, dy)
    assert len(made) == len(returned) == 1
    assert made[0][0] == main != ops._side_stream() and returned[0][0] == ops._side_stream()
    assert returned[0][1] == returned[0][2] == made[0][1]
    assert all(torch.isfinite(g).all() for g in grads)
