"""``mas_hip.ops.cross_entropy`` (csrc/token_loss.hip) on the GPU against the float64 reference of tests/helpers/token_ce_ref.py, which
tests/test_token_loss_cpu.py pins to ``F.cross_entropy`` in float64 on the same cases.

Bounds, per case (the yardstick is ATen's ``F.cross_entropy`` on ``logits.float()`` on the same GPU and ITS maximum error against fp64):
  loss           max |error| <= max(4 x yardstick, 4 * 2^-23 * max(1, |loss|))
  fp32 gradient  max |error| <= max(4 x yardstick, 8 * 2^-24 * |w|)
  bf16 gradient  |g - g64| <= 2^-8 |g64| + 8 * 2^-24 |w|        (one bf16 ulp: the same fp32 value rounded near a tie)
w is the row's weight in dx = w (p - (1 - eps) [j = t] - eps / V).  The factor 4 and the floors cover a fast exp (about 2 ulp plus an
argument rounded at |x - m| <= 88) and another summation order."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import token_ce_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _place(x32, t, case, dtype, dev):
    """the case's logits on the device in its layout -> (logits view, target of the view's leading shape)"""
    rows, v = x32.shape
    x = torch.from_numpy(x32).to(dev).to(dtype)
    tt = torch.from_numpy(t).to(dev)
    if case["layout"] == "slice":                                # the [2, 5, V] slice of [2, 9, V]
        base = torch.full((2, 9, v), 777.0, dtype=dtype, device=dev)
        base[:, 2:7] = x.view(2, 5, v)
        view = base[:, 2:7]
        assert not view.is_contiguous()
        return view, tt.view(2, 5)
    if case["layout"] == "offset":                               # starts 4 bytes off a 16-byte boundary
        k = 4 // x.element_size()
        buf = torch.zeros(rows * v + 64, dtype=dtype, device=dev)
        view = buf[k:k + rows * v].view(rows, v)
        view.copy_(x)
        assert view.data_ptr() % 16 == 4
        return view, tt
    return x, tt


def _run(fn, view, tt, case, g, dev):
    xin = view.detach().requires_grad_(True)                     # (detach keeps the strides: still the view's memory)
    loss = fn(xin, tt)
    loss.backward(torch.as_tensor(g, device=dev).reshape(loss.shape))
    return loss.detach(), xin.grad.detach()


def _maxerr(got, ref):
    """max |got - ref| where ref is finite; NaN must sit exactly where ref has it"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    ok = ~np.isnan(ref)
    return float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.CASES, ids=[c["id"] for c in R.CASES])
def test_cross_entropy_vs_fp64(case, dtype):
    from mas_hip import ops
    dev = _dev()
    x32, t, g = R.make_case(case, dtype)
    v, red, eps = case["v"], case["reduction"], case["eps"]
    ref_loss, ref_dx, w = R.ce_ref(x32, t, red, R.IGNORE, eps, g)
    view, tt = _place(x32, t, case, dtype, dev)
    before = view.clone()
    loss, dx = _run(lambda a, b: ops.cross_entropy(a, b, reduction=red, ignore_index=R.IGNORE, label_smoothing=eps), view, tt, case, g, dev)
    assert loss.dtype == torch.float32 and loss.shape == (tt.shape if red == "none" else ())
    assert dx.dtype == dtype and dx.shape == view.shape and torch.equal(view, before)
    loss, dx = loss.cpu().numpy().reshape(np.shape(ref_loss)), dx.float().cpu().numpy().reshape(ref_dx.shape)

    # the yardstick: ATen on logits.float() (targets outside [0, V) would device-assert there: those rows are ignored rows for ATen and
    # compared for NaN only; reduction "none" keeps every other row apart from them)
    bad = (t != R.IGNORE) & ((t < 0) | (t >= v))
    ta = torch.from_numpy(np.where(bad, R.IGNORE, t)).to(dev).view(tt.shape)
    a_loss, a_dx = _run(lambda a, b: F.cross_entropy(a.float().reshape(-1, v), b.reshape(-1), reduction=red, ignore_index=R.IGNORE,
                                                     label_smoothing=eps).reshape(() if red != "none" else b.shape), view, ta, case, g, dev)
    a_loss, a_dx = a_loss.cpu().numpy().reshape(np.shape(ref_loss)), a_dx.float().cpu().numpy().reshape(ref_dx.shape)
    if bad.any():
        assert red == "none" and np.isnan(loss[bad]).all() and np.isnan(dx[bad]).all()          # NaN in those rows ...
        a_loss, a_dx = np.where(bad, np.nan, a_loss), np.where(bad[:, None], np.nan, a_dx)
        assert np.isfinite(loss[~bad]).all() and np.isfinite(dx[~bad]).all()                     # ... and only there
    y_loss, e_loss = _maxerr(a_loss, ref_loss), _maxerr(loss, ref_loss)
    scale = np.maximum(1.0, np.abs(np.nan_to_num(np.asarray(ref_loss, dtype=np.float64), nan=0.0, posinf=0.0)))
    finite = ~np.isnan(np.asarray(ref_loss, dtype=np.float64))
    err = np.where(finite, np.abs(np.nan_to_num(np.asarray(loss, dtype=np.float64) - ref_loss)), 0.0)
    y_dx, e_dx = _maxerr(a_dx, ref_dx), _maxerr(dx, ref_dx)
    print("%s %s: loss err %.3e (ATen %.3e), grad err %.3e (ATen %.3e)" % (case["id"], str(dtype)[6:], e_loss, y_loss, e_dx, y_dx))
    assert (err <= np.maximum(4 * y_loss, 4 * 2.0 ** -23 * scale)).all(), (e_loss, y_loss)
    ok = ~np.isnan(ref_dx)
    d = np.where(ok, np.abs(np.nan_to_num(dx.astype(np.float64)) - np.nan_to_num(ref_dx)), 0.0)
    wabs = np.abs(np.nan_to_num(w, posinf=0.0))[:, None]
    if dtype == torch.float32:
        assert (d <= np.maximum(4 * y_dx, 8 * 2.0 ** -24 * wabs)).all(), (e_dx, y_dx)
    else:
        assert (d <= 2.0 ** -8 * np.abs(np.nan_to_num(ref_dx)) + 8 * 2.0 ** -24 * wabs).all(), e_dx
    ign = t == R.IGNORE
    assert (dx[ign] == 0).all()                                  # ignored rows: exact zeros
    if red == "none":
        assert (loss[ign] == 0).all()


def test_split_max_and_log_sum_at_large_logits():
    """1e4 + randn in fp32: a kernel that kept lse = m + log l would be 1e-3 / 100x off; the bound here is the floor alone"""
    from mas_hip import ops
    dev = _dev()
    case = dict(kind="big1e4", v=2049, rows=5, layout="contig", reduction="none", eps=0.0, ignore=False)
    x32, t, g = R.make_case(case, torch.float32)
    ref_loss, ref_dx, w = R.ce_ref(x32, t, "none", R.IGNORE, 0.0, g)
    view, tt = _place(x32, t, case, torch.float32, dev)
    loss, dx = _run(lambda a, b: ops.cross_entropy(a, b, reduction="none"), view, tt, case, g, dev)
    e_loss, e_dx = _maxerr(loss.cpu().numpy(), ref_loss), _maxerr(dx.cpu().numpy(), ref_dx)
    print("1e4 + randn, V = 2049, fp32: loss err %.3e, grad err %.3e" % (e_loss, e_dx))
    assert e_loss <= 4 * 2.0 ** -23 * max(1.0, float(np.abs(ref_loss).max())) and e_dx <= 8 * 2.0 ** -24 * float(np.abs(w).max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_rows_times_classes_past_2_31(dtype):
    """rows * V = 2^31 + V elements: the last rows sit past a 32-bit element index, in the logits and in the gradient"""
    from mas_hip import ops
    dev = _dev()
    v = 8192
    rows = (1 << 31) // v + 1
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.empty((rows, v), dtype=dtype, device=dev).normal_(generator=gen)
    t = torch.randint(0, v, (rows,), device=dev, generator=gen)
    pick = [0, 1, rows - 2, rows - 1]
    xin = x.requires_grad_(True)
    loss = ops.cross_entropy(xin, t, reduction="sum")
    loss.backward()
    rl, rdx, w = R.ce_ref(x.detach()[pick].double().cpu().numpy(), t[pick].cpu().numpy(), "none", R.IGNORE, 0.0, 1.0)
    dx = xin.grad[pick].double().cpu().numpy()
    assert (np.abs(dx - rdx) <= (2.0 ** -8 if dtype == torch.bfloat16 else 0.0) * np.abs(rdx) + 8 * 2.0 ** -24).all()      # w = 1
    per_row = ops.cross_entropy(x.detach(), t, reduction="none")
    assert np.abs(per_row[pick].double().cpu().numpy() - rl).max() <= 4 * 2.0 ** -23 * max(1.0, float(np.abs(rl).max()))
    assert abs(float(loss) - float(per_row.double().sum())) <= 2.0 ** -23 * abs(float(loss))     # the fp64 sum, rounded once
    del xin, x, loss


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_calls_give_identical_bits(dtype):
    from mas_hip import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 37, 2049, generator=gen).to(dev).to(dtype)
    t = torch.randint(0, 2049, (2, 37), generator=gen).to(dev)
    t[0, 3] = R.IGNORE
    outs = []
    for _ in range(2):
        xin = x.clone().requires_grad_(True)
        loss = ops.cross_entropy(xin, t, label_smoothing=0.1)
        loss.backward()
        outs.append((loss.detach().clone(), xin.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[0][0])) and outs[0][1].abs().sum() > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_forward_and_backward_capture_into_a_graph(dtype):
    """forward + backward captured once on a side stream (one stream, no branches), replayed twice: the eager bits each time"""
    from mas_hip import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(12)
    base = torch.randn(2, 9, 2049, generator=gen).to(dev).to(dtype)
    t = torch.randint(0, 2049, (2, 5), generator=gen).to(dev)
    t[1, 4] = R.IGNORE

    def step(xin):
        loss = ops.cross_entropy(xin[:, 2:7], t, label_smoothing=0.1)
        (gx,) = torch.autograd.grad(loss, xin)
        return loss, gx

    xin = base.clone().requires_grad_(True)
    e_loss, e_gx = step(xin)
    e_loss, e_gx = e_loss.detach().clone(), e_gx.clone()
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        step(xin)                                                # warm-up on the capture stream
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_loss, g_gx = step(xin)
    main.wait_stream(side)
    for _ in range(2):
        g_loss.detach().zero_()
        g_gx.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_loss.detach(), e_loss) and torch.equal(g_gx, e_gx)
    assert (e_gx[:, :2] == 0).all() and (e_gx[:, 7:] == 0).all() and e_gx[:, 2:7].abs().sum() > 0
