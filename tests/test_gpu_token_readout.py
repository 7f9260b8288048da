"""``ops.token_readout`` / ``ops.token_agreement`` / ``MakeAScene.validation_metrics`` (csrc/token_readout.hip) on the GPU
against the float64 reference of tests/helpers/token_readout_ref.py, which tests/test_token_readout_cpu.py pins to torch in float64 on the
same cases.

Bounds, per row (the yardstick is the ATen fp32 expression on ``logits.float()`` on the same GPU and ITS maximum error against fp64):
  rank, argmax   EXACTLY the reference's, every row of every case (the reference settles every tie by rule)
  nll            |error| <= max(4 x yardstick, 4 * 2^-23 * max(1, |nll|))               (the bound of tests/test_gpu_token_loss.py)
  entropy        |error| <= max(4 x yardstick, 8 * 2^-23 * max(1, log V))
The entropy floor of 8 ulp of max(1, log V): log l, the quotient and the difference are rounded once each (3 ulp of a value <= log V), and
each of the two sums carries the fast exp's 2 ulp plus an argument rounded at |x - m| and another summation order.
Sentinels of ignored and invalid rows, counts, hits, histogram: exact.  Position sums: bit-equal to the ordered fp64 sum of the kernel's
own fp32 rows."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import token_readout_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
ULP = 2.0 ** -23
ACC_FIELDS = ("nll_sum", "entropy_sum", "count", "hits", "rank_hist", "invalid")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _place(x32, t, layout, dtype, dev):
    """the case's logits on the device in its layout -> (logits view, target of the view's leading shape)"""
    rows, v = x32.shape
    x = torch.from_numpy(x32).to(dev).to(dtype)
    tt = torch.from_numpy(t).to(dev)
    if layout == "slice":                                        # the [2, 3, V] slice of [2, 5, V]
        base = torch.full((2, 5, v), 777.0, dtype=dtype, device=dev)
        base[:, 1:4] = x.view(2, 3, v)
        view = base[:, 1:4]
        assert not view.is_contiguous()
        return view, tt.view(2, 3)
    if layout == "offset":                                       # starts 4 bytes off a 16-byte boundary
        k = 4 // x.element_size()
        buf = torch.zeros(rows * v + 64, dtype=dtype, device=dev)
        view = buf[k:k + rows * v].view(rows, v)
        view.copy_(x)
        assert view.data_ptr() % 16 == 4
        return view, tt
    if layout == "far":                                          # [2, 3, V] whose outer stride is 2^31 + 8 elements: 64-bit offsets
        stride = (1 << 31) + 8
        buf = torch.empty(stride + 3 * v, dtype=dtype, device=dev)
        view = buf.as_strided((2, 3, v), (stride, v, 1))
        view.copy_(x.view(2, 3, v))
        assert not view.is_contiguous() and view.stride(0) > 2 ** 31
        return view, tt.view(2, 3)
    return x, tt


def _aten(view, tt, v):
    """the yardstick: the ATen fp32 expression on logits.float() -> (nll, entropy) float64 numpy [rows]; rows ATen would device-assert
    on (a target outside [0, V)) are ignored rows for it"""
    xf = view.float().reshape(-1, v)
    t = tt.reshape(-1)
    safe = torch.where((t < 0) | (t >= v), torch.full_like(t, R.IGNORE), t)
    nll = F.cross_entropy(xf, safe, reduction="none", ignore_index=R.IGNORE)
    logp = torch.log_softmax(xf, dim=-1)
    ent = -torch.where(torch.isneginf(logp), torch.zeros_like(logp), logp.exp() * logp).sum(-1)
    return nll.double().cpu().numpy(), ent.double().cpu().numpy()


def _check_rows(got, x32, t, view, tt, label):
    """every assertion on the four per-row outputs of one case; prints the measured errors before it asserts"""
    rows, v = x32.shape
    nll, ent, rank, arg = got
    assert nll.dtype == ent.dtype == torch.float32 and rank.dtype == arg.dtype == torch.int32
    assert nll.shape == ent.shape == rank.shape == arg.shape == tt.shape
    nll, ent = nll.reshape(-1).double().cpu().numpy(), ent.reshape(-1).double().cpu().numpy()
    rank, arg = rank.reshape(-1).cpu().numpy().astype(np.int64), arg.reshape(-1).cpu().numpy().astype(np.int64)
    r_nll, r_ent, r_arg, r_rank = R.readout_ref(x32, t)
    assert np.array_equal(rank, r_rank), (label, np.nonzero(rank != r_rank)[0][:8])
    assert np.array_equal(arg, r_arg), (label, np.nonzero(arg != r_arg)[0][:8])
    ign = t == R.IGNORE
    inv = ~ign & (r_arg < 0)
    assert (nll[ign] == 0).all() and (ent[ign] == 0).all()       # (rank = argmax = -1 were compared above)
    assert np.isnan(nll[inv]).all() and np.isnan(ent[inv]).all() and (rank[inv] == v).all() and (arg[inv] == -1).all()
    ok = ~ign & ~inv
    if not ok.any():
        print("%s: no counted row" % label)
        return
    a_nll, a_ent = _aten(view, tt, v)
    assert not np.isnan(nll[ok]).any() and not np.isnan(ent[ok]).any()
    assert np.array_equal(np.isinf(nll[ok]), np.isinf(r_nll[ok])) and (nll[ok][np.isinf(nll[ok])] > 0).all()     # x_t = -inf: +inf
    fin = ok & np.isfinite(r_nll)
    err = lambda a, b, m: float(np.abs(a[m] - b[m]).max()) if m.any() else 0.0  # noqa: E731
    y_nll, e_nll, y_ent, e_ent = err(a_nll, r_nll, fin), err(nll, r_nll, fin), err(a_ent, r_ent, ok), err(ent, r_ent, ok)
    print("%s: nll err %.3e (ATen %.3e), entropy err %.3e (ATen %.3e)" % (label, e_nll, y_nll, e_ent, y_ent))
    assert (np.abs(nll[fin] - r_nll[fin]) <= np.maximum(4 * y_nll, 4 * ULP * np.maximum(1.0, np.abs(r_nll[fin])))).all(), (e_nll, y_nll)
    assert (np.abs(ent[ok] - r_ent[ok]) <= max(4 * y_ent, 8 * ULP * max(1.0, math.log(v)))).all(), (e_ent, y_ent)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.CASES, ids=[c["id"] for c in R.CASES])
def test_readout_vs_fp64(case, dtype):
    from mas_hip import ops
    dev = _dev()
    x32, t = R.make_case(case, dtype)
    view, tt = _place(x32, t, case["layout"], dtype, dev)
    before = view.clone()
    got = ops.token_readout(view, tt, ignore_index=R.IGNORE)
    assert torch.equal(view, before) or case["kind"] == "nan_row"
    _check_rows(got, x32, t, view, tt, "%s %s" % (case["id"], str(dtype)[6:]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_outer_stride_past_2_31(dtype):
    """a [2, 3, 2049] slice whose second batch starts 2^31 + 8 elements after the first: the row offset needs 64 bits"""
    from mas_hip import ops
    dev = _dev()
    case = dict(kind="randn", v=2049, rows=6, layout="far", ignore=False)
    x32, t = R.make_case(case, dtype, seed=3)
    view, tt = _place(x32, t, "far", dtype, dev)
    got = ops.token_readout(view, tt)
    _check_rows(got, x32, t, view, tt, "far-V2049 %s" % str(dtype)[6:])
    acc = ops.token_agreement(view, tt, ks=(1, 5))
    assert int(acc.count.sum()) == 6 and tuple(acc.count.shape) == (3,)
    del view, got


# (dtype, V, ld or None for a contiguous [6, V], the branch of the row walk it reaches); "slice": the [2, 3, V] slice of [2, 5, V]
SAME_WALK = [
    (torch.bfloat16, 8, None, "one unit, no tail"),
    (torch.bfloat16, 8192, None, "the last fully resident row"),
    (torch.bfloat16, 8200, None, "first streaming row, units only"),
    (torch.bfloat16, 2049, 2056, "resident with a one-element tail"),
    (torch.bfloat16, 2049, None, "ld = 2049: unaligned rows stream element by element"),
    (torch.float32, 4096, None, "resident limit"),
    (torch.float32, 4100, None, "streaming"),
    (torch.float32, 1003, 1004, "resident, three-element tail"),
    (torch.bfloat16, 2049, "slice", "outer_stride != inner * ld"),
    (torch.float32, 2049, "slice", "outer_stride != inner * ld"),
]


@pytest.mark.parametrize("dtype,v,ld,branch", SAME_WALK, ids=["%s-V%d-%s" % (str(c[0])[6:], c[1], c[2]) for c in SAME_WALK])
def test_nll_is_the_loss_row_value_bit_for_bit(dtype, v, ld, branch):
    """the read-out's nll and cross_entropy(reduction="none", label_smoothing=0) walk a row with the same code (csrc/token_row_core.h) and
    form m, l and (m - x_t) + log l with the same fp32 operations in the same order: equal bits, not close values.  Finite logits at two
    scales, valid targets and one ignored row (both give 0)."""
    from mas_hip import ops
    dev = _dev()
    for scale in (1.0, 30.0):
        g = torch.Generator().manual_seed(1000 * v + int(scale))
        x = (torch.randn(6, v, generator=g) * scale).to(dev).to(dtype)
        t = torch.randint(0, v, (6,), generator=g).to(dev)
        t[4] = R.IGNORE
        if ld == "slice":
            base = torch.full((2, 5, v), 777.0, dtype=dtype, device=dev)
            base[:, 1:4] = x.view(2, 3, v)
            view, tt = base[:, 1:4], t.view(2, 3)
            assert not view.is_contiguous() and view.stride(0) != view.shape[1] * view.stride(1)
        elif ld is not None:
            buf = torch.zeros(1, 6, ld, dtype=dtype, device=dev)
            buf[0, :, :v] = x
            view, tt = buf[:, :, :v], t.view(1, 6)
            assert not view.is_contiguous() and view.stride(1) == ld and (ld * view.element_size()) % 16 == 0
        else:
            view, tt = x, t
        nll = ops.token_readout(view, tt, ignore_index=R.IGNORE)[0]
        loss = ops.cross_entropy(view, tt, reduction="none", ignore_index=R.IGNORE, label_smoothing=0.0)
        assert nll.shape == tt.shape and torch.isfinite(nll).all() and float(nll.reshape(-1)[4]) == 0.0
        assert torch.equal(nll, loss), (branch, scale, (nll - loss).abs().max().item())


def _acc_numpy(acc):
    return {k: getattr(acc, k).cpu().numpy() for k in ACC_FIELDS}


def _assert_acc_equal(got, ref, label):
    for k in ACC_FIELDS:
        g, r = got[k], ref[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (label, k, g.shape, r.shape, g.dtype, r.dtype)
        assert np.array_equal(g, r, equal_nan=True), (label, k)   # floats: bit-equal (no -0.0 can arise from a sum that starts at +0.0)


def _acc_case(rows, v, dtype, seed, dev):
    """randn logits with an ignored row, a NaN row and a target outside [0, V) among them (where there are rows enough)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, v)).astype(np.float32) * 2.0
    t = rng.integers(0, v, size=rows).astype(np.int64)
    if rows >= 9:
        t[2], t[rows - 1] = R.IGNORE, v
        x[5, v // 2] = np.nan
        x[7, t[7]] += 30.0                                       # a sure top-1 hit
    x = torch.from_numpy(x).to(dtype).float().numpy()
    return x, t, torch.from_numpy(x).to(dev).to(dtype), torch.from_numpy(t).to(dev)


KS_SETS = [(1,), (1, 5), (1, 2, 3, 5, 10, 64, 255, 1000)]        # the last: eight thresholds, one above V = 256


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("ks", KS_SETS, ids=["k1", "k1_5", "k8"])
@pytest.mark.parametrize("rows,L", [(3, 1), (9, 3), (3072, 1024), (257, 1)], ids=["L1", "L3", "L1024", "L1x257"])
def test_accumulation_is_exact_and_ordered(rows, L, ks, dtype):
    from mas_hip import ops
    dev = _dev()
    v = 256                                                      # every row 16-byte aligned: a row's bits do not depend on its index
    x32, t, x, tt = _acc_case(rows, v, dtype, 17 + rows, dev)
    nll, ent, rank, arg = (o.cpu().numpy() for o in ops.token_readout(x, tt))
    assert np.array_equal(rank.astype(np.int64), R.readout_ref(x32, t)[3])
    first = ops.token_agreement(x.view(rows // L, L, v), tt.view(rows // L, L), ks=ks)            # positions defaults to L
    assert first.ks == ks and first.positions == L
    ref1 = R.accumulate_ref(nll, ent, arg, rank, t, L, ks)
    _assert_acc_equal(_acc_numpy(first), ref1, "one call")
    n_ign, n_inv = int((t == R.IGNORE).sum()), int(((t != R.IGNORE) & (arg < 0)).sum())
    assert int(first.invalid) == n_inv == (2 if rows >= 9 else 0) and int(first.count.sum()) == rows - n_ign - n_inv
    assert int(first.rank_hist.sum()) == int(first.count.sum()) and (first.hits[:, -1] <= first.count).all()
    if ks[-1] > v:
        assert torch.equal(first.hits[:, -1], first.count)       # a threshold above V: every counted row is a hit
    # a second batch into the same holder: the held value takes ONE addition of the second batch's local sums
    y32, u, y, uu = _acc_case(rows, v, dtype, 99 + rows, dev)
    n2, e2, r2, a2 = (o.cpu().numpy() for o in ops.token_readout(y, uu))
    same = ops.token_agreement(y, uu, positions=L, ks=ks, out=first)
    assert same is first
    ref2 = R.accumulate_ref(n2, e2, a2, r2, u, L, ks, into=ref1)
    _assert_acc_equal(_acc_numpy(first), ref2, "two calls")
    # ... and equals one call on the concatenation: integers exactly, sums up to the one regrouping (a + b) + (c + d) vs ((a + b) + c) + d
    both = ops.token_agreement(torch.cat([x, y]), torch.cat([tt, uu]), positions=L, ks=ks)
    for k in ("count", "hits", "rank_hist", "invalid"):
        assert torch.equal(getattr(both, k), getattr(first, k)), k
    cat_rows = [o.cpu().numpy() for o in ops.token_readout(torch.cat([x, y]), torch.cat([tt, uu]))]
    for a, b in zip(cat_rows, (np.concatenate([nll, n2]), np.concatenate([ent, e2]), np.concatenate([rank, r2]), np.concatenate([arg, a2]))):
        assert np.array_equal(a, b, equal_nan=True)              # the rows of the concatenation are the rows of the two batches
    refcat = R.accumulate_ref(cat_rows[0], cat_rows[1], cat_rows[3], cat_rows[2], np.concatenate([t, u]), L, ks)
    _assert_acc_equal(_acc_numpy(both), refcat, "concatenation")
    for k in ("nll_sum", "entropy_sum"):
        a, b = getattr(both, k), getattr(first, k)
        assert ((a - b).abs() <= (2 * rows // L) * 2.0 ** -52 * a.abs()).all(), k     # positive terms: n eps at the most
    with pytest.raises(ValueError, match="out holds"):
        ops.token_agreement(y, uu, positions=L, ks=ks + (7,) if len(ks) < 8 else ks[:-1], out=first)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_calls_give_identical_bits(dtype):
    from mas_hip import ops
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 37, 8200, generator=gen).to(dev).to(dtype)
    t = torch.randint(0, 8200, (2, 37), generator=gen).to(dev)
    t[0, 3] = R.IGNORE
    for xx in (x, x[..., :2049].contiguous()):                   # streaming and register-resident rows
        outs = []
        for _ in range(2):
            tt = t.clamp(max=xx.shape[-1] - 1)
            outs.append(ops.token_readout(xx, tt) + ops.token_agreement(xx, tt, ks=(1, 5, 50)).tensors())
        assert len(outs[0]) == 10
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(outs[0][0]).all()) and int(outs[0][6].sum()) == 2 * 37 - 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_token_agreement_captures_into_a_graph(dtype):
    """one eager call into the holder, then the call captured once (one stream, no branches) and replayed twice without a host read:
    exactly three calls' worth.  The warm-up on the capture stream goes into a holder of its own."""
    from mas_hip import ops
    from mas_hip.tokenmetrics import TokenAgreement
    dev = _dev()
    gen = torch.Generator().manual_seed(12)
    base = torch.randn(2, 9, 2049, generator=gen).to(dev).to(dtype)
    t = torch.randint(0, 2049, (2, 5), generator=gen).to(dev)
    t[1, 4] = R.IGNORE
    ks = (1, 5)
    one = ops.token_agreement(base[:, 2:7], t, ks=ks)
    acc = TokenAgreement(5, ks, device=dev)
    ops.token_agreement(base[:, 2:7], t, ks=ks, out=acc)
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        ops.token_agreement(base[:, 2:7], t, ks=ks, out=TokenAgreement(5, ks, device=dev))      # warm-up on the capture stream
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.token_agreement(base[:, 2:7], t, ks=ks, out=acc)
    main.wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(acc.count, one.count)                     # capturing ran nothing
    torch.cuda.set_sync_debug_mode("error")
    try:
        graph.replay()
        graph.replay()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for k in ("count", "hits", "rank_hist", "invalid"):
        assert torch.equal(getattr(acc, k), 3 * getattr(one, k)), k
    for k in ("nll_sum", "entropy_sum"):
        s = getattr(one, k)
        assert torch.equal(getattr(acc, k), (s + s) + s), k      # the held value takes one addition per call
    assert int(acc.count.sum()) == 27 and float(acc.nll) > 0


# ---- model level ---------------------------------------------------------------------------------------------------------------
CFG = dict(num_layers=2, hidden_dim=64, num_attn_heads=4, image_vocab_size=128, seg_vocab_size=40, text_vocab_size=58,
           image_tokens_per_dim=4, seg_tokens_per_dim=2, text_length=8)
B = 3


@pytest.fixture(scope="module")
def model():
    dev = _dev()
    from models.transformer import MakeAScene
    from oracle import transformer_oracle as TO
    m = MakeAScene(**CFG)
    m.load_state_dict(TO.synth_transformer_state_dict(CFG, seed=7), strict=True)
    m = m.to(dev).eval()
    text, seg, img = (t.to(dev) for t in TO.synth_tokens(CFG, batch=B, seed=7))
    return m, text, seg, img


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16_autocast"])
def test_validation_metrics_equal_the_reference_on_forward_logits(model, amp):
    from mas_hip.tokenmetrics import TokenAgreement
    m, text, seg, img = model
    v, L = CFG["image_vocab_size"], CFG["image_tokens_per_dim"] ** 2
    ks = (1, 5)
    with torch.no_grad(), torch.autocast("cuda", dtype=amp, enabled=amp is not None):
        logits = m(text, seg, img)
        got = m.validation_metrics(text, seg, img, ks=ks)
        loss = m.token_loss(text, seg, img, reduction="mean")
    assert isinstance(got, TokenAgreement) and got.positions == L and got.ks == ks
    assert logits.dtype == (amp or torch.float32) and tuple(logits.shape) == (B, L, v)
    x64 = logits.double().cpu().numpy().reshape(B * L, v)
    t = img.cpu().numpy().reshape(-1)
    r_nll, r_ent, r_arg, r_rank = R.readout_ref(x64, t)
    ref = R.accumulate_ref(r_nll, r_ent, r_arg, r_rank, t, L, ks)
    g = _acc_numpy(got)
    for k in ("count", "hits", "rank_hist", "invalid"):
        assert np.array_equal(g[k], ref[k]), k
    a_nll, a_ent = _aten(logits, img, v)
    y_nll, y_ent = float(np.abs(a_nll - r_nll).max()), float(np.abs(a_ent - r_ent).max())
    b_nll = np.maximum(4 * y_nll, 4 * ULP * np.maximum(1.0, np.abs(r_nll))).reshape(B, L).sum(0)  # B rows per position, each within its bound
    b_ent = B * max(4 * y_ent, 8 * ULP * max(1.0, math.log(v)))
    print("model %s: nll_sum err %.3e (bound %.3e), entropy_sum err %.3e (bound %.3e)"
          % (amp, np.abs(g["nll_sum"] - ref["nll_sum"]).max(), b_nll.min(), np.abs(g["entropy_sum"] - ref["entropy_sum"]).max(), b_ent))
    assert (np.abs(g["nll_sum"] - ref["nll_sum"]) <= b_nll).all() and (np.abs(g["entropy_sum"] - ref["entropy_sum"]) <= b_ent).all()
    mean = float(r_nll.mean())
    assert abs(float(got.nll) - float(loss)) <= max(4 * y_nll, 4 * ULP * max(1.0, abs(mean)))
    assert abs(float(got.nll) - mean) <= max(4 * y_nll, 4 * ULP * max(1.0, abs(mean)))
    assert float(got.perplexity) == pytest.approx(math.exp(float(got.nll)), rel=1e-12) and tuple(got.grid(4).shape) == (4, 4)
    again = m.validation_metrics(text, seg, img, ks=ks, out=got) if amp is None else None
    if again is not None:
        assert again is got and np.array_equal(again.count.cpu().numpy(), 2 * ref["count"])


def test_validation_metrics_raises_in_training_mode(model):
    m, text, seg, img = model
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.validation_metrics(text, seg, img)
    finally:
        m.eval()
