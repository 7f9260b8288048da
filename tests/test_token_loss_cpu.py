"""CPU checks of the token cross-entropy (csrc/token_loss.hip, ``mas_hip.ops.cross_entropy``): the three entry points are declared,
exported and bound (ABI 9, 10 today) and refuse bad arguments before anything is launched; the float64 reference the GPU tests measure
against (tests/helpers/token_ce_ref.py) equals ``F.cross_entropy`` in float64 on every case of the GPU test; the Python surface raises
without touching a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import token_ce_ref as R  # noqa: E402

ENTRIES = ("mas_token_ce_fwd", "mas_token_ce_reduce", "mas_token_ce_bwd")


def test_entries_are_declared_exported_and_bound():
    import mas_hip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mas_hip.h")).read(), flags=re.S)
    assert "#define MAS_ABI_VERSION 10" in txt and mas_hip.ABI_VERSION == 10
    L = mas_hip.lib()
    assert L.mas_abi_version() == 10
    raw = ctypes.CDLL(mas_hip.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name + " is not declared in include/mas_hip.h"
        assert hasattr(raw, name), name + " is not exported"
        assert name in mas_hip.EXPORTS and getattr(L, name).argtypes == mas_hip._SIGNATURES[name][1]
    assert (mas_hip.CE_NONE, mas_hip.CE_MEAN, mas_hip.CE_SUM) == (0, 1, 2)
    assert re.search(r"MAS_CE_NONE\s*=\s*0,\s*MAS_CE_MEAN\s*=\s*1,\s*MAS_CE_SUM\s*=\s*2", txt)


def test_bad_arguments_come_back_as_codes_before_any_launch():
    """nothing here is a device pointer: a launch would fault, a code with a message comes back instead"""
    import mas_hip
    L = mas_hip.lib()
    p = 4096                                                     # any non-null value; never dereferenced on the host
    ok_fwd = dict(logits=p, dtype=mas_hip.BF16, rows=4, V=16, inner=4, outer=0, ld=16, target=p, ignore=-100, eps=0.0, row_loss=p, stats=p)

    def fwd(**kw):
        a = dict(ok_fwd, **kw)
        return L.mas_token_ce_fwd(a["logits"], a["dtype"], a["rows"], a["V"], a["inner"], a["outer"], a["ld"], a["target"], a["ignore"],
                                  a["eps"], a["row_loss"], a["stats"], None)

    def bwd(reduction=mas_hip.CE_SUM, loss_count=p, **kw):
        a = dict(ok_fwd, **kw)
        return L.mas_token_ce_bwd(a["logits"], a["dtype"], a["rows"], a["V"], a["inner"], a["outer"], a["ld"], a["target"], a["ignore"],
                                  a["eps"], a["stats"], kw.get("grad", p), loss_count, reduction, kw.get("dx", p), None)

    for call in (fwd, bwd):
        for kw in (dict(logits=None), dict(target=None), dict(stats=None)):
            assert call(**kw) == -1 and b"null" in L.mas_last_error(), kw
        for kw in (dict(rows=0), dict(rows=-3), dict(V=0), dict(V=-1), dict(inner=0)):
            assert call(**kw) == -1 and b"positive" in L.mas_last_error(), kw
        assert call(ld=-16) == -1 and b"stride" in L.mas_last_error()
        assert call(eps=1.5) == -1 and b"label_smoothing" in L.mas_last_error()
        assert call(eps=float("nan")) == -1
        assert call(dtype=7) == -2 and b"dtype" in L.mas_last_error()
    assert fwd(row_loss=None) == -1 and b"null" in L.mas_last_error()
    assert bwd(grad=None) == -1 and bwd(dx=None) == -1
    assert bwd(reduction=3) == -1 and b"reduction" in L.mas_last_error()
    assert bwd(reduction=mas_hip.CE_MEAN, loss_count=None) == -1 and b"count" in L.mas_last_error()
    assert L.mas_token_ce_reduce(None, p, 4, -100, mas_hip.CE_MEAN, p, None) == -1 and b"null" in L.mas_last_error()
    assert L.mas_token_ce_reduce(p, p, 4, -100, mas_hip.CE_MEAN, None, None) == -1
    assert L.mas_token_ce_reduce(p, p, 0, -100, mas_hip.CE_MEAN, p, None) == -1 and b"positive" in L.mas_last_error()
    for bad in (mas_hip.CE_NONE, 3, -1):
        assert L.mas_token_ce_reduce(p, p, 4, -100, bad, p, None) == -1 and b"reduction" in L.mas_last_error()


def _torch64(x, t, reduction, eps, g):
    xt = torch.from_numpy(x).double().requires_grad_(True)
    loss = F.cross_entropy(xt, torch.from_numpy(t), reduction=reduction, ignore_index=R.IGNORE, label_smoothing=eps)
    loss.backward(torch.as_tensor(g).double())
    return loss.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.CASES, ids=[c["id"] for c in R.CASES])
def test_reference_equals_torch_float64(case, dtype):
    """the yardstick before a GPU sees it.  torch raises on a target outside [0, V): those rows are checked for NaN and compared as
    ignored rows (reduction "none", so no other row feels them)."""
    x, t, g = R.make_case(case, dtype)
    loss, dx, w = R.ce_ref(x, t, case["reduction"], R.IGNORE, case["eps"], g)
    assert (w[t == R.IGNORE] == 0).all()
    bad = (t != R.IGNORE) & ((t < 0) | (t >= case["v"]))
    if bad.any():
        assert case["reduction"] == "none" and np.isnan(loss[bad]).all() and np.isnan(dx[bad]).all()
        assert np.isfinite(loss[~bad]).all() and np.isfinite(dx[~bad]).all()
        t = np.where(bad, R.IGNORE, t)
        loss, dx = np.where(bad, 0.0, loss), np.where(bad[:, None], 0.0, dx)
    ref_loss, ref_dx = _torch64(x, t, case["reduction"], case["eps"], g)
    assert np.shape(loss) == ref_loss.shape and dx.shape == ref_dx.shape
    if case["kind"] == "all_ignored" and case["reduction"] == "mean":
        assert np.isnan(loss) and np.isnan(ref_loss) and (dx == 0).all()
        return
    assert np.isfinite(ref_loss).all() and np.isfinite(ref_dx).all()
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dx, ref_dx, rtol=1e-11, atol=1e-14)


def test_case_list_reaches_every_path():
    vs = {c["v"] for c in R.CASES if c["kind"] == "randn" and c["layout"] == "contig"}
    assert vs == set(R.VS) == {1, 7, 8, 255, 2048, 2049, 8192, 8200}
    assert {c["rows"] for c in R.CASES if c["kind"] == "randn" and c["layout"] == "contig"} == {1, 3, 257}
    assert {c["layout"] for c in R.CASES} == {"contig", "slice", "offset"} and {c["kind"] for c in R.CASES} == {"randn", *R.HARD}
    for red in R.REDUCTIONS:
        for eps in (0.0, 0.1):
            assert any(c["reduction"] == red and c["eps"] == eps for c in R.CASES), (red, eps)
            assert any(c["reduction"] == red and c["eps"] == eps and c["ignore"] for c in R.CASES), (red, eps)


def test_cross_entropy_raises_without_a_device():
    from mas_hip import ops
    x, t = torch.randn(4, 16), torch.randint(0, 16, (4,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cross_entropy(x, t)
    with pytest.raises(ValueError, match="reduction"):
        ops.cross_entropy(x, t, reduction="batchmean")
    for eps in (-0.1, 1.5):
        with pytest.raises(ValueError, match="label_smoothing"):
            ops.cross_entropy(x, t, label_smoothing=eps)
    with pytest.raises(ValueError, match="probability"):
        ops.cross_entropy(x, torch.softmax(x, -1))
    with pytest.raises(ValueError, match="weight"):
        ops.cross_entropy(x, t, weight=torch.ones(16))
    with pytest.raises(ValueError, match="shape"):
        ops.cross_entropy(x, t[:3])


def test_model_surface_has_token_loss_and_log_likelihood():
    from models.transformer import MakeAScene
    m = MakeAScene(num_layers=1, hidden_dim=32, num_attn_heads=2, image_vocab_size=32, seg_vocab_size=8, text_vocab_size=16,
                   image_tokens_per_dim=2, seg_tokens_per_dim=1, text_length=4)
    assert callable(m.token_loss) and callable(m.log_likelihood)
    assert "rerank" in MakeAScene.log_likelihood.__doc__.lower() and "forward()" in MakeAScene.token_loss.__doc__
