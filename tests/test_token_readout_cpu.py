"""CPU checks of the stage-2 read-out (csrc/token_readout.hip, ``ops.token_readout`` / ``ops.token_agreement``): the two
entry points are declared, exported and bound under ABI 10 and refuse bad arguments before anything is launched; the float64 reference the
GPU tests measure against (tests/helpers/token_readout_ref.py) equals torch in float64 on every case of the GPU test; ``TokenAgreement``
adds, refuses and derives its numbers without a device."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import token_readout_ref as R  # noqa: E402

ENTRIES = ("mas_token_readout", "mas_token_readout_accumulate")


def test_entries_are_declared_exported_and_bound():
    import mas_hip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mas_hip.h")).read(), flags=re.S)
    assert "#define MAS_ABI_VERSION 10" in txt and mas_hip.ABI_VERSION == 10
    L = mas_hip.lib()
    raw = ctypes.CDLL(mas_hip.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name + " is not declared in include/mas_hip.h"
        assert hasattr(raw, name), name + " is not exported"
        assert name in mas_hip.EXPORTS and getattr(L, name).argtypes == mas_hip._SIGNATURES[name][1]
    assert (mas_hip.TOKEN_MAX_KS, mas_hip.TOKEN_RANK_BINS) == (8, 33) == (R.MAX_KS, R.RANK_BINS)
    for name in ("token_readout.hip", "token_row_core.h", "mas_wave.h"):   # the file and the headers that hold its row walk
        src = open(os.path.join(ROOT, "make-a-scene_amd", "csrc", name)).read()
        assert "asm" not in re.sub(r"//[^\n]*", "", src), name   # no inline assembly in this file


def test_bad_arguments_come_back_as_codes_before_any_launch():
    """null pointers throughout, as tests/test_abi.py does: the shape and threshold checks come first and name what they refuse"""
    import mas_hip
    L = mas_hip.lib()
    ks = (ctypes.c_int * 9)(1, 5, 10, 20, 50, 100, 1000, 10000, 7)

    def acc(rows=6, L_=3, ks=ks, nk=2):
        return L.mas_token_readout_accumulate(None, None, None, None, None, rows, -100, L_, ks, nk, None, None, None, None, None, None, None)

    assert acc(rows=7, L_=3) == mas_hip.EINVAL == -1 and b"multiple" in L.mas_last_error()
    assert acc(nk=9) == -1 and b"thresholds" in L.mas_last_error()
    assert acc(ks=(ctypes.c_int * 2)(1, 0)) == -1 and b"at least 1" in L.mas_last_error()
    assert acc(ks=(ctypes.c_int * 2)(-3, 5)) == -1 and b"at least 1" in L.mas_last_error()
    assert acc(rows=0) == -1 and acc(L_=0) == -1 and b"positive" in L.mas_last_error()
    assert acc(ks=None) == -1 and b"null" in L.mas_last_error()
    assert acc() == -1 and b"null" in L.mas_last_error()         # a valid shape: the null pointers are what is left to refuse
    p = 4096                                                     # any non-null value; never dereferenced on the host

    def ro(logits=p, dtype=mas_hip.BF16, rows=4, V=16, inner=4, outer=0, ld=16, target=p, nll=p, ent=p, arg=p, rank=p):
        return L.mas_token_readout(logits, dtype, rows, V, inner, outer, ld, target, -100, nll, ent, arg, rank, None)

    for kw in (dict(logits=None), dict(target=None), dict(nll=None), dict(ent=None), dict(arg=None), dict(rank=None)):
        assert ro(**kw) == -1 and b"null" in L.mas_last_error(), kw
    for kw in (dict(rows=0), dict(V=0), dict(V=-1), dict(inner=0)):
        assert ro(**kw) == -1 and b"positive" in L.mas_last_error(), kw
    assert ro(ld=-16) == -1 and b"stride" in L.mas_last_error()
    assert ro(dtype=7) == mas_hip.EUNSUPPORTED == -2 and b"dtype" in L.mas_last_error()


def _torch64(x, t):
    """torch in float64 on the CPU for the rows torch accepts -> (nll, entropy, argmax, rank)"""
    xt = torch.from_numpy(x).double()
    tt = torch.from_numpy(t)
    nll = F.cross_entropy(xt, tt, reduction="none").numpy()
    logp = torch.log_softmax(xt, dim=-1)
    ent = -torch.where(torch.isneginf(logp), torch.zeros_like(logp), logp.exp() * logp).sum(-1).numpy()   # the -inf convention
    order = torch.argsort(xt, dim=-1, descending=True, stable=True)
    rank = (order == tt[:, None]).long().argmax(-1).numpy()
    return nll, ent, xt.argmax(-1).numpy(), rank


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.CASES, ids=[c["id"] for c in R.CASES])
def test_reference_equals_torch_float64(case, dtype):
    """the yardstick before a GPU sees it.  Ignored and invalid rows are checked for their sentinels; torch sees the other rows only."""
    x, t = R.make_case(case, dtype)
    v = case["v"]
    nll, ent, arg, rank = R.readout_ref(x, t)
    ign = t == R.IGNORE
    with np.errstate(invalid="ignore"):
        inv = ~ign & ((t < 0) | (t >= v) | np.isnan(x).any(1) | (x == np.inf).any(1) | (x == -np.inf).all(1))
    assert (nll[ign] == 0).all() and (ent[ign] == 0).all() and (arg[ign] == -1).all() and (rank[ign] == -1).all()
    assert np.isnan(nll[inv]).all() and np.isnan(ent[inv]).all() and (arg[inv] == -1).all() and (rank[inv] == v).all()
    ok = ~ign & ~inv
    expect_inv = dict(all_neginf=2, nan_row=3, posinf_row=3, bad_targets=2)
    assert inv.sum() == expect_inv.get(case["kind"], 0) and (case["kind"] != "all_ignored" or ign.all())
    if not ok.any():
        return
    t_nll, t_ent, t_arg, t_rank = _torch64(x[ok], t[ok])
    assert np.array_equal(arg[ok], t_arg) and np.array_equal(rank[ok], t_rank)
    assert not np.isnan(nll[ok]).any() and np.array_equal(np.isinf(nll[ok]), np.isinf(t_nll))
    if case["kind"] == "neginf_target":
        assert np.isinf(nll[ok]).all()
    fin = np.isfinite(t_nll)
    np.testing.assert_allclose(nll[ok][fin], t_nll[fin], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ent[ok], t_ent, rtol=1e-11, atol=1e-12)
    assert (ent[ok] >= -1e-12).all() and (ent[ok] <= math.log(v) + 1e-12).all()
    if case["kind"] == "const":
        assert np.array_equal(rank[ok], t[ok]) and (arg[ok] == 0).all()
        np.testing.assert_allclose(ent[ok], math.log(v), rtol=1e-12)
    if case["kind"] == "ties":
        for r in np.nonzero(ok)[0]:
            assert (x[r, :t[r]] == x[r, t[r]]).sum() >= 8 and (x[r, t[r] + 1:] == x[r, t[r]]).sum() >= 8


def test_case_list_reaches_every_path():
    plain = [c for c in R.CASES if c["kind"] == "randn" and c["layout"] == "contig"]
    assert {c["v"] for c in plain} == set(R.VS) == {1, 7, 8, 255, 2048, 2049, 8192, 8200}
    assert {(c["v"], c["rows"]) for c in plain} == {(v, r) for v in R.VS for r in (1, 3, 257)}
    assert {c["layout"] for c in R.CASES} == {"contig", "slice", "offset"} and {c["kind"] for c in R.CASES} == {"randn", *R.HARD}
    assert any(c["ignore"] for c in plain) and any(not c["ignore"] for c in plain)
    x, _ = R.make_case(dict(kind="randn", v=2048, rows=3, ignore=False), torch.bfloat16)
    assert all(len(np.unique(row)) < 2048 for row in x)         # every bf16 randn row at V >= 2048 holds equal values


def test_accumulation_order_and_bins():
    assert [R.rank_bin(k) for k in (0, 1, 2, 3, 4, 7, 8, 2 ** 31 - 1)] == [0, 1, 2, 2, 3, 3, 4, 31]
    rng = np.random.default_rng(5)
    L, rows, ks = 3, 12, (1, 5)
    nll = rng.random(rows).astype(np.float32) * 9
    ent = rng.random(rows).astype(np.float32)
    rank = rng.integers(0, 9, rows)
    arg = rng.integers(0, 9, rows)
    t = rng.integers(0, 9, rows)
    t[4] = R.IGNORE
    arg[7], rank[7], nll[7], ent[7] = -1, 9, np.nan, np.nan     # an invalid row
    acc = R.accumulate_ref(nll, ent, arg, rank, t, L, ks)
    keep = (t != R.IGNORE) & (arg >= 0)
    assert acc["invalid"][0] == 1 and acc["count"].sum() == 10 and acc["rank_hist"].sum() == 10
    for p in range(L):
        rs = [r for r in range(p, rows, L) if keep[r]]
        s = 0.0
        for r in rs:
            s += float(nll[r])
        assert acc["nll_sum"][p] == s and acc["count"][p] == len(rs)
        assert acc["hits"][p, 0] == sum(rank[r] < 1 for r in rs) and acc["hits"][p, 1] == sum(rank[r] < 5 for r in rs)
    twice = R.accumulate_ref(nll, ent, arg, rank, t, L, ks, into=R.accumulate_ref(nll, ent, arg, rank, t, L, ks))
    assert np.array_equal(twice["count"], 2 * acc["count"]) and np.array_equal(twice["nll_sum"], acc["nll_sum"] + acc["nll_sum"])


def test_token_agreement_holder_arithmetic():
    from mas_hip.tokenmetrics import MAX_KS, RANK_BINS, TokenAgreement
    assert (MAX_KS, RANK_BINS) == (8, 33)
    a, b = TokenAgreement(4, (1, 5)), TokenAgreement(4, (1, 5))
    assert [tuple(t.shape) for t in a.tensors()] == [(4,), (4,), (4,), (4, 2), (33,), (1,)]
    assert [t.dtype for t in a.tensors()] == [torch.float64, torch.float64] + [torch.int64] * 4
    a.nll_sum += torch.tensor([2.0, 4.0, 0.0, 6.0], dtype=torch.float64)
    a.entropy_sum += torch.tensor([1.0, 1.0, 0.0, 1.0], dtype=torch.float64)
    a.count += torch.tensor([1, 2, 0, 3])
    a.hits += torch.tensor([[1, 1], [0, 2], [0, 0], [1, 3]])
    a.rank_hist[0] += 2
    a.rank_hist[2] += 4
    b.nll_sum += 1.0
    b.count += 1
    b.invalid += 2
    assert float(a.nll) == 2.0 and float(a.perplexity) == pytest.approx(math.exp(2.0), rel=1e-15)
    assert float(a.bits_per_token) == pytest.approx(2.0 / math.log(2.0), rel=1e-15) and float(a.mean_entropy) == 0.5
    assert a.accuracy.tolist() == [2 / 6, 1.0] and a.accuracy.dtype == torch.float64
    by = a.nll_by_position
    assert by.tolist()[:2] == [2.0, 2.0] and math.isnan(by[2]) and by[3] == 2.0
    acc = a.accuracy_by_position
    assert tuple(acc.shape) == (4,) and acc[0] == 1.0 and acc[1] == 0.0 and math.isnan(acc[2]) and float(acc[3]) == pytest.approx(1 / 3)
    assert tuple(a.topk_by_position.shape) == (4, 2) and tuple(a.grid(2).shape) == (2, 2) and torch.equal(a.grid(2)[1, 1], by[3])
    assert tuple(a.grid(2, a.topk_by_position).shape) == (2, 2, 2)
    with pytest.raises(ValueError, match="grid"):
        a.grid(3)
    c = a + b
    assert c.count.tolist() == [2, 3, 1, 4] and c.nll_sum.tolist() == [3.0, 5.0, 1.0, 7.0] and int(c.invalid) == 2 and int(a.invalid) == 0
    held = a.count
    a += b
    assert a.count is held and a.count.tolist() == [2, 3, 1, 4] and int(a.invalid) == 2 and int(a.rank_hist.sum()) == 6
    for other in (TokenAgreement(4, (1,)), TokenAgreement(4, (1, 6)), TokenAgreement(5, (1, 5))):
        with pytest.raises(ValueError, match="cannot be added"):
            a += other
        with pytest.raises(ValueError, match="cannot be added"):
            a + other
    with pytest.raises(ValueError, match="cannot add"):
        a + 3
    for ks in ((), (0,), (1, -2), tuple(range(1, 10)), (1.5,), "ab"):
        with pytest.raises(ValueError, match="ks"):
            TokenAgreement(4, ks)
    with pytest.raises(ValueError, match="positive"):
        TokenAgreement(0)
    with pytest.raises(ValueError, match="count"):
        TokenAgreement(4, (1, 5), tensors=[t.float() if i == 2 else t for i, t in enumerate(b.tensors())])
    empty = TokenAgreement(2, (1,))
    assert math.isnan(empty.nll) and math.isnan(empty.accuracy[0]) and torch.isnan(empty.nll_by_position).all()


def test_python_surface_raises_without_a_device():
    from mas_hip import ops
    from mas_hip.tokenmetrics import TokenAgreement
    x, t = torch.randn(2, 3, 16), torch.randint(0, 16, (2, 3))
    for fn in (ops.token_readout, ops.token_agreement):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, t)
        with pytest.raises(ValueError, match="probability"):
            fn(x, torch.softmax(x, -1)[..., 0])
        with pytest.raises(ValueError, match="shape"):
            fn(x, t[:1])
    with pytest.raises(ValueError, match="ks"):
        ops.token_agreement(x, t, ks=(0,))
    with pytest.raises(ValueError, match="multiple"):
        ops.token_agreement(x, t, positions=4)
    for out in (TokenAgreement(3, (1,)), TokenAgreement(2, (1, 5))):
        with pytest.raises(ValueError, match="out holds"):
            ops.token_agreement(x, t, out=out)
    with pytest.raises(ValueError, match="TokenAgreement"):
        ops.token_agreement(x, t, out=torch.zeros(3))


def test_model_surface_has_validation_metrics():
    from models.transformer import MakeAScene
    m = MakeAScene(num_layers=1, hidden_dim=32, num_attn_heads=2, image_vocab_size=32, seg_vocab_size=8, text_vocab_size=16,
                   image_tokens_per_dim=2, seg_tokens_per_dim=1, text_length=4)
    assert "forward()" in MakeAScene.validation_metrics.__doc__ and "ops.token_agreement(" in MakeAScene.validation_metrics.__doc__
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.validation_metrics(torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
