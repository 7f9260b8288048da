"""The row-wise attention check (tests/helpers/attn_rowwise_check.py) has teeth, shown without a GPU:

  * its fp64 reference equals the plain oracle (``oracle.transformer_oracle.causal_attention_scores`` + softmax) on the gauss inputs;
  * the onehot and uniform preconditions hold for every case, head width 16 included;
  * REQUIRED is what the cases reach when every case takes the kernel it names;
  * a CPU model of the kernels' arithmetic (fp32 online softmax over 32- / 64-key tiles, P and dS cast to bf16 where the kernels cast)
    stays inside the bounds in every mode of every case;
  * each mutation of that model (CHK.MUTATIONS) lands outside the bounds or breaks an exact check in at least one case, and the printed table
    says which of them the old criterion, max|got - ref| / max|ref| < 3e-2 (gradients 6e-2) on the gauss inputs, lets through.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import attn_rowwise_check as CHK  # noqa: E402

_cache = {}


def prepared(c, mode):
    """inputs, dropout Z and reference of a (case, mode): computed once, shared, never modified"""
    key = (c["name"], mode)
    if key not in _cache:
        ins = CHK.make_inputs(c, mode)
        Z = CHK.drop_z(c)
        _cache[key] = (ins, Z, CHK.reference(ins, Z))
    return _cache[key]


def _by_name(name):
    return next(c for c in CHK.CASES if c["name"] == name)


def test_case_names_are_unique_and_families_known():
    names = [c["name"] for c in CHK.CASES]
    assert len(set(names)) == len(names)
    assert {c["family"] for c in CHK.CASES} == set(CHK.FAMILIES)
    assert {c["S"] for c in CHK.CASES} == set(CHK.S_ALL) and max(CHK.S_ALL) == 321


def test_required_is_reached_by_the_cases():
    got = CHK.reached([(c, c["fwd"], c["bwd"] if c["bwd_layout"] else None) for c in CHK.CASES])
    for kern, feats in CHK.REQUIRED.items():
        assert feats <= got.get(kern, set()), (kern, sorted(feats - got.get(kern, set())))


@pytest.mark.parametrize("name", ["v2_fast64-bf16-hd64-B2H3S129-fused", "bf16_generic-bf16-hd16-B2H3S33-fused", "f32_generic-f32-hd128-B2H3S257-fused",
                                  "f32_generic-f32-hd32-B1H1S65-fused"])
def test_reference_equals_oracle(name):
    from oracle import transformer_oracle as TO
    c = _by_name(name)
    ins, _, ref = prepared(c, "gauss")
    q, k, v = (torch.from_numpy(ins[n]) for n in ("q", "k", "v"))
    S = c["S"]
    assert ins["scale"] == float(np.float32(c["hd"] ** -0.5))
    mask = torch.tril(torch.ones(S, S, dtype=torch.float64))[None, None]
    probs = torch.softmax(TO.causal_attention_scores(q, k, mask, c["hd"]), dim=-1)
    o = torch.matmul(probs, v).numpy()
    # (the helper's scale is hd^-0.5 rounded to fp32, the operand the kernel gets: 6e-8 relative on the scores)
    assert np.abs(probs.numpy() - ref["P"]).max() < 1e-6
    assert np.abs(o - ref["o"]).max() < 1e-6 * np.abs(ref["A_o"]).max()
    # and the gradients against autograd on the same formula
    qkv = [torch.from_numpy(ins[n]).requires_grad_(True) for n in ("q", "k", "v")]
    s = torch.matmul(qkv[0], qkv[1].transpose(-1, -2)) * ins["scale"]
    s = s.masked_fill(mask == 0, float("-inf"))
    out = torch.matmul(torch.softmax(s, dim=-1), qkv[2])
    out.backward(torch.from_numpy(ins["do"]))
    assert np.abs(out.detach().numpy() - ref["o"]).max() < 1e-12 * max(1.0, np.abs(ref["A_o"]).max())
    assert np.abs(torch.logsumexp(s, dim=-1).detach().numpy() - ref["lse"]).max() < 1e-12 * max(1.0, ref["smax"].max())
    for key, t in zip(("dq", "dk", "dv"), qkv):
        assert np.abs(t.grad.numpy() - ref[key]).max() < 1e-11 * max(1.0, np.abs(ref["A_" + key]).max()), key


def test_onehot_and_uniform_preconditions():
    seen_hd = set()
    for c in CHK.CASES:
        if "onehot" not in c["modes"]:
            continue
        seen_hd.add(c["hd"])
        ins, _, ref = prepared(c, "onehot")
        CHK.onehot_precondition(ins, ref)
        S = c["S"]
        tg = ins["target"]
        assert ((tg >= 0) & (tg <= np.arange(S))).all()
        # operands exact in bf16, lse = the winning score to fp32 accuracy, o = v[t] in the reference itself
        for n in ("q", "k", "v", "do"):
            assert (CHK.bf16_round(ins[n]) == ins[n]).all(), (c["name"], n)
        win = ins["scale"] * np.einsum("bhsd,bhsd->bhs", ins["q"], ins["k"][:, :, tg])
        assert np.abs(ref["lse"] - win).max() < 2.0 ** -30
        assert np.abs(ref["o"] - ins["v"][:, :, tg]).max() < 2.0 ** -28
        ins, _, ref = prepared(c, "uniform")
        n = np.arange(1, S + 1, dtype=np.float64)
        assert np.abs(ref["lse"] - np.log(n)).max() < 1e-12
        assert np.abs(ref["o"] - np.cumsum(ins["v"], axis=2) / n[:, None]).max() < 1e-12
    assert seen_hd == {16, 32, 64, 128}


def test_hard_inputs_are_hard():
    c = _by_name("v2_fast64-bf16-hd64-B2H3S321-fused")
    ins, _, ref = prepared(c, "hard")
    tg = ins["target"]
    rows = np.nonzero(tg >= 0)[0]
    assert 0 < (tg < 0).sum() < len(tg) // 4                                  # a share of rows keeps gauss scores
    for n in ("q", "k"):
        assert (CHK.bf16_round(ins[n]) == ins[n]).all()
    s = ins["scale"] * ins["q"] @ np.swapaxes(ins["k"], -1, -2)
    at = s[:, :, rows, tg[rows]]
    assert at.min() > 50 and at.max() < 70                                    # about +60 at the target ...
    assert ref["P"][:, :, rows, tg[rows]].min() > 0.99                        # ... which holds the mass
    assert s.min() < -50                                                      # and about -60 at the complement
    # the maximum rises in the query's LAST 64-key tile, sits in the FIRST tile far above what follows, and on 31 / 32 / 63 / 64
    last, first = (tg[rows] // 64 == rows // 64) & (rows >= 128), (tg[rows] < 64) & (rows >= 128)
    assert last.sum() > 20 and first.sum() > 20
    assert {31, 32, 63, 64} <= set(tg[rows] % 128) | set(tg[rows])


def test_model_inside_bounds_in_every_mode():
    worst = {}
    fails = []
    for c in CHK.CASES:
        for mode in c["modes"]:
            ins, Z, ref = prepared(c, mode)
            f, w = CHK.judge(c, mode, ins, ref, CHK.model(c, ins, ref, Z))
            fails += f
            for k, v in w.items():
                key = (c["family"] + " " + c["dtype"], k)
                worst[key] = max(worst.get(key, 0.0), v)
    print("\nCPU model, worst |y - r| / bound per family and tensor:")
    for fam in sorted({f for f, _ in worst}):
        print("  %-20s" % fam + "  ".join("%s %.3f" % (k, worst[(fam, k)]) for k in ("o", "lse", "delta", "dv", "dq", "dk") if (fam, k) in worst))
    assert not fails, "\n".join(fails[:40])


MUT_CASES = ("v2_fast64-bf16-hd64-B2H3S321-fused", "v2_fast64-bf16-hd64-B2H3S129-fused", "bf16_generic-bf16-hd32-B2H3S257-fused",
             "bf16_generic-bf16-hd16-B2H3S129-fused", "fast128-bf16-hd128-B2H3S257-fused", "dropout-bf16-hd64-B2H3S257-fused-drop")


def test_every_mutation_is_caught_and_the_old_norm_misses_some():
    rows = []
    for mut in CHK.MUTATIONS:
        caught, old_ok = [], {}
        for name in MUT_CASES:
            c = _by_name(name)
            for mode in c["modes"]:
                ins, Z, ref = prepared(c, mode)
                got = CHK.model(c, ins, ref, Z, mut=mut)
                f, _ = CHK.judge(c, mode, ins, ref, got)
                if f:
                    caught.append(f"{c['family']}/S{c['S']}/{mode}")
                if mode == "gauss":
                    for key in CHK.old_norm_passes(c, ref, got):
                        old_ok[key] = old_ok.get(key, 0) + 1
        rows.append((mut, caught, old_ok))
    print(f"\nmutation: (case, mode) pairs of {len(MUT_CASES)} cases in which the row-wise check catches it | tensors that still pass the old "
          "max-norm criterion on the gauss inputs (in how many of the cases)")
    for mut, caught, old_ok in rows:
        print(f"  {mut:16s} {len(caught):2d}, e.g. {', '.join(caught[:3])} | " + (", ".join(f"{k} {n}" for k, n in old_ok.items()) or "none"))
    missed = [mut for mut, caught, _ in rows if not caught]
    assert not missed, missed
    # the gap was real: defects that the old criterion lets through entirely (all four tensors, every case)
    through = [mut for mut, _, old_ok in rows if all(old_ok.get(k) == len(MUT_CASES) for k in ("o", "dq", "dk", "dv"))]
    print("  pass the old criterion in every tensor of every case:", ", ".join(through))
    assert through
