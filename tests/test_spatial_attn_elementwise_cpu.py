"""The element-wise check of the AttnBlock attention core (tests/helpers/spatial_attn_check.py) has teeth, shown without a GPU:

  * case names are unique and REQUIRED is what the cases reach;
  * its fp64 reference equals the torch formula of tests/test_gpu_spatial_attn.py (in float64, gradients by autograd);
  * the onehot and uniform preconditions hold for every case, and the hard inputs are hard;
  * removing any one key moves an element of o outside the uniform mode's check, at every uniform case;
  * a CPU model of each kernel set's arithmetic (fp32 softmax, P and dS cast to bf16 where the kernels cast, the chunk walk of the chunked
    kernels) stays inside the bounds and passes every exact check, in every mode of every case;
  * each mutation of that model (CHK.MUTATIONS) lands outside the bounds or breaks an exact check on each kernel set it applies to, and
    the printed table says which of them the old criterion (test_spatial_attention_fwd_bwd_vs_torch: relmax 2e-2 / 4e-2, rel-L2
    1e-2 / 2e-2, gauss operands of scale 1.5) lets through; a P truncated to bf16 instead of rounded is one of them.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import spatial_attn_check as CHK  # noqa: E402


@functools.lru_cache(maxsize=48)
def prepared(name, mode):
    """inputs and reference of a (case, mode): computed once, shared, never modified"""
    c = _by_name(name)
    ins = CHK.make_inputs(c, mode)
    return ins, CHK.reference(ins, c["kset"])


def _by_name(name):
    return next(c for c in CHK.CASES if c["name"] == name)


def test_case_names_are_unique_and_within_the_envelope():
    names = [c["name"] for c in CHK.CASES]
    assert len(set(names)) == len(names)
    assert {c["kset"] for c in CHK.CASES} == {"shipped", "flash"}
    assert max(c["S"] for c in CHK.CASES if c["kset"] == "shipped") == 256
    assert max(c["S"] for c in CHK.CASES) == 769 and max(c["N"] for c in CHK.CASES) == 8
    assert all(c["N"] >= 2 for c in CHK.CASES)                               # image mix-ups are possible everywhere


def test_required_is_reached_by_the_cases():
    got = CHK.reached([(c, k) for c in CHK.CASES for k in CHK.LAUNCH[c["kset"]]])
    for kern, feats in CHK.REQUIRED.items():
        assert feats <= got.get(kern, set()), (kern, sorted(feats - got.get(kern, set())))
    # the issue's own shape list
    ship = {(c["S"], c["C"]) for c in CHK.CASES if c["kset"] == "shipped"}
    assert {(S, 64) for S in (1, 16, 31, 32, 33, 35, 64, 81, 128, 129, 255, 256)} <= ship
    assert {(S, C) for C in (32, 96, 160, 384, 512) for S in (33, 129, 256)} <= ship
    fl = {(c["S"], c["C"]) for c in CHK.CASES if c["kset"] == "flash"}
    assert {(S, 64) for S in (1, 33, 256, 257, 288, 400, 512, 513, 600, 769)} <= fl and {(257, 512), (513, 512)} <= fl
    assert {c["C"] for c in CHK.CASES if c["kset"] == "flash"} >= {32, 64, 160, 512}
    assert not [sc for sc in fl if sc[1] == 512 and sc[0] not in (257, 513)]


@pytest.mark.parametrize("name", ["shipped-N2S81C64", "shipped-N2S129C160", "flash-N2S400C64"])
def test_reference_equals_the_torch_formula(name):
    c = _by_name(name)
    ins, ref = prepared(name, "gauss")
    C = c["C"]
    assert ins["scale"] == float(np.float32(C ** -0.5))
    t = torch.from_numpy(np.concatenate([ins["q"], ins["k"], ins["v"]], -1)).requires_grad_(True)
    q, k, v = t[..., :C], t[..., C:2 * C], t[..., 2 * C:]
    s = torch.bmm(q, k.transpose(1, 2)) * ins["scale"]         # (the helper's scale is C^-1/2 rounded to fp32, the operand the kernel gets)
    out = torch.bmm(torch.softmax(s, dim=2), v)
    out.backward(torch.from_numpy(ins["do"]))
    rel = lambda y, key: np.abs(y - ref[key]).max() / max(1.0, np.abs(ref["A_" + key]).max())
    assert rel(out.detach().numpy(), "o") < 1e-12
    assert np.abs(torch.logsumexp(s, dim=2).detach().numpy() - ref["lse"]).max() < 1e-12 * max(1.0, ref["smax"].max())
    g = t.grad.numpy()
    for i, key in enumerate(("dq", "dk", "dv")):
        assert rel(g[..., i * C:(i + 1) * C], key) < 1e-12, key
    assert np.abs((ins["do"] * ref["o"]).sum(-1) - ref["delta"]).max() < 1e-12 * max(1.0, ref["A_delta"].max())


def test_onehot_and_uniform_preconditions():
    for c in CHK.CASES:
        S = c["S"]
        ins, ref = prepared(c["name"], "onehot")
        CHK.onehot_precondition(ins, ref)
        tg = ins["target"]
        assert ((tg >= 0) & (tg < S)).all()
        for n in ("q", "k", "v", "do"):
            assert (CHK.bf16_round(ins[n]) == ins[n]).all(), (c["name"], n)
        assert (ref["argmax"] == tg[None]).all()
        assert np.abs(ref["lse"] - ref["s_target"]).max() < 2.0 ** -30
        assert np.abs(ref["o"] - ins["v"][:, tg]).max() < 2.0 ** -28
        if c["N"] > 1 and S > 4:
            assert not (ins["k"][0] == ins["k"][1]).all()                    # every image has its own key permutation
        ins, ref = prepared(c["name"], "uniform")
        assert np.abs(ref["lse"] - np.log(S)).max() < 1e-12
        assert np.abs(ref["o"] - ins["v"].mean(1, keepdims=True)).max() < 1e-12
        assert (ins["q"] == 0).all() and (ins["v"] == np.round(ins["v"])).all() and (np.abs(ins["v"]) >= 1).all()


def test_removing_any_one_key_fails_the_uniform_check():
    """for every uniform case and every key j: o without key j (its weight gone from the sum, renormalised or not) has an element outside
    the check the uniform mode applies (the tight one where there is one, else the general bound)"""
    for c in CHK.CASES:
        S = c["S"]
        if S == 1:
            continue
        ins, ref = prepared(c["name"], "uniform")
        v = ins["v"]
        tot = v.sum(1, keepdims=True)
        for o_mut in ((tot - v) / (S - 1), (tot - v) / S):                    # [N, key j removed, C]: every row of o would be this
            y = CHK.bf16_round(o_mut).astype(np.float64)
            r = np.broadcast_to(ref["o"][:, :1], y.shape)
            cc = dict(c, S=S)
            bad, _ = CHK.uniform_o_check(cc, dict(v=v), dict(o=r), y)
            if bad is None:
                bad = ~(np.abs(y - r) <= CHK.bound(dict(o=r, A_o=np.broadcast_to(ref["A_o"][:, :1], y.shape)), "o", c["kset"]))
            assert bad.any(-1).all(), (c["name"], int((~bad.any(-1)).sum()))


def test_hard_inputs_are_hard():
    for name in ("flash-N2S769C64", "shipped-N2S256C512", "flash-N2S600C32"):
        c = _by_name(name)
        S = c["S"]
        ins, ref = prepared(name, "hard")
        tg = ins["target"]
        rows = np.nonzero(tg >= 0)[0]
        assert 0 < (tg < 0).sum() < len(tg) // 4                              # a share of rows keeps gauss scores
        for n in ("q", "k"):
            assert (CHK.bf16_round(ins[n]) == ins[n]).all()
        assert ref["s_target"].min() > 55 and ref["s_target"].max() < 70      # about +60 at the target ...
        assert ref["p_target"].min() > 0.99                                   # ... which holds the mass
        assert (ref["argmax"][:, rows] == tg[rows][None]).all()
        assert ref["smin"] < -55                                              # and about -60 at the complement
        # the planted keys: both ends, the diagonal, the edges of the row's tile, the ragged tile, 255 / 256, the last chunk's ends
        want = {0, S - 1, ((S - 1) // 32) * 32, min(255, S - 1), min(256, S - 1), ((S - 1) // 256) * 256}
        assert want <= set(tg[rows])
        assert (tg[rows] == rows).any() and (tg[rows] == (rows // 32) * 32).any() and (tg[rows] == np.minimum((rows // 32) * 32 + 31, S - 1)).any()
        if S > 256:                                                           # maxima in every chunk, from the rows of every chunk that has 13
            nch = -(-S // 256)
            full = [a for a in range(nch) if min(S, 256 * (a + 1)) - 256 * a >= 13]
            assert {(a, b) for a, b in zip(rows // 256, tg[rows] // 256)} >= {(a, b) for a in full for b in range(nch)}


def test_model_inside_bounds_in_every_mode():
    worst, fails = {}, []
    for c in CHK.CASES:
        for mode in c["modes"]:
            ins, ref = prepared(c["name"], mode)
            f, w = CHK.judge(c, mode, ins, ref, CHK.model(c, ins, ref))
            fails += f
            for k, v in w.items():
                worst[(c["kset"], k)] = max(worst.get((c["kset"], k), 0.0), v)
    print("\nCPU model, worst |y - r| / bound per kernel set and tensor:")
    for ks in ("shipped", "flash"):
        print("  %-8s" % ks + "  ".join("%s %.3f" % (k, worst[(ks, k)]) for k in ("o", "lse", "delta", "dv", "dq", "dk")))
    assert not fails, "\n".join(fails[:40])


MUT_CASES = ("shipped-N2S129C160", "shipped-N2S256C64", "shipped-N2S256C512", "shipped-N2S81C64",
             "flash-N2S400C64", "flash-N2S600C64", "flash-N2S513C512", "flash-N2S288C160")


def test_every_mutation_is_caught_and_the_old_norm_misses_some():
    rows, missed = [], []
    for mut in CHK.MUTATIONS:
        caught, old_ok = {"shipped": [], "flash": []}, {"shipped": [], "flash": []}
        for name in MUT_CASES:
            c = _by_name(name)
            if c["kset"] == "shipped" and mut in CHK.FLASH_ONLY:
                continue
            for mode in c["modes"]:
                ins, ref = prepared(name, mode)
                got = CHK.model(c, ins, ref, mut=mut)
                f, _ = CHK.judge(c, mode, ins, ref, got)
                if f:
                    caught[c["kset"]].append(f"S{c['S']}C{c['C']}/{mode}/" + "+".join(sorted({x.split(", ")[1].split(":")[0].split(" ")[0] for x in f})))
                if mode == "gauss":
                    old_ok[c["kset"]].append(CHK.old_norm_passes(ref, got))
        rows.append((mut, caught, old_ok))
        missed += [(mut, ks) for ks in ("shipped", "flash") if not caught[ks] and not (ks == "shipped" and mut in CHK.FLASH_ONLY)]
    print("\nmutation | kernel set: (case, mode) pairs in which the element-wise check catches it, e.g. | cases that still pass the old norm criterion")
    for mut, caught, old_ok in rows:
        for ks in ("shipped", "flash"):
            if caught[ks] or old_ok[ks]:
                print(f"  {mut:20s} {ks:8s} {len(caught[ks]):2d}, e.g. {', '.join(caught[ks][:2])} | {sum(old_ok[ks])} of {len(old_ok[ks])}")
    assert not missed, missed
    # the gap was real: defects that the old criterion lets through on every case of both kernel sets
    through = [mut for mut, _, old_ok in rows if all(all(v) for v in old_ok.values() if v)]
    print("  pass the old criterion on every case:", ", ".join(through))
    assert "truncate_p" in through
