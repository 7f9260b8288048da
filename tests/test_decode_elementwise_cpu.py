"""The element-wise judgement of decode attention (tests/helpers/decode_elementwise_check.py) has teeth, shown without a GPU:

  * the case names are unique, every length category and every axis value is used on every route, and REQUIRED is what the cases reach
    when every case takes the kernel it names;
  * the onehot precondition holds on the reference alone for every case (asserted inside ``prepare``), and the planted operands are exact
    in bf16;
  * the float32 model of the three key walks stays under a QUARTER of the fp32 bound C_F32 TAU A_o + FLOOR in every mode of every case
    (bf16 cases: its value before the store), inside the whole bound after the store's rounding, and meets the exact modes bitwise;
  * each mutation of the model (D.MUTATIONS) lands outside a bound or breaks an exact check in at least one case.  The printed table says
    what the old criterion, max|y - ref| / max|ref| < 1e-2 on the bf16 gauss inputs of about 1000 keys, makes of each: the truncated store
    passes it (5.4e-3 and 2.5e-3; asserted).  A dropped key or a key counted twice does NOT pass it in these two cases (1.5e-2 .. 3.1e-2:
    the worst of 6 (slice, head) pairs x hd columns over max|ref| is several times the typical 4e-3), so that is printed, not asserted.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import attn_rowwise_check as CHK  # noqa: E402
import decode_elementwise_check as D  # noqa: E402


def test_cases_cover_every_axis_and_required_is_reached():
    names = [c["name"] for c in D.CASES]
    assert len(set(names)) == len(names)
    for route in D.ROUTES:
        cs = [c for c in D.CASES if c["route"] == route]
        assert {(c["dtype"], c["hd"]) for c in cs} == set(D.COMBOS)
        if route != "shared":
            assert set(D.L_CATEGORIES) <= {c["cat"] for c in cs}, route
    un, sp, sh = ([c for c in D.CASES if c["route"] == r] for r in D.ROUTES)
    assert {c["nq"] for c in un} == {1, 2, 5} and {c["layout"] for c in un} == {"plain", "strided"}
    assert {c["nsplit"] for c in sp} == {1, 2, 3, 8, 32}
    assert any(c["nsplit"] == 32 and c["S"] == 33 for c in sp)
    assert any(c["nsplit"] == 32 and all(e > b for b, e in D.walks(c)) for c in sp)
    assert any([e - b for b, e in D.walks(c) if e > b][-1] == 1 for c in sp)
    assert {c["group"] for c in sh} == {1, 3, 4, 5, 9} and {c["own"] for c in sh} >= {1, 32, 33}
    assert {c["plen"] for c in sh} >= {1, 31, 33} and {(c["nsp"], c["nso"]) for c in sh} == {(1, 1), (2, 3), (5, 1), (32, 32)}
    assert {c["hd"] for c in sh if c["nsp"] + c["nso"] == 64} == {16, 128}
    for c in sh:
        if c["cat"] == "pass+1":
            assert c["plen"] == D.geom("shared", c["dtype"], c["hd"])["keys_per_pass"] + 1
    got = D.reached([(c, {"host": D.HOST[c["route"]], **({"dev": D.DEV[c["route"]]} if D.has_dev(c) else {})}) for c in D.CASES])
    for kern, feats in D.REQUIRED.items():
        assert feats <= got.get(kern, set()), (kern, sorted(feats - got.get(kern, set())))


def test_model_meets_a_quarter_of_the_bound_and_the_exact_modes():
    worst, fails = {}, []
    cold = 0
    for c in D.CASES:
        for mode in c["modes"]:
            ins, ref = D.prepare(c, mode)                   # asserts the onehot precondition on the reference alone
            if c["dtype"] == "bf16":
                for n in ("q", "k", "v"):
                    assert (CHK.bf16_round(ins[n]) == ins[n]).all(), (c["name"], mode, n)
            cold += int((ins["dtarget"] == D.COLD).any())
            f, w = D.judge(c, mode, ins, ref, D.model(c, ins))
            fails += f
            y32 = D.model(c, ins, cast=False).astype(np.float64)
            w4 = float((np.abs(y32 - ref["o"]) / D.bound(c, ref, f32_part=True)).max())
            key = (c["route"], c["dtype"], mode)
            worst[key] = max(worst.get(key, (0.0, 0.0)), (w4, w))
            if not w4 < 0.25:
                fails.append(f"{c['name']} {mode}: the float32 model reaches {w4:.3f} of the fp32 bound (limit 0.25)")
    print("\nfloat32 model, worst |y - r| / bound: before the store vs the fp32 bound | after the store vs the whole bound")
    for key in sorted(worst):
        print("  %-8s %-5s %-8s %.3f | %.3f" % (key + worst[key]))
    assert cold > 0
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


MUT_CASES = ("dec_split-bf16-hd128-B2H3L993-n32", "dec_shared-bf16-hd16-g2x1H3-p31o993-n32_32", "dec_split-bf16-hd16-B2H3L33-n32",
             "dec_unsplit-bf16-hd64-B2H3L257nq5", "dec_shared-bf16-hd128-g2x5H3-p33o33-n32_32", "dec_shared-bf16-hd64-g2x9H3-p33o32-n2_3",
             "dec_split-f32-hd64-B2H3L33-n32", "dec_shared-f32-hd32-g2x5H3-p1o33-n2_3")
OLD_PASSES = ("truncate_out",)
OLD_CASES = MUT_CASES[:2]                                   # bf16, about 1000 keys: where a key weighs 4e-3 of max|ref|


def test_every_mutation_is_caught_and_the_old_criterion_misses_the_truncated_store():
    cases = [next(c for c in D.CASES if c["name"].startswith(n)) for n in MUT_CASES]
    prepared = {(c["name"], mode): D.prepare(c, mode) for c in cases for mode in c["modes"]}
    rows = []
    for mut in D.MUTATIONS:
        caught, old = [], {}
        for c in cases:
            if not D.applies(c, mut):
                continue
            for mode in c["modes"]:
                ins, ref = prepared[(c["name"], mode)]
                y = D.model(c, ins, mut=mut)
                if D.judge(c, mode, ins, ref, y)[0]:
                    caught.append(f"{c['name']}/{mode}")
                if mode == "gauss" and c["name"].startswith(OLD_CASES):
                    old[c["name"]] = D.old_criterion_passes(c, ref, y)
        rows.append((mut, caught, old))
    print("\nmutation: (case, mode) pairs that catch it | old criterion on the bf16 gauss inputs of ~1000 keys (passes, rel-max)")
    for mut, caught, old in rows:
        print(f"  {mut:24s} {len(caught):2d}, e.g. {', '.join(caught[:2])} | " + ", ".join(f"{ok} {e:.1e}" for ok, e in old.values()))
    assert not [mut for mut, caught, _ in rows if not caught]
    for mut, _, old in rows:
        if mut in OLD_PASSES:
            assert old and all(ok for ok, _ in old.values()), (mut, old)
