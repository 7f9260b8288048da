"""The CPU side of tests/test_gpu_vq_elementwise.py, checked without a GPU (tests/helpers/vq_elementwise_check.py):

  * the fp64 references equal ``oracle.vq_oracle.codebook_forward`` and its autograd in float64 on the same operands to 1e-12, and the
    fp32 oracle takes the same index wherever its own top-2 gap exceeds the bound;
  * the launch geometry the helper restates agrees with the literals in csrc/vq_core.h, csrc/vq.hip and mas_common.h's ``acc_row`` and
    gives the table the forward cases were chosen for (empty trailing splits, the split count capped by 1024 / row blocks, two tiles
    per split with a ragged last tile);
  * input conditions, from the reference alone: no *gauss* row and at most 10 % of a *far* case's rows are left to the slack rule, every
    tie relation the geometry of an *int* case has room for is planted in at least 4 latent rows, and a planted row's distance 0 is
    shared by exactly the duplicates;
  * an fp32 model of every kernel -- the same trees in numpy float32, the split / tile / half-wave merge order written out -- stays
    inside EVERY bound and meets every int-mode equality for every case in both settings;
  * teeth: each of sixteen planted errors drives the same judge to fail, on the easy operands and on the far / planted ones separately
    where the error can live in both (an error in the tie order lives in the planted ties alone, bf16 operands are exact on the small
    integers, a padded code never wins against rows shifted by +8)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import vq_elementwise_check as CHK  # noqa: E402
from oracle import vq_oracle  # noqa: E402

CSRC = os.path.join(ROOT, "make-a-scene_amd", "csrc")


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.abs(a - b).max())
    assert err <= 1e-12 * max(1.0, float(np.abs(b).max())), (what, err)


def _as_map(rows):
    return rows.view(1, 1, rows.shape[0], rows.shape[1]).permute(0, 3, 1, 2)


@pytest.mark.parametrize("name,mode", [("f_161x100x64", "gauss"), ("f_161x100x64", "far"), ("f_97x161x128", "far"), ("f_129x257x256", "gauss"),
                                       ("f_130x2080x32", "int"), ("f_3x8x32", "gauss")])
def test_forward_reference_is_the_oracle_in_float64(name, mode):
    c = CHK.CASES[name]
    ref = CHK.reference_fwd(c, mode)
    ins, first = ref["ins"], ref["first"]
    z, cb = torch.from_numpy(ins["z"]), torch.from_numpy(ins["cb"])
    zq, loss, idx = vq_oracle.codebook_forward(cb.double(), _as_map(z.double()), CHK.BETA)
    _close(ref["d64"], vq_oracle.vq_distances(z.double(), cb.double()).numpy(), "distances")
    assert np.array_equal(idx.numpy(), first)
    _close(CHK.loss_reference(c, ins, first, mode)[0], float(loss), "loss")
    assert float(ref["bound"].min()) > 0
    # the fp32 oracle: the same index wherever its own gap is wide
    d32 = vq_oracle.vq_distances(z, cb).double().numpy()
    idx32 = d32.argmin(1)
    if c["K"] > 1:
        rows = np.arange(c["M"])
        low2 = np.sort(d32, 1)[:, :2]
        wide32 = low2[:, 1] - low2[:, 0] > ref["bound"][rows, first] + ref["bound"][rows, ref["second"]]
        assert wide32.any() and np.array_equal(idx32[wide32], first[wide32])


@pytest.mark.parametrize("name", ["b_rand_147_d128", "b_edges_403_d256", "b_small_3_d64", "b_ragged_k41_d32"])
def test_backward_reference_is_the_oracle_autograd_in_float64(name):
    c = CHK.CASES[name]
    ins = CHK.make_inputs(c, "gauss")
    z = torch.from_numpy(ins["z"]).double().requires_grad_(True)
    cb = torch.from_numpy(ins["cb"]).double().requires_grad_(True)
    zq, loss, idx = vq_oracle.codebook_forward(cb, _as_map(z), CHK.BETA)
    assert np.array_equal(idx.numpy(), ins["pick"])
    g_zq = _as_map(torch.from_numpy(ins["g_zq"]).double())
    torch.autograd.backward([zq, loss], [g_zq, torch.tensor(ins["g_loss"], dtype=torch.float64)])
    for setting in ("default", "atomic"):
        ref = CHK.bwd_reference(c, ins, ins["pick"], setting)
        _close(ref["dz"], z.grad.numpy(), "dz")
        _close(ref["dcb"], cb.grad.numpy(), "dcb")
        picked = np.zeros(c["K"], bool)
        picked[ins["pick"]] = True
        assert float(ref["bdz"].min()) > 0 and float(ref["bdcb"][picked].min()) > 0 and float(np.abs(ref["bdcb"][~picked]).max(initial=0)) == 0


def test_restated_geometry():
    core, vq, common = (open(os.path.join(CSRC, f)).read() for f in ("vq_core.h", "vq.hip", "mas_common.h"))
    literal = lambda src, name: int(re.search(r"\b%s = (\d+)\b" % name, src).group(1))
    assert [literal(core, n) for n in ("NT", "ROWS_PER_BLOCK", "CODES_PER_TILE", "MAX_KSPLIT")] == \
        [CHK.NT, CHK.ROWS_PER_BLOCK, CHK.CODES_PER_TILE, CHK.MAX_KSPLIT] == [256, 128, 32, 64]
    assert literal(vq, "VB_CODES") == CHK.VB_CODES == 8
    for src, pattern in ((core, r"int ks = mas_cdiv\(1024, rb\);"), (core, r"tiles_per = \(ntiles \+ ksplit - 1\) / ksplit"),
                         (core, r"float best = INFINITY; int besti = 0x7fffffff;"), (core, r"if \(d < best\)"),
                         (core, r"v < bv \|\| \(v == bv && i < bi\)"), (core, r"__shfl_xor\(best, 32\)"),
                         (common, r"acc_row\(int lane, int r\) \{ return \(r & 3\) \+ 8 \* \(r >> 2\) \+ 4 \* \(lane >> 5\); \}"),
                         (vq, r"per = \(M \+ NT / 64 - 1\) / \(NT / 64\)"), (vq, r"for \(int base = lo; base < hi; base \+= 64\)"),
                         (vq, r"if \(bi == 0x7fffffff\) bi = 0;"), (vq, r'mas_env_int\("MAS_VQ_BWD_DET", 1\)')):
        assert re.search(pattern, src), pattern
    assert sorted(CHK.ACC_ROW.reshape(-1).tolist()) == list(range(32)) and (np.diff(CHK.ACC_ROW, axis=1) > 0).all()
    # the forward cases: (ntiles, ksplit, tiles_per, active, empty, codes in the last tile)
    table = {(130, 2080, 32): (65, 64, 2, 33, 31, 32), (33, 2049, 256): (65, 64, 2, 33, 31, 1), (2049, 1985, 32): (63, 61, 2, 32, 29, 1),
             (161, 100, 64): (4, 4, 1, 4, 0, 4), (97, 161, 128): (6, 6, 1, 6, 0, 1), (129, 257, 256): (9, 9, 1, 9, 0, 1)}
    for c in CHK.FWD_CASES:
        g = CHK.geometry(c["M"], c["K"])
        if (c["M"], c["K"], c["D"]) in table:
            assert (g["ntiles"], g["ksplit"], g["tiles_per"], g["active"], g["empty"], g["last_codes"]) == table[(c["M"], c["K"], c["D"])], c["name"]
        assert (g["active"] - 1) * g["tiles_per"] < g["ntiles"] <= g["active"] * g["tiles_per"] and g["ksplit"] <= 64
    assert [CHK.pick_ksplit(m, k) for m, k in ((1, 1), (1, 33), (3, 8))] == [1, 2, 1]
    assert [c["name"] for c in CHK.FWD_CASES if CHK.geometry(c["M"], c["K"])["capped"]] == ["f_2049x1985x32"]
    g = CHK.geometry(2049, 1985)
    assert (g["rb"], CHK.cdiv(1024, g["rb"])) == (17, 61)
    assert CHK.geometry(130, 2080)["rb"] == 2 and 130 - CHK.ROWS_PER_BLOCK == 2           # the second row block has 2 rows
    assert {c["D"] for c in CHK.FWD_CASES} == {c["D"] for c in CHK.BWD_CASES} == {32, 64, 128, 256}
    # the backward cases
    assert CHK.quarters(403) == [(0, 101), (101, 202), (202, 303), (303, 403)] and CHK.quarters(3) == [(0, 1), (1, 2), (2, 3), (3, 3)]
    assert CHK.quarters(1) == [(0, 1), (1, 1), (1, 1), (1, 1)]
    assert CHK.edge_rows(403) == [0, 63, 64, 100, 101, 164, 165, 201, 202, 265, 266, 302, 303, 366, 367, 402]
    assert CHK.edge_rows(256) == [0, 63, 64, 127, 128, 191, 192, 255] and len(CHK.edge_rows(512)) == 16
    for c in CHK.BWD_CASES:
        pick = CHK.make_inputs(c, "gauss")["pick"]
        k, last = c["K"], (c["K"] - 1) // CHK.VB_CODES * CHK.VB_CODES
        assert k % CHK.VB_CODES in (1, 5), c["name"]                     # every backward case has a ragged last group
        if c["pattern"] == "one":
            assert len(set(pick.tolist())) == 1 and c["D"] in (128, 256)
        if c["pattern"] == "edges":
            grp = pick // CHK.VB_CODES == CHK.EDGE_GROUP
            assert sorted(np.nonzero(grp)[0].tolist()) == CHK.edge_rows(c["M"])
        if c["pattern"] == "ragged":
            assert pick[0] == k - 1 and pick[1] == last and pick[-1] == k - 1
        if c["pattern"] == "small":
            assert c["M"] in (1, 3) and pick[0] == k - 1
        if c["pattern"] == "rand16":
            assert c["M"] >= 147 and len(set(pick.tolist())) <= 16
        if c["direct"]:
            assert any(x not in set(pick.tolist()) for x in range(last, k))
    assert {(c["pattern"], c["D"]) for c in CHK.BWD_CASES} >= {("one", 128), ("one", 256), ("edges", 128), ("edges", 256)}


@pytest.mark.parametrize("c", CHK.FWD_CASES, ids=lambda c: c["name"])
def test_input_conditions(c):
    m = c["M"]
    assert CHK.near_tie_rows(c, "gauss") == 0
    near = CHK.near_tie_rows(c, "far")
    print(f"{c['name']}: {near} of {m} far rows are judged by the slack rule alone")
    assert near <= CHK.NEAR_TIE_CAP * m
    ref = CHK.reference_fwd(c, "int")
    ins, d64 = ref["ins"], ref["d64"]
    assert np.array_equal(d64, np.round(d64)) and float(np.abs(d64).max()) <= 64 * c["D"]
    count = {}
    for row, rel, codes in ins["ties"]:
        assert np.array_equal(np.nonzero(d64[row] == 0)[0], np.array(codes)) and d64[row].min() == 0, (c["name"], row, rel)
        assert rel in CHK.classify_ties(list(codes), c)
        for r in CHK.classify_ties(list(codes), c):
            count[r] = count.get(r, 0) + 1
    print(f"{c['name']}: planted tie rows per relation {count}")
    if m >= 33:
        room = CHK.relations_with_room(c)
        assert all(count.get(r, 0) >= 4 for r in room), (c["name"], room, count)
        assert set(room) >= set(CHK.TIE_RELATIONS) - {"next_tile", "first_last_split"}
        assert len(ins["zero_rows"]) == 2
    natural = float(np.mean((d64 == d64.min(1, keepdims=True)).sum(1) > 1))
    print(f"{c['name']}: share of rows with a tied minimum {natural:.3f}")


def test_every_tie_relation_is_planted_somewhere():
    have = set()
    for c in CHK.FWD_CASES:
        if c["M"] >= 33:
            have |= set(CHK.relations_with_room(c))
    assert have == set(CHK.TIE_RELATIONS)


_clean = {}          # the unplanted model's verdicts, judged once


def _judge_model(c, mode, plant=None, setting="default"):
    key = (c["name"], mode, setting)
    if plant is None and key in _clean:
        return _clean[key]
    out = CHK.judge(c, mode, CHK.model_record(c, mode, plant, setting), setting)
    if plant is None:
        _clean[key] = out
    return out


@pytest.mark.parametrize("label,c", [(s, c) for s, _, cases in CHK.SETTINGS for c in cases], ids=lambda v: v if isinstance(v, str) else v["name"])
def test_fp32_model_stays_inside_every_bound(label, c):
    for mode in CHK.modes_of(c):
        rows, reached, failures, notes = _judge_model(c, mode, None, label)
        for key, fam, fig, verdict in rows:
            print(f"{label:8s} {c['name']:20s} {mode:5s} {key:40s} {fam:24s} {fig:>8s} {verdict}")
        assert not failures, "\n".join(failures)
        assert rows and reached
        assert all(float(fig) < 1 for _, _, fig, verdict in rows if verdict != "equal")


def test_model_reaches_everything_the_gpu_test_requires():
    import test_gpu_vq_elementwise as GPU
    reached = {s: set() for s, _, _ in CHK.SETTINGS}
    for label, _, cases in CHK.SETTINGS:
        for c in cases:
            for mode in CHK.modes_of(c):
                reached[label] |= _judge_model(c, mode, None, label)[1]
    for part, (label, want) in GPU.REQUIRED.items():
        missing = sorted((k, f) for k, fs in want.items() for f in fs if (k, f) not in reached[label])
        assert not missing, (part, missing)


FWD_TEETH_CASES = ["f_130x2080x32", "f_161x100x64", "f_97x161x128"]
BWD_TEETH_CASES = ["b_one_256_d128", "b_one_403_d256", "b_edges_512_d32", "b_rand_256_d32", "b_direct_147_d256"]
# planted error -> (cases, the operand modes in which it has to be caught)
TEETH = {
    "lane_le": (FWD_TEETH_CASES, ["int"]),                 # a lane's own d <= best
    "take_min_high": (FWD_TEETH_CASES, ["int"]),
    "halfwave_le": (FWD_TEETH_CASES, ["int"]),
    "finalize_last": (FWD_TEETH_CASES, ["int"]),
    "empty_zero": (["f_130x2080x32", "f_33x2049x256"], ["gauss", "far", "int"]),
    "padded_code": (["f_161x100x64", "f_97x161x128"], ["gauss", "int"]),
    "last_tile_dropped": (FWD_TEETH_CASES, ["gauss", "far", "int"]),
    "bf16_dot": (FWD_TEETH_CASES, ["gauss", "far"]),
    "ee_shifted": (FWD_TEETH_CASES, ["gauss", "far", "int"]),
    "zq_next": (FWD_TEETH_CASES, ["gauss", "far", "int"]),
    "loss_last_block": (FWD_TEETH_CASES, ["gauss", "far", "int"]),
    "dz_no_gzq": (BWD_TEETH_CASES, ["gauss", "int"]),
    "fourth_quarter": (BWD_TEETH_CASES, ["gauss", "int"]),
    "hit_lo64": (BWD_TEETH_CASES, ["gauss", "int"]),
    "beta_squared": (BWD_TEETH_CASES, ["gauss", "int"]),
    "unstored_row": (["b_direct_147_d256"], ["gauss"]),
}


@pytest.mark.parametrize("kind", list(TEETH))
def test_teeth_planted_error_is_caught(kind):
    names, need = TEETH[kind]
    settings = ["default"] if names[0].startswith("f_") or kind in ("dz_no_gzq", "unstored_row") else ["default", "atomic"]
    for setting in settings:
        caught = {}
        for name in names:
            c = CHK.CASES[name]
            for mode in CHK.modes_of(c):
                _, _, failures, _ = _judge_model(c, mode, kind, setting)
                caught.setdefault(mode, []).extend(failures)
                print(f"teeth {kind:18s} {setting:8s} {name:18s} {mode:5s}: {len(failures)} checks fail" + (f" ({failures[0]})" if failures else ""))
        for mode in need:
            assert caught.get(mode), (kind, setting, mode, "the planted error passes")


def test_teeth_tie_errors_are_caught_by_the_planted_rows():
    """each tie-order error flips exactly rows whose minimum is shared; the three differ in which relations they flip"""
    c = CHK.CASES["f_130x2080x32"]
    ins = CHK.make_inputs(c, "int")
    flipped = {}
    for kind in ("take_min_high", "halfwave_le", "finalize_last"):
        idx = CHK.model_record(c, "int", kind)["idx"].numpy()
        flipped[kind] = {rel for row, rel, codes in ins["ties"] if idx[row] != codes[0]}
        assert all(idx[row] in codes for row, rel, codes in ins["ties"])
    assert flipped["take_min_high"] >= {"other_half_wave", "adjacent_splits", "first_last_split", "code0_last_code", "triple_three_splits"}
    assert "other_half_wave" in flipped["halfwave_le"] and "other_half_wave" not in flipped["finalize_last"]
    assert flipped["finalize_last"] >= {"adjacent_splits", "first_last_split", "code0_last_code", "triple_three_splits"}
    assert not any("adjacent_registers" in f for f in flipped.values())       # one lane's strict <: none of the three touches it ...
    idx = CHK.model_record(c, "int", "lane_le")["idx"].numpy()                 # ... a lane's own <= does, and the next tile of its split
    assert {rel for row, rel, codes in ins["ties"] if idx[row] != codes[0]} == {"adjacent_registers", "next_tile"}


def test_nonfinite_rows_in_the_model():
    c = CHK.NONFINITE
    rec = CHK.model_record(c, "gauss")
    ins = CHK.make_inputs(c, "gauss")
    idx = rec["idx"].numpy()
    assert len(ins["bad_rows"]) == 6 and (idx[ins["bad_rows"]] == 0).all() and not np.isfinite(float(rec["loss"]))
    assert np.isnan(ins["z"][list(CHK.NF_ALL_NAN)]).all() and np.isnan(ins["z"][CHK.NF_ONE_NAN]).sum() == 1
    assert np.isposinf(ins["z"][CHK.NF_PINF]).sum() == 1 and np.isneginf(ins["z"][CHK.NF_NINF]).sum() == 1
