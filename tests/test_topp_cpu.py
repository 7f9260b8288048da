"""CPU checks of nucleus (top-p) sampling: the rule of include/mas_hip.h "Top-p" as tests/helpers/topp_ref.py restates it -- hand-made
rows, ties, the order top-k then top-p, -inf entries, its equivalence with the sort / shift-by-one rule of ruDALL-E and HF, draw
frequencies --, the argument checks of ``mas_sample_tokens_topp`` and of ``MakeAScene.generate(top_p=...)``."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sample_ref as S  # noqa: E402
import topp_ref as P  # noqa: E402


def _tied_row(v=64):
    lg = np.full(v, -2.0, np.float32)
    lg[:5] = [3.0, 2.0, 2.0, 2.0, 1.0]
    return lg


def _q(lg):
    w = np.exp(np.asarray(lg, np.float64) - np.max(lg))
    return w / w.sum()


def test_ties_at_the_threshold_are_all_kept():
    lg = _tied_row()
    q = _q(lg)
    for top_p in (q[0] + 1e-3, q[0] + 1.5 * q[1], q[0] + 3 * q[1] - 1e-3):      # between q(3) and q(3) + q(2): all three 2s stay
        keep, margin = P.kept_p(lg, None, top_p)
        assert np.flatnonzero(keep).tolist() == [0, 1, 2, 3]
        assert margin == pytest.approx(min(top_p - q[0], q[0] + 3 * q[1] - top_p))
    assert np.flatnonzero(P.kept_p(lg, None, q[0] - 1e-3)[0]).tolist() == [0]
    assert np.flatnonzero(P.kept_p(lg, None, q[0] + 3 * q[1] + 1e-3)[0]).tolist() == [0, 1, 2, 3, 4]


def test_tiny_top_p_keeps_the_maximum_and_its_ties():
    lg = _tied_row()
    assert np.flatnonzero(P.kept_p(lg, None, 1e-6)[0]).tolist() == [0]
    lg[7] = 3.0
    assert np.flatnonzero(P.kept_p(lg, None, 1e-6)[0]).tolist() == [0, 7]
    assert np.flatnonzero(P.kept_p(lg, 1, 1e-6)[0]).tolist() == [0, 7]          # top-k keeps the tie, top-p cannot empty the set


def test_top_p_one_and_none_keep_what_top_k_keeps():
    rng = np.random.default_rng(1)
    lg = rng.standard_normal(100).astype(np.float32)
    for top_p in (None, 1.0, 1.5, float("nan")):
        keep, margin = P.kept_p(lg, None, top_p)
        assert keep.all() and margin == np.inf
        assert np.array_equal(P.kept_p(lg, 7, top_p)[0], S.kept(lg, 7))


def test_top_k_comes_first_and_top_p_sees_the_renormalised_masses():
    lg = np.log(np.array([0.4, 0.3, 0.2, 0.1])).astype(np.float32)
    # top_k = 2 re-normalises to {4/7, 3/7}: the mass above entry 1 is 0.571
    assert np.flatnonzero(P.kept_p(lg, 2, 0.6)[0]).tolist() == [0, 1]           # <= 0.6: both stay
    assert np.flatnonzero(P.kept_p(lg, 2, 0.5)[0]).tolist() == [0]              # > 0.5: entry 1 goes
    other_order = P.kept_p(lg, None, 0.5)[0] & S.kept(lg, 2)                    # top-p on the full row (0.4 <= 0.5 keeps 1), then top-k
    assert np.flatnonzero(other_order).tolist() == [0, 1]


def test_minus_infinity_entries_are_kept_only_when_they_tie_the_maximum():
    lg = np.array([1.0, -np.inf, 0.5, -np.inf, 0.0], np.float32)
    for top_p in (1e-6, 0.5, 0.9, 0.999999):
        keep = P.kept_p(lg, None, top_p)[0]
        assert keep[0] and not keep[1] and not keep[3]
    assert np.flatnonzero(P.kept_p(lg, None, 0.999999)[0]).tolist() == [0, 2, 4]
    allinf = np.full(5, -np.inf, np.float32)
    assert P.kept_p(allinf, None, 0.3)[0].all()                                 # every entry ties the maximum


def _sort_shift_rule(lg, top_p):
    """ruDALL-E / HF top_p filtering: sort descending, remove where the inclusive cumulative probability > top_p, shifted right by one"""
    order = np.argsort(-lg.astype(np.float64), kind="stable")
    cum = np.cumsum(_q(lg)[order])
    remove = cum > top_p
    remove[1:] = remove[:-1].copy()
    remove[0] = False
    keep = np.zeros(lg.shape, dtype=bool)
    keep[order[~remove]] = True
    return keep


def test_value_rule_equals_the_sort_and_shift_rule_on_tie_free_rows():
    rng = np.random.default_rng(2)
    checked = 0
    for trial in range(60):
        v = int(rng.integers(2, 400))
        lg = (rng.standard_normal(v) * rng.uniform(0.5, 4.0)).astype(np.float32)
        if len(np.unique(lg)) != v:
            continue
        for top_p in (0.05, 0.3, 0.5, 0.9, 0.99):
            keep, margin = P.kept_p(lg, None, top_p)
            if margin < 1e-9:
                continue
            assert np.array_equal(keep, _sort_shift_rule(lg, top_p)), (trial, top_p)
            checked += 1
    assert checked > 250


def test_midpoint_keeps_exactly_n():
    rng = np.random.default_rng(4)
    lg = (rng.standard_normal(500) * 2).astype(np.float32)
    for top_k in (None, 50):
        for n in (1, 2, 5, 40):
            keep, margin = P.kept_p(lg, top_k, P.midpoint_p(lg, top_k, n))
            assert keep.sum() == n and margin > 0
            assert np.array_equal(np.flatnonzero(keep), np.sort(np.argsort(-lg, kind="stable")[:n]))


def test_draw_frequencies_follow_the_restricted_softmax():
    """the rule, with the mapping's uniforms, is a draw from softmax(lg) restricted to the top-k-then-top-p set (20 000 rows)"""
    lg = np.array([1.0, 0.5, 0.0, -0.5, 2.0, 0.0, -3.0], np.float32)
    keep, margin = P.kept_p(lg, 6, 0.85)
    assert np.flatnonzero(keep).tolist() == [0, 1, 2, 4, 5] and margin > 1e-2    # 0.0 is the threshold value: both zeros stay
    toks, _ = P.select_rows_p(lg, None, None, 1.0, 6, 0.85, 11, 3, 20000, 0)
    assert not np.isin(toks, np.flatnonzero(~keep)).any()
    p = np.where(keep, np.exp(lg.astype(np.float64)), 0)
    p /= p.sum()
    freq = np.bincount(toks, minlength=7) / len(toks)
    assert np.abs(freq - p).max() < 0.015
    # off: the tokens of the top-p-free reference
    a, _ = P.select_rows_p(lg, None, None, 1.0, 5, None, 11, 3, 200, 0)
    b, _ = S.select_rows(lg, None, None, 1.0, 5, 11, 3, 200, 0)
    assert np.array_equal(a, b)


def test_topp_entry_validates_arguments_without_gpu():
    sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
    import mas_hip
    L = mas_hip.lib()
    assert L.mas_abi_version() == mas_hip.ABI_VERSION == 10
    assert "mas_sample_tokens_topp" in mas_hip.EXPORTS
    assert L.mas_sample_tokens_topp(None, 0, 0, 1, 8, 0, 1, 0, None, None, None, 1, None, 0, None, 1, None, 0, None) == -1
    assert b"null" in L.mas_last_error()


@pytest.mark.parametrize("top_p", [0, 0.0, -0.1, 1.5, math.nan])
@pytest.mark.parametrize("graph", [False, True])
def test_generate_rejects_a_top_p_outside_its_range(top_p, graph):
    import torch
    from models.transformer import MakeAScene
    m = MakeAScene(num_layers=1, hidden_dim=32, num_attn_heads=2, image_vocab_size=16, seg_vocab_size=5, text_vocab_size=20,
                   image_tokens_per_dim=2, seg_tokens_per_dim=1, text_length=4).eval()
    text, seg = torch.ones((1, 4), dtype=torch.long), torch.zeros((1, 1), dtype=torch.long)
    with pytest.raises(ValueError, match="top_p"):
        m.generate(text, seg, top_p=top_p, graph=graph)
