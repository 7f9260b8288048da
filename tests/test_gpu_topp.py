"""Nucleus (top-p) sampling on the MI355X: ``mas_sample_tokens_topp`` (make-a-scene_amd/csrc/decode_step.hip) against the float64 rule of
tests/helpers/topp_ref.py -- kept set, draw statistics, the Gumbel-max reference, ties at the threshold, -inf entries, "off is off",
repeatability -- and ``MakeAScene.generate(top_p=p)`` on the eager and the graph path.

Every kernel case fixes ``top_p`` at the float32 midpoint between two neighbouring cumulative masses of the reference and first asserts,
on the CPU, that the reference's p-margin (the distance of top_p from the nearest cumulative mass) is >= 2e-4: ten times what a naive
sequential fp32 summation of 8192 masses loses (2.1e-5), so any reasonable implementation lands on the reference's side of the line."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sample_ref as S  # noqa: E402
import topp_ref as P  # noqa: E402

MARGIN = 2e-4
SEED = (12345, 678)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _sample(logits_pair, rows, temperature=1.0, cond_scale=None, top_k=0, top_p=None, seed=SEED, entry_topp=None):
    """tokens of ``rows`` output rows sharing one logits row (pair); ``top_p`` None and ``entry_topp`` unset: ``mas_sample_tokens``"""
    from mas_hip import decode
    dev = logits_pair.device
    tokens = torch.zeros((rows, 1), dtype=torch.long, device=dev)
    use_p = (top_p is not None) if entry_topp is None else entry_topp
    vals = [temperature, cond_scale or 0.0] + ([top_p] if use_p else [])
    params = torch.tensor(vals, dtype=torch.float32, device=dev)
    sd = torch.tensor(list(seed), dtype=torch.int64, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    decode.sample_tokens(logits_pair, tokens, step, params, decode.SAMPLE, top_k=top_k, guided=cond_scale is not None, seed=sd, rows=rows,
                         top_p=use_p)
    return tokens[:, 0].cpu().numpy()


def _rows(v, scale, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(v) * scale).astype(np.float32), (rng.standard_normal(v) * 0.5).astype(np.float32)


# (V, scale, n_kept, temperature, cond_scale, top_k, row seed): fixed seeds at which the reference margin clears MARGIN
CASES = [
    (64, 2.0, 1, 0.8, None, 0, 0), (64, 2.0, 2, 1.0, 2.0, 10, 0), (64, 2.0, 5, 1.0, None, 10, 0), (64, 2.0, 40, 1.0, None, 0, 0),
    (1001, 3.0, 1, 1.0, 3.0, 0, 0), (1001, 3.0, 2, 0.7, None, 0, 0), (1001, 3.0, 5, 1.0, None, 0, 0), (1001, 3.0, 40, 0.9, None, 0, 0),
    (8192, 3.0, 1, 1.0, None, 200, 2), (8192, 3.0, 2, 1.0, 2.5, 200, 2), (8192, 3.0, 5, 0.7, None, 0, 2), (8192, 3.0, 40, 1.0, None, 200, 2),
    (8192, 1.0, 300, 1.0, None, 0, 9),
]


def _reference(v, scale, n, temp, cs, top_k, seed):
    """(lc, lu or None, lg, top_p, keep, margin) of a case, all from the float64 reference"""
    lc, lu = _rows(v, scale, seed)
    lu = lu if cs is not None else None
    lg = (S.mix(lc, lu, cs) / np.float32(temp)).astype(np.float32)
    top_p = P.midpoint_p(lg, top_k, n)
    keep, margin = P.kept_p(lg, top_k, top_p)
    return lc, lu, lg, top_p, keep, margin


@pytest.mark.parametrize("v,scale,n,temp,cs,top_k,seed", CASES)
def test_kept_set_and_statistics(v, scale, n, temp, cs, top_k, seed):
    from scipy import stats
    lc, lu, lg, top_p, keep, margin = _reference(v, scale, n, temp, cs, top_k, seed)
    assert len(np.unique(lg)) == v and keep.sum() == n and 0 < top_p < 1
    assert margin >= MARGIN, margin                                      # before anything touches the GPU
    dev = _dev()
    pair = torch.from_numpy(np.stack([lc, lu]) if cs is not None else lc[None]).to(dev)
    rows = 100_000
    toks = _sample(pair, rows, temp, cs, top_k, top_p)
    counts = np.bincount(toks, minlength=v)
    assert counts[~keep].sum() == 0, f"a token outside the kept set was drawn: {np.flatnonzero(counts * ~keep)[:8]}"
    if n == 1:
        assert counts[keep][0] == rows                                   # one category: chi-square has no degree of freedom left
    else:
        p = np.exp(lg[keep].astype(np.float64) - lg[keep].max())
        p /= p.sum()
        pval = stats.chisquare(counts[keep], p * rows).pvalue
        assert pval > 1e-3, pval
    m = 2000 if v == 64 else 300
    want, gap = P.select_rows_p(lc, lu, cs, temp, top_k, top_p, SEED[0], SEED[1], m, 0)
    sure = gap > 1e-4
    assert sure.mean() > 0.9 and (toks[:m][sure] == want[sure]).all()


def test_ties_at_the_threshold_are_kept():
    dev = _dev()
    lg = np.full(64, -2.0, np.float32)
    lg[:5] = [3.0, 2.0, 2.0, 2.0, 1.0]
    w = np.exp(lg.astype(np.float64))
    q = w / w.sum()
    top_p = float(np.float32(q[0] + 1.5 * q[1]))                        # inside the three tied entries: all of them stay, 1.0 goes
    keep, margin = P.kept_p(lg, None, top_p)
    assert np.flatnonzero(keep).tolist() == [0, 1, 2, 3] and margin >= MARGIN
    toks = _sample(torch.from_numpy(lg[None]).to(dev), 60_000, top_p=top_p)
    assert set(np.unique(toks).tolist()) == {0, 1, 2, 3}


def test_minus_infinity_entries_are_never_drawn():
    dev = _dev()
    lc, _ = _rows(8192, 3.0, 21)
    dead = np.random.default_rng(22).random(8192) < 0.3
    dead[np.argsort(-lc)[:3]] = [False, True, False]                      # one of them where the second largest value was
    lc[dead] = -np.inf
    for top_k, top_p in ((0, 0.9), (200, 0.5), (0, 0.999999)):
        toks = _sample(torch.from_numpy(lc[None]).to(dev), 100_000, 1.0, None, top_k, top_p)
        assert not dead[toks].any(), (top_k, top_p)
        keep, margin = P.kept_p(lc, top_k, top_p)
        if margin >= MARGIN:
            assert keep[toks].all(), (top_k, top_p)


@pytest.mark.parametrize("v", [64, 8192])
@pytest.mark.parametrize("top_k", [0, 20])
def test_off_is_off(v, top_k):
    """the new entry with top_p absent from the decision -- 1.0, beyond 1, NaN -- draws the tokens of ``mas_sample_tokens``"""
    dev = _dev()
    lc, lu = _rows(v, 2.0, 31 + v)
    rows = 100_000
    for cs, temp in ((None, 0.9), (2.0, 1.0)):
        pair = torch.from_numpy(np.stack([lc, lu]) if cs is not None else lc[None]).to(dev)
        base = _sample(pair, rows, temp, cs, top_k)
        for top_p in (1.0, 1.5, float("nan")):
            got = _sample(pair, rows, temp, cs, top_k, top_p, entry_topp=True)
            assert np.array_equal(got, base), (cs, top_p)
        assert not np.array_equal(_sample(pair, rows, temp, cs, top_k, 0.5), base)


def test_repeatable():
    dev = _dev()
    v, scale, n, temp, cs, top_k, seed = CASES[11]
    assert (v, n) == (8192, 40)
    lc, lu, lg, top_p, keep, margin = _reference(v, scale, n, temp, cs, top_k, seed)
    pair = torch.from_numpy(lc[None]).to(dev)
    a = _sample(pair, 100_000, temp, cs, top_k, top_p)
    b = _sample(pair, 100_000, temp, cs, top_k, top_p)
    c = _sample(pair, 100_000, temp, cs, top_k, top_p, seed=(12345, 679))
    assert np.array_equal(a, b) and not np.array_equal(a, c)


# ------------------------------------------------------------------------------------------------------------------------------- model
def _small_model(dev, seed=0, hidden=64, heads=4, vocab=64):
    from models.transformer import MakeAScene
    torch.manual_seed(seed)
    m = MakeAScene(num_layers=2, hidden_dim=hidden, num_attn_heads=heads, image_vocab_size=vocab, seg_vocab_size=11, text_vocab_size=48,
                   image_tokens_per_dim=4, seg_tokens_per_dim=2, text_length=8).to(dev).eval()
    g = torch.Generator().manual_seed(seed + 1)
    text = torch.randint(1, 40, (3, 8), generator=g).to(dev)
    text[:, 6:] = 0
    seg = torch.randint(0, 11, (3, 4), generator=g).to(dev)
    return m, text, seg


@pytest.mark.parametrize("cs", [None, 3.0], ids=["plain", "guided"])
def test_tiny_top_p_is_greedy(cs):
    dev = _dev()
    m, text, seg = _small_model(dev)
    with torch.no_grad():
        for graph in (True, False):
            greedy = m.generate(text, seg, temperature=0, cond_scale=cs, graph=graph)
            got = m.generate(text, seg, top_p=1e-6, cond_scale=cs, graph=graph)
            assert torch.equal(got, greedy), graph


def _membership(tokens, logits, top_k, top_p, temperature=1.0):
    """every token inside ``kept_p`` of its logits row, over the rows whose p-margin clears MARGIN -> (rows checked / rows, masks)"""
    toks, lgs = tokens.cpu().numpy().reshape(-1), logits.cpu().numpy().reshape(-1, logits.shape[-1])
    clear = np.zeros(len(toks), dtype=bool)
    for i, (t, row) in enumerate(zip(toks, lgs)):
        lg = (row / np.float32(temperature)).astype(np.float32)
        keep, margin = P.kept_p(lg, top_k, top_p)
        clear[i] = margin >= MARGIN
        assert keep[t] or not clear[i], (i, int(t), margin)
    return clear


def test_generate_draws_inside_the_nucleus():
    dev = _dev()
    m, text, seg = _small_model(dev)
    kw = dict(top_p=0.5, top_k=20, return_logits=True)
    with torch.no_grad():
        tg, lg = m.generate(text, seg, graph=True, generator=torch.Generator(device=dev).manual_seed(3), **kw)
        t2, l2 = m.generate(text, seg, graph=True, generator=torch.Generator(device=dev).manual_seed(3), **kw)
        te, le = m.generate(text, seg, graph=False, generator=torch.Generator(device=dev).manual_seed(3), **kw)
    assert torch.equal(tg, t2) and torch.equal(lg, l2)                   # the same seed: the same tokens
    clear = _membership(tg, lg, 20, 0.5)
    assert clear.mean() >= 0.8, clear.mean()
    assert _membership(te, le, 20, 0.5).mean() >= 0.8
    # the Gumbel-max reference: generate draws {seed, offset} from the generator as decode_graph._draw_seed does
    sd = torch.randint(0, 2 ** 63 - 1, (2,), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).tolist()
    toks, rows = tg.cpu().numpy(), lg.cpu().numpy()
    sure = 0
    for r in range(toks.shape[0]):
        for k in range(toks.shape[1]):
            if not clear[r * toks.shape[1] + k]:
                continue
            u = S.uniform(S.sample_bits(sd[0], sd[1], r, k, np.arange(64, dtype=np.uint64)))
            want, gap = P.select_p(rows[r, k], top_k=20, top_p=0.5, u=u)
            if gap > 1e-4:
                sure += 1
                assert toks[r, k] == want, (r, k)
    assert sure > 0.7 * toks.size


def test_top_p_is_device_state_and_none_is_the_old_path():
    dev = _dev()
    m, text, seg = _small_model(dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(11)
    with torch.no_grad():
        before = m.generate(text, seg, top_k=16, graph=True, generator=gen())
        n0 = m.decode_graph_captures
        a = m.generate(text, seg, top_k=16, top_p=0.3, graph=True, generator=gen())
        n1 = m.decode_graph_captures
        b = m.generate(text, seg, top_k=16, top_p=0.9, graph=True, generator=gen())
        c = m.generate(text, seg, top_k=16, top_p=0.3, graph=True, generator=gen())
        assert m.decode_graph_captures == n1 == n0 + 1                   # on / off are two keys, the value is none
        assert torch.equal(a, c) and not torch.equal(a, b)
        after = m.generate(text, seg, top_k=16, top_p=None, graph=True, generator=gen())
        one = m.generate(text, seg, top_k=16, top_p=1.0, graph=True, generator=gen())
        assert m.decode_graph_captures == n1
    assert torch.equal(after, before) and torch.equal(one, before)


def test_no_host_synchronisation_between_replays_with_top_p(monkeypatch):
    from models import decode_graph
    dev = _dev()
    m, text, seg = _small_model(dev)
    seen = []
    orig = decode_graph._replay

    def checked(e, n):
        torch.cuda.set_sync_debug_mode("error")
        try:
            orig(e, n)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        seen.append(n)

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        m.generate(text, seg, top_k=8, top_p=0.7, cond_scale=3.0, graph=True)
        monkeypatch.setattr(decode_graph, "_replay", checked)
        m.generate(text, seg, top_k=8, top_p=0.4, cond_scale=3.0, graph=True)
    assert seen == [15] and m.decode_graph_captures == 1


def test_top_p_with_split_decode_attention():
    dev = _dev()
    m, text, seg = _small_model(dev)
    with torch.no_grad():
        t, lg = m.generate(text, seg, top_p=0.5, top_k=20, return_logits=True, graph=True, kv_splits=2,
                           generator=torch.Generator(device=dev).manual_seed(5))
    assert t.shape == (3, 16) and _membership(t, lg, 20, 0.5).mean() >= 0.8
