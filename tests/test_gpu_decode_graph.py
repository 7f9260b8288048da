"""``MakeAScene.generate(graph=True)`` on the MI355X: the device-state decode kernels (``mas_attn_decode_dev``, ``mas_sample_tokens``)
against their references, and the captured decode step against the eager sampler -- teacher-forced logits and greedy tokens bit for bit,
through them the reference's golden logits, seeding, graph reuse, invalidation when weights move or change, no host synchronisation
between replays, the eager fallback outside the envelope, and tokens that decode to an image."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sample_ref as S  # noqa: E402


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def relerr(got, ref):
    got = got.detach().float().cpu()
    ref = torch.as_tensor(ref).float()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


# ---------------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_attn_decode_dev_equals_decode_after_append(dt):
    from mas_hip import decode, ops
    dev = _dev()
    b, h, cap = 2, 2, 1536
    for hd in (16, 32, 64, 128):
        d = h * hd
        g = torch.Generator().manual_seed(hd)
        kc0 = torch.randn(b, cap, d, generator=g).to(dt).to(dev)
        vc0 = torch.randn(b, cap, d, generator=g).to(dt).to(dev)
        for past in (0, 1, 255, 256, 1535):
            qkv = torch.randn(b, 1, 3 * d, generator=g).to(dt).to(dev)
            kr, vr = kc0.clone(), vc0.clone()
            kr[:, past] = qkv[:, 0, d:2 * d]
            vr[:, past] = qkv[:, 0, 2 * d:]
            ref = ops.attention_decode(qkv[..., :d], kr, vr, past, h)
            kc, vc = kc0.clone(), vc0.clone()
            got = decode.attention_decode_dev(qkv, kc, vc, torch.tensor([past], dtype=torch.int32, device=dev), h)
            assert torch.equal(got, ref), (hd, past)
            assert torch.equal(kc, kr) and torch.equal(vc, vr), (hd, past)


def test_attn_decode_dev_writes_nothing_at_capacity():
    from mas_hip import decode
    dev = _dev()
    b, h, hd, cap, guard = 2, 2, 64, 256, 4096
    d = h * hd
    n = b * cap * d
    kflat = torch.randn(n + guard, device=dev).to(torch.bfloat16)
    vflat = torch.randn(n + guard, device=dev).to(torch.bfloat16)
    k0, v0 = kflat.clone(), vflat.clone()
    qkv = torch.randn(b, 1, 3 * d, device=dev).to(torch.bfloat16)
    out = torch.full((b, 1, d), 7.0, device=dev, dtype=torch.bfloat16)
    for past in (cap, cap + 5, -1):
        decode.attention_decode_dev(qkv, kflat[:n].view(b, cap, d), vflat[:n].view(b, cap, d),
                                    torch.tensor([past], dtype=torch.int32, device=dev), h, out=out)
        torch.cuda.synchronize()
        assert torch.equal(kflat.view(torch.int16), k0.view(torch.int16)) and torch.equal(vflat.view(torch.int16), v0.view(torch.int16))
        assert bool((out == 7.0).all())


def _sample(logits_pair, rows, mode, temperature=1.0, cond_scale=None, top_k=0, seed=(12345, 678), logits_out=False):
    from mas_hip import decode
    dev = logits_pair.device
    tokens = torch.zeros((rows, 1), dtype=torch.long, device=dev)
    params = torch.tensor([temperature, cond_scale or 0.0], dtype=torch.float32, device=dev)
    sd = torch.tensor(list(seed), dtype=torch.int64, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    lo = torch.empty((rows, 1, logits_pair.shape[1]), dtype=torch.float32, device=dev) if logits_out else None
    forced = torch.arange(rows, device=dev).view(rows, 1) % logits_pair.shape[1] if mode == decode.FORCED else None
    decode.sample_tokens(logits_pair, tokens, step, params, mode, top_k=top_k, guided=cond_scale is not None, seed=sd, forced=forced,
                         logits_out=lo, rows=rows)
    return tokens[:, 0], lo


@pytest.mark.parametrize("v,top_k,temp,cs", [(64, 0, 0.8, None), (64, 10, 1.0, 2.0), (8192, 50, 0.7, None), (8192, 200, 1.3, 3.0)])
def test_sampler_statistics(v, top_k, temp, cs):
    from mas_hip import decode
    from scipy import stats
    dev = _dev()
    rng = np.random.default_rng(v + top_k)
    lc = (rng.standard_normal(v) * (1.0 if v == 64 else 2.0)).astype(np.float32)
    lu = (rng.standard_normal(v) * 0.5).astype(np.float32)
    pair = torch.from_numpy(np.stack([lc, lu]) if cs is not None else lc[None]).to(dev)
    rows = 100_000
    toks, _ = _sample(pair, rows, decode.SAMPLE, temp, cs, top_k)
    toks = toks.cpu().numpy()
    lg = (S.mix(lc, lu, cs) / np.float32(temp)).astype(np.float32)
    keep = S.kept(lg, top_k)
    counts = np.bincount(toks, minlength=v)
    assert counts[~keep].sum() == 0, "a token outside the top-k set was drawn"
    p = np.exp(lg[keep].astype(np.float64) - lg[keep].max())
    p /= p.sum()
    pval = stats.chisquare(counts[keep], p * rows).pvalue
    assert pval > 1e-3, pval
    # the numpy float64 Gumbel-max reference on the first rows, wherever the best two perturbed scores are apart by more than 1e-4
    n = 2000 if v == 64 else 300
    want, gap = S.select_rows(lc, lu, cs, temp, top_k, 12345, 678, n, 0)
    sure = gap > 1e-4
    assert sure.mean() > 0.9 and (toks[:n][sure] == want[sure]).all()


def test_sampler_keeps_ties_and_mixes_guidance_exactly():
    from mas_hip import decode
    dev = _dev()
    lg = np.full(64, -2.0, np.float32)
    lg[:5] = [3.0, 2.0, 2.0, 2.0, 1.0]                                  # top_k = 2: kth = 2, the three tied entries are kept
    toks, _ = _sample(torch.from_numpy(lg[None]).to(dev), 60_000, decode.SAMPLE, 1.0, None, 2)
    drawn = set(np.unique(toks.cpu().numpy()).tolist())
    assert drawn == {0, 1, 2, 3}
    rng = np.random.default_rng(3)
    lc, lu = rng.standard_normal(8192).astype(np.float32) * 4, rng.standard_normal(8192).astype(np.float32) * 4
    for s in (3.0, 0.3, -1.7, 7.25):
        _, lo = _sample(torch.from_numpy(np.stack([lc, lu])).to(dev), 4, decode.FORCED, cond_scale=s, logits_out=True)
        got = lo.cpu().numpy()
        assert all(np.array_equal(got[r, 0], S.mix(lc, lu, s)) for r in range(4))
        # the same expression with torch's own fp32 kernels (the eager generate)
        lt, ut = torch.from_numpy(lc).to(dev), torch.from_numpy(lu).to(dev)
        assert torch.equal(lo[0, 0], ut + float(s) * (lt - ut))
    toks, _ = _sample(torch.from_numpy(np.stack([lc, lu])).to(dev), 3, decode.GREEDY, cond_scale=3.0)
    assert (toks.cpu().numpy() == int(np.argmax(S.mix(lc, lu, 3.0)))).all()


# ------------------------------------------------------------------------------------------------------------------------------- model
def _golden_model(golden_dir, dev):
    from models.transformer import MakeAScene
    from oracle import transformer_oracle as TO
    cfg = dict(num_layers=2, hidden_dim=64, num_attn_heads=4, image_vocab_size=96, seg_vocab_size=40, text_vocab_size=58,
               image_tokens_per_dim=4, seg_tokens_per_dim=2, text_length=8)
    m = MakeAScene(**cfg)
    m.load_state_dict(TO.synth_transformer_state_dict(cfg, seed=5), strict=True)
    text, seg, img = (t.to(dev) for t in TO.synth_tokens(cfg, batch=2, seed=5))
    return m.to(dev).eval(), text, seg, img, np.load(os.path.join(golden_dir, "transformer_tiny.npz"))


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


def _autocast(on):
    return torch.autocast("cuda", dtype=torch.bfloat16) if on else torch.autocast("cuda", enabled=False)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cs", [None, 2.5], ids=["plain", "guided"])
def test_teacher_forced_graph_equals_eager_and_golden(golden_dir, bf16, cs):
    dev = _dev()
    m, text, seg, img, g = _golden_model(golden_dir, dev)
    with torch.no_grad(), _autocast(bf16):
        te, le = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=cs)
        tg, lg = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=cs, graph=True)
    assert m.decode_graph_captures == 1
    assert torch.equal(tg, img) and torch.equal(te, img) and lg.shape == le.shape == (2, 16, 96) and lg.dtype == torch.float32
    assert torch.equal(lg, le), f"graph vs eager logits: max rel {relerr(lg, le.cpu()):.3e}"
    if cs is None:
        assert relerr(lg, g["logits"]) < (1e-3 if not bf16 else 3e-2)


@pytest.mark.parametrize("cs", [None, 3.0], ids=["plain", "guided"])
def test_greedy_graph_tokens_equal_eager(cs):
    dev = _dev()
    m, text, seg = _small_model(dev)
    with torch.no_grad():
        for bf16 in (False, True):
            with _autocast(bf16):
                te = m.generate(text, seg, temperature=0, cond_scale=cs)
                tg = m.generate(text, seg, temperature=0, cond_scale=cs, graph=True)
            assert tg.dtype == torch.long and tg.shape == (3, 16)
            assert torch.equal(tg, te), bf16


def test_seeding_reproduces_tokens():
    dev = _dev()
    m, text, seg = _small_model(dev)
    run = lambda **kw: m.generate(text, seg, temperature=1.0, top_k=16, graph=True, **kw)
    with torch.no_grad():
        torch.manual_seed(7)
        a = run()
        torch.manual_seed(7)
        b = run()
        torch.manual_seed(8)
        c = run()
        ga = run(generator=torch.Generator(device=dev).manual_seed(5))
        gb = run(generator=torch.Generator(device=dev).manual_seed(5))
        gc = run(generator=torch.Generator(device=dev).manual_seed(6))
        cpu = run(generator=torch.Generator().manual_seed(5))
        cpu2 = run(generator=torch.Generator().manual_seed(5))
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(ga, gb) and not torch.equal(ga, gc)
    assert torch.equal(cpu, cpu2)
    assert int(a.max()) < 64 and int(a.min()) >= 0
    assert m.decode_graph_captures == 1


def _teacher(m, text, seg, img, graph):
    return m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=2.0, graph=graph)[1]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_graph_reuse_and_invalidation(bf16):
    from mas_hip import ops
    from models import decode_graph
    dev = _dev()
    m, text, seg = _small_model(dev)
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 64, (3, 16), generator=g).to(dev)
    img2 = torch.randint(0, 64, (3, 16), generator=g).to(dev)
    text2 = torch.randint(1, 40, (3, 8), generator=g).to(dev)

    def same(tag, captures):
        with torch.no_grad(), _autocast(bf16):
            for t, i in ((text, img), (text2, img2)):
                a, b = _teacher(m, t, seg, i, False), _teacher(m, t, seg, i, True)
                assert torch.equal(a, b), f"{tag}: max rel {relerr(b, a.cpu()):.3e}"
            sig = decode_graph._pointer_signature(m, bf16)
        assert m.decode_graph_captures == captures, tag
        assert all(e.sig == sig for e in m._decode_graphs.values()), tag        # no entry holds a pointer that is not live

    same("two prompts", 1)
    other, _, _ = _small_model(dev, seed=4)
    m.load_state_dict(other.state_dict())
    same("load_state_dict", 1)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    for p in m.parameters():
        p.grad = torch.randn_like(p) * 0.02
    opt.step()
    same("optimizer step", 1)
    # (the old storage is held while the new one is allocated, so the caching allocator cannot hand the same addresses back)
    held = [e[2] for e in ops._bf16_shadows.params.values()]
    ops.invalidate_weight_cache()
    same("invalidate_weight_cache", 2 if bf16 else 1)                           # new bf16 shadows: recaptured
    held = [p.data for p in m.parameters()]
    m.cpu()
    m.to(dev)
    same(".to()", 3 if bf16 else 2)                                               # new parameter storage: recaptured
    del held
    m.release_decode_graphs()
    assert not m.__dict__.get("_decode_graphs")


def test_temperature_and_cond_scale_do_not_recapture():
    dev = _dev()
    m, text, seg = _small_model(dev)
    with torch.no_grad():
        outs = [m.generate(text, seg, temperature=t, top_k=8, cond_scale=s, graph=True,
                           generator=torch.Generator(device=dev).manual_seed(1)) for t, s in ((1.0, 2.0), (0.5, 2.0), (1.0, 5.0), (2.0, 0.5))]
    assert m.decode_graph_captures == 1
    assert len({tuple(o.flatten().tolist()) for o in outs}) > 1


def test_no_host_synchronisation_between_replays(monkeypatch):
    """the replay loop of a call whose graph is already captured runs under torch's sync debug mode "error": any synchronising call
    (``.item()``, a blocking copy, a stream or device synchronise) between the first and the last replay raises"""
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

    with torch.no_grad(), _autocast(True):
        m.generate(text, seg, temperature=1.0, top_k=8, cond_scale=3.0, graph=True)
        monkeypatch.setattr(decode_graph, "_replay", checked)
        m.generate(text, seg, temperature=1.0, top_k=8, cond_scale=3.0, graph=True)
    assert seen == [15] and m.decode_graph_captures == 1


@pytest.mark.parametrize("hidden,heads", [(96, 4), (100, 5)], ids=["hd24", "hd20"])
def test_fallback_outside_the_envelope_warns_once_and_equals_eager(hidden, heads):
    dev = _dev()
    m, text, seg = _small_model(dev, seed=2, hidden=hidden, heads=heads)
    img = torch.randint(0, 64, (3, 16), generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        te = m.generate(text, seg, temperature=0)
        with pytest.warns(RuntimeWarning, match="head width"):
            tg = m.generate(text, seg, temperature=0, graph=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            lg = m.generate(text, seg, img_tokens=img, return_logits=True, graph=True)[1]
        le = m.generate(text, seg, img_tokens=img, return_logits=True)[1]
    assert torch.equal(tg, te) and torch.equal(lg, le)
    assert m.decode_graph_captures == 0


def test_greedy_graph_tokens_decode_to_an_image():
    from models import VQBASE
    dev = _dev()
    m, text, seg = _small_model(dev)
    with torch.no_grad():
        tok = m.generate(text, seg, temperature=0, graph=True)
        assert tok.shape == (3, 16) and int(tok.max()) < 64
        assert (m(text, seg, tok).argmax(-1) == tok).float().mean() > 0.95
    vq = VQBASE(ddconfig=dict(z_channels=32, in_channels=3, out_channels=3, channels=[32, 32, 64], num_res_blocks=1, resolution=16,
                              attn_resolutions=[8], dropout=0.0), n_embed=64, embed_dim=32, init_steps=10, reservoir_size=100).to(dev).eval()
    with torch.no_grad():
        img = vq.decode_code(tok.view(3, 4, 4))
    assert img.shape == (3, 3, 8, 8) and torch.isfinite(img).all()
