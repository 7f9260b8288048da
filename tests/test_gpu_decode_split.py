"""Split-key decode attention on the MI355X (``mas_attn_decode_split`` / ``mas_attn_decode_split_dev``, ``generate(kv_splits=...)``): the
kernel pair against a torch fp32 CPU softmax(qK^T)V at the tolerances the unsplit kernel is held to (tests/test_gpu_sampling.py) and
against the float64 split-and-merge restatement (tests/helpers/decode_split_ref.py); the device-``past`` form against the host form bit
for bit, its append, and its silence at ``past`` = capacity; repeatability; and the sampler with ``kv_splits`` -- teacher-forced logits
against the uncached forward and the reference's golden logits, graph == eager bit for bit, graph reuse per split count, no host
synchronisation between replays, and nothing left behind on the modules."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import decode_split_ref as R  # noqa: E402

HEAD_DIMS = (16, 32, 64, 128)
SPLITS = (2, 3, 8, 16)
PASTS = (0, 1, 63, 64, 255, 256, 1000, 1534)
CAP = 1536


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def relerr(got, ref):
    got = got.detach().float().cpu()
    ref = torch.as_tensor(ref).float()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


def _past_t(past, dev):
    return torch.tensor([past], dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_split_decode_vs_torch(hd, dt):
    """every split count x cache length against torch's fp32 softmax(qK^T)V on the CPU: rel-max < 2e-5 (fp32), < 1e-2 (bf16); rows past
    the valid length are NaN, so an over-read shows; the float64 split-and-merge restatement agrees with both"""
    from mas_hip import ops
    dev = _dev()
    b, h = 2, 2
    d = h * hd
    tol = 2e-5 if dt == torch.float32 else 1e-2
    g = torch.Generator().manual_seed(100 + hd)
    kc0 = torch.randn(b, CAP, d, generator=g).to(dt)
    vc0 = torch.randn(b, CAP, d, generator=g).to(dt)
    worst = 0.0
    for past in PASTS:
        L = past + 1
        q = torch.randn(b, 1, d, generator=g).to(dt)
        kc, vc = kc0.clone(), vc0.clone()
        kc[:, L:] = float("nan")                     # rows past the valid length must never be read
        vc[:, L:] = float("nan")
        qq = q[:, 0].float().view(b, h, 1, hd) / math.sqrt(hd)
        k = kc[:, :L].float().view(b, L, h, hd).permute(0, 2, 1, 3)
        v = vc[:, :L].float().view(b, L, h, hd).permute(0, 2, 1, 3)
        ref = (torch.softmax(qq @ k.transpose(-1, -2), -1) @ v).reshape(b, 1, d)
        qd, kd, vd = q.to(dev), kc.to(dev), vc.to(dev)
        qkv = torch.randn(b, 1, 3 * d, generator=g).to(dt)
        qkv[..., :d] = q
        qs = qkv.to(dev)[..., :d]                    # a strided view of a fused qkv projection as the query (what SelfAttention passes)
        for n in SPLITS:
            out = ops.attention_decode(qd, kd, vd, past, h, kv_splits=n)
            assert out.dtype == dt and out.shape == (b, 1, d)
            err = relerr(out, ref)
            worst = max(worst, err)
            assert err < tol, (hd, dt, past, n, err)
            assert torch.equal(ops.attention_decode(qs, kd, vd, past, h, kv_splits=n), out)
            # second reference: the float64 restatement of the pair on head (1, 1)
            r64 = R.split_attention(qq[1, 1, 0].double().numpy(), k[1, 1].double().numpy(), v[1, 1].double().numpy(), n)
            assert np.abs(r64 - ref[1, 0, hd:].double().numpy()).max() < 1e-5
            got = out[1, 0, hd:].float().cpu().double().numpy()
            assert np.abs(got - r64).max() / np.abs(r64).max() < tol, (hd, dt, past, n)
    print(f"split decode hd={hd} {dt}: worst rel-max error {worst:.3e} (bound {tol:g})")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_split_dev_equals_split_after_append(dt):
    """device-``past`` form == host-``past`` form on a cache where the row was appended by the host, bit for bit, and the caches after
    the call are the appended ones"""
    from mas_hip import decode, ops
    dev = _dev()
    b, h = 2, 2
    for hd in HEAD_DIMS:
        d = h * hd
        g = torch.Generator().manual_seed(hd)
        kc0 = torch.randn(b, CAP, d, generator=g).to(dt).to(dev)
        vc0 = torch.randn(b, CAP, d, generator=g).to(dt).to(dev)
        for past in PASTS + (CAP - 1,):
            qkv = torch.randn(b, 1, 3 * d, generator=g).to(dt).to(dev)
            kr, vr = kc0.clone(), vc0.clone()
            kr[:, past] = qkv[:, 0, d:2 * d]
            vr[:, past] = qkv[:, 0, 2 * d:]
            for n in SPLITS:
                ref = ops.attention_decode(qkv[..., :d], kr, vr, past, h, kv_splits=n)
                kc, vc = kc0.clone(), vc0.clone()
                got = decode.attention_decode_dev(qkv, kc, vc, _past_t(past, dev), h, kv_splits=n)
                assert torch.equal(got, ref), (hd, past, n)
                assert torch.equal(kc, kr) and torch.equal(vc, vr), (hd, past, n)


def test_split_dev_writes_nothing_at_capacity():
    """guard pages of a sentinel around the caches and the workspace: at past outside [0, capacity) nothing is written anywhere (the
    workspace and the output included); at a valid past only cache row ``past`` and the workspace proper change"""
    from mas_hip import decode
    dev = _dev()
    b, h, hd, cap, guard, n = 2, 2, 64, 256, 4096, 8
    d = h * hd
    nel = b * cap * d
    kflat = torch.randn(nel + 2 * guard, device=dev).to(torch.bfloat16)
    vflat = torch.randn(nel + 2 * guard, device=dev).to(torch.bfloat16)
    need = decode.split_workspace_floats(b, h, hd, n)
    wflat = torch.full((need + 2 * guard,), -777.0, device=dev)
    k0, v0, w0 = kflat.clone(), vflat.clone(), wflat.clone()
    kc, vc = (t[guard:guard + nel].view(b, cap, d) for t in (kflat, vflat))
    ws = wflat[guard:guard + need]
    qkv = torch.randn(b, 1, 3 * d, device=dev).to(torch.bfloat16)
    out = torch.full((b, 1, d), 7.0, device=dev, dtype=torch.bfloat16)
    bits = lambda t: t.view(torch.int16)
    for past in (cap, cap + 5, -1):
        decode.attention_decode_dev(qkv, kc, vc, _past_t(past, dev), h, out=out, kv_splits=n, workspace=ws)
        torch.cuda.synchronize()
        assert torch.equal(bits(kflat), bits(k0)) and torch.equal(bits(vflat), bits(v0)), past
        assert torch.equal(wflat, w0), past
        assert bool((out == 7.0).all()), past
    past = cap - 1
    decode.attention_decode_dev(qkv, kc, vc, _past_t(past, dev), h, out=out, kv_splits=n, workspace=ws)
    torch.cuda.synchronize()
    k1, v1 = k0.clone(), v0.clone()
    k1[guard:guard + nel].view(b, cap, d)[:, past] = qkv[:, 0, d:2 * d]
    v1[guard:guard + nel].view(b, cap, d)[:, past] = qkv[:, 0, 2 * d:]
    assert torch.equal(bits(kflat), bits(k1)) and torch.equal(bits(vflat), bits(v1))
    assert torch.equal(wflat[:guard], w0[:guard]) and torch.equal(wflat[guard + need:], w0[guard + need:])
    assert bool((ws != -777.0).all()) and bool(torch.isfinite(out.float()).all()) and not bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match="workspace"):
        decode.attention_decode_dev(qkv, kc, vc, _past_t(past, dev), h, out=out, kv_splits=n, workspace=ws[:-1])


def test_split_is_repeatable_and_one_split_is_the_unsplit_kernel():
    from mas_hip import decode, ops
    dev = _dev()
    b, h, hd, past = 2, 16, 64, 1200
    d = h * hd
    g = torch.Generator().manual_seed(3)
    for dt in (torch.float32, torch.bfloat16):
        qkv = torch.randn(b, 1, 3 * d, generator=g).to(dt).to(dev)
        kc = torch.randn(b, CAP, d, generator=g).to(dt).to(dev)
        vc = torch.randn(b, CAP, d, generator=g).to(dt).to(dev)
        q = qkv[..., :d]
        today = ops.attention_decode(q, kc, vc, past, h)
        assert torch.equal(ops.attention_decode(q, kc, vc, past, h, kv_splits=None), today)
        assert torch.equal(ops.attention_decode(q, kc, vc, past, h, kv_splits=1), today)
        for n in SPLITS:
            a = ops.attention_decode(q, kc, vc, past, h, kv_splits=n)
            assert torch.equal(ops.attention_decode(q, kc, vc, past, h, kv_splits=n), a), n
            assert relerr(a, today.cpu()) < (2e-5 if dt == torch.float32 else 1e-2)
        dev_today = decode.attention_decode_dev(qkv, kc.clone(), vc.clone(), _past_t(past, dev), h)
        for n in (None, 1):
            assert torch.equal(decode.attention_decode_dev(qkv, kc.clone(), vc.clone(), _past_t(past, dev), h, kv_splits=n), dev_today)
        for n in SPLITS:
            a = decode.attention_decode_dev(qkv, kc.clone(), vc.clone(), _past_t(past, dev), h, kv_splits=n)
            assert torch.equal(decode.attention_decode_dev(qkv, kc.clone(), vc.clone(), _past_t(past, dev), h, kv_splits=n), a), n
    q3 = torch.randn(b, 3, d, generator=g).to(dev)
    ops.attention_decode(q3, kc.float(), vc.float(), 10, h)                        # nq = 3 is the unsplit kernel's ground ...
    with pytest.raises(RuntimeError, match="nq"):
        ops.attention_decode(q3, kc.float(), vc.float(), 10, h, kv_splits=2)       # ... and an error with splits
    with pytest.raises(RuntimeError, match="kv_splits"):
        ops.attention_decode(q, kc, vc, past, h, kv_splits=33)


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


def _long_model(dev, seed=11):
    """2 layers, D = 128, 2 heads of 64, 64 text + 8x8 seg + 16x16 image = 384 positions, seeded weights"""
    from models.transformer import MakeAScene
    torch.manual_seed(seed)
    m = MakeAScene(num_layers=2, hidden_dim=128, num_attn_heads=2, image_vocab_size=64, seg_vocab_size=16, text_vocab_size=200,
                   image_tokens_per_dim=16, seg_tokens_per_dim=8, text_length=64).to(dev).eval()
    g = torch.Generator().manual_seed(seed + 1)
    text = torch.randint(1, 130, (2, 64), generator=g)
    text[:, 50:] = 0
    seg = torch.randint(0, 16, (2, 64), generator=g)
    img = torch.randint(0, 64, (2, 256), generator=g)
    return m, text.to(dev), seg.to(dev), img.to(dev)


def _autocast(on):
    return torch.autocast("cuda", dtype=torch.bfloat16) if on else torch.autocast("cuda", enabled=False)


def _uncached(m, text, seg, img, cs):
    """the uncached forward (the training attention kernel), mixed as ``generate`` mixes under guidance"""
    lc = m(text, seg, img).float()
    if cs is None:
        return lc
    lu = m(torch.zeros_like(text), seg, img).float()
    return lu + float(cs) * (lc - lu)


@pytest.mark.parametrize("cs", [None, 2.5], ids=["plain", "guided"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("n", [2, 8])
def test_teacher_forced_golden_model(golden_dir, n, graph, cs):
    """the bounds of test_cached_decoding_*: vs the uncached forward < 1e-4 (fp32), vs the reference's golden logits < 1e-3 (fp32) and
    < 3e-2 (bf16 autocast)"""
    dev = _dev()
    m, text, seg, img, g = _golden_model(golden_dir, dev)
    with torch.no_grad():
        full = _uncached(m, text, seg, img, cs)
        toks, logits = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=cs, graph=graph, kv_splits=n)
        with _autocast(True):
            _, lb = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=cs, graph=graph, kv_splits=n)
    assert torch.equal(toks, img) and logits.shape == (2, 16, 96) and logits.dtype == torch.float32
    e_full = relerr(logits, full.cpu())
    print(f"kv_splits={n} graph={graph} cs={cs}: vs uncached forward {e_full:.2e}")
    assert e_full < 1e-4
    if cs is None:
        e_gold, e_bf = relerr(logits, g["logits"]), relerr(lb, g["logits"])
        print(f"    vs reference golden {e_gold:.2e} (fp32), {e_bf:.2e} (bf16 autocast)")
        assert e_gold < 1e-3
        assert e_bf < 3e-2
    if graph:
        assert m.decode_graph_captures == 2                                     # one per autocast state


@pytest.mark.parametrize("cs", [None, 2.5], ids=["plain", "guided"])
def test_teacher_forced_long_model_vs_its_uncached_forward(cs):
    """384 positions (up to 383 cached rows: every split has keys): < 1e-4 in fp32 against the model's own uncached forward"""
    dev = _dev()
    m, text, seg, img = _long_model(dev)
    with torch.no_grad():
        full = _uncached(m, text, seg, img, cs).cpu()
        for n in (2, 8):
            for graph in (False, True):
                toks, logits = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=cs, graph=graph, kv_splits=n)
                err = relerr(logits, full)
                print(f"long model kv_splits={n} graph={graph} cs={cs}: vs uncached forward {err:.2e}")
                assert torch.equal(toks, img) and logits.shape == (2, 256, 64)
                assert err < 1e-4, (n, graph, err)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cs", [None, 3.0], ids=["plain", "guided"])
def test_graph_equals_eager_at_equal_kv_splits(bf16, cs):
    """teacher-forced logits and greedy tokens, bit for bit -- what the unsplit pair guarantees"""
    dev = _dev()
    m, text, seg, img = _long_model(dev, seed=21)
    with torch.no_grad(), _autocast(bf16):
        for n in (2, 8):
            le = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=cs, kv_splits=n)[1]
            lg = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=cs, graph=True, kv_splits=n)[1]
            assert torch.equal(lg, le), f"kv_splits={n}: graph vs eager logits max rel {relerr(lg, le.cpu()):.3e}"
            te = m.generate(text, seg, temperature=0, cond_scale=cs, kv_splits=n)
            tg = m.generate(text, seg, temperature=0, cond_scale=cs, graph=True, kv_splits=n)
            assert tg.dtype == torch.long and tg.shape == (2, 256)
            assert torch.equal(tg, te), n


def test_one_graph_per_split_count_and_no_sync_between_replays(monkeypatch):
    from models import decode_graph
    dev = _dev()
    m, text, seg, img = _long_model(dev, seed=31)
    run = lambda n: m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=2.0, graph=True, kv_splits=n)[1]
    with torch.no_grad():
        a8 = run(8)
        assert m.decode_graph_captures == 1
        a2 = run(2)
        assert m.decode_graph_captures == 2                                     # another split count: a second graph ...
        assert torch.equal(run(8), a8) and torch.equal(run(2), a2)              # ... and the first still replays
        assert m.decode_graph_captures == 2                                     # same count: no recapture
        a0 = run(None)
        assert m.decode_graph_captures == 3 and torch.equal(run(1), a0) and m.decode_graph_captures == 3   # None and 1 share the unsplit graph
        assert torch.equal(a0, m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=2.0, graph=True)[1])
        auto = decode_graph.decode.resolve_kv_splits("auto", 4, 2, torch.cuda.get_device_properties(dev).multi_processor_count)
        assert auto > 1
        la = run("auto")
        assert torch.equal(la, run(auto))
        keys = {k[-1] for k in m._decode_graphs}
        assert keys == {1, 2, 8, auto}
        assert all((e.split_ws is None) == (e.kv_splits == 1) for e in m._decode_graphs.values())
        captures = m.decode_graph_captures

        seen = []
        orig = decode_graph._replay

        def checked(e, n):
            torch.cuda.set_sync_debug_mode("error")
            try:
                orig(e, n)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            seen.append((e.kv_splits, n))

        monkeypatch.setattr(decode_graph, "_replay", checked)
        with _autocast(False):
            assert torch.equal(run(8), a8)
    assert seen == [(8, 255)] and m.decode_graph_captures == captures


def test_kv_splits_leaves_nothing_behind():
    """after generate(kv_splits=8) a plain generate() returns the bits it returned before: the attribute was restored"""
    dev = _dev()
    m, text, seg, img = _long_model(dev, seed=41)
    attns = [layer.attn for layer in m.transformer.layers]
    with torch.no_grad():
        before = m.generate(text, seg, img_tokens=img, return_logits=True)[1]
        greedy = m.generate(text, seg, temperature=0)
        split = m.generate(text, seg, img_tokens=img, return_logits=True, kv_splits=8)[1]
        assert all("decode_kv_splits" not in a.__dict__ for a in attns)
        assert torch.equal(m.generate(text, seg, img_tokens=img, return_logits=True)[1], before)
        assert torch.equal(m.generate(text, seg, temperature=0), greedy)
        assert relerr(split, before.cpu()) < 1e-4                                # another summation order, the same logits
        with pytest.raises(ValueError):
            m.generate(text, seg, temperature=0, kv_splits=0)
        with pytest.raises(ValueError):
            m.generate(text, seg, temperature=0, kv_splits="fast")
        assert all("decode_kv_splits" not in a.__dict__ for a in attns)
        # an attribute the caller set is put back, not removed
        for a in attns:
            a.decode_kv_splits = 2
        two = m.generate(text, seg, img_tokens=img, return_logits=True)[1]      # kv_splits=None -> 1 for the call
        assert torch.equal(two, before) and all(a.decode_kv_splits == 2 for a in attns)
