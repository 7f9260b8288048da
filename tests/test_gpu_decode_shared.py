"""Shared-prompt decode attention on the MI355X (``mas_attn_decode_shared`` / ``mas_attn_decode_shared_dev``,
``generate(num_samples=n)``): the kernel pair against a torch fp32 CPU softmax(qK^T)V over the concatenated keys at the tolerances the
unsplit kernel is held to and against the float64 restatement (tests/helpers/decode_shared_ref.py); what is bit-stable (device ``past``
== host ``past``, repeats, a row's place in its group, other groups' prompts); the device guard with sentinel pages; and the sampler:
teacher-forced logits of every candidate against the golden logits and the uncached forward, the expanded paths bit for bit, seeds,
``keep``, the entry's buffers, one capture per configuration and no host synchronisation between replays."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import decode_shared_ref as S  # noqa: E402

HEAD_DIMS = (16, 32, 64, 128)
GROUPS, H, CAP = 2, 2, 72
GROUP_SIZES = (1, 3, 5, 8, 9)            # QT and QT + 1 for a tile of 4 or of 8 queries
PROMPT_LENS = (1, 31, 33, 300)           # 300 keys in 2 ranges: more than one pass of the key loop at hd 64 bf16 (128 keys per pass)
OWN_PASTS = (0, 1, 31, 32, 70)
PROMPT_SPLITS = (1, 2, 5)
KV_SPLITS = (1, 3)
# the thinned cross: every value of every axis, and (300, 2 prompt ranges) at i = 7
CASES = [(GROUP_SIZES[i % 5], PROMPT_LENS[i % 4], OWN_PASTS[(2 * i) % 5], PROMPT_SPLITS[i % 3], KV_SPLITS[i % 2]) for i in range(10)]


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


def _case(hd, dt, group, plen, own_past, g, same_rows=False):
    """CPU tensors of one case: q [rows, 1, d] inside a fused qkv row, two different prompt blocks as views of a buffer whose other
    rows are NaN, own caches whose rows past the valid length are NaN, and the torch fp32 reference [rows, 1, d]"""
    d = H * hd
    rows = GROUPS * group
    L = own_past + 1
    qkv = torch.randn(rows, 1, 3 * d, generator=g).to(dt)
    kc = torch.randn(rows, CAP, d, generator=g).to(dt)
    vc = torch.randn(rows, CAP, d, generator=g).to(dt)
    if same_rows:                                    # every row of a group: the same query, the same own cache
        for t in (qkv, kc, vc):
            t.copy_(t.view(GROUPS, group, *t.shape[1:])[:, :1].expand(GROUPS, group, *t.shape[1:]).reshape(t.shape))
    kc[:, L:] = float("nan")                         # rows past the valid length must never be read
    vc[:, L:] = float("nan")
    big_k = torch.full((GROUPS, plen + 4, d), float("nan")).to(dt)
    big_v = torch.full((GROUPS, plen + 4, d), float("nan")).to(dt)
    big_k[:, 2:2 + plen] = torch.randn(GROUPS, plen, d, generator=g).to(dt)
    big_v[:, 2:2 + plen] = torch.randn(GROUPS, plen, d, generator=g).to(dt)
    q = qkv[:, 0, :d].float().view(rows, H, 1, hd) / math.sqrt(hd)
    keys = torch.cat([big_k[:, 2:2 + plen].float().repeat_interleave(group, 0), kc[:, :L].float()], dim=1)
    vals = torch.cat([big_v[:, 2:2 + plen].float().repeat_interleave(group, 0), vc[:, :L].float()], dim=1)
    k = keys.view(rows, plen + L, H, hd).permute(0, 2, 1, 3)
    v = vals.view(rows, plen + L, H, hd).permute(0, 2, 1, 3)
    ref = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).permute(0, 2, 1, 3).reshape(rows, 1, d)
    return qkv, big_k, big_v, kc, vc, ref, (q, k, v)


def _to_dev(dev, qkv, big_k, big_v, kc, vc, plen):
    bk, bv = big_k.to(dev), big_v.to(dev)
    return qkv.to(dev), bk[:, 2:2 + plen], bv[:, 2:2 + plen], kc.to(dev), vc.to(dev)


# ---------------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_shared_decode_vs_torch(hd, dt):
    """rel-max < 2e-5 (fp32), < 1e-2 (bf16) against torch's fp32 softmax over the concatenated keys on the CPU; NaN everywhere the
    kernel has no business (around the prompt blocks, past the own rows): an over-read or a wrong group shows; the float64 restatement
    agrees with both"""
    from mas_hip import ops
    dev = _dev()
    d = H * hd
    tol = 2e-5 if dt == torch.float32 else 1e-2
    g = torch.Generator().manual_seed(300 + hd)
    worst = 0.0
    for group, plen, own_past, nsp, nso in CASES:
        qkv, big_k, big_v, kc, vc, ref, (q, k, v) = _case(hd, dt, group, plen, own_past, g)
        qkv_d, pk, pv, kc_d, vc_d = _to_dev(dev, qkv, big_k, big_v, kc, vc, plen)
        past = plen + own_past
        qs = qkv_d[..., :d]                          # a strided view of a fused qkv row, what the step passes
        out = ops.attention_decode_shared(qs, pk, pv, kc_d, vc_d, past, H, group=group, prompt_splits=nsp, kv_splits=nso)
        assert out.dtype == dt and out.shape == (GROUPS * group, 1, d)
        err = relerr(out, ref)
        worst = max(worst, err)
        print(f"shared decode hd={hd} {dt} group={group} plen={plen} own_past={own_past} splits=({nsp},{nso}): rel-max {err:.3e}")
        assert err < tol, (hd, dt, group, plen, own_past, nsp, nso, err)
        assert torch.equal(ops.attention_decode_shared(qs.contiguous(), pk, pv, kc_d, vc_d, past, H, group=group, prompt_splits=nsp,
                                                       kv_splits=nso), out)
        # second reference: the float64 restatement on the last row (group 1), head 1
        r = GROUPS * group - 1
        k64, v64 = k[r, 1].double().numpy(), v[r, 1].double().numpy()
        r64 = S.shared_attention(q[r, 1, 0].double().numpy(), k64[:plen], v64[:plen], k64[plen:], v64[plen:], nsp, nso)
        assert np.abs(r64 - ref[r, 0, hd:].double().numpy()).max() < 1e-5
        got = out[r, 0, hd:].float().cpu().double().numpy()
        assert np.abs(got - r64).max() / np.abs(r64).max() < tol, (hd, dt, group, plen, own_past, nsp, nso)
    print(f"shared decode hd={hd} {dt}: worst rel-max error {worst:.3e} (bound {tol:g})")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_shared_dev_equals_host_form_and_repeats(dt):
    """device-``past`` form == host form on a host-appended cache, bit for bit; the caches afterwards are the appended ones; a second
    call returns the same bits"""
    from mas_hip import decode, ops
    dev = _dev()
    for hd in HEAD_DIMS:
        d = H * hd
        g = torch.Generator().manual_seed(400 + hd)
        for group, plen, own_past, nsp, nso in CASES[3:8]:
            qkv, big_k, big_v, kc, vc, _, _ = _case(hd, dt, group, plen, own_past, g)
            qkv_d, pk, pv, kc0, vc0 = _to_dev(dev, qkv, big_k, big_v, kc, vc, plen)
            past = plen + own_past
            kr, vr = kc0.clone(), vc0.clone()                       # row own_past holds random data: the append must replace it
            kr[:, own_past] = qkv_d[:, 0, d:2 * d]
            vr[:, own_past] = qkv_d[:, 0, 2 * d:]
            ref = ops.attention_decode_shared(qkv_d[..., :d], pk, pv, kr, vr, past, H, group=group, prompt_splits=nsp, kv_splits=nso)
            assert torch.equal(ops.attention_decode_shared(qkv_d[..., :d], pk, pv, kr, vr, past, H, group=group, prompt_splits=nsp,
                                                           kv_splits=nso).view(torch.uint8), ref.view(torch.uint8))
            for _ in range(2):
                kc_d, vc_d = kc0.clone(), vc0.clone()
                got = decode.attention_decode_shared_dev(qkv_d, pk, pv, kc_d, vc_d, _past_t(past, dev), H, group=group,
                                                         prompt_splits=nsp, kv_splits=nso)
                assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8)), (hd, group, plen, own_past, nsp, nso)
                bits = lambda t: t.view(torch.uint8)                # NaN rows compare as bytes
                assert torch.equal(bits(kc_d), bits(kr)) and torch.equal(bits(vc_d), bits(vr))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_rows_of_a_group_and_other_groups(dt):
    """rows of a group with the same query and the same own cache return the same bits wherever they sit in the query tile (9 rows:
    tiles of 4 + 4 + 1, or 8 + 1); another group's prompt block does not reach this group's bits"""
    from mas_hip import ops
    dev = _dev()
    for hd in HEAD_DIMS:
        d = H * hd
        g = torch.Generator().manual_seed(500 + hd)
        group, plen, own_past, nsp, nso = 9, 300, 70, 2, 3
        qkv, big_k, big_v, kc, vc, ref, _ = _case(hd, dt, group, plen, own_past, g, same_rows=True)
        qkv_d, pk, pv, kc_d, vc_d = _to_dev(dev, qkv, big_k, big_v, kc, vc, plen)
        run = lambda: ops.attention_decode_shared(qkv_d[..., :d], pk, pv, kc_d, vc_d, plen + own_past, H, group=group,
                                                  prompt_splits=nsp, kv_splits=nso)
        out = run()
        assert relerr(out, ref) < (2e-5 if dt == torch.float32 else 1e-2)
        for grp in range(GROUPS):
            rows = out[grp * group:(grp + 1) * group]
            assert torch.equal(rows, rows[:1].expand_as(rows)), (hd, grp)
        assert not torch.equal(out[0], out[group])                  # the two prompt blocks hold different data
        pk[1].normal_()                                              # group 1's block (a view: group 0's bytes stay)
        pv[1].normal_()
        out2 = run()
        assert torch.equal(out2[:group], out[:group]) and not torch.equal(out2[group:], out[group:])


def test_shared_dev_guard_with_sentinel_pages():
    """sentinel pages around the caches, the prompt blocks, the workspace and the output: at *past < prompt_len and at *past -
    prompt_len >= capacity nothing is written anywhere; at the last valid past only that cache row, the workspace proper and the output
    change; a workspace one float short raises"""
    from mas_hip import decode
    dev = _dev()
    group, hd, cap, plen, guard, nsp, nso = 5, 64, 40, 33, 4096, 2, 3
    rows, d = GROUPS * group, H * hd
    dt = torch.bfloat16
    bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t

    def paged(n, fill=None):
        flat = torch.randn(n + 2 * guard, device=dev).to(dt) if fill is None else torch.full((n + 2 * guard,), fill, device=dev)
        return flat, flat[guard:guard + n]

    kflat, kin = paged(rows * cap * d)
    vflat, vin = paged(rows * cap * d)
    pkflat, pkin = paged(GROUPS * plen * d)
    pvflat, pvin = paged(GROUPS * plen * d)
    need = decode.shared_workspace_floats(rows, H, hd, nsp, nso)
    wflat, ws = paged(need, -777.0)
    oflat, oin = paged(rows * d, 7.0)
    oflat = oflat.to(dt)
    oin = oflat[guard:guard + rows * d]
    kc, vc = kin.view(rows, cap, d), vin.view(rows, cap, d)
    pk, pv = pkin.view(GROUPS, plen, d), pvin.view(GROUPS, plen, d)
    out = oin.view(rows, 1, d)
    flats = (kflat, vflat, pkflat, pvflat, wflat, oflat)
    before = [t.clone() for t in flats]
    qkv = torch.randn(rows, 1, 3 * d, device=dev).to(dt)
    call = lambda past, w=ws: decode.attention_decode_shared_dev(qkv, pk, pv, kc, vc, _past_t(past, dev), H, group=group,
                                                                 prompt_splits=nsp, kv_splits=nso, workspace=w, out=out)
    for past in (plen - 1, 0, -1, plen + cap, plen + cap + 5):
        call(past)
        torch.cuda.synchronize()
        for t, t0 in zip(flats, before):
            assert torch.equal(bits(t), bits(t0)), past
    past = plen + cap - 1                                            # the last valid one: own row cap - 1
    call(past)
    torch.cuda.synchronize()
    k1, v1 = before[0].clone(), before[1].clone()
    k1[guard:guard + rows * cap * d].view(rows, cap, d)[:, cap - 1] = qkv[:, 0, d:2 * d]
    v1[guard:guard + rows * cap * d].view(rows, cap, d)[:, cap - 1] = qkv[:, 0, 2 * d:]
    assert torch.equal(bits(kflat), bits(k1)) and torch.equal(bits(vflat), bits(v1))
    assert torch.equal(bits(pkflat), bits(before[2])) and torch.equal(bits(pvflat), bits(before[3]))
    assert torch.equal(wflat[:guard], before[4][:guard]) and torch.equal(wflat[guard + need:], before[4][guard + need:])
    assert torch.equal(bits(oflat[:guard]), bits(before[5][:guard])) and torch.equal(bits(oflat[guard + rows * d:]),
                                                                                   bits(before[5][guard + rows * d:]))
    assert bool((ws != -777.0).all()) and bool(torch.isfinite(out.float()).all()) and not bool((out == 7.0).any())
    with pytest.raises(RuntimeError, match="workspace"):
        call(past, ws[:-1])


def test_wrappers_reject_non_integer_splits_and_other_devices():
    from mas_hip import decode, ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    qkv, big_k, big_v, kc, vc, _, _ = _case(16, torch.float32, 3, 31, 1, g)
    qkv_d, pk, pv, kc_d, vc_d = _to_dev(dev, qkv, big_k, big_v, kc, vc, 31)
    q = qkv_d[..., :2 * 16]
    for bad in (2.7, True, "2", 0, 33):
        for kw in (dict(prompt_splits=bad), dict(kv_splits=bad)):
            with pytest.raises(RuntimeError, match="splits"):
                ops.attention_decode_shared(q, pk, pv, kc_d, vc_d, 32, H, group=3, **kw)
            with pytest.raises(RuntimeError, match="splits"):
                decode.attention_decode_shared_dev(qkv_d, pk, pv, kc_d, vc_d, _past_t(32, dev), H, group=3, **kw)
    with pytest.raises(RuntimeError, match="device"):
        ops.attention_decode_shared(q, pk.cpu(), pv.cpu(), kc_d, vc_d, 32, H, group=3)
    with pytest.raises(RuntimeError, match="device"):
        decode.attention_decode_shared_dev(qkv_d, pk, pv, kc_d.cpu(), vc_d.cpu(), _past_t(32, dev), H, group=3)
    for bad_group in (0, 4, 2.0, True):
        with pytest.raises(RuntimeError, match="group"):
            ops.attention_decode_shared(q, pk, pv, kc_d, vc_d, 32, H, group=bad_group)


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
def test_golden_model_three_candidates(golden_dir, cs):
    """num_samples=3, teacher-forced with every prompt's golden tokens: every candidate row's logits vs the reference's golden logits
    for its prompt < 1e-3 (fp32), < 3e-2 (bf16 autocast), vs the uncached forward < 1e-4 (fp32)"""
    dev = _dev()
    m, text, seg, img, g = _golden_model(golden_dir, dev)
    img3 = img.repeat_interleave(3, 0)
    with torch.no_grad():
        full = _uncached(m, text, seg, img, cs).repeat_interleave(3, 0)
        kw = dict(img_tokens=img3, return_logits=True, cond_scale=cs, graph=True, num_samples=3, share_prompt=True)
        toks, logits = m.generate(text, seg, **kw)
        with _autocast(True):
            _, lb = m.generate(text, seg, **kw)
    assert torch.equal(toks, img3) and logits.shape == (6, 16, 96) and logits.dtype == torch.float32
    assert any(e.group == 3 for e in m._decode_graphs.values())                 # the shared path ran, not the expanded one
    e_full = relerr(logits, full.cpu())
    print(f"num_samples=3 cs={cs}: vs uncached forward {e_full:.2e}")
    assert e_full < 1e-4
    for j in range(6):
        assert relerr(logits[j], full[j].cpu()) < 1e-4, j
    if cs is None:
        gold = torch.as_tensor(g["logits"]).repeat_interleave(3, 0)
        for j in range(6):
            e_gold, e_bf = relerr(logits[j], gold[j]), relerr(lb[j], gold[j])
            print(f"    row {j}: vs reference golden {e_gold:.2e} (fp32), {e_bf:.2e} (bf16 autocast)")
            assert e_gold < 1e-3
            assert e_bf < 3e-2
    assert m.decode_graph_captures == 2                                          # one per autocast state


@pytest.mark.parametrize("cs", [None, 2.5], ids=["plain", "guided"])
def test_long_model_five_candidates_vs_uncached_forward(cs):
    """every candidate teacher-forced with its own random tokens: < 1e-4 in fp32 against the uncached forward on the expanded prompts,
    at kv_splits None and 8"""
    dev = _dev()
    m, text, seg, _ = _long_model(dev)
    n = 5
    img = torch.randint(0, 64, (2 * n, 256), generator=torch.Generator().manual_seed(77)).to(dev)
    te, se = text.repeat_interleave(n, 0), seg.repeat_interleave(n, 0)
    with torch.no_grad():
        full = _uncached(m, te, se, img, cs).cpu()
        for splits in (None, 8):
            toks, logits = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=cs, graph=True, num_samples=n,
                                      share_prompt=True, kv_splits=splits)
            err = relerr(logits, full)
            print(f"long model num_samples={n} kv_splits={splits} cs={cs}: vs uncached forward {err:.2e}")
            assert torch.equal(toks, img) and logits.shape == (2 * n, 256, 64)
            assert err < 1e-4, (splits, err)
    assert {(k[-3], k[-1]) for k in m._decode_graphs} == {(n, 1), (n, 8)}


def test_unshared_paths_are_the_expanded_call_bit_for_bit(golden_dir):
    """share_prompt=False (the default: DESIGN 2.6 has the measurement) and graph=False with num_samples=n: the existing call on
    repeat_interleave'd prompts (the 16-token model: the eager loop costs host time per token)"""
    dev = _dev()
    m, text, seg, _, _ = _golden_model(golden_dir, dev)
    n = 3
    img = torch.randint(0, 96, (2 * n, 16), generator=torch.Generator().manual_seed(78)).to(dev)
    te, se = text.repeat_interleave(n, 0), seg.repeat_interleave(n, 0)
    with torch.no_grad():
        for graph, kw in ((True, dict(share_prompt=False)), (True, {}), (False, {}), (False, dict(share_prompt=True))):
            want = m.generate(te, se, img_tokens=img, return_logits=True, cond_scale=2.0, graph=graph)[1]
            got = m.generate(text, seg, img_tokens=img, return_logits=True, cond_scale=2.0, graph=graph, num_samples=n, **kw)[1]
            assert torch.equal(got, want), (graph, kw)
        for graph, kw in ((True, dict(share_prompt=False)), (False, {})):
            want = m.generate(te, se, temperature=0, graph=graph)
            got = m.generate(text, seg, temperature=0, graph=graph, num_samples=n, **kw)
            assert got.shape == (2 * n, 16) and torch.equal(got, want), (graph, kw)
    assert all(len(k) == 12 for k in m._decode_graphs)                           # no shared entry was made


def test_seeds_keep_and_entry(monkeypatch):
    """seeded sampling repeats and the candidates differ; kept positions are exact; the entry holds image_length own rows and
    [groups, plen, D] prompt blocks; one capture per (num_samples, split counts); a call without num_samples afterwards returns the
    bits it returned before; the replay loop makes no host call"""
    from models import decode_graph
    dev = _dev()
    m, text, seg, img2 = _long_model(dev, seed=31)
    n = 4
    with torch.no_grad():
        plain_before = m.generate(text, seg, img_tokens=img2, return_logits=True, cond_scale=2.0, graph=True)[1]
        base = m.decode_graph_captures
        draw = lambda: m.generate(text, seg, temperature=1.0, top_k=20, cond_scale=2.0, graph=True, num_samples=n,
                                  share_prompt=True, generator=torch.Generator(device=dev).manual_seed(5))
        a = draw()
        assert a.shape == (2 * n, 256) and a.dtype == torch.long and m.decode_graph_captures == base + 1
        assert torch.equal(draw(), a) and m.decode_graph_captures == base + 1   # same seed, same tokens, no recapture
        for b in range(2):
            cand = a[b * n:(b + 1) * n]
            assert not torch.equal(cand, cand[:1].expand_as(cand))               # the candidates of one prompt are not all equal
            assert len({tuple(r.tolist()) for r in cand}) == n

        (key, e), = [(k, v) for k, v in m._decode_graphs.items() if len(k) > 12]
        assert key[-3] == n and key[-1] == 1 and key[-2] == e.prompt_splits >= 1
        plen = m.text_length + m.seg_length
        assert e.group == n and e.rows == 4 * n and len(e.kc) == 2
        assert all(t.shape == (4 * n, m.image_length, 128) for t in e.kc + e.vc)
        assert all(t.shape == (4, plen, 128) for t in e.pk + e.pv)

        # keep: the top half of every candidate's image stays, the rest is sampled
        img = torch.randint(0, 64, (2 * n, 256), generator=torch.Generator().manual_seed(79)).to(dev)
        keep = torch.zeros(2 * n, 256, dtype=torch.bool)
        keep[:, :128] = True
        keep[1::2, 200:210] = True
        kept = m.generate(text, seg, temperature=1.0, top_k=20, cond_scale=2.0, graph=True, num_samples=n, share_prompt=True,
                          img_tokens=img, keep=keep,
                          generator=torch.Generator(device=dev).manual_seed(6))
        kd = keep.to(dev)
        assert torch.equal(kept[kd], img[kd]) and not torch.equal(kept[~kd], img[~kd])
        assert m.decode_graph_captures == base + 2                               # "prompted" is one more configuration
        m.generate(text, seg, temperature=1.0, top_k=20, cond_scale=2.0, graph=True, num_samples=n, share_prompt=True, kv_splits=2,
                   generator=torch.Generator(device=dev).manual_seed(5))
        assert m.decode_graph_captures == base + 3                               # another own split count: another capture
        captures = m.decode_graph_captures

        seen = []
        orig = decode_graph._replay

        def checked(entry, count):
            torch.cuda.set_sync_debug_mode("error")
            try:
                orig(entry, count)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            seen.append((entry.group, count))

        monkeypatch.setattr(decode_graph, "_replay", checked)
        assert torch.equal(draw(), a)
        assert torch.equal(m.generate(text, seg, img_tokens=img2, return_logits=True, cond_scale=2.0, graph=True)[1], plain_before)
    assert seen == [(n, 255), (0, 255)] and m.decode_graph_captures == captures
