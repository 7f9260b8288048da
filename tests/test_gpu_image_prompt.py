"""Image prompts on the MI355X: ``MakeAScene.generate(img_tokens=..., keep=...)`` keeps the chosen image tokens and samples the rest.
The sampler entry ``mas_sample_tokens_prompt`` against torch, the eager and the graph path against each other and against the existing
teacher-forced path bit for bit, the prefix prefill against the step-by-step path within the project's cached-against-uncached bound
(``relerr < 1e-4`` in fp32, 3e-2 against the fp32 forward under bf16 autocast: tests/test_gpu_sampling.py), and that calls without
``keep`` are what they were.  Tiny transformer: 2 layers, head width 16, 4 + 4 prompt tokens, 16 image tokens, 48 image codes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(num_layers=2, hidden_dim=64, num_attn_heads=4, image_vocab_size=48, seg_vocab_size=11, text_vocab_size=40,
           image_tokens_per_dim=4, seg_tokens_per_dim=2, text_length=4)
L = 16
BOUND = 1e-4        # cached against uncached decoding, fp32 (tests/test_gpu_sampling.py)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def relerr(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


_SD = {}


def _model(dev, seed=5):
    """a fresh module (its own graphs and capture count) with seeded weights, and a batch of two prompts with an image to keep from"""
    from models.transformer import MakeAScene
    from oracle import transformer_oracle as TO
    if seed not in _SD:
        _SD[seed] = (TO.synth_transformer_state_dict(CFG, seed=seed), TO.synth_tokens(CFG, batch=2, seed=seed))
    sd, toks = _SD[seed]
    m = MakeAScene(**CFG)
    m.load_state_dict(sd, strict=True)
    text, seg, img = (t.to(dev) for t in toks)
    return m.to(dev).eval(), text, seg, img


def _mask(rows):
    keep = torch.zeros((len(rows), L), dtype=torch.bool)
    for r, cols in enumerate(rows):
        keep[r, list(cols)] = True
    return keep


SCATTERED = _mask([{1, 5}, {0, 2}])                                         # no common prefix
PREFIX5 = _mask([set(range(5)) | {9}, set(range(7)) | {12}])                # common prefix 5


def _autocast(on):
    return torch.autocast("cuda", dtype=torch.bfloat16) if on else torch.autocast("cuda", enabled=False)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("v", [40, 300])            # smaller than the work-group of 256; not a multiple of it
@pytest.mark.parametrize("cs", [None, 2.0], ids=["plain", "guided"])
def test_kernel_against_torch(v, cs):
    from mas_hip import decode
    from models import common_prefix
    assert common_prefix(SCATTERED) == 0 and common_prefix(PREFIX5) == 5
    dev = _dev()
    b, length, k = 3, 4, 2
    g = torch.Generator().manual_seed(v)
    logits = (torch.randn((2 * b if cs is not None else b, v), generator=g) * 2).to(dev)
    mixed = logits[b:] + cs * (logits[:b] - logits[b:]) if cs is not None else logits
    forced = torch.randint(0, v, (b, length), generator=g).to(dev)
    keep = torch.zeros((b, length), dtype=torch.uint8, device=dev)
    keep[1, k] = 1                                  # row 1 is kept at this step
    keep[0, k - 1] = keep[2, k + 1] = 1             # other steps of the free rows: not this step's business
    step = torch.full((1,), k, dtype=torch.int32, device=dev)
    seed = torch.tensor([12345, 678], dtype=torch.int64, device=dev)

    def run(mode, params, with_keep, **kw):
        tokens = torch.full((b, length), -1, dtype=torch.long, device=dev)
        lout = torch.full((b, length, v), float("nan"), device=dev)
        decode.sample_tokens(logits, tokens, step, torch.tensor(params, dtype=torch.float32, device=dev), mode, guided=cs is not None,
                             seed=seed, forced=forced if with_keep else None, logits_out=lout, keep=keep if with_keep else None, **kw)
        assert (tokens[:, [0, 1, 3]] == -1).all() and torch.isnan(lout[:, [0, 1, 3]]).all()      # one step, one column
        return tokens[:, k], lout[:, k]

    tok, lout = run(decode.GREEDY, [1.0, cs or 0.0, 1.0], True)
    want = mixed.argmax(dim=-1)
    want[1] = forced[1, k]
    assert torch.equal(tok, want)
    assert torch.equal(lout, mixed)                 # written for the kept row too
    params = [0.8, cs or 0.0, 0.7]
    base, _ = run(decode.SAMPLE, params, False, top_k=10, top_p=True)
    tok, lout = run(decode.SAMPLE, params, True, top_k=10)
    assert tok[1] == forced[1, k] and torch.equal(tok[[0, 2]], base[[0, 2]])
    assert torch.equal(lout, mixed)


# ------------------------------------------------------------------------------------------------------------------------------- model
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_kept_positions_are_returned_exactly(graph):
    dev = _dev()
    m, text, seg, img = _model(dev)
    with torch.no_grad():
        for kw in (dict(temperature=0), dict(temperature=0.9, top_k=8, top_p=0.9, generator=_gen(dev, 3))):
            tok = m.generate(text, seg, img_tokens=img, keep=SCATTERED, graph=graph, **kw)
            assert tok.shape == (2, L) and tok.dtype == torch.long and int(tok.min()) >= 0 and int(tok.max()) < 48
            assert torch.equal(tok[SCATTERED.to(dev)], img[SCATTERED.to(dev)]), kw
    # the free positions are sampled, not copied: greedy tokens do not depend on what img_tokens holds there
    with torch.no_grad():
        other = torch.where(SCATTERED.to(dev), img, (img + 7) % 48)
        a = m.generate(text, seg, img_tokens=img, keep=SCATTERED, temperature=0, graph=graph)
        b = m.generate(text, seg, img_tokens=other, keep=SCATTERED, temperature=0, graph=graph)
    assert torch.equal(a, b)


def test_greedy_is_self_consistent_exactly():
    dev = _dev()
    m, text, seg, img = _model(dev)
    free = ~SCATTERED.to(dev)
    with torch.no_grad():
        t, lg = m.generate(text, seg, img_tokens=img, keep=SCATTERED, temperature=0, prefill_prefix=False, return_logits=True)
        t2, forced = m.generate(text, seg, img_tokens=t, return_logits=True)            # the existing teacher-forced path
    assert torch.equal(t2, t)
    assert torch.equal(forced.argmax(dim=-1)[free], t[free])
    assert torch.equal(lg, forced)


@pytest.mark.parametrize("case", ["fp32", "bf16", "guided", "prefix"])
def test_eager_and_graph_agree_bit_for_bit(case):
    dev = _dev()
    m, text, seg, img = _model(dev)
    keep = PREFIX5 if case == "prefix" else SCATTERED
    kw = dict(img_tokens=img, keep=keep, temperature=0, return_logits=True, cond_scale=3.0 if case == "guided" else None,
              prefill_prefix=case == "prefix")
    with torch.no_grad(), _autocast(case == "bf16"):
        te, le = m.generate(text, seg, **kw)
        tg, lg = m.generate(text, seg, graph=True, **kw)
    assert m.decode_graph_captures == 1
    assert le.shape == lg.shape == (2, L, 48) and lg.dtype == torch.float32
    assert torch.equal(tg, te)
    assert torch.equal(lg, le), f"graph vs eager logits: max rel {relerr(lg, le):.3e}"
    assert torch.equal(tg[keep.to(dev)], img[keep.to(dev)])


def test_first_call_on_a_fresh_module_with_a_prefix(monkeypatch):
    """the warm-up step of the capture runs at step m + 1: the rewind behind it has to go there, not to step 1"""
    from models import decode_graph
    dev = _dev()
    m, text, seg, img = _model(dev)
    replays = []
    orig = decode_graph._replay
    monkeypatch.setattr(decode_graph, "_replay", lambda e, n: (replays.append(n), orig(e, n))[1])
    kw = dict(img_tokens=img, temperature=0, return_logits=True)
    with torch.no_grad():
        tg, lg = m.generate(text, seg, keep=PREFIX5, graph=True, **kw)               # the first call this module sees
        assert m.decode_graph_captures == 1 and replays == [L - 1 - 5]
        te, le = m.generate(text, seg, keep=PREFIX5, graph=False, **kw)
        assert torch.equal(tg, te) and torch.equal(lg, le)
        del replays[:]
        ta, la = m.generate(text, seg, keep=torch.ones((2, L), dtype=torch.bool), graph=True, **kw)      # m = L - 1
        assert torch.equal(ta, img) and sum(replays) == 0
        ea, ela = m.generate(text, seg, keep=torch.ones((2, L), dtype=torch.bool), graph=False, **kw)
        assert torch.equal(ea, img) and torch.equal(la, ela)
        t0, l0 = m.generate(text, seg, keep=SCATTERED, graph=True, **kw)             # m = 0
        e0, el0 = m.generate(text, seg, keep=SCATTERED, graph=False, **kw)
        assert torch.equal(t0, e0) and torch.equal(l0, el0) and replays[-1] == L - 1
        assert m.decode_graph_captures == 1
        other = (img + 11) % 48
        keep4 = _mask([{0, 1, 2, 8}, {0, 1, 2, 3, 15}])                              # m = 3, other kept tokens
        t4, l4 = m.generate(text, seg, keep=keep4, graph=True, img_tokens=other, temperature=0, return_logits=True)
        e4, el4 = m.generate(text, seg, keep=keep4, graph=False, img_tokens=other, temperature=0, return_logits=True)
        assert m.decode_graph_captures == 1 and replays[-1] == L - 1 - 3
        assert torch.equal(t4, e4) and torch.equal(l4, el4) and torch.equal(t4[keep4.to(dev)], other[keep4.to(dev)])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_all_true_mask_step_by_step_is_teacher_forcing(graph):
    dev = _dev()
    m, text, seg, img = _model(dev)
    with torch.no_grad():
        t, lg = m.generate(text, seg, img_tokens=img, keep=torch.ones((2, L), dtype=torch.bool), prefill_prefix=False,
                           return_logits=True, graph=graph)
        t0, lg0 = m.generate(text, seg, img_tokens=img, return_logits=True, graph=graph)
    assert torch.equal(t, img) and torch.equal(t0, img) and torch.equal(lg, lg0)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_prefix_prefill_against_step_by_step_fp32(graph):
    """the prefill kernel and the decode kernel sum in different orders: the logits agree within the cached-against-uncached bound, and
    the greedy tokens are equal because no top-two gap of the step-by-step run is within reach of that bound.  |l_on - l_off| <= BOUND *
    max|l_off| for every entry, so the order of two entries can change only when they are closer than twice that."""
    dev = _dev()
    m, text, seg, img = _model(dev)
    kw = dict(img_tokens=img, keep=PREFIX5, temperature=0, return_logits=True, graph=graph)
    with torch.no_grad():
        t_on, l_on = m.generate(text, seg, prefill_prefix=True, **kw)
        t_off, l_off = m.generate(text, seg, prefill_prefix=False, **kw)
    err = relerr(l_on, l_off)
    top2 = l_off.topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1])[~PREFIX5.to(dev)].min())
    reach = 2 * BOUND * float(l_off.abs().max())
    print(f"prefix prefill vs step-by-step: relerr {err:.3e} (bound {BOUND}), smallest free top-two gap {gap:.3e} (reach {reach:.3e})")
    assert err < BOUND
    assert gap > reach, "pick another seed: a near-tie could hide a failure"
    assert torch.equal(t_on, t_off)


def test_prefix_prefill_and_step_by_step_under_bf16_autocast():
    dev = _dev()
    m, text, seg, img = _model(dev)
    kw = dict(img_tokens=img, keep=PREFIX5, temperature=0, return_logits=True)
    for on in (True, False):
        with torch.no_grad():
            with _autocast(True):
                t, lg = m.generate(text, seg, prefill_prefix=on, **kw)
            full = m(text, seg, t)                                                   # fp32, uncached, fed the run's own tokens
        err = relerr(lg, full)
        print(f"bf16 prefill_prefix={on}: vs fp32 uncached forward {err:.3e}")
        assert err < 3e-2, on
        assert torch.equal(t[PREFIX5.to(dev)], img[PREFIX5.to(dev)])


def test_sampled_graph_is_seeded_and_its_replay_loop_makes_no_host_call(monkeypatch):
    from models import decode_graph
    dev = _dev()
    m, text, seg, img = _model(dev)
    free = ~PREFIX5.to(dev)
    kw = dict(img_tokens=img, keep=PREFIX5, temperature=1.0, top_k=16, top_p=0.95, cond_scale=2.0, graph=True)      # keep: a CPU tensor
    seen = []
    orig = decode_graph._replay

    def checked(e, n):
        torch.cuda.set_sync_debug_mode("error")
        try:
            orig(e, n)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        seen.append(n)

    with torch.no_grad():
        a = m.generate(text, seg, generator=_gen(dev, 5), **kw)
        monkeypatch.setattr(decode_graph, "_replay", checked)
        b = m.generate(text, seg, generator=_gen(dev, 5), **kw)
        c = m.generate(text, seg, generator=_gen(dev, 6), **kw)
    assert seen == [L - 1 - 5] * 2 and m.decode_graph_captures == 1
    assert torch.equal(a, b)
    assert not torch.equal(a[free], c[free])
    for t in (a, c):
        assert torch.equal(t[~free], img[~free])


@pytest.mark.parametrize("mode", ["greedy", "sampled", "forced"])
def test_off_is_off(mode):
    dev = _dev()
    m, text, seg, img = _model(dev)
    kw = dict(greedy=dict(temperature=0), sampled=dict(temperature=0.9, top_k=12), forced=dict(img_tokens=img))[mode]
    run = lambda **more: m.generate(text, seg, return_logits=True, graph=True, **dict(kw, **more),
                                    **(dict(generator=_gen(dev, 9)) if mode == "sampled" else {}))
    with torch.no_grad():
        t0, l0 = run()
        assert m.decode_graph_captures == 1
        tp, _ = run(img_tokens=img, keep=PREFIX5)
        n = m.decode_graph_captures
        t1, l1 = run()
        assert m.decode_graph_captures == n == 2                                     # its own entry; the unprompted one is still there
    assert torch.equal(t1, t0) and torch.equal(l1, l0)
    assert torch.equal(tp[PREFIX5.to(dev)], img[PREFIX5.to(dev)])


def test_validation_leaves_the_graphs_alone():
    dev = _dev()
    m, text, seg, img = _model(dev)
    with torch.no_grad():
        m.generate(text, seg, img_tokens=img, keep=SCATTERED, temperature=0, graph=True)
        n = m.decode_graph_captures
        for kw in (dict(keep=SCATTERED), dict(img_tokens=img, keep=SCATTERED[:, :15]), dict(img_tokens=img, keep=SCATTERED[:1]),
                   dict(img_tokens=img, keep=SCATTERED.float()), dict(img_tokens=img, keep=SCATTERED.to(dev).to(torch.uint8))):
            for graph in (True, False):
                with pytest.raises(ValueError):
                    m.generate(text, seg, temperature=0, graph=graph, **kw)
    assert m.decode_graph_captures == n == 1
