"""``MakeAScene.token_loss`` / ``MakeAScene.log_likelihood`` against ``F.cross_entropy(model(...))`` on a two-layer model: the loss and every
parameter gradient (fp32 mode within relative L2 1e-4 -- the bound DESIGN 2.6 uses for the same GEMMs at another row count; bf16 autocast
within the bounds tests/test_gpu_transformer.py uses for bf16 autocast against fp32: loss 1e-2, gradients 6e-2 of their maximum), the
scorer against the logits ``generate`` itself reports, and ``forward`` untouched by any of it."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CFG = dict(num_layers=2, hidden_dim=64, num_attn_heads=4, image_vocab_size=128, seg_vocab_size=40, text_vocab_size=58,
           image_tokens_per_dim=4, seg_tokens_per_dim=2, text_length=8)
B = 2


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from models.transformer import MakeAScene
    from oracle import transformer_oracle as TO
    dev = torch.device("cuda:0")
    m = MakeAScene(**CFG)
    m.load_state_dict(TO.synth_transformer_state_dict(CFG, seed=7), strict=True)
    m = m.to(dev)
    text, seg, img = (t.to(dev) for t in TO.synth_tokens(CFG, batch=B, seed=7))
    # the reference, once: F.cross_entropy on forward()'s logits in fp32 mode, its gradients and its per-token terms
    m.zero_grad(set_to_none=True)
    logits = m(text, seg, img)
    loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), img.reshape(-1))
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    with torch.no_grad():
        per_token = F.cross_entropy(logits.detach().reshape(-1, logits.shape[-1]), img.reshape(-1), reduction="none").view(B, -1)
    m.zero_grad(set_to_none=True)
    return dict(m=m, text=text, seg=seg, img=img, loss=loss.detach().clone(), grads=grads, per_token=per_token,
                logits=logits.detach().clone())


def _l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _maxrel(a, b):
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12))


def test_token_loss_fp32_matches_cross_entropy_of_forward(setup):
    s = setup
    m = s["m"]
    m.zero_grad(set_to_none=True)
    loss = m.token_loss(s["text"], s["seg"], s["img"])
    loss.backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(float(loss) - float(s["loss"])) <= 1e-4 * abs(float(s["loss"]))
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert set(got) == set(s["grads"])
    for k, g in s["grads"].items():
        assert _l2(got[k], g) < 1e-4, (k, _l2(got[k], g))
    m.zero_grad(set_to_none=True)


def test_token_loss_bf16_autocast_matches_fp32(setup):
    s = setup
    m = s["m"]
    m.zero_grad(set_to_none=True)
    seen = []
    from mas_hip import ops
    orig = ops._TokenCrossEntropy.forward

    def spy(ctx, logits, *a):
        seen.append(logits.dtype)
        return orig(ctx, logits, *a)
    ops._TokenCrossEntropy.forward = staticmethod(spy)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = m.token_loss(s["text"], s["seg"], s["img"])
    finally:
        ops._TokenCrossEntropy.forward = staticmethod(orig)
    loss.backward()
    assert seen == [torch.bfloat16] and loss.dtype == torch.float32      # the bf16 logits went in as they were: no cast
    assert abs(float(loss) - float(s["loss"])) < 1e-2 * abs(float(s["loss"]))
    for k, g in s["grads"].items():
        p = dict(m.named_parameters())[k]
        assert p.grad.dtype == torch.float32 and _maxrel(p.grad, g) < 6e-2, (k, _maxrel(p.grad, g))
    m.zero_grad(set_to_none=True)


def test_token_loss_options_follow_cross_entropy(setup):
    s = setup
    m, img = s["m"], s["img"].clone()
    img_ign = img.clone()
    img_ign[0, 3] = -100
    with torch.no_grad():
        got = m.token_loss(s["text"], s["seg"], img, reduction="none", label_smoothing=0.1)
        ref = F.cross_entropy(s["logits"].reshape(-1, 128), img.reshape(-1), reduction="none", label_smoothing=0.1).view(B, -1)
        assert got.shape == ref.shape and float((got - ref).abs().max()) < 1e-4
        # an ignored TARGET (the token is still fed to the model)
        ref_i = F.cross_entropy(s["logits"].reshape(-1, 128), img_ign.reshape(-1), reduction="sum")
        logits = m._image_logits(s["text"], s["seg"], img)
        from mas_hip import ops
        got_i = ops.cross_entropy(logits, img_ign, reduction="sum")
        assert abs(float(got_i) - float(ref_i)) < 1e-4 * abs(float(ref_i))


def test_log_likelihood(setup):
    s = setup
    m = s["m"]
    L = m.image_length
    ll = m.log_likelihood(s["text"], s["seg"], s["img"])
    pt = m.log_likelihood(s["text"], s["seg"], s["img"], per_token=True)
    assert ll.shape == (B,) and ll.dtype == torch.float32 and pt.shape == (B, L) and not ll.requires_grad
    assert torch.equal(pt.sum(1), ll)                                    # per_token sums to the [B] form exactly
    assert float((ll + s["per_token"].sum(1)).abs().max()) <= 1e-4 * L
    assert float((pt + s["per_token"]).abs().max()) <= 1e-4
    # the scorer agrees with the logits generate() drew its own tokens from
    tokens, logits = m.generate(s["text"], s["seg"], temperature=0, return_logits=True)
    want = torch.log_softmax(logits.float(), -1).gather(-1, tokens[..., None])[..., 0].sum(1)
    got = m.log_likelihood(s["text"], s["seg"], tokens)
    assert float((got - want).abs().max()) <= 2e-4 * L, (got, want)
    assert bool((got <= 0).all())


def test_forward_is_bit_identical_around_token_loss(setup):
    s = setup
    m = s["m"]
    with torch.no_grad():
        before = m(s["text"], s["seg"], s["img"])
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.token_loss(s["text"], s["seg"], s["img"]).backward()
    m.log_likelihood(s["text"], s["seg"], s["img"])
    m.zero_grad(set_to_none=True)
    with torch.no_grad():
        after = m(s["text"], s["seg"], s["img"])
    assert torch.equal(before, after)
    assert all(torch.equal(v, state[k]) for k, v in m.state_dict().items())
