"""Training with dropout: attention dropout inside the flash kernels (``mas_attn_causal_fwd_drop`` / ``_bwd_drop``) and ResnetBlock's
element-wise dropout (``mas_dropout_apply``).  Masks against the numpy restatement (tests/helpers/philox_ref.py), fused attention
against an fp32 oracle built from the reference's score formula with the materialised mask, statistics, seeding, checkpoint replay,
and that nothing [S, S] is stored."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import philox_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {torch.float32: 2e-4, torch.bfloat16: 3e-2}          # those of tests/test_gpu_transformer.py::test_causal_attention_vs_oracle


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def relerr(got, ref):
    got = got.detach().float().cpu()
    ref = torch.as_tensor(ref).float()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


@pytest.fixture(autouse=True)
def _restore_dtype():
    from mas_hip import ops
    old = ops.compute_dtype()
    yield
    ops.set_compute_dtype(old)


def attn_mask(seed, B, H, S, p):
    """[B, H, S, S] uint8 keep mask from the library's own mask kernel"""
    import mas_hip
    from mas_hip import ops
    keep = torch.empty((B, H, S, S), dtype=torch.uint8, device=seed.device)
    mas_hip.check(mas_hip.lib().mas_attn_dropout_mask(ops._ptr(seed), B, H, S, float(p), ops._ptr(keep), ops._stream()), "attn_dropout_mask")
    return keep


# --------------------------------------------------------------------------- #
# the two layers that raised before
# --------------------------------------------------------------------------- #
def test_transformer_layer_with_attention_dropout_trains():
    from models.transformer import TransformerLayer
    dev = _dev()
    torch.manual_seed(0)
    layer = TransformerLayer(64, 4, attn_dropout_prop=0.1, out_dropout_prob=0.0).to(dev).train()
    x = torch.randn(2, 40, 64, device=dev, requires_grad=True)
    y = layer(x, None)[0]
    y.square().mean().backward()
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert all(torch.isfinite(p.grad).all() for p in layer.parameters() if p.grad is not None)
    with torch.no_grad():
        y_eval = layer.eval()(x, None)[0]
    assert (y - y_eval).abs().max() > 1e-3                  # dropout acted in training, not in eval


def test_resnet_block_with_dropout_trains():
    from models.modules import ResnetBlock
    dev = _dev()
    torch.manual_seed(0)
    blk = ResnetBlock(in_channels=64, out_channels=128, dropout=0.1).to(dev).train()
    x = torch.randn(2, 64, 16, 16, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = blk(x)
    y.float().square().mean().backward()
    assert y.shape == (2, 128, 16, 16) and torch.isfinite(y.float()).all() and torch.isfinite(x.grad.float()).all()
    assert all(torch.isfinite(p.grad).all() for p in blk.parameters() if p.grad is not None)


# --------------------------------------------------------------------------- #
# masks, bit for bit
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("B,H,S,p", [(1, 1, 8, 0.5), (2, 3, 37, 0.1), (1, 2, 130, 0.9)])
def test_attention_mask_equals_restatement(B, H, S, p):
    from mas_hip import ops
    dev = _dev()
    torch.manual_seed(B * 100 + S)
    seed = ops.drop_seed(dev)
    sd, off = (int(v) for v in seed.cpu())
    got = attn_mask(seed, B, H, S, p).cpu().numpy().astype(bool)
    assert (got == R.attention_keep(sd, off, B, H, S, p)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [8, 1000, 4099])
def test_elementwise_mask_equals_restatement(dtype, n):
    from mas_hip import ops
    dev = _dev()
    p = 0.3
    seed = ops.drop_seed(dev)
    sd, off = (int(v) for v in seed.cpu())
    x = torch.randn(n, device=dev).to(dtype)
    y = ops._dropout_apply(x, p, seed)
    want = torch.from_numpy(R.elementwise_keep(sd, off, n, p))
    sc = R.scale(R.threshold(p))
    ref = torch.where(want, x.float().cpu() * sc, torch.zeros(()))
    assert torch.equal(y.cpu(), ref.to(dtype))


# --------------------------------------------------------------------------- #
# fused attention against the fp32 oracle with the materialised mask
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 4, 24, 16), (1, 3, 130, 32), (2, 2, 333, 64), (2, 16, 1536, 64), (2, 2, 200, 128), (1, 3, 77, 48)])
def test_attention_dropout_vs_oracle(shape, dtype, p):
    from mas_hip import ops
    from oracle import transformer_oracle as TO
    dev = _dev()
    b, h, s, hd = shape
    d = h * hd
    rs = np.random.RandomState(b * 1000 + s)
    qkv = torch.from_numpy(rs.randn(b, s, 3 * d).astype(np.float32))
    if dtype == torch.bfloat16:
        qkv = qkv.bfloat16().float()
    go = torch.from_numpy(rs.randn(b, s, d).astype(np.float32))
    torch.manual_seed(s)
    x = qkv.clone().to(dev).requires_grad_(True)
    out = ops.causal_attention(x, h, dtype=dtype, dropout_p=p)
    out.backward(go.to(dev))
    torch.manual_seed(s)                                     # the same draw the op made
    seed = ops.drop_seed(dev)
    z = attn_mask(seed, b, h, s, p).cpu().float() * R.scale(R.threshold(p))
    ref_in = qkv.clone().requires_grad_(True)
    q, k, v = (t.view(b, s, h, hd).permute(0, 2, 1, 3) for t in torch.split(ref_in, d, dim=-1))
    mask = torch.tril(torch.ones(s, s))[None, None]
    probs = torch.softmax(TO.causal_attention_scores(q, k, mask, hd), dim=-1)
    ref = torch.matmul(probs * z, v).permute(0, 2, 1, 3).reshape(b, s, d)
    ref.backward(go)
    assert relerr(out, ref) < TOL[dtype]
    assert relerr(x.grad, ref_in.grad) < 2 * TOL[dtype]


def test_attention_dropout_edge_cases():
    from mas_hip import ops
    dev = _dev()
    x = torch.randn(1, 70, 3 * 4 * 64, device=dev).bfloat16().requires_grad_(True)
    torch.manual_seed(1)
    y1 = ops.causal_attention(x, 4, dropout_p=1.0)             # p = 1: zeros, zero gradient
    y1.float().sum().backward()
    assert (y1 == 0).all() and (x.grad == 0).all()
    state = torch.cuda.get_rng_state()
    y0 = ops.causal_attention(x, 4, dropout_p=0.0)             # p = 0: the plain kernels, nothing drawn
    assert torch.equal(torch.cuda.get_rng_state(), state)
    assert torch.equal(y0, ops.causal_attention(x, 4))


# --------------------------------------------------------------------------- #
# statistics and seeding
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction_and_independence(p):
    from mas_hip import ops
    dev = _dev()
    B, H, S = 2, 4, 1200                                     # 11.5 M scores
    torch.manual_seed(3)
    s1, s2 = ops.drop_seed(dev), ops.drop_seed(dev)
    m = attn_mask(s1, B, H, S, p)
    q = 1.0 - R.threshold(p) / 65536.0
    n = m.numel()
    frac = float(m.double().mean())
    assert abs(frac - q) < 6 * np.sqrt(q * (1 - q) / n), (frac, q)
    diff = lambda a, b: float((a != b).double().mean())
    assert diff(m[0, 0], m[0, 1]) > 0.5 * 2 * q * (1 - q) and diff(m[0, 0], m[1, 0]) > 0.5 * 2 * q * (1 - q)
    assert diff(m, attn_mask(s2, B, H, S, p)) > 0.9 * 2 * q * (1 - q)          # a new call, a new mask


def test_manual_seed_reproduces_and_checkpoint_replays():
    from models.transformer import SelfAttention
    from mas_hip import ops
    dev = _dev()
    x0 = torch.randn(2, 96, 3 * 4 * 32, device=dev)

    def run():
        x = x0.clone().requires_grad_(True)
        torch.manual_seed(11)
        y = ops.causal_attention(x, 4, dropout_p=0.2)
        y.square().sum().backward()
        return y.detach(), x.grad
    (ya, ga), (yb, gb) = run(), run()
    assert torch.equal(ya, yb) and torch.equal(ga, gb)

    torch.manual_seed(0)
    att = SelfAttention(128, 4, attn_dropout_prob=0.2, out_dropout_prob=0.0).to(dev).train()
    xin = torch.randn(2, 96, 128, device=dev)

    def grads(ckpt):
        att.zero_grad(set_to_none=True)
        x = xin.clone().requires_grad_(True)
        torch.manual_seed(5)
        f = lambda t: att(t, None)[0]
        y = torch.utils.checkpoint.checkpoint(f, x, use_reentrant=False) if ckpt else f(x)
        y.square().sum().backward()
        return [x.grad] + [p.grad.clone() for p in att.parameters()]
    plain, ck = grads(False), grads(True)
    assert all(torch.equal(a, b) for a, b in zip(plain, ck))


def test_no_score_sized_memory():
    from mas_hip import ops
    dev = _dev()
    B, H, S, hd = 2, 16, 1536, 64
    x0 = torch.randn(B, S, 3 * H * hd, device=dev).bfloat16()
    go = torch.randn(B, S, H * hd, device=dev).bfloat16()

    def peak(p):
        x = x0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ops.causal_attention(x, H, dropout_p=p).backward(go)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    p0, p1 = peak(0.0), peak(0.1)
    assert p1 - p0 < B * H * S * S, (p0, p1)


# --------------------------------------------------------------------------- #
# ResnetBlock with dropout against an fp32 restatement
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128)])
def test_resnet_block_dropout_vs_oracle(dtype, cin, cout):
    from models.modules import ResnetBlock
    from mas_hip import ops
    from oracle import vq_oracle as O
    dev = _dev()
    ops.set_compute_dtype(dtype)
    torch.manual_seed(0)
    blk = ResnetBlock(in_channels=cin, out_channels=cout, dropout=0.3)
    with torch.no_grad():
        for prm in blk.parameters():                             # non-trivial affine GroupNorm parameters
            if prm.dim() == 1:
                prm.add_(0.1 * torch.randn_like(prm))
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    if dtype == torch.bfloat16:
        sd = {k: (v.bfloat16().float() if k.endswith("weight") and v.dim() == 4 else v) for k, v in sd.items()}
    blk = blk.to(dev).train()
    xc = torch.randn(2, cin, 16, 16)
    if dtype == torch.bfloat16:
        xc = xc.bfloat16().float()
    x = xc.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    go = torch.randn(2, cout, 16, 16)
    torch.manual_seed(9)
    y = blk(x)
    y.float().backward(go.to(dev))
    torch.manual_seed(9)                                         # the one draw of the forward: ops.dropout's seed
    ones = torch.ones(2, cout, 16, 16, device=dev, dtype=dtype).contiguous(memory_format=torch.channels_last)
    zs = ops.dropout(ones, 0.3).float().cpu()
    assert set(torch.unique(zs).tolist()) <= {0.0, R.scale(R.threshold(0.3))} or dtype == torch.bfloat16
    xr = xc.clone().requires_grad_(True)
    h = O.conv(sd, "conv1", O.swish(O.group_norm(sd, "norm1", xr)), padding=1)
    a = O.swish(O.group_norm(sd, "norm2", h)) * zs
    sc = xr if cin == cout else O.conv(sd, "nin_shortcut", xr)
    ref = O.conv(sd, "conv2", a, padding=1) + sc
    ref.backward(go)
    tol = 2e-3 if dtype == torch.float32 else 3e-2
    assert relerr(y, ref) < tol
    assert relerr(x.grad, xr.grad) < 2 * tol
