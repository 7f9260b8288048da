"""The AttnBlock core beyond 256 tokens on the chunked kernels (``mas_spatial_attn_flash_fwd / _bwd``: online softmax over 256-key
chunks) against torch fp32 on the CPU: forward and the gradient w.r.t. the fused q|k|v projection at the 512x512 model's 32x32x512
block, at the chunk / tile edges and at both ends of the envelope; softmax inputs that move the running maximum at every chunk or
underflow every chunk but the first; bit-for-bit repeatability; the switch and the dispatch of ``ops.spatial_attention``; a narrow
VQBASE whose AttnBlocks see 400 tokens.  Tolerances: those of tests/test_gpu_spatial_attn.py (the bf16 kernels' yardstick)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_MAX, FWD_L2, GRAD_L2, GRAD_MAX = 2e-2, 1e-2, 2e-2, 4e-2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel_l2(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-12))


def relmax(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


@contextlib.contextmanager
def _flash(on):
    from mas_hip import ops
    old = ops.set_spatial_flash(on)
    try:
        yield
    finally:
        ops.set_spatial_flash(old)


@contextlib.contextmanager
def _counting(cls):
    """counts the calls of an autograd Function's forward"""
    calls = []
    orig = cls.forward
    cls.forward = staticmethod(lambda ctx, a, b: (calls.append(1), orig(ctx, a, b))[1])
    try:
        yield calls
    finally:
        cls.forward = staticmethod(orig)


def _reference(qkv, go, c):
    """torch fp32 on the CPU, as in tests/test_gpu_spatial_attn.py: (out, d qkv, lse)"""
    n, c3, h, w = qkv.shape
    ref_in = qkv.float().requires_grad_(True)
    t = ref_in.permute(0, 2, 3, 1).reshape(n, h * w, 3 * c)
    q, k, v = t[..., :c], t[..., c:2 * c], t[..., 2 * c:]
    s = torch.bmm(q, k.transpose(1, 2)) * (c ** -0.5)
    ref = torch.bmm(torch.softmax(s, dim=2), v).reshape(n, h, w, c).permute(0, 3, 1, 2)
    ref.backward(go.float())
    return ref.detach(), ref_in.grad, torch.logsumexp(s.detach(), dim=2)


def _inputs(case, seed=None):
    n, c, h, w = case
    g = torch.Generator().manual_seed(c + h if seed is None else seed)
    qkv = (torch.randn(n, 3 * c, h, w, generator=g) * 1.5).bfloat16()
    go = torch.randn(n, c, h, w, generator=g).bfloat16()
    return qkv, go


def _on_gpu(qkv, dev):
    return qkv.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)


def _check(tag, y, dx, ref, dref):
    f_max, f_l2, g_l2, g_max = relmax(y, ref), rel_l2(y, ref), rel_l2(dx, dref), relmax(dx, dref)
    print(f"{tag}: fwd rel-L2 {f_l2:.2e} max {f_max:.2e}; dqkv rel-L2 {g_l2:.2e} max {g_max:.2e}")
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert f_max < FWD_MAX and f_l2 < FWD_L2
    assert g_l2 < GRAD_L2 and g_max < GRAD_MAX


CASES = [
    # n, c, h, w
    (1, 64, 1, 257),      # first S past the old envelope: one full 256-key chunk plus one key, ragged last query block
    (2, 64, 16, 18),      # 288: one chunk plus one 32-key tile
    (2, 512, 32, 32),     # 1024: the AttnBlock of conf/img_config.yaml at 512x512
    (1, 512, 32, 33),     # 1056: ragged past it
    (1, 160, 24, 24),     # 576: channel groups partly full
    (8, 64, 16, 20),      # 320; 80 blocks, a multiple of 8: the XCD remap taken
    (3, 64, 16, 20),      # 320; 30 blocks: the XCD remap not taken
    (1, 32, 64, 64),      # 4096: the far end of the envelope, cheap at C = 32
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_flash_fwd_bwd_vs_torch(case):
    from mas_hip import ops
    n, c, h, w = case
    dev = _dev()
    qkv, go = _inputs(case)
    ref, dref, _ = _reference(qkv, go, c)
    x = _on_gpu(qkv, dev)
    with _flash(True), _counting(ops._SpatialAttentionFlash) as calls:
        y = ops.spatial_attention(x, c)
    assert calls, "the chunked HIP kernel was not dispatched"
    y.backward(go.to(dev))
    assert y.shape == (n, c, h, w) and y.dtype == torch.bfloat16
    _check(str(case), y, x.grad, ref, dref)


def test_one_chunk_loop_through_the_function():
    """16 tokens: inside the shipped kernel's envelope, so the dispatcher never sends it here -- the Function is called directly"""
    from mas_hip import ops
    case = (1, 96, 4, 4)
    dev = _dev()
    qkv, go = _inputs(case)
    ref, dref, _ = _reference(qkv, go, 96)
    x = _on_gpu(qkv, dev)
    with _counting(ops._SpatialAttentionFlash) as calls:
        y = ops._SpatialAttentionFlash.apply(x, 96)
    assert calls
    y.backward(go.to(dev))
    _check(str(case), y, x.grad, ref, dref)


@pytest.mark.parametrize("where", ["last", "first"])
def test_hard_softmax_inputs(where):
    """(1, 64, 20, 20): 400 tokens = two key chunks (256 + 144).  Logits reach +-60.  'last': every row's largest score lies in the
    last chunk in memory order, 'first': in the first, and the other chunk's exponentials underflow to 0 against it.  (A block may walk
    the chunks in either order: between the two variants every block sees its maximum rise at the second chunk and sees the second
    chunk vanish.)"""
    import mas_hip
    from mas_hip import ops
    n, c, h, w = 1, 64, 20, 20
    s = h * w
    dev = _dev()
    g = torch.Generator().manual_seed(7 if where == "last" else 8)
    u = torch.randn(c, generator=g)
    u = u / u.norm()
    # q = a u + noise, k = b_j u + noise: logits = a b_j / 8 + small.  a = 24; b_j = +20 at one key of the chosen chunk (logit +60),
    # within +-6 at its other keys; the OTHER chunk's keys have b_j in [-20, -12] (logits -60 .. -36, one of them -60): against the
    # row maximum their exponentials are exp(-96) and less, 0 in fp32.
    b = (torch.rand(s, generator=g) * 2 - 1) * 6
    hot, cold = (300, 100) if where == "last" else (100, 300)
    other = slice(0, 256) if where == "last" else slice(256, s)
    b[other] = -12.0 - 8.0 * torch.rand(s, generator=g)[other]
    b[hot], b[cold] = 20.0, -20.0
    q = 24.0 * u[None, :] + 0.3 * torch.randn(s, c, generator=g)
    k = b[:, None] * u[None, :] + 0.3 * torch.randn(s, c, generator=g)
    v = torch.randn(s, c, generator=g)
    qkv = torch.cat([q, k, v], dim=1).t().reshape(1, 3 * c, h, w).bfloat16()
    go = torch.randn(n, c, h, w, generator=g).bfloat16()
    ref, dref, ref_lse = _reference(qkv, go, c)
    t = qkv.float().permute(0, 2, 3, 1).reshape(1, s, 3 * c)
    logits = torch.bmm(t[..., :c], t[..., c:2 * c].transpose(1, 2)) * (c ** -0.5)
    print(f"{where}: logits in [{float(logits.min()):.1f}, {float(logits.max()):.1f}]")
    assert float(logits.max()) > 55 and float(logits.min()) < -55
    assert bool((logits.argmax(dim=2) == hot).all())
    x = _on_gpu(qkv, dev)
    with _flash(True), _counting(ops._SpatialAttentionFlash) as calls:
        y = ops.spatial_attention(x, c)
    assert calls
    y.backward(go.to(dev))
    _check(where, y, x.grad, ref, dref)
    # the log-sum-exp itself, from the C entry
    xin = x.detach()
    o = torch.empty_like(y)
    lse = torch.empty((n, s), dtype=torch.float32, device=dev)
    mas_hip.check(mas_hip.lib().mas_spatial_attn_flash_fwd(xin.data_ptr(), o.data_ptr(), lse.data_ptr(), mas_hip.BF16, n, s, c,
                                                           torch.cuda.current_stream().cuda_stream), "flash_fwd")
    err = float((lse.cpu() - ref_lse).abs().max())
    print(f"{where}: lse max abs error {err:.2e}")
    assert torch.equal(o, y.detach()) and err < 1e-3


def test_second_run_gives_equal_bits():
    from mas_hip import ops
    case = (2, 512, 32, 32)
    dev = _dev()
    qkv, go = _inputs(case)
    outs = []
    with _flash(True):
        for _ in range(2):
            x = _on_gpu(qkv, dev)
            y = ops.spatial_attention(x, 512)
            y.backward(go.to(dev))
            outs.append((y.detach(), x.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_agrees_with_the_shipped_kernel_at_256_tokens():
    """not bit for bit: P is rounded to bf16 before the normalisation here and after it there"""
    from mas_hip import ops
    case = (2, 256, 16, 16)
    dev = _dev()
    qkv, go = _inputs(case)
    xa, xb = _on_gpu(qkv, dev), _on_gpu(qkv, dev)
    ya = ops._SpatialAttentionFlash.apply(xa, 256)
    ya.backward(go.to(dev))
    yb = ops._SpatialAttention.apply(xb, 256)
    yb.backward(go.to(dev))
    _check("flash vs shipped", ya, xa.grad, yb, xb.grad)


def test_switch_off_is_the_library_path():
    from mas_hip import ops
    case = (1, 64, 32, 32)
    dev = _dev()
    qkv, go = _inputs(case)
    x = _on_gpu(qkv, dev)
    with _flash(False), _counting(ops._SpatialAttentionFlash) as calls:
        y = ops.spatial_attention(x, 64)
    assert not calls
    t = x.detach().permute(0, 2, 3, 1).reshape(1, 1024, 192)
    lib = torch.bmm(torch.softmax(torch.bmm(t[..., :64], t[..., 64:128].transpose(1, 2)) * (64 ** -0.5), dim=2), t[..., 128:])
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(1, 1024, 64), lib)
    with _flash(False):
        assert ops.set_spatial_flash(True) is False and ops.set_spatial_flash(False) is True


def test_fp32_keeps_the_library_path():
    from mas_hip import ops
    dev = _dev()
    x = torch.randn(1, 96, 32, 32, device=dev).contiguous(memory_format=torch.channels_last)
    with _flash(True), _counting(ops._SpatialAttentionFlash) as calls:
        y = ops.spatial_attention(x, 32)
    assert not calls and y.dtype == torch.float32 and y.shape == (1, 32, 32, 32)


@pytest.mark.parametrize("on", [True, False])
def test_256_tokens_stay_on_the_shipped_kernel(on):
    from mas_hip import ops
    dev = _dev()
    qkv, _ = _inputs((1, 64, 16, 16))
    x = qkv.to(dev).contiguous(memory_format=torch.channels_last)
    with _flash(on), _counting(ops._SpatialAttentionFlash) as new, _counting(ops._SpatialAttention) as old:
        ops.spatial_attention(x, 64)
    assert old and not new


def test_no_grad_forward_equals_the_grad_enabled_one():
    from mas_hip import ops
    dev = _dev()
    qkv, _ = _inputs((2, 128, 24, 24))
    with _flash(True), _counting(ops._SpatialAttentionFlash) as calls:
        with torch.no_grad():
            a = ops.spatial_attention(qkv.to(dev).contiguous(memory_format=torch.channels_last), 128)
        b = ops.spatial_attention(_on_gpu(qkv, dev), 128)
    assert len(calls) == 2 and torch.equal(a, b.detach())


def test_narrow_model_with_400_token_attention_vs_oracle():
    """VQBASE with AttnBlocks on a 20x20 map of 64 channels, bf16 compute, forward + backward vs the oracle: the yardsticks of
    tests/test_gpu_model.py::test_odd_input_size_batch_and_attention_placement_vs_oracle[bf16] (4e-2 on z and on the decoder fed the
    oracle's z_q, finite gradients)."""
    from models import VQBASE
    from mas_hip import ops
    from oracle import vq_oracle as O
    dev = _dev()
    tol = 4e-2
    cfg = dict(ddconfig=dict(z_channels=32, in_channels=3, out_channels=3, channels=[32, 32, 64], num_res_blocks=1, resolution=40,
                             attn_resolutions=[20], dropout=0.0), n_embed=48, embed_dim=32, init_steps=3000, reservoir_size=12500)
    sd = O.synth_state_dict(cfg["ddconfig"], 48, 32, seed=11)
    x = O.synth_image_batch(2, 3, 40, seed=11)
    taps = {}
    with torch.no_grad():
        ref, ref_q, ref_idx, ref_z = O.vqbase_forward(sd, x, cfg["ddconfig"], training=True, taps=taps)

    def relerr(got, want):
        got, want = got.detach().float().cpu(), want.detach().float()
        assert got.shape == want.shape
        return float((got - want).abs().max() / (want.abs().max() + 1e-12))

    old = ops.compute_dtype()
    ops.set_compute_dtype(torch.bfloat16)
    try:
        m = VQBASE(**cfg)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).train()
        m.quantize.q_counter = m.quantize.q_re_end
        got = {}
        m.quant_conv.register_forward_hook(lambda mod, i, o: got.__setitem__("z", o.detach()))
        with _flash(True), _counting(ops._SpatialAttentionFlash) as calls:
            rec, q = m(x.to(dev))
            ((x.to(dev) - rec).abs().mean() + q).backward()
            with torch.no_grad():
                dec = m.decode(taps["z_q"].detach().to(dev))
            torch.cuda.synchronize()
    finally:
        ops.set_compute_dtype(old)
    assert calls, "no AttnBlock took the chunked kernels"
    e_z, e_dec = relerr(got["z"], ref_z), relerr(dec, ref)
    print(f"z {e_z:.2e} dec {e_dec:.2e} ({len(calls)} AttnBlock forwards)")
    assert rec.shape == ref.shape and e_z < tol and e_dec < tol
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
