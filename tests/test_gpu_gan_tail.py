"""csrc/gan_loss.hip and the ``hip_tail`` switch of ``losses.loss_img.VQLPIPSWithDiscriminator`` on the GPU, against the numpy
restatement tests/helpers/gan_tail_ref.py (which tests/test_gan_tail_cpu.py holds to oracle/loss_oracle.py in fp64).

Forward sums: a lane adds RUN = 8 fp32 terms as a pairwise tree, everything beyond is fp64 and the total is rounded once, so a sum of
non-negative terms is within (1 + 2^-24)^5 - 1 of the fp64 sum; asserted is RUN * 2^-24 = 4.8e-7 relative (``gan_tail_ref.sum_bound``), on
the sum of the terms' absolute values where they have signs.  Backward values: bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "make-a-scene_amd"), ROOT):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import gan_tail_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
U = R.U
FORMS = [(dt, cl) for dt in (torch.float32, torch.bfloat16) for cl in (False, True)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _form(x, dt, channels_last, dev):
    x = x.to(dev).to(dt)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()


def _np(t):
    """the tensor's values in logical order as fp32"""
    return t.detach().float().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scalar(v, dev):
    return torch.full((1,), v, dtype=torch.float32, device=dev)


# ---- the L1 term -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (3, 3, 33, 31), (2, 3, 64, 64)])
def test_l1_sum_and_gradient_every_dtype_and_layout(shape):
    """fp32 / bf16 x NCHW / channels_last on each operand (16 pairings per shape), one element in eleven with rec == img.  Forward:
    |sum - fp64 sum| <= RUN 2^-24 sum (derivation: the module docstring); the nll output, sum / n + w mean(p) rounded once more, within
    that over n plus 2^-24 |nll|.  Backward: the gradient's bits, its dtype and its strides (those of rec), and the perceptual term's.
    Measured on an MI355X: largest |sum - fp64| / sum over the 48 cases 4.9e-8 (bound 4.8e-7)."""
    from mas_hip import gan_tail as T
    dev = _dev()
    g = torch.Generator().manual_seed(sum(shape))
    img0 = torch.rand(shape, generator=g) * 2 - 1
    rec0 = torch.rand(shape, generator=g) * 2 - 1
    img0.view(-1)[::11] = 0.5                                  # (exact in bf16: equal after either cast)
    rec0.view(-1)[::11] = 0.5
    p = torch.rand(shape[0], 1, 1, 1, generator=g).to(dev)
    gup = _scalar(0.37, dev)
    worst = 0.0
    for idt, icl in FORMS:
        for rdt, rcl in FORMS:
            img, rec = _form(img0, idt, icl, dev), _form(rec0, rdt, rcl, dev)
            x, r = _np(img), _np(rec)
            out = T.l1_fwd(img, rec, p.view(-1), 0.8).cpu().numpy().astype(np.float64)
            want, want_nll = R.l1_sum(x, r), R.nll(x, r, _np(p), 0.8)
            err = abs(out[0] - want)
            worst = max(worst, err / want)
            assert err <= R.sum_bound(want), (shape, idt, icl, rdt, rcl, out[0], want)
            assert abs(out[1] - want_nll) <= R.sum_bound(want) / r.size + 1.01 * U * abs(want_nll), (out[1], want_nll)
            drec, dp = T.l1_bwd(img, rec, gup, shape[0], 0.8)
            assert drec.dtype == rec.dtype and drec.stride() == rec.stride()
            ref = R.l1_backward(x, r, np.float32(0.37), bf16=rdt == torch.bfloat16)
            assert np.array_equal(_bits(_np(drec)), _bits(ref)), (shape, idt, icl, rdt, rcl)
            assert np.count_nonzero(ref == 0) >= (r.size + 10) // 11 and _np(drec).reshape(-1)[0] == 0
            assert np.array_equal(_bits(_np(dp)), _bits(np.full(shape[0], R.perceptual_backward(0.37, shape[0], 0.8))))
    print(f"L1 sum {shape}: largest relative error {worst:.2e} (bound {R.RUN * U:.2e})")


def test_l1_nan_and_the_autograd_node():
    """a NaN in either input makes the sum NaN (as the ATen expression) and leaves a zero in the gradient at its own element only; the node
    ``gan_tail.nll`` hands ``rec`` and the perceptual term their gradients and ``images`` none"""
    from mas_hip import gan_tail as T
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    img0, rec0 = torch.rand(3, 3, 33, 31, generator=g), torch.rand(3, 3, 33, 31, generator=g)
    for which in (0, 1):
        a, b = img0.clone(), rec0.clone()
        (a, b)[which].view(-1)[4097] = float("nan")
        img, rec = _form(a, torch.float32, True, dev), _form(b, torch.bfloat16, False, dev)
        out = T.l1_fwd(img, rec).cpu()
        assert torch.isnan(out).all()
        drec, dp = T.l1_bwd(img, rec, _scalar(1.0, dev))
        ref = R.l1_backward(_np(img), _np(rec), np.float32(1.0), bf16=True)
        assert dp is None and np.array_equal(_bits(_np(drec)), _bits(ref)) and ref.reshape(-1)[4097] == 0 and np.count_nonzero(ref == 0) == 1
    img, rec = _form(img0, torch.float32, False, dev), _form(rec0, torch.float32, True, dev).requires_grad_(True)
    p = torch.rand(3, 1, 1, 1, generator=g).to(dev).requires_grad_(True)
    nll, l1_sum = T.nll(img, rec, p, 0.5, return_sum=True)
    assert nll.dim() == 0 and nll.dtype == torch.float32 and not l1_sum.requires_grad
    assert abs(float(nll.detach()) - R.nll(_np(img), _np(rec), _np(p), 0.5)) <= 1e-6
    (nll * 3.0).backward()
    assert np.array_equal(_bits(_np(rec.grad)), _bits(R.l1_backward(_np(img), _np(rec), np.float32(3.0))))
    assert rec.grad.stride() == rec.stride() and p.grad.shape == p.shape
    assert np.array_equal(_bits(_np(p.grad).reshape(-1)), _bits(np.full(3, R.perceptual_backward(3.0, 3, 0.5))))
    with pytest.raises(ValueError, match="not differentiated"):
        T.nll(img.clone().requires_grad_(True), rec)


# ---- the PatchGAN logit terms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 1, 6, 6), (3, 1, 30, 30)])
def test_logit_terms_and_gradients(shape):
    """values planted exactly at the hinge knees (real == 1, fake == -1; the one-logit shape is nothing else).  The three means within
    RUN 2^-24 of the mean of the terms' absolute values plus the final rounding, the gated loss within both; every gradient bit for bit, on
    both sides of the gate, zero at the knees."""
    from mas_hip import gan_tail as T
    dev = _dev()
    g = torch.Generator().manual_seed(40 + shape[-1])
    real, fake = torch.randn(shape, generator=g) * 1.5, torch.randn(shape, generator=g) * 1.5
    real.view(-1)[::5] = 1.0
    fake.view(-1)[::5] = -1.0
    rd, fd = real.to(dev), fake.to(dev)
    r, f, n = real.numpy(), fake.numpy(), real.numel()
    start, factor = 1000, 0.5
    want = R.logit_terms(f, r)
    slack = [R.sum_bound(np.abs(f.astype(np.float64)).sum()) / n + 1.01 * U * abs(want[0]), R.sum_bound(want[1] * n) / n + 1.01 * U * want[1],
             R.sum_bound(want[2] * n) / n + 1.01 * U * want[2]]
    for s in (start - 1, start):
        step = torch.tensor(s, dtype=torch.int64, device=dev)
        out_d = T.logits_fwd(fd, rd, step, start, factor)
        out = out_d.cpu().numpy().astype(np.float64)
        assert out[4] == R.gate(s, start, factor)
        for k in range(3):
            assert abs(out[k] - want[k]) <= slack[k], (shape, k, out[k], want[k])
        d_ref = R.hinge_d_loss(r, f, s, start, factor)
        assert abs(out[3] - d_ref) <= 0.5 * factor * (slack[1] + slack[2]) + 1.01 * U * abs(d_ref)
        assert (out[3] == 0.0) == (s < start or d_ref == 0.0)            # (the one-logit shape sits on both knees: 0 either way)
        step += 5                                               # (the backward reads the gate the forward stored, not the counter)
        dfake, dreal = T.logits_bwd(fd, rd, None, _scalar(0.37, dev), out_d[4:])
        ref_real, ref_fake = R.hinge_backward(r, f, np.float32(0.37), s, start, factor)
        assert np.array_equal(_bits(_np(dreal)), _bits(ref_real)) and np.array_equal(_bits(_np(dfake)), _bits(ref_fake))
        assert _np(dreal).reshape(-1)[0] == 0 and _np(dfake).reshape(-1)[0] == 0
        if s >= start and n > 1:
            assert np.count_nonzero(ref_real) > 0 and np.count_nonzero(ref_fake) > 0
    # the generator's half: fake alone, no step
    out = T.logits_fwd(fd).cpu().numpy().astype(np.float64)
    assert abs(out[0] - want[0]) <= slack[0] and abs(out[2] - want[2]) <= slack[2] and out[1] == 0 and out[3] == 0
    dfake, dreal = T.logits_bwd(fd, None, _scalar(0.37, dev))
    assert dreal is None and np.array_equal(_bits(_np(dfake)), _bits(R.generator_term_backward(f, np.float32(0.37))))
    # ... and through the autograd nodes
    fl = fd.clone().requires_grad_(True)
    (T.generator_term(fl) * 0.37).backward()
    assert np.array_equal(_bits(_np(fl.grad)), _bits(R.generator_term_backward(f, np.float32(0.37))))
    fl, rl = fd.clone().requires_grad_(True), rd.clone().requires_grad_(True)
    step = torch.tensor(start, dtype=torch.int64, device=dev)
    (T.hinge_d_loss(rl, fl, step, start, factor) * 0.37).backward()
    ref_real, ref_fake = R.hinge_backward(r, f, np.float32(0.37), start, start, factor)
    assert np.array_equal(_bits(_np(rl.grad)), _bits(ref_real)) and np.array_equal(_bits(_np(fl.grad)), _bits(ref_fake))


# ---- the combine -------------------------------------------------------------------------------------------------------------------------
def test_combine_gate_clamp_counter_and_gradients():
    """the gate at disc_start - 1 and at disc_start from the DEVICE counter; |g_grads| = 0 clamps the ratio at 1e4; |nll_grads| = 0 gives
    weight 0; no gradient reaches the two gradient tensors; the counter advances by exactly 1 when asked and not otherwise.  The weights are
    exact in fp32 (0.75, 0.5, 0.25), so: d_weight one rounding of its fp64 value, the loss one rounding of its own plus the two of
    c_g = fp32(d_weight) * gate -- bounds below."""
    from mas_hip import gan_tail as T
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    start, kw = 250001, dict(disc_factor=0.5, disc_weight=0.75, codebook_weight=0.25)
    a, b = torch.randn(3, 32, 3, 3, generator=g), 0.3 * torch.randn(3, 32, 3, 3, generator=g)
    zero = torch.zeros_like(a)
    vals = dict(nll=0.41, g_loss=-0.23, face=0.05, obj=0.02)
    cb = torch.rand(3, generator=g)
    for na, nb in ((a, b), (a, zero), (zero, b)):
        for s in (start - 1, start):
            for advance in (False, True):
                step = torch.tensor(s, dtype=torch.int64, device=dev)
                leaf = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in vals.items()}
                cbd = cb.to(dev).requires_grad_(True)
                nad, nbd = na.to(dev).requires_grad_(True), nb.to(dev).requires_grad_(True)
                loss, terms = T.combine(leaf["nll"], leaf["g_loss"], cbd, nad, nbd, step, disc_start=start, face_loss=leaf["face"],
                                        object_loss=leaf["obj"], advance=advance, **kw)
                assert int(step) == s + int(advance)
                f32 = lambda v: float(np.float32(v))
                ref, d_w = R.generator_loss(f32(vals["nll"]), f32(vals["g_loss"]), cb.numpy(), na.numpy(), nb.numpy(), s, start,
                                            face_loss=f32(vals["face"]), object_loss=f32(vals["obj"]), **kw)
                gate = R.gate(s, start, 0.5)
                t = terms.cpu().numpy().astype(np.float64)
                assert abs(t[0] - d_w) <= 1.01 * U * d_w and t[2] == gate and t[1] == float(np.float32(t[0]) * np.float32(gate))
                if nb is zero:
                    assert t[0] == 7500.0                       # 1e4 * disc_weight: the clamp
                if na is zero:
                    assert t[0] == 0.0
                assert abs(float(loss.detach()) - ref) <= 1.01 * U * (abs(ref) + 2 * abs(d_w * gate * vals["g_loss"])), (float(loss.detach()), ref)
                (loss * 0.37).backward()
                g_nll, g_g, g_cb = R.combine_backward(np.float32(0.37), np.float32(t[1]), 0.25, 3)
                assert nad.grad is None and nbd.grad is None
                assert float(leaf["nll"].grad) == float(leaf["face"].grad) == float(leaf["obj"].grad) == float(g_nll)
                assert np.array_equal(_bits(_np(leaf["g_loss"].grad)), _bits(g_g))
                assert np.array_equal(_bits(_np(cbd.grad)), _bits(np.full(3, g_cb))) and ((g_g == 0) == (s < start or na is zero))
    with pytest.raises(TypeError, match="int64"):
        T.combine(leaf["nll"], leaf["g_loss"], cbd, nad, nbd, 7, disc_start=start)


# ---- the module behind the switch --------------------------------------------------------------------------------------------------------
CFG = dict(ddconfig=dict(z_channels=32, in_channels=3, out_channels=3, channels=[32, 32, 64], num_res_blocks=1, resolution=64,
                         attn_resolutions=[16], dropout=0.0), n_embed=64, embed_dim=32, init_steps=3000, reservoir_size=12500)


@pytest.fixture(scope="module")
def step_case():
    """the tiny VQBASE and loss of test_gpu_lpips_hip's generator-step test: 64 x 64 input, B = 2, synthetic LPIPS weights, no face term"""
    dev = _dev()
    from losses.loss_img import VQLPIPSWithDiscriminator
    from models import VQBASE
    from oracle import vq_oracle as O
    from oracle.lpips_oracle import synth_lpips_state_dict
    m = VQBASE(**CFG)
    m.load_state_dict(O.synth_state_dict(CFG["ddconfig"], 64, 32, seed=0), strict=True)
    m = m.to(dev).train()
    m.quantize.enable_device_reservoir(seed=3)
    m.quantize.q_counter = m.quantize.q_re_end
    torch.manual_seed(0)
    lf = VQLPIPSWithDiscriminator(disc_start=5, perceptual_loss="lpips", face_loss=None)
    lf.perceptual_loss.load_state_dict(synth_lpips_state_dict(3), strict=True)
    lf = lf.to(dev)
    return m, lf, O.synth_image_batch(2, 3, 64, seed=4).to(dev)


class _Record:
    """the step's own tensors: what the discriminator returned, call by call, and the two gradients of the adaptive weight"""

    def __init__(self, lf, monkeypatch):
        self.logits, self.grads = [], []
        self._hook = lf.discriminator.register_forward_hook(lambda mod, i, o: self.logits.append(o.detach().double().cpu().numpy()))
        grad = torch.autograd.grad

        def recording(*a, **k):
            out = grad(*a, **k)
            self.grads.append(out[0].detach().double().cpu().numpy())
            return out
        monkeypatch.setattr(torch.autograd, "grad", recording)

    def close(self):
        self._hook.remove()


@pytest.mark.parametrize("global_step", [4, 5])
def test_module_both_halves_switch_on_against_off(step_case, monkeypatch, global_step):
    """both ``optimizer_idx`` with the switch on and off, each against the fp64 restatement evaluated on that call's own tensors (images,
    reconstructions, the per-image perceptual term, the logits and the two last-layer gradients as the call saw them): the switch-on
    loss deviates from it by at most 1.2 x the switch-off path's deviation + 1e-6 |loss| -- both are fp32 roundings of one expression.
    The gate (disc_start = 5) closed and open.  Every model parameter gets a finite gradient, the discriminator none from the generator
    half.  Measured on an MI355X (step 5): generator loss 1.656327, deviation off 7.1e-8, on 7.1e-8; d_loss 1.160864, off 2.1e-8, on 2.1e-8
    (step 4: 1.970906, 1.3e-8 both; d_loss exactly 0 both): the two paths round to the same fp32 values here."""
    from losses.loss_img import hip_tail
    m, lf, img = step_case
    disc = list(lf.discriminator.parameters())
    m.zero_grad(set_to_none=True)
    lf.zero_grad(set_to_none=True)
    rec, q = m(img)
    with torch.no_grad():
        p = lf.perceptual_loss(img, rec, None).double().cpu().numpy()
    x, r = _np(img).astype(np.float64), _np(rec).astype(np.float64)
    dev_of = {}
    for on in (False, True):
        rc = _Record(lf, monkeypatch)
        try:
            with hip_tail(on):
                d_loss = lf(1, global_step, img, rec)
                for p_ in disc:
                    p_.requires_grad_(False)
                loss, (nll, obj, face) = lf(0, global_step, img, rec, q, last_layer=m.decoder.model[-1])
        finally:
            rc.close()
            monkeypatch.undo()
            for p_ in disc:
                p_.requires_grad_(True)
        assert len(rc.logits) == 3 and len(rc.grads) == 2 and loss.dim() == 0 and d_loss.dim() == 0 and float(obj) == 0 and float(face) == 0
        ref_d = R.hinge_d_loss(rc.logits[0], rc.logits[1], global_step, 5, 1.0)
        g_term = R.logit_terms(rc.logits[2])[0]
        ref_g, d_w = R.generator_loss(R.nll(x, r, p, 1.0), g_term, _np(q), rc.grads[0], rc.grads[1], global_step, 5)
        assert abs(float(nll) - R.nll(x, r, p, 1.0)) <= 1e-6 * R.nll(x, r, p, 1.0)
        dev_of[on] = (abs(float(loss) - ref_g), abs(float(d_loss) - ref_d), ref_g, ref_d)
        if on:
            assert abs(float(lf.last_terms["d_weight"]) - d_w) <= 1e-6 * d_w and abs(float(lf.last_terms["g_loss"]) - g_term) <= 1e-6 * abs(g_term)
            d_loss.backward()
            assert all(p_.grad is not None and torch.isfinite(p_.grad).all() for p_ in disc)
            kept = [p_.grad.clone() for p_ in disc]
            for p_ in disc:
                p_.requires_grad_(False)
            try:
                loss.backward()
            finally:
                for p_ in disc:
                    p_.requires_grad_(True)
            assert all(torch.equal(a, p_.grad) for a, p_ in zip(kept, disc))                 # nothing from the generator half
            missing = [n for n, p_ in m.named_parameters() if p_.requires_grad and (p_.grad is None or not torch.isfinite(p_.grad).all())]
            assert not missing, missing
    (g_off, d_off, ref_g, ref_d), (g_on, d_on, _, _) = dev_of[False], dev_of[True]
    print(f"global_step {global_step}: generator loss {ref_g:.6f}, deviation off {g_off:.2e}, on {g_on:.2e}; d_loss {ref_d:.6f}, off {d_off:.2e}, on {d_on:.2e}")
    assert (ref_d == 0.0) == (global_step < 5)
    assert g_on <= 1.2 * g_off + 1e-6 * abs(ref_g), (g_on, g_off, ref_g)
    assert d_on <= 1.2 * d_off + 1e-6 * abs(ref_d), (d_on, d_off, ref_d)


def test_module_tensor_step_reads_nothing_on_the_host(step_case):
    """a switch-on forward + backward of both halves with a tensor ``global_step`` under ``set_sync_debug_mode("error")``; the counter
    advances only when the module is told to; with the switch off a tensor step raises"""
    from losses.loss_img import hip_tail
    from losses.lpips import hip_path
    m, lf, img = step_case
    dev = img.device
    step = torch.tensor(7, dtype=torch.int64, device=dev)
    with hip_tail(True), hip_path(True):
        rec, q = m(img)
        lf(0, step, img, rec, q, last_layer=m.decoder.model[-1])[0].backward()         # (settles every workspace before the guarded call)
        rec, q = m(img)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            lf(1, step, img, rec).backward()
            loss, _ = lf(0, step, img, rec, q, last_layer=m.decoder.model[-1])
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert int(step) == 7 and bool(torch.isfinite(loss))
        rec, q = m(img)
        lf.advance_global_step = True
        try:
            lf(0, step, img, rec, q, last_layer=m.decoder.model[-1])
        finally:
            lf.advance_global_step = False
        assert int(step) == 8
        lf(0, 3, img, rec, q, last_layer=m.decoder.model[-1])                           # an int: the module's own scalar, the tensor untouched
        assert int(step) == 8
    with hip_tail(False), pytest.raises(TypeError, match="hip_tail"):
        lf(1, step, img, rec)
