"""The numpy restatement of the VQ-IMG objective's tail (tests/helpers/gan_tail_ref.py) against the CPU oracle of the loss stack
(oracle/loss_oracle.py: ``generator_loss``, ``discriminator_loss``, ``adaptive_weight``) in fp64, on both sides of the discriminator's gate,
and the header's declaration of the entry points the GPU tests drive.  No GPU."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "make-a-scene_amd"), ROOT):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import gan_tail_ref as R  # noqa: E402
from oracle import loss_oracle as LO  # noqa: E402

DISC_START = 250001
KW = dict(codebook_weight=0.7, disc_factor=0.9, disc_weight=0.8)


@pytest.fixture()
def case(monkeypatch):
    """images / reconstructions [2, 3, 16, 16] (the reconstruction a 3x3 convolution of a fixed map, so that it has a last layer), a
    one-block discriminator whose logits are [2, 1, 6, 6], everything fp64"""
    monkeypatch.setattr(LO, "disc_forward", functools.partial(LO.disc_forward, nf=8, n_layers=1))
    g = torch.Generator().manual_seed(20)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in LO.synth_disc_state_dict(seed=2, nf=8, n_layers=1).items()}
    images = torch.rand(2, 3, 16, 16, generator=g, dtype=torch.float64) * 2 - 1
    h = torch.randn(2, 4, 16, 16, generator=g, dtype=torch.float64)
    w = (0.2 * torch.randn(3, 4, 3, 3, generator=g, dtype=torch.float64)).requires_grad_(True)
    q = torch.rand(3, generator=g, dtype=torch.float64)
    return sd, images, h, w, q


@pytest.mark.parametrize("step", [DISC_START - 1, DISC_START])
def test_restatement_equals_the_oracle_in_fp64(case, step):
    sd, images, h, w, q = case
    rec = F.conv2d(h, w, padding=1)
    loss, nll, g_loss, d_w = LO.generator_loss(sd, images, rec, q, w, step, DISC_START, **KW)
    d_loss = LO.discriminator_loss(sd, images, rec, step, DISC_START, disc_factor=KW["disc_factor"])
    logits_fake, logits_real = LO.disc_forward(sd, rec, True), LO.disc_forward(sd, images, True)
    assert tuple(logits_fake.shape) == (2, 1, 6, 6)
    nll_grads = torch.autograd.grad(nll, w, retain_graph=True)[0].numpy()
    g_grads = torch.autograd.grad(g_loss, w, retain_graph=True)[0].numpy()
    x, r, lf, lr = images.numpy(), rec.detach().numpy(), logits_fake.detach().numpy(), logits_real.detach().numpy()
    loss, nll_v, g_loss_v, d_loss = loss.detach(), nll.detach(), g_loss.detach(), d_loss.detach()
    close = lambda a, b: abs(float(a) - float(b)) <= 1e-12 * max(1.0, abs(float(b)))
    assert close(R.nll(x, r), nll_v) and close(R.l1_sum(x, r) / r.size, nll_v)
    g_term, m_real, m_fake = R.logit_terms(lf, lr)
    assert close(g_term, g_loss_v) and close(0.5 * (m_real + m_fake), LO.hinge_d_loss(logits_real, logits_fake).detach())
    assert close(R.adaptive_weight(nll_grads, g_grads, KW["disc_weight"]), d_w)
    got, got_w = R.generator_loss(R.nll(x, r), g_term, q.numpy(), nll_grads, g_grads, step, DISC_START, **KW)
    assert close(got, loss) and close(got_w, d_w)
    assert close(R.hinge_d_loss(lr, lf, step, DISC_START, KW["disc_factor"]), d_loss)
    open_ = step >= DISC_START
    assert R.gate(step, DISC_START, 0.9) == (0.9 if open_ else 0.0) == LO.adopt_weight(0.9, step, DISC_START)
    assert (float(d_loss) != 0.0) == open_ and (abs(float(loss) - float(nll_v) - 0.7 * float(q.mean())) > 1e-9) == open_


def test_backward_rules_are_torchs_in_fp32():
    """the fp32 rules the kernels are held to bit for bit are what autograd computes for the torch expressions on the CPU: torch.abs's
    subgradient (0 where rec == images) under a mean, and relu's zero at the hinge knees"""
    g = torch.Generator().manual_seed(21)
    images = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    rec = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1)
    rec.view(-1)[::7] = images.view(-1)[::7]
    rec.requires_grad_(True)
    up = torch.tensor(0.37)
    (torch.mean(torch.abs(images - rec)) * up).backward()
    want = R.l1_backward(images.numpy(), rec.detach().numpy(), np.float32(0.37))
    assert np.array_equal(rec.grad.numpy(), want) and (want[np.unravel_index(0, want.shape)] == 0) and np.count_nonzero(want == 0) >= 220
    real = torch.randn(2, 1, 6, 6, generator=g)
    fake = torch.randn(2, 1, 6, 6, generator=g)
    real.view(-1)[::5] = 1.0
    fake.view(-1)[::5] = -1.0
    real.requires_grad_(True), fake.requires_grad_(True)
    # (0.5 * gate) as one factor: with gate 1 the product with the upstream gradient is the exact half of it
    (LO.hinge_d_loss(real, fake) * up).backward()
    dreal, dfake = R.hinge_backward(real.detach().numpy(), fake.detach().numpy(), np.float32(0.37), 5, 5, 1.0)
    assert np.array_equal(real.grad.numpy(), dreal) and np.array_equal(fake.grad.numpy(), dfake)
    assert dreal.reshape(-1)[0] == 0 and dfake.reshape(-1)[0] == 0
    fake.grad = None
    (-torch.mean(fake) * up).backward()
    assert np.array_equal(fake.grad.numpy(), R.generator_term_backward(fake.detach().numpy(), np.float32(0.37)))


def test_bf16_rounding_of_the_restatement_is_torchs():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(22)) * 3
    x[:4] = torch.tensor([0.0, -0.0, float("inf"), 1.00390625])          # (the last one: a tie, rounded to even)
    assert np.array_equal(R.bf16_round(x.numpy()), x.bfloat16().float().numpy())


def test_header_declares_the_entry_points():
    import mas_hip
    want = {"mas_gan_l1_blocks", "mas_gan_l1_fwd", "mas_gan_l1_finalize", "mas_gan_l1_bwd", "mas_gan_logits_fwd", "mas_gan_logits_bwd",
            "mas_gan_combine_fwd", "mas_gan_combine_bwd"}
    assert want <= set(mas_hip.EXPORTS), sorted(want - set(mas_hip.EXPORTS))
    assert mas_hip.GAN_RUN == R.RUN and mas_hip.ABI_VERSION == 10
