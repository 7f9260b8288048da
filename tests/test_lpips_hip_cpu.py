"""The whole-image LPIPS HIP path without a GPU: the fp64 restatement (tests/helpers/lpips_ref.py) against torch's own fp64 autograd of
today's ``LPIPS.forward`` expressions, the reachability of the GPU tests' bounds by torch's fp32 evaluation alone, the zero-norm rule,
the C ABI's argument checks and the switch (``losses.lpips.hip_path``) in its off position."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lpips_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_tiny.npz")
ENTRIES = ("mas_lpips_pack_fwd", "mas_lpips_pack_bwd", "mas_lpips_relu_fwd", "mas_lpips_pool_fwd", "mas_lpips_pool_bwd", "mas_lpips_head_blocks",
           "mas_lpips_head_fwd", "mas_lpips_finalize", "mas_lpips_head_bwd")


@pytest.fixture(scope="module")
def sd():
    from oracle.lpips_oracle import expected_keys, synth_lpips_state_dict
    z = np.load(GOLD)
    assert [str(k) for k in z["keys"]] == expected_keys()           # the weights the golden was written with: the same layout
    return synth_lpips_state_dict(3)


def _inputs():
    """the golden's own 32 x 32 pair, and an odd-sized pair whose levels are 40x56 -> 20x28 -> 10x14 -> 5x7 -> 2x3"""
    z = np.load(GOLD)
    return [(torch.from_numpy(z["real"]), torch.from_numpy(z["fake"])), R.images(2, 40, 56, seed=5)]


@pytest.fixture(scope="module")
def fp64_autograd(sd):
    """[(real, fake, dout, out, d fake)] from torch's fp64 autograd of the module's expressions"""
    out = []
    for k, (real, fake) in enumerate(_inputs()):
        dout = torch.rand(real.shape[0], generator=torch.Generator().manual_seed(k)).double() + 0.5
        f = fake.double().requires_grad_(True)
        v = R.torch_expression(R.f64(sd), real.double(), f)
        (g,) = torch.autograd.grad((v.view(-1) * dout).sum(), f)
        assert torch.isfinite(g).all()                               # no all-zero pixel on these inputs (torch would give NaN)
        out.append((real, fake, dout, v.detach().view(-1), g))
    return out


def test_restatement_equals_torch_fp64_autograd(sd, fp64_autograd):
    for real, fake, dout, want, dwant in fp64_autograd:
        got, dgot = R.lpips(sd, real, fake, dout)
        assert float(((got - want).abs() / want.abs()).max()) <= 1e-12
        assert R.rel_l2(dgot, dwant) <= 1e-12 and float((dgot - dwant).abs().max()) <= 1e-12 * float(dwant.abs().max())


def test_restatement_reproduces_the_reference_golden(sd):
    z = np.load(GOLD)
    got, dgot = R.lpips(sd, torch.from_numpy(z["real"]), torch.from_numpy(z["fake"]))
    assert np.allclose(got.numpy(), z["out"].reshape(-1), rtol=1e-5)
    assert R.rel_l2(dgot, torch.from_numpy(z["dfake"])) < 1e-4


def test_torch_fp32_alone_stays_inside_the_gpu_tests_bounds(sd, fp64_autograd):
    """value 1e-5 relative (1e-4 at 40 x 56) and gradient 1e-4 relative L2: what tests/test_gpu_lpips_hip.py asks of the kernels is
    reachable by the reference's own fp32 arithmetic, on the whole op and on the head alone"""
    for real, fake, dout, want, dwant in fp64_autograd:
        f = fake.clone().requires_grad_(True)
        v = R.torch_expression(sd, real, f).view(-1)
        (g,) = torch.autograd.grad((v * dout.float()).sum(), f)
        err = float(((v.detach().double() - want).abs() / want.abs()).max())
        print(f"whole op {tuple(real.shape)}: fp32 value rel {err:.2e}, gradient rel-L2 {R.rel_l2(g, dwant):.2e}")
        assert err <= (1e-4 if real.shape[2] == 40 else 1e-5) and R.rel_l2(g, dwant) <= 1e-4
    for c in (64, 128, 256, 512):
        for h, w in ((1, 1), (3, 5), (16, 16), (40, 56)):
            f, wts, dout = R.head_case(c, h, w, seed=1)
            want = R.head_sums(f[:2].double(), f[2:].double(), wts.double()) / (h * w)
            dwant = R.head_bwd(f[:2].double(), f[2:].double(), wts.double(), dout.double())
            ff = f[2:].clone().requires_grad_(True)
            nt = lambda t: t / (torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True)) + 1e-10)
            got = (((nt(f[:2]) - nt(ff)) ** 2) * wts.view(1, -1, 1, 1)).sum(dim=1, keepdim=True).mean([2, 3]).view(-1)
            (g,) = torch.autograd.grad((got * dout).sum(), ff)
            err = float(((got.detach().double() - want).abs() / want.abs()).max())
            assert err <= (1e-4 if (h, w) == (40, 56) else 1e-5), (c, h, w, err)
            assert R.rel_l2(g, dwant) <= 1e-4, (c, h, w, R.rel_l2(g, dwant))


def test_zero_norm_rule_is_finite_where_torch_gives_nan():
    f, wts, dout = R.head_case(64, 3, 5, seed=2, kind="zeros")
    seed = R.head_bwd(f[:2].double(), f[2:].double(), wts.double(), dout.double())
    assert torch.isfinite(seed).all()
    # where the rec pixel is all zero the value is sum_c w_c (r_c / |r|)^2 and the gradient is the derivative of the eps-quotient alone
    r0 = f[:2, :, 0, 0].double()
    want0 = 2.0 * (dout.double() / 15).view(-1, 1) * wts.double() * (r0 / (r0.norm(dim=1, keepdim=True) + R.EPS)) / R.EPS * -1.0
    assert torch.allclose(seed[:, :, 0, 0], want0, rtol=1e-12)
    assert torch.count_nonzero(seed[:, :, 0, 2]) == 0                 # both sides zero: e = 0
    ff = f[2:].double().requires_grad_(True)
    nt = lambda t: t / (torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True)) + 1e-10)
    v = (((nt(f[:2].double()) - nt(ff)) ** 2) * wts.double().view(1, -1, 1, 1)).sum(1).mean([1, 2])
    (g,) = torch.autograd.grad((v * dout.double()).sum(), ff)
    assert torch.isnan(g[:, :, 0, 0]).all() and torch.isnan(g[:, :, 0, 2]).all()      # sqrt's backward at 0
    ok = torch.ones(3, 5, dtype=torch.bool)
    ok[0, 0] = ok[0, 2] = False
    assert R.rel_l2(seed[:, :, ok], g[:, :, ok]) <= 1e-12           # every other pixel: torch's own gradient


def test_pool_restatement_routes_to_the_first_maximum():
    g = torch.Generator().manual_seed(3)
    x = torch.tensor(R.BF16_SET, dtype=torch.float64)[torch.randint(0, 8, (2, 8, 5, 7), generator=g)]
    a = R.relu(x)
    assert torch.equal(R.pool(a), torch.nn.functional.max_pool2d(a, 2, 2))
    dz, seed = torch.randn(2, 8, 2, 3, generator=g).double(), torch.randn(2, 8, 5, 7, generator=g).double()
    xr = x.clone().requires_grad_(True)
    ar = torch.relu(xr)
    ((torch.nn.functional.max_pool2d(ar, 2, 2) * dz).sum() + (ar * seed).sum()).backward()
    assert torch.equal(R.pool_bwd(a, seed, dz), xr.grad)
    assert torch.equal(R.pool_bwd(a, seed, None)[:, :, 4], (seed * (a > 0))[:, :, 4])      # the unpooled last row: the seed only


def test_lpips_entries_are_exported():
    import mas_hip
    assert set(ENTRIES) <= set(mas_hip.EXPORTS)
    assert mas_hip.lib().mas_abi_version() == 10


def test_lpips_entries_reject_bad_arguments_without_gpu():
    import mas_hip
    L = mas_hip.lib()
    img = mas_hip.FaceImage(8, mas_hip.F32, 2, 3, 16, 16, 0, 768, 256, 16, 1)
    other = mas_hip.FaceImage(8, mas_hip.F32, 2, 3, 16, 20, 0, 960, 320, 20, 1)
    bad = mas_hip.FaceImage(8, 7, 2, 3, 16, 16, 0, 768, 256, 16, 1)
    r = ctypes.byref
    assert L.mas_lpips_pack_fwd(None, None, None, None, None, 0, None) == -1
    assert L.mas_lpips_pack_fwd(r(img), r(other), 8, 8, 8, mas_hip.F32, None) == -1 and b"differ" in L.mas_last_error()
    assert L.mas_lpips_pack_fwd(r(img), r(bad), 8, 8, 8, mas_hip.F32, None) == -1           # image dtype
    assert L.mas_lpips_pack_fwd(r(img), r(img), 8, 8, 8, 5, None) == -1                     # canvas dtype
    assert L.mas_lpips_pack_bwd(None, mas_hip.F32, 8, r(img), None) == -1
    assert L.mas_lpips_pack_bwd(8, mas_hip.F32, 8, r(bad), None) == -1
    assert L.mas_lpips_relu_fwd(8, 12, mas_hip.F32, None) == -1                             # n % 8
    assert L.mas_lpips_relu_fwd(None, 16, mas_hip.F32, None) == -1
    assert L.mas_lpips_pool_fwd(8, 8, 2, 1, 4, 64, mas_hip.F32, None) == -1                 # no window in one row
    assert L.mas_lpips_pool_fwd(8, 8, 2, 4, 4, 12, mas_hip.F32, None) == -1                 # C % 8
    assert L.mas_lpips_pool_bwd(8, None, None, 8, 2, 0, 4, 64, mas_hip.F32, None) == -1     # H < 1
    assert L.mas_lpips_pool_bwd(None, None, None, 8, 2, 4, 4, 64, mas_hip.F32, None) == -1
    assert L.mas_lpips_head_blocks(16, 16, 96) == -1 and L.mas_lpips_head_blocks(0, 16, 64) == -1
    assert (L.mas_lpips_head_blocks(1, 1, 64), L.mas_lpips_head_blocks(40, 56, 64), L.mas_lpips_head_blocks(40, 56, 512)) == (1, 18, 140)
    assert L.mas_lpips_head_fwd(8, 8, 2, 4, 4, 96, mas_hip.F32, 8, None) == -1 and b"C 96" in L.mas_last_error()
    assert L.mas_lpips_head_fwd(8, 8, 2, 4, 4, 64, 9, 8, None) == -1
    assert L.mas_lpips_head_fwd(8, None, 2, 4, 4, 64, mas_hip.F32, 8, None) == -1
    assert L.mas_lpips_head_bwd(8, 8, 2, 4, 0, 64, mas_hip.F32, 8, 8, None) == -1
    assert L.mas_lpips_head_bwd(8, 8, 2, 4, 4, 1024, mas_hip.F32, 8, 8, None) == -1
    assert L.mas_lpips_head_bwd(8, 8, 2, 4, 4, 64, mas_hip.F32, None, 8, None) == -1
    hw, blocks = (ctypes.c_int32 * 2)(16, 4), (ctypes.c_int32 * 2)(1, 0)
    assert L.mas_lpips_finalize(8, 2, 2, hw, blocks, 8, None) == -1 and b"level 1" in L.mas_last_error()
    assert L.mas_lpips_finalize(8, 2, 9, hw, blocks, 8, None) == -1                         # more than 8 levels
    assert L.mas_lpips_finalize(8, 2, 2, None, blocks, 8, None) == -1


def _module(sd):
    from losses.lpips import LPIPS
    m = LPIPS().eval()
    m.load_state_dict(sd, strict=True)
    return m


def _inline(m, real_x, fake_x):
    """``LPIPS.forward`` as it stood before the switch existed (evaluation mode)"""
    from losses.lpips import norm_tensor, spatial_average
    b = real_x.shape[0]
    feats = m.vgg(m.scaling_layer(torch.cat([real_x, fake_x], dim=0)))
    total = 0
    for i, f in enumerate(feats):
        f = f.float()
        d = (norm_tensor(f[:b]) - norm_tensor(f[b:])) ** 2
        w = m.lins[i].model[1].weight.float()
        total = total + spatial_average((d * w).sum(dim=1, keepdim=True))
    return total


def test_switch_is_off_by_default_and_restores():
    from losses import lpips as M
    assert os.environ.get("MAS_LPIPS_HIP", "0") == "1" or not M.hip_path_enabled()
    before = M.hip_path_enabled()
    with M.hip_path(True):
        assert M.hip_path_enabled()
        with M.hip_path(False):
            assert not M.hip_path_enabled()
        assert M.hip_path_enabled()
    assert M.hip_path_enabled() == before
    M.hip_path(True)                                                    # as a setter
    assert M.hip_path_enabled()
    M.hip_path(before)
    assert M.hip_path_enabled() == before


def test_cpu_tensors_never_take_the_hip_path(sd, monkeypatch):
    """off, and on with tensors outside the envelope (CPU): the module's torch expression runs -- here up to its first convolution,
    which has no CPU fallback -- and ``lpips_distance`` is never entered"""
    from losses import lpips as M
    import mas_hip.lpips as H
    m = _module(sd)
    real, fake = R.images(2, 16, 16, seed=1)
    monkeypatch.setattr(H, "lpips_distance", lambda *a, **k: pytest.fail("the HIP path was taken"))
    for on in (False, True):
        with M.hip_path(on):
            assert not m._takes_hip_path(real, fake)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                m(real, fake)


def test_switch_off_is_the_inline_expression_bit_for_bit(sd, monkeypatch):
    """the convolutions stand in as F.conv2d (the module's own need a GPU): with the switch off, and on with CPU tensors, forward
    and gradient equal the inline expression's bits"""
    import torch.nn.functional as F
    from losses import lpips as M
    from models.modules import Conv2d
    monkeypatch.setattr(Conv2d, "forward", lambda self, x: F.conv2d(x, self.weight, self.bias, padding=1))
    m = _module(sd)
    real, fake = R.images(2, 24, 16, seed=2)
    fa = fake.clone().requires_grad_(True)
    want = _inline(m, real, fa)
    (gw,) = torch.autograd.grad(want.sum(), fa)
    for on in (False, True):
        with M.hip_path(on):
            fb = fake.clone().requires_grad_(True)
            got = m(real, fb)
            (gg,) = torch.autograd.grad(got.sum(), fb)
        assert got.shape == (2, 1, 1, 1) and torch.equal(got, want) and torch.equal(gg, gw)
