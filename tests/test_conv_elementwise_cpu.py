"""The element-wise convolution checker (tests/helpers/conv_elementwise_check.py, used by tests/test_gpu_conv_elementwise.py) tested on
the CPU: a stand-in kernel -- ``F.conv2d`` in fp32 on the same operands, rounded once to bf16 -- must pass both operand modes, and each of
six injected faults of the size real kernels make must be rejected in BOTH modes (where gauss mode cannot see one at this shape, the
test says so and int mode must).  The two references that follow the library's documented arithmetic instead of the plain formula (the
sub-pixel phase filters, the two roundings of the sumpool2x data-gradient fallback) are checked against the plain one here too."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import conv_elementwise_check as CHK  # noqa: E402

TAU = 2.0 ** -18
CASE = CHK._case("standin", 2, 128, 128, 20, 36, res=True)            # 2 x 128 x 20 x 36 -> 128, 3x3, K = 1152
N0, H0, W0 = 1, 7, 11                                                  # the pixel the single-pixel faults hit
KH, KW, C0 = 0, 2, 40                                                  # ... and the tap / channel (slot 40 ... 47) they hit


@pytest.fixture(scope="module", params=CHK.MODES)
def setup(request):
    mode = request.param
    ins = CHK.make_inputs(CASE, mode)
    r, s = CHK.reference_fwd(CASE, ins)
    x, w = ins["x"].float(), ins["w"]
    acc = F.conv2d(x, w, ins["b"], padding=1)                          # the stand-in's fp32 accumulator, before residual and rounding
    return dict(mode=mode, ins=ins, r=r, s=s, x=x, w=w, acc=acc, res=ins["res"].float())


def verdict(st, y):
    """does the checker accept y?  (gauss: every element inside the bound; int: bitwise)"""
    if st["mode"] == "gauss":
        return CHK.gauss_ratio(y, st["r"], st["s"], TAU)[1] == 0
    return CHK.int_equal(y, st["r"])[0]


def truncate(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def test_standin_passes(setup):
    y = (setup["acc"] + setup["res"]).bfloat16()
    assert verdict(setup, y)
    if setup["mode"] == "gauss":
        ratio, bad = CHK.gauss_ratio(y, setup["r"], setup["s"], TAU)
        assert bad == 0 and 0.5 < ratio <= 1.0, ratio                  # the bound is tight: rounding alone comes within a few per cent of it
    else:
        above, ties = CHK.int_teeth(setup["r"])
        assert above >= 0.25 and ties >= 0.05, (above, ties)


def test_a_truncated_output_is_rejected(setup):
    y = truncate(setup["acc"] + setup["res"])
    assert not verdict(setup, y)
    if setup["mode"] == "gauss":
        assert CHK.gauss_ratio(y, setup["r"], setup["s"], TAU)[1] > 0.15 * y.numel()      # (truncation moves about a quarter of all outputs out of the bound)


def test_b_one_dropped_product_is_rejected(setup):
    acc = setup["acc"].clone()
    acc[N0, :, H0, W0] -= setup["w"][:, C0, KH, KW] * setup["x"][N0, C0, H0 + KH - 1, W0 + KW - 1]
    assert not verdict(setup, (acc + setup["res"]).bfloat16())


def test_c_top_border_row_one_tap_row_off_is_rejected(setup):
    shifted = F.conv2d(F.pad(setup["x"], (1, 1, 0, 2)), setup["w"], setup["ins"]["b"])       # every tap reads one row too low
    acc = setup["acc"].clone()
    acc[:, :, 0] = shifted[:, :, 0]
    assert not verdict(setup, (acc + setup["res"]).bfloat16())


def test_d_two_swapped_taps_are_rejected(setup):
    w = setup["w"].clone()
    w[:, :, 0, 1], w[:, :, 1, 0] = setup["w"][:, :, 1, 0], setup["w"][:, :, 0, 1]
    y = (F.conv2d(setup["x"], w, setup["ins"]["b"], padding=1) + setup["res"]).bfloat16()
    assert not verdict(setup, y)


def test_e_one_channel_slot_from_the_neighbouring_pixel_is_rejected(setup):
    x, w = setup["x"], setup["w"]
    right, wrong = x[N0, C0:C0 + 8, H0 + KH - 1, W0 + KW - 1], x[N0, C0:C0 + 8, H0 + KH - 1, W0 + KW - 2]
    acc = setup["acc"].clone()
    acc[N0, :, H0, W0] += w[:, C0:C0 + 8, KH, KW] @ (wrong - right)
    assert not verdict(setup, (acc + setup["res"]).bfloat16())


def test_f_residual_added_after_the_rounding_is_rejected(setup):
    y = (setup["acc"].bfloat16().float() + setup["res"]).bfloat16()
    assert not verdict(setup, y)


def test_teeth_counts_ties_and_large_values():
    r = torch.tensor([0.0, 255.0, 257.0, 258.0, 511.0, 514.0, 516.0, 1026.0, -300.0, -301.0]).double()
    above, ties = CHK.int_teeth(r)
    assert above == pytest.approx(0.8) and ties == pytest.approx(0.4)                     # ties: 257, 511, 514, -301
    for v in (257.0, 511.0, 514.0, -301.0):                                                  # ... and they ARE ties: truncation and RNE differ
        t = torch.tensor([v])
        assert float(t.bfloat16()) != v and abs(float(t.bfloat16()) - v) == abs(float(truncate(t)) - v)


def test_phase_filters_restate_upsample_conv():
    """``linear_map_phases`` with the UNROUNDED tap sums is the plain Upsample + 3x3 convolution (forward and adjoint); with integer taps the
    rounded sums are exact, so int mode can use the plain reference for the sub-pixel kernels; with gauss taps the rounding of the phase
    filters alone breaks the plain bound -- the reason the gauss reference of those kernels goes through ``phase_weights``."""
    c = CHK._case("phases", 2, 64, 128, 12, 20, up=True)
    for mode in CHK.MODES:
        ins = CHK.make_inputs(c, mode)
        plain, s = CHK.reference_fwd(c, ins)
        a, w = ins["x"].double(), ins["w"].double()
        sets = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
        exact = torch.zeros(2, 2, 128, 64, 2, 2, dtype=torch.float64)
        for pa, pb, r_, s_ in [(i, j, k, l) for i in range(2) for j in range(2) for k in range(2) for l in range(2)]:
            exact[pa, pb, :, :, r_, s_] = sum(w[:, :, kh, kw] for kh in sets[(pa, r_)] for kw in sets[(pb, s_)])
        via = CHK.linear_map_phases(c, a, exact) + ins["b"].double()[None, :, None, None]
        assert float((via - plain).abs().max()) <= 1e-12 * float(s.max())
        rounded, s_ph = CHK.reference_fwd(c, ins, phases=True)
        d_plain, _ = CHK.reference_dgrad(c, ins)
        d_round, _ = CHK.reference_dgrad(c, ins, phases=True)
        if mode == "int":
            assert torch.equal(rounded, plain) and torch.equal(d_round, d_plain)
        else:
            y = rounded.float().bfloat16()                          # a sub-pixel stand-in: exact accumulation of the rounded phase filters
            assert CHK.gauss_ratio(y, rounded, s_ph, TAU)[1] == 0
            assert CHK.gauss_ratio(y, plain, s, TAU)[1] > 0
            assert float((d_round - d_plain).abs().max()) > 0


def test_two_stage_data_gradient_reference():
    """the sumpool2x fallback: bf16(sum of four bf16-rounded high-resolution gradients).  The composed bound accepts exactly that, the
    single-rounding bound does not always, and a pool that drops one of the four pixels at one place is rejected in both modes."""
    c = CHK._case("two_stage", 2, 128, 128, 12, 20, up=True)
    for mode in CHK.MODES:
        ins = CHK.make_inputs(c, mode)
        r_hi, s_hi = CHK.reference_dgrad(c, ins, high_res=True)
        r_lo, s_lo = CHK.reference_dgrad(c, ins)
        assert float((CHK.pool4(r_hi) - r_lo).abs().max()) <= 1e-12 * float(s_lo.max())
        hi = r_hi.float().bfloat16()
        dx = CHK.pool4(hi.float()).bfloat16()
        broken = hi.float().clone()
        broken[1, 5, 6, 8] = 0.0
        dx_broken = CHK.pool4(broken).bfloat16()
        assert not torch.equal(dx, dx_broken)
        if mode == "int":
            assert CHK.int_equal(dx, r_hi, expected=CHK.int_expected_two_stage(r_hi))[0]
            assert not CHK.int_equal(dx_broken, r_hi, expected=CHK.int_expected_two_stage(r_hi))[0]
            assert not CHK.int_equal(dx, r_lo)[0]                    # (two roundings are not one: the plain expectation would be wrong here)
        else:
            r, bound = CHK.two_stage_bound(r_hi, s_hi, TAU)
            assert CHK.gauss_ratio(dx, r, None, TAU, bound=bound)[1] == 0
            assert CHK.gauss_ratio(dx_broken, r, None, TAU, bound=bound)[1] > 0
