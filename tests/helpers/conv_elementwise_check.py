#!/usr/bin/env python3
"""GPU child of tests/test_gpu_conv_elementwise.py, and the CPU side both that test and tests/test_conv_elementwise_cpu.py import.

    conv_elementwise_check.py SETTING OUT.pt

runs every case of SETTINGS[SETTING] (the dispatch switches of that setting are already in the environment: the library reads them once
per process) in both operand modes and writes, per case and mode: y from ``ops.conv_fwd_raw``, y and dx from ``ops.norm_act_conv``
with ``requires_grad`` on x only (exactly the data-gradient launches autograd makes), the kernel name right after every launch
(``ops.last_kernel()``), and the tile height of every stream-kernel launch.  Nothing numeric is judged here.

The CPU side: ``make_inputs`` (seeded operands of a case in *gauss* or *int* mode), ``reference_fwd`` / ``reference_dgrad`` (fp64, with
the magnitudes S), ``gauss_ratio`` / ``int_expected`` / ``int_teeth`` (the comparisons: they take tensors and know nothing of a GPU)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ACT_NONE, ACT_AFFINE, ACT_AFFINE_SILU = 0, 1, 2
MODES = ("gauss", "int")
HALF_ULP = 2.0 ** -8          # half a bf16 ulp relative to the value, round to nearest even


def _case(name, n, cin, cout, h, w, ks=3, stride=1, pad=(1, 1, 1, 1), up=False, act=ACT_NONE, res=False, bias=True, dt="bf16", out="bf16",
          fwd=None, dgrad=None, want=(), xr=8, wr=4, dyr=4):
    """pad = (top, bottom, left, right).  fwd / dgrad: the kernel each launch has to take ("*": whatever the dispatch gives, recorded;
    dgrad None: no data gradient in this case; a tuple: the data-movement launches around it included).  want: (kernel, feature) pairs this case is there to reach.
    xr / wr / dyr: *int* mode ranges (|x| <= xr, |w| <= wr + ks * ks // 2, |dy| <= dyr)."""
    hl, wl = (2 * h, 2 * w) if up else (h, w)
    ho, wo = (hl + pad[0] + pad[1] - ks) // stride + 1, (wl + pad[2] + pad[3] - ks) // stride + 1
    return dict(name=name, n=n, cin=cin, cout=cout, h=h, w=w, ks=ks, stride=stride, pad=tuple(pad), up=up, act=act, res=res, bias=bias,
                dt=dt, out=out, fwd=fwd, dgrad=dgrad, want=tuple(want), xr=xr, wr=wr, dyr=dyr, ho=ho, wo=wo)


WIDE, STREAM, UP2F, UP2D, GEN = "conv3x3_wide", "conv3x3_stream", "conv_up2_fwd", "conv_up2_dgrad", "conv_fwd"
P2 = (2, 2, 2, 2)
DOWN = (0, 1, 0, 1)
WIDE_ENV = {"MAS_CONV_WIDE_MIN_TILES_PER_CU": "0", "MAS_CONV_WIDE_ANY_WIDTH": "1"}

# (label, environment, cases).  The shapes are the few-tile ones of wide_check.py / stream_check.py / up2_check.py / CONV_CASES.
SETTINGS = [
    ("default", {}, [
        # 1x1 GEMM: 189 pixels (M % 128 = 61), 3 and 7 channel chunks of 64, two cout tiles; a data gradient takes it when both channel
        # counts are multiples of 128 (the others' data gradients are the general kernel's KS = 1 instance)
        _case("pw_192_256", 3, 192, 256, 9, 7, ks=1, pad=(0, 0, 0, 0), xr=24, dyr=16, res=True, fwd="conv1x1", dgrad=GEN,
              want=[("conv1x1", "ragged_m"), ("conv1x1", "chunks3"), ("conv1x1", "res"), ("conv1x1", "cout_tiles2"), (GEN, "k1")]),
        _case("pw_448_256", 2, 448, 256, 5, 11, ks=1, pad=(0, 0, 0, 0), xr=24, dyr=16, fwd="conv1x1", dgrad=GEN, want=[("conv1x1", "chunks7")]),
        _case("pw_128_256", 3, 128, 256, 9, 7, ks=1, pad=(0, 0, 0, 0), xr=24, dyr=16, fwd="conv1x1", dgrad="conv1x1", want=[("conv1x1", "dgrad")]),
        # thin RGB-edge layers at an odd map: each is the other's data gradient (K = 72: wider *int* ranges, see the parent's table)
        _case("thin_8_128", 2, 8, 128, 33, 17, fwd="conv_thin_fwd", dgrad="conv_thin_out", xr=48, wr=8, dyr=4,
              want=[("conv_thin_fwd", "fwd"), ("conv_thin_out", "dgrad")]),
        _case("thin_128_8", 2, 128, 8, 33, 17, fwd="conv_thin_out", dgrad="conv_thin_fwd", xr=8, wr=4, dyr=48,
              want=[("conv_thin_out", "fwd"), ("conv_thin_fwd", "dgrad")]),
        # Downsample: stride 2, pad (0, 1, 0, 1); even and odd maps, all four parity classes of dx ragged
        _case("s2_even", 2, 128, 128, 18, 34, stride=2, pad=DOWN, dyr=12, fwd="conv_s2_fwd", dgrad="conv_s2_dgrad",
              want=[("conv_s2_fwd", "even"), ("conv_s2_dgrad", "even")]),
        _case("s2_odd", 2, 128, 256, 13, 35, stride=2, pad=DOWN, dyr=12, fwd="conv_s2_fwd", dgrad="conv_s2_dgrad",
              want=[("conv_s2_fwd", "odd"), ("conv_s2_dgrad", "odd"), ("conv_s2_fwd", "cout_tiles2")]),
        # a 9 x 13 map is too narrow for conv_s2: the general stride-2 instance, and the zero-stuffed data gradient
        _case("s2_small", 2, 128, 128, 9, 13, stride=2, pad=DOWN, dyr=12, fwd=GEN, dgrad=("zero_stuff2x", "*"),
              want=[(GEN, "k3s2")]),
        # the general kernel
        _case("gen_32_32", 2, 32, 32, 9, 13, xr=12, dyr=12, fwd=GEN, dgrad=GEN, res=True, want=[(GEN, "bc32"), (GEN, "res")]),
        _case("gen_64_96", 2, 64, 96, 9, 13, fwd=GEN, dgrad=GEN, want=[(GEN, "bc128")]),
        _case("gen_64_96_affine", 2, 64, 96, 9, 13, act=ACT_AFFINE, fwd=GEN, want=[(GEN, "affine")]),
        _case("gen_64_96_silu", 2, 64, 96, 9, 13, act=ACT_AFFINE_SILU, res=True, fwd=GEN, want=[(GEN, "silu")]),
        _case("gen_k4s2", 2, 64, 128, 18, 22, ks=4, stride=2, fwd=GEN, dgrad=("zero_stuff2x", GEN), want=[(GEN, "k4s2")]),
        _case("gen_k4s1", 2, 64, 64, 11, 13, ks=4, fwd=GEN, dgrad=GEN, want=[(GEN, "k4s1")]),
        _case("gen_k4s1_one", 2, 128, 8, 7, 9, ks=4, dyr=24, fwd=GEN, dgrad=GEN),                       # the PatchGAN's 1-channel head (padded to 8)
        _case("gen_bf16_f32", 2, 64, 96, 9, 13, out="f32", fwd=GEN, want=[(GEN, "bf16_f32")]),
        _case("gen_f32_f32", 2, 40, 24, 9, 13, dt="f32", out="f32", dyr=16, fwd=GEN, dgrad=GEN, want=[(GEN, "f32_f32")]),
        # stride-1 3x3 shapes of few tiles: whatever they take by default (recorded; the wide / stream families have their own children)
        _case("few_128", 2, 128, 128, 20, 36, fwd="*", dgrad="*"),
    ]),
    ("wide", WIDE_ENV, [
        _case("w_one_tile", 1, 64, 128, 16, 32, fwd=WIDE, dgrad=None, want=[(WIDE, "one_tile"), (WIDE, "cin64")]),
        _case("w_ragged_res", 2, 128, 128, 40, 72, res=True, fwd=WIDE, dgrad=WIDE,
              want=[(WIDE, "ragged"), (WIDE, "cin128"), (WIDE, "res"), (WIDE, "transposed")]),
        _case("w_c256", 3, 256, 128, 20, 36, fwd=WIDE, dgrad=None, want=[(WIDE, "cin256")]),
        _case("w_cout256", 2, 128, 256, 33, 47, res=True, fwd=WIDE, dgrad=WIDE, want=[(WIDE, "cout_tiles2")]),
        _case("w_c512", 1, 512, 512, 16, 32, fwd=WIDE, dgrad=None, want=[(WIDE, "cin512"), (WIDE, "cout_tiles4")]),
        _case("w_pad2", 2, 128, 128, 31, 35, pad=P2, fwd=WIDE, dgrad=None, want=[(WIDE, "pad2")]),
        _case("w_affine", 2, 128, 256, 18, 34, act=ACT_AFFINE, fwd=WIDE, want=[(WIDE, "affine")]),
        _case("w_silu", 3, 256, 128, 20, 36, act=ACT_AFFINE_SILU, res=True, fwd=WIDE, want=[(WIDE, "silu")]),
        # sub-pixel Upsample + conv: ragged low-resolution maps, n_spatial = 3 / 10 / 12 (the tile count is padded to a multiple of 8)
        _case("u_64_128", 3, 64, 128, 12, 20, up=True, fwd=UP2F, dgrad=("*", "sumpool2x"),
              want=[(UP2F, "cin64"), (UP2F, "ragged"), (UP2F, "pad8")]),
        _case("u_128_256", 5, 128, 256, 12, 40, up=True, fwd=UP2F, dgrad=UP2D,
              want=[(UP2F, "cin128"), (UP2F, "cout_tiles2"), (UP2D, "cin128"), (UP2D, "ragged"), (UP2D, "pad8")]),
        _case("u_256_128", 3, 256, 128, 20, 33, up=True, fwd=UP2F, dgrad=UP2D, want=[(UP2D, "cout_tiles2")]),
        _case("u_128_64", 3, 128, 64, 12, 20, up=True, fwd="*", dgrad=UP2D, want=[(UP2D, "cin64")]),
    ]),
    ("wide_noup2", dict(WIDE_ENV, MAS_CONV_UP2="0"), [
        _case("wf_128", 2, 128, 128, 12, 20, up=True, fwd=WIDE, dgrad=(WIDE, "sumpool2x"),
              want=[(WIDE, "upfold"), (WIDE, "sumpool_dgrad")]),
        _case("wf_64_256", 3, 64, 256, 9, 21, up=True, fwd=WIDE, dgrad=None),
    ]),
    ("stream", {"MAS_CONV_WIDE": "0", "MAS_CONV_UP2": "0"}, [
        _case("s_one_tile", 1, 128, 128, 16, 16, fwd=STREAM, dgrad=None, want=[(STREAM, "cin128")]),
        _case("s_ragged_res", 2, 128, 128, 40, 24, res=True, fwd=STREAM, dgrad=STREAM, want=[(STREAM, "ragged"), (STREAM, "res")]),
        _case("s_c256", 3, 256, 128, 20, 36, fwd=STREAM, dgrad=None, want=[(STREAM, "cin256")]),
        _case("s_cout256", 2, 128, 256, 33, 17, res=True, fwd=STREAM, dgrad=STREAM, want=[(STREAM, "cout_tiles2")]),
        _case("s_affine", 2, 128, 256, 18, 18, act=ACT_AFFINE, fwd=STREAM, want=[(STREAM, "affine")]),
        _case("s_silu", 3, 256, 128, 20, 36, act=ACT_AFFINE_SILU, res=True, fwd=STREAM, want=[(STREAM, "silu")]),
        _case("s_upfold", 2, 128, 128, 12, 20, up=True, fwd=STREAM, dgrad=(STREAM, "sumpool2x"), want=[(STREAM, "upfold")]),
    ]),
    ("stream_th16", {"MAS_CONV_WIDE": "0", "MAS_CONV_STREAM_TH8": "0"}, [
        _case("s16_ragged", 2, 128, 128, 40, 24, res=True, fwd=STREAM, dgrad=None),
    ]),
    ("multi", dict(WIDE_ENV, MAS_CONV_WGS_PER_CU="1"), [
        # more tiles than work-groups at one work-group per CU (asserted in the child from the launch geometry)
        _case("m_wide", 136, 64, 256, 16, 32, fwd=WIDE, dgrad=None),
        _case("m_up2", 33, 64, 256, 16, 32, up=True, fwd=UP2F, dgrad=None),
    ]),
    ("nos2", {"MAS_CONV_S2": "0"}, [
        _case("z_s2", 2, 128, 128, 18, 34, stride=2, pad=DOWN, dyr=12, fwd=GEN, dgrad=("zero_stuff2x", "*"), want=[("zero_stuff2x", "pad2_dgrad")]),
    ]),
]
CASES = {c["name"]: c for _, _, cs in SETTINGS for c in cs}


# --------------------------------------------------------------------------------------------------------------------------- operands
def _tdt(s):
    return torch.bfloat16 if s == "bf16" else torch.float32


def int_weight(g, cout, cin, ks, wr):
    """integer filter with structure: a random part in [-wr, wr] plus an offset that is different for each of the ks * ks taps and
    rotates with o and i -- a swap of two taps, or kh / kw transposed, changes the result"""
    kk = ks * ks
    base = torch.randint(-wr, wr + 1, (cout, cin, ks, ks), generator=g)
    t = torch.arange(kk).view(1, 1, ks, ks)
    rot = (t + torch.arange(cout).view(-1, 1, 1, 1) + 2 * torch.arange(cin).view(1, -1, 1, 1)) % kk
    return (base + rot - kk // 2).float()


def make_inputs(c, mode):
    """seeded CPU operands: x, w (fp32 tensor holding bf16 values when the case is bf16), bias (fp32 or None), res, ss ([N][Cin][2] or
    None), dy"""
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])) * 2 + (mode == "int"))
    dt, odt = _tdt(c["dt"]), _tdt(c["out"])
    n, cin, cout, h, w, ks = c["n"], c["cin"], c["cout"], c["h"], c["w"], c["ks"]
    k = cin * ks * ks
    if mode == "gauss":
        x = torch.randn(n, cin, h, w, generator=g).to(dt)
        wt = (torch.randn(cout, cin, ks, ks, generator=g) / k ** 0.5).to(dt).float()
        b = 0.1 * torch.randn(cout, generator=g)
        res = torch.randn(n, cout, c["ho"], c["wo"], generator=g).to(odt)
        dy = torch.randn(n, cout, c["ho"], c["wo"], generator=g).to(dt)
    else:
        xr, wr, dyr = c["xr"], c["wr"], c["dyr"]
        x = torch.randint(-xr, xr + 1, (n, cin, h, w), generator=g).to(dt)
        wt = int_weight(g, cout, cin, ks, wr)
        b = torch.randint(-16, 17, (cout,), generator=g).float()
        res = torch.randint(-16, 17, (n, cout, c["ho"], c["wo"]), generator=g).to(odt)
        dy = torch.randint(-dyr, dyr + 1, (n, cout, c["ho"], c["wo"]), generator=g).to(dt)
        wmax = wr + ks * ks // 2
        assert k * (2 * xr + 1) * wmax + 32 < 2 ** 24 and 16 * cout * ks * ks * dyr * wmax < 2 ** 24, c["name"]   # every partial sum exact in fp32
    ss = None
    if c["act"] != ACT_NONE:
        if c["act"] == ACT_AFFINE:            # x * s + b exact in fp32 (power-of-two scales; shifts multiples of 1/4): no room for a different rounding
            sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n, cin), generator=g)]
            sh = torch.randint(-4, 5, (n, cin), generator=g).float() * 0.25
        else:
            sc, sh = 1.0 + 0.2 * torch.randn(n, cin, generator=g), 0.3 * torch.randn(n, cin, generator=g)
        ss = torch.stack([sc, sh], dim=-1).contiguous()
    return dict(x=x, w=wt, b=b if c["bias"] else None, res=res if c["res"] else None, ss=ss, dy=dy)


# ------------------------------------------------------------------------------------------------------------------------- references
def _silu(u):
    return u * torch.sigmoid(u)


def activated(c, x, ss):
    """the operand the convolution reads: act(x * s + b) in fp32, rounded to the input type as the kernel's loader does (fp64 out)"""
    if c["act"] == ACT_NONE:
        return x.double()
    a = x.float() * ss[..., 0][:, :, None, None] + ss[..., 1][:, :, None, None]
    if c["act"] == ACT_AFFINE_SILU:
        a = _silu(a)
    return a.to(x.dtype).double()


def linear_map(c, a, w):
    """Upsample, zero padding, convolution: the bare linear map of a case, in the dtype of its arguments"""
    if c["up"]:
        a = a.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    t, b, l, r = c["pad"]
    return F.conv2d(F.pad(a, (l, r, t, b)), w, stride=c["stride"])


def phase_weights(w):
    """The sub-pixel image of Upsample + 3x3 (include/mas_hip.h, MAS_WLAYOUT_UP2) restated: Wp[a][b][:, :, r, s] = the sum of the taps
    (kh in R(a, r), kw in R(b, s)) added in fp32 in kh, kw order and rounded ONCE to bf16.  R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1},
    R(1,1) = {2}.  -> [2][2][Cout][Cin][2][2] fp32 holding bf16 values"""
    sets = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    out = torch.zeros(2, 2, w.shape[0], w.shape[1], 2, 2)
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for s in range(2):
                    v = torch.zeros(w.shape[0], w.shape[1])
                    for kh in sets[(a, r)]:
                        for kw in sets[(b, s)]:
                            v = v + w[:, :, kh, kw].float()
                    out[a, b, :, :, r, s] = v.bfloat16().float()
    return out


def linear_map_phases(c, a, wp):
    """the same Upsample + 3x3 / pad 1 convolution through the four 2x2 phase filters: y[2i + a, 2j + b] = sum_rs Wp[a][b][r][s] x[i + a + r - 1, j + b + s - 1]"""
    assert c["up"] and c["ks"] == 3 and c["stride"] == 1 and c["pad"] == (1, 1, 1, 1)
    n, _, h, w = a.shape
    ap = F.pad(a, (1, 1, 1, 1))
    y = a.new_zeros(n, wp.shape[2], 2 * h, 2 * w)
    for pa in range(2):
        for pb in range(2):
            y[:, :, pa::2, pb::2] = F.conv2d(ap, wp[pa, pb].to(a.dtype))[:, :, pa:pa + h, pb:pb + w]
    return y


def reference_fwd(c, ins, phases=False, mags=True):
    """(r, S) in fp64: r = conv(act(x)) + b + res on exactly the operands the kernel reads, S = the same sum of absolute values.
    phases: through the rounded phase filters (what the sub-pixel kernel is handed) instead of the nine taps.  mags = False (*int* mode,
    which needs no S): S is not computed"""
    a = activated(c, ins["x"], ins["ss"])
    w = ins["w"].double()
    if phases:
        wp = phase_weights(ins["w"]).double()
        r, s = linear_map_phases(c, a, wp), (linear_map_phases(c, a.abs(), wp.abs()) if mags else torch.zeros(()))
    else:
        r, s = linear_map(c, a, w), (linear_map(c, a.abs(), w.abs()) if mags else torch.zeros(()))
    if ins["b"] is not None:
        r, s = r + ins["b"].double()[None, :, None, None], s + ins["b"].double().abs()[None, :, None, None]
    if ins["res"] is not None:
        r, s = r + ins["res"].double(), s + ins["res"].double().abs()
    return r, s


def reference_dgrad(c, ins, phases=False, high_res=False, mags=True):
    """(r, S) in fp64 of dx = the adjoint of the case's linear map applied to dy.  high_res (Upsample cases): the gradient with respect
    to the UPSAMPLED map, which the fallback path rounds to bf16 before ``sumpool2x`` sums it (``two_stage_bound``)"""
    shape = (c["n"], c["cin"], c["h"], c["w"])
    cc = dict(c, up=False) if high_res else c
    if high_res:
        shape = (c["n"], c["cin"], 2 * c["h"], 2 * c["w"])
    outs = []
    for absolute in ((False, True) if mags else (False,)):
        z = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        dy = ins["dy"].double()
        if phases:
            wp = phase_weights(ins["w"]).double()
            y = linear_map_phases(cc, z, wp.abs() if absolute else wp)
        else:
            w = ins["w"].double()
            y = linear_map(cc, z, w.abs() if absolute else w)
        outs.append(torch.autograd.grad(y, z, dy.abs() if absolute else dy)[0])
    return outs[0], (outs[1] if mags else None)


def pool4(t):
    return t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2] + t[:, :, 1::2, 0::2] + t[:, :, 1::2, 1::2]


# -------------------------------------------------------------------------------------------------------------------------- comparisons
def gauss_bound(r, s, tau, out_bf16=True):
    """|y - r| <= 2^-8 (|r| + tau S) + tau S: half a bf16 ulp of the exactly accumulated value (round to nearest even: derived, not
    measured) on top of tau S, the fp32 accumulation of the products.  fp32 outputs: tau S alone."""
    acc = tau * s
    return HALF_ULP * (r.abs() + acc) + acc if out_bf16 else acc


def gauss_ratio(y, r, s, tau, out_bf16=True, bound=None):
    """(worst |y - r| / bound over EVERY element, number of elements outside); a non-finite output is outside"""
    y = y.double()
    bound = gauss_bound(r, s, tau, out_bf16) if bound is None else bound
    err = (y - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(y), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max()), int((ratio > 1).sum())


def two_stage_bound(r_hi, s_hi, tau):
    """The Upsample fold's fallback data gradient: the 3x3 kernel writes the high-resolution gradient in bf16 (bound e_i per element as
    above), ``sumpool2x`` adds four of them in fp32 (3 roundings of at most 2^-24 of the partial sums) and rounds once more.
    -> (r, bound) at the low resolution: sum e_i + 2^-8 (|sum r_i| + sum e_i) + 3 * 2^-24 sum (|r_i| + e_i)"""
    e = gauss_bound(r_hi, s_hi, tau)
    r, se, sa = pool4(r_hi), pool4(e), pool4(r_hi.abs() + e)
    return r, se + HALF_ULP * (r.abs() + se) + 3 * 2.0 ** -24 * sa


def int_expected(r, out_bf16=True):
    """*int* mode: every partial sum is an integer (or a multiple of 1/4) below 2^24, exact in fp32 in any order, so the kernel's
    accumulator holds r itself and its output is r rounded once"""
    assert float(r.abs().max()) < 2 ** 24
    return r.float().bfloat16() if out_bf16 else r.float()


def int_expected_two_stage(r_hi):
    hi = r_hi.float().bfloat16().float()
    return pool4(hi).bfloat16()


def int_equal(y, r, out_bf16=True, expected=None):
    """(bitwise equal, number of elements that differ)"""
    want = int_expected(r, out_bf16) if expected is None else expected
    y = y.contiguous()
    return torch.equal(y, want.to(y.dtype)), int((y.float() != want.float()).sum())


def int_teeth(r):
    """(share of |r| above 256, share of exact bf16 ties) of an integer reference: above 256 a bf16 holds no odd integer, so rounding is
    exercised; odd integers in [256, 512) and values = 2 mod 4 in [512, 1024) sit exactly between two bf16 values, so rounding half away
    from zero or truncating differs from nearest-even there"""
    a = r.abs().round().long()
    ties = ((a >= 256) & (a < 512) & (a % 2 == 1)) | ((a >= 512) & (a < 1024) & (a % 4 == 2))
    return float((a > 256).double().mean()), float(ties.double().mean())


# --------------------------------------------------------------------------------------------------------------------------- GPU child
def _stream_th(c, dims, env, cus):
    """tile height conv3x3_stream.hip gives a launch: 8 rows for a prologue-free launch of fewer 16-row tiles than CUs"""
    n, ho, wo, cout, act = dims
    tiles16 = n * ((ho + 15) // 16) * ((wo + 15) // 16) * (cout // 128)
    return 8 if env.get("MAS_CONV_STREAM_TH8", "1") != "0" and act == ACT_NONE and tiles16 < cus else 16


def run(setting, out_path):
    from mas_hip import ops
    label, env, cases = next(s for s in SETTINGS if s[0] == setting)
    for k, v in env.items():
        assert os.environ.get(k) == v, f"start this child with {k}={v}"
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ops.set_compute_dtype(torch.bfloat16)
    seen = []
    ops.set_launch_hook(lambda kind, shape, launch: (launch(), seen.append((kind, ops.last_kernel(), shape))))
    moved = {}
    for name in ("zero_stuff2x", "sumpool2x"):           # the data-movement launches around a fallback data gradient, recorded like the rest
        def wrap(fn, name=name):
            def f(*a):
                y = fn(*a)
                seen.append((name, ops.last_kernel(), None))
                return y
            return f
        moved[name] = getattr(ops, name)
        setattr(ops, name, wrap(moved[name]))
    cl = lambda t: None if t is None else t.to(dev).contiguous(memory_format=torch.channels_last)
    results = {}
    try:
        for c in cases:
            for mode in MODES:
                if mode == "int" and c["act"] == ACT_AFFINE_SILU:
                    continue
                ins = make_inputs(c, mode)
                n, cin, cout, h, w, ks, st = c["n"], c["cin"], c["cout"], c["h"], c["w"], c["ks"], c["stride"]
                ho, wo, (pt, pb, pl, pr) = c["ho"], c["wo"], c["pad"]
                out = {}
                wd, bd = ins["w"].to(dev), (ins["b"].to(dev) if ins["b"] is not None else None)
                del seen[:]
                y = ops.conv_fwd_raw(cl(ins["x"]), ins["ss"].to(dev) if ins["ss"] is not None else None, ops.ConvWeight(wd, False), bd, cl(ins["res"]),
                                     n, h, w, cin, ho, wo, cout, ks, st, pt, pl, c["act"], c["up"], _tdt(c["out"]))
                out["fwd_kernel"] = ops.last_kernel()
                torch.cuda.synchronize()
                assert [k for k, _, _ in seen] == ["conv_fwd"] and seen[0][1] == out["fwd_kernel"], seen
                out["y"] = y.cpu().contiguous()
                feats = set()
                if out["fwd_kernel"] == STREAM:
                    feats.add("th%d" % _stream_th(c, (n, ho, wo, cout, c["act"]), os.environ, cus))
                if setting == "multi":                   # launch geometry: grid = min(tiles, MAS_CONV_WGS_PER_CU * CUs)
                    if out["fwd_kernel"] == WIDE:
                        tiles = n * ((ho + 15) // 16) * ((wo + 31) // 32) * (cout // 128)
                    else:
                        tiles = (n * ((h + 15) // 16) * ((w + 31) // 32) + 7) // 8 * 8 * 4 * (cout // 128)
                    assert int(os.environ["MAS_CONV_WGS_PER_CU"]) == 1 and tiles > cus, (c["name"], tiles, cus)
                    feats.add("tiles_gt_grid")
                if c["dgrad"] is not None:
                    assert c["act"] == ACT_NONE and c["out"] == c["dt"], c["name"]
                    # the launches autograd makes: weight and bias frozen, so no weight gradient runs
                    xd = cl(ins["x"]).requires_grad_(True)
                    del seen[:]
                    y2 = ops.norm_act_conv(xd, wd, bd, residual=cl(ins["res"]), stride=st, padding=(pt, pb, pl, pr), upsample=c["up"],
                                           in_dtype=_tdt(c["dt"]), out_dtype=_tdt(c["out"]))
                    n_fwd = len(seen)
                    y2.backward(cl(ins["dy"]))
                    last = ops.last_kernel()
                    torch.cuda.synchronize()
                    # (conv_s2_dgrad is launched without the hook: the process's last kernel names it)
                    names = [k for _, k, _ in seen[n_fwd:]] or [last]
                    out["nac_fwd_kernel"] = seen[0][1]
                    out["dgrad_kernels"] = names
                    out["y_nac"] = y2.detach().cpu().contiguous()
                    out["dx"] = xd.grad.cpu().contiguous()
                    if STREAM in names:
                        hl, wl = (2 * h, 2 * w) if c["up"] else (h, w)
                        feats.add("dgrad_th%d" % _stream_th(c, (n, hl, wl, cin, ACT_NONE), os.environ, cus))
                out["features"] = sorted(feats)
                results[(c["name"], mode)] = out
                print(f"{label:12s} {c['name']:18s} {mode:5s} fwd {out['fwd_kernel']:15s} dgrad {out.get('dgrad_kernels')} {sorted(feats)}", flush=True)
    finally:
        ops.set_launch_hook(None)
        for name, fn in moved.items():
            setattr(ops, name, fn)
    torch.save(dict(results=results, cus=cus, env={k: os.environ.get(k) for k in env}), out_path)


if __name__ == "__main__":
    run(sys.argv[1], sys.argv[2])
