"""Decode attention on the MI355X, every element of the context row against fp64, on every route: ``mas_attn_decode`` /
``mas_attn_decode_dev`` (attn_decode.hip, attn_decode_core.h, decode_step.hip), ``mas_attn_decode_split`` / ``_split_dev``
(attn_decode_split.hip) and ``mas_attn_decode_shared`` / ``_shared_dev`` (attn_decode_shared.hip, attn_decode_tile.h).  Cases, inputs,
reference, bounds and the GPU runner are tests/helpers/decode_elementwise_check.py (read its docstring first);
tests/test_decode_elementwise_cpu.py shows on the CPU that this judgement catches a dropped key, a key counted twice, a skipped rescale,
an empty split taken as m = 0, a combine that ignores state 63, a neighbour head's K unit, swapped V rows, a truncated store, exchanged
query slots and a stray store over a ragged group's last row.

One test per route family, so that a failure names its kernel.  B = 2, H = 3 (one B = H = 1 case per route), bf16 and fp32, hd 16 / 32 /
64 / 128, visible lengths on the edges of the 32-key granule, of the key slots (KPP) and of a pass (KPP * KU keys; 256 for the unsplit
kernel), four operand modes (gauss, hard, onehot, uniform).  Every case with one query runs the host-``past`` form and the
device-``past`` form, whose cache row ``past`` holds NaN before the call; the two must agree bit for bit.  Cache rows past the valid
length, the gaps of strided rows and the memory around the prompt blocks hold NaN.  ``mas_last_kernel`` names every launch and
REQUIRED lists the (launch, feature) pairs the union of the cases has to reach.

Bounds (U = 2^-8, TAU = 2^-18, C_F32 = 32, FLOOR from attn_rowwise_check; A_o = P |v|):
  bf16  |y - r| <= U |r| + C_F32 TAU A_o + FLOOR        fp32  |y - r| <= C_F32 TAU A_o + FLOOR
  onehot: o == v[target] bitwise; uniform at a power-of-two length: o == sum(v) / L bitwise (bf16: after the one rounding).

Measured on an MI355X, worst |y - r| / bound over all cases and modes (1 = the bound):
                             bf16    fp32
  attn_decode                0.935   0.040      (nq 1, 2, 5; plain and strided layouts)
  attn_decode_dev            0.892   0.040
  attn_decode_split          0.920   0.033
  attn_decode_split_dev      0.920   0.033
  attn_decode_shared         0.946   0.032
  attn_decode_shared_dev     0.946   0.032
The bf16 figures are the store's rounding (up to U |r| by itself); the fp32 figures are all of C_F32 TAU A_o the kernels use, hard mode
the worst.  Every onehot and power-of-two uniform case is bitwise on every route, every device form equals its host form bit for bit, and
no defect showed: no kernel was changed.  141 cases; the file takes about 11 s on an MI355X box: unsplit 2.5 s, split 2.1 s, shared 4.5 s,
most of it the fp64 reference on the CPU.
"""
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import decode_elementwise_check as D  # noqa: E402

_done = {}
_spent = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _family(route):
    """runs and judges every (case, mode) of a route once: (failures, worst ratio per (kernel, dtype), [(case, {form: kernel})])"""
    if route in _done:
        return _done[route]
    t0 = time.perf_counter()
    fails, worst, ran = [], {}, []
    for c in D.CASES:
        if c["route"] != route:
            continue
        kern = {}
        for mode in c["modes"]:
            ins, ref = D.prepare(c, mode)
            got, kern = D.run(c, ins)
            want = {"host": D.HOST[route]}
            if D.has_dev(c):
                want["dev"] = D.DEV[route]
            if kern != want:
                fails.append(f"{c['name']} {mode}: launched {kern}, not {want}")
            for form, y in got.items():
                f, w = D.judge(c, mode, ins, ref, y, tag=form)
                fails += f
                key = (kern[form], c["dtype"])
                worst[key] = max(worst.get(key, 0.0), w)
            if "dev" in got and not (got["dev"].view("int64") == got["host"].view("int64")).all():
                fails.append(f"{c['name']} {mode}: the device-past form differs from the host form in "
                             f"{int((got['dev'].view('int64') != got['host'].view('int64')).sum())} elements")
        ran.append((c, kern))
    _spent[route] = time.perf_counter() - t0
    _done[route] = (fails, worst, ran)
    return _done[route]


def _check(route):
    _dev()
    fails, worst, ran = _family(route)
    for (k, dt), w in sorted(worst.items()):
        print(f"\n{k} {dt}: worst |y - r| / bound {w:.3f}")
    print(f"{route}: {len(ran)} cases in {_spent[route]:.1f} s")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


def test_unsplit_host_and_device_past():
    _check("unsplit")


def test_split_host_and_device_past():
    _check("split")


def test_shared_host_and_device_past():
    _check("shared")


def test_every_required_route_and_feature_was_reached():
    _dev()
    ran = []
    for route in D.ROUTES:
        ran += _family(route)[2]
    got = D.reached(ran)
    missing = {k: sorted(f - got.get(k, set())) for k, f in D.REQUIRED.items() if not f <= got.get(k, set())}
    print(f"\ndecode element-wise: {sum(_spent.values()):.1f} s in all")
    assert not missing, missing
