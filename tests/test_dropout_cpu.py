"""CPU checks of the dropout generator and mapping: Philox4x32-10 against the Random123 known-answer vectors, the numpy restatement
(tests/helpers/philox_ref.py) against the C++ header the kernels include (make-a-scene_amd/csrc/mas_philox.h, compiled here as host
code), the p quantisation and scale rule, and the argument checks of the new entries."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import philox_ref as R  # noqa: E402

KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(v) for v in R.philox4x32_10(*ctr, *key)) == want


_HOST = r'''
#include "mas_philox.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
    const unsigned long long seed = strtoull(argv[1], 0, 10), off = strtoull(argv[2], 0, 10);
    const unsigned B = atoi(argv[3]), H = atoi(argv[4]), S = atoi(argv[5]); const float p = (float)atof(argv[6]);
    const unsigned s0 = (unsigned)seed, s1 = (unsigned)(seed >> 32), o = (unsigned)off, t = mas_drop_threshold(p);
    printf("%u %.9g\n", t, mas_drop_scale(t));
    for (unsigned bh = 0; bh < B * H; ++bh)                  /* query-major form: [bh][query][key] */
        for (unsigned q = 0; q < S; ++q) {
            for (unsigned k = 0; k < S; k += 4) { unsigned m = mas_attn_keep_q(s0, s1, o, bh, q, k, t); for (unsigned e = 0; e < 4 && k + e < S; ++e) putchar('0' + ((m >> e) & 1)); }
            putchar('\n');
        }
    for (unsigned bh = 0; bh < B * H; ++bh)                  /* key-major form: [bh][key][query] */
        for (unsigned k = 0; k < S; ++k) {
            for (unsigned q = 0; q < S; q += 4) { unsigned m = mas_attn_keep_k(s0, s1, o, bh, k, q, t); for (unsigned e = 0; e < 4 && q + e < S; ++e) putchar('0' + ((m >> e) & 1)); }
            putchar('\n');
        }
    for (unsigned long long g = 0; g < 9; ++g) { unsigned m = mas_ew_keep8(s0, s1, o, g, t); for (int e = 0; e < 8; ++e) putchar('0' + ((m >> e) & 1)); }
    putchar('\n');
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_philox(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to check mas_philox.h"
    d = tmp_path_factory.mktemp("philox")
    src, exe = d / "p.cpp", d / "p"
    src.write_text(_HOST)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "make-a-scene_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("seed,off,B,H,S,p", [(0, 0, 1, 1, 8, 0.5), (2 ** 63 - 25, 123456789012, 2, 3, 13, 0.1),
                                              (987654321987, 4 * 2 ** 32 + 5, 1, 2, 37, 0.9)])
def test_numpy_mapping_equals_header(host_philox, seed, off, B, H, S, p):
    out = subprocess.run([host_philox, str(seed), str(off), str(B), str(H), str(S), repr(p)], check=True, capture_output=True,
                         text=True).stdout.split("\n")
    t, sc = out[0].split()
    assert int(t) == R.threshold(p) and abs(float(sc) - R.scale(R.threshold(p))) <= 1e-6 * float(sc)
    want = R.attention_keep(seed, off, B, H, S, p).reshape(B * H, S, S)
    qmaj = np.array([[c == "1" for c in row] for row in out[1:1 + B * H * S]]).reshape(B * H, S, S)
    kmaj = np.array([[c == "1" for c in row] for row in out[1 + B * H * S:1 + 2 * B * H * S]]).reshape(B * H, S, S)
    assert (qmaj == want).all()
    assert (kmaj.transpose(0, 2, 1) == want).all()             # both kernel orientations draw the same mask
    ew = np.array([c == "1" for c in out[1 + 2 * B * H * S]])
    assert (ew == R.elementwise_keep(seed, off, 72, p)).all()


def test_mapping_is_tile_free_and_distinct():
    """the mask depends on (b*H + h, query, key) only: a sub-block of a larger problem is the same sub-block; heads / offsets differ"""
    big = R.attention_keep(7, 3, 2, 2, 40, 0.5)
    small = R.attention_keep(7, 3, 2, 2, 17, 0.5)
    assert (big[:, :, :17, :17] == small).all()
    assert (big[0, 0] != big[0, 1]).mean() > 0.4 and (big[0, 0] != big[1, 0]).mean() > 0.4
    assert (R.attention_keep(7, 4, 1, 1, 40, 0.5) != big[0, 0]).mean() > 0.4
    flat = R.elementwise_keep(7, 3, 200_000, 0.25)
    assert abs(flat.mean() - 0.75) < 6 * np.sqrt(0.75 * 0.25 / flat.size)


@pytest.mark.parametrize("p,t", [(0.0, 0), (1e-6, 0), (0.1, 6554), (0.5, 32768), (0.9, 58982), (1 - 1e-7, 65536), (1.0, 65536)])
def test_p_quantisation_and_scale(p, t):
    assert R.threshold(p) == t
    sc = R.scale(t)
    if t == 65536:
        assert sc == 0.0                                       # p = 1: zeros, never inf * 0
    else:
        assert abs(sc * (1 - t / 65536) - 1) < 1e-6            # unbiased for the p actually used: E[Z s] = (1 - t/65536) s = 1


def test_dropout_entries_validate_arguments_without_gpu():
    import mas_hip
    L = mas_hip.lib()
    assert L.mas_abi_version() == 10
    assert L.mas_dropout_apply(None, None, 8, mas_hip.BF16, ctypes.c_float(0.1), None, None) == -1 and b"null" in L.mas_last_error()
    assert L.mas_dropout_apply(16, 16, 8, mas_hip.BF16, ctypes.c_float(1.5), 16, None) == -1 and b"outside" in L.mas_last_error()
    assert L.mas_dropout_apply(24, 16, 8, mas_hip.BF16, ctypes.c_float(0.1), 16, None) == -1 and b"aligned" in L.mas_last_error()
    assert L.mas_attn_dropout_mask(None, 1, 1, 8, ctypes.c_float(0.1), None, None) == -1
    assert L.mas_attn_causal_fwd_drop(1, 1, 1, 1, None, mas_hip.BF16, 1, 1, 8, 64, 192, 192, 192, 0, 0, 0, ctypes.c_float(0.125),
                                      ctypes.c_float(0.1), None, None) == -1 and b"seed" in L.mas_last_error()
    assert L.mas_attn_causal_bwd_drop(1, 1, 1, 1, 1, 1, mas_hip.BF16, 1, 1, 8, 64, ctypes.c_float(0.125), ctypes.c_float(-0.1), 16,
                                      None) == -1


def test_dropout_refuses_cpu_tensors():
    import torch
    from mas_hip import ops
    x = torch.ones(16)
    assert ops.dropout(x, 0.0) is x and ops.dropout(x, 0.5, training=False) is x     # nothing drawn
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dropout(x, 0.5)
    with pytest.raises(ValueError):
        ops.dropout(x, 1.5)
