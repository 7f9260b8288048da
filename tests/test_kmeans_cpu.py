"""CPU checks for the device k-means (csrc/kmeans.hip, include/mas_hip.h "K-means re-initialisation"): the CONDITION ON THE INPUTS that
tests/test_gpu_kmeans.py relies on, re-derived from the fp64 oracle alone (never from the code under test); the C contract's presence
inside ABI 10; the keyed bijection's shared header compiled as host C++ against its numpy restatement at stream 2; and the argument
checks that need no device."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kmeans_cases as KC  # noqa: E402
import reservoir_ref as RR  # noqa: E402

ALL = KC.all_cases()


@pytest.mark.parametrize("i", range(len(ALL)))
def test_inputs_keep_the_fp32_run_on_the_oracles_trajectory(i):
    """top-2 gap >= 128 fp32 ulps at every iteration and point (a D-term fp32 FMA chain rounds by about sqrt(D) / 2 <= 8 ulps), every
    non-zero shift >= 100 tol (so `shift <= tol` is decided far from the threshold), and the table's iteration counts and events"""
    name, pts, init = ALL[i]
    tr, cent, assign = KC.trace(pts, init)
    ref_c, ref_a, ref_it = KC.oracle(name, pts, init)
    assert len(tr) == ref_it and np.array_equal(cent, ref_c) and np.array_equal(assign, ref_a)      # the trace IS the oracle's run
    gap = min(t["gap_ulps"] for t in tr)
    shifts = [t["shift"] for t in tr]
    print(f"{name}: M={len(pts)}, {len(tr)} iterations, gap {gap:.1f} ulps, shifts {['%.3g' % s for s in shifts]}, empty {[t['empty'] for t in tr]}")
    assert gap >= KC.MIN_GAP_ULPS
    assert all(s >= KC.MIN_SHIFT_OVER_TOL * KC.TOL for s in shifts if s > 0.0) and shifts[-1] <= KC.TOL
    if i < len(KC.CASES):
        c = KC.CASES[i]
        assert len(pts) == c["M"] and pts.shape[1] == c["d"] and len(init) == c["k"] == len(set(init.tolist()))
        assert len(tr) == c["iters"] and abs(gap - c["gap"]) < 1.0
        for it, t in enumerate(tr, start=1):
            stay = set(t["empty"]).intersection(*[set(u["empty"]) for u in tr[it - 1:]])
            want = sum(n for first, n in c["empties"].items() if it >= first)
            assert len(stay) == want, (it, t["empty"])
        for k in tr[-1]["empty"]:
            assert not ref_c[k].any()
    else:
        # the duplicate initial centroid: the higher index never wins the tie, so cluster 1 holds nothing at any iteration and is the zero vector
        assert init[1] == init[0] and all(1 in t["empty"] for t in tr) and not ref_c[1].any() and 1 not in ref_a


def test_capped_case_stops_unconverged_in_the_oracle():
    name, pts, init = ALL[KC.CAPPED]
    tr, _, _ = KC.trace(pts, init, max_iter=2)
    assert len(tr) == 2 and tr[-1]["shift"] > KC.TOL and KC.oracle(name, pts, init, 2)[2] == 2
    assert min(t["shift"] for t in KC.trace(pts, init)[0] if t["shift"] > 0) == pytest.approx(9.24, abs=0.01)


def test_header_declares_the_entries_inside_abi_10():
    import ctypes as C
    import mas_hip
    assert mas_hip.ABI_VERSION == 10
    sig = mas_hip._SIGNATURES
    assert {"mas_kmeans_workspace", "mas_kmeans_init", "mas_kmeans_fit"} <= set(mas_hip.EXPORTS)
    assert sig["mas_kmeans_workspace"] == (C.c_size_t, [C.c_int, C.c_int])
    assert sig["mas_kmeans_init"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    assert sig["mas_kmeans_fit"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    # the entries that were there keep their place in front of them
    assert mas_hip.EXPORTS.index("mas_reservoir_collect") < mas_hip.EXPORTS.index("mas_kmeans_workspace")


_HOST = r'''
#include "mas_bijection.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
    const unsigned long long seed = strtoull(argv[1], 0, 10);
    const unsigned N = atoi(argv[2]), K = atoi(argv[3]), calls = atoi(argv[4]);
    for (unsigned x = 0; x < K; ++x) printf("%u\n", rsv_perm(x, N, rsv_half_bits(N), 2u, calls, (unsigned)seed, (unsigned)(seed >> 32)));
    return 0;
}
'''


def test_shared_bijection_header_on_the_host_at_stream_2(tmp_path):
    """csrc/mas_bijection.h (the one copy reservoir.hip and kmeans.hip include) as host C++: the initial rows P(0) .. P(K-1)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to check mas_bijection.h"
    csrc = os.path.join(ROOT, "make-a-scene_amd", "csrc")
    for f in ("reservoir.hip", "kmeans.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "mas_bijection.h"' in text and "rsv_feistel(uint32_t x" not in text, f        # no second copy
    src, exe = tmp_path / "b.cpp", tmp_path / "b"
    src.write_text(_HOST)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", csrc, str(src), "-o", str(exe)], check=True)
    for seed, M, K, draw in [(77, 403, 45, 0), (77, 403, 45, 6), (0x9E3779B97F4A7C15, 70, 48, 3), (2 ** 62 + 12345, 70, 70, 11), (1, 1, 1, 0),
                             (5, 12500, 300, 9000)]:
        out = subprocess.run([str(exe), str(seed), str(M), str(K), str(draw)], check=True, capture_output=True, text=True).stdout
        got = [int(v) for v in out.split()]
        assert got == RR.perm(np.arange(K), M, 2, draw, seed).tolist(), (seed, M, K, draw)
        assert len(set(got)) == K and max(got) < M


def test_argument_checks_without_a_device(monkeypatch):
    import mas_hip
    from mas_hip import ops
    from models import kmeans as KM
    from models.modules import Codebook
    L = mas_hip.lib()
    a = 1 << 20                                               # any non-null, 16-byte aligned address: the checks look at no memory
    fit = lambda M, K, D, it, p=a, ws=1 << 40: L.mas_kmeans_fit(p, a, M, K, D, it, 1e-4, a, a, a, a, ws, None)
    assert fit(400, 40, 512, 10) == -2 and b"{32,64,128,256}" in L.mas_last_error()
    assert fit(400, 40, 48, 10) == -2
    assert fit(40, 41, 32, 10) == -1 and b"K <= M" in L.mas_last_error()
    assert fit(40, 0, 32, 10) == -1
    assert fit(400, 40, 32, 0) == -1 and b"max_iter" in L.mas_last_error()
    assert fit(400, 40, 32, 10, p=a + 4) == -1 and b"16-byte" in L.mas_last_error()
    assert fit(400, 40, 32, 10, p=None) == -1 and b"null" in L.mas_last_error()
    assert fit(400, 40, 32, 10, ws=L.mas_kmeans_workspace(400, 40) - 1) == mas_hip.EWORKSPACE == -4
    assert L.mas_kmeans_init(a, 40, 41, 32, 1, 0, a, None, None) == -1 and b"K <= M" in L.mas_last_error()
    assert L.mas_kmeans_init(a, 400, 40, 100, 1, 0, a, None, None) == -2
    assert L.mas_kmeans_init(a + 8, 400, 40, 32, 1, 0, a, None, None) == -1 and b"16-byte" in L.mas_last_error()
    # the workspace holds the lookup's own layout and the fp64 partials behind it
    assert L.mas_kmeans_workspace(403, 45) >= 4 * (403 + 45 + 2 * 403 * 64) + 8 * 6
    pts = torch.zeros(40, 32)
    with pytest.raises(ValueError, match="256"):
        ops.kmeans_fit(torch.zeros(40, 512), 8, seed=1)
    with pytest.raises(ValueError, match="n_clusters <= M"):
        ops.kmeans_fit(pts, 41, seed=1)
    with pytest.raises(ValueError, match="either init_idx"):
        ops.kmeans_fit(pts, 8)
    with pytest.raises(ValueError, match="either init_idx"):
        ops.kmeans_fit(pts, 8, seed=1, init_idx=torch.arange(8))
    with pytest.raises(ValueError, match="max_iter"):
        ops.kmeans_fit(pts, 8, seed=1, max_iter=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_fit(pts, 8, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KM.kmeans_fit(pts, 8, on_device=True, seed=1)
    monkeypatch.delenv("MAS_KMEANS_DEVICE", raising=False)
    assert KM.device_default() is False
    monkeypatch.setenv("MAS_KMEANS_DEVICE", "1")
    assert KM.device_default() is True
    monkeypatch.setenv("MAS_KMEANS_DEVICE", "0")
    assert KM.device_default() is False
    cb = Codebook(64, 32, beta=0.25, init_steps=2, reservoir_size=64)
    with pytest.raises(RuntimeError, match="enable_device_reservoir"):
        cb.enable_device_reservoir(seed=3, device_kmeans=True)
    assert not cb.device_reservoir
