"""CPU checks of the device reservoir's rule (include/mas_hip.h, "Codebook reservoir") on its numpy restatement
(tests/helpers/reservoir_ref.py): positions and drop sets are distinct by construction, a candidate survives a full reservoir with
frequency R / (R + n) and every slot is replaced equally often -- the bounds tests/test_gpu_reservoir.py then holds the kernel to --
the C++ bijection (csrc/reservoir.hip's arithmetic, compiled as host code from mas_philox.h) against the restatement, and the argument
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
import reservoir_ref as RR  # noqa: E402

SEEDS = (1, 0x9E3779B97F4A7C15, 2 ** 62 + 12345)
# survival: 40 000 candidates, p = 64 / 84, sigma <= 0.5 / sqrt(40 000) = 0.0025 (the binomial bound): 5 sigma < 0.0125
# replacement: 2000 calls, a slot is among the 20 dropped of 84 with p = 20 / 84: 476 expected, sigma = sqrt(2000 p (1 - p)) = 19
FREQ = dict(R=64, B=2, HW=16, calls=2000, survive=64 / 84, survive_tol=0.012, replaced=2000 * 20 / 84, replaced_tol=100)


@pytest.mark.parametrize("HW", [10, 16, 100, 256])
def test_positions_are_ten_distinct_positions(HW):
    for seed in SEEDS:
        for calls in range(50):
            pos = RR.perm(np.arange(10), HW, 0, calls, seed)
            assert len(set(pos.tolist())) == 10 and pos.min() >= 0 and pos.max() < HW
    # and over many calls every position is drawn (HW = 10: always all of them)
    seen = set()
    for calls in range(200):
        seen |= set(RR.perm(np.arange(10), HW, 0, calls, SEEDS[0]).tolist())
    assert seen == set(range(HW))


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 16, 17, 84, 255, 256, 257, 1000])
def test_the_bijection_is_one(N):
    for seed in SEEDS[:2]:
        for stream in (0, 1):
            y = RR.perm(np.arange(N), N, stream, 7, seed)
            assert sorted(y.tolist()) == list(range(N))
    assert 4 ** RR.half_bits(N) >= N and (RR.half_bits(N) == 1 or 4 ** (RR.half_bits(N) - 1) < N)


@pytest.mark.parametrize("R,B", [(20, 1), (20, 2), (64, 2), (64, 3), (70, 2), (70, 3), (30, 3), (10, 1)])
def test_drop_sets_and_slots(R, B):
    """over a sequence of calls from empty: the drop set has m - R distinct members, every surviving candidate gets its own slot, free
    slots first and in order, then the dropped old rows' slots in draw order; c = min(R, 10 B k)"""
    n, c = 10 * B, 0
    for k in range(12):
        pos, drop, dst, src, c_new = RR.plan(SEEDS[1], k, c, R, B, 16)
        m = c + n
        assert len(drop) == max(m - R, 0) == len(set(drop.tolist())) and all(0 <= x < m for x in drop)
        alive = dst[dst >= 0]
        assert len(set(alive.tolist())) == len(alive) == n - int((drop >= c).sum()) and c_new == min(R, m) == min(R, n * (k + 1))
        free = list(range(c, R))
        assert alive.tolist()[:len(free)] == free[:len(alive)]
        if m > R:
            assert alive.tolist()[len(free):] == [int(x) for x in drop if x < c] and len(alive) >= len(free)
        assert all(dst[i] == -1 for i in (drop[drop >= c] - c)) and alive.max() < R
        assert src.tolist() == [(i // 10) * 16 + int(pos[i % 10]) for i in range(n)]
        c = c_new


def frequencies(plans, R, n):
    """(fraction of candidates that survived, replacements per slot) over plans = [(drop, dst), ...] of full-reservoir calls"""
    survived, replaced = 0, np.zeros(R, dtype=np.int64)
    for drop, dst in plans:
        survived += int((dst >= 0).sum())
        replaced[dst[dst >= 0]] += 1
    return survived / (n * len(plans)), replaced


@pytest.mark.parametrize("seed", SEEDS)
def test_survival_and_replacement_frequencies(seed):
    f = FREQ
    plans = []
    for k in range(f["calls"]):
        _, drop, dst, _, c = RR.plan(seed, k, f["R"], f["R"], f["B"], f["HW"])
        assert c == f["R"] and len(drop) == 20
        plans.append((drop, dst))
    survive, replaced = frequencies(plans, f["R"], 10 * f["B"])
    print(f"seed {seed:#x}: survival {survive:.4f} (expected {f['survive']:.4f}), replacements per slot {replaced.min()} .. {replaced.max()}")
    assert abs(survive - f["survive"]) <= f["survive_tol"]
    assert np.abs(replaced - f["replaced"]).max() <= f["replaced_tol"]


_HOST = r'''
#include "mas_philox.h"
#include <stdio.h>
#include <stdlib.h>
%s
int main(int argc, char** argv) {
    const unsigned long long seed = strtoull(argv[1], 0, 10);
    const unsigned N = atoi(argv[2]), stream = atoi(argv[3]), calls = atoi(argv[4]);
    for (unsigned x = 0; x < N; ++x) printf("%%u\n", rsv_perm(x, N, rsv_half_bits(N), stream, calls, (unsigned)seed, (unsigned)(seed >> 32)));
    return 0;
}
'''


def test_restatement_matches_the_kernels_own_arithmetic(tmp_path):
    """the three functions between the markers of csrc/reservoir.hip, compiled as host C++"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to check reservoir.hip's bijection"
    text = open(os.path.join(ROOT, "make-a-scene_amd", "csrc", "reservoir.hip")).read()
    body = text[text.index("MAS_HD uint32_t rsv_half_bits"):text.index("// exclusive scan")]
    src, exe = tmp_path / "r.cpp", tmp_path / "r"
    src.write_text(_HOST % ("#define RSV_ROUNDS 4\n" + body))
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "make-a-scene_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    for seed, N, stream, calls in [(SEEDS[0], 84, 1, 0), (SEEDS[1], 16, 0, 5), (SEEDS[2], 257, 1, 123456), (SEEDS[1], 3, 1, 2), (SEEDS[2], 100, 0, 9)]:
        out = subprocess.run([str(exe), str(seed), str(N), str(stream), str(calls)], check=True, capture_output=True, text=True).stdout
        assert [int(v) for v in out.split()] == RR.perm(np.arange(N), N, stream, calls, seed).tolist(), (seed, N, stream, calls)


def test_argument_checks_without_a_device():
    import mas_hip
    from mas_hip import graphs, ops
    from models.modules import Codebook
    L = mas_hip.lib()
    assert mas_hip.RESERVOIR_PER_IMAGE == ops.RESERVOIR_PER_IMAGE == RR.PER_IMAGE == 10 and mas_hip.ABI_VERSION == 10
    # (z, buf, state, plan, seed, R, B, HW, D, stream): shapes first, before any pointer is looked at
    assert L.mas_reservoir_collect(None, None, None, None, 1, 64, 2, 9, 32, None) == -1 and b"positions" in L.mas_last_error()
    assert L.mas_reservoir_collect(None, None, None, None, 1, 19, 2, 16, 32, None) == -1 and b"exceed" in L.mas_last_error()
    assert L.mas_reservoir_collect(None, None, None, None, 1, 64, 2, 16, 30, None) == -1 and b"multiple of 4" in L.mas_last_error()
    assert L.mas_reservoir_collect(None, None, None, None, 1, 1 << 20, 205, 16, 32, None) == -2
    assert L.mas_reservoir_collect(None, None, None, None, 1, 64, 2, 16, 32, None) == -1 and b"null" in L.mas_last_error()
    z, buf, state = torch.zeros(2, 16, 32), torch.zeros(64, 32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="reservoir_collect"):
        ops.reservoir_collect(torch.zeros(2, 9, 32), buf, state, 1)
    with pytest.raises(ValueError, match="reservoir_collect"):
        ops.reservoir_collect(z, torch.zeros(19, 32), state, 1)
    with pytest.raises(ValueError, match="reservoir_collect"):
        ops.reservoir_collect(torch.zeros(2, 16, 30), torch.zeros(64, 30), state, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.reservoir_collect(z, buf, state, 1)
    cb = Codebook(64, 32, beta=0.25, init_steps=2, reservoir_size=64)
    keys = list(cb.state_dict())
    with pytest.raises(RuntimeError, match="enable_device_reservoir"):
        cb.enable_device_reservoir(seed=3)
    assert not cb.device_reservoir and list(cb.state_dict()) == keys == ["embedding.weight"]
    assert [cb.phase(q) for q in (1, 2, 3, 5, 6, 7)] == [0, 0, 1, 1, 2, 2]
    for bad, err in ((0, ValueError), (-2, ValueError), (2.0, TypeError), ("3", TypeError), (True, TypeError), (None, TypeError)):
        with pytest.raises(err, match="accumulate"):
            graphs.GraphedTrainStep(lambda x: x.sum(), None, torch.zeros(1), accumulate=bad)


def test_host_reservoir_schedule_call_by_call(monkeypatch):
    """the host-reservoir training forward over 70 calls (init_steps = 2: past q_re_end = 60): per call, whether the reservoir grew,
    whether the call returned unquantised, whether the re-initialisation ran -- against the schedule written out from the four
    constants.  The lookup kernel has no CPU path: it is stubbed (the schedule is decided before it is reached)."""
    from mas_hip import ops
    from models.modules import Codebook
    cb = Codebook(64, 32, beta=0.25, init_steps=2, reservoir_size=64).train()
    assert (cb.q_start_collect, cb.q_init, cb.q_re_end, cb.q_re_step) == (2, 6, 60, 1)
    fired = []
    monkeypatch.setattr(cb, "_reinit_from_reservoir", lambda: fired.append(cb.q_counter))
    monkeypatch.setattr(ops, "vq_lookup", lambda z, w, beta: (z, z.new_tensor(0), torch.zeros(z.numel() // z.shape[1], dtype=torch.long)))
    gen = torch.Generator().manual_seed(9)
    for q in range(1, 71):
        before, n_fired = cb.reservoir, len(fired)
        _, _, idx = cb(torch.randn(2, 32, 4, 4, generator=gen))
        assert cb.q_counter == q
        # a collecting call takes 20 rows into a reservoir of 64: 20, 40, 60, then full -- and a new tensor every time, full or not
        assert (cb.reservoir is not before) == (q > cb.q_start_collect) == (q > 2), q
        assert (0 if cb.reservoir is None else cb.reservoir.shape[0]) == min(64, 20 * max(q - 2, 0)), q
        assert (idx is None) == (q < 6), q
        assert (len(fired) > n_fired) == (6 <= q < 60 and (q - 6) % 1 == 0), q
    assert fired == list(range(6, 60))
