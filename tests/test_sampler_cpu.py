"""CPU checks of the on-device sampler of ``MakeAScene.generate(graph=True)``: the numpy restatement of the sampling counter -> uniform
mapping (tests/helpers/sample_ref.py) against the header the kernel includes (make-a-scene_amd/csrc/mas_philox.h, compiled here as host
code), the selection rule (guidance mix, temperature, top-k with ties, Gumbel-max) on hand-made cases, and the argument checks of the new
C entries."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import sample_ref as S  # noqa: E402

_HOST = r'''
#include "mas_philox.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char** argv) {
    const unsigned long long seed = strtoull(argv[1], 0, 10), off = strtoull(argv[2], 0, 10);
    const unsigned row = (unsigned)strtoul(argv[3], 0, 10), step = (unsigned)strtoul(argv[4], 0, 10);
    const unsigned s0 = (unsigned)seed, s1 = (unsigned)(seed >> 32), o = (unsigned)off;
    for (int a = 5; a < argc; ++a) {
        const unsigned j = (unsigned)strtoul(argv[a], 0, 10);
        const MasU32x4 w = mas_sample_bits4(s0, s1, o, row, step, j >> 2);
        const unsigned words[4] = {w.x, w.y, w.z, w.w};
        const unsigned bits = words[j & 3];
        const float u = mas_sample_uniform(bits);
        unsigned ub; memcpy(&ub, &u, 4);
        printf("%u %u\n", bits, ub);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_sampler(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to check mas_philox.h"
    d = tmp_path_factory.mktemp("sampler")
    src, exe = d / "s.cpp", d / "s"
    src.write_text(_HOST)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "make-a-scene_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("seed,off,row,step", [(0, 0, 0, 0), (2 ** 63 - 25, 123456789012, 7, 1023), (987654321987, 4 * 2 ** 32 + 5, 15, 1),
                                               (1, 2 ** 32 - 1, 65535, 511)])
def test_numpy_mapping_equals_header(host_sampler, seed, off, row, step):
    js = [0, 1, 2, 3, 4, 5, 17, 255, 1022, 8191, 65535]
    out = subprocess.run([host_sampler, str(seed), str(off), str(row), str(step)] + [str(j) for j in js], check=True, capture_output=True,
                         text=True).stdout.split("\n")
    got = np.array([[int(x) for x in line.split()] for line in out if line.strip()], dtype=np.uint64)
    want = S.sample_bits(seed, off, row, step, np.array(js, dtype=np.uint64))
    assert (got[:, 0] == want.astype(np.uint64)).all()
    u32 = np.float32(S.uniform(want)).view(np.uint32)                   # exact in float32: the header's float equals the numpy value
    assert (got[:, 1] == u32.astype(np.uint64)).all()
    u = S.uniform(want)
    assert ((u > 0) & (u < 1)).all()


def test_mapping_separates_rows_steps_and_entries():
    j = np.arange(64, dtype=np.uint64)
    a = S.sample_bits(5, 9, 0, 0, j)
    assert len(set(a.tolist())) == 64
    for other in (S.sample_bits(5, 9, 1, 0, j), S.sample_bits(5, 9, 0, 1, j), S.sample_bits(5, 10, 0, 0, j), S.sample_bits(6, 9, 0, 0, j)):
        assert (other != a).mean() > 0.95


def test_greedy_is_first_index_of_the_maximum():
    assert S.select([1.0, 3.0, 3.0, 2.0], temperature=0)[0] == 1
    lc, lu = np.array([0.0, 1.0, 2.0], np.float32), np.array([0.0, 2.0, 0.0], np.float32)
    assert S.select(lc, lu, 3.0, temperature=0)[0] == 2               # 0 + 3 * (2 - 0) = 6 beats 2 + 3 * (1 - 2) = -1


def test_guidance_mix_is_the_fp32_expression():
    rng = np.random.default_rng(0)
    lc, lu = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    m = S.mix(lc, lu, 3.0)
    assert m.dtype == np.float32
    want = np.array([np.float32(b) + np.float32(np.float32(3.0) * np.float32(np.float32(a) - np.float32(b))) for a, b in zip(lc, lu)],
                    dtype=np.float32)
    assert np.array_equal(m, want)


def test_top_k_keeps_ties_at_the_kth_value():
    lg = np.array([5.0, 4.0, 4.0, 4.0, 1.0, 0.0], np.float32)
    assert S.kept(lg, 2).tolist() == [True, True, True, True, False, False]
    assert S.kept(lg, 1).tolist() == [True, False, False, False, False, False]
    assert S.kept(lg, 6).all() and S.kept(lg, None).all()


def test_gumbel_max_on_hand_made_uniforms():
    # -log(-log 0.9) = 2.2504, -log(-log 0.1) = -0.8340: equal logits -> the larger uniform wins
    assert S.select([0.0, 0.0], u=[0.9, 0.1])[0] == 0
    assert S.select([0.0, 0.0], u=[0.1, 0.9])[0] == 1
    # a 4-unit logit lead beats a 3.08-unit perturbation lead
    assert S.select([4.0, 0.0], u=[0.1, 0.9])[0] == 0
    # ... unless the temperature flattens it: 4 / 2 = 2 < 3.08
    assert S.select([4.0, 0.0], temperature=2.0, u=[0.1, 0.9])[0] == 1
    # top-k removes the entry with the best perturbed score
    assert S.select([1.0, 3.0, 2.0], top_k=2, u=[0.999999, 0.5, 0.5])[0] == 1
    tok, gap = S.select([0.0, 0.0, 0.0], u=[0.2, 0.7, 0.4])
    assert tok == 1 and gap == pytest.approx(-np.log(-np.log(0.7)) + np.log(-np.log(0.4)))


def test_gumbel_max_frequencies_follow_the_softmax():
    """the rule, with the mapping's uniforms, is a draw from softmax(lg) restricted to the top-k (20 000 rows, one logits row)"""
    lg = np.array([1.0, 0.5, 0.0, -0.5, 2.0, 0.0, -3.0], np.float32)
    toks, _ = S.select_rows(lg, None, None, 1.0, 5, 11, 3, 20000, 0)
    keep = S.kept(lg, 5)
    assert not np.isin(toks, np.flatnonzero(~keep)).any()
    p = np.where(keep, np.exp(lg.astype(np.float64)), 0)
    p /= p.sum()
    freq = np.bincount(toks, minlength=7) / len(toks)
    assert np.abs(freq - p).max() < 0.015


def test_new_entries_validate_arguments_without_gpu():
    sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
    import mas_hip
    L = mas_hip.lib()
    assert L.mas_attn_decode_dev(None, None, None, 0, None, None, 64, 0, 1, None, 0, mas_hip.BF16, 1, 1, 64, None, 0.125, None) == -1
    assert b"null" in L.mas_last_error()
    assert L.mas_decode_embed(None, 16, None, None, 8, None, None, 4, None, 1, 1, 64, None) == -1
    assert L.mas_sample_tokens(None, 0, 0, 1, 8, 0, 0, 0, None, None, None, 1, None, 0, None, 1, None, 0, None) == -1
    assert L.mas_decode_advance(None, 2, None) == -1
