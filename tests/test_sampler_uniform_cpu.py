"""CPU checks of the sampler's uniform (``mas_sample_uniform``, make-a-scene_amd/csrc/mas_philox.h, compiled here as host code): every one
of its values is strictly inside (0, 1) in float32 and gives a finite Gumbel perturbation -log(-log u).  A uniform of exactly 1 makes one
score +inf, and that entry then wins whatever its logit."""
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
#include <math.h>
#include <stdio.h>
#include <string.h>
static unsigned fbits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
int main() {
    /* every distinct value: bits >> 9 takes 2^23 values, the low 9 bits do not matter */
    unsigned bad = 0;
    float lo = 2.0f, hi = -1.0f, glo = INFINITY, ghi = -INFINITY;
    for (unsigned t = 0; t < (1u << 23); ++t) {
        const float u = mas_sample_uniform((t << 9) | (t & 511u));
        const float g = -logf(-logf(u));
        if (!(u > 0.0f && u < 1.0f && isfinite(g))) ++bad;
        lo = fminf(lo, u); hi = fmaxf(hi, u); glo = fminf(glo, g); ghi = fmaxf(ghi, g);
    }
    printf("%u %u %u %.9g %.9g\n", bad, fbits(lo), fbits(hi), glo, ghi);
    const unsigned ends[4] = {0u, 0xffffffffu, 0xffffffeeu, 0x000001ffu};
    for (int i = 0; i < 4; ++i) { const float u = mas_sample_uniform(ends[i]); printf("%u %u %d\n", ends[i], fbits(u), isfinite(-logf(-logf(u))) ? 1 : 0); }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_out(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to check mas_philox.h"
    d = tmp_path_factory.mktemp("uniform")
    src, exe = d / "u.cpp", d / "u"
    src.write_text(_HOST)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "make-a-scene_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")


def test_every_uniform_is_inside_the_open_interval_with_a_finite_score(host_out):
    bad, lo, hi, glo, ghi = host_out[0].split()
    assert int(bad) == 0
    lo, hi = np.uint32(int(lo)).view(np.float32), np.uint32(int(hi)).view(np.float32)
    assert lo == np.float32(2.0 ** -24) and hi == np.float32(1 - 2.0 ** -24)
    assert np.isfinite(float(glo)) and np.isfinite(float(ghi))


def test_endpoints_equal_the_numpy_restatement(host_out):
    for line in host_out[1:5]:
        bits, ub, finite = (int(v) for v in line.split())
        u = np.uint32(ub).view(np.float32)
        assert 0.0 < u < 1.0 and finite == 1
        assert float(u) == S.uniform(np.uint32(bits))                 # exact: the float32 value is the float64 one
    assert S.uniform(np.uint32(0xFFFFFFFF)) == 1 - 2.0 ** -24 and S.uniform(np.uint32(0)) == 2.0 ** -24


def test_the_counter_that_used_to_reach_one():
    """seed 12345, offset 678, row 2648, step 0, entry 6388: the word is 0xffffffee, whose top 24 bits are all ones (the GPU test
    tests/test_gpu_sampler_uniform.py samples exactly this row)"""
    assert int(S.sample_bits(12345, 678, 2648, 0, np.uint64(6388))) == 0xFFFFFFEE
    assert S.uniform(np.uint32(0xFFFFFFEE)) < 1.0
