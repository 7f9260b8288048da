"""CPU checks of the split-key decode attention (``generate(kv_splits=...)``): the ``resolve_kv_splits`` rule, the argument checks of the
two C entries, and the float64 restatement of "split the keys, merge the states in split order" against the plain softmax(qK^T)V."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import decode_split_ref as R  # noqa: E402

MAX = 32


def test_resolve_kv_splits_table():
    import mas_hip
    from mas_hip import decode
    assert mas_hip.ATTN_DECODE_MAX_SPLITS == MAX
    hdr = open(os.path.join(ROOT, "include", "mas_hip.h")).read()
    assert f"#define MAS_ATTN_DECODE_MAX_SPLITS {MAX}\n" in hdr
    r = decode.resolve_kv_splits
    assert r(None, 2, 16, 256) == 1
    for n in (1, 2, 3, 8, 16, MAX):
        assert r(n, 2, 16, 256) == n and r(n, 512, 16, 256) == n          # integers pass through whatever the chip holds
    # "auto": the largest power of two n with rows * heads * n <= 2 * n_cus, within [1, 8] (the measured rule)
    assert decode.AUTO_MAX_SPLITS == 8
    for rh in range(1, 513):
        for rows, heads in ((rh, 1), (1, rh)) + (((rh // 16, 16),) if rh % 16 == 0 else ()):
            n = r("auto", rows, heads, 256)
            assert 1 <= n <= 8 and n & (n - 1) == 0
            assert n == 1 or rh * n <= 512
            assert n == 8 or rh * 2 * n > 512
            if rh > 256:
                assert n == 1                                               # beyond twice the chip: the unsplit kernel
    assert [r("auto", rows, 16, 256) for rows in (1, 2, 4, 8, 16, 32, 64)] == [8, 8, 8, 4, 2, 1, 1]
    assert r("auto", 1, 1, 256) == 8 and r("auto", 8, 16, 304) == 4 and r("auto", 1, 16, 32) == 4
    for bad in (0, -1, MAX + 1, 2.0, "8", "Auto", True, [2]):
        with pytest.raises(ValueError):
            r(bad, 2, 16, 256)
    with pytest.raises(ValueError):
        r("auto", 0, 16, 256)
    assert decode.split_workspace_floats(2, 16, 64, 8) == 2 * 16 * 8 * 66


def test_split_entries_validate_arguments_without_gpu():
    """error convention: negative code + message, nothing launched: nsplit < 1, nsplit above the maximum, null workspace, a workspace
    smaller than rows * H * nsplit * (hd + 2) floats, nq != 1, null tensors"""
    import mas_hip
    L = mas_hip.lib()
    assert {"mas_attn_decode_split", "mas_attn_decode_split_dev"} <= set(mas_hip.EXPORTS)
    assert L.mas_abi_version() == mas_hip.ABI_VERSION == 10
    P = 4096            # any non-null 16-byte aligned address: every call below returns before it would be used
    b, h, hd = 2, 16, 64

    def host(nsplit, ws, ws_floats, nq=1, q=P):
        return L.mas_attn_decode_split(q, P, P, P, mas_hip.BF16, b, h, nq, 5, hd, 3072, 1024, 1024, 1024, 3072, 1 << 20, 1 << 20, 1024,
                                       0.125, nsplit, ws, ws_floats, None)

    def dev(nsplit, ws, ws_floats, past=P):
        return L.mas_attn_decode_split_dev(P, P, P, 3072, P, P, 1024, 1536 * 1024, 1536, P, 1024, mas_hip.BF16, b, h, hd, past, 0.125,
                                           nsplit, ws, ws_floats, None)

    need = b * h * 8 * (hd + 2)
    for fn, name in ((host, b"attn_decode_split"), (dev, b"attn_decode_split_dev")):
        assert fn(0, P, need) == -1 and b"nsplit" in L.mas_last_error() and name in L.mas_last_error()
        assert fn(-3, P, need) == -1 and b"nsplit" in L.mas_last_error()
        assert fn(MAX + 1, P, 1 << 30) == -1 and b"nsplit" in L.mas_last_error()
        assert fn(8, None, need) == -1 and b"workspace" in L.mas_last_error()
        assert fn(8, P, need - 1) == -4 and b"workspace too small" in L.mas_last_error()
        assert fn(8, P, 0) == -4
    assert host(8, P, need, nq=2) == -1 and b"nq" in L.mas_last_error()
    assert host(8, P, need, nq=0) == -1
    assert host(8, P, need, q=None) == -1 and b"null" in L.mas_last_error()
    assert dev(8, P, need, past=None) == -1 and b"null" in L.mas_last_error()
    assert L.mas_attn_decode_split(P + 2, P, P, P, mas_hip.BF16, b, h, 1, 5, hd, 3072, 1024, 1024, 1024, 3072, 1 << 20, 1 << 20, 1024,
                                   0.125, 8, P, need, None) == -2                       # rows 16-byte aligned
    with pytest.raises(RuntimeError):
        mas_hip.check(-4, "probe")
    assert isinstance(ctypes.c_size_t(need).value, int)


def test_split_ranges_cover_the_keys_once():
    for L in (1, 2, 31, 32, 33, 64, 256, 257, 1001, 1535, 1536):
        for n in (1, 2, 3, 5, 8, 16, MAX):
            rg = R.split_ranges(L, n)
            assert len(rg) == n and rg[0][0] == 0
            keys = [k for b, e in rg for k in range(b, e)]
            assert keys == list(range(L)), (L, n)
            assert all((e - b) % R.GRAN == 0 for b, e in rg if e < L)          # every range but the last with keys is whole granules
            owners = [s for s, (b, e) in enumerate(rg) if b <= L - 1 < e]
            assert len(owners) == 1                                             # exactly one split appends key `past` = L - 1
    assert R.split_ranges(1535, 16)[-1] == (1440, 1535) and R.split_ranges(1, 8)[1:] == [(32 * s, 32 * s) for s in range(1, 8)]


@pytest.mark.parametrize("hd", [16, 64, 128])
def test_split_then_merge_equals_plain_softmax(hd):
    """float64: splitting the keys, keeping (m, l, o) per split -- the neutral state for an empty one -- and merging in split order is
    softmax(qK^T)V"""
    rng = np.random.default_rng(hd)
    for L in (1, 2, 64, 65, 256, 1001, 1535):
        q = rng.standard_normal(hd) / np.sqrt(hd)
        k = rng.standard_normal((L, hd)) * 3.0                                  # scores spread over tens of units: the rescaling matters
        v = rng.standard_normal((L, hd))
        want = R.plain_attention(q, k, v)
        for n in (1, 2, 3, 8, 16, MAX):
            got = R.split_attention(q, k, v, n)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (L, n)
    # an empty split is neutral wherever it stands in the order
    st = [R.partial_state(q, k, v, 0, 700), (R.NEUTRAL_M, 0.0, np.zeros(hd)), R.partial_state(q, k, v, 700, L)]
    assert np.abs(R.combine(st) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
