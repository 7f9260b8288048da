"""CPU checks of the shared-prompt decode attention (``generate(num_samples=n)``): the two C entries are exported and refuse bad
arguments without a launch, ``shared_workspace_floats`` and ``resolve_prompt_splits`` as tables, the float64 restatement of "states of
the prompt ranges, then of the own ranges, merged in that order" against the plain softmax(qK^T)V over the concatenated keys, and the
argument checks of ``generate(num_samples=...)`` on a CPU model."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))
import decode_shared_ref as S  # noqa: E402
import decode_split_ref as R  # noqa: E402

MAX = 32


def test_shared_entries_are_exported_and_declared():
    import mas_hip
    hdr = open(os.path.join(ROOT, "include", "mas_hip.h")).read()
    for name in ("mas_attn_decode_shared", "mas_attn_decode_shared_dev"):
        assert name in mas_hip.EXPORTS and f"int {name}(" in hdr
        assert hasattr(mas_hip.lib(), name)
    assert mas_hip.lib().mas_abi_version() == mas_hip.ABI_VERSION == 10
    assert f"#define MAS_ATTN_DECODE_SHARED_QT {mas_hip.ATTN_DECODE_SHARED_QT}\n" in hdr and mas_hip.ATTN_DECODE_SHARED_QT in (4, 8)


def test_shared_entries_validate_arguments_without_gpu():
    """error convention: a negative code + message, nothing launched: null pointers, group < 1, rows % group != 0, prompt_len < 1,
    host past < prompt_len, either split count out of range, a workspace one float short (-4), misaligned rows (-2)"""
    import mas_hip
    L = mas_hip.lib()
    P = 4096            # any non-null 16-byte aligned address: every call below returns before it would be used
    rows, group, h, hd, plen, cap = 6, 3, 16, 64, 40, 64
    d = h * hd
    good = dict(q=P, kn=P, vn=P, pk=P, pv=P, kc=P, vc=P, o=P, past=P, rows=rows, group=group, plen=plen, nsp=2, nso=3, ws=P,
                ws_floats=rows * h * 5 * (hd + 2), host_past=plen + 7, new_bs=3 * d)

    def host(**kw):
        a = dict(good, **kw)
        return L.mas_attn_decode_shared(a["q"], a["new_bs"], a["pk"], a["pv"], d, plen * d if a["plen"] < 1 else a["plen"] * d, a["plen"],
                                        a["kc"], a["vc"], d, cap * d, cap, a["o"], d, mas_hip.BF16, a["rows"], a["group"], h, hd,
                                        a["host_past"], 0.125, a["nsp"], a["nso"], a["ws"], a["ws_floats"], None)

    def dev(**kw):
        a = dict(good, **kw)
        return L.mas_attn_decode_shared_dev(a["q"], a["kn"], a["vn"], a["new_bs"], a["pk"], a["pv"], d,
                                            plen * d if a["plen"] < 1 else a["plen"] * d, a["plen"], a["kc"], a["vc"], d, cap * d, cap,
                                            a["o"], d, mas_hip.BF16, a["rows"], a["group"], h, hd, a["past"], 0.125, a["nsp"], a["nso"],
                                            a["ws"], a["ws_floats"], None)

    err = L.mas_last_error
    for fn, name, ptrs in ((host, b"attn_decode_shared", ("q", "pk", "pv", "kc", "vc", "o")),
                           (dev, b"attn_decode_shared_dev", ("q", "kn", "vn", "pk", "pv", "kc", "vc", "o", "past"))):
        for ptr in ptrs:
            assert fn(**{ptr: None}) == -1 and b"null" in err() and name in err(), ptr
        assert fn(group=0) == -1 and b"group" in err() and name in err()
        assert fn(group=-2) == -1 and b"group" in err()
        assert fn(group=4) == -1 and b"multiple of group" in err()
        assert fn(plen=0) == -1 and b"prompt_len" in err()
        assert fn(plen=-5) == -1 and b"prompt_len" in err()
        for bad in (0, -3, MAX + 1):
            assert fn(nsp=bad, ws_floats=1 << 30) == -1 and b"nsplit_prompt" in err()
            assert fn(nso=bad, ws_floats=1 << 30) == -1 and b"nsplit_own" in err()
        assert fn(nsp=MAX, nso=MAX, ws_floats=rows * h * 2 * MAX * (hd + 2) - 1) == -4
        assert fn(ws=None) == -1 and b"workspace" in err()
        assert fn(ws_floats=good["ws_floats"] - 1) == -4 and b"workspace too small" in err() and name in err()
        assert fn(ws_floats=0) == -4
        assert fn(q=P + 2) == -2 and b"16-byte" in err()
        assert fn(pk=P + 8) == -2
        assert fn(new_bs=3 * d + 4) == -2
    assert host(host_past=plen - 1) == -1 and b"past" in err()
    assert host(host_past=0) == -1 and b"past" in err()
    assert host(host_past=plen + cap) == -1 and b"past" in err()       # the own cache holds `cap` rows: past - prompt_len < cap
    with pytest.raises(RuntimeError):
        mas_hip.check(-4, "probe")


def test_shared_workspace_and_prompt_split_tables():
    import mas_hip
    from mas_hip import decode
    qt = mas_hip.ATTN_DECODE_SHARED_QT
    cap = decode.AUTO_MAX_PROMPT_SPLITS
    assert decode.shared_workspace_floats(64, 16, 64, 2, 8) == 64 * 16 * 10 * 66
    assert decode.shared_workspace_floats(3, 2, 16, 1, 1) == 3 * 2 * 2 * 18
    assert decode.shared_workspace_floats(6, 2, 128, 5, 3) == 6 * 2 * 8 * 130
    r = decode.resolve_prompt_splits
    for n in (1, 2, 3, 5, 8, 16, MAX):
        assert r(n, 1, 8, 16, 256) == n and r(n, 64, 32, 16, 256) == n   # integers pass through whatever the chip holds
    for groups in (1, 2, 3, 4, 16):
        for group in (1, 2, qt - 1, qt, qt + 1, 8, 9, 32, 33, 100):
            for heads in (1, 2, 16):
                for n_cus in (32, 256, 304):
                    n = r("auto", groups, group, heads, n_cus)
                    blocks = groups * -(-group // qt) * heads            # the prompt work-groups of the partial launch, unsplit
                    assert 1 <= n <= cap <= 8 and n & (n - 1) == 0
                    assert n == 1 or blocks * n <= n_cus                 # the occupancy inequality (measured bound: DESIGN 2.6) holds for n ...
                    assert n == cap or blocks * 2 * n > n_cus            # ... and fails for the next power of two, up to the measured clamp
    assert r("auto", 1, 1, 1, 256) == cap == 4 and r("auto", 64, 64, 16, 256) == 1
    assert r("auto", 1, 8 * qt, 16, 256) == 2                            # 8 * 16 = 128 work-groups: twice fits, four times does not
    assert r("auto", 1, 8 * qt + 1, 16, 256) == 1                        # 144 work-groups: twice does not
    # the four measured points (one prompt, 8 / 32 candidates, plain / guided, 16 heads, 256 compute units)
    assert [r("auto", g, n, 16, 256) for n in (8, 32) for g in (1, 2)] == [4, 4, 2, 1]
    for bad in (0, -1, MAX + 1, 2.0, "8", "Auto", True, None, [2]):
        with pytest.raises(ValueError):
            r(bad, 2, 8, 16, 256)
    for zero in ((0, 8, 16, 256), (2, 0, 16, 256), (2, 8, 0, 256), (2, 8, 16, 0)):
        with pytest.raises(ValueError):
            r("auto", *zero)


@pytest.mark.parametrize("hd", [16, 64, 128])
def test_prompt_then_own_states_equal_plain_softmax(hd):
    """float64: states of the prompt ranges, then of the own ranges -- the neutral state for an empty one -- merged in that order are
    softmax(qK^T)V over the concatenated keys"""
    rng = np.random.default_rng(700 + hd)
    empties = 0
    for plen in (1, 31, 33, 300):
        for l_own in (1, 32, 71):
            q = rng.standard_normal(hd) / np.sqrt(hd)
            pk = rng.standard_normal((plen, hd)) * 3.0                   # scores spread over tens of units: the rescaling matters
            pv = rng.standard_normal((plen, hd))
            ok = rng.standard_normal((l_own, hd)) * 3.0
            ov = rng.standard_normal((l_own, hd))
            want = S.plain_shared_attention(q, pk, pv, ok, ov)
            for nsp in (1, 2, 5):
                for nso in (1, 3):
                    st = S.shared_states(q, pk, pv, ok, ov, nsp, nso)
                    assert len(st) == nsp + nso
                    empties += sum(1 for m, l, _ in st if m == R.NEUTRAL_M and l == 0.0)
                    got = S.shared_attention(q, pk, pv, ok, ov, nsp, nso)
                    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (plen, l_own, nsp, nso)
    assert empties > 0                                                   # e.g. 31 prompt keys in 5 ranges of 32: four are empty
    # an own cache of one key next to a long prompt, and the reverse
    assert R.split_ranges(1, 3)[1:] == [(32, 32), (64, 64)] and R.split_ranges(300, 5)[-1] == (256, 300)


def test_generate_num_samples_arguments_raise_on_a_cpu_model():
    from models.transformer import MakeAScene
    torch.manual_seed(0)
    m = MakeAScene(num_layers=1, hidden_dim=32, num_attn_heads=2, image_vocab_size=20, seg_vocab_size=8, text_vocab_size=30,
                   image_tokens_per_dim=2, seg_tokens_per_dim=2, text_length=4).eval()
    text = torch.randint(1, 20, (2, 4))
    seg = torch.randint(0, 8, (2, 4))
    for graph in (False, True):
        for bad in (0, -1, 2.5, True, "3"):
            with pytest.raises(ValueError, match="num_samples"):
                m.generate(text, seg, temperature=0, num_samples=bad, graph=graph)
        img = torch.randint(0, 20, (2, 4))                               # B rows where B * n = 6 are due
        with pytest.raises(ValueError, match="img_tokens"):
            m.generate(text, seg, img_tokens=img, num_samples=3, graph=graph)
        with pytest.raises(ValueError):
            m.generate(text, seg, img_tokens=img.repeat_interleave(3, 0), keep=torch.zeros(2, 4, dtype=torch.bool), num_samples=3,
                       graph=graph)
