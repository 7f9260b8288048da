"""CPU checks of image prompts (``MakeAScene.generate(img_tokens=..., keep=...)``): the border mask and the common prefix of
models/image_prompt.py against masks written out by hand, the new sampler entry ``mas_sample_tokens_prompt`` in the library and its
argument checks, and ``generate``'s validation of the mask."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))


def _grid(rows):
    return torch.tensor([[c == "#" for c in r] for r in rows], dtype=torch.bool).reshape(-1)


@pytest.mark.parametrize("borders,rows", [
    (dict(), ["....", "....", "....", "...."]),
    (dict(up=1), ["####", "....", "....", "...."]),
    (dict(down=2), ["....", "....", "####", "####"]),
    (dict(left=1), ["#...", "#...", "#...", "#..."]),
    (dict(right=3), [".###", ".###", ".###", ".###"]),
    (dict(up=2, left=1), ["####", "####", "#...", "#..."]),
    (dict(up=1, down=1, left=1, right=1), ["####", "#..#", "#..#", "####"]),
    (dict(up=4), ["####", "####", "####", "####"]),
    (dict(right=9), ["####", "####", "####", "####"]),
], ids=["none", "up", "down", "left", "right", "up+left", "frame", "up=grid", "right>grid"])
def test_border_keep_mask_against_hand_written_masks(borders, rows):
    from models import border_keep_mask
    got = border_keep_mask(4, **borders)
    assert got.dtype == torch.bool and got.shape == (16,)
    assert torch.equal(got, _grid(rows))


def test_border_keep_mask_rejects_bad_borders():
    from models import border_keep_mask
    for bad in (dict(up=-1), dict(left=1.5), dict(down=True)):
        with pytest.raises(ValueError):
            border_keep_mask(4, **bad)
    with pytest.raises(ValueError):
        border_keep_mask(0)


def test_common_prefix():
    from models import common_prefix
    L = 16
    keep = torch.zeros((2, L), dtype=torch.bool)
    assert common_prefix(keep) == 0
    keep[0, :3] = True
    keep[1, :5] = True
    keep[0, 7] = keep[1, 9] = True                  # kept positions behind the run do not count
    assert common_prefix(keep) == 3
    assert common_prefix(torch.ones((2, L), dtype=torch.bool)) == L - 1
    one = torch.zeros((2, L), dtype=torch.bool)
    one[1, 0] = True
    assert common_prefix(one) == 0
    with pytest.raises(ValueError):
        common_prefix(torch.ones((2, L)))


def _entry_args(mode, forced, keep, L=4, ld_keep=None):
    """(buffers kept alive, argument tuple) of a mas_sample_tokens_prompt call on host buffers: the checks under test reject the call
    before anything is launched"""
    f32, i64, i32, u8 = ctypes.c_float, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint8
    bufs = dict(logits=(f32 * 8)(), params=(f32 * 3)(), seed=(i64 * 2)(), step=(i32 * 1)(), forced=(i64 * L)(), tokens=(i64 * L)(),
                keep=(u8 * L)())
    ptr = lambda name: ctypes.cast(bufs[name], ctypes.c_void_p)
    args = (ptr("logits"), 8, 0, 1, 8, 0, mode, 0, ptr("params"), ptr("seed"), ptr("step"), L, ptr("forced") if forced else None, L,
            ptr("tokens"), L, None, 0, ptr("keep") if keep else None, L if ld_keep is None else ld_keep, None)
    return bufs, args


def test_prompt_entry_is_exported_and_validates_arguments_without_gpu():
    import mas_hip
    L = mas_hip.lib()
    assert L.mas_abi_version() == mas_hip.ABI_VERSION == 10
    assert "mas_sample_tokens_prompt" in mas_hip.EXPORTS and hasattr(L, "mas_sample_tokens_prompt")
    for mode, forced, keep, ld_keep, word in ((0, False, True, None, b"kept tokens"), (1, False, True, None, b"kept tokens"),
                                              (0, True, False, None, b"mask"), (2, True, True, None, b"mode 2"),
                                              (1, True, True, 3, b"at least L")):
        bufs, args = _entry_args(mode, forced, keep, ld_keep=ld_keep)
        assert L.mas_sample_tokens_prompt(*args) == -1, (mode, forced, keep)
        assert word in L.mas_last_error(), L.mas_last_error()


def test_binding_rejects_keep_without_forced_and_with_teacher_forcing():
    from mas_hip import decode
    logits = torch.zeros((1, 8))
    tokens = torch.zeros((1, 4), dtype=torch.long)
    step = torch.zeros(1, dtype=torch.int32)
    params = torch.ones(3)
    keep = torch.ones((1, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="keep needs the forced tokens"):
        decode.sample_tokens(logits, tokens, step, params, decode.GREEDY, keep=keep)
    with pytest.raises(RuntimeError, match="FORCED keeps every position"):
        decode.sample_tokens(logits, tokens, step, params, decode.FORCED, forced=tokens.clone(), keep=keep)


def _tiny():
    from models.transformer import MakeAScene
    m = MakeAScene(num_layers=1, hidden_dim=32, num_attn_heads=2, image_vocab_size=16, seg_vocab_size=5, text_vocab_size=20,
                   image_tokens_per_dim=2, seg_tokens_per_dim=1, text_length=4).eval()
    return m, torch.ones((1, 4), dtype=torch.long), torch.zeros((1, 1), dtype=torch.long)


@pytest.mark.parametrize("graph", [False, True])
def test_generate_rejects_a_bad_mask_before_touching_the_device(graph):
    m, text, seg = _tiny()
    img = torch.zeros((1, 4), dtype=torch.long)
    ok = torch.ones((1, 4), dtype=torch.bool)
    with pytest.raises(ValueError, match="img_tokens"):
        m.generate(text, seg, keep=ok, graph=graph)
    for bad in (torch.ones((1, 3), dtype=torch.bool), torch.ones((2, 4), dtype=torch.bool), torch.ones(4, dtype=torch.bool),
                torch.ones((1, 4)), torch.ones((1, 4), dtype=torch.uint8), [[True] * 4]):
        with pytest.raises(ValueError, match="keep"):
            m.generate(text, seg, img_tokens=img, keep=bad, graph=graph)
    with pytest.raises(ValueError, match="img_tokens"):
        m.generate(text, seg, img_tokens=img[:, :3], keep=ok, graph=graph)
