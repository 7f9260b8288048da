"""CPU-side checks of the chunked spatial-attention entries (``mas_spatial_attn_flash_fwd / _bwd``): exported, declared in
include/mas_hip.h and bound; bad arguments come back as a negative code with a message and nothing is launched; the entries they
stand beside keep their envelope and the ABI keeps its version."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mas_spatial_attn_flash_fwd", "mas_spatial_attn_flash_bwd")


def test_entries_are_exported_declared_and_bound():
    import mas_hip
    txt = open(os.path.join(ROOT, "include", "mas_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mas_[a-z0-9_]+)\s*\(", txt))
    raw = ctypes.CDLL(mas_hip.LIB_PATH)
    for s in NEW:
        assert s in declared, f"{s} not declared in include/mas_hip.h"
        assert hasattr(raw, s), f"{s} not exported"
        assert s in mas_hip.EXPORTS, f"{s} not in the ctypes table"
        assert getattr(mas_hip.lib(), s).restype is ctypes.c_int
    assert len(mas_hip.lib().mas_spatial_attn_flash_fwd.argtypes) == 8 and len(mas_hip.lib().mas_spatial_attn_flash_bwd.argtypes) == 11


def test_argument_validation_without_gpu():
    import mas_hip
    L = mas_hip.lib()
    bf16, f32 = mas_hip.BF16, mas_hip.F32
    assert L.mas_spatial_attn_flash_fwd(None, 1, None, bf16, 1, 1024, 512, None) == -1 and b"null" in L.mas_last_error()
    assert L.mas_spatial_attn_flash_fwd(1, None, None, bf16, 1, 1024, 512, None) == -1
    assert L.mas_spatial_attn_flash_bwd(1, None, 1, 1, 1, 1, bf16, 1, 1024, 512, None) == -1       # the saved output
    assert L.mas_spatial_attn_flash_bwd(1, 1, 1, None, 1, 1, bf16, 1, 1024, 512, None) == -1       # lse
    assert L.mas_spatial_attn_flash_bwd(1, 1, 1, 1, None, 1, bf16, 1, 1024, 512, None) == -1       # delta
    assert L.mas_spatial_attn_flash_bwd(1, 1, 1, 1, 1, None, bf16, 1, 1024, 512, None) == -1       # dqkv
    for fwd in (True, False):
        def call(dtype, s, c):
            if fwd:
                return L.mas_spatial_attn_flash_fwd(1, 1, None, dtype, 1, s, c, None)
            return L.mas_spatial_attn_flash_bwd(1, 1, 1, 1, 1, 1, dtype, 1, s, c, None)
        assert call(f32, 1024, 512) == -2 and b"bf16" in L.mas_last_error()
        assert call(bf16, 4097, 64) == -2 and b"4096" in L.mas_last_error()
        assert call(bf16, 1024, 48) == -2
        assert call(bf16, 1024, 544) == -2
        assert call(bf16, 0, 64) == -2
    with __import__("pytest").raises(RuntimeError):
        mas_hip.check(L.mas_spatial_attn_flash_fwd(1, 1, None, bf16, 1, 4097, 64, None), "probe")


def test_the_shipped_entries_and_the_abi_version_are_unchanged():
    import mas_hip
    L = mas_hip.lib()
    assert L.mas_abi_version() == mas_hip.ABI_VERSION == 10
    assert L.mas_spatial_attn_fwd(1, 1, None, mas_hip.BF16, 1, 300, 64, None) == -2 and b"256" in L.mas_last_error()
    assert L.mas_spatial_attn_bwd(1, 1, 1, 1, 1, mas_hip.BF16, 1, 300, 64, None) == -2


def test_switch_reads_the_environment_at_call_time_and_returns_the_previous_value(monkeypatch):
    from mas_hip import ops
    saved = ops._sp_flash["on"]
    try:
        for env, want in (("1", True), ("0", False)):
            ops._sp_flash["on"] = None                       # as after import: nothing has asked yet
            monkeypatch.setenv("MAS_SP_FLASH", env)
            assert ops.set_spatial_flash(not want) is want
            assert ops.set_spatial_flash(want) is (not want)
    finally:
        ops._sp_flash["on"] = saved
