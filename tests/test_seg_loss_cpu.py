"""CPU side of the VQ-SEG objective on HIP (csrc/seg_loss.hip, ``mas_hip.ops.seg_loss``): the float64 restatement that the GPU tests
measure against reproduces the reference's own classes (tests/golden/loss_seg.npz, made by tests/golden/make_golden_r6.py); header,
library and binding carry the new entry points under the unchanged ABI version; CPU tensors keep to the torch expression."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests", "golden")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import seg_loss_ref as R  # noqa: E402
from make_golden_r6 import loss_seg_inputs  # noqa: E402

ENTRY_POINTS = ("mas_seg_loss_blocks", "mas_seg_loss_fwd", "mas_seg_loss_reduce", "mas_seg_loss_bwd")


@pytest.mark.parametrize("cw", [1.0, 0.25])
@pytest.mark.parametrize("name,mse", [("BCELossWithQuant", False), ("VQVAEWithBCELoss", True)])
def test_fp64_helper_reproduces_the_reference_fixture(name, mse, cw):
    """loss within 1e-6, gradient within 2^-23 of its largest element (measured: 5e-8, and 1.1e-10 against 9.8e-4: the fixture's fp32)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "loss_seg.npz"))
    pred, target, qloss = loss_seg_inputs()
    loss, _, _, dx = R.seg_loss_ref(pred, target, g[f"{name}:weight"], mse)
    ref_loss, ref_dx = float(g[f"{name}:{cw}:loss"]), g[f"{name}:{cw}:grad"].astype(np.float64)
    e_loss, e_dx = abs(loss + cw * float(qloss) - ref_loss), float(np.abs(dx - ref_dx).max())
    print(f"{name} cw={cw}: loss err {e_loss:.2e}, grad err {e_dx:.2e} of max {np.abs(ref_dx).max():.2e}")
    assert e_loss <= 1e-6
    assert e_dx <= 2.0 ** -23 * float(np.abs(ref_dx).max())
    assert np.array_equal(R.module_weight(), g[f"{name}:weight"])


def test_entry_points_in_header_library_and_binding():
    import mas_hip
    if not os.path.exists(mas_hip.LIB_PATH):
        from mas_hip import build
        build.build(verbose=False)
    txt = open(os.path.join(ROOT, "include", "mas_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mas_[a-z0-9_]+)\s*\(", txt))
    L = ctypes.CDLL(mas_hip.LIB_PATH)
    for s in ENTRY_POINTS:
        assert s in declared, f"{s} not declared in include/mas_hip.h"
        assert hasattr(L, s), f"{s} not exported by libmas_hip.so"
        assert s in mas_hip.EXPORTS, f"{s} not in the ctypes binding"
    assert mas_hip.lib().mas_abi_version() == mas_hip.ABI_VERSION == 10
    assert re.search(r"#define\s+MAS_ABI_VERSION\s+10\b", txt)
    assert (mas_hip.SEG_NCHW, mas_hip.SEG_NHWC, mas_hip.SEG_U8) == (0, 1, 2)


def test_entry_points_validate_arguments_without_gpu():
    """negative code + message, nothing launched"""
    import mas_hip
    L = mas_hip.lib()
    assert L.mas_seg_loss_blocks(0, 159, 8, 8, mas_hip.F32, mas_hip.SEG_NHWC, mas_hip.SEG_NCHW) == -1 and b"seg_loss" in L.mas_last_error()
    assert L.mas_seg_loss_blocks(2, 159, 8, 8, 7, mas_hip.SEG_NHWC, mas_hip.SEG_NCHW) == -2
    assert L.mas_seg_loss_blocks(2, 159, 8, 8, mas_hip.F32, 5, mas_hip.SEG_NCHW) == -1
    assert L.mas_seg_loss_fwd(None, mas_hip.F32, 0, None, mas_hip.F32, 0, None, 2, 159, 8, 8, 1, None, 0, None) == -1
    assert b"null" in L.mas_last_error()
    assert L.mas_seg_loss_bwd(None, mas_hip.F32, 0, None, mas_hip.F32, 0, None, 2, 159, 8, 8, 1, None, None, None) == -1
    assert L.mas_seg_loss_reduce(None, 1, 10, 0, None, None) == -1
    # the grid is a function of the shape (and the CU count): a mixed-layout tile is 32 pixels at C = 159, one image of 8 x 8 is two tiles
    assert L.mas_seg_loss_blocks(2, 159, 8, 8, mas_hip.F32, mas_hip.SEG_NHWC, mas_hip.SEG_NCHW) == 4
    assert L.mas_seg_loss_blocks(2, 159, 8, 8, mas_hip.F32, mas_hip.SEG_NCHW, mas_hip.SEG_NCHW) == 5      # 20352 elements / 4096 per tile


def test_cpu_tensors_keep_the_torch_path(monkeypatch):
    """with MAS_SEG_LOSS unset the classes on CPU tensors never reach the op (which refuses CPU tensors) and give the fixture's numbers"""
    import losses
    from mas_hip import ops
    monkeypatch.delenv("MAS_SEG_LOSS", raising=False)

    def boom(*a, **k):
        raise AssertionError("ops.seg_loss called for CPU tensors")
    monkeypatch.setattr(ops, "seg_loss", boom)
    g = np.load(os.path.join(ROOT, "tests", "golden", "loss_seg.npz"))
    pred, target, qloss = loss_seg_inputs()
    for name in ("BCELossWithQuant", "VQVAEWithBCELoss"):
        m = getattr(losses, name)(image_channels=159, codebook_weight=0.25)
        p = torch.from_numpy(pred).requires_grad_(True)
        loss = m(torch.tensor(qloss), torch.from_numpy(target), p)
        loss.backward()
        assert abs(float(loss.detach()) - float(g[f"{name}:0.25:loss"])) < 1e-6 * max(1.0, abs(float(loss.detach())))
        assert p.grad is not None and sorted(m.state_dict().keys()) == list(g[f"{name}:state_keys"])


def test_op_refuses_cpu_tensors_by_name():
    from mas_hip import ops
    x = torch.zeros(1, 3, 2, 2)
    with pytest.raises((ValueError, RuntimeError), match="seg_loss"):
        ops.seg_loss(x, x.clone(), torch.ones(3))
    with pytest.raises((ValueError, RuntimeError), match="seg_loss"):
        ops.seg_loss(x, torch.zeros(1, 3, 2, 3), torch.ones(3))
    with pytest.raises((ValueError, RuntimeError), match="seg_loss"):
        ops.seg_loss(x, x.clone(), torch.ones(4))
