"""Host-side state of the weight-gradient path that needs no GPU: importing ``mas_hip.ops`` leaves the process environment alone (the CU
budget of the weight-gradient grid travels in ``MasConvDesc.wgrad_cus``), and ``_ColsumHint`` empties its table at the end of every
backward that put an entry, also after an earlier backward raised."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMPORT_CHILD = """
import os, sys
sys.path.insert(0, sys.argv[1])
import torch                      # (whatever torch's own import adds is not the package's doing)
before = dict(os.environ)
from mas_hip import ops
added = sorted(set(os.environ) - set(before))
changed = sorted(k for k in before if os.environ.get(k) != before[k])
assert added == ["GPU_MAX_HW_QUEUES"] and not changed, (added, changed)
assert ops._WGRAD_CUS_USER is None
"""


def test_importing_ops_adds_only_the_hardware_queue_count_to_the_environment():
    env = {k: v for k, v in os.environ.items() if k not in ("MAS_WGRAD_CUS", "GPU_MAX_HW_QUEUES")}
    p = subprocess.run([sys.executable, "-c", IMPORT_CHILD, os.path.join(ROOT, "make-a-scene_amd")], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr


def test_the_budget_is_the_users_value_or_the_side_stream_default(monkeypatch):
    """MAS_WGRAD_CUS is read once at import (``_WGRAD_CUS_USER``); without it -1 while the side stream is on, 0 for a device whose probe
    refused it, 0 with MAS_WGRAD_STREAM=0.  ``_side_ok`` plays no part."""
    from mas_hip import ops
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    monkeypatch.setattr(ops, "_WGRAD_CUS_USER", None)
    monkeypatch.setattr(ops, "_WGRAD_STREAM", True)
    monkeypatch.setattr(ops, "_wgrad_cus", {})
    monkeypatch.setattr(ops, "_side_ok", {3: False})
    assert ops.wgrad_cus() == -1
    ops._wgrad_cus[2] = 0
    assert ops.wgrad_cus() == -1                         # another device's refusal
    ops._wgrad_cus[3] = 0
    assert ops.wgrad_cus() == 0
    monkeypatch.setattr(ops, "_WGRAD_CUS_USER", 64)
    assert ops.wgrad_cus() == 64
    monkeypatch.setattr(ops, "_WGRAD_CUS_USER", None)
    monkeypatch.setattr(ops, "_WGRAD_STREAM", False)
    monkeypatch.setattr(ops, "_wgrad_cus", {})
    assert ops.wgrad_cus() == 0
    monkeypatch.setattr(ops, "_WGRAD_STREAM", True)
    d = ops._wgrad_desc(4, 36, 44, 64, 36, 44, 128, 3, 1, 1, 1, torch.bfloat16, ops.ACT_NONE, False)
    assert d.wgrad_cus == -1 and d.w_layout == 0
    assert ops._desc(4, 36, 44, 64, 36, 44, 128, 3, 1, 1, 1, torch.bfloat16, torch.bfloat16, ops.ACT_NONE, False).wgrad_cus == 0


class _Put(torch.autograd.Function):
    """identity whose backward leaves its gradient in the hint table, as ``_layer_norm_bwd`` does"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        from mas_hip import ops
        ops._colsum_hint.put(g, g.sum(0))
        return g


class _Raise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("a later node of the backward fails")


def test_colsum_hint_is_emptied_by_the_backward_after_a_failed_one():
    """The autograd engine drops its queued callbacks when a backward raises.  The next backward that puts an entry must queue its own
    clean-up: the table is empty when it ends (CPU tensors: key (None, 0))."""
    from mas_hip import ops
    ops._colsum_hint.clear()
    try:
        x = torch.randn(4, 8, requires_grad=True)
        with pytest.raises(RuntimeError, match="a later node"):
            _Put.apply(_Raise.apply(x)).sum().backward()             # _Put's backward runs first, then _Raise's
        _Put.apply(x).sum().backward()
        assert ops._colsum_hint.slots == {}
        _Put.apply(x).sum().backward()                               # and a clean pass after a clean pass
        assert ops._colsum_hint.slots == {}
    finally:
        ops._colsum_hint.clear()
