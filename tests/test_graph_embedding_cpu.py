"""``mas_hip.graphs.embedding``: outside a capture and on the CPU it IS the module call; the chunked backward it takes under a capture sums
ATen's dense backward over slices of the indices, which equals the gradient of ``F.embedding`` (checked here in float64, where the order
of the additions does not show at 1e-12).  The capture itself is tests/test_gpu_graph_step.py."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "make-a-scene_amd"))


def test_off_the_gpu_it_is_the_module_call():
    from mas_hip import graphs
    emb = torch.nn.Embedding(50, 8)
    idx = torch.randint(0, 50, (3, 3000), generator=torch.Generator().manual_seed(0))          # more than a chunk
    with graphs.embedding_grad_in_chunks():
        out = graphs.embedding(emb, idx)
    assert torch.equal(out, emb(idx)) and type(out.grad_fn).__name__ == "EmbeddingBackward0"
    assert graphs._chunks_always is False


@pytest.mark.parametrize("n", [1, 2048, 2049, 5000])
def test_chunked_backward_is_the_gradient_of_embedding(n):
    from mas_hip import graphs
    g = torch.Generator().manual_seed(n)
    w = torch.randn(37, 6, generator=g, dtype=torch.float64, requires_grad=True)
    idx = torch.randint(0, 37, (n,), generator=g).view(1, n)
    dy = torch.randn(1, n, 6, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(torch.nn.functional.embedding(idx, w), w, dy)
    out = graphs._EmbeddingGradInChunks.apply(w, idx)
    assert torch.equal(out, torch.nn.functional.embedding(idx, w))
    (got,) = torch.autograd.grad(out, w, dy)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    if n <= graphs.EMBEDDING_GRAD_CHUNK:
        assert torch.equal(got, want)                        # one slice: ATen's own result
