"""The on-device sampler never hands an entry an infinite Gumbel score.  Seed {12345, 678}, step 0: the Philox word of row 2648, entry
6388 is 0xffffffee (tests/test_sampler_uniform_cpu.py).  A uniform built from its top 24 bits rounds to exactly 1 in float32, which makes
-log(-log u) = +inf; entry 6388, at logit -20, would then beat entry 0 at +20.  Every row must draw entry 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_no_entry_wins_by_an_infinite_score():
    from mas_hip import decode
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    rows, v = 2649, 8192
    logits = torch.full((1, v), -20.0, device=dev)
    logits[0, 0] = 20.0
    tokens = torch.full((rows, 1), -1, dtype=torch.long, device=dev)
    params = torch.tensor([1.0, 0.0], device=dev)
    seed = torch.tensor([12345, 678], dtype=torch.int64, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    decode.sample_tokens(logits, tokens, step, params, decode.SAMPLE, seed=seed, rows=rows)
    t = tokens[:, 0].cpu()
    assert int(t[2648]) == 0, int(t[2648])
    assert bool((t == 0).all())
