"""The codebook's device reservoir (csrc/reservoir.hip, ``ops.reservoir_collect``, ``Codebook.enable_device_reservoir``): the kernels
against the numpy restatement of the rule (tests/helpers/reservoir_ref.py) slot by slot and bit for bit over sequences of calls; what
holds whatever the restatement says (every held row is a row of this or an earlier batch, c = min(R, 10 B k)); the two frequency bounds
of tests/test_reservoir_cpu.py on the device; and a ``Codebook`` run eagerly through collect, warm-up and re-initialisations, twice."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import reservoir_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
GRID = {10: (2, 5), 16: (4, 4), 100: (10, 10)}
SEED = 0x9E3779B97F4A7C15
CASES = [(D, B, HW, R) for D in (32, 256) for B in (1, 2, 3) for HW in (10, 16, 100) for R in (20, 64, 70) if 10 * B <= R]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _latent(B, D, HW, seed, dev):
    """fp32 [B, D, H, W]-logical in NHWC memory, as ``Codebook.forward`` holds it; and its rows [B * HW, D] on the host as int32 bits"""
    from mas_hip import ops
    h, w = GRID[HW]
    z = ops.nhwc(torch.randn(B, D, h, w, generator=torch.Generator().manual_seed(seed)).to(dev), torch.float32)
    rows = z.permute(0, 2, 3, 1).reshape(B * HW, D).contiguous().view(torch.int32).cpu().numpy()
    return z, rows


@pytest.mark.parametrize("D,B,HW,R", CASES)
def test_kernel_against_the_restatement_and_on_its_own_terms(D, B, HW, R):
    dev = _dev()
    from mas_hip import ops
    assert (20, 2) in {(r, b) for _, b, _, r in CASES} and (70, 2) in {(r, b) for _, b, _, r in CASES}     # 10 B = R; crossing mid-call
    buf = torch.full((R, D), float("nan"), device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    ref = RR.Reservoir(SEED, R, B, HW)
    batches, seen = [], set()
    for k in range(2 + (2 * R) // (10 * B)):                    # past capacity, then a few full calls
        z, rows = _latent(B, D, HW, 100 * k + B, dev)
        batches.append(rows)
        seen |= {r.tobytes() for r in rows}
        plan = ops.reservoir_collect(z, buf, state, SEED)
        pos, drop, dst, src = ref.collect()
        got = buf.view(torch.int32).cpu().numpy()
        c, calls = state.tolist()
        assert (c, calls) == (ref.c, ref.calls) == (min(R, 10 * B * (k + 1)), k + 1)
        p = plan.cpu().numpy().reshape(-1, 2)
        assert p[:, 0].tolist() == dst.tolist() and p[:, 1].tolist() == src.tolist(), k
        for slot in range(R):
            if ref.rows[slot] is None:
                assert slot >= c and np.isnan(got[slot].view(np.float32)).all()       # never written
            else:
                call, row = ref.rows[slot]
                assert slot < c and np.array_equal(got[slot], batches[call][row]), (k, slot)
        # whatever the restatement says: every held row is, bit for bit, a row of this or an earlier batch
        assert all(got[slot].tobytes() in seen for slot in range(c))
        if 10 * B * (k + 1) <= R:                               # appended: this call's rows are its 10 positions of every image
            new = {got[slot].tobytes() for slot in range(c - 10 * B, c)}
            assert len(new) == 10 * B and new <= {r.tobytes() for r in rows}


def test_frequencies_on_the_device():
    """R = 64, B = 2, HW = 16, 2000 calls on a full reservoir: a candidate survives with frequency 64 / 84 +- 0.012 and every slot is
    replaced 476 +- 100 times (tests/test_reservoir_cpu.py derives both bounds and holds the rule itself to them)"""
    dev = _dev()
    from mas_hip import ops
    from test_reservoir_cpu import FREQ as f, frequencies
    R, B, HW, calls = f["R"], f["B"], f["HW"], f["calls"]
    z, _ = _latent(B, 32, HW, 1, dev)
    buf, state = torch.zeros(R, 32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    fill = -(-R // (10 * B))
    plans = torch.empty(fill + calls, ops.reservoir_plan_elems(B), dtype=torch.int32, device=dev)
    for k in range(fill + calls):
        ops.reservoir_collect(z, buf, state, SEED, plans[k])
    assert state.tolist() == [R, fill + calls]
    dst = plans.cpu().numpy().reshape(fill + calls, -1, 2)[fill:, :, 0]
    want = [RR.plan(SEED, fill + k, R, R, B, HW)[2] for k in (0, 1, calls - 1)]
    assert all(dst[k].tolist() == w.tolist() for k, w in zip((0, 1, calls - 1), want))
    survive, replaced = frequencies([(None, d) for d in dst], R, 10 * B)
    print(f"device: survival {survive:.4f} (expected {f['survive']:.4f}), replacements per slot {replaced.min()} .. {replaced.max()}")
    assert abs(survive - f["survive"]) <= f["survive_tol"]
    assert np.abs(replaced - f["replaced"]).max() <= f["replaced_tol"]


def test_refusals_on_the_device():
    dev = _dev()
    from mas_hip import ops
    z, _ = _latent(2, 32, 16, 0, dev)
    buf, state = torch.zeros(64, 32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    for bad in (lambda: ops.reservoir_collect(z, torch.zeros(19, 32, device=dev), state, 1),
                lambda: ops.reservoir_collect(z, torch.zeros(64, 16, device=dev), state, 1),
                lambda: ops.reservoir_collect(z.contiguous(), buf, state, 1),                     # NCHW memory
                lambda: ops.reservoir_collect(z, buf, state.long(), 1),
                lambda: ops.reservoir_collect(z, buf, state, 1, torch.zeros(8, dtype=torch.int32, device=dev))):
        with pytest.raises((ValueError, RuntimeError), match="reservoir_collect"):
            bad()
    assert state.tolist() == [0, 0] and not bool(buf.any())


def _run_codebook(dev, device_reservoir, calls=9):
    """a Codebook (48 codes of 32, init_steps = 2: collecting from call 3, lookup and a re-initialisation at every call from 6 on), B = 2
    on an 8 x 8 latent, reservoir of 70 rows (call 6 crosses its capacity); -> per call (outputs, embedding, data_ptr), the reservoir"""
    from mas_hip import ops
    from models.modules import Codebook
    torch.manual_seed(1234)
    cb = Codebook(48, 32, beta=0.25, init_steps=2, reservoir_size=70).to(dev).train()
    if device_reservoir:
        cb.enable_device_reservoir()
    out = []
    for k in range(calls):
        z = ops.nhwc(torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(50 + k)).to(dev), torch.float32)
        zq, loss, idx = cb(z)
        out.append((zq.detach().clone(), loss.detach().clone(), None if idx is None else idx.clone(), cb.embedding.weight.detach().clone(),
                    cb.embedding.weight.data_ptr()))
    return cb, out


def test_codebook_with_the_device_reservoir_repeats_bit_for_bit():
    dev = _dev()
    cb1, a = _run_codebook(dev, True)
    cb2, b = _run_codebook(dev, True)
    assert cb1._dev["seed"] == cb2._dev["seed"] and cb1.q_counter == 9
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x[2] is None) == (y[2] is None) == (k + 1 < 6), k
        assert torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)) and torch.equal(x[1], y[1]), k
        assert x[2] is None or torch.equal(x[2], y[2]), k
        assert torch.equal(x[3].view(torch.int32), y[3].view(torch.int32)), k
    assert torch.equal(cb1._dev["buf"].view(torch.int32), cb2._dev["buf"].view(torch.int32))
    assert cb1._dev["state"].tolist() == cb2._dev["state"].tolist() == [70, 7] and cb1._dev["c"] == 70
    assert cb1.reservoir.shape == (70, 32) and cb1.reservoir.data_ptr() == cb1._dev["buf"].data_ptr()
    # the re-initialisations (calls 6, 7, ...) moved the codebook, in the storage it had from the start
    assert len({x[4] for x in a}) == 1
    assert torch.equal(a[0][3], a[4][3]) and not torch.equal(a[4][3], a[5][3]) and not torch.equal(a[5][3], a[6][3])
    assert list(cb1.state_dict()) == ["embedding.weight"]
    # the mirror of c follows the schedule with nothing read back: 20 rows per collecting call
    cb3, _ = _run_codebook(dev, True, calls=4)
    assert cb3._dev["c"] == 40 and cb3.reservoir.shape == (40, 32) and cb3._dev["state"].tolist() == [40, 2]


def test_default_codebook_still_replaces_its_weight():
    dev = _dev()
    cb, out = _run_codebook(dev, False, calls=6)
    assert not cb.device_reservoir and out[5][2] is not None and out[4][2] is None
    assert out[5][4] != out[4][4] and len({x[4] for x in out[:5]}) == 1
    assert cb.reservoir.shape == (70, 32) and cb.reservoir.data_ptr() != cb.embedding.weight.data_ptr()
