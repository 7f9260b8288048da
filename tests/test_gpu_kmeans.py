"""The device k-means (``ops.kmeans_fit``, csrc/kmeans.hip) on the GPU: parity with the fp64 oracle on inputs whose top-2 gaps keep an
fp32 run on the oracle's trajectory (tests/helpers/kmeans_cases.py; tests/test_kmeans_cpu.py asserts that condition on the oracle alone),
the iteration cap, nothing written after convergence, bitwise repeatability, no host read (eager under the sync-debug mode, and one graph
replayed on new points), the seeded initial rows, the refusals, and the re-initialisation inside the graphed VQ-SEG training loop."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (os.path.join(ROOT, "tests", "helpers"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "make-a-scene_amd"), ROOT):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import kmeans_cases as KC  # noqa: E402
import reservoir_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = KC.all_cases()
IDS = [c[0] for c in ALL]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel_l2(got, ref):
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.linalg.norm(got - ref.astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))


def _fit(dev, pts, init, **kw):
    from mas_hip import ops
    return ops.kmeans_fit(torch.from_numpy(pts).to(dev), len(init), init_idx=torch.from_numpy(init).to(dev), tol=KC.TOL, **kw)


def _bits_equal(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("i", range(len(ALL)), ids=IDS)
def test_parity_with_the_oracle(i):
    dev = _dev()
    name, pts, init = ALL[i]
    ref_c, ref_a, ref_it = KC.oracle(name, pts, init)
    cent, assign, info = _fit(dev, pts, init)
    err = _rel_l2(cent, ref_c)
    print(f"{name}: info {info.tolist()} (oracle {ref_it} iterations), centroids rel-L2 {err:.2e}")
    assert info.dtype == torch.int32 and info.is_cuda and info.tolist() == [ref_it, 1]
    assert assign.dtype == torch.int64 and np.array_equal(assign.cpu().numpy(), ref_a)
    assert err < 1e-5
    empty = np.flatnonzero(np.bincount(ref_a, minlength=len(init)) == 0)
    if i == 2 or i == len(ALL) - 1:                           # the case whose cluster empties in iteration 2, and the duplicate centroid
        assert len(empty) == 1 and (i == 2 or empty[0] == 1)
    for k in empty:
        assert not bool(cent[k].view(torch.int32).any()), k   # exactly +0.0


def test_models_kmeans_on_device_and_padded_width():
    """``models.kmeans.kmeans_fit(on_device=True)`` hands over to the same entry; a width that is no instantiation (40: the 32 columns of
    the first case and 8 of zeros, which add nothing to any distance or mean) is zero-padded to 64 and follows the same trajectory"""
    dev = _dev()
    from models.kmeans import kmeans_fit
    name, pts, init = ALL[0]
    ref_c, ref_a, ref_it = KC.oracle(name, pts, init)
    cent, idx, info = kmeans_fit(torch.from_numpy(pts).to(dev), len(init), tol=KC.TOL, init_idx=torch.from_numpy(init).to(dev), return_info=True,
                                 on_device=True)
    assert torch.is_tensor(info) and info.is_cuda and info.tolist() == [ref_it, 1]
    assert np.array_equal(idx.cpu().numpy(), ref_a) and _rel_l2(cent, ref_c) < 1e-5
    only = kmeans_fit(torch.from_numpy(pts).to(dev), len(init), tol=KC.TOL, init_idx=torch.from_numpy(init).to(dev), on_device=True)
    assert torch.equal(only, cent)
    wide = np.concatenate([pts, np.zeros((len(pts), 8), np.float32)], axis=1)
    cw, aw, iw = _fit(dev, wide, init)
    assert cw.shape == (len(init), 40) and cw.is_contiguous() and iw.tolist() == [ref_it, 1] and np.array_equal(aw.cpu().numpy(), ref_a)
    assert _rel_l2(cw[:, :32], ref_c) < 1e-5 and not bool(cw[:, 32:].any())


def test_cap_stops_unconverged():
    dev = _dev()
    name, pts, init = ALL[KC.CAPPED]
    ref_c, ref_a, ref_it = KC.oracle(name, pts, init, 2)
    cent, assign, info = _fit(dev, pts, init, max_iter=2)
    assert ref_it == 2 and info.tolist() == [2, 0]
    assert np.array_equal(assign.cpu().numpy(), ref_a) and _rel_l2(cent, ref_c) < 1e-5


@pytest.mark.parametrize("i", range(len(ALL)), ids=IDS)
def test_frozen_after_convergence_and_repeatable(i):
    """max_iter = 100 against max_iter = the oracle's iteration count: the 95+ skipped iterations write nothing; and a second fit from
    the same inputs repeats the first bit for bit"""
    dev = _dev()
    name, pts, init = ALL[i]
    ref_it = KC.oracle(name, pts, init)[2]
    long = _fit(dev, pts, init, max_iter=100, return_shift=True)
    short = _fit(dev, pts, init, max_iter=ref_it, return_shift=True)
    again = _fit(dev, pts, init, max_iter=100, return_shift=True)
    assert long[2].tolist() == [ref_it, 1] and long[3].dtype == torch.float64 and 0.0 <= float(long[3]) <= KC.TOL
    assert _bits_equal(long, short)
    assert _bits_equal(long, again)


def test_no_host_read_eager_and_one_graph_replayed_on_new_points():
    dev = _dev()
    from mas_hip import ops
    name, pts, init = ALL[0]
    k = len(init)
    first, second = torch.from_numpy(pts).to(dev), torch.from_numpy(np.ascontiguousarray(pts[::-1])).to(dev)
    idx = torch.from_numpy(init).to(dev)
    static = first.clone()
    ops.kmeans_fit(static, k, init_idx=idx, tol=KC.TOL)       # (code objects loaded, the allocator warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager_first = ops.kmeans_fit(static, k, init_idx=idx, tol=KC.TOL, return_shift=True)
        seeded = ops.kmeans_fit(static, k, seed=77, draw=3, tol=KC.TOL)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert eager_first[2].tolist() == [KC.CASES[0]["iters"], 1] and seeded[2].tolist()[0] >= 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # one stream, no branches
        out = ops.kmeans_fit(static, k, init_idx=idx, tol=KC.TOL, return_shift=True)
    graph.replay()
    torch.cuda.synchronize()
    assert _bits_equal(out, eager_first)
    static.copy_(second)
    torch.cuda.set_sync_debug_mode("error")
    try:
        graph.replay()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    eager_second = ops.kmeans_fit(second, k, init_idx=idx, tol=KC.TOL, return_shift=True)
    assert _bits_equal(out, eager_second)
    assert not torch.equal(eager_second[0], eager_first[0])   # (the new points gave other centroids: the replay read them)


@pytest.mark.parametrize("M,K", [(403, 45), (70, 48)])
def test_seeded_start(M, K):
    dev = _dev()
    from mas_hip import ops
    pts = torch.randn(M, 32, generator=torch.Generator().manual_seed(M)).to(dev)
    for seed, draw in ((77, 0), (77, 6), (0x9E3779B97F4A7C15, 1234567)):
        cent, idx = ops.kmeans_init(pts, K, seed, draw)
        want = RR.perm(np.arange(K), M, 2, draw, seed)
        assert idx.dtype == torch.int32 and idx.cpu().tolist() == want.tolist() and len(set(want.tolist())) == K
        assert torch.equal(cent.view(torch.int32), pts[torch.from_numpy(want).to(dev)].view(torch.int32))
    # the fit from a seed is the fit from those rows
    a = ops.kmeans_fit(pts, K, seed=77, draw=6, max_iter=3, return_shift=True)
    b = ops.kmeans_fit(pts, K, init_idx=torch.from_numpy(RR.perm(np.arange(K), M, 2, 6, 77)).to(dev), max_iter=3, return_shift=True)
    assert _bits_equal(a, b) and a[2].tolist()[0] >= 1


def test_refusals_name_the_limit():
    dev = _dev()
    from mas_hip import ops
    pts = torch.zeros(403, 32, device=dev)
    with pytest.raises(ValueError, match=r"D=512 outside the kernel envelope: widths up to 256"):
        ops.kmeans_fit(torch.zeros(64, 512, device=dev), 8, seed=1)
    with pytest.raises(ValueError, match=r"1 <= n_clusters <= M .* n_clusters=404, M=403"):
        ops.kmeans_fit(pts, 404, seed=1)
    off = torch.zeros(403 * 32 + 1, device=dev)[1:].view(403, 32)
    assert off.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.kmeans_fit(off, 45, seed=1)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.kmeans_init(off, 45, 1)


def test_reinitialisation_inside_the_graphed_training_loop(monkeypatch):
    """the configuration of tests/test_gpu_graph_vq.py (K = 48, D = 32, reservoir 70, init_steps = 2: calls 6 .. 12 re-initialise) with
    ``device_kmeans=True``: the graphed run and its eager twin agree bit for bit, the replay loop then crosses two more
    re-initialisations under the sync-debug mode without a new capture, and torch's determinism switch is never touched"""
    dev = _dev()
    import test_gpu_graph_vq as G
    from mas_hip import graphs
    from mas_hip.optim import AdamW
    switched = []
    real = torch.use_deterministic_algorithms
    monkeypatch.setattr(torch, "use_deterministic_algorithms", lambda *a, **k: (switched.append((a, k)), real(*a, **k))[1])
    before = torch.are_deterministic_algorithms_enabled()
    batches = G._batches(dev, G.CALLS + 2)
    kw = dict(lr=1e-3, betas=(0.9, 0.95), weight_decay=0.01, device_step=True)

    def model():
        torch.manual_seed(11)
        m, crit = G._model(dev, device_reservoir=False)
        m.quantize.enable_device_reservoir(seed=77, device_kmeans=True)
        assert m.quantize._dev["device_kmeans"] is True
        return m, crit
    mt, ct = model()
    ot, ft = AdamW(mt.parameters(), **kw), G._loss_fn(mt, ct)
    eager = [G._eager_call(ft, ot, planes, True) for planes in batches]
    mg, cg = model()
    og = AdamW(mg.parameters(), **kw)
    step = graphs.GraphedTrainStep(G._loss_fn(mg, cg), og, batches[0], modules=[mg])
    graphed = [step(planes).clone() for planes in batches[1:G.CALLS]]
    assert step.captures == 3 and mg.quantize.q_counter == G.CALLS and mg.quantize.phase() == 2
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for planes in batches[G.CALLS:]:
            assert mg.quantize.q_init <= mg.quantize.q_counter + 1 < mg.quantize.q_re_end      # a re-initialisation is due in this call
            graphed.append(step(planes).clone())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert step.captures == 3 and step.calls == G.CALLS + 2 == mg.quantize.q_counter == mt.quantize.q_counter
    for k, (lg, lt) in enumerate(zip(graphed, eager[1:]), start=2):
        assert torch.equal(lg, lt), (k, float(lg), float(lt))
    assert G._same(G._bits(mg, og), G._bits(mt, ot)) and bool(torch.isfinite(graphed[-1]))
    assert mg.quantize._dev["state"].tolist() == [70, G.CALLS]
    assert switched == [] and torch.are_deterministic_algorithms_enabled() == before
