"""The inputs of the device k-means tests (tests/test_kmeans_cpu.py, tests/test_gpu_kmeans.py): blob data from the generator
tests/test_gpu_model.py::test_kmeans_reinit_vs_oracle uses, at the smallest shapes that cross every edge of the kernels (the 128-row
assignment block, the 32-code tile, the 64-wide ballot, the four-wave split of M, the 8-code update range, all four widths), with seeds
SCANNED (300 per shape) for a wide top-2 distance gap at every iteration of the fp64 oracle.

The gap is a CONDITION ON THE INPUTS: an fp32 run and the fp64 oracle follow the same trajectory only while no assignment flips, and at
the usual seeds the smallest gap between a point's nearest and second-nearest centroid is 1-30 fp32 ulps -- within the rounding of a
D-term fp32 FMA chain (about sqrt(D) / 2 ulps, <= 8 at D = 256).  tests/test_kmeans_cpu.py re-derives the columns below from the oracle
alone and asserts gap >= MIN_GAP_ULPS and every non-zero shift >= MIN_SHIFT_OVER_TOL * tol."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.kmeans_oracle import kmeans_lloyd  # noqa: E402

TOL = 1e-4
MIN_GAP_ULPS = 128
MIN_SHIFT_OVER_TOL = 100

# iters: the oracle's iterations at max_iter = 100;  gap: the smallest top-2 gap over all iterations and points, in ulps of fp32 at the
# magnitude |x|^2 + |c|^2, c the larger of the two centroids (floor);  empties: {iteration (1-based): how many clusters have no point
# in that iteration's assignment and in every later one}
CASES = [
    dict(k=45, d=32, per=9, drop=2, seed=232, M=403, iters=3, gap=1180, empties={}),
    dict(k=45, d=64, per=9, drop=2, seed=232, M=403, iters=3, gap=689, empties={}),
    dict(k=13, d=128, per=31, drop=2, seed=151, M=401, iters=3, gap=414, empties={2: 1}),
    dict(k=21, d=256, per=19, drop=2, seed=32, M=397, iters=3, gap=296, empties={}),
    dict(k=70, d=32, per=7, drop=1, seed=37, M=489, iters=5, gap=1136, empties={}),
]
CAPPED = 4              # the 5-iteration case (the cap test runs it with max_iter = 2)
DUPLICATE_OF = 1        # the sixth case: this one with init[1] = init[0]; cluster 1 is empty at EVERY iteration of the oracle (in case 0
                        # the zero vector wins points back in iteration 2)


def make(case):
    """-> (points fp32 [M, d], init int64 [k])"""
    rs = np.random.RandomState(case["seed"])
    k, d, per = case["k"], case["d"], case["per"]
    centers = 4 * rs.randn(k, d)
    pts = (centers[:, None] + 0.3 * rs.randn(k, per, d)).reshape(-1, d).astype(np.float32)
    rs.shuffle(pts)
    pts = pts[:len(pts) - case["drop"]]
    init = rs.choice(len(pts), k, replace=False)
    return pts, init.astype(np.int64)


def all_cases():
    """-> [(name, points, init)]: the five of the table and the duplicate-initial-centroid case"""
    out = []
    for c in CASES:
        pts, init = make(c)
        out.append((f"k{c['k']}_d{c['d']}_s{c['seed']}", pts, init))
    name, pts, init = out[DUPLICATE_OF]
    dup = init.copy()
    dup[1] = dup[0]
    out.append((name + "_dup", pts, dup))
    return out


def trace(points, init, max_iter=100, tol=TOL):
    """the fp64 oracle's rule, iteration by iteration (oracle/kmeans_oracle.py restated with its intermediate values kept; the CPU test
    checks the end state against ``kmeans_lloyd`` itself) -> [dict(gap_ulps, shift, empty)] per executed iteration.  Exact ties between
    IDENTICAL centroids (the duplicate case) are no near-tie: the gap is taken over the distinct centroid rows."""
    x = points.astype(np.float64)
    cent = x[init].copy()
    k = cent.shape[0]
    xx = (x * x).sum(1)
    out = []
    for _ in range(max_iter):
        cc = (cent * cent).sum(1)
        d = xx[:, None] + cc[None, :] - 2.0 * x @ cent.T
        assign = d.argmin(1)
        _, first = np.unique(cent, axis=0, return_index=True)
        first = np.sort(first)
        du = d[:, first]
        order = np.argsort(du, axis=1)[:, :2]
        rows = np.arange(len(x))
        d1, d2 = du[rows, order[:, 0]], du[rows, order[:, 1]]
        mag = xx + np.maximum(cc[first][order[:, 0]], cc[first][order[:, 1]])
        gap = float(((d2 - d1) / np.spacing(mag.astype(np.float32)).astype(np.float64)).min())
        cnt = np.bincount(assign, minlength=k).astype(np.float64)
        new = np.zeros_like(cent)
        np.add.at(new, assign, x)
        new = np.where(cnt[:, None] > 0, new / np.maximum(cnt, 1)[:, None], 0.0)
        shift = float(((new - cent) ** 2).sum())
        out.append(dict(gap_ulps=gap, shift=shift, empty=np.flatnonzero(cnt == 0).tolist()))
        cent = new
        if shift <= tol:
            break
    return out, cent.astype(np.float32), assign


_oracle = {}


def oracle(name, points, init, max_iter=100):
    """``kmeans_lloyd`` once per (case, max_iter); the results are shared and must not be written to"""
    key = (name, max_iter)
    if key not in _oracle:
        _oracle[key] = kmeans_lloyd(points, init, max_iter=max_iter, tol=TOL)
    return _oracle[key]
