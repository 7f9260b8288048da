"""The CPU restatement of the split-K weight-gradient walks (tests/helpers/wgrad_walk.py): for thousands of (shape, nsplit) pairs every
kernel's walk visits every tile / chunk / pixel exactly once -- above all the LDS-DMA kernel's incremental cursor with its column, row
and image carries, which no division re-derives.  tests/test_gpu_wgrad_splits.py uses the same code to classify what the GPU ran."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wgrad_walk as W  # noqa: E402


def _geo(n, h, w, cin, cout, ks=3, stride=1, ho=None, wo=None):
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, ks=ks, stride=stride, ho=h if ho is None else ho, wo=w if wo is None else wo)


def _nsplits(ceil, rng):
    ks = set(range(1, min(ceil, 40) + 1)) | {ceil}
    ks |= {rng.randint(1, ceil) for _ in range(8)}
    return sorted(ks)


@pytest.mark.parametrize("kernel", ["conv_wgrad_dma", "conv_wgrad_up2", "wgrad_s2", "wgrad_thin", "conv_wgrad_tr", "conv_wgrad"])
def test_tile_walks_visit_every_tile_once(kernel):
    rng = random.Random(sum(map(ord, kernel)))
    pairs = 0
    regimes = set()
    for _ in range(120):
        n, h, w = rng.randint(1, 5), rng.randint(1, 70), rng.randint(1, 90)
        g = _geo(n, h, w, 64, 128, ks=rng.choice((1, 3, 4)) if kernel == "conv_wgrad_tr" else 3,
                 stride=rng.choice((1, 2)) if kernel == "conv_wgrad" else 1)
        if kernel == "wgrad_s2" or (kernel == "conv_wgrad" and g["stride"] == 2):
            g["ho"], g["wo"] = (h + 1 - 3) // 2 + 1 if h >= 2 else 1, (w + 1 - 3) // 2 + 1 if w >= 2 else 1
        ceil = W.ceiling(kernel, g)
        assert ceil == (W.n_units(kernel, g) // 4 or 1 if kernel == "wgrad_thin" else W.n_units(kernel, g))
        for ns in _nsplits(ceil, rng):
            per_wg, seen = W.walk(kernel, g, ns)
            assert len(per_wg) == ns
            assert W.covers_once(kernel, g, per_wg), (kernel, g, ns)
            regimes |= {k for k, v in seen.items() if v}
            pairs += 1
    assert pairs >= 2000
    want = {"nsplit1", "one_per_wg", "multi_per_wg", "uneven", "image_cross"}
    if kernel in ("conv_wgrad_dma", "conv_wgrad_up2"):
        want |= {"col_carry", "row_carry"}
    if kernel == "wgrad_thin":
        want -= {"one_per_wg"}            # ceiling n_tiles / 4: a thin work-group walks one tile only when the map has fewer than 8
    assert want <= regimes, want - regimes


def test_dma_cursor_carries_at_known_shapes():
    # tiles_w = 3, nsplit = 7: adv_w = 1 column, adv_q = 2 rows -> split 2 walks (0, 0, 2) -> (0, 3, 0): a column carry into the row
    per_wg, seen = W.dma_walk(5, 3, 2, 7)
    assert per_wg[2][:2] == [(0, 0, 2), (0, 3, 0)] and seen["col_carry"]
    # nsplit % tiles_w == 0 (the benched layers): no column carry at all
    assert not W.dma_walk(32, 16, 1, 96)[1]["col_carry"]
    # tiles_w = 1 (16 x 16 maps): no column carry either, whatever the split
    assert not any(W.dma_walk(2, 1, 16, k)[1]["col_carry"] for k in range(1, 32))


def test_pointwise_walks_cover_every_pixel_once():
    rng = random.Random(7)
    pairs = 0
    for _ in range(150):
        g = _geo(rng.randint(1, 4), rng.randint(1, 40), rng.randint(1, 40), 128, 128, ks=1)
        ceil = W.ceiling("wgrad1x1", g)
        for ns in range(1, ceil + 1):
            per_wg, _ = W.walk("wgrad1x1", g, ns)
            assert W.covers_once("wgrad1x1", g, per_wg) and min(len(u) for u in per_wg) >= (1 if W.n_units("wgrad1x1", g) < 2 else 2)
            pairs += 1
        gf = _geo(g["n"], g["h"], g["w"], 4 * rng.randint(1, 40), 4 * rng.randint(1, 40), ks=1)
        seen_ns = set()
        for k in [0] + list(range(1, 300, 7)):
            ns = W.splits("wgrad1x1_f32", gf, cus=256, override=k)
            if ns in seen_ns:
                continue
            seen_ns.add(ns)
            per_wg, _ = W.walk("wgrad1x1_f32", gf, ns)
            assert W.covers_once("wgrad1x1_f32", gf, per_wg) and all(per_wg), (gf, k, ns)
            pairs += 1
    assert pairs >= 1000


def test_override_keeps_every_clamp():
    """MAS_WGRAD_SPLITS replaces the CU-based start only: the kernel's clamps still bound what it yields (min(k, ceiling); the fp32 1x1
    setup then rounds its pixel ranges), and the unset knob is the production sizing"""
    rng = random.Random(3)
    for _ in range(200):
        n, h, w = rng.randint(1, 4), rng.randint(4, 48), rng.randint(4, 48)
        for kernel, g in (("conv_wgrad_dma", _geo(n, h, w, 64 * rng.randint(1, 3), 128 * rng.randint(1, 3))),
                          ("conv_wgrad_up2", _geo(n, h, w, 64, 128, ho=2 * h, wo=2 * w)), ("wgrad_s2", _geo(n, h, w, 64, 128, stride=2)),
                          ("wgrad_thin", _geo(n, h, w, 8, 128)), ("wgrad1x1", _geo(n, h, w, 128, 256, ks=1)),
                          ("wgrad1x1_f32", _geo(n, h, w, 36, 20, ks=1)), ("conv_wgrad_tr", _geo(n, h, w, 96, 160))):
            assert W.splits(kernel, g, cus=256, override=0) == W.splits(kernel, g, cus=256)
            ceil = W.ceiling(kernel, g)
            for k in (1, 2, 3, 5, 7, 32, 33, 47, 10 ** 4):
                got = W.splits(kernel, g, cus=256, override=k)
                if kernel == "wgrad1x1_f32":
                    m = n * h * w
                    assert got == W.cdiv(m, W.roundup(W.cdiv(m, min(k, ceil)), 32))
                else:
                    assert got == min(k, ceil), (kernel, g, k)


def test_reduce_variant_rule():
    assert W.reduce_variant("conv_wgrad_dma", 3, 31) == "G4" and W.reduce_variant("conv_wgrad_dma", 3, 32) == "G16"
    assert W.reduce_variant("wgrad1x1", 1, 200) == "G4" and W.reduce_variant("conv_wgrad_up2", 3, 64) == "up2"
