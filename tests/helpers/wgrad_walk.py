"""CPU restatement of how every split-K weight-gradient kernel cuts its work: the split count each setup chooses (CU-based start, or
MAS_WGRAD_SPLITS, then the kernel's own clamps), the tiles a work-group walks, and which `mas_wgrad_reduce` variant adds the slabs.

    conv_wgrad_dma.hip   dma_setup / up2_wgrad_setup; the incremental tile cursor (first_tile / next_tile: adv_w, adv_q, adv_h, adv_n)
    conv_s2.hip          s2_wgrad_setup; tiles split, split + nsplit, ...
    conv_thin.hip        thin_wgrad_setup; same walk
    conv1x1.hip          pw_wgrad_setup (64-pixel chunks), pw_f32_setup (contiguous pixel ranges)
    conv_wgrad.hip       launch / launch_tr in slab mode; for (pt = split; pt < n_pt; pt += nsplit)
    misc.hip             mas_wgrad_reduce: G = 16 when nsplit >= 32 and ks > 1, else G = 4; mas_wgrad_reduce_up2: one variant

`walk(...)` returns, per work-group, the list of units it visits and the regimes the walk took; tests/test_wgrad_walk_cpu.py checks
that every unit is visited exactly once, tests/test_gpu_wgrad_splits.py classifies what its GPU children ran with the same code."""


def cdiv(a, b):
    return (a + b - 1) // b


def roundup(a, b):
    return cdiv(a, b) * b


def start(occupancy, override):
    """mas_wgrad_split_start: MAS_WGRAD_SPLITS = k > 0 replaces the CU-based estimate"""
    return override if override > 0 else occupancy


def _clamp(ns, hi):
    return max(1, min(ns, hi))


# ---- geometry of each family: (units a work-group walks, tile grid) -----------------------------------------------------------------
# kernel names are what mas_last_kernel reports
TILE = {"conv_wgrad_dma": (8, 16), "conv_wgrad_up2": (8, 16), "wgrad_s2": (4, 16), "wgrad_thin": (4, 16), "conv_wgrad_tr": (8, 16)}


def general_thw(ks, stride):
    """tile height of the general kernels (conv_wgrad.hip launch_t): 8 x 16 pixels, 4 x 16 at stride 2"""
    return 4 if stride == 2 else 8


def general_bci(kernel, ks):
    """input channels per work-group: launch_tr<4, 32>, launch_tr<2, 64>, launch_tr<1|3> (default BCI_) = 64; launch_t (BCI) = 32"""
    if kernel == "conv_wgrad_tr":
        return 32 if ks == 4 else 64
    return 32


def splits(kernel, g, cus, oversub=1, budget=None, override=0):
    """nsplit of the setup behind `kernel` for geometry g (dict: n, h, w, cin, ho, wo, cout, ks, stride; the DESCRIPTOR's values, i.e.
    after the 4x4 / stride-2 space-to-depth rewrite).  cus = mas_num_cus(); budget = wgrad_cus(d) (MasConvDesc.wgrad_cus, DMA 3x3 only)."""
    ov = oversub if oversub > 0 else 1
    if kernel == "conv_wgrad_dma":
        n_pt = g["n"] * cdiv(g["ho"], 8) * cdiv(g["wo"], 16)
        ot = (g["cout"] // 128) * (g["cin"] // 64)
        return _clamp(start(cdiv((budget if budget is not None else cus) * ov, ot), override), n_pt)
    if kernel == "conv_wgrad_up2":                        # the tiles walk the LOW-resolution grid; four phases share the CUs
        n_pt = g["n"] * cdiv(g["h"], 8) * cdiv(g["w"], 16)
        ot = (g["cout"] // 128) * (g["cin"] // 64) * 4
        return _clamp(start(cdiv(cus * ov, ot), override), n_pt)
    if kernel == "wgrad_s2":
        n_t = g["n"] * cdiv(g["ho"], 4) * cdiv(g["wo"], 16)
        return _clamp(start(cdiv(cus, (g["cout"] // 128) * (g["cin"] // 64)), override), n_t)
    if kernel == "wgrad_thin":
        n_t = g["n"] * cdiv(g["h"], 4) * cdiv(g["w"], 16)
        return _clamp(start(2 * cus, override), n_t // 4)
    if kernel == "wgrad1x1":
        m = g["n"] * g["h"] * g["w"]
        ns = start(cdiv(2 * cus, (g["cout"] // 128) * (g["cin"] // 128)), override)
        return max(1, min(ns, cdiv(m, 64) // 2, 256))
    if kernel == "wgrad1x1_f32":
        return f32_ranges(g, cus, override)[0]
    if kernel in ("conv_wgrad_tr", "conv_wgrad"):
        thw = 8 if kernel == "conv_wgrad_tr" else general_thw(g["ks"], g["stride"])
        n_pt = g["n"] * cdiv(g["ho"], thw) * cdiv(g["wo"], 16)
        ot = cdiv(g["cout"], 128) * cdiv(g["cin"], general_bci(kernel, g["ks"]))
        return _clamp(start(cdiv(cus, ot), override), n_pt)
    raise KeyError(kernel)


def f32_ranges(g, cus, override=0):
    """pw_f32_setup: (nsplit, pixels per split)"""
    m = g["n"] * g["h"] * g["w"]
    ns = start(cdiv(2 * cus, cdiv(g["cout"], 64) * cdiv(g["cin"], 64)), override)
    ns = max(1, min(ns, cdiv(m, 4 * 32), 256))
    pps = roundup(cdiv(m, ns), 32)
    return cdiv(m, pps), pps


def ceiling(kernel, g):
    """the largest split count the kernel's clamps allow (what MAS_WGRAD_SPLITS = 10^4 gives)"""
    return splits(kernel, g, cus=1, oversub=1, budget=1, override=1 << 30)


def n_units(kernel, g):
    """what the split walks over: pixel tiles, 64-pixel chunks (bf16 1x1) or pixels (fp32 1x1)"""
    if kernel in ("conv_wgrad_dma", "wgrad_s2", "wgrad_thin", "conv_wgrad_tr", "conv_wgrad"):
        th, tw, nimg = tile_grid(kernel, g)
        return nimg * th * tw
    if kernel == "conv_wgrad_up2":
        return g["n"] * cdiv(g["h"], 8) * cdiv(g["w"], 16)
    m = g["n"] * g["h"] * g["w"]
    return cdiv(m, 64) if kernel == "wgrad1x1" else m


def tile_grid(kernel, g):
    """(tiles_h, tiles_w, images) of the tile-walking kernels"""
    if kernel == "conv_wgrad_up2":
        return cdiv(g["h"], 8), cdiv(g["w"], 16), g["n"]
    if kernel == "wgrad_thin":
        return cdiv(g["h"], 4), cdiv(g["w"], 16), g["n"]
    if kernel == "conv_wgrad":
        return cdiv(g["ho"], general_thw(g["ks"], g["stride"])), cdiv(g["wo"], 16), g["n"]
    th, tw = TILE[kernel]
    return cdiv(g["ho"], th), cdiv(g["wo"], tw), g["n"]


# ---- the walks ------------------------------------------------------------------------------------------------------------------------
def dma_walk(tiles_h, tiles_w, n_img, nsplit):
    """conv_wgrad_dma_kernel's tile cursor, statement by statement (D_THW = 8, D_TWW = 16): per work-group the (n, h0, w0) it visits,
    plus the carries the walk took.  n_mine = ceil((n_pt - split) / nsplit)."""
    THW, TWW = 8, 16
    n_pt = n_img * tiles_h * tiles_w
    adv_w, adv_q = (nsplit % tiles_w) * TWW, nsplit // tiles_w
    adv_h, adv_n = (adv_q % tiles_h) * THW, adv_q // tiles_h
    lim_w, lim_h = tiles_w * TWW, tiles_h * THW
    seen = {"col_carry": False, "row_carry": False, "image_cross": False}
    per_wg = []
    for split in range(nsplit):
        n_mine = (n_pt - split + nsplit - 1) // nsplit
        t = split
        w0 = (t % tiles_w) * TWW
        t //= tiles_w
        h0, n = (t % tiles_h) * THW, t // tiles_h
        mine = []
        for idx in range(n_mine):
            if idx > 0:
                w0 += adv_w
                cy = w0 >= lim_w
                w0 -= lim_w if cy else 0
                seen["col_carry"] |= cy
                h0 += adv_h + (THW if cy else 0)
                cy = h0 >= lim_h
                h0 -= lim_h if cy else 0
                seen["row_carry"] |= cy
                n_prev = n
                n += adv_n + int(cy)
                seen["image_cross"] |= n != n_prev
            mine.append((n, h0 // THW, w0 // TWW))
        per_wg.append(mine)
    return per_wg, seen


def stride_walk(tiles_h, tiles_w, n_img, nsplit):
    """the general / stride-2 / thin kernels: tiles split, split + nsplit, ... decoded (n, row, column) by division"""
    n_pt = n_img * tiles_h * tiles_w
    per_wg, cross = [], False
    for split in range(nsplit):
        mine = []
        for pt in range(split, n_pt, nsplit):
            tw_i, t = pt % tiles_w, pt // tiles_w
            mine.append((t // tiles_h, t % tiles_h, tw_i))
        cross |= any(a[0] != b[0] for a, b in zip(mine, mine[1:]))
        per_wg.append(mine)
    return per_wg, {"image_cross": cross}


def chunk_walk(n_chunks, nsplit):
    """wgrad1x1_kernel: 64-pixel chunks split, split + nsplit, ..."""
    return [list(range(s, n_chunks, nsplit)) for s in range(nsplit)], {}


def range_walk(m, pps, nsplit):
    """wgrad1x1_f32_kernel: work-group `split` owns pixels [split * pps, min(M, split * pps + pps))"""
    return [list(range(s * pps, min(m, s * pps + pps))) for s in range(nsplit)], {}


def reduce_variant(kernel, ks, tot):
    """which reduce adds the `tot` slabs: 'up2' (mas_wgrad_reduce_up2), or mas_wgrad_reduce's G (misc.hip: 16 iff tot >= 32 and ks > 1)"""
    if kernel == "conv_wgrad_up2":
        return "up2"
    return "G16" if tot >= 32 and ks > 1 else "G4"


def walk(kernel, g, nsplit):
    """(per work-group unit lists, regime flags of the walk) for one launch of `kernel` at geometry g with `nsplit` work-groups"""
    if kernel == "conv_wgrad_dma" or kernel == "conv_wgrad_up2":
        th, tw, nimg = tile_grid(kernel, g)
        per_wg, seen = dma_walk(th, tw, nimg, nsplit)
    elif kernel in ("wgrad_s2", "wgrad_thin", "conv_wgrad_tr", "conv_wgrad"):
        th, tw, nimg = tile_grid(kernel, g)
        per_wg, seen = stride_walk(th, tw, nimg, nsplit)
    elif kernel == "wgrad1x1":
        per_wg, seen = chunk_walk(cdiv(g["n"] * g["h"] * g["w"], 64), nsplit)
    elif kernel == "wgrad1x1_f32":
        m = g["n"] * g["h"] * g["w"]
        pps = roundup(cdiv(m, nsplit), 32)
        assert cdiv(m, pps) == nsplit, "an fp32 1x1 split count pw_f32_setup cannot produce"
        per_wg, seen = range_walk(m, pps, nsplit)
    else:
        raise KeyError(kernel)
    units = n_units(kernel, g)
    loads = [len(u) for u in per_wg]
    seen = dict(seen)
    seen["nsplit1"] = nsplit == 1
    seen["one_per_wg"] = max(loads) == 1
    seen["multi_per_wg"] = max(loads) >= 2
    seen["uneven"] = (units % pps != 0) if kernel == "wgrad1x1_f32" else units % nsplit != 0     # (fp32 1x1: a short last range)
    seen["at_ceiling"] = nsplit == ceiling(kernel, g)
    return per_wg, seen


def covers_once(kernel, g, per_wg):
    """every unit of the launch appears in exactly one work-group's walk, exactly once"""
    flat = [u for mine in per_wg for u in mine]
    if kernel in ("wgrad1x1", "wgrad1x1_f32"):
        want = list(range(n_units(kernel, g)))
        return sorted(flat) == want
    th, tw, nimg = tile_grid(kernel, g)
    want = sorted((n, r, c) for n in range(nimg) for r in range(th) for c in range(tw))
    return sorted(flat) == want
