"""``mas_hip.objects.ObjectAtlas`` without a GPU: the atlas of the object term at fixed capacity.  Its plan is ``make_plan`` on the
atlas's canvases cell for cell; the table it writes has the fixed strides of include/mas_hip.h (restated here in numpy and compared
with the bytes); the head's fixed grid bounds every plan's block count; an overflow is refused and leaves the table alone."""
import random

import numpy as np
import pytest
import torch

H, W, MAX = 96, 160, 8              # the small atlas of the GPU tests: one canvas of 6 x 10 tiles
CHANNELS = (64, 128, 256, 512, 512)


def _atlas(n_images=2, **kw):
    from mas_hip import objects as O
    return O.ObjectAtlas("cpu", n_images, **dict(dict(height=H, width=W, canvases=1, max_cells=MAX), **kw))


def _seeded_boxes(rng, n_images=2, size=64):
    """0..4 boxes of 8..64 px per image, some partly outside the image, some under 16 px on a side (not used)"""
    out = []
    for _ in range(n_images):
        boxes = []
        for _ in range(rng.randint(0, 4)):
            h, w = rng.randint(8, 64), rng.randint(8, 64)
            y0, x0 = rng.randint(-h // 3, size - 2 * h // 3), rng.randint(-w // 3, size - 2 * w // 3)
            boxes.append([x0, y0, x0 + w, y0 + h])
        out.append(boxes)
    return out


def _restated_table(atlas, plan):
    """the table of include/mas_hip.h, written down independently: header | cells | img_cell0 | blk0 [5][max + 1] | tiles"""
    n = 0 if plan is None else plan.n_cells
    header = np.array([n, atlas.max_cells, atlas.n_images, atlas.n_canvas, atlas.H, atlas.W, 0, 0], dtype=np.int32)
    cells = np.zeros((atlas.max_cells, 8), dtype=np.int32)
    img0 = np.full(atlas.n_images + 1, n, dtype=np.int32)
    blk0 = np.zeros((5, atlas.max_cells + 1), dtype=np.int32)
    tiles = np.full((atlas.n_canvas, atlas.H // 16, atlas.W // 16), -1, dtype=np.int32)
    if plan is not None:
        img0[:len(plan.img_cell0)] = plan.img_cell0
        for k, (c, oy, ox, h, w, b, top, left) in enumerate(plan.cells):
            cells[k] = (c, oy, ox, h, w, b, top, left)
            tiles[c, oy // 16:-(-(oy + h) // 16), ox // 16:-(-(ox + w) // 16)] = k
        for l, ch in enumerate(CHANNELS):
            blocks = [-(-((h >> l) * (w >> l)) // (8192 // ch)) for (_, _, _, h, w, *_r) in plan.cells]
            blk0[l, 1:n + 1] = np.cumsum(blocks)
            blk0[l, n + 1:] = blk0[l, n]
    return np.concatenate([header, cells.reshape(-1), img0, blk0.reshape(-1), tiles.reshape(-1)])


def _bytes(t):
    return t.numpy().tobytes()


def test_plan_is_make_plan_on_the_atlas_and_the_table_has_fixed_strides():
    from mas_hip import objects as O
    atlas = _atlas()
    boxes = [[[4, 6, 40, 50], [10, -5, 30, 25], [0, 0, 10, 40]], [[20, 20, 48, 50]]]     # one box under 16 px wide, two outside the image
    plan, want = atlas.plan(boxes), O.make_plan(boxes, 2, width=W, max_height=H)
    assert plan.cells == want.cells and plan.img_cell0 == want.img_cell0 and plan.blk0 == want.blk0 and plan.n_cells == 3
    assert (plan.n_canvas, plan.W) == (1, W) and plan.H <= H
    assert atlas.write(boxes) == 3 and atlas.n_cells == 3
    table = _restated_table(atlas, want)
    assert atlas.n_ints == table.size == 8 + 8 * MAX + 3 + 5 * (MAX + 1) + 6 * 10
    assert _bytes(atlas.dev) == table.tobytes()
    assert _bytes(atlas._host[0]) == table.tobytes()                 # the pinned image the copy was issued from
    a = atlas.dev.numpy()
    assert a[0] == 3 and list(a[atlas.o_img0:atlas.o_blk0]) == [0, 2, 3]
    blk = a[atlas.o_blk0:atlas.o_tiles].reshape(5, MAX + 1)
    assert [list(r[:4]) for r in blk] == want.blk0 and all((r[4:] == r[3]).all() for r in blk)
    assert 0 < atlas.efficiency() == sum(c[3] * c[4] for c in want.cells) / float(H * W) < 1
    from mas_hip import lib
    assert lib().mas_obj_atlas_ints(MAX, 2, 1, H, W) == atlas.n_ints
    assert [lib().mas_obj_head_grid_dev(l, MAX, 1, H, W) for l in range(5)] == atlas.grids
    assert lib().mas_obj_atlas_ints(MAX, 2, 1, H + 8, W) < 0 and lib().mas_obj_head_grid_dev(5, MAX, 1, H, W) < 0


def test_fewer_box_lists_than_images_and_two_buffers():
    atlas = _atlas(n_images=3)
    one = [[[0, 0, 32, 32]]]                                          # the zip stops at the shorter: images 1 and 2 have no cell
    assert atlas.write(one) == 1
    assert list(atlas.dev.numpy()[atlas.o_img0:atlas.o_blk0]) == [0, 1, 1, 1]
    two = [[], [[5, 5, 40, 30]], [[1, 2, 20, 60]]]
    assert atlas.write(two) == 2
    assert _bytes(atlas._host[0]) == _restated_table(atlas, atlas.plan(one)).tobytes()       # the buffers alternate
    assert _bytes(atlas._host[1]) == _bytes(atlas.dev) == _restated_table(atlas, atlas.plan(two)).tobytes()


def test_fixed_grid_bounds_every_plan_and_partials_do_not_overlap():
    from mas_hip import objects as O
    atlas = _atlas()
    want_grids = [-(-((H >> l) * (W >> l)) // (8192 // c)) + MAX for l, c in enumerate(CHANNELS)]
    assert atlas.grids == want_grids and atlas.n_partial == sum(want_grids)
    assert atlas.partial_offsets == [sum(want_grids[:l]) for l in range(5)]
    rng, fit, small, outside = random.Random(2024), 0, 0, 0
    for _ in range(1000):
        boxes = _seeded_boxes(rng)
        if not atlas.fits(boxes):
            continue
        plan = atlas.plan(boxes)
        if plan is None:
            continue
        fit += 1
        small += any(not O.is_used(b) for bs in boxes for b in bs)
        outside += any(b[0] < 0 or b[1] < 0 or b[2] > 64 or b[3] > 64 for bs in boxes for b in bs if O.is_used(b))
        for l in range(5):
            assert plan.level_blocks(l) <= atlas.grids[l], (boxes, l)
            # level l's partial sums [off_l, off_l + blocks) end before level l + 1's begin
            assert atlas.partial_offsets[l] + plan.level_blocks(l) <= (atlas.partial_offsets[l + 1] if l < 4 else atlas.n_partial)
        assert plan.n_cells <= MAX and all(oy + h <= H and ox + w <= W and n == 0 for (n, oy, ox, h, w, *_r) in plan.cells)
    assert fit >= 200 and small >= 20 and outside >= 20, (fit, small, outside)


def test_overflow_by_area_and_by_count_leaves_the_table_alone():
    from mas_hip import objects as O
    atlas = _atlas()
    good = [[[0, 0, 40, 40]], [[8, 8, 60, 50]]]
    atlas.write(good)
    before = _bytes(atlas.dev)
    by_area = [[[0, 0, 64, 64], [0, 0, 60, 60]], [[0, 0, 64, 60]]]                     # three 80-px footprints: 96 x 160 holds two
    by_count = [[[4 * k, 0, 4 * k + 16, 16] for k in range(5)], [[0, 4 * k, 16, 4 * k + 16] for k in range(4)]]     # nine crops, eight cells
    too_wide = [[[-50, 0, 100, 20]], []]                                                 # a 150-px crop: footprint 176 > 160
    too_tall = [[[0, -10, 20, 80]], []]                                                  # a 90-px crop: footprint 112 > 96
    assert issubclass(O.AtlasOverflow, ValueError)
    for boxes, n_out in ((by_area, 1), (by_count, 1), (too_wide, 1), (too_tall, 1)):
        assert not atlas.fits(boxes)
        with pytest.raises(O.AtlasOverflow, match=rf"{n_out} of \d+ used crops \(\d+ of \d+ px") as e:
            atlas.write(boxes)
        assert isinstance(e.value, ValueError)
        assert _bytes(atlas.dev) == before and atlas.n_cells == 2
    with pytest.raises(ValueError):
        atlas.write([[[0, 0, 40]], []])                                                  # a malformed box
    assert _bytes(atlas.dev) == before
    assert atlas.fits(good) and atlas.fits([[], []]) and atlas.fits(by_count[:1])
    # the same boxes fit an atlas of twice the area / one more cell
    assert _atlas(height=2 * H).fits(by_area) and _atlas(max_cells=9).fits(by_count)
    assert _atlas(canvases=2).fits(by_area) and _atlas(canvases=2).plan(by_area).n_canvas == 2


def test_empty_box_list_writes_an_empty_table():
    atlas = _atlas()
    fresh = _bytes(atlas.dev)
    assert fresh == _restated_table(atlas, None).tobytes()            # as constructed: empty
    atlas.write([[[0, 0, 40, 40]], []])
    for empty in ([[], []], None, [[[0, 0, 10, 40]], [[5, 5, 60, 12]]]):
        assert atlas.write(empty) == 0 and atlas.n_cells == 0 and atlas.plan(empty if empty is not None else []) is None
        a = atlas.dev.numpy()
        assert a[0] == 0 and (a[atlas.o_tiles:] == -1).all() and _bytes(atlas.dev) == fresh
        atlas.write([[[0, 0, 40, 40]], []])
    assert atlas.efficiency() == 40 * 40 / float(H * W)


def test_geometry_is_checked_and_the_default_holds_eight_256_crops():
    from mas_hip import objects as O
    for kw in (dict(height=100), dict(width=8), dict(max_cells=0), dict(canvases=0), dict(n_images=0), dict(max_cells=5000)):
        with pytest.raises(ValueError):
            _atlas(**kw)
    atlas = O.ObjectAtlas("cpu", 2)
    assert (atlas.H, atlas.W, atlas.n_canvas, atlas.max_cells) == (544, 1088, 1, 64)
    eight = [[[0, 0, 256, 256]] * 4] * 2
    assert atlas.fits(eight) and not atlas.fits([[[0, 0, 256, 256]] * 5, [[0, 0, 256, 256]] * 4])
    assert atlas.dev.dtype == torch.int32 and atlas.dev.numel() == atlas.n_ints
