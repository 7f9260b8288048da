"""The object-aware term of the VQ-IMG objective (Make-A-Scene section 3.2) as ONE autograd node over libmas_hip (csrc/object.hip +
the convolution dispatch): LPIPS-VGG16 on every object crop of the batch at once.

The term (the reference's commented block, losses/loss_img.py): for every image, the boxes with both sides >= 16 px are cropped from
the real and the reconstructed image (torchvision ``crop``: the part outside the image is 0), each pair goes through LPIPS in
evaluation mode, and the image contributes ``sum / (n_used + 1)``; the term is the SUM over images.

The "atlas": the host packer places every used crop at a 16-aligned origin of one or a few NHWC canvases, with a zero gutter of
>= 16 px after each; the real crops and the rec crops take the same places in two canvas images.  Each of VGG16's thirteen
convolutions then runs once for the whole batch, and after each one a ReLU + mask pass zeroes everything outside the crops' valid
rectangles of that level -- so every crop's values are those of an isolated LPIPS on it.  The backward runs VGG on the rec canvas
only (the real side's features are kept from the forward) and reaches ``reconstructions`` only: ``images`` is data.

Everything here is computed from host data: list boxes cost no device-to-host synchronisation (a box tensor on the GPU costs one,
its ``tolist``).  ``pack`` and ``make_plan`` are pure functions of the boxes.

``ObjectAtlas`` / ``object_loss_static``: the same term at fixed capacity.  The canvases' geometry and the number of cells are fixed
at construction, and the cells sit in ONE device table with fixed strides that the host rewrites before each call (planning stays here,
on the host boxes); the node's launches, grids and shapes then depend on the atlas alone, so a captured graph of it follows the table
of each replay (``mas_hip.graphs.GraphedGanStep``)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ACT_NONE, OBJ_ALIGN, OBJ_ATLAS_HEADER, OBJ_CANVAS_C, OBJ_MIN_SIDE, ObjPlan, _DT, _image, _ptr as _p, _require_cuda, _stream, check, lib
from . import ops

# ALIGN, MIN_SIDE and CP are the header's MAS_OBJ_ALIGN, MAS_OBJ_MIN_SIDE and MAS_OBJ_CANVAS_C
ALIGN = OBJ_ALIGN     # crop origins (and canvas sizes) are multiples of 16: every 2x2 pool window of a valid output stays in one crop
GUTTER = 16           # zeros after every crop: >= 1 zero pixel between crops down to level 4 (16 >> 4)
MIN_SIDE = OBJ_MIN_SIDE   # a box with a side under 16 px is skipped (VGG's fourth pool would have no output: the reference raises)
CANVAS_W = 1024       # canvas width (wider when a crop needs it)
CANVAS_H_MAX = 2048   # canvas height before a new canvas starts (taller when a crop needs it)
CP = OBJ_CANVAS_C     # canvas channels: RGB and five zeros (the first convolution's input, one 16-byte bf16 vector)
LEVELS = 5
CHANNELS = (64, 128, 256, 512, 512)


def head_pixels(c: int) -> int:
    """pixels per block of the head's forward (``MAS_OBJ_HEAD_PIX``)"""
    return 8192 // c


def _ceil(v: int, a: int = ALIGN) -> int:
    return -(-v // a) * a


# --------------------------------------------------------------------------- #
# boxes and packing (host, pure)
# --------------------------------------------------------------------------- #
def box_lists(bbox_obj):
    """One list of integer [x_min, y_min, x_max, y_max] per image: what the reference's ``collate_fn`` produces, or a [B, K, 4]
    tensor converted with ``int()`` as the collate does (a tensor on the GPU costs one synchronisation)."""
    if isinstance(bbox_obj, torch.Tensor):
        if bbox_obj.dim() != 3 or bbox_obj.shape[-1] != 4:
            raise ValueError(f"ObjectLoss: a box tensor must be [B, K, 4], got {tuple(bbox_obj.shape)}")
        bbox_obj = bbox_obj.tolist()
    return [[[int(v) for v in box[:4]] for box in boxes] for boxes in bbox_obj]


def is_used(box) -> bool:
    """both sides >= 16 px (the reference raises on a smaller box: INTEGRATION section 3)"""
    x0, y0, x1, y1 = box[:4]
    return (y1 - y0) >= MIN_SIDE and (x1 - x0) >= MIN_SIDE


def used_boxes(bbox_obj, n_images: int):
    """[(image, box)] in the reference's order (``zip`` stops at the shorter of images and box lists), and the first entry of every
    image: img_cell0 [n + 1], n = the number of images the zip visits."""
    lists = box_lists(bbox_obj)
    n = min(n_images, len(lists))
    cells, img0 = [], [0]
    for b in range(n):
        cells += [(b, box) for box in lists[b] if is_used(box)]
        img0.append(len(cells))
    return cells, img0


def pack(sizes, width: int = CANVAS_W, max_height: int = CANVAS_H_MAX):
    """Shelf packing of (h, w) crops: -> (origins [(canvas, oy, ox)] in the order of ``sizes``, n_canvas, H, W).  A crop's
    footprint is its size plus the gutter, rounded up to 16; footprints never overlap, so every origin is 16-aligned and every crop
    is followed by >= 16 zero rows and columns.  Crops are placed tallest first; H is the tallest canvas's used height."""
    if not sizes:
        return [], 0, 0, 0
    fp = [(_ceil(h + GUTTER), _ceil(w + GUTTER)) for h, w in sizes]
    W = max(_ceil(width), max(f[1] for f in fp))
    hmax = max(_ceil(max_height), max(f[0] for f in fp))
    order = sorted(range(len(sizes)), key=lambda i: (-fp[i][0], -fp[i][1], i))
    origins = [None] * len(sizes)
    n, y, x, shelf = 0, 0, 0, 0
    used = [0]
    for i in order:
        fh, fw = fp[i]
        if x + fw > W:
            y, x, shelf = y + shelf, 0, 0
        if y + fh > hmax:
            n, y, x, shelf = n + 1, 0, 0, 0
            used.append(0)
        origins[i] = (n, y, x)
        x += fw
        shelf = max(shelf, fh)
        used[n] = max(used[n], y + fh)
    return origins, n + 1, max(used), W


class Plan:
    """The atlas of one call (host side): cells (n, oy, ox, h, w, b, top, left) in (image, box) order, img_cell0, the canvas
    geometry, the 16 x 16 tile map and the head's block table.  ``table()`` is the int32 image of the device tables."""

    def __init__(self, cells, img_cell0, n_canvas, H, W):
        self.cells, self.img_cell0 = cells, img_cell0
        self.n_cells, self.n_images = len(cells), len(img_cell0) - 1
        self.n_canvas, self.H, self.W = n_canvas, H, W
        self.tiles = np.full((n_canvas, H // ALIGN, W // ALIGN), -1, dtype=np.int32)
        for k, (n, oy, ox, h, w, *_rest) in enumerate(cells):
            t = self.tiles[n, oy // ALIGN:-(-(oy + h) // ALIGN), ox // ALIGN:-(-(ox + w) // ALIGN)]
            if (t >= 0).any():
                raise AssertionError("ObjectLoss: two crops share a 16 x 16 tile")
            t[...] = k
        self.blocks = []                      # [level][cell]
        for l, c in enumerate(CHANNELS):
            self.blocks.append([-(-((h >> l) * (w >> l)) // head_pixels(c)) for (_, _, _, h, w, *_r) in cells])
        self.blk0 = [[0] + np.cumsum(bl).tolist() for bl in self.blocks]

    def level_blocks(self, l: int) -> int:
        return self.blk0[l][-1]

    def efficiency(self) -> float:
        """crop area / canvas area: the share of the convolutions' pixels that belong to a crop"""
        return sum(h * w for (_, _, _, h, w, *_r) in self.cells) / float(self.n_canvas * self.H * self.W)

    def table(self):
        """-> (int32 array, element offsets of cells, img_cell0, blk0, tiles)"""
        parts = [np.asarray(self.cells, dtype=np.int32).reshape(-1), np.asarray(self.img_cell0, dtype=np.int32),
                 np.asarray(self.blk0, dtype=np.int32).reshape(-1), self.tiles.reshape(-1)]
        offs = np.cumsum([0] + [p.size for p in parts[:-1]]).tolist()
        return np.concatenate(parts), offs


def make_plan(bbox_obj, n_images: int, width: int = CANVAS_W, max_height: int = CANVAS_H_MAX):
    """boxes -> Plan, or None when no box is used"""
    used, img0 = used_boxes(bbox_obj, n_images)
    if not used:
        return None
    sizes = [(box[3] - box[1], box[2] - box[0]) for _, box in used]
    origins, nc, H, W = pack(sizes, width, max_height)
    cells = [(n, oy, ox, h, w, b, box[1], box[0]) for (b, box), (h, w), (n, oy, ox) in zip(used, sizes, origins)]
    return Plan(cells, img0, nc, H, W)


def upload(plan: Plan, device):
    """-> (device int32 tensor, ObjPlan pointing into it): one host-to-device copy from pinned memory, no synchronisation"""
    arr, offs = plan.table()
    host = torch.from_numpy(arr)
    if device.type == "cuda":
        host = host.pin_memory()
    dev = host.to(device, non_blocking=True)
    base = dev.data_ptr()
    p = ObjPlan(base + 4 * offs[0], base + 4 * offs[1], base + 4 * offs[3], base + 4 * offs[2], plan.n_cells, plan.n_images, plan.n_canvas,
                plan.H, plan.W, 0)
    return dev, p


# --------------------------------------------------------------------------- #
# the atlas at fixed capacity (what a captured graph reads)
# --------------------------------------------------------------------------- #
ATLAS_HEADER = OBJ_ATLAS_HEADER    # MAS_OBJ_ATLAS_HEADER: {n_cells, max_cells, n_images, n_canvas, H, W, 0, 0}
MAX_ATLAS_CELLS = 4096             # the library's bound on max_cells


class AtlasOverflow(ValueError):
    """the used crops of a call do not fit an ``ObjectAtlas``: too many of them, or too much area for its canvases"""


class ObjectAtlas:
    """The atlas at FIXED capacity: ``canvases`` canvases of ``height`` x ``width`` (multiples of 16) and at most ``max_cells`` crops,
    in ONE int32 table on ``device`` with fixed strides that the host rewrites before every call of the static node
    (``object_loss_static``) -- the only thing about a batch's boxes that reaches the device.  The geometry never changes after
    construction, so every tensor shape, grid and kernel argument of the node is a function of it and of the image shape, and a
    captured graph of the node follows the table of each replay (``mas_hip.graphs.GraphedGanStep``).

    The table (include/mas_hip.h, ``mas_obj_*_dev``): header [8] = {n_cells, max_cells, n_images, n_canvas, H, W, 0, 0} | cells
    [max_cells][8] | img_cell0 [n_images + 1] | blk0 [5][max_cells + 1] | tiles [canvases][H / 16][W / 16].  Unused cells are zeros,
    img_cell0 and every blk0 row repeat their last value, tiles outside the crops are -1.

    ``plan`` is pure host code (``used_boxes`` and the shelf ``pack`` with the atlas as ``width`` / ``max_height``) and works on a CPU
    ``device``.  ``write`` plans, fills a pinned host image of the whole table and issues ONE asynchronous copy on the current stream;
    nothing is read back.  TWO pinned buffers alternate, each with an event behind its copy, as in ``face.FaceTable``: a buffer is
    rewritten only after the copy issued from it two writes ago has completed.

    The default, one canvas of 544 x 1088 and 64 cells, holds eight 256 x 256 crops (a footprint is 272 px with the gutter: four per
    shelf, two shelves) -- four whole-picture objects per image at the reference's B = 2.  The node's cost follows the CANVAS area,
    whatever the boxes are: at B = 2 / accumulate 8 with 0 / 2 / 6 crops per image the replayed step takes 18.5 ms per call on this
    atlas and 19.5 ms on one of twice the area (the node alone 2.1 against 3.5 ms; the list path 1.3-1.5 ms on its tight canvas; the
    eager step 25-26 ms), so the default is the smallest canvas that holds such a batch, and a call that does not fit
    runs on the list path (``GraphedGanStep(on_overflow="eager")``).  Larger batches want ``canvases`` / ``max_cells`` scaled with B,
    and at B = 32 the replayed step is slower than the eager one."""

    def __init__(self, device, n_images, height=544, width=1088, canvases=1, max_cells=64):
        vals = dict(n_images=n_images, height=height, width=width, canvases=canvases, max_cells=max_cells)
        for k, v in vals.items():
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"ObjectAtlas: {k} must be a positive integer, got {v!r}")
        if height % ALIGN or width % ALIGN:
            raise ValueError(f"ObjectAtlas: height and width must be multiples of {ALIGN}, got {height} x {width}")
        if max_cells > MAX_ATLAS_CELLS or canvases * height * width > 1 << 28:
            raise ValueError(f"ObjectAtlas: at most {MAX_ATLAS_CELLS} cells and 2^28 canvas pixels, got {max_cells} cells and "
                             f"{canvases} x {height} x {width}")
        self.n_images, self.H, self.W, self.n_canvas, self.max_cells = n_images, height, width, canvases, max_cells
        self.height, self.width, self.canvases = height, width, canvases
        self.o_cells = ATLAS_HEADER
        self.o_img0 = self.o_cells + 8 * max_cells
        self.o_blk0 = self.o_img0 + n_images + 1
        self.o_tiles = self.o_blk0 + LEVELS * (max_cells + 1)
        self.n_ints = self.o_tiles + canvases * (height // ALIGN) * (width // ALIGN)
        # the head's fixed grid per level and the first partial of every level: the cells' level-l rectangles are disjoint and inside
        # the canvases and each cell rounds up to whole blocks once, so grids[l] >= every plan's level_blocks(l)
        self.grids = [-(-(canvases * (height >> l) * (width >> l)) // head_pixels(c)) + max_cells for l, c in enumerate(CHANNELS)]
        self.partial_offsets = np.cumsum([0] + self.grids[:-1]).tolist()
        self.n_partial = sum(self.grids)
        self.device = torch.device(device)
        pin = self.device.type == "cuda"
        self._host = [torch.zeros(self.n_ints, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
        self._events = [None, None]                         # behind the last copy issued from each pinned buffer
        self._turn = 0
        self.dev = torch.from_numpy(self.image(None)).to(self.device)      # an empty table
        self.n_cells, self.last_plan = 0, None

    def _overflow(self, used, plan):
        sizes = [(box[3] - box[1], box[2] - box[0]) for _, box in used]
        if plan is None:                                    # too many crops: the ones beyond max_cells have no slot
            out = sizes[self.max_cells:]
        else:
            out = [(h, w) for (n, oy, ox, h, w, *_r) in plan.cells
                   if n >= self.n_canvas or oy + _ceil(h + GUTTER) > self.H or ox + _ceil(w + GUTTER) > self.W]
        return AtlasOverflow(f"ObjectAtlas: {len(out)} of {len(sizes)} used crops ({sum(h * w for h, w in out)} of "
                             f"{sum(h * w for h, w in sizes)} px of crop area) do not fit {self.n_canvas} canvas(es) of {self.H} x {self.W} "
                             f"with {self.max_cells} cells (a crop's footprint is its size plus a {GUTTER} px gutter, rounded up to {ALIGN})")

    def plan(self, bbox_obj):
        """boxes -> ``Plan`` on this atlas's canvases (``make_plan(bbox_obj, n_images, width=W, max_height=H)`` cell for cell), or
        None when no box is used; ``AtlasOverflow`` when the crops are more than ``max_cells`` or leave the canvases"""
        used, _ = used_boxes(bbox_obj, self.n_images)
        if not used:
            return None
        if len(used) > self.max_cells:
            raise self._overflow(used, None)
        plan = make_plan(bbox_obj, self.n_images, self.W, self.H)
        if plan.n_canvas > self.n_canvas or plan.H > self.H or plan.W != self.W:
            raise self._overflow(used, plan)
        return plan

    def fits(self, bbox_obj) -> bool:
        try:
            self.plan(bbox_obj)
        except AtlasOverflow:
            return False
        return True

    def image(self, plan):
        """the int32 image of the whole table for ``plan`` (None: the empty table, n_cells = 0 and all tiles -1)"""
        a = np.zeros(self.n_ints, dtype=np.int32)
        n = 0 if plan is None else plan.n_cells
        a[:6] = (n, self.max_cells, self.n_images, self.n_canvas, self.H, self.W)
        tiles = a[self.o_tiles:].reshape(self.n_canvas, self.H // ALIGN, self.W // ALIGN)
        tiles[...] = -1
        if plan is not None:
            a[self.o_cells:self.o_cells + 8 * n] = np.asarray(plan.cells, dtype=np.int32).reshape(-1)
            img0 = a[self.o_img0:self.o_blk0]
            img0[:len(plan.img_cell0)] = plan.img_cell0
            img0[len(plan.img_cell0):] = n                  # images the boxes do not reach have no cells
            blk0 = a[self.o_blk0:self.o_tiles].reshape(LEVELS, self.max_cells + 1)
            for l in range(LEVELS):
                blk0[l, :n + 1] = plan.blk0[l]
                blk0[l, n + 1:] = plan.blk0[l][-1]
            tiles[:plan.n_canvas, :plan.H // ALIGN, :plan.W // ALIGN] = plan.tiles
        return a

    def write(self, bbox_obj) -> int:
        """plans the boxes on the host (a ValueError -- overflow, malformed boxes -- leaves the table as it was), then overwrites the
        device table with one asynchronous copy; -> the number of used crops (0: an empty table)"""
        plan = self.plan(bbox_obj if bbox_obj is not None else [])
        arr = self.image(plan)
        k = self._turn
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._host[k].copy_(torch.from_numpy(arr))
        self.dev.copy_(self._host[k], non_blocking=True)
        if self.device.type == "cuda":
            if self._events[k] is None:
                self._events[k] = torch.cuda.Event()
            self._events[k].record()
        self._turn = 1 - k
        self.n_cells, self.last_plan = (0 if plan is None else plan.n_cells), plan
        return self.n_cells

    def efficiency(self) -> float:
        """crop area of the last written boxes / canvas area"""
        if self.last_plan is None:
            return 0.0
        return sum(h * w for (_, _, _, h, w, *_r) in self.last_plan.cells) / float(self.n_canvas * self.H * self.W)

    def data_ptr(self):
        return self.dev.data_ptr()

    def _args(self):
        """what every ``mas_obj_*_dev`` entry takes about the atlas"""
        return C.c_void_p(self.dev.data_ptr()), self.max_cells, self.n_images, self.n_canvas, self.H, self.W


# --------------------------------------------------------------------------- #
# kernel calls (``p``: the ``ObjPlan`` of one call, or an ``ObjectAtlas`` -- the same passes on the fixed-capacity table)
# --------------------------------------------------------------------------- #
def _nhwc(n, c, h, w, dtype, device):
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)


def _fixed(p) -> bool:
    return isinstance(p, ObjectAtlas)


def canvas_fwd(img, rec, p, shift, scale, dtype):
    """[2 * n_canvas, 8, H, W] (channels_last): the scaled crops of img (first half) and rec (second half), zeros elsewhere"""
    out = _nhwc(2 * p.n_canvas, CP, p.H, p.W, dtype, img.device)
    gi, gr = _image(img, "ObjectLoss"), _image(rec, "ObjectLoss")
    if _fixed(p):
        check(lib().mas_obj_canvas_fwd_dev(C.byref(gi), C.byref(gr), *p._args(), _p(shift), _p(scale), _p(out), _DT[dtype], _stream()),
              "obj_canvas_fwd_dev")
        return out
    check(lib().mas_obj_canvas_fwd(C.byref(gi), C.byref(gr), C.byref(p), _p(shift), _p(scale), _p(out), _DT[dtype], _stream()),
          "obj_canvas_fwd")
    return out


def canvas_bwd(dcanvas, p, scale, like):
    """d ``like`` (its dtype and strides, written in full) from the rec-side canvas gradient [n_canvas, 8, H, W]"""
    drec = torch.empty_like(like)
    g = _image(drec, "ObjectLoss")
    if _fixed(p):
        check(lib().mas_obj_canvas_bwd_dev(_p(dcanvas), _DT[dcanvas.dtype], *p._args(), _p(scale), C.byref(g), _stream()), "obj_canvas_bwd_dev")
        return drec
    check(lib().mas_obj_canvas_bwd(_p(dcanvas), _DT[dcanvas.dtype], C.byref(p), _p(scale), C.byref(g), _stream()), "obj_canvas_bwd")
    return drec


def relu_fwd(y, p, level: int):
    n, c = y.shape[:2]
    if _fixed(p):
        check(lib().mas_obj_relu_fwd_dev(_p(y), *p._args(), level, n, c, _DT[y.dtype], _stream()), "obj_relu_fwd_dev")
        return y
    check(lib().mas_obj_relu_fwd(_p(y), C.byref(p), level, n, c, _DT[y.dtype], _stream()), "obj_relu_fwd")
    return y


def relu_bwd(da, a, out=None):
    dy = da if out is None else out
    check(lib().mas_obj_relu_bwd(_p(da), _p(a), _p(dy), a.numel(), _DT[a.dtype], _stream()), "obj_relu_bwd")
    return dy


def pool_fwd(x, p, level: int):
    n, c, h, w = x.shape
    y = _nhwc(n, c, h // 2, w // 2, x.dtype, x.device)
    if _fixed(p):
        check(lib().mas_obj_pool_fwd_dev(_p(x), _p(y), *p._args(), level, n, c, _DT[x.dtype], _stream()), "obj_pool_fwd_dev")
        return y
    check(lib().mas_obj_pool_fwd(_p(x), _p(y), C.byref(p), level, n, c, _DT[x.dtype], _stream()), "obj_pool_fwd")
    return y


def pool_bwd(a, seed, dz, p, level: int):
    n, c = a.shape[:2]
    dy = torch.empty_like(a)
    if _fixed(p):
        check(lib().mas_obj_pool_bwd_dev(_p(a), _p(seed), _p(dz), _p(dy), *p._args(), level, n, c, _DT[a.dtype], _stream()), "obj_pool_bwd_dev")
        return dy
    check(lib().mas_obj_pool_bwd(_p(a), _p(seed), _p(dz), _p(dy), C.byref(p), level, n, c, _DT[a.dtype], _stream()), "obj_pool_bwd")
    return dy


def head_fwd(feat, w, p: ObjPlan, plan: Plan, level: int, partial):
    c = feat.shape[1]
    check(lib().mas_obj_head_fwd(_p(feat), _p(w), C.byref(p), level, c, _DT[feat.dtype], plan.level_blocks(level), _p(partial), _stream()),
          "obj_head_fwd")


def head_fwd_dev(feat, w, atlas: ObjectAtlas, level: int, partial):
    """level ``level`` on the atlas's fixed grid; ``partial``: the WHOLE buffer of ``atlas.n_partial`` floats (the level's offset is fixed)"""
    if feat.shape[1] != CHANNELS[level] or partial.numel() < atlas.n_partial:
        raise ValueError(f"ObjectLoss: level {level} has {CHANNELS[level]} channels and the atlas {atlas.n_partial} partial sums")
    check(lib().mas_obj_head_fwd_dev(_p(feat), _p(w), *atlas._args(), level, _DT[feat.dtype], _p(partial), _stream()), "obj_head_fwd_dev")


def finalize(partial, p, device):
    if _fixed(p):
        out = torch.empty(1 + p.max_cells, dtype=torch.float32, device=device)
        check(lib().mas_obj_finalize_dev(_p(partial), *p._args(), _p(out), _stream()), "obj_finalize_dev")
        return out
    out = torch.empty(1 + p.n_cells, dtype=torch.float32, device=device)
    check(lib().mas_obj_finalize(_p(partial), C.byref(p), _p(out), _stream()), "obj_finalize")
    return out


def head_bwd(feat, w, p, level: int, dout):
    """the rec side's seed [n_canvas, C, H >> l, W >> l] (channels_last)"""
    nc = p.n_canvas
    c, h, wd = feat.shape[1:]
    seed = _nhwc(nc, c, h, wd, feat.dtype, feat.device)
    if _fixed(p):
        if c != CHANNELS[level] or dout.numel() != 1 + p.max_cells:
            raise ValueError(f"ObjectLoss: level {level} has {CHANNELS[level]} channels and the atlas {1 + p.max_cells} outputs")
        check(lib().mas_obj_head_bwd_dev(_p(feat), _p(w), *p._args(), level, _DT[feat.dtype], _p(dout), _p(seed), _stream()), "obj_head_bwd_dev")
        return seed
    check(lib().mas_obj_head_bwd(_p(feat), _p(w), C.byref(p), level, c, _DT[feat.dtype], _p(dout), _p(seed), _stream()), "obj_head_bwd")
    return seed


# --------------------------------------------------------------------------- #
# the network
# --------------------------------------------------------------------------- #
def vgg_convs(lp):
    """[[nn.Conv2d] per level]: the 2, 2, 3, 3, 3 convolutions of ``lp.vgg``'s five slices"""
    return [[m for m in getattr(lp.vgg, f"slice{i + 1}") if isinstance(m, nn.Conv2d)] for i in range(LEVELS)]


def _weight(conv, level, j):
    """(OIHW weight, the parameters it comes from): the first convolution's 3 input channels padded to the canvas's 8"""
    if level == 0 and j == 0:
        return F.pad(conv.weight.detach(), (0, 0, 0, 0, 0, CP - conv.in_channels)), (conv.weight,)
    return conv.weight, None


def _conv(x, conv, level, j, transpose):
    n, _, h, w = x.shape
    wt, src = _weight(conv, level, j)
    cout, cin = wt.shape[:2]
    if transpose:
        cin, cout = cout, cin
    bias = None if transpose or conv.bias is None else conv.bias.detach().float()
    return ops.conv_fwd_raw(x, None, ops.ConvWeight(wt, transpose, src), bias, None, n, h, w, cin, h, w, cout, 3, 1, 1, 1, ACT_NONE, False,
                            x.dtype)


def network_forward(convs, canvas, p: ObjPlan):
    """canvas [2 n_canvas, 8, H, W] -> (the five masked ReLU features, every convolution's masked ReLU output per level)"""
    feats, acts, x = [], [], canvas
    for l in range(LEVELS):
        if l > 0:
            x = pool_fwd(x, p, l - 1)
        level_acts = []
        for j, conv in enumerate(convs[l]):
            x = relu_fwd(_conv(x, conv, l, j, False), p, l)
            level_acts.append(x)
        acts.append(level_acts)
        feats.append(x)
    return feats, acts


def _lin_weights(lp):
    return [lp.lins[i].model[1].weight.detach().float().reshape(-1).contiguous() for i in range(LEVELS)]


class _ObjectLoss(torch.autograd.Function):
    """img, rec -> [1 + n_cells] fp32: the loss, then every crop's LPIPS.  Forward: canvas, 13 x (convolution, ReLU + mask), 4
    masked pools, 5 heads, finalize -- 37 launches.  Backward (rec side): per level the head's seed, the pool backward with the ReLU
    mask, the convolutions' data gradients with the ReLU masks between them, and the canvas adjoint -- 32 launches."""

    @staticmethod
    def forward(ctx, img, rec, lp, plan, dtype):
        dev = img.device
        table, p = upload(plan, dev)
        shift = lp.scaling_layer.shift.detach().float().reshape(-1).contiguous()
        scale = lp.scaling_layer.scale.detach().float().reshape(-1).contiguous()
        convs = vgg_convs(lp)
        lins = _lin_weights(lp)
        canvas = canvas_fwd(img, rec, p, shift, scale, dtype)
        feats, acts = network_forward(convs, canvas, p)
        partial = torch.empty(sum(plan.level_blocks(l) for l in range(LEVELS)), dtype=torch.float32, device=dev)
        off = 0
        for l in range(LEVELS):
            head_fwd(feats[l], lins[l], p, plan, l, partial[off:])
            off += plan.level_blocks(l)
        out = finalize(partial, p, dev)
        ctx.plan, ctx.p, ctx.table, ctx.convs, ctx.lins, ctx.scale = plan, p, table, convs, lins, scale
        ctx.feats, ctx.acts = feats, acts
        ctx.save_for_backward(rec)
        return out

    @staticmethod
    def backward(ctx, dout):
        (rec,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        return None, _rec_gradient(ctx, ctx.p, rec, dout), None, None, None


def _rec_gradient(ctx, p, rec, dout):
    """d rec of either node (``p``: the call's ``ObjPlan`` or the ``ObjectAtlas``) from the saved rec-side maps"""
    nc = p.n_canvas
    dout = dout.float().contiguous()
    d = None                                   # gradient of the pooled input of the level above
    for l in range(LEVELS - 1, -1, -1):
        feat = ctx.feats[l]
        seed = head_bwd(feat, ctx.lins[l], p, l, dout)
        dy = pool_bwd(feat[nc:], seed, d, p, l)
        for j in range(len(ctx.convs[l]) - 1, -1, -1):
            da = _conv(dy, ctx.convs[l][j], l, j, True)
            if j > 0:
                dy = relu_bwd(da, ctx.acts[l][j - 1][nc:])
            else:
                d = da
    return canvas_bwd(d, p, ctx.scale, rec)


class _ObjectLossStatic(torch.autograd.Function):
    """``_ObjectLoss`` at fixed capacity: img, rec -> [1 + max_cells] fp32 (the loss, the used crops' LPIPS, zeros).  The cells come
    from an ``ObjectAtlas``; the canvases, the thirteen convolutions, the head's grids, ``partial`` and ``out`` have the atlas's
    geometry whatever the table holds, so the 37 + 32 launches, their arguments and every shape are the same for every batch --
    nothing is read on the host, and a captured graph of this node follows the table of each replay.  Outside the crops the canvases
    are zeros and the masks keep them so; an empty table gives ``out`` of exact zeros and d rec of exact zeros."""

    @staticmethod
    def forward(ctx, img, rec, lp, atlas, dtype):
        dev = img.device
        shift = lp.scaling_layer.shift.detach().float().reshape(-1).contiguous()
        scale = lp.scaling_layer.scale.detach().float().reshape(-1).contiguous()
        convs = vgg_convs(lp)
        lins = _lin_weights(lp)
        canvas = canvas_fwd(img, rec, atlas, shift, scale, dtype)
        feats, acts = network_forward(convs, canvas, atlas)
        partial = torch.empty(atlas.n_partial, dtype=torch.float32, device=dev)
        for l in range(LEVELS):
            head_fwd_dev(feats[l], lins[l], atlas, l, partial)
        out = finalize(partial, atlas, dev)
        ctx.atlas, ctx.convs, ctx.lins, ctx.scale = atlas, convs, lins, scale
        ctx.feats, ctx.acts = feats, acts
        ctx.save_for_backward(rec)
        return out

    @staticmethod
    def backward(ctx, dout):
        (rec,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        return None, _rec_gradient(ctx, ctx.atlas, rec, dout), None, None, None


def object_loss_static(lp, img, rec, atlas, dtype=None):
    """The object-aware term on an ``ObjectAtlas``: -> [1 + max_cells] fp32 (the loss, every used crop's LPIPS in (image, box) order,
    zeros in the unused slots), ALWAYS: the node runs whatever the table holds (whether a batch has a used crop at all is the
    caller's to decide from ``atlas.write``'s return value).  No host synchronisation; its backward reaches ``rec`` only."""
    _require_cuda(img, "ObjectLoss")
    _require_cuda(rec, "ObjectLoss")
    if img.shape != rec.shape:
        raise ValueError(f"ObjectLoss: images {tuple(img.shape)} and reconstructions {tuple(rec.shape)} differ")
    if atlas.device != img.device:
        raise RuntimeError(f"ObjectLoss: the atlas is on {atlas.device}, the images on {img.device}")
    if atlas.n_images > img.shape[0]:
        raise ValueError(f"ObjectLoss: the atlas was made for {atlas.n_images} images, the batch has {img.shape[0]}")
    dtype = dtype or ops.compute_dtype()
    if dtype not in _DT:
        raise TypeError(f"ObjectLoss: compute dtype {dtype}")
    return _ObjectLossStatic.apply(img, rec, lp, atlas, dtype)


def object_loss(lp, img, rec, bbox_obj, dtype=None):
    """The object-aware term on the HIP path: -> [1 + n_cells] fp32 (the loss, then every used crop's LPIPS in (image, box)
    order), or None when no box is used (nothing launched)."""
    _require_cuda(img, "ObjectLoss")
    _require_cuda(rec, "ObjectLoss")
    if img.shape != rec.shape:
        raise ValueError(f"ObjectLoss: images {tuple(img.shape)} and reconstructions {tuple(rec.shape)} differ")
    plan = make_plan(bbox_obj, min(img.shape[0], rec.shape[0]))
    if plan is None:
        return None
    dtype = dtype or ops.compute_dtype()
    if dtype not in _DT:
        raise TypeError(f"ObjectLoss: compute dtype {dtype}")
    return _ObjectLoss.apply(img, rec, lp, plan, dtype)
