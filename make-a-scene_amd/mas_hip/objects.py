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
its ``tolist``).  ``pack`` and ``make_plan`` are pure functions of the boxes."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ACT_NONE, OBJ_ALIGN, OBJ_CANVAS_C, OBJ_MIN_SIDE, ObjPlan, _DT, _image, _ptr as _p, _require_cuda, _stream, check, lib
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
# kernel calls
# --------------------------------------------------------------------------- #
def _nhwc(n, c, h, w, dtype, device):
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)


def canvas_fwd(img, rec, p: ObjPlan, shift, scale, dtype):
    """[2 * n_canvas, 8, H, W] (channels_last): the scaled crops of img (first half) and rec (second half), zeros elsewhere"""
    out = _nhwc(2 * p.n_canvas, CP, p.H, p.W, dtype, img.device)
    gi, gr = _image(img, "ObjectLoss"), _image(rec, "ObjectLoss")
    check(lib().mas_obj_canvas_fwd(C.byref(gi), C.byref(gr), C.byref(p), _p(shift), _p(scale), _p(out), _DT[dtype], _stream()),
          "obj_canvas_fwd")
    return out


def canvas_bwd(dcanvas, p: ObjPlan, scale, like):
    """d ``like`` (its dtype and strides, written in full) from the rec-side canvas gradient [n_canvas, 8, H, W]"""
    drec = torch.empty_like(like)
    g = _image(drec, "ObjectLoss")
    check(lib().mas_obj_canvas_bwd(_p(dcanvas), _DT[dcanvas.dtype], C.byref(p), _p(scale), C.byref(g), _stream()), "obj_canvas_bwd")
    return drec


def relu_fwd(y, p: ObjPlan, level: int):
    n, c = y.shape[:2]
    check(lib().mas_obj_relu_fwd(_p(y), C.byref(p), level, n, c, _DT[y.dtype], _stream()), "obj_relu_fwd")
    return y


def relu_bwd(da, a, out=None):
    dy = da if out is None else out
    check(lib().mas_obj_relu_bwd(_p(da), _p(a), _p(dy), a.numel(), _DT[a.dtype], _stream()), "obj_relu_bwd")
    return dy


def pool_fwd(x, p: ObjPlan, level: int):
    n, c, h, w = x.shape
    y = _nhwc(n, c, h // 2, w // 2, x.dtype, x.device)
    check(lib().mas_obj_pool_fwd(_p(x), _p(y), C.byref(p), level, n, c, _DT[x.dtype], _stream()), "obj_pool_fwd")
    return y


def pool_bwd(a, seed, dz, p: ObjPlan, level: int):
    n, c = a.shape[:2]
    dy = torch.empty_like(a)
    check(lib().mas_obj_pool_bwd(_p(a), _p(seed), _p(dz), _p(dy), C.byref(p), level, n, c, _DT[a.dtype], _stream()), "obj_pool_bwd")
    return dy


def head_fwd(feat, w, p: ObjPlan, plan: Plan, level: int, partial):
    c = feat.shape[1]
    check(lib().mas_obj_head_fwd(_p(feat), _p(w), C.byref(p), level, c, _DT[feat.dtype], plan.level_blocks(level), _p(partial), _stream()),
          "obj_head_fwd")


def finalize(partial, p: ObjPlan, device):
    out = torch.empty(1 + p.n_cells, dtype=torch.float32, device=device)
    check(lib().mas_obj_finalize(_p(partial), C.byref(p), _p(out), _stream()), "obj_finalize")
    return out


def head_bwd(feat, w, p: ObjPlan, level: int, dout):
    """the rec side's seed [n_canvas, C, H >> l, W >> l] (channels_last)"""
    nc = p.n_canvas
    c, h, wd = feat.shape[1:]
    seed = _nhwc(nc, c, h, wd, feat.dtype, feat.device)
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
        p, nc = ctx.p, ctx.p.n_canvas
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
        drec = canvas_bwd(d, p, ctx.scale, rec)
        return None, drec, None, None, None


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
