"""FaceLoss (reference losses/face_loss.py) as ONE autograd node over libmas_hip (csrc/face.hip + the convolution dispatch).

Host side of the face-aware VQ-IMG term: the face geometry (torchvision's crop / ``Resize(256)`` / ``CenterCrop(254)`` rules, computed
from the host boxes -- no device-to-host synchronisation), the reference's ``faces[:6]`` row selection, and the frozen ResNet-50 in
evaluation mode, forward and data gradient.  Activations are NHWC in the compute dtype (bf16 by default, fp32 in parity mode).  The
backward runs the network only for the rows that come from ``rec``: they are always the tail of the surviving rows (the row pairs
are (q, half + q) and ``half = min(n, 3) <= n``), so it works on slices of the saved maps.

``FaceTable`` / ``_FaceLossStatic``: the same term at fixed capacity.  The rows sit in six fixed slots of a DEVICE table that the host
rewrites before each call (planning and checks stay here, on the host boxes); the node always runs six rows forward and the slice [3:6]
backward, so its launches and shapes do not depend on the boxes and a captured graph of it follows the table of each replay
(``mas_hip.graphs.GraphedGanStep``)."""
from __future__ import annotations

import ctypes as C

import torch

from . import ACT_NONE, FACE_SIZE, FACE_SLOTS, FACE_TABLE_INTS, FaceBnItem, FaceFeats, FaceRow, _DT, _image, _ptr as _p, _require_cuda, _stream, check, lib
from . import ops

FACE = FACE_SIZE      # CenterCrop(254): MAS_FACE_SIZE of include/mas_hip.h
RESIZE = 256          # Resize(256): the short side
MAX_ROWS = 6          # faces[:6] (reference face_loss.py:140)
ALPHAS = (0.1, 0.25 * 0.01, 0.25 * 0.1, 0.25 * 0.2, 0.25 * 0.02)


# --------------------------------------------------------------------------- #
# geometry (host)
# --------------------------------------------------------------------------- #
def resized_size(h: int, w: int):
    """torchvision ``Resize(256)`` on an h x w crop: the short side becomes 256, the long one ``int(256 * long / short)``."""
    if w <= h:
        return int(RESIZE * h / w), RESIZE
    return RESIZE, int(RESIZE * w / h)


def center_offsets(rh: int, rw: int):
    """torchvision ``CenterCrop(254)``: Python's ``round`` (halves to even)."""
    return int(round((rh - FACE) / 2.0)), int(round((rw - FACE) / 2.0))


def face_geometry(box):
    """[x_min, y_min, x_max, y_max] -> dict(top, left, h, w, rh, rw, ct, cl); a box without area is a ValueError (the reference's
    Resize would divide by zero)."""
    x0, y0, x1, y1 = (int(v) for v in box)
    h, w = y1 - y0, x1 - x0
    if h <= 0 or w <= 0:
        raise ValueError(f"FaceLoss: face box {[x0, y0, x1, y1]} has no area (height {h}, width {w})")
    rh, rw = resized_size(h, w)
    ct, cl = center_offsets(rh, rw)
    return dict(top=y0, left=x0, h=h, w=w, rh=rh, rw=rw, ct=ct, cl=cl)


def face_list(bboxes, n_images: int):
    """(image index, box) per face in the reference's order: images, then boxes (``zip(imgs, recs, bboxes)`` stops at the shorter)."""
    out = []
    for b, boxes in zip(range(n_images), bboxes):
        for box in boxes:
            out.append((b, box))
    return out


def surviving_rows(n: int):
    """The rows of ``cat([gt faces], [rec faces])[:6]`` as (src, face): src 0 = img, 1 = rec.  Pairs are (q, half + q),
    half = len // 2: for n = 4 that is (gt0, gt3), (gt1, rec0), (gt2, rec1); for n >= 6 no rec row survives."""
    return ([(0, i) for i in range(n)] + [(1, i) for i in range(n)])[:MAX_ROWS]


def plan(bboxes, n_images: int):
    """-> (n faces, list of MasFaceRow for the surviving rows).  Geometry of the dropped rows is still validated, as the reference
    crops them."""
    faces = face_list(bboxes, n_images)
    geo = [face_geometry(box) for _, box in faces]
    rows = []
    for src, i in surviving_rows(len(faces)):
        g = geo[i]
        rows.append(FaceRow(src, faces[i][0], g["top"], g["left"], g["h"], g["w"], g["rh"], g["rw"], g["ct"], g["cl"]))
    return len(faces), rows


# --------------------------------------------------------------------------- #
# the rows as six fixed slots of a device table (what a captured graph reads)
# --------------------------------------------------------------------------- #
SLOTS = FACE_SLOTS    # MAS_FACE_SLOTS of include/mas_hip.h
PAIRS = SLOTS // 2


class FaceSlots(C.Structure):
    """The table's MAS_FACE_TABLE_INTS int32 (include/mas_hip.h), named: six rows, six flags, the pair count, a zero."""
    _fields_ = [("row", FaceRow * SLOTS), ("valid", C.c_int32 * SLOTS), ("n_pairs", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(FaceRow) == 40 and C.sizeof(FaceSlots) == 4 * FACE_TABLE_INTS


def slots(bboxes, n_images: int):
    """-> (n faces, [6 x MasFaceRow or None]): surviving row q < half in slot q, row half + q in slot 3 + q (half = rows // 2 <= 3), so
    pair q is always (slot q, slot 3 + q) and every rec row sits in slots 3..5:  n = 1: gt0 | rec0;  n = 4: gt0 gt1 gt2 | gt3 rec0 rec1;
    n >= 6: gt only.  The pairing is ``plan``'s (the reference's), a box without area raises as there."""
    n, rows = plan(bboxes, n_images)
    half = len(rows) // 2
    out = [None] * SLOTS
    for q in range(half):
        out[q], out[PAIRS + q] = rows[q], rows[half + q]
    return n, out


def check_slots(records, n_images: int):
    """the library's ``check_rows`` conditions on every filled slot, and 0 <= b < n_images; raises ValueError"""
    if len(records) != SLOTS:
        raise ValueError(f"FaceLoss: a face table has {SLOTS} slots, got {len(records)} records")
    for s, r in enumerate(records):
        if r is None:
            continue
        if (r.h <= 0 or r.w <= 0 or r.rh < FACE or r.rw < FACE or r.ct < 0 or r.cl < 0 or r.ct + FACE > r.rh or r.cl + FACE > r.rw
                or r.src not in (0, 1)):
            raise ValueError(f"FaceLoss: slot {s} has an invalid geometry")
        if not 0 <= r.b < n_images:
            raise ValueError(f"FaceLoss: slot {s} names image {r.b} of a batch of {n_images}")
    if any((records[q] is None) != (records[PAIRS + q] is None) for q in range(PAIRS)) or \
            any(records[q] is None and records[q + 1] is not None for q in range(PAIRS - 1)):
        raise ValueError("FaceLoss: the filled slots must be the pairs (q, 3 + q) for q < n_pairs")


def pack_slots(records, n_images: int) -> FaceSlots:
    """the table (``FaceSlots``) of six slot records (checked first); an empty slot is all zeros"""
    check_slots(records, n_images)
    t = FaceSlots()
    for s, r in enumerate(records):
        if r is not None:
            t.row[s], t.valid[s] = r, 1
    t.n_pairs = sum(r is not None for r in records[:PAIRS])
    return t


class FaceTable:
    """One table of six face slots (``FaceSlots``: MAS_FACE_TABLE_INTS int32) on ``device`` that the host rewrites before every call of the static node (``_FaceLossStatic``) -- the only
    thing about a batch's faces that reaches the device, so a captured graph that reads the table follows the boxes of each replay.

    ``write`` fills a pinned host buffer and issues one asynchronous copy on the current stream; it reads nothing back.  TWO pinned
    buffers alternate, each with an event recorded behind its copy: a buffer is rewritten only after the copy issued from it two
    writes ago has completed (``event.synchronize()``: a wait on that one small copy, which has almost always finished long before).
    On a CPU ``device`` the table is a plain buffer (the packing can be looked at without a GPU)."""
    NBYTES = C.sizeof(FaceSlots)

    def __init__(self, device):
        self.dev = torch.zeros(self.NBYTES, dtype=torch.uint8, device=device)                 # all slots empty
        self.device = self.dev.device
        self._host = [torch.zeros(self.NBYTES, dtype=torch.uint8, pin_memory=self.device.type == "cuda") for _ in range(2)]
        self._events = [None, None]                         # behind the last copy issued from each pinned buffer
        self._turn = 0
        self.n_faces, self.n_images = 0, 0

    def write(self, bboxes, n_images: int) -> int:
        """plans and checks the boxes on the host (a ValueError leaves the table as it was), then overwrites the device table; -> n faces"""
        n, records = slots(bboxes if bboxes is not None else [], n_images)
        raw = bytes(pack_slots(records, n_images))
        k = self._turn
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._host[k].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        self.dev.copy_(self._host[k], non_blocking=True)
        if self.device.type == "cuda":
            if self._events[k] is None:
                self._events[k] = torch.cuda.Event()
            self._events[k].record()
        self._turn = 1 - k
        self.n_faces, self.n_images = n, int(n_images)
        return n

    def data_ptr(self):
        return self.dev.data_ptr()


def _rows_array(rows):
    arr = (FaceRow * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = r
    return arr


def crop_faces(img, rec, rows, dtype):
    """[R, 3, 254, 254] (channels_last, ``dtype``): CenterCrop(Resize(crop(.))) of every row, one launch."""
    out = torch.empty((len(rows), 3, FACE, FACE), dtype=dtype, device=img.device, memory_format=torch.channels_last)
    gi, gr = _image(img, "FaceLoss"), _image(rec, "FaceLoss")
    check(lib().mas_face_crop_fwd(C.byref(gi), C.byref(gr), _rows_array(rows), len(rows), C.c_void_p(out.data_ptr()), _DT[dtype], _stream()),
          "face_crop_fwd")
    return out


def crop_faces_bwd(dfaces: torch.Tensor, rows, like: torch.Tensor):
    """d ``like`` (its dtype and layout) from the fp32 NHWC gradients of ``rows`` (all taken as rows of ``like``), one launch."""
    drec = torch.empty_like(like)
    g = _image(drec, "FaceLoss")
    check(lib().mas_face_crop_bwd(C.c_void_p(dfaces.data_ptr()), _rows_array(rows), len(rows), C.byref(g), _stream()), "face_crop_bwd")
    return drec


class FaceCrop(torch.autograd.Function):
    """The crop pass as an autograd node of its own (``FaceLoss.prepare_faces`` and the training-mode path)."""

    @staticmethod
    def forward(ctx, img, rec, rows, dtype):
        ctx.rows = rows
        ctx.save_for_backward(img, rec)
        return crop_faces(img, rec, rows, dtype)

    @staticmethod
    def backward(ctx, dfaces):
        img, rec = ctx.saved_tensors
        d = dfaces.float().contiguous(memory_format=torch.channels_last)
        grads = []
        for src, t in ((0, img), (1, rec)):
            if not ctx.needs_input_grad[src]:
                grads.append(None)
                continue
            sel = [i for i, r in enumerate(ctx.rows) if r.src == src]
            if not sel:
                grads.append(torch.zeros_like(t))
                continue
            grads.append(crop_faces_bwd(d[sel].contiguous(memory_format=torch.channels_last), [ctx.rows[i] for i in sel], t))
        return grads[0], grads[1], None, None


# --------------------------------------------------------------------------- #
# the network (evaluation mode)
# --------------------------------------------------------------------------- #
def blocks_of(mod):
    """[(layer index 1..4, Bottleneck)] in forward order"""
    return [(li, blk) for li in range(1, 5) for blk in getattr(mod, f"layer{li}")]


def bn_layers(mod):
    out = [mod.bn1]
    for _, blk in blocks_of(mod):
        out += [blk.bn1, blk.bn2, blk.bn3]
        if blk.downsample is not None:
            out.append(blk.downsample[1])
    return out


_bn_tables = {}


def fold_bn(mod):
    """The 53 evaluation-mode affine pairs from the CURRENT running statistics, one launch: -> (scale_shift [sum C, 2] fp32,
    {id(bn): channel offset}).  Only the device table of buffer ADDRESSES is cached (keyed on them); the values are read every call."""
    bns = bn_layers(mod)
    dev = bns[0].running_mean.device
    for bn in bns:
        for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise RuntimeError("FaceLoss: BatchNorm parameters and buffers must be contiguous fp32 on the loss's device")
    key = (dev.index,) + tuple((bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.eps))
                               for bn in bns)
    offs, off = {}, 0
    for bn in bns:
        offs[id(bn)] = off
        off += bn.num_features
    table = _bn_tables.get(key)
    if table is None:
        items = (FaceBnItem * len(bns))()
        for i, bn in enumerate(bns):
            items[i] = FaceBnItem(bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_features,
                                  offs[id(bn)], float(bn.eps), 0)
        host = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8)
        table = host.to(dev)
        _bn_tables.clear()                      # one live module layout at a time is the common case; stale addresses are never reused
        _bn_tables[key] = table
    ss = torch.empty((off, 2), dtype=torch.float32, device=dev)
    check(lib().mas_face_bn_fold(C.c_void_p(table.data_ptr()), len(bns), C.c_void_p(ss.data_ptr()), _stream()), "face_bn_fold")
    return ss, offs


def _ssp(ss, offs, bn):
    return C.c_void_p(ss.data_ptr() + 8 * offs[id(bn)]) if bn is not None else None


def _conv1x1(x, w, cout, residual=None, transpose=False):
    n, cin, h, wd = x.shape
    return ops.conv_fwd_raw(x, None, ops.ConvWeight(w, transpose), None, residual, n, h, wd, cin, h, wd, cout, 1, 1, 0, 0, ACT_NONE, False, x.dtype)


def _conv3x3(x, w, cout, transpose=False):
    n, cin, h, wd = x.shape
    return ops.conv_fwd_raw(x, None, ops.ConvWeight(w, transpose), None, None, n, h, wd, cin, h, wd, cout, 3, 1, 1, 1, ACT_NONE, False, x.dtype)


def _bn_relu(y, ss, offs, bn):
    n, c, h, w = y.shape
    out = torch.empty_like(y)
    check(lib().mas_bn_apply_act(_p(y), _ssp(ss, offs, bn), _p(out), 0.0, _DT[y.dtype], n * h * w, c, _stream()), "bn_apply_act")
    return out


def _subsample(x):
    n, c, h, w = x.shape
    y = torch.empty((n, c, (h + 1) // 2, (w + 1) // 2), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    check(lib().mas_face_subsample2x(_p(x), _p(y), _DT[x.dtype], n, h, w, c, _stream()), "face_subsample2x")
    return y


def _block_fwd(blk, x, ss, offs):
    """-> (out, saved (a1, a2)).  The stride sits on the first 1x1 (and the downsample 1x1): both read x[:, :, ::2, ::2]."""
    planes = blk.conv1.out_channels
    xs = _subsample(x) if blk.stride == 2 else x
    a1 = _bn_relu(_conv1x1(xs, blk.conv1.weight, planes), ss, offs, blk.bn1)
    a2 = _bn_relu(_conv3x3(a1, blk.conv2.weight, planes), ss, offs, blk.bn2)
    y3 = _conv1x1(a2, blk.conv3.weight, 4 * planes)
    if blk.downsample is not None:
        r, bnr = _conv1x1(xs, blk.downsample[0].weight, 4 * planes), blk.downsample[1]
    else:
        r, bnr = x, None
    out = torch.empty_like(y3)
    n, c, h, w = y3.shape
    check(lib().mas_face_join_fwd(_p(y3), _ssp(ss, offs, blk.bn3), _p(r), _ssp(ss, offs, bnr), _p(out), _DT[out.dtype], n * h * w, c,
                                  _stream()), "face_join_fwd")
    return out, (a1, a2)


def _block_bwd(blk, x_shape, dout, dadd, out, a1, a2, ss, offs):
    """data gradient of one Bottleneck for the rows of ``out``; x_shape: its input's (C, H, W)"""
    planes = blk.conv1.out_channels
    n, c, h, w = out.shape
    m = n * h * w
    dt = _DT[out.dtype]
    dy3 = torch.empty_like(out)
    dr = torch.empty_like(out)
    bnr = blk.downsample[1] if blk.downsample is not None else None
    check(lib().mas_face_join_bwd(_p(dout), _p(dadd), _p(out), _ssp(ss, offs, blk.bn3), _ssp(ss, offs, bnr), _p(dy3), _p(dr), dt, m, c,
                                  _stream()), "face_join_bwd")
    da2 = _conv1x1(dy3, blk.conv3.weight, planes, transpose=True)
    dy2 = torch.empty_like(da2)
    check(lib().mas_face_relu_bn_bwd(_p(da2), _p(a2), _ssp(ss, offs, blk.bn2), _p(dy2), dt, m, planes, _stream()), "face_relu_bn_bwd")
    da1 = _conv3x3(dy2, blk.conv2.weight, planes, transpose=True)
    dy1 = torch.empty_like(da1)
    check(lib().mas_face_relu_bn_bwd(_p(da1), _p(a1), _ssp(ss, offs, blk.bn1), _p(dy1), dt, m, planes, _stream()), "face_relu_bn_bwd")
    cin, hin, win = x_shape
    dres = _conv1x1(dr, blk.downsample[0].weight, cin, transpose=True) if blk.downsample is not None else dr
    dxs = _conv1x1(dy1, blk.conv1.weight, cin, residual=dres, transpose=True)        # the shortcut's gradient in the epilogue
    if blk.stride == 2:
        return ops.zero_stuff2x(dxs, hin, win)
    return dxs


def network_forward(mod, faces, ss, offs):
    """faces [R, 3, 254, 254] NHWC -> (five features, saved tensors for the backward)"""
    r = faces.shape[0]
    dt = faces.dtype
    y0 = torch.empty((r, 64, 127, 127), dtype=dt, device=faces.device, memory_format=torch.channels_last)
    w0 = mod.conv1.weight.detach().float().contiguous()
    check(lib().mas_face_stem_fwd(_p(faces), _p(w0), _p(y0), _DT[dt], r, _stream()), "face_stem_fwd")
    z = torch.empty((r, 64, 63, 63), dtype=dt, device=faces.device, memory_format=torch.channels_last)
    idx = torch.empty(r * 63 * 63 * 64, dtype=torch.uint8, device=faces.device)
    check(lib().mas_face_pool_fwd(_p(y0), _ssp(ss, offs, mod.bn1), _p(z), _p(idx), _DT[dt], r, 127, 127, 64, _stream()), "face_pool_fwd")
    feats, saved, h = [y0], [], z
    for li, blk in blocks_of(mod):
        shape_in = tuple(h.shape[1:])
        h, (a1, a2) = _block_fwd(blk, h, ss, offs)
        saved.append((shape_in, a1, a2, h))
        if blk is getattr(mod, f"layer{li}")[-1]:
            feats.append(h)
    return feats, (w0, idx, saved)


def _feats_table(feats, half):
    f = FaceFeats()
    for i, t in enumerate(feats):
        f.p[i] = t.data_ptr()
        f.chw[i] = t[0].numel()
        f.alpha[i] = ALPHAS[i]
    f.half, f.dtype = half, _DT[feats[0].dtype]
    return f


def l1_forward(feats, half):
    """[6] fp32: alpha_i * mean over (C, H, W) of the pair-summed |p0 - p1|, i = 0..4, and their sum"""
    f = _feats_table(feats, half)
    nws = lib().mas_face_l1_workspace(C.byref(f))
    if nws < 0:
        check(nws, "face_l1_workspace")
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=feats[0].device)
    out = torch.empty(6, dtype=torch.float32, device=feats[0].device)
    check(lib().mas_face_l1_fwd(C.byref(f), _p(ws), _p(out), _stream()), "face_l1_fwd")
    return out


def _network_backward(mod, ss, offs, feats, saved, idx, w0, seeds, row0, nb):
    """the data gradient of the network for rows [row0, row0 + nb) of the saved maps, from the five seeds of those rows: the Bottlenecks
    in reverse, pool, stem -> d faces [nb, 254, 254, 3] fp32"""
    blocks = blocks_of(mod)
    d = None
    for k in range(len(blocks) - 1, -1, -1):
        li, blk = blocks[k]
        shape_in, a1, a2, out = saved[k]
        last = blk is getattr(mod, f"layer{li}")[-1]
        d = _block_bwd(blk, shape_in, d, seeds[li] if last else None, out[row0:row0 + nb], a1[row0:row0 + nb], a2[row0:row0 + nb], ss, offs)
    y0 = feats[0][row0:row0 + nb]
    dy0 = torch.empty_like(y0)
    idx = idx[row0 * 63 * 63 * 64:]
    dt = _DT[y0.dtype]
    check(lib().mas_face_pool_bwd(_p(y0), _ssp(ss, offs, mod.bn1), _p(d), _p(idx), _p(seeds[0]), _p(dy0), dt, nb, 127, 127, 64, _stream()),
          "face_pool_bwd")
    dfaces = torch.empty((nb, FACE, FACE, 3), dtype=torch.float32, device=y0.device)
    check(lib().mas_face_stem_dgrad(_p(dy0), _p(w0), _p(dfaces), dt, nb, _stream()), "face_stem_dgrad")
    return dfaces


class _FaceLoss(torch.autograd.Function):
    """img, rec -> [d_0 .. d_4, loss]: crop, stem, bn1 + ReLU + pool, 16 Bottlenecks, L1 -- ~105 launches.  Backward: the seeds of
    the five L1 terms for the rec rows, the Bottlenecks in reverse (join, conv3^T, ReLU-BN, conv2^T, ReLU-BN, [downsample^T],
    conv1^T with the shortcut gradient in its epilogue, [zero-stuff]), pool, stem, crop adjoint."""

    @staticmethod
    def forward(ctx, img, rec, mod, rows, n_faces, dtype):
        faces = crop_faces(img, rec, rows, dtype)
        ss, offs = fold_bn(mod)
        feats, (w0, idx, saved) = network_forward(mod, faces, ss, offs)
        half = len(rows) // 2
        out = l1_forward(feats, half)
        ctx.mod, ctx.rows, ctx.n, ctx.half = mod, rows, n_faces, half
        ctx.rec_like = (rec.shape, rec.dtype)
        ctx.idx, ctx.ss, ctx.offs, ctx.w0, ctx.feats, ctx.saved = idx, ss, offs, w0, feats, saved
        ctx.save_for_backward(rec)
        return out

    @staticmethod
    def backward(ctx, dl6):
        (rec,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        row0 = ctx.n                               # the rec rows: [n, len(rows)) -- the tail
        nb = len(ctx.rows) - row0
        if nb <= 0:                                # n >= 6: every surviving row is a gt row
            return None, torch.zeros_like(rec), None, None, None, None
        mod, ss, offs, feats = ctx.mod, ctx.ss, ctx.offs, ctx.feats
        dl6 = dl6.float().contiguous()
        seeds = [torch.empty((nb,) + tuple(f.shape[1:]), dtype=f.dtype, device=f.device, memory_format=torch.channels_last) for f in feats]
        f = _feats_table(feats, ctx.half)
        sp = (C.c_void_p * 5)(*[s.data_ptr() for s in seeds])
        check(lib().mas_face_l1_bwd(C.byref(f), row0, nb, _p(dl6), sp, _stream()), "face_l1_bwd")
        dfaces = _network_backward(mod, ss, offs, feats, ctx.saved, ctx.idx, ctx.w0, seeds, row0, nb)
        drec = crop_faces_bwd(dfaces, ctx.rows[row0:], rec)
        return None, drec, None, None, None, None


class _FaceLossStatic(torch.autograd.Function):
    """``_FaceLoss`` at fixed capacity: the rows come from a ``FaceTable``, the network always runs on six rows and its backward on
    the slice [3:6] (every rec row sits there), so the launches, their arguments and every shape are the same whatever the table holds
    -- nothing is read on the host, and a captured graph of this node follows the table of each replay.  Empty slots are zero crops;
    the L1 sums add exactly 0 for them and their seeds are zeros, so their rows carry zeros through the backward and the crop adjoint
    skips them.  A table without faces gives a loss of exactly 0 and d rec of exact zeros."""

    @staticmethod
    def forward(ctx, img, rec, mod, table, dtype):
        tp = C.c_void_p(table.data_ptr())
        faces = torch.empty((SLOTS, 3, FACE, FACE), dtype=dtype, device=img.device, memory_format=torch.channels_last)
        gi, gr = _image(img, "FaceLoss"), _image(rec, "FaceLoss")
        check(lib().mas_face_crop_fwd_dev(C.byref(gi), C.byref(gr), tp, C.c_void_p(faces.data_ptr()), _DT[dtype], _stream()), "face_crop_fwd_dev")
        ss, offs = fold_bn(mod)
        feats, (w0, idx, saved) = network_forward(mod, faces, ss, offs)
        f = _feats_table(feats, PAIRS)
        nws = lib().mas_face_l1_workspace(C.byref(f))
        if nws < 0:
            check(nws, "face_l1_workspace")
        ws = torch.empty(max(nws, 1), dtype=torch.float32, device=img.device)
        out = torch.empty(6, dtype=torch.float32, device=img.device)
        check(lib().mas_face_l1_fwd_dev(C.byref(f), tp, _p(ws), _p(out), _stream()), "face_l1_fwd_dev")
        ctx.mod, ctx.table = mod, table
        ctx.idx, ctx.ss, ctx.offs, ctx.w0, ctx.feats, ctx.saved = idx, ss, offs, w0, feats, saved
        ctx.save_for_backward(rec)
        return out

    @staticmethod
    def backward(ctx, dl6):
        (rec,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        mod, ss, offs, feats = ctx.mod, ctx.ss, ctx.offs, ctx.feats
        tp = C.c_void_p(ctx.table.data_ptr())
        row0, nb = PAIRS, PAIRS
        dl6 = dl6.float().contiguous()
        seeds = [torch.empty((nb,) + tuple(f.shape[1:]), dtype=f.dtype, device=f.device, memory_format=torch.channels_last) for f in feats]
        f = _feats_table(feats, PAIRS)
        sp = (C.c_void_p * 5)(*[s.data_ptr() for s in seeds])
        check(lib().mas_face_l1_bwd_dev(C.byref(f), tp, _p(dl6), sp, _stream()), "face_l1_bwd_dev")
        dfaces = _network_backward(mod, ss, offs, feats, ctx.saved, ctx.idx, ctx.w0, seeds, row0, nb)
        drec = torch.empty_like(rec)
        g = _image(drec, "FaceLoss")
        check(lib().mas_face_crop_bwd_dev(C.c_void_p(dfaces.data_ptr()), tp, C.byref(g), _stream()), "face_crop_bwd_dev")
        return None, drec, None, None, None


def face_loss_static(mod, img, rec, table, dtype=None):
    """The evaluation-mode FaceLoss on a ``FaceTable``: -> [6] fp32 as ``face_loss``, ALWAYS (the node runs whatever the table holds;
    whether a batch has faces at all is the caller's to decide from ``table.write``'s return value)."""
    _require_cuda(img, "FaceLoss")
    _require_cuda(rec, "FaceLoss")
    if table.device != img.device:
        raise RuntimeError(f"FaceLoss: the face table is on {table.device}, the images on {img.device}")
    if table.n_images > min(img.shape[0], rec.shape[0]):
        raise ValueError(f"FaceLoss: the face table was written for {table.n_images} images, the batch has {min(img.shape[0], rec.shape[0])}")
    return _FaceLossStatic.apply(img, rec, mod, table, dtype or ops.compute_dtype())


def face_loss(mod, img, rec, bbox, dtype=None):
    """The evaluation-mode FaceLoss on the HIP path: -> [6] fp32 (five weighted feature distances and the loss), or None without
    faces (nothing launched)."""
    _require_cuda(img, "FaceLoss")
    _require_cuda(rec, "FaceLoss")
    n, rows = plan(bbox, min(img.shape[0], rec.shape[0]))
    if n == 0:
        return None
    return _FaceLoss.apply(img, rec, mod, rows, n, dtype or ops.compute_dtype())
