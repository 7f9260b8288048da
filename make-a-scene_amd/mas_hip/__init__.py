"""ctypes binding of libmas_hip.so (the C ABI declared in include/mas_hip.h).

The product path has NO fallback: if the shared library is missing or a kernel call
fails, a RuntimeError is raised.  PyTorch is used only for device memory, streams and
torch.distributed.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

# HIP gives a process four hardware queues by default and hands them to streams in creation order; RCCL's own streams take the three beside
# the default stream's, after which ops' side stream (weight gradients beside the GroupNorm backward) lands on the default stream's queue and
# its kernels serialise behind barrier packets: +1.7 ms per step instead of -1.2 (profiles/r06_wgrad_stream.txt).  The runtime reads this at
# its first HIP call -- after `import torch` is early enough, after torch.cuda.is_available() is not (ops probes the streams and refuses the
# side stream when they do not overlap).  A value the user exported wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import torch  # noqa: F401,E402  -- must come first: PyTorch-ROCm bundles its own libamdhip64; loading ours before it leaves torch without GPUs

from . import _header  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MAS_HIP_LIB") or os.path.join(_HERE, "libmas_hip.so")   # env override: A/B kernel experiments


class ConvDesc(C.Structure):
    """Mirror of ``MasConvDesc`` (include/mas_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "N", "H", "W", "Cin", "Ho", "Wo", "Cout", "ks", "stride", "pad_top", "pad_left",
        "in_dtype", "out_dtype", "act", "upsample", "w_layout", "wgrad_cus")]


class PackItem(C.Structure):
    """Mirror of ``MasPackItem`` (include/mas_hip.h): one entry of the batched weight-pack table."""
    _fields_ = [("w_oihw", C.c_void_p), ("packed", C.c_void_p)] + [(n, C.c_int32) for n in (
        "Cout", "Cin", "ks", "transpose", "dtype", "layout", "first_block", "n_blocks")]


class PackTileItem(C.Structure):
    """Mirror of ``MasPackTileItem`` (include/mas_hip.h): one parameter and up to four bf16 images of it."""
    _fields_ = [("w_oihw", C.c_void_p), ("img", C.c_void_p * 4), ("transpose", C.c_int32 * 4), ("layout", C.c_int32 * 4)] + \
               [(n, C.c_int32) for n in ("n_img", "Cout", "Cin", "ks", "first_block", "pad_")]


class AdamItem(C.Structure):
    """Mirror of ``MasAdamItem`` (include/mas_hip.h): one fp32 parameter with its gradient and the two Adam moments."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_longlong), ("first_block", C.c_int32),
                ("pad_", C.c_int32)]


class FaceRow(C.Structure):
    """Mirror of ``MasFaceRow`` (include/mas_hip.h): one face row of FaceLoss, its geometry computed on the host."""
    _fields_ = [(n, C.c_int32) for n in ("src", "b", "top", "left", "h", "w", "rh", "rw", "ct", "cl")]


class FaceImage(C.Structure):
    """Mirror of ``MasFaceImage`` (include/mas_hip.h): a [N,3,H,W] image of any element strides."""
    _fields_ = [("data", C.c_void_p)] + [(n, C.c_int32) for n in ("dtype", "N", "C", "H", "W", "pad_")] + \
               [(n, C.c_int64) for n in ("sn", "sc", "sh", "sw")]


class FaceBnItem(C.Structure):
    """Mirror of ``MasFaceBnItem`` (include/mas_hip.h): one BatchNorm2d layer of the evaluation-mode fold."""
    _fields_ = [(n, C.c_void_p) for n in ("weight", "bias", "mean", "var")] + [("C", C.c_int32), ("off", C.c_int32), ("eps", C.c_float),
                                                                                ("pad_", C.c_int32)]


class FaceFeats(C.Structure):
    """Mirror of ``MasFaceFeats`` (include/mas_hip.h): the five feature maps of the face L1 distance."""
    _fields_ = [("p", C.c_void_p * 5), ("chw", C.c_int32 * 5), ("half", C.c_int32), ("dtype", C.c_int32), ("alpha", C.c_float * 5)]


class ObjCell(C.Structure):
    """Mirror of ``MasObjCell`` (include/mas_hip.h): one object crop of the atlas: canvas, origin, size, image, box corner."""
    _fields_ = [(n, C.c_int32) for n in ("n", "oy", "ox", "h", "w", "b", "top", "left")]


class ObjPlan(C.Structure):
    """Mirror of ``MasObjPlan`` (include/mas_hip.h): the atlas's device tables and canvas geometry."""
    _fields_ = [("cells", C.c_void_p), ("img_cell0", C.c_void_p), ("tiles", C.c_void_p), ("blk0", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("n_cells", "n_images", "n_canvas", "H", "W", "pad_")]


# Every prototype and every integer constant of include/mas_hip.h, read from the header itself (_header.py says what it can read and
# raises on the rest).  _SIGNATURES: {name: (restype, [argtypes])} in header order; MAS_X is this module's X (F32, BF16, ACT_*,
# WLAYOUT_*, CE_*, SEG_*, ABI_VERSION, ATTN_DECODE_MAX_SPLITS, FACE_SIZE, OBJ_ALIGN, ...).  The structs above are the ones the host
# fills in; the five it hands over by reference are named here, and a pointer to any other struct is a device table: c_void_p.
_SIGNATURES, constants = _header.load({"MasConvDesc": ConvDesc, "MasFaceImage": FaceImage, "MasFaceRow": FaceRow, "MasFaceFeats": FaceFeats,
                                       "MasObjPlan": ObjPlan})
globals().update((name[len("MAS_"):], value) for name, value in constants.items())
EXPORTS = tuple(_SIGNATURES)

_lib = None
_lock = threading.Lock()


def lib():
    """Loads libmas_hip.so once; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                        "(hipcc --offload-arch=gfx950); there is no PyTorch/CPU fallback for this path")
                L = C.CDLL(LIB_PATH)
                for name, (res, args) in _SIGNATURES.items():
                    try:
                        fn = getattr(L, name)
                    except AttributeError:
                        raise RuntimeError(f"{LIB_PATH} does not export {name}, which include/mas_hip.h declares: rebuild it") from None
                    fn.restype, fn.argtypes = res, args
                if L.mas_abi_version() != constants["MAS_ABI_VERSION"]:
                    raise RuntimeError(f"libmas_hip.so ABI {L.mas_abi_version()} != binding {constants['MAS_ABI_VERSION']}")
                _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().mas_last_error()
        raise RuntimeError(f"libmas_hip {what} failed (code {rc}): {msg.decode() if msg else ''}")


# What every caller of the library needs beside lib() and check(): dtype codes, pointers, the current stream.
_DT = {torch.float32: constants["MAS_F32"], torch.bfloat16: constants["MAS_BF16"]}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _require_cuda(t, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the MI355X path needs a GPU tensor (no CPU fallback); got device {t.device}")


def _image(t, who: str) -> FaceImage:
    """``MasFaceImage`` of a [N, 3, H, W] tensor of any strides; ``who``: the loss the error messages name"""
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{who}: images must be [N, 3, H, W], got {tuple(t.shape)}")
    if t.dtype not in _DT:
        raise TypeError(f"{who}: images must be float32 or bfloat16, got {t.dtype}")
    n, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    return FaceImage(t.data_ptr(), _DT[t.dtype], n, c, h, w, 0, sn, sc, sh, sw)
