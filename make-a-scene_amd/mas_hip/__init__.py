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

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MAS_HIP_LIB") or os.path.join(_HERE, "libmas_hip.so")   # env override: A/B kernel experiments

F32, BF16 = 0, 1
ACT_NONE, ACT_AFFINE, ACT_AFFINE_SILU = 0, 1, 2
ABI_VERSION = 10
WLAYOUT_K64, WLAYOUT_K32, WLAYOUT_UP2 = 0, 1, 2
ATTN_DECODE_MAX_SPLITS = 32   # MAS_ATTN_DECODE_MAX_SPLITS
CE_NONE, CE_MEAN, CE_SUM = 0, 1, 2   # MAS_CE_*
SEG_NCHW, SEG_NHWC, SEG_U8 = 0, 1, 2   # MAS_SEG_*: layout codes; the uint8 target dtype beside F32 / BF16
SEG_LABELS_TILE, SEG_MAX_PLANES = 256, 8   # MAS_SEG_LABELS_TILE: pixels of one tile of the label-plane kernels; MAS_SEG_MAX_PLANES


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


_p, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_SIGNATURES = {
    "mas_abi_version": (C.c_int, []),
    "mas_last_error": (C.c_char_p, []),
    "mas_last_kernel": (C.c_char_p, []),
    "mas_packed_weight_elems": (_sz, [_i, _i, _i]),
    "mas_packed_weight_elems_up2": (_sz, [_i, _i]),
    "mas_pack_conv_weight": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "mas_conv_weight_layout": (_i, [C.POINTER(ConvDesc)]),
    "mas_pack_conv_weight_layout": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "mas_pack_batch_blocks": (_i, [_i, _i, _i, _i, _i, _i]),
    "mas_adam_blocks": (_i, [C.c_longlong]),
    "mas_adam_multi": (_i, [_p, _i, _i, _f, _f, _f, _f, _f, C.c_double, C.c_double, _p]),
    "mas_grad_sqnorm_multi": (_i, [_p, _i, _i, _p, _p]),
    "mas_grad_clip_coef": (_i, [_p, _i, _p, _i, _f, _p, _p]),
    "mas_adam_multi_ex": (_i, [_p, _i, _i, _f, _f, _f, _f, _f, C.c_double, C.c_double, _p, _i, _p]),
    "mas_grad_scale_multi": (_i, [_p, _i, _i, _p, _p]),
    "mas_pack_conv_weight_batch": (_i, [_p, _i, _i, _p]),
    "mas_pack_tile_blocks": (_i, [_i, _i, _i]),
    "mas_pack_conv_weight_tiles": (_i, [_p, _i, _i, _i, _p]),
    "mas_gn_stats_workspace": (_sz, [_i, _i]),
    "mas_gn_stats": (_i, [_p, _i, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p, _sz, _p]),
    "mas_gn_bwd_workspace": (_sz, [_i, _i]),
    "mas_gn_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "mas_gn_bwd_3pass": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "mas_gn_act": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "mas_gn_small_supported": (_i, [_i, _i, _i, _i]),
    "mas_gn_stats_act": (_i, [_p, _p, _i, _i, _i, _i, _i, _f, _p, _p, _i, _p, _p, _p]),
    "mas_conv_fwd": (_i, [C.POINTER(ConvDesc), _p, _p, _p, _p, _p, _p, _p]),
    "mas_conv_stat_rows": (_i, [C.POINTER(ConvDesc)]),
    "mas_conv_fwd_stats": (_i, [C.POINTER(ConvDesc), _p, _p, _p, _p, _p, _p, _p, _p]),
    "mas_gn_stats_from_partials": (_i, [_p, _i, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p]),
    "mas_conv_wgrad": (_i, [C.POINTER(ConvDesc), _p, _p, _p, _p, _p, _p]),
    "mas_wgrad_commit": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "mas_conv_s2_dgrad_supported": (_i, [C.POINTER(ConvDesc)]),
    "mas_conv_s2_dgrad": (_i, [C.POINTER(ConvDesc), _p, _p, _p, _p]),
    "mas_conv_up2_supported": (_i, [C.POINTER(ConvDesc)]),
    "mas_conv_up2_dgrad_supported": (_i, [C.POINTER(ConvDesc)]),
    "mas_conv_up2_dgrad": (_i, [C.POINTER(ConvDesc), _p, _p, _p, _p]),
    "mas_conv_up2_wgrad_splits": (_i, [C.POINTER(ConvDesc)]),
    "mas_conv_up2_wgrad_partial": (_i, [C.POINTER(ConvDesc), _p, _p, _p, _p, _p]),
    "mas_wgrad_reduce_up2": (_i, [_p, _p, _i, _p, _p, _i, _i, _p]),
    "mas_conv_wgrad_splits": (_i, [C.POINTER(ConvDesc)]),
    "mas_conv_wgrad_partial": (_i, [C.POINTER(ConvDesc), _p, _p, _p, _p, _p, _p]),
    "mas_wgrad_reduce": (_i, [_p, _p, _i, _p, _p, _i, _i, _i, _p]),
    "mas_vq_workspace": (_sz, [_i, _i]),
    "mas_vq_argmin_fwd": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _sz, _p]),
    "mas_vq_bwd": (_i, [_p, _p, _p, _p, _p, _f, _i, _i, _i, _p, _p, _p]),
    "mas_attn_causal_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, C.c_longlong, C.c_longlong, C.c_longlong, _f, _p]),
    "mas_attn_causal_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p]),
    "mas_attn_causal_fwd_drop": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, C.c_longlong, C.c_longlong, C.c_longlong, _f, _f, _p,
                                      _p]),
    "mas_attn_causal_bwd_drop": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _p, _p]),
    "mas_attn_dropout_mask": (_i, [_p, _i, _i, _i, _f, _p, _p]),
    "mas_dropout_apply": (_i, [_p, _p, C.c_longlong, _i, _f, _p, _p]),
    "mas_spatial_attn_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "mas_spatial_attn_bwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "mas_spatial_attn_flash_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "mas_spatial_attn_flash_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "mas_attn_decode": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _f, _p]),
    "mas_attn_decode_dev": (_i, [_p, _p, _p, C.c_longlong, _p, _p, _i, C.c_longlong, _i, _p, C.c_longlong, _i, _i, _i, _i, _p, _f, _p]),
    "mas_decode_embed": (_i, [_p, C.c_longlong, _p, _p, _i, _p, _p, _i, _p, _i, _i, _i, _p]),
    "mas_sample_tokens": (_i, [_p, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, C.c_longlong, _p, C.c_longlong, _p,
                               C.c_longlong, _p]),
    "mas_sample_tokens_topp": (_i, [_p, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, C.c_longlong, _p, C.c_longlong,
                                    _p, C.c_longlong, _p]),
    "mas_sample_tokens_prompt": (_i, [_p, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, C.c_longlong, _p, C.c_longlong,
                                      _p, C.c_longlong, _p, C.c_longlong, _p]),
    "mas_decode_advance": (_i, [_p, _i, _p]),
    "mas_attn_decode_split": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_longlong, C.c_longlong, C.c_longlong,
                                   C.c_longlong, _f, _i, _p, _sz, _p]),
    "mas_attn_decode_split_dev": (_i, [_p, _p, _p, C.c_longlong, _p, _p, _i, C.c_longlong, _i, _p, C.c_longlong, _i, _i, _i, _i, _p, _f,
                                       _i, _p, _sz, _p]),
    "mas_upsample2x": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "mas_sumpool2x": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "mas_zero_stuff2x": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "mas_space_to_depth2x": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "mas_gelu_tanh_fwd": (_i, [_p, _p, _i, C.c_longlong, _p]),
    "mas_gelu_tanh_bwd": (_i, [_p, _p, _p, _i, C.c_longlong, _p]),
    "mas_gelu_tanh_bwd_colsum_workspace": (_sz, [_i, _i]),
    "mas_gelu_tanh_bwd_colsum": (_i, [_p, _p, _p, _p, _i, C.c_longlong, _i, _p, _sz, _p]),
    "mas_token_ce_fwd": (_i, [_p, _i, C.c_longlong, _i, C.c_longlong, C.c_longlong, C.c_longlong, _p, C.c_longlong, _f, _p, _p, _p]),
    "mas_token_ce_reduce": (_i, [_p, _p, C.c_longlong, C.c_longlong, _i, _p, _p]),
    "mas_token_ce_bwd": (_i, [_p, _i, C.c_longlong, _i, C.c_longlong, C.c_longlong, C.c_longlong, _p, C.c_longlong, _f, _p, _p, _p, _i, _p,
                              _p]),
    "mas_seg_loss_blocks": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "mas_seg_loss_fwd": (_i, [_p, _i, _i, _p, _i, _i, _p, _i, _i, _i, _i, _i, _p, _i, _p]),
    "mas_seg_loss_reduce": (_i, [_p, _i, C.c_longlong, _i, _p, _p]),
    "mas_seg_loss_bwd": (_i, [_p, _i, _i, _p, _i, _i, _p, _i, _i, _i, _i, _i, _p, _p, _p]),
    "mas_seg_expand": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _i, _i, _i, _p]),
    "mas_seg_loss_labels_blocks": (_i, [_p, _i, _i, _i, _i, _i, _i, _i]),
    "mas_seg_loss_labels_fwd": (_i, [_p, _i, _i, _p, _p, _i, _i, _p, _i, _i, _i, _i, _p, _i, _p]),
    "mas_seg_loss_labels_bwd": (_i, [_p, _i, _i, _p, _p, _i, _i, _p, _i, _i, _i, _i, _p, _p, _p]),
    "mas_seg_classify": (_i, [_p, _i, _i, _p, _i, _i, _p, _i, _i, _i, _p, _p]),
    "mas_seg_agreement": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "mas_layernorm_fwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _p]),
    "mas_layernorm_bwd_workspace": (_sz, [_i, _i]),
    "mas_layernorm_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "mas_layernorm_bwd_add": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "mas_bn_workspace": (_sz, [_i, _i]),
    "mas_bn_partial_sums": (_i, [_p, _p, _p, _i, _i, _p, _p, _sz, _p]),
    "mas_bn_finalize": (_i, [_p, _p, _p, _f, _f, _p, _p, _p, _p, _i, _p]),
    "mas_bn_apply": (_i, [_p, _p, _p, _i, _i, _p]),
    "mas_bn_bwd_apply": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _p]),
    "mas_bn_partial_sums_act": (_i, [_p, _p, _p, _p, _f, _i, _i, _i, _p, _p, _sz, _p]),
    "mas_bn_apply_act": (_i, [_p, _p, _p, _f, _i, _i, _i, _p]),
    "mas_bn_bwd_apply_act": (_i, [_p, _p, _p, _p, _p, _f, _p, _p, _i, _i, _i, _p]),
    "mas_layernorm_bwd_colsum": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "mas_layernorm_pair_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _p]),
    "mas_colsum_workspace": (_sz, [_i, _i]),
    "mas_colsum": (_i, [_p, _i, _i, _i, _p, _p, _sz, _p]),
    "mas_face_crop_fwd": (_i, [C.POINTER(FaceImage), C.POINTER(FaceImage), C.POINTER(FaceRow), _i, _p, _i, _p]),
    "mas_face_crop_bwd": (_i, [_p, C.POINTER(FaceRow), _i, C.POINTER(FaceImage), _p]),
    "mas_face_stem_fwd": (_i, [_p, _p, _p, _i, _i, _p]),
    "mas_face_stem_dgrad": (_i, [_p, _p, _p, _i, _i, _p]),
    "mas_face_bn_fold": (_i, [_p, _i, _p, _p]),
    "mas_face_pool_fwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "mas_face_pool_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "mas_face_join_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "mas_face_join_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "mas_face_relu_bn_bwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "mas_face_subsample2x": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "mas_face_l1_workspace": (_i, [C.POINTER(FaceFeats)]),
    "mas_face_l1_fwd": (_i, [C.POINTER(FaceFeats), _p, _p, _p]),
    "mas_face_l1_bwd": (_i, [C.POINTER(FaceFeats), _i, _i, _p, C.POINTER(_p), _p]),
    "mas_obj_canvas_fwd": (_i, [C.POINTER(FaceImage), C.POINTER(FaceImage), C.POINTER(ObjPlan), _p, _p, _p, _i, _p]),
    "mas_obj_canvas_bwd": (_i, [_p, _i, C.POINTER(ObjPlan), _p, C.POINTER(FaceImage), _p]),
    "mas_obj_relu_fwd": (_i, [_p, C.POINTER(ObjPlan), _i, _i, _i, _i, _p]),
    "mas_obj_relu_bwd": (_i, [_p, _p, _p, C.c_longlong, _i, _p]),
    "mas_obj_pool_fwd": (_i, [_p, _p, C.POINTER(ObjPlan), _i, _i, _i, _i, _p]),
    "mas_obj_pool_bwd": (_i, [_p, _p, _p, _p, C.POINTER(ObjPlan), _i, _i, _i, _i, _p]),
    "mas_obj_head_fwd": (_i, [_p, _p, C.POINTER(ObjPlan), _i, _i, _i, _i, _p, _p]),
    "mas_obj_finalize": (_i, [_p, C.POINTER(ObjPlan), _p, _p]),
    "mas_obj_head_bwd": (_i, [_p, _p, C.POINTER(ObjPlan), _i, _i, _i, _p, _p, _p]),
}
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
                    fn = getattr(L, name, None)
                    if fn is None:
                        continue          # optional symbol of a later ABI revision; callers check
                    fn.restype, fn.argtypes = res, args
                if L.mas_abi_version() != ABI_VERSION:
                    raise RuntimeError(f"libmas_hip.so ABI {L.mas_abi_version()} != binding {ABI_VERSION}")
                _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().mas_last_error()
        raise RuntimeError(f"libmas_hip {what} failed (code {rc}): {msg.decode() if msg else ''}")
