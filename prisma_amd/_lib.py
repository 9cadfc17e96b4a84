"""ctypes binding of libprisma_bands.so (include/prisma_bands.h).

The library is the product; there is no Python/torch/numpy fallback.  If the shared object is
missing or was built without its kernels this module raises at import of the symbols, loudly.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRISMA_BANDS_LIB") or os.path.join(_HERE, "libprisma_bands.so")      # the override is for A/B timing of two builds


class pb_tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("dtype", C.c_int32), ("ndim", C.c_int32),
                ("shape", C.c_int64 * 6), ("data", C.c_void_p)]


class pb_depth_cfg(C.Structure):
    _fields_ = [("embed_dim", C.c_int32), ("depth", C.c_int32), ("heads", C.c_int32), ("features", C.c_int32),
                ("out_channels", C.c_int32 * 4), ("pos_grid", C.c_int32), ("max_batch", C.c_int32), ("metric", C.c_int32),
                ("precision", C.c_int32)]


class pb_flow_cfg(C.Structure):
    _fields_ = [("precision", C.c_int32)]


PREC_F16, PREC_SPLIT = 0, 1
ABI_VERSION = 3          # include/prisma_bands.h PB_ABI_VERSION this binding was written against


def default_precision() -> int:
    """pb_precision the engine classes use when none is given: PRISMA_PRECISION=0 selects the single-pass fp16 mode
    (faster; max-norm error up to 1.6e-3 against the fp32 reference), anything else / unset the split-fp16 mode that
    meets the 1e-3 bound the parity tests assert."""
    return PREC_F16 if os.environ.get("PRISMA_PRECISION", "1") == "0" else PREC_SPLIT


class pb_mask_cfg(C.Structure):
    _fields_ = [("blocks", C.c_int32 * 4), ("scale_long", C.c_int32), ("scale_short", C.c_int32), ("num_classes", C.c_int32),
                ("feat_channels", C.c_int32), ("stacked_convs", C.c_int32), ("num_grids", C.c_int32 * 5),
                ("strides", C.c_int32 * 5), ("mask_feat_channels", C.c_int32), ("mask_out_channels", C.c_int32),
                ("nms_pre", C.c_int32), ("max_per_img", C.c_int32), ("score_thr", C.c_float), ("mask_thr", C.c_float),
                ("filter_thr", C.c_float), ("sigma", C.c_float), ("max_batch", C.c_int32), ("precision", C.c_int32)]


class pb_kernel_stat(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_double), ("flops", C.c_double), ("exec_flops", C.c_double), ("bytes", C.c_double),
                ("launches", C.c_int32)]


class pb_yuv_fmt(C.Structure):
    _fields_ = [("chroma", C.c_int32), ("depth", C.c_int32), ("full_range", C.c_int32), ("matrix", C.c_int32)]


class pb_jpeg_cfg(C.Structure):
    _fields_ = [("chroma", C.c_int32), ("quality", C.c_int32)]


YUV_MATRICES = ("bt601", "bt709")       # pb_yuv_fmt.matrix: PB_YUV_BT601, PB_YUV_BT709


class YuvFormat(collections.namedtuple("YuvFormat", "chroma depth full_range matrix")):
    """A planar YUV layout (include/prisma_bands.h pb_yuv_fmt): chroma 400 / 420 / 422 / 444, depth 8 .. 16, full_range, matrix "bt601" / "bt709"."""
    __slots__ = ()

    def c(self) -> pb_yuv_fmt:
        m = YUV_MATRICES.index(self.matrix) if self.matrix in YUV_MATRICES else -1       # a name the library does not know: it refuses -1
        return pb_yuv_fmt(int(self.chroma), int(self.depth), int(bool(self.full_range)), m)


I420 = YuvFormat(420, 8, False, "bt601")       # what "frames_i420" means


# every symbol include/prisma_bands.h declares: (restype, argtypes)
_P = C.c_void_p
_F = C.POINTER(C.c_float)
_U8 = C.POINTER(C.c_uint8)
SYMBOLS = {
    "pb_last_error": (C.c_char_p, []),
    "pb_version": (C.c_int, []),
    "pb_abi_version": (C.c_int, []),
    "pb_struct_size": (C.c_int, [C.c_int]),
    "pb_device_count": (C.c_int, []),
    "pb_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.POINTER(pb_tensor), C.c_int, _P, C.c_size_t]),
    "pb_destroy": (None, [_P]),
    "pb_depth_infer_batch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int]),
    "pb_depth_infer_batch_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int]),
    "pb_sync": (C.c_int, [_P]),
    "pb_depth_submit_batch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int]),
    "pb_flow_submit_sequence": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _P, _P, _P]),
    "pb_wait": (C.c_int, [_P]),
    "pb_flow_submit_sequence_masks": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float,
                                                _P, _P, _P, _P]),
    "pb_host_alloc": (C.c_int, [_P, C.POINTER(_P), C.c_size_t]),
    "pb_host_free": (C.c_int, [_P, _P]),
    "pb_comm_unique_id": (C.c_int, [_P]),
    "pb_comm_init": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "pb_gather_scalars": (C.c_int, [_P, _P, C.c_int, _P]),
    "pb_depth_encode_still": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _F, _F]),
    "pb_depth_point_cloud": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_float] * 4 + [_P]),
    "pb_depth_point_cloud_dev": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_float] * 4 + [_P]),
    "pb_rgbd_boxes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_rgbd_depth": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "pb_rgbd_depth_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "pb_i420_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "pb_i420_to_rgb": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_i420_to_rgb_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_rgb_to_i420": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_rgb_to_i420_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_yuv_bytes": (C.c_int64, [C.POINTER(pb_yuv_fmt), C.c_int, C.c_int]),
    "pb_yuv_coeffs": (C.c_int, [C.POINTER(pb_yuv_fmt), C.POINTER(C.c_int32)]),
    "pb_yuv_to_rgb": (C.c_int, [_P, C.POINTER(pb_yuv_fmt), _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_yuv_to_rgb_dev": (C.c_int, [_P, C.POINTER(pb_yuv_fmt), _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_set_frame_format": (C.c_int, [_P, C.POINTER(pb_yuv_fmt)]),
    "pb_yuv_fwd_coeffs": (C.c_int, [C.POINTER(pb_yuv_fmt), C.POINTER(C.c_int32)]),
    "pb_rgb_to_yuv": (C.c_int, [_P, C.POINTER(pb_yuv_fmt), _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_rgb_to_yuv_dev": (C.c_int, [_P, C.POINTER(pb_yuv_fmt), _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_set_out_format": (C.c_int, [_P, C.POINTER(pb_yuv_fmt)]),
    "pb_jpeg_bound": (C.c_int64, [C.POINTER(pb_jpeg_cfg), C.c_int, C.c_int]),
    "pb_jpeg_encode": (C.c_int, [_P, C.POINTER(pb_jpeg_cfg), _P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "pb_jpeg_encode_dev": (C.c_int, [_P, C.POINTER(pb_jpeg_cfg), _P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    "pb_rgb_resize": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "pb_rgb_resize_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int]),
    "pb_depth_net_size": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_depth_get_stage": (C.c_int64, [_P, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "pb_mask_infer_batch": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, C.c_int, _P]),
    "pb_mask_infer_batch_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, C.c_int, _P]),
    "pb_mask_get_instances": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "pb_mask_net_size": (C.c_int, [C.POINTER(pb_mask_cfg), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_mask_get_stage": (C.c_int64, [_P, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "pb_flow_set_inference_size": (C.c_int, [_P, C.c_int, C.c_int]),
    "pb_flow_set_matching": (C.c_int, [_P, C.c_int, C.c_int]),
    "pb_flow_num_scales": (C.c_int, [_P]),
    "pb_flow_set_alternate_corr": (C.c_int, [_P, C.c_int]),
    "pb_flow_arena_bytes": (C.c_int64, [_P]),
    "pb_mask_set_sdf": (C.c_int, [_P, _P, _P, C.c_int]),
    "pb_mask_sdf_green": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int]),
    "pb_mask_sdf_green_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int]),
    "pb_flow_out_size": (C.c_int, [C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pb_flow_infer_sequence": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _P, _P, _P]),
    "pb_flow_infer_sequence_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _P, _P, _P]),
    "pb_flow_infer_sequence_masks": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float,
                                               _P, _P, _P, _P]),
    "pb_flow_infer_sequence_masks_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                                   C.c_float, _P, _P, _P, _P]),
    "pb_flow_fwdbwd_mask": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P]),
    "pb_flow_get_stage": (C.c_int64, [_P, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "pb_dev_alloc": (C.c_int, [_P, C.POINTER(_P), C.c_size_t]),
    "pb_dev_free": (C.c_int, [_P, _P]),
    "pb_memcpy_h2d": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "pb_memcpy_d2h": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "pb_set_profiling": (C.c_int, [_P, C.c_int]),
    "pb_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "pb_get_kernel_stats": (C.c_int, [_P, C.POINTER(pb_kernel_stat), C.c_int]),
    "pb_op_gemm": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "pb_op_gemm_bench": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "pb_op_corr_volume": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_op_corr_volume_blocked": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_op_corr_layout_index": (C.c_int, [C.c_int, C.c_int, C.c_int, _P]),
    "pb_op_attention_bench": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "pb_op_layernorm": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int]),
    "pb_op_attention": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "pb_op_attention128": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int]),
    "pb_op_attention128_split": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "pb_op_conv2d": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 10),
    "pb_op_conv2d_split": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 18 + [_P, _P, _P, C.c_int]),
    "pb_op_dense_split": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 9 + [_P, _P, _P, C.c_int]),
    "pb_op_gemm_resid": (C.c_int, [_P, _P, _P, _P, _P, _P] + [C.c_int] * 7 + [_P, _P, _P, C.c_int]),
    "pb_op_gemm_qkv": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 6 + [_P, _P, _P, _P, _P, C.c_int]),
    "pb_op_gemm_patch": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 6 + [_P, _P, _P, C.c_int]),
    "pb_op_raft_gru_zr": (C.c_int, [_P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 9 + [_P, _P, _P, _P, C.c_int]),
    "pb_op_raft_gru_q": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P] + [C.c_int] * 9 + [_P, _P, _P, C.c_int]),
    "pb_op_conv_pixshuf": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 6 + [_P, _P, _P, C.c_int]),
    "pb_op_gemm_fc1": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [_P, _P, _P, C.c_int]),
    "pb_op_gemm_pixshuf": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 8 + [_P, _P, _P, C.c_int]),
    "pb_op_conv_head": (C.c_int, [_P, _P, _P, _P, _P, C.c_float] + [C.c_int] * 6 + [_P, _P, _P, C.c_int]),
    "pb_op_raft_geometry": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "pb_op_raft_lookup": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [_P, _P]),
    "pb_op_raft_lookup_otf": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [_P]),
    "pb_op_raft_convf1": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 7 + [_P]),
    "pb_op_raft_flow_head2": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 5),
    "pb_op_raft_upsample": (C.c_int, [_P, _P, _P] + [C.c_int] * 8 + [_P, _P]),
    "pb_op_raft_instnorm": (C.c_int, [_P, _P, _P] + [C.c_int] * 8 + [_P, _P]),
    "pb_op_raft_state": (C.c_int, [_P, _P, _P] + [C.c_int] * 4 + [_P, _P, _P, _P]),
    "pb_op_flow_geometry": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_int)]),
    "pb_op_flow_taps": (C.c_int, [C.c_int, C.c_int, C.c_float, _P, _P]),
    "pb_op_flow_prep": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float] + [C.c_int] * 7 + [_P, _P, C.POINTER(C.c_int)]),
    "pb_op_flow_resize_back": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P, _P]),
    "pb_op_flow_encode": (C.c_int, [_P, _P, _P] + [C.c_int] * 4 + [_P, _P]),
    "pb_op_gm_tables": (C.c_int, [C.c_int, C.c_int, _P, _P]),
    "pb_op_gm_tables_n": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P]),
    "pb_op_gm_tokens_warped": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 4 + [_P, _P]),
    "pb_op_gm_warp": (C.c_int, [_P, _P, _P] + [C.c_int] * 5 + [_P, _P]),
    "pb_op_gm_upsample": (C.c_int, [_P, _P, _P] + [C.c_int] * 9 + [_P, _P]),
    "pb_op_gm_pack_n": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P, _P, C.c_int, C.c_int, _P]),
    "pb_op_gm_ln_n": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 9 + [_P]),
    "pb_op_gm_window_block_n": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 8),
    "pb_op_gm_tokens": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "pb_op_gm_split_rows": (C.c_int, [_P, _P] + [C.c_int] * 4 + [_P]),
    "pb_op_gm_grid_vt": (C.c_int, [_P] + [C.c_int] * 3 + [_P]),
    "pb_op_gm_pack": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P, _P, C.c_int, C.c_int, _P]),
    "pb_op_gm_ln": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 8 + [_P]),
    "pb_op_gm_match_flow": (C.c_int, [_P, _P] + [C.c_int] * 4 + [_P, _P]),
    "pb_op_gm_upsampler_in": (C.c_int, [_P, _P, _P] + [C.c_int] * 5 + [_P, _P]),
    "pb_op_attention128_cfg": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P] + [C.c_int] * 9 + [C.c_float]),
    "pb_op_gm_window_block": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 6),
    "pb_op_gm_match": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P]),
    "pb_op_gm_propagate": (C.c_int, [_P, _P, _P, _P, _P] + [C.c_int] * 6 + [_P, _P, _P]),
    "pb_op_gm_local_match": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P]),
    "pb_op_gm_local_propagate": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 6 + [_P]),
    "pb_op_mask_prep": (C.c_int, [_P, _P] + [C.c_int] * 7 + [_P, _P, C.c_int, C.c_int, _P, _P]),
    "pb_op_mask_maxpool": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P]),
    "pb_op_mask_nearest_add": (C.c_int, [_P, _P, _P] + [C.c_int] * 8 + [_P]),
    "pb_op_mask_subsample2": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P]),
    "pb_op_mask_coord_concat": (C.c_int, [_P, _P] + [C.c_int] * 7 + [_P]),
    "pb_op_mask_bilinear": (C.c_int, [_P, _P, _P] + [C.c_int] * 10 + [_P]),
    "pb_op_mask_gn_relu": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 5 + [_P, _P]),
    "pb_op_mask_cls_points_nms": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P]),
    "pb_op_mask_gather_rows": (C.c_int, [_P, _P, C.c_int, _P] + [C.c_int] * 5 + [_P]),
    "pb_op_mask_stats": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _P]),
    "pb_op_mask_intersections": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_int, _P, C.c_int, _P]),
    "pb_op_mask_matrix_nms": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_float, C.c_int, _P, _P]),
    "pb_op_mask_sigmoid_rows": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_op_mask_dynconv": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "pb_op_mask_band_accumulate": (C.c_int, [_P, _P, _P] + [C.c_int] * 7 + [C.c_float, C.c_int, _P, _P]),
    "pb_op_depth_layernorm": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 8 + [C.c_float, C.c_int, C.c_int, _P, _P]),
    "pb_op_depth_attention": (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 6 + [C.c_float, C.c_int, _P]),
    "pb_op_depth_preprocess": (C.c_int, [_P, _P] + [C.c_int] * 7 + [_P, _P]),
    "pb_op_depth_cls_rows":(C.c_int, [_P, _P, _P] + [C.c_int] * 4 + [_P]),
    "pb_op_depth_dpt_tail": (C.c_int, [_P, _P, _P, _P, C.c_float] + [C.c_int] * 8 + [_P, _P]),
    "pb_op_depth_resize_minmax": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P, _P]),
    "pb_op_zoe_softplus": (C.c_int, [_P, _P] + [C.c_int] * 4),
    "pb_op_zoe_dot32_relu": (C.c_int, [_P, _P, C.c_int, _P, C.c_float, C.c_int, C.c_int, _P]),
    "pb_op_zoe_bilerp_add": (C.c_int, [_P, _P, _P] + [C.c_int] * 10 + [_P]),
    "pb_op_zoe_attractor": (C.c_int, [_P, _P, C.c_int, C.c_int, _P] + [C.c_int] * 5 + [C.c_float, C.c_int, _P]),
    "pb_op_zoe_cat": (C.c_int, [_P, _P, C.c_int, _P, _P] + [C.c_int] * 7 + [_P]),
    "pb_op_zoe_logbinom_depth": (C.c_int, [_P, _P, C.c_int, _P] + [C.c_int] * 5 + [C.c_float, C.c_float, C.c_int, _P]),
    "pb_op_zoe_pil_resize": (C.c_int, [_P, _P] + [C.c_int] * 6 + [_P]),
    "pb_op_bilinear": (C.c_int, [_P, _P, _P] + [C.c_int] * 7),
    "pb_op_preprocess": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int]),
    "pb_op_encode_depth": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
}

_lib = None


class PrismaBandsError(RuntimeError):
    pass


def load():
    """Load the shared library and bind every declared symbol (raises if any is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PrismaBandsError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C prisma_amd/csrc).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.pb_abi_version() != ABI_VERSION:
        raise PrismaBandsError(f"{LIB_PATH}: ABI version {lib.pb_abi_version()}, this binding expects {ABI_VERSION} - rebuild the library "
                               "(make -C prisma_amd/csrc) or update prisma_amd/_lib.py")
    for which, st in ((0, pb_tensor), (1, pb_depth_cfg), (2, pb_flow_cfg), (3, pb_mask_cfg), (4, pb_kernel_stat), (6, pb_yuv_fmt), (7, pb_jpeg_cfg)):
        if lib.pb_struct_size(which) != C.sizeof(st):
            raise PrismaBandsError(f"{LIB_PATH}: sizeof({st.__name__}) is {lib.pb_struct_size(which)} in the library, {C.sizeof(st)} in the binding")
    _lib = lib
    return lib


def check(rc: int):
    if rc < 0:
        raise PrismaBandsError(f"libprisma_bands: {load().pb_last_error().decode()} (status {rc})")
    return rc
