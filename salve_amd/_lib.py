"""ctypes binding of libsalve_hip.so (C ABI: include/salve_hip.h).

The product path has NO fallback: if the HIP library has not been built
(`python -c "import __graft_entry__ as g; g.build()"`) every entry point raises.
"""

from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np

import os

# SALVE_HIP_LIB: development override (ablation builds of tools/probe/build_ablations.sh); the product loads the in-tree library
LIB_PATH = Path(os.environ.get("SALVE_HIP_LIB") or (Path(__file__).resolve().parent / "libsalve_hip.so"))

SALVE_OK = 0
EXPECTED_ABI = 7          # include/salve_hip.h: SALVE_HIP_ABI_VERSION
TILE_F32_NCHW = 0
TILE_F16_NHWC = 1
TILE_U8X4 = 2
TILE_F32_NHWC = 3         # salve_bev_train_tiles only
TILE_BF16_NHWC = 4

# every symbol include/salve_hip.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = (
    "salve_hip_version",
    "salve_last_error",
    "salve_bev_workspace_bytes",
    "salve_bev_pano_index_bytes",
    "salve_bev_pano_index_build",
    "salve_bev_render_batch",
    "salve_bev_scatter",
    "salve_bev_densify",
    "salve_bev_scatter_points",
    "salve_zorder_winners",
    "salve_remove_hallucinated",
    "salve_bev_keys_from_pixels",
    "salve_bev_export_u8",
    "salve_layout_rasterise",
    "salve_bev_tiles",
    "salve_bev_tile_pairs",
    "salve_bev_densify_tiles",
    "salve_resize_rgb_u8",
    "salve_resnet_create",
    "salve_resnet_destroy",
    "salve_resnet_workspace_bytes",
    "salve_resnet_forward",
    "salve_resnet_num_layers",
    "salve_resnet_f32_create",
    "salve_resnet_f32_destroy",
    "salve_resnet_f32_workspace_bytes",
    "salve_resnet_f32_forward",
    "salve_resnet_bf16x3_create",
    "salve_bev_tiles_aug",
    "salve_conv_f32_workspace_bytes",
    "salve_conv_f32_forward",
    "salve_conv_f32_backward_data",
    "salve_conv_f32_backward_weight",
    "salve_conv_bf16_workspace_bytes",
    "salve_conv_bf16_forward",
    "salve_conv_bf16_backward_data",
    "salve_conv_bf16_backward_weight",
    "salve_bn_workspace_bytes",
    "salve_bn_f32_forward",
    "salve_bn_f32_backward",
    "salve_bn_bf16_forward",
    "salve_bn_bf16_backward",
    "salve_bn_f32_stats",
    "salve_bn_bf16_stats",
    "salve_bn_combine",
    "salve_bn_f32_apply",
    "salve_bn_bf16_apply",
    "salve_bn_f32_backward_reduce",
    "salve_bn_bf16_backward_reduce",
    "salve_bn_f32_backward_apply",
    "salve_bn_bf16_backward_apply",
    "salve_bev_train_tiles",
    "salve_bev_pano_index_update",
    "salve_layout_pose",
    "salve_adam_step",
    "salve_head_workspace_bytes",
    "salve_head_f32_forward",
    "salve_head_f32_backward",
    "salve_head_bf16_forward",
    "salve_head_bf16_backward",
    "salve_bev_jpeg_roundtrip_workspace_bytes",
    "salve_bev_jpeg_roundtrip",
    "salve_bev_jpeg_encode_workspace_bytes",
    "salve_bev_jpeg_encode_max_bytes",
    "salve_bev_jpeg_encode",
    "salve_bev_jpeg_decode_workspace_bytes",
    "salve_bev_jpeg_decode",
    "salve_bev_jpeg_decode_lanes_workspace_bytes",
    "salve_bev_jpeg_subseq_bytes",
    "salve_bev_jpeg_decode_lanes",
    "salve_bev_jpeg_decode_sampled_workspace_bytes",
    "salve_bev_jpeg_decode_lanes_sampled_workspace_bytes",
    "salve_bev_jpeg_decode_sampled",
    "salve_bev_jpeg_decode_lanes_sampled",
    "salve_bev_train_tiles_jitter_workspace_bytes",
    "salve_bev_train_tiles_jitter",
    "salve_flat_pack",
    "salve_flat_unpack",
    "salve_bev_pair_overlap",
    "salve_pose_graph_workspace_bytes",
    "salve_pose_graph_solve",
    "salve_pose_graph_sample_workspace_bytes",
    "salve_pose_graph_sample_trees",
    "salve_pose_graph_optimise_workspace_bytes",
    "salve_pose_graph_optimise",
    "salve_floor_align",
    "salve_floor_iou_workspace_bytes",
    "salve_floor_iou",
    "salve_hypotheses_generate",
    "salve_pose_graph_axis_align",
)
# salve_resnet_create flags (include/salve_hip.h: SALVE_RESNET_*): kernel selection for the bit-identity tests; 0 = product
RESNET_CONV_IGEMM_ONLY, RESNET_CONV8_WHEREVER, RESNET_ROUND_ROBIN_TILES, RESNET_NO_STEM_FUSE, RESNET_NO_BLOCK_FUSE = 1, 2, 4, 8, 16
RESNET_NO_PROJ_FUSE, RESNET_NO_CHAIN, RESNET_CHAIN_EXPAND_ONLY, RESNET_CHAIN_16_WAVES, RESNET_CHAIN_NO_SPLIT = 32, 64, 128, 256, 512
RESNET_CHAIN_STORE_ALL, RESNET_NO_TRANSPOSED_TILES, RESNET_NO_NEXT_FUSE = 1024, 2048, 4096
JPEG_STAGE_ENTROPY, JPEG_STAGE_INVERSE, JPEG_STAGES_ALL = 1, 2, 3   # salve_bev_jpeg_decode's `stages`
JPEG_SAMPLINGS = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2, "grey": 3}     # include/salve_hip.h: SALVE_JPEG_SAMPLING_* by salve_amd.jpeg's names
STATUS_WALK_FAILED = 1
STATUS_FP16_RANGE = 2
STATUS_BAD_HYPOTHESIS = 4
STATUS_LAYOUT_THICKNESS = 8
STATUS_BAD_TILE_JOB = 16
STATUS_BAD_PANO_SLOT = 32
STATUS_BAD_LAYOUT = 64
STATUS_BAD_GRAPH_ROW = 128
STATUS_BAD_FLOOR_TABLE = 256
STATUS_BAD_AXIS_ROW = 512


class BevConfig(ctypes.Structure):
    """salve_bev_config_t"""

    _fields_ = [
        ("pano_h", ctypes.c_int32), ("pano_w", ctypes.c_int32), ("crop_rows", ctypes.c_int32),
        ("bev_h", ctypes.c_int32), ("bev_w", ctypes.c_int32), ("mask_k", ctypes.c_int32),
        ("depth_scale", ctypes.c_float), ("out_flags", ctypes.c_int32),
        ("win_xmin", ctypes.c_double), ("win_xmax", ctypes.c_double),
        ("win_ymin", ctypes.c_double), ("win_ymax", ctypes.c_double),
        ("img_tx", ctypes.c_double), ("img_ty", ctypes.c_double), ("img_scale", ctypes.c_double),
        ("rot_pre", ctypes.c_double * 4),
        ("z_lo", ctypes.c_double * 2), ("z_hi", ctypes.c_double * 2),
        ("z_min", ctypes.c_double), ("n_slices", ctypes.c_int32), ("reserved1", ctypes.c_int32),
    ]


HYP_DTYPE = np.dtype(
    [("pano_idx", "<i4"), ("surface", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)), ("apply_pose", "<i4"),
     ("reserved", "<i4")]
)
TILE_JOB_DTYPE = np.dtype([("bev_offset", "<i8"), ("slot", "<i4"), ("chan", "<i4")])
LAYOUT_DTYPE = np.dtype([("n_poly", "<i4"), ("poly_off", "<i4"), ("n_seg", "<i4"), ("seg_off", "<i4")])
LAYOUT_POSE_DTYPE = np.dtype([("pano", "<i4"), ("poly_off", "<i4"), ("seg_off", "<i4"), ("reserved", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)),
                              ("s", "<f8")])
JPEG_SEGMENT_DTYPE = np.dtype([("offset", "<i8"), ("bytes", "<i4"), ("image", "<i4"), ("first_mcu", "<i4"), ("mcu_count", "<i4")])   # salve_jpeg_segment_t
JPEG_MAX_SEGMENTS = 1 << 24
TILE_AUG_DTYPE = np.dtype([("crop_y", "<i4"), ("crop_x", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])
TILE_HFLIP, TILE_VFLIP = 1, 2
assert LAYOUT_POSE_DTYPE.itemsize == 48 and HYP_DTYPE.itemsize == 40 and TILE_JOB_DTYPE.itemsize == 16 and TILE_AUG_DTYPE.itemsize == 16
OVERLAP_JOB_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4")])   # salve_overlap_job_t (salve_bev_pair_overlap): image index into bev_a / bev_b
assert OVERLAP_JOB_DTYPE.itemsize == 8
# salve_pose_graph_solve (include/salve_hip.h: salve_graph_row_t and the three output records)
GRAPH_MAX_NODES = 256
GRAPH_ROW_DTYPE = np.dtype([("i1", "<i4"), ("i2", "<i4"), ("prob", "<f4"), ("y_hat", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)), ("s", "<f8")])
GRAPH_ROW_OUT_DTYPE = np.dtype([("chosen", "<i4"), ("consistent", "<i4"), ("n_triplets", "<i4"), ("n_consistent", "<i4"), ("min_rot_err", "<f4"),
                                ("min_trans_err", "<f4")])
GRAPH_NODE_OUT_DTYPE = np.dtype([("localized", "<i4"), ("parent", "<i4"), ("depth", "<i4"), ("reserved", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)),
                                 ("s", "<f8")])
GRAPH_FLOOR_OUT_DTYPE = np.dtype([("n_chosen", "<i4"), ("n_triplets", "<i4"), ("n_consistent_triplets", "<i4"), ("n_consistent_edges", "<i4"),
                                  ("n_localized", "<i4"), ("origin", "<i4")])
assert GRAPH_ROW_DTYPE.itemsize == 48 and GRAPH_ROW_OUT_DTYPE.itemsize == 24 and GRAPH_NODE_OUT_DTYPE.itemsize == 48 and GRAPH_FLOOR_OUT_DTYPE.itemsize == 24
# salve_pose_graph_sample_trees (salve_graph_tree_out_t, salve_graph_sample_floor_out_t)
GRAPH_TREE_OUT_DTYPE = np.dtype([("avg_rot_err", "<f8"), ("avg_trans_err", "<f8"), ("n_localized", "<i4"), ("n_measured", "<i4"), ("n_edges", "<i4"),
                                 ("origin", "<i4"), ("floor", "<i4"), ("reserved", "<i4")])
GRAPH_SAMPLE_FLOOR_OUT_DTYPE = np.dtype([("best", "<i4"), ("n_candidates", "<i4"), ("n_hyps", "<i4"), ("n_improvements", "<i4"), ("avg_rot_err", "<f8"),
                                         ("avg_trans_err", "<f8")])
assert GRAPH_TREE_OUT_DTYPE.itemsize == 40 and GRAPH_SAMPLE_FLOOR_OUT_DTYPE.itemsize == 32
# salve_pose_graph_optimise (salve_graph_pgo_floor_out_t, SALVE_PGO_*)
GRAPH_PGO_FLOOR_OUT_DTYPE = np.dtype([("n_unknown_nodes", "<i4"), ("n_factors", "<i4"), ("n_iterations", "<i4"), ("n_rejected", "<i4"),
                                      ("n_downweighted", "<i4"), ("stop_reason", "<i4"), ("lambda", "<f8"), ("cost_initial", "<f8"), ("cost_final", "<f8")])
assert GRAPH_PGO_FLOOR_OUT_DTYPE.itemsize == 48
PGO_LDS_NODES = 56
PGO_STOP_EMPTY, PGO_STOP_ABSOLUTE, PGO_STOP_RELATIVE, PGO_STOP_LAMBDA, PGO_STOP_MAX_ITERATIONS, PGO_STOP_NON_FINITE = 0, 1, 2, 3, 4, 5
PGO_STOP_NAMES = ("empty", "absolute_error_tol", "relative_error_tol", "lambda_bound", "max_iterations", "non_finite")
# salve_pose_graph_axis_align (salve_axis_wdo_t, salve_axis_row_out_t, salve_axis_floor_out_t, SALVE_AXIS_*)
AXIS_WDO_DTYPE = np.dtype([("type", "<i4"), ("index", "<i4")])
AXIS_ROW_OUT_DTYPE = np.dtype([("status", "<i4"), ("reserved", "<i4"), ("correction_deg", "<f8"), ("theta_deg", "<f8"), ("t", "<f8", (2,))])
AXIS_FLOOR_OUT_DTYPE = np.dtype([("n_applied", "<i4"), ("n_too_large", "<i4"), ("n_no_angle", "<i4"), ("n_no_room", "<i4"), ("n_malformed", "<i4"),
                                 ("bad_extent", "<i4")])
assert AXIS_WDO_DTYPE.itemsize == 8 and AXIS_ROW_OUT_DTYPE.itemsize == 40 and AXIS_FLOOR_OUT_DTYPE.itemsize == 24
AXIS_APPLIED, AXIS_TOO_LARGE, AXIS_NO_ANGLE, AXIS_NO_ROOM, AXIS_MALFORMED = 0, 1, 2, 3, 4
AXIS_STATUS_NAMES = ("applied", "too_large", "no_angle", "no_room", "malformed")
# salve_floor_align, salve_floor_iou (salve_floor_hyp_out_t, salve_floor_align_out_t, salve_floor_iou_out_t)
FLOOR_MASK_WORDS = 8
FLOOR_HYP_OUT_DTYPE = np.dtype([("R", "<f8", (4,)), ("t", "<f8", (2,)), ("s", "<f8"), ("rot_err", "<f8"), ("trans_err", "<f8"), ("n_pairs", "<i4"),
                                ("floor", "<i4")])
FLOOR_ALIGN_OUT_DTYPE = np.dtype([("best", "<i4"), ("n_hyps", "<i4"), ("n_est", "<i4"), ("n_gt", "<i4"), ("avg_rot_err", "<f8"),
                                  ("avg_trans_err", "<f8"), ("percent_localized", "<f8"), ("R", "<f8", (4,)), ("t", "<f8", (2,)), ("s", "<f8")])
FLOOR_IOU_OUT_DTYPE = np.dtype([("n_est", "<i4"), ("n_gt", "<i4"), ("inter", "<i4"), ("uni", "<i4"), ("bad", "<i4"), ("reserved", "<i4"), ("iou", "<f8")])
assert FLOOR_HYP_OUT_DTYPE.itemsize == 80 and FLOOR_ALIGN_OUT_DTYPE.itemsize == 96 and FLOOR_IOU_OUT_DTYPE.itemsize == 32
# salve_hypotheses_generate (salve_hyp_pair_t, salve_hyp_row_t, salve_hyp_pair_out_t)
HYP_MAX_WDO_PER_TYPE = 32
HYP_MAX_CAPACITY = 5120
HYP_PAIR_DTYPE = np.dtype([("pano1", "<i4"), ("pano2", "<i4"), ("capacity", "<i4"), ("reserved", "<i4"), ("row_offset", "<i8")])
HYP_ROW_DTYPE = np.dtype([("R", "<f4", (4,)), ("t", "<f4", (2,)), ("type", "<i4"), ("i", "<i4"), ("j", "<i4"), ("configuration", "<i4"), ("label", "<i4"),
                          ("reserved", "<i4")])
HYP_PAIR_OUT_DTYPE = np.dtype([("n_kept", "<i4"), ("n_valid", "<i4"), ("n_rejected", "<i4"), ("visibly_adjacent", "<i4"), ("R", "<f4", (4,)),
                               ("t", "<f4", (2,)), ("s", "<f8")])
assert HYP_PAIR_DTYPE.itemsize == 24 and HYP_ROW_DTYPE.itemsize == 48 and HYP_PAIR_OUT_DTYPE.itemsize == 48
# salve_tile_jitter_t (salve_bev_train_tiles_jitter): one ColorJitter draw per image; the operation codes are torchvision's fn_id and the mask's bit numbers
TILE_JITTER_DTYPE = np.dtype([("order", "u1", (4,)), ("mask", "<i4"), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue", "<f4"),
                              ("brightness_c", "<f4"), ("contrast_c", "<f4"), ("saturation_c", "<f4"), ("reserved", "<i4")])
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = 0, 1, 2, 3
assert TILE_JITTER_DTYPE.itemsize == 40

# salve_conv_f32_* / salve_conv_bf16_* passes (include/salve_hip.h: SALVE_CONV_*)
CONV_FWD, CONV_DGRAD, CONV_WGRAD = 0, 1, 2
SALVE_ERR_BAD_ARG, SALVE_ERR_UNSUPPORTED = -1, -2


class ConvDesc(ctypes.Structure):
    """salve_conv_desc_t"""

    _fields_ = [(n, ctypes.c_int32) for n in ("batch", "Hi", "Wi", "Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad")]


# salve_bn_* flags and passes (include/salve_hip.h: SALVE_BN_*)
BN_RELU, BN_ADD, BN_EVAL = 1, 2, 4
BN_FWD, BN_BWD = 0, 1
BN_STATS, BN_BWD_REDUCE = 16, 17   # the split (synchronised) entries' workspace passes
BN_MAX_WORLD = 64


class BnDesc(ctypes.Structure):
    """salve_bn_desc_t"""

    _fields_ = [("rows", ctypes.c_int32), ("C", ctypes.c_int32), ("flags", ctypes.c_int32), ("eps", ctypes.c_float),
                ("momentum", ctypes.c_float)]


# salve_adam_step tables (include/salve_hip.h: salve_adam_segment_t, salve_adam_chunk_t, SALVE_ADAM_CHUNK)
ADAM_CHUNK = 4096
ADAM_SEGMENT_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("shadow_bf16", "<u8"), ("n", "<i8"),
                               ("step_size", "<f4"), ("sqrt_bc2", "<f4"), ("beta1", "<f4"), ("beta2", "<f4"), ("eps", "<f4"),
                               ("weight_decay", "<f4"), ("one_minus_beta1", "<f4"), ("one_minus_beta2", "<f4")])
ADAM_CHUNK_DTYPE = np.dtype([("segment", "<i4"), ("reserved", "<i4"), ("offset", "<i8")])
assert ADAM_SEGMENT_DTYPE.itemsize == 80 and ADAM_CHUNK_DTYPE.itemsize == 16
# salve_flat_pack / salve_flat_unpack (include/salve_hip.h: salve_flat_segment_t); the chunk map is salve_adam_step's
FLAT_SEGMENT_DTYPE = np.dtype([("tensor", "<u8"), ("n", "<i8"), ("offset", "<i8")])
assert FLAT_SEGMENT_DTYPE.itemsize == 24

# salve_head_* (include/salve_hip.h: SALVE_HEAD_*, salve_head_desc_t, salve_head_meter_t): the training classifier head.  It stands
# behind the reference's avgpool + flatten + fc (salve/models/early_fusion.py:78-83), its softmax and cross-entropy
# (salve/train_utils.py:18-41) and its per-class accuracy meter (salve/utils/avg_meter.py)
HEAD_MAX_CLASSES = 16
HEAD_ACCUMULATE_LOSS = 1
HEAD_FWD, HEAD_BWD = 0, 1
HEAD_METER_DTYPE = np.dtype([("total", "<i8", (HEAD_MAX_CLASSES,)), ("correct", "<i8", (HEAD_MAX_CLASSES,)), ("loss_sum", "<f8"), ("loss_rows", "<i8"),
                             ("bad_targets", "<i8")])
assert HEAD_METER_DTYPE.itemsize == 280


class HeadDesc(ctypes.Structure):
    """salve_head_desc_t"""

    _fields_ = [(n, ctypes.c_int32) for n in ("B", "HW", "C", "K", "flags")]


_lib = None


class SalveHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load the HIP library or raise -- never substitute a CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise SalveHipError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run __graft_entry__.build() "
            "(hipcc --offload-arch=gfx950). salve_amd has no CPU fallback."
        )
    lib = ctypes.CDLL(str(LIB_PATH))
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    lib.salve_hip_version.restype = ctypes.c_int
    lib.salve_last_error.restype = ctypes.c_char_p
    lib.salve_bev_workspace_bytes.argtypes = [ctypes.POINTER(BevConfig), i32]
    lib.salve_bev_workspace_bytes.restype = sz
    lib.salve_bev_pano_index_bytes.argtypes = [ctypes.POINTER(BevConfig), i32]
    lib.salve_bev_pano_index_bytes.restype = sz
    lib.salve_bev_pano_index_build.argtypes = [ctypes.POINTER(BevConfig), vp, i32, vp, vp, sz, vp]
    lib.salve_bev_pano_index_build.restype = ctypes.c_int
    lib.salve_bev_pano_index_update.argtypes = [ctypes.POINTER(BevConfig), vp, i32, vp, vp, sz, vp, i32, vp, vp]
    lib.salve_bev_pano_index_update.restype = ctypes.c_int
    lib.salve_bev_render_batch.argtypes = [ctypes.POINTER(BevConfig), vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.salve_bev_render_batch.restype = ctypes.c_int
    lib.salve_bev_scatter.argtypes = [ctypes.POINTER(BevConfig), vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.salve_bev_scatter.restype = ctypes.c_int
    lib.salve_bev_densify.argtypes = [ctypes.POINTER(BevConfig), i32, vp, vp, vp, vp, vp, sz, vp]
    lib.salve_bev_densify.restype = ctypes.c_int
    lib.salve_bev_scatter_points.argtypes = [ctypes.POINTER(BevConfig), vp, vp, i32, vp, vp, vp, sz, vp]
    lib.salve_bev_scatter_points.restype = ctypes.c_int
    lib.salve_zorder_winners.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp]
    lib.salve_zorder_winners.restype = ctypes.c_int
    lib.salve_remove_hallucinated.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    lib.salve_remove_hallucinated.restype = ctypes.c_int
    lib.salve_bev_keys_from_pixels.argtypes = [ctypes.POINTER(BevConfig), vp, vp, i32, vp, vp, sz, vp]
    lib.salve_bev_keys_from_pixels.restype = ctypes.c_int
    lib.salve_layout_rasterise.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp]
    lib.salve_layout_rasterise.restype = ctypes.c_int
    f64, i64 = ctypes.c_double, ctypes.c_int64
    lib.salve_layout_pose.argtypes = [vp, vp, i64, vp, vp, vp, i64, i32, vp, i32, f64, f64, f64, i32, vp, vp, i32, vp, i32, vp, vp]
    lib.salve_layout_pose.restype = ctypes.c_int
    lib.salve_bev_export_u8.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.salve_bev_export_u8.restype = ctypes.c_int
    lib.salve_bev_tiles.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp]
    lib.salve_bev_tiles.restype = ctypes.c_int
    lib.salve_bev_tile_pairs.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp]
    lib.salve_bev_tile_pairs.restype = ctypes.c_int
    lib.salve_bev_densify_tiles.argtypes = [ctypes.POINTER(BevConfig), i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, sz, vp]
    lib.salve_bev_densify_tiles.restype = ctypes.c_int
    lib.salve_resize_rgb_u8.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, vp, vp]
    lib.salve_resize_rgb_u8.restype = ctypes.c_int
    lib.salve_resnet_create.argtypes = [i32, i32, vp, i32, vp, sz, vp, sz, vp, sz, i32]
    lib.salve_resnet_create.restype = vp
    lib.salve_resnet_destroy.argtypes = [vp]
    lib.salve_resnet_destroy.restype = None
    lib.salve_resnet_workspace_bytes.argtypes = [vp, i32]
    lib.salve_resnet_workspace_bytes.restype = sz
    lib.salve_resnet_forward.argtypes = [vp, vp, i32, vp, vp, sz, vp, vp]
    lib.salve_resnet_forward.restype = ctypes.c_int
    lib.salve_resnet_num_layers.argtypes = [vp]
    lib.salve_resnet_num_layers.restype = ctypes.c_int
    lib.salve_resnet_f32_create.argtypes = [i32, i32, vp, i32, vp, sz, vp, sz, vp, sz, i32]
    lib.salve_resnet_f32_create.restype = vp
    lib.salve_resnet_bf16x3_create.argtypes = [i32, i32, vp, i32, vp, sz, vp, sz, vp, sz, i32]
    lib.salve_resnet_bf16x3_create.restype = vp
    lib.salve_resnet_f32_destroy.argtypes = [vp]
    lib.salve_resnet_f32_destroy.restype = None
    lib.salve_resnet_f32_workspace_bytes.argtypes = [vp, i32]
    lib.salve_resnet_f32_workspace_bytes.restype = sz
    lib.salve_resnet_f32_forward.argtypes = [vp, vp, i32, vp, vp, sz, vp, vp]
    lib.salve_resnet_f32_forward.restype = ctypes.c_int
    lib.salve_bev_tiles_aug.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, i32, vp, vp, i32, vp]
    lib.salve_bev_tiles_aug.restype = ctypes.c_int
    lib.salve_bev_train_tiles.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp, i32, vp, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp]
    lib.salve_bev_train_tiles.restype = ctypes.c_int
    lib.salve_bev_train_tiles_jitter_workspace_bytes.argtypes = [i32, i32]
    lib.salve_bev_train_tiles_jitter_workspace_bytes.restype = sz
    lib.salve_bev_train_tiles_jitter.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp, i32, vp, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, sz, vp, vp]
    lib.salve_bev_train_tiles_jitter.restype = ctypes.c_int
    lib.salve_bev_pair_overlap.argtypes = [vp, i32, vp, i32, i32, i32, vp, i32, vp, vp, vp]   # bev_a, n_a, bev_b, n_b, h, w, jobs, n_jobs, out, status, stream
    lib.salve_bev_pair_overlap.restype = ctypes.c_int
    lib.salve_pose_graph_workspace_bytes.argtypes = [i32, i32]
    lib.salve_pose_graph_workspace_bytes.restype = sz
    # rows, n_rows, floor_start, n_nodes, n_floors, max_nodes, confidence, rot_deg, trans, cycle_filter, out_rows, out_nodes, out_floors, ws, ws_bytes, status, stream
    lib.salve_pose_graph_solve.argtypes = [vp, i32, vp, vp, i32, i32, ctypes.c_float, ctypes.c_float, ctypes.c_float, i32, vp, vp, vp, vp, sz, vp, vp]
    lib.salve_pose_graph_solve.restype = ctypes.c_int
    lib.salve_pose_graph_sample_workspace_bytes.argtypes = [i32, i32]
    lib.salve_pose_graph_sample_workspace_bytes.restype = sz
    # rows, n_rows, floor_start, n_nodes, n_floors, max_nodes, confidence, hyp_start, hyp_mask, n_hyps, mask_words, out_trees, out_inlier, out_nodes,
    # out_floors, ws, ws_bytes, status, stream
    lib.salve_pose_graph_sample_trees.argtypes = [vp, i32, vp, vp, i32, i32, ctypes.c_float, vp, vp, i32, i32, vp, vp, vp, vp, vp, sz, vp, vp]
    lib.salve_pose_graph_sample_trees.restype = ctypes.c_int
    lib.salve_pose_graph_optimise_workspace_bytes.argtypes = [i32, i32]
    lib.salve_pose_graph_optimise_workspace_bytes.restype = sz
    # rows, n_rows, floor_start, n_nodes, n_floors, max_nodes, confidence, init, robust, huber_k, HOST odometry_sigmas, HOST prior_sigmas, max_iterations,
    # relative_error_tol, absolute_error_tol, out_nodes, out_pose, out_floors, ws, ws_bytes, status, stream
    lib.salve_pose_graph_optimise.argtypes = [vp, i32, vp, vp, i32, i32, ctypes.c_float, vp, i32, ctypes.c_double, vp, vp, i32, ctypes.c_double,
                                              ctypes.c_double, vp, vp, vp, vp, sz, vp, vp]
    lib.salve_pose_graph_optimise.restype = ctypes.c_int
    # (node_start, n_floors, n_nodes, truth, est, hyp_start, hyp_mask, n_hyps, gt_scale, metres, out_hyps, out_nodes, out_rot_err, out_trans_err,
    #  out_floors, status, stream)
    lib.salve_floor_align.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.salve_floor_align.restype = ctypes.c_int
    lib.salve_floor_iou_workspace_bytes.argtypes = [ctypes.c_int64, i32]
    lib.salve_floor_iou_workspace_bytes.restype = sz
    # (room_xy, room_off, n_room_xy, node_start, n_floors, n_nodes, est, truth, metres, img_h, img_w, offset_x, offset_y, pixels_per_metre, out,
    #  out_masks, workspace, workspace_bytes, status, stream)
    lib.salve_floor_iou.argtypes = [vp, vp, ctypes.c_int64, vp, i32, i32, vp, vp, vp, i32, i32, ctypes.c_float, ctypes.c_float, ctypes.c_double, vp, vp,
                                    vp, sz, vp, vp]
    lib.salve_floor_iou.restype = ctypes.c_int
    # wdo_xy, wdo_type, wdo_off, n_wdo, gt_xy, gt_off, n_gt, poses, n_panos, pairs, n_pairs, max_capacity, min_width_ratio, out_rows, n_rows, out_pairs, stream
    lib.salve_hypotheses_generate.argtypes = [vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, i32, vp, ctypes.c_int64, i32, ctypes.c_double, vp,
                                              ctypes.c_int64, vp, vp]
    lib.salve_hypotheses_generate.restype = ctypes.c_int
    # rows, n_rows, floor_start, n_nodes, n_floors, row_wdo, pano_base, room_off, room_xy, n_room_xy, wdo_off, wdo_xy, wdo_type, n_wdo, vanishing_deg,
    # n_panos, out_rows, out_axis, out_floors, status, stream
    lib.salve_pose_graph_axis_align.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int64, vp, i32, vp, vp, vp,
                                                vp, vp]
    lib.salve_pose_graph_axis_align.restype = ctypes.c_int
    lib.salve_conv_f32_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc), i32]
    lib.salve_conv_f32_workspace_bytes.restype = sz
    lib.salve_conv_bf16_workspace_bytes.argtypes = [ctypes.POINTER(ConvDesc), i32]
    lib.salve_conv_bf16_workspace_bytes.restype = sz
    for name in ("salve_conv_f32_forward", "salve_conv_f32_backward_data", "salve_conv_f32_backward_weight", "salve_conv_bf16_forward",
                 "salve_conv_bf16_backward_data", "salve_conv_bf16_backward_weight"):
        getattr(lib, name).argtypes = [ctypes.POINTER(ConvDesc), vp, vp, vp, vp, sz, vp]
        getattr(lib, name).restype = ctypes.c_int
    lib.salve_bn_workspace_bytes.argtypes = [ctypes.POINTER(BnDesc), i32]
    lib.salve_bn_workspace_bytes.restype = sz
    for name in ("salve_bn_f32_forward", "salve_bn_bf16_forward"):   # d, x, residual, gamma, beta, running_mean, running_var, y, save_mean, save_invstd
        getattr(lib, name).argtypes = [ctypes.POINTER(BnDesc)] + [vp] * 9 + [vp, sz, vp]
        getattr(lib, name).restype = ctypes.c_int
    for name in ("salve_bn_f32_backward", "salve_bn_bf16_backward"):   # d, dy, x, y, gamma, save_mean, save_invstd, dx, dres, dgamma, dbeta
        getattr(lib, name).argtypes = [ctypes.POINTER(BnDesc)] + [vp] * 10 + [vp, sz, vp]
        getattr(lib, name).restype = ctypes.c_int
    for t in ("f32", "bf16"):   # the split entries (SyncBatchNormHipFunction)
        getattr(lib, f"salve_bn_{t}_stats").argtypes = [ctypes.POINTER(BnDesc), vp, vp, vp, sz, vp]   # d, x, partial
        getattr(lib, f"salve_bn_{t}_apply").argtypes = [ctypes.POINTER(BnDesc)] + [vp] * 7 + [vp]   # d, x, residual, gamma, beta, mean, invstd, y
        getattr(lib, f"salve_bn_{t}_backward_reduce").argtypes = [ctypes.POINTER(BnDesc)] + [vp] * 6 + [vp, sz, vp]   # d, dy, x, y, mean, invstd, sums
        # d, dy, x, y, gamma, mean, invstd, sums, world, total_rows, dx, dres
        getattr(lib, f"salve_bn_{t}_backward_apply").argtypes = [ctypes.POINTER(BnDesc)] + [vp] * 7 + [i32, ctypes.c_int64, vp, vp, vp]
        for e in ("stats", "apply", "backward_reduce", "backward_apply"):
            getattr(lib, f"salve_bn_{t}_{e}").restype = ctypes.c_int
    lib.salve_bn_combine.argtypes = [ctypes.POINTER(BnDesc), vp, vp, i32, vp, vp, vp, vp, vp]   # d, partials, HOST rows, world, running_mean, running_var, mean, invstd
    lib.salve_bn_combine.restype = ctypes.c_int
    lib.salve_adam_step.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    lib.salve_adam_step.restype = ctypes.c_int
    for name in ("salve_flat_pack", "salve_flat_unpack"):   # table, n_segments, chunk_map, n_chunks, HOST table, HOST chunk_map, flat, flat_elems, scale, stream
        getattr(lib, name).argtypes = [vp, i32, vp, i32, vp, vp, vp, ctypes.c_int64, ctypes.c_float, vp]
        getattr(lib, name).restype = ctypes.c_int
    lib.salve_head_workspace_bytes.argtypes = [ctypes.POINTER(HeadDesc), i32]
    lib.salve_head_workspace_bytes.restype = sz
    for name in ("salve_head_f32_forward", "salve_head_bf16_forward"):   # d, x, weight, bias, target, pooled, logits, probs, loss, meter
        getattr(lib, name).argtypes = [ctypes.POINTER(HeadDesc)] + [vp] * 9 + [vp, sz, vp]
        getattr(lib, name).restype = ctypes.c_int
    for name in ("salve_head_f32_backward", "salve_head_bf16_backward"):   # d, pooled, probs, target, weight, grad_loss, dlogits, dw, db, dx
        getattr(lib, name).argtypes = [ctypes.POINTER(HeadDesc)] + [vp] * 9 + [vp, sz, vp]
        getattr(lib, name).restype = ctypes.c_int
    lib.salve_bev_jpeg_roundtrip_workspace_bytes.argtypes = [i32, i32, i32]
    lib.salve_bev_jpeg_roundtrip_workspace_bytes.restype = sz
    lib.salve_bev_jpeg_roundtrip.argtypes = [vp, vp, i32, i32, i32, vp, vp, sz, vp]   # bev_in, bev_out, n, h, w, HOST qtab, ws, ws_bytes, stream
    lib.salve_bev_jpeg_roundtrip.restype = ctypes.c_int
    lib.salve_bev_jpeg_encode_workspace_bytes.argtypes = [i32, i32, i32]
    lib.salve_bev_jpeg_encode_workspace_bytes.restype = sz
    lib.salve_bev_jpeg_encode_max_bytes.argtypes = [i32, i32]
    lib.salve_bev_jpeg_encode_max_bytes.restype = sz
    lib.salve_bev_jpeg_encode.argtypes = [vp, i32, i32, i32, vp, vp, sz, vp, vp, sz, vp]   # bev, n, h, w, HOST qtab, scan, scan_stride, scan_bytes, ws, ws_bytes, stream
    lib.salve_bev_jpeg_encode.restype = ctypes.c_int
    lib.salve_bev_jpeg_decode_workspace_bytes.argtypes = [i32, i32, i32]
    lib.salve_bev_jpeg_decode_workspace_bytes.restype = sz
    # scans, scans_size, scan_offset, scan_bytes, n, h, w, HOST qtab, HOST huffman, bev_out, image_status, ws, ws_bytes, stages, stream
    lib.salve_bev_jpeg_decode.argtypes = [vp, sz, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp]
    lib.salve_bev_jpeg_decode.restype = ctypes.c_int
    lib.salve_bev_jpeg_decode_lanes_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.salve_bev_jpeg_decode_lanes_workspace_bytes.restype = sz
    lib.salve_bev_jpeg_subseq_bytes.argtypes = []
    lib.salve_bev_jpeg_subseq_bytes.restype = i32
    lib.salve_bev_jpeg_decode_lanes.argtypes = [vp, sz, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp]
    lib.salve_bev_jpeg_decode_lanes.restype = ctypes.c_int
    # the same four with `sampling`: last in the size queries, behind w in the calls
    lib.salve_bev_jpeg_decode_sampled_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.salve_bev_jpeg_decode_sampled_workspace_bytes.restype = sz
    lib.salve_bev_jpeg_decode_lanes_sampled_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    lib.salve_bev_jpeg_decode_lanes_sampled_workspace_bytes.restype = sz
    lib.salve_bev_jpeg_decode_sampled.argtypes = [vp, sz, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp]
    lib.salve_bev_jpeg_decode_sampled.restype = ctypes.c_int
    lib.salve_bev_jpeg_decode_lanes_sampled.argtypes = [vp, sz, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, ctypes.c_uint32, vp]
    lib.salve_bev_jpeg_decode_lanes_sampled.restype = ctypes.c_int
    # The bindings above are written for ONE ABI: an older or newer library (a stale git-ignored .so, a SALVE_HIP_LIB override
    # built from another revision) would be called with shifted arguments -- device memory corruption instead of an error.
    got = int(lib.salve_hip_version())
    if got != EXPECTED_ABI:
        raise SalveHipError(f"{LIB_PATH} reports ABI version {got}, these bindings are written for {EXPECTED_ABI}: rebuild it "
                            "(python __graft_entry__.py --force)")
    _lib = lib
    return lib


def check_status_word(word: int, what: str) -> None:
    """Raise for a non-zero device status word (include/salve_hip.h: SALVE_STATUS_*)."""
    if word & STATUS_WALK_FAILED:
        raise SalveHipError(f"{what}: a Delaunay star walk did not close; the BEV image of at least one render is incomplete")
    if word & STATUS_FP16_RANGE:
        raise SalveHipError(f"{what}: an activation of the verifier exceeded the fp16 range and was saturated; the logits are "
                            "not those of the fp32 network (a network without trained normalisation statistics does this)")
    if word & STATUS_BAD_HYPOTHESIS:
        raise SalveHipError(f"{what}: a render row names a panorama outside the uploaded batch (or an unknown surface); its image is empty")
    if word & STATUS_LAYOUT_THICKNESS:
        raise SalveHipError(f"{what}: a layout segment of 19 pixels or more was left out (its OpenCV end caps are not implemented)")
    if word & STATUS_BAD_TILE_JOB:
        raise SalveHipError(f"{what}: a train-tile job names another sample, channels or an image outside its arrays (or a draw has unknown "
                            "flag bits, or a jitter record is malformed); that sample was not written -- or a pair-overlap job names an image "
                            "outside its arrays; its row is -1")
    if word & STATUS_BAD_PANO_SLOT:
        raise SalveHipError(f"{what}: a panorama-index update names a slot outside the resident pool; that slot's index was not rebuilt")
    if word & STATUS_BAD_LAYOUT:
        raise SalveHipError(f"{what}: a layout image record names a panorama outside the layout tables or output outside its tables, or a "
                            "posed coordinate lies more than 2^24 pixels away; that layout image is empty")
    if word & STATUS_BAD_GRAPH_ROW:
        raise SalveHipError(f"{what}: a floor's pose-graph rows are not sorted by (i1, i2), name a node outside the floor or have i1 >= i2 (or the "
                            "floor's extents are malformed); that floor was written empty")
    if word & STATUS_BAD_FLOOR_TABLE:
        raise SalveHipError(f"{what}: a floor-report table is malformed (a floor's panorama or hypothesis extent, a room's vertex extent) or a "
                            "posed room vertex is not finite or lies more than 2^24 pixels away; that floor was written empty")
    if word & STATUS_BAD_AXIS_ROW:
        raise SalveHipError(f"{what}: an axis-alignment row names a panorama outside its floor or a W/D/O its panorama does not hold, or a table "
                            "extent is malformed; that row was copied unchanged (a floor with a malformed row extent was not written)")
    if word:
        raise SalveHipError(f"{what}: device status word {word:#x}")


def check(status: int, what: str) -> None:
    if status != SALVE_OK:
        msg = load().salve_last_error().decode("utf-8", "replace")
        raise SalveHipError(f"{what} failed with status {status}: {msg}")
