"""ctypes binding of libpp_hip.so (include/pp_hip.h).  Fails loudly when the HIP
extension is missing: there is no CPU fallback in the product path."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpp_hip.so")
PP_MAX_CLASSES = 12
PP_LOSS_TERMS = 21
PP_ASSIGN_MAX_GT = 4096
PP_AUG_MAX_BOXES = 256
PP_AUG_MAX_TRIES = 128
PP_AUG_PARAMS = 16
PP_GT_CHUNK = 1024
PP_OPT_CHUNK = 2048
PP_OPT_GROUP = 32

c_f = ctypes.c_float
c_i32 = ctypes.c_int32
c_i64 = ctypes.c_int64
c_p = ctypes.c_void_p


class PPConfig(ctypes.Structure):
    _fields_ = [
        ("voxel_size", c_f * 3),
        ("offset", c_f * 3),
        ("grid_size", c_i32 * 3),
        ("max_voxels", c_i32),
        ("max_num_points", c_i32),
        ("num_point_features", c_i32),
        ("max_points", c_i32),
        ("num_anchor_per_loc", c_i32),
        ("num_classes", c_i32),
        ("class_begin", c_i32 * PP_MAX_CLASSES),
        ("class_end", c_i32 * PP_MAX_CLASSES),
        ("center_limit", ctypes.c_double * 6),
        ("norm_kind", c_i32),
        ("nms_pre_max", c_i32),
        ("nms_post_max", c_i32),
        ("nms_iou_threshold", c_f),
        ("score_threshold", c_f),
        ("max_batch", c_i32),
    ]


# name -> (restype, argtypes); must list every symbol include/pp_hip.h declares
PROTOTYPES = {
    "pp_create": (c_p, [ctypes.c_int, ctypes.POINTER(PPConfig)]),
    "pp_destroy": (None, [c_p]),
    "pp_last_error": (ctypes.c_char_p, [c_p]),
    "pp_load_weights": (ctypes.c_int, [c_p, ctypes.c_char_p, c_p, ctypes.POINTER(c_i64), ctypes.c_int]),
    "pp_commit_weights": (ctypes.c_int, [c_p]),
    "pp_set_precision": (ctypes.c_int, [c_p, ctypes.c_int]),
    "pp_effective_precision": (ctypes.c_int, [c_p]),
    "pp_set_anchors": (ctypes.c_int, [c_p, c_p, c_p, c_i64]),
    "pp_voxelize": (ctypes.c_int, [c_p, c_p, ctypes.c_int, ctypes.c_int, c_p, c_p, c_p, c_p, c_p]),
    "pp_anchor_mask": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p]),
    "pp_pfn": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_scatter": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_backbone": (ctypes.c_int, [c_p, c_p, c_p, c_p]),
    "pp_head": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_postprocess": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_int, c_p]),
    "pp_select_candidates": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_infer_frame": (ctypes.c_int, [c_p, c_p, ctypes.c_int, c_p, c_p, ctypes.c_int, c_p]),
    "pp_infer_batch": (ctypes.c_int, [c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p, ctypes.c_int, c_p]),
    "pp_fetch_frame_tensor": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, c_p, c_p]),
    "pp_debug_layer": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, c_p, c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_debug_layer_skip": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, c_p, c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_int, c_p]),
    "pp_debug_head_cls": (ctypes.c_int, [c_p, ctypes.c_int, c_p, ctypes.c_int, c_p, c_p, c_p, c_p]),
    "pp_head_cls_tiling": (ctypes.c_char_p, [c_p]),
    "pp_set_head_defer": (ctypes.c_int, [c_p, ctypes.c_int]),
    "pp_head_defer_active": (ctypes.c_int, [c_p]),
    "pp_set_sparse_conv1": (ctypes.c_int, [c_p, ctypes.c_int]),
    "pp_set_tile_skip": (ctypes.c_int, [c_p, ctypes.c_int]),
    "pp_tile_skip_active": (ctypes.c_int, [c_p]),
    "pp_set_assign_thresholds": (ctypes.c_int, [c_p, c_p, c_p]),
    "pp_assign_targets": (ctypes.c_int, [c_p, c_p, c_p, c_p, ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p, c_p, c_p, c_p]),
    "pp_target_loss": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p]),
    "pp_batch_loss": (ctypes.c_int, [c_p, c_p, c_p, ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p]),
    "pp_target_loss_grad": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_int, ctypes.c_int, c_f, c_p, c_p, c_p, c_p]),
    "pp_head_backward": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_update_head_weights": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_backbone_taps": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_neck_backward": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p, c_p]),
    "pp_update_neck_weights": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p]),
    "pp_unit_backward": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p, c_p]),
    "pp_unit_backward_mp": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p,
                                           c_p]),
    "pp_unit_backward_path": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "pp_backbone_block_taps": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_update_block_weights": (ctypes.c_int, [c_p, ctypes.c_int, c_p, ctypes.c_int, c_p]),
    "pp_down_backward": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p, c_p]),
    "pp_down_backward_mp": (ctypes.c_int, [c_p] + [ctypes.c_int] * 5 + [c_p] * 4 + [ctypes.c_int, c_p, c_p, c_p]),
    "pp_down_backward_path": (ctypes.c_int, [c_p] + [ctypes.c_int] * 5),
    "pp_neck_backward_mp": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p, c_p]),
    "pp_neck_backward_path": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int]),
    "pp_backbone_stage_taps": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_update_down_weight": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p]),
    "pp_backbone_train_taps": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_update_rpn_weights": (ctypes.c_int, [c_p, c_p, c_p]),
    "pp_backbone_train_taps_mp": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_update_rpn_weights_mp": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p]),
    "pp_update_neck_weights_mp": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p, c_p, c_p]),
    "pp_update_head_weights_mp": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_debug_image16": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p, c_p, c_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), c_p]),
    "pp_unit_backward_affine": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p, c_p,
                                               c_p, c_p]),
    "pp_down_backward_affine": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_int,
                                               c_p, c_p, c_p, c_p, c_p]),
    "pp_neck_backward_affine": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p]),
    "pp_bn_fold": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_bn_affine_grad": (ctypes.c_int, [c_p, ctypes.c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pp_update_bn_fold": (ctypes.c_int, [c_p, c_p, c_p]),
    "pp_backbone_train_taps_bn": (ctypes.c_int, [c_p, c_p, ctypes.c_int] + [c_p] * 12),
    "pp_unit_backward_bn": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [c_p] * 8 + [ctypes.c_int] + [c_p] * 4 + [ctypes.c_int, c_p]),
    "pp_down_backward_bn": (ctypes.c_int, [c_p] + [ctypes.c_int] * 4 + [c_p] * 8 + [ctypes.c_int] + [c_p] * 4 + [ctypes.c_int, c_p]),
    "pp_neck_backward_bn": (ctypes.c_int, [c_p, ctypes.c_int] + [c_p] * 8 + [ctypes.c_int] + [c_p] * 4 + [ctypes.c_int, c_p]),
    # the six BatchNorm backwards with `int mode` behind the context (their fp32 siblings' lists otherwise), and their path queries
    "pp_unit_backward_affine_mp": (ctypes.c_int, [c_p] + [ctypes.c_int] * 4 + [c_p] * 6 + [ctypes.c_int] + [c_p] * 5),
    "pp_down_backward_affine_mp": (ctypes.c_int, [c_p] + [ctypes.c_int] * 5 + [c_p] * 6 + [ctypes.c_int] + [c_p] * 5),
    "pp_neck_backward_affine_mp": (ctypes.c_int, [c_p] + [ctypes.c_int] * 2 + [c_p] * 6 + [ctypes.c_int] + [c_p] * 5),
    "pp_unit_backward_bn_mp": (ctypes.c_int, [c_p] + [ctypes.c_int] * 4 + [c_p] * 8 + [ctypes.c_int] + [c_p] * 4 + [ctypes.c_int, c_p]),
    "pp_down_backward_bn_mp": (ctypes.c_int, [c_p] + [ctypes.c_int] * 5 + [c_p] * 8 + [ctypes.c_int] + [c_p] * 4 + [ctypes.c_int, c_p]),
    "pp_neck_backward_bn_mp": (ctypes.c_int, [c_p] + [ctypes.c_int] * 2 + [c_p] * 8 + [ctypes.c_int] + [c_p] * 4 + [ctypes.c_int, c_p]),
    "pp_unit_backward_bn_path": (ctypes.c_int, [c_p] + [ctypes.c_int] * 4),
    "pp_down_backward_bn_path": (ctypes.c_int, [c_p] + [ctypes.c_int] * 5),
    "pp_neck_backward_bn_path": (ctypes.c_int, [c_p] + [ctypes.c_int] * 2),
    "pp_set_train_chunk_frames": (ctypes.c_int, [c_p, ctypes.c_int]),
    "pp_pfn_train_forward": (ctypes.c_int, [c_p] * 12),
    "pp_scatter_backward": (ctypes.c_int, [c_p] * 6),
    "pp_pfn_backward": (ctypes.c_int, [c_p] * 15),
    "pp_update_pfn_weights": (ctypes.c_int, [c_p] * 7),
    "pp_grad_norm": (ctypes.c_int, [c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_i64), ctypes.c_int, c_f, c_p, c_p]),
    "pp_scale_grads": (ctypes.c_int, [c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_i64), ctypes.c_int, c_p, c_p]),
    "pp_adam_step": (ctypes.c_int, [c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p), ctypes.POINTER(c_p), ctypes.POINTER(c_p), ctypes.POINTER(c_i64),
                                    ctypes.c_int, c_i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_int, c_p, c_p]),
    "pp_augment_draw": (ctypes.c_int, [c_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(c_i64), ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p, c_p, c_p, c_p]),
    "pp_augment_noise": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, ctypes.c_int, ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p, c_p, c_p]),
    "pp_augment_boxes": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p, c_p, c_p, c_p]),
    "pp_augment_points": (ctypes.c_int, [c_p, c_p, c_p, ctypes.POINTER(c_i32), c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_i32), ctypes.c_int,
                                         c_p, c_p]),
    "pp_gt_count": (ctypes.c_int, [c_p, c_p, ctypes.POINTER(c_i32), c_p, ctypes.POINTER(c_i32), ctypes.c_int, ctypes.POINTER(c_f), c_p, c_p]),
    "pp_gt_extract": (ctypes.c_int, [c_p, c_p, ctypes.POINTER(c_i32), c_p, ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_i64, c_p, c_p]),
    "pp_gt_select": (ctypes.c_int, [c_p, c_p, ctypes.POINTER(c_i32), c_p, ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p]),
    "pp_gt_paste_count": (ctypes.c_int, [c_p, c_p, ctypes.POINTER(c_i32), c_p, c_p, c_p, ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_i64, c_i64,
                                         ctypes.c_int, c_p, c_p, c_p]),
    "pp_gt_paste": (ctypes.c_int, [c_p, c_p, ctypes.POINTER(c_i32), c_p, c_p, c_p, ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p, c_i64, c_i64,
                                   ctypes.c_int, c_p, ctypes.POINTER(c_i32), c_p, c_p]),
    "pp_gt_draw": (ctypes.c_int, [c_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(c_i64), ctypes.POINTER(c_i32), ctypes.c_int,
                                  ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), ctypes.c_int, c_p, c_p]),
    "pp_box_decode": (ctypes.c_int, [c_p, c_p, c_p, c_i64, c_p]),
    "pp_corners2d": (ctypes.c_int, [c_p, c_p, c_p, c_p, c_i64, c_p]),
    "pp_standup2d": (ctypes.c_int, [c_p, c_p, c_i64, c_p]),
    "pp_nms": (ctypes.c_int, [c_p, ctypes.c_int, ctypes.c_int, c_f, c_p, c_p, ctypes.c_int, c_p]),
    "pp_rotated_iou": (ctypes.c_int, [c_p, c_p, c_p, ctypes.c_int, ctypes.c_int, c_p]),
    "pp_unpack_points": (ctypes.c_int, [c_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, c_p, c_p, ctypes.c_int, c_p, c_p]),
    "pp_rotated_iou_eval": (ctypes.c_int, [c_p, c_p, c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_p]),
    "pp_eval_statistics": (ctypes.c_int, [c_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_p, c_p, c_p, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_int, c_p, c_p, c_p]),
    "pp_eval_fused_statistics": (ctypes.c_int, [c_p, ctypes.c_int64, c_p, c_p, c_p, ctypes.c_int, c_p, c_p, c_p, ctypes.c_double, c_p,
                                                ctypes.c_int]),
    "pp_eval_class_ap": (ctypes.c_int, [ctypes.POINTER(c_p), c_p, ctypes.c_int, c_p, c_p, c_i64, c_p, c_p, c_p, ctypes.c_double, c_i64, ctypes.c_int,
                                        c_p, c_p]),
    "pp_profile_begin": (ctypes.c_int, [c_p]),
    "pp_profile_end": (ctypes.c_int, [c_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i32), ctypes.POINTER(ctypes.c_double)]),
    "pp_dominant_kernel": (ctypes.c_char_p, [c_p]),
    "pp_dominant_executed_ratio": (ctypes.c_double, [c_p]),
    "pp_stage_profile_begin": (ctypes.c_int, [c_p]),
    "pp_stage_profile_end": (ctypes.c_int, [c_p, ctypes.POINTER(ctypes.c_double)]),
    "pp_layer_tilings": (ctypes.c_int, [c_p, ctypes.c_char_p, ctypes.c_int]),
    "pp_weight_image": (ctypes.c_int, [c_p, ctypes.c_int, c_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), c_p]),
    "pp_tune_export": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "pp_tune_import": (ctypes.c_int, [ctypes.c_char_p]),
    "pp_menu_names": (ctypes.c_int, [ctypes.c_int] * 12 + [ctypes.c_char_p, ctypes.c_int]),
    "pp_version": (ctypes.c_int, []),
}

_lib = None


def load():
    """Load libpp_hip.so; raise (never fall back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C 3d_object_detection_amd/csrc)")
        # torch first: its wheel bundles the HIP runtime as lib/libamdhip64.so (SONAME libamdhip64.so.7), which then also
        # satisfies libpp_hip.so's NEEDED libamdhip64.so.7 -- ONE runtime per process.  Loaded the other way round,
        # libpp_hip.so pulls /opt/rocm's copy, torch still loads its own (its NEEDED entry is the unversioned file name),
        # and with two HIP runtimes in the process the first HIP call fails with "no ROCm-capable device is detected".
        import torch  # noqa: F401
        lib = ctypes.CDLL(os.environ.get("PP_HIP_LIB", LIB_PATH))  # PP_HIP_LIB: developer override (diagnostic builds)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)  # AttributeError if the .so is stale: loud by design
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, ctx=None, what=""):
    if rc != 0:
        msg = load().pp_last_error(ctx)
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
