"""ctypes binding of libs2anet_hip.so (C ABI declared in include/s2anet_hip.h).

PyTorch is used here only as plumbing: device memory (tensors own the buffers and the
caching allocator provides the workspaces) and the current HIP stream.
"""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("S2A_LIB_PATH") or os.path.join(_HERE, "libs2anet_hip.so")   # override: A/B builds

OK, EINVAL, EWORKSPACE, EHIP, ENOTIMPL = 0, -1, -2, -3, -4
DTYPE_F32, DTYPE_F16, DTYPE_F64 = 0, 1, 2
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1

c_i64, c_int, c_f32, c_sz, c_vp = (ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t,
                                   ctypes.c_void_p)


class DcnParams(ctypes.Structure):
    _fields_ = [("batch", c_i64), ("channels", c_i64), ("height", c_i64), ("width", c_i64),
                ("out_channels", c_i64),
                ("kW", c_int), ("kH", c_int), ("dW", c_int), ("dH", c_int), ("padW", c_int),
                ("padH", c_int), ("dilationW", c_int), ("dilationH", c_int), ("group", c_int),
                ("deformable_group", c_int), ("dtype", c_int), ("offset_dtype", c_int),
                ("layout", c_int), ("relu", c_int)]


class AlignParams(ctypes.Structure):
    _fields_ = [("batch", c_i64), ("channels", c_i64), ("height", c_i64), ("width", c_i64),
                ("out_channels", c_i64), ("stride", c_f32), ("dtype", c_int), ("layout", c_int),
                ("relu", c_int), ("weight_packed", c_int)]


class Pyramid(ctypes.Structure):
    """s2a_pyramid: FPN level table of a pyramid-packed buffer"""
    _fields_ = [("n_levels", ctypes.c_int32), ("height", ctypes.c_int32 * 8), ("width", ctypes.c_int32 * 8),
                ("stride", c_f32 * 8)]


LOSS_MAX_LEVELS = 8


class LossMap(ctypes.Structure):
    """s2a_loss_map: one (module, level) of the training loss"""
    _fields_ = [("cls", c_vp), ("bbox", c_vp), ("anchors", c_vp), ("grad_cls", c_vp), ("grad_bbox", c_vp),
                ("anchor_batch_stride", c_i64), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("cls_dtype", ctypes.c_int32), ("bbox_dtype", ctypes.c_int32), ("fpn_balance", c_f32),
                ("reserved", ctypes.c_int32)]


class LossParams(ctypes.Structure):
    """s2a_loss_params"""
    _fields_ = [("batch", ctypes.c_int32), ("num_classes", ctypes.c_int32), ("n_levels", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("fl_gamma", c_f32), ("fl_alpha", c_f32), ("smooth_l1_beta", c_f32),
                ("reg_balance", c_f32), ("odm_balance", c_f32), ("map", (LossMap * LOSS_MAX_LEVELS) * 2)]


class LossGradMap(ctypes.Structure):
    """s2a_loss_grad_map"""
    _fields_ = [("src", c_vp), ("dst", c_vp), ("numel", c_i64), ("dtype", ctypes.c_int32), ("norm_index", ctypes.c_int32)]


class EvalCurves(ctypes.Structure):
    """s2a_eval_curves: optional per-position outputs of s2a_eval_task1 (NULL members are not written)"""
    _fields_ = [("order", c_vp), ("ovmax", c_vp), ("argmax", c_vp), ("tp_cum", c_vp), ("fp_cum", c_vp), ("rec", c_vp),
                ("prec", c_vp), ("seg_start", c_vp)]


class OptimTensor(ctypes.Structure):
    """s2a_optim_tensor: one row of the training update's device tensor table"""
    _fields_ = [("p", c_vp), ("grad", c_vp), ("momentum_buf", c_vp), ("ema", c_vp), ("numel", c_i64),
                ("group", ctypes.c_int32), ("kind", ctypes.c_int32)]


class TrainUpdateArgs(ctypes.Structure):
    """s2a_train_update_args"""
    _fields_ = [("tensors", c_vp), ("chunks", c_vp), ("n_tensors", c_i64), ("n_chunks", c_i64), ("n_trained_chunks", c_i64),
                ("lr", c_vp), ("hyper", c_vp), ("n_groups", ctypes.c_int32), ("scaling_enabled", ctypes.c_int32),
                ("scale", c_vp), ("counters", c_vp), ("skip", c_vp), ("skip_elem_bytes", ctypes.c_int32),
                ("growth_interval", ctypes.c_int32), ("max_norm", c_f32), ("growth_factor", c_f32),
                ("backoff_factor", c_f32), ("reserved", c_f32), ("ema_decay", ctypes.c_double), ("ema_tau", ctypes.c_double),
                ("stats", c_vp)]


OPTIM_CHUNK, OPTIM_STATS, OPTIM_TRAINED, OPTIM_EMA_ONLY = 4096, 8, 0, 1


class AnchorSet(ctypes.Structure):
    """s2a_anchor_set: one anchor set of s2a_assign_labels_batched"""
    _fields_ = [("anchors", c_vp), ("batch_stride", c_i64)]


# every symbol include/s2anet_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "s2a_last_error": (ctypes.c_char_p, []),
    "s2a_version": (ctypes.c_char_p, []),
    "s2a_set_deterministic": (c_int, [c_int]),
    "s2a_get_deterministic": (c_int, []),
    "s2a_box_iou_rotated_workspace_bytes": (c_sz, [c_i64, c_i64]),
    "s2a_box_iou_rotated": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_sz, c_vp]),
    "s2a_box_iou_rotated_pairs": (c_int, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "s2a_polyiou_pairs": (c_int, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "s2a_polyiou_match": (c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "s2a_assign_labels_workspace_bytes": (c_sz, [c_i64, c_i64]),
    "s2a_assign_labels": (c_int, [c_vp, c_i64, c_vp, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, c_int, c_int, c_int,
                                  c_vp, c_vp, c_sz, c_vp]),
    "s2a_assign_labels_batched_workspace_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i64]),
    "s2a_assign_labels_batched": (c_int, [ctypes.POINTER(AnchorSet), c_int, c_i64, c_i64, c_vp, c_i64, c_vp, c_f32, c_f32,
                                          c_f32, c_f32, c_f32, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp,
                                          c_sz, c_vp]),
    "s2a_nms_poly_workspace_bytes": (c_sz, [c_i64]),
    "s2a_nms_poly": (c_int, [c_vp, c_i64, ctypes.c_double, c_vp, c_vp, ctypes.POINTER(c_i64), c_vp, c_sz, c_vp]),
    "s2a_nms_rotated_workspace_bytes": (c_sz, [c_i64, c_i64]),
    "s2a_ml_nms_rotated": (c_int, [c_vp, c_vp, c_vp, c_i64, c_f32, c_vp, c_vp,
                                   ctypes.POINTER(c_i64), c_vp, c_sz, c_vp]),
    "s2a_nms_rotated": (c_int, [c_vp, c_vp, c_i64, c_f32, c_vp, c_vp, ctypes.POINTER(c_i64), c_vp,
                                c_sz, c_vp]),
    "s2a_nms_rotated_f64_workspace_bytes": (c_sz, [c_i64]),
    "s2a_nms_rotated_f64": (c_int, [c_vp, c_vp, c_vp, c_i64, c_f32, c_vp, c_vp, ctypes.POINTER(c_i64), c_vp, c_sz, c_vp]),
    "s2a_nms_rotated_segmented": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, ctypes.c_int32,
                                          ctypes.c_int32, c_f32, c_vp, c_vp, c_vp, ctypes.c_int32,
                                          c_vp, c_sz, c_vp]),
    "s2a_nms_rotated_segmented_dets": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, ctypes.c_int32, ctypes.c_int32, c_f32,
                                               ctypes.c_int32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "s2a_multiclass_candidates_workspace_bytes": (c_sz, [c_i64]),
    "s2a_multiclass_candidates": (c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_f32, c_i64, c_vp, c_vp, c_vp,
                                          c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "s2a_arf_forward": (c_int, [c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_int, c_int, c_vp,
                                c_vp]),
    "s2a_arf_backward": (c_int, [c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "s2a_modulated_deform_conv_forward": (c_int, [c_vp] * 6 + [ctypes.POINTER(DcnParams), c_vp]),
    "s2a_rie_forward": (c_int, [c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_vp, c_vp]),
    "s2a_rie_backward": (c_int, [c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp, c_vp]),
    "s2a_rot_inv_pool": (c_int, [c_vp, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_vp, c_vp]),
    "s2a_rot_inv_pool_backward": (c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_vp, c_vp]),
    "s2a_s2anet_loss_workspace_bytes": (c_sz, [c_i64, c_i64]),
    "s2a_s2anet_loss_forward": (c_int, [ctypes.POINTER(LossParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "s2a_s2anet_loss_backward": (c_int, [ctypes.POINTER(LossGradMap), c_int, c_vp, c_vp, c_vp]),
    "s2a_deform_conv_workspace_bytes": (c_sz, [ctypes.POINTER(DcnParams)]),
    "s2a_deform_conv_forward": (c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(DcnParams), c_vp,
                                        c_sz, c_vp]),
    "s2a_align_offsets": (c_int, [c_vp, c_i64, c_i64, c_i64, c_f32, c_int, c_vp, c_vp]),
    "s2a_align_conv_workspace_bytes": (c_sz, [ctypes.POINTER(AlignParams)]),
    "s2a_align_conv_forward": (c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(AlignParams), c_vp,
                                       c_sz, c_vp]),
    "s2a_dcn_packed_elems": (c_i64, [c_i64, c_i64, c_int]),
    "s2a_nms_small_stats": (c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "s2a_dcn_pack_weight": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    "s2a_bias_act_nhwc": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp]),
    "s2a_bias_act_nhwc_to": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_int, c_vp]),
    "s2a_conv_pack_weight_f16": (c_int, [c_vp, c_i64, c_i64, c_int, c_vp, c_vp]),
    "s2a_conv_nhwc_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_int,
                                  c_int, c_vp]),
    "s2a_conv_nhwc_f16_form": (c_int, [c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_int, ctypes.POINTER(ctypes.c_int32)]),
    "s2a_conv_pack_weight_train": (c_int, [c_vp, c_int, c_i64, c_i64, c_int, c_vp, c_vp, c_vp]),
    "s2a_conv_backward_prep_f16_workspace_bytes": (c_sz, [c_i64, c_i64]),
    "s2a_conv_backward_prep_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_i64, c_i64, c_vp, c_sz, c_vp]),
    "s2a_conv_backward_weight_f16_workspace_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i64, c_int]),
    "s2a_conv_backward_weight_f16": (c_int, [c_vp, c_vp, c_vp, c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_vp, c_sz,
                                             c_vp]),
    "s2a_conv_backward_input_s2_f16": (c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_vp]),
    "s2a_conv_backward_weight_s2_slices": (c_int, [c_i64, c_i64, c_i64, c_i64, c_i64, c_int]),
    "s2a_conv_backward_weight_s2_f16": (c_int, [c_vp, c_vp, c_vp, c_int, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_vp]),
    "s2a_conv_backward_weight_s2_reduce": (c_int, [c_vp, c_int, c_i64, c_vp, c_int, c_vp]),
    "s2a_debug_read_stamps": (c_int, [c_vp, c_i64]),
    "s2a_build_flags": (c_int, []),
    "s2a_deform_conv_backward_input_workspace_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i64]),
    "s2a_deform_conv_backward_weight_workspace_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i64]),
    "s2a_deform_conv_backward_workspace_bytes": (c_sz, [c_int, c_i64, c_i64, c_i64, c_i64, c_i64]),
    "s2a_deform_conv_backward": (c_int, [c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_i64, c_i64, c_i64, c_i64,
                                         c_i64, c_vp, c_sz, c_vp]),
    "s2a_deform_conv_backward_typed": (c_int, [c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, c_i64, c_i64, c_i64, c_i64,
                                               c_i64, c_vp, c_sz, c_vp]),
    "s2a_deform_conv_backward_input_f32_workspace_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i64]),
    "s2a_deform_conv_backward_weight_f32_workspace_bytes": (c_sz, [c_i64, c_i64, c_i64, c_i64, c_i64]),
    "s2a_deform_conv_backward_weight_f32": (c_int, [c_vp, c_vp, c_vp, c_vp, c_f32, c_i64, c_i64, c_i64, c_i64, c_i64,
                                                    c_vp, c_sz, c_vp]),
    "s2a_deform_conv_backward_input_f32": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64,
                                                   c_vp, c_sz, c_vp]),
    "s2a_deform_conv_backward_weight_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_sz, c_vp]),
    "s2a_deform_conv_backward_input_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64,
                                           c_vp, c_sz, c_vp]),
    "s2a_deformable_im2col": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(DcnParams), c_vp]),
    "s2a_deformable_col2im": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(DcnParams), c_vp]),
    "s2a_deformable_col2im_coord": (c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(DcnParams), c_vp]),
    "s2a_conv3x3_tail1x1_f16": (c_int, [c_vp] * 10 + [c_i64] * 7 + [c_vp]),
    "s2a_conv1x1_chain_f16": (c_int, [c_vp] * 8 + [c_i64] * 6 + [c_vp]),
    "s2a_conv1x1_add_up2_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp]),
    "s2a_sum_pool2x2_f16": (c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_i64, c_vp]),
    "s2a_pyramid_pixels": (c_i64, [ctypes.POINTER(Pyramid), c_i64]),
    "s2a_conv3x3_pyramid_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_int,
                                        ctypes.POINTER(Pyramid), c_vp]),
    "s2a_conv3x3_head_pyramid_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_int,
                                             ctypes.POINTER(Pyramid), c_vp]),
    "s2a_conv3x3_narrow_pyramid_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_int, ctypes.POINTER(Pyramid), c_vp]),
    "s2a_orconv_pool_pyramid_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, ctypes.POINTER(Pyramid), c_vp]),
    "s2a_conv_wino_packed_elems": (c_i64, [c_i64, c_i64]),
    "s2a_conv_wino_pack_weight_f16": (c_int, [c_vp, c_i64, c_i64, c_vp, c_vp]),
    "s2a_conv3x3_wino_pyramid_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_int,
                                             ctypes.POINTER(Pyramid), c_vp]),
    "s2a_quantize_e4m3": (c_int, [c_vp, c_vp, c_i64, c_i64, c_f32, c_vp]),
    "s2a_conv_pack_weight_fp8": (c_int, [c_vp, c_i64, c_i64, c_vp, c_vp]),
    "s2a_conv3x3_pyramid_fp8": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_f32, c_i64, c_i64, c_i64, c_int,
                                        ctypes.POINTER(Pyramid), c_vp]),
    "s2a_align_conv_pyramid_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_int,
                                           ctypes.POINTER(Pyramid), c_vp]),
    "s2a_fam_refine_anchors_pyramid": (c_int, [c_vp, c_i64, c_i64, ctypes.POINTER(Pyramid), c_f32, c_vp, c_vp]),
    "s2a_stem_packed_elems": (c_i64, []),
    "s2a_stem_pack_weight_f16": (c_int, [c_vp, c_vp, c_vp]),
    "s2a_stem_u8_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_f32, c_vp]),
    "s2a_stem_u8_f16_train": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_f32, c_vp]),
    "s2a_stem_backward_slices": (c_int, [c_i64, c_i64, c_i64]),
    "s2a_stem_backward_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_i64, c_i64, c_i64, c_f32, c_vp]),
    "s2a_pyramid_candidates_count": (c_i64, [ctypes.POINTER(Pyramid), c_i64]),
    "s2a_pyramid_candidates": (c_int, [c_vp, c_vp, c_vp, c_i64, ctypes.POINTER(Pyramid), c_int, c_i64, c_f32, c_vp, c_vp, c_vp, c_vp]),
    "s2a_rbox_to_poly": (c_int, [c_vp, c_i64, c_i64, c_vp, c_vp]),
    "s2a_scene_gather_u8": (c_int, [c_vp, c_i64, c_i64, c_vp, c_i64, ctypes.c_int32, c_vp, c_vp]),
    "s2a_scene_merge_workspace_bytes": (c_sz, [c_i64, c_i64]),
    "s2a_scene_merge": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, ctypes.c_int32, ctypes.c_double, c_i64,
                                c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "s2a_eval_task1_workspace_bytes": (c_sz, [c_i64, c_i64, ctypes.c_int32, ctypes.c_int32]),
    "s2a_eval_task1": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, ctypes.c_int32, ctypes.c_int32,
                               ctypes.c_double, c_int, c_int, ctypes.POINTER(ctypes.c_double)] + [c_vp] * 9 +
                       [ctypes.POINTER(EvalCurves), c_vp, c_sz, c_vp]),
    "s2a_train_update_workspace_bytes": (c_sz, [c_i64]),
    "s2a_train_update": (c_int, [ctypes.POINTER(TrainUpdateArgs), c_vp, c_sz, c_vp]),
    "s2a_augment_draw": (c_int, [c_vp, c_vp, c_i64, c_int, c_f32, c_f32, c_vp, c_vp]),
    "s2a_augment_images_u8": (c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp]),
    "s2a_augment_labels": (c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i64, c_int, c_vp, c_vp, c_vp]),
    "s2a_bn_slices": (c_int, [c_i64, c_i64]),
    "s2a_bn_train_stats_f16": (c_int, [c_vp, c_i64, c_i64, ctypes.c_double, ctypes.c_double, c_vp, c_int, c_vp, c_vp, c_vp, c_vp,
                                       c_int, c_vp]),
    "s2a_bn_train_apply_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_i64, c_int, c_vp]),
    "s2a_bn_backward_reduce_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_vp, c_i64, c_i64,
                                           c_vp]),
    "s2a_bn_backward_input_f16": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_i64, c_vp]),
    "s2a_delta2bbox_rotated": (c_int, [c_vp, c_vp, c_i64, c_f32, c_vp, c_vp]),
    "s2a_fam_refine_anchors": (c_int, [c_vp, c_i64, c_i64, c_i64, c_f32, c_f32, c_int, c_int,
                                       c_vp, c_vp]),
}


def build(force=False):
    """compile libs2anet_hip.so in-tree (hipcc --offload-arch=gfx950)"""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "-s", "clean"])
    subprocess.check_call(["make", "-C", csrc, "-s", "-j4"])
    return LIB_PATH


_lib = None


def lib():
    """the loaded library; raises (never falls back) when it is missing"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` or `make -C s2anet_amd/csrc` — s2anet_amd has no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        flags = L.s2a_build_flags()
        if flags and not os.environ.get("S2A_ALLOW_MEASURE_BUILD"):
            raise RuntimeError(
                f"{LIB_PATH} holds an object compiled with a measurement / ablation switch (s2a_build_flags() = {flags:#x}): "
                "rebuild with `make -C s2anet_amd/csrc` (scripts that build such objects set S2A_ALLOW_MEASURE_BUILD=1)")
        _lib = L
    return _lib


class _ModeGuard:
    """what deterministic(on) returns: the previous value, and a context manager that puts it back"""

    def __init__(self, previous):
        self.previous = bool(previous)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        lib().s2a_set_deterministic(int(self.previous))
        return False

    def __repr__(self):
        return f"<deterministic: was {self.previous}>"


def deterministic(on=None):
    """deterministic training mode of the library (s2a_set_deterministic; initial value: S2A_DETERMINISTIC).
    deterministic() -> bool, the current value.  deterministic(on) sets it at once and returns a guard holding `.previous`;
    `with deterministic(True): ...` restores the previous value on the way out, also after an exception.  The flag is read
    when a call is issued: a captured graph keeps the mode it was captured in."""
    if on is None:
        return bool(lib().s2a_get_deterministic())
    return _ModeGuard(lib().s2a_set_deterministic(int(bool(on))))


def check(rc):
    if rc != OK:
        msg = lib().s2a_last_error().decode("utf-8", "replace")
        if rc == ENOTIMPL:
            raise NotImplementedError(msg)
        raise RuntimeError(f"s2anet_hip error {rc}: {msg}")


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            # reference: DeformConvFunction raises NotImplementedError on CPU tensors
            # (models/dcn/deform_conv.py:58-59); the product has no CPU path at all
            raise NotImplementedError("s2anet_amd ops run on the GPU only (got a CPU tensor)")


def dtype_code(t, f64=False):
    """f64=True: entry points with a float64 instantiation (deformable convolution generic path, ARF)"""
    if t.dtype == torch.float32:
        return DTYPE_F32
    if t.dtype == torch.float16:
        return DTYPE_F16
    if f64 and t.dtype == torch.float64:
        return DTYPE_F64
    raise TypeError(f"unsupported dtype {t.dtype} (float32 / float16{' / float64' if f64 else ''} only)")


_ws_cache = {}


def workspace(nbytes, device, tag="ws"):
    """grow-only per-(device, stream, tag) scratch buffer from the torch caching allocator"""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 16), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf
