"""s2anet_amd — MI355X-native (gfx950) dense-inference hot path of S2ANet.

Host-side mirror of the reference's operator surface over the C-ABI
library ``libs2anet_hip.so`` (include/s2anet_hip.h).  There is NO CPU fallback: every op
raises if the HIP library is missing or a tensor is not on the GPU.
"""
from . import _lib  # noqa: F401
from ._lib import deterministic
from .rotated import (box_iou_rotated, nms_rotated, ml_nms_rotated, multiclass_nms_rotated,
                      batched_multiclass_nms_rotated, assign_labels, assign_labels_batched)
from .orn import arf_forward, arf_backward, active_rotating_filter, ORConv2d, RotationInvariantPooling
from .dcn import DeformConv, DeformConvFunction, deform_conv, deform_conv_forward_cuda
from .alignconv import AlignConv, AlignConvFunction, align_conv
from .orn import RotInvPoolFunction, rot_inv_pool, rot_inv_pool_backward
from .loss import S2ANetLossFunction, s2anet_loss, grid_anchors
from .fused import drop_weight_caches, train_kernels, train_conv_ok, train_conv_strided_ok, FusedConv2d, FusedConvFunction, \
    StemU8Function, FusedConvUp2Function, train_up2_ok
from .scene import tile_grid, chip_names, gather_chips, merge_detections, SceneDetections
from .evaluate import evaluate_task1, Task1Evaluator, Task1Result, claim_tp_fp
from .optim import TrainUpdate, reference_param_groups, reference_lr
from .fp8 import quantize_weight_e4m3, calibrate_fp8, fp8_towers
from .augment import TrainAugment
from .norm import BatchNormTrainFunction, batch_norm_train, train_bn_ok, train_batchnorm

__all__ = [
    "box_iou_rotated", "nms_rotated", "ml_nms_rotated", "multiclass_nms_rotated",
    "batched_multiclass_nms_rotated", "assign_labels", "assign_labels_batched", "arf_forward", "arf_backward", "active_rotating_filter", "ORConv2d",
    "RotationInvariantPooling", "DeformConv", "DeformConvFunction", "deform_conv",
    "deform_conv_forward_cuda", "AlignConv", "AlignConvFunction", "align_conv", "RotInvPoolFunction", "rot_inv_pool",
    "rot_inv_pool_backward", "S2ANetLossFunction", "s2anet_loss", "grid_anchors", "drop_weight_caches",
    "tile_grid", "chip_names", "gather_chips", "merge_detections", "SceneDetections",
    "evaluate_task1", "Task1Evaluator", "Task1Result", "claim_tp_fp",
    "TrainUpdate", "reference_param_groups", "reference_lr",
    "train_kernels", "train_conv_ok", "train_conv_strided_ok", "FusedConv2d", "FusedConvFunction",
    "StemU8Function", "FusedConvUp2Function", "train_up2_ok",
    "quantize_weight_e4m3", "calibrate_fp8", "fp8_towers", "deterministic", "TrainAugment",
    "BatchNormTrainFunction", "batch_norm_train", "train_bn_ok", "train_batchnorm",
]
