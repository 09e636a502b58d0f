"""Opt-in FP8 (OCP e4m3fn) route for the head's plain 256 -> 256 tower convolutions (csrc/conv_fp8_ops.hip).

Off by default.  ``calibrate_fp8`` records the activation ranges once on the f16 path, ``fp8_towers`` switches the five
launches ``fam_reg_ls[0]``, ``fam_cls_ls[0]``, ``odm_reg_ls[0]``, ``odm_reg_ls[1]`` and ``odm_cls_ls[1]`` of
``S2ANetHead.forward_pyramid`` to ``s2a_conv3x3_pyramid_fp8``.  Filters are quantised per output channel, activations per
tensor with host floats fixed at calibration: nothing is read back at run time, so ``detect`` stays capturable.  The
scales are plain attributes of the head: its ``state_dict`` stays the reference's.
"""
import torch

E4M3_MAX = 448.0
# the tensors that are quantised: the FPN buffer, ORConv's output, the outputs of odm_reg_ls[0] and odm_cls_ls[0]
FP8_TENSORS = ("x", "or_feat", "odm_reg_ls0", "odm_cls_ls0")
FP8_LAYERS = ("fam_reg_ls.0", "fam_cls_ls.0", "odm_reg_ls.0", "odm_reg_ls.1", "odm_cls_ls.1")


def dequantize_e4m3(q):
    """uint8 tensor of e4m3fn bytes -> float32"""
    return q.view(torch.float8_e4m3fn).float()


def quantize_weight_e4m3(w):
    """[O,C,3,3] filter -> (w_q uint8 [O,C,3,3] of e4m3fn bytes, s_w f32[O]) with w ~ s_w[o] * deq(w_q):
    s_w[o] = max|w[o]| / 448 (1.0 for an all-zero filter), w_q = e4m3_rne(w / s_w).  Pure torch: runs on the CPU too."""
    w32 = w.detach().float().contiguous()
    absmax = w32.abs().amax(dim=tuple(range(1, w32.dim())))
    s_w = torch.where(absmax > 0, absmax / E4M3_MAX, torch.ones_like(absmax))
    q = (w32 / s_w.view(-1, *([1] * (w32.dim() - 1)))).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), s_w.contiguous()


def _head_of(model_or_head):
    return model_or_head.head if hasattr(model_or_head, "head") else model_or_head


def fp8_supported(head):
    """the head shapes the fp8 route is built for: two stacked 3x3 convs per tower, ORConv with 8 orientations, fused
    layers whose channel counts the kernel takes"""
    from .fused import FusedConv2d
    if not (head.stacked_convs == 2 and head.with_orconv):
        return False
    layers = (head.fam_reg_ls[0][0], head.fam_cls_ls[0][0], head.odm_reg_ls[0][0], head.odm_reg_ls[1][0], head.odm_cls_ls[1][0])
    return all(isinstance(c, FusedConv2d) and c.fp8_ok() for c in layers)


def _scale_of(absmax):
    return absmax / E4M3_MAX if absmax > 0 else 1.0


@torch.no_grad()
def calibrate_fp8(model_or_head, batches, scales=None):
    """Record the ranges of the tensors the fp8 route quantises and store them on the head as ``fp8_scales``
    (dict name -> float, x = scale * x_q; names in FP8_TENSORS).

    model: ``batches`` are device image batches as ``detect`` takes them; head: ``batches`` are (layout, x) pairs, x the
    pyramid-packed f16 feature buffer.  Every batch runs the f16 ``forward_pyramid`` with ``trace`` and the absolute
    maxima are read back (offline work).  ``scales``: use these values instead of measuring (dict with the names in
    FP8_TENSORS).  Returns the dict."""
    head = _head_of(model_or_head)
    if scales is None:
        was, head.fp8_enabled = getattr(head, "fp8_enabled", False), False
        amax = dict.fromkeys(FP8_TENSORS, 0.0)
        try:
            for batch in batches:
                tr = {}
                if head is model_or_head:
                    layout, x = batch
                    head.forward_pyramid(layout, x, trace=tr)
                else:
                    m = model_or_head
                    if m.backbone.stem_fusable(batch):
                        m.features_to_pred(batch, m.backbone.forward_u8(batch, 255.0), trace=tr)
                    else:
                        m.features_to_pred(batch, trace=tr)
                for k in FP8_TENSORS:
                    v = float(tr[k].float().abs().max())
                    if v != v or v == float("inf"):
                        raise ValueError(f"calibrate_fp8: {k} holds a non-finite value")
                    amax[k] = max(amax[k], v)
        finally:
            head.fp8_enabled = was
        scales = {k: _scale_of(v) for k, v in amax.items()}
    else:
        scales = {k: float(scales[k]) for k in FP8_TENSORS}
        if not all(0 < v < float("inf") for v in scales.values()):
            raise ValueError("calibrate_fp8: scales must be positive and finite")
    head.fp8_scales = scales
    return scales


def fp8_towers(model_or_head, enabled=True):
    """switch the head's five plain 256 -> 256 tower launches to the e4m3 kernels (or back).  Raises before calibration
    (``calibrate_fp8``) and for a head the route is not built for.  Returns the head."""
    head = _head_of(model_or_head)
    if enabled:
        if getattr(head, "fp8_scales", None) is None:
            raise RuntimeError("fp8_towers: calibrate first (calibrate_fp8(model_or_head, batches))")
        if not fp8_supported(head):
            raise RuntimeError("fp8_towers: needs the fused head (fuse_epilogues) with two stacked convs per tower, ORConv and "
                               "channel counts that are multiples of 128")
    head.fp8_enabled = bool(enabled)
    return head
