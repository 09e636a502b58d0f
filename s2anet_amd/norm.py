"""Training-mode BatchNorm on the own kernels (csrc/bn_ops.hip) for the unfolded trunk: torch.nn.BatchNorm2d as the
reference trains it (models/backbone.py:54-83) -- batch statistics, learned gamma / beta, running statistics moved every
step.  The modules stay nn.BatchNorm2d: state_dict keys, parameter groups and fold_batchnorm are untouched; what changes,
behind the opt-in train_batchnorm(model), is the route a grad-enabled training forward of a bottleneck takes
(detector.BottleNeck._forward_plain)."""
import torch
import torch.nn as nn

from . import _lib

_CL = torch.channels_last


_BN_WIDTH, _BN_BYTES = "the channel count is not bn.num_features or no multiple of 64", "2^31 bytes or more"


def bn_shape_problem(P, C):
    """why the kernels cannot take a [P, C] problem (P = B H W positions of C channels), or None: bn::plan_ok of csrc/bn_plan.hpp
    on the Python side, and its one statement there (tests/test_train_limits_cpu.py holds it against s2a_bn_slices)"""
    if not (C > 0 and C % 64 == 0):
        return _BN_WIDTH
    if P < 2:
        return "fewer than 2 values per channel"
    return None if C < (1 << 24) and P < (1 << 31) and P * C * 2 < (1 << 31) else _BN_BYTES


def bn_layer_problem(bn, need_cuda=True):
    """why an nn.BatchNorm2d's own state keeps it off the kernels, whatever it is fed, or None"""
    if not (bn.affine and bn.track_running_stats) or bn.weight is None or bn.running_mean is None:
        return "the layer is not affine with running statistics"
    if not isinstance(bn.momentum, float):
        return "momentum is not a float"
    w, b, rm, rv = bn.weight, bn.bias, bn.running_mean, bn.running_var
    if w.dtype not in (torch.float16, torch.float32) or b.dtype != w.dtype:
        return "weight and bias are not both float16 or both float32"
    if rm.dtype != rv.dtype or rm.dtype not in (torch.float32, w.dtype):
        return "running statistics are neither float32 nor the parameters' dtype"
    if need_cuda and not (w.is_cuda and b.is_cuda and rm.is_cuda and rv.is_cuda):
        return "the layer is not on the GPU"
    return None


def _bn_problem(x, bn, residual=None, need_cuda=True):
    """why batch_norm_train cannot take (x, bn, residual), or None.  Limits only, no speed heuristic.  need_cuda=False leaves
    the device out (the other limits can then be read off CPU tensors)"""
    if not isinstance(bn, nn.BatchNorm2d):
        return "not an nn.BatchNorm2d"
    if need_cuda and not x.is_cuda:
        return "x is not on the GPU"
    if x.dtype != torch.float16:
        return "x is not float16"
    if x.dim() != 4 or x.numel() == 0 or not x.is_contiguous(memory_format=_CL):
        return "x is not a channels-last 4-D tensor"
    B, C, H, W = x.shape
    shape = _BN_WIDTH if C != bn.num_features else bn_shape_problem(B * H * W, C)
    if shape not in (None, _BN_BYTES):
        return shape
    if residual is not None and not ((residual.is_cuda or not need_cuda) and residual.dtype == torch.float16 and
                                     tuple(residual.shape) == tuple(x.shape) and residual.is_contiguous(memory_format=_CL)):
        shape = "the residual has not the output's shape, dtype and layout"
    return bn_layer_problem(bn, need_cuda) or shape         # (the layer's own state, then the residual, the size limits last)


def train_bn_ok(x, bn, residual=None):
    """limits of the own training route of a BatchNorm2d (BatchNormTrainFunction), and nothing but limits: a CUDA f16
    channels-last 4-D x with C == bn.num_features, C % 64 == 0 and at least 2 values per channel; an affine layer with running
    statistics and a float momentum; weight and bias of one dtype, f16 or f32; running statistics in f32 or that dtype; a
    residual of the output's shape and layout; tensors under 2^31 bytes, C under 2^24 (bn_shape_problem)"""
    return _bn_problem(x, bn, residual) is None


class BatchNormTrainFunction(torch.autograd.Function):
    """relu?(batch_norm(x; batch statistics, weight, bias) (+ residual)) with its backward on the own kernels.
    Forward: s2a_bn_train_stats_f16 (mean, invstd; running_mean / running_var moved in place as nn.BatchNorm2d moves them) and
    s2a_bn_train_apply_f16 (normalise, scale, shift, residual and ReLU in one launch, one rounding; the ReLU keeps a NaN).
    num_batches_tracked += 1 by the stock in-place op.  Saved: x, weight, mean, invstd, and out only behind a ReLU.
    Backward: s2a_bn_backward_reduce_f16 (ReLU mask, grad_bias = sum g, grad_weight = sum g xhat, in the parameters' dtype) and
    s2a_bn_backward_input_f16 (dx = weight invstd (g - mean(g) - xhat mean(g xhat))); only what needs_input_grad asks for is
    computed, and g is written as a tensor only when the residual wants a gradient behind a ReLU (it is that gradient).
    No host read, no float atomic, no memset node, geometry from shapes only, buffers from the torch allocator: capturable,
    and bit-equal from run to run."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, num_batches_tracked, eps, momentum, relu):
        B, C, H, W = x.shape
        P = B * H * W
        if P < 2:       # torch.nn.functional.batch_norm's own refusal (_verify_batch_size)
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
        L, dev = _lib.lib(), x.device
        slices = L.s2a_bn_slices(P, C)
        if slices <= 0:
            raise RuntimeError(f"batch_norm_train: [{P}, {C}] is outside the kernels' limits (train_bn_ok)")
        partial = torch.empty((slices, 2, C), dtype=torch.float32, device=dev)
        mean = torch.empty((C,), dtype=torch.float32, device=dev)
        invstd = torch.empty_like(mean)
        out = torch.empty_like(x)
        w, b = weight.detach(), bias.detach()
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            _lib.check(L.s2a_bn_train_stats_f16(_lib.ptr(x), P, C, float(eps), float(momentum), _lib.ptr(partial), slices,
                                                _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(running_mean), _lib.ptr(running_var),
                                                0 if running_mean is None else _lib.dtype_code(running_mean), st))
            _lib.check(L.s2a_bn_train_apply_f16(_lib.ptr(x), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(w), _lib.ptr(b),
                                                _lib.dtype_code(w), _lib.ptr(residual), _lib.ptr(out), P, C, int(bool(relu)), st))
        if num_batches_tracked is not None:
            num_batches_tracked.add_(1)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        sums = need_x or need_w or need_b
        ctx.save_for_backward(x if sums else None, w if need_x else None, mean if sums else None, invstd if sums else None,
                              out if relu else None)
        ctx.geom = (P, C, slices, weight.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, w, mean, invstd, out = ctx.saved_tensors
        P, C, slices, pdtype = ctx.geom
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        L, dev = _lib.lib(), grad_out.device
        go = grad_out if grad_out.dtype == torch.float16 else grad_out.to(torch.float16)
        go = go.contiguous(memory_format=_CL)
        sums = need_x or need_w or need_b
        g = torch.empty_like(go) if (need_r and out is not None) else None       # the residual's gradient behind the mask
        gx = gw = gb = None
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            if sums:
                partial = torch.empty((slices, 2, C), dtype=torch.float32, device=dev)
                coef = torch.empty((2, C), dtype=torch.float32, device=dev)
                gw = torch.empty((C,), dtype=pdtype, device=dev) if need_w else None
                gb = torch.empty((C,), dtype=pdtype, device=dev) if need_b else None
                _lib.check(L.s2a_bn_backward_reduce_f16(_lib.ptr(go), _lib.ptr(x), _lib.ptr(out), _lib.ptr(mean), _lib.ptr(invstd),
                                                        _lib.ptr(g), _lib.ptr(partial), slices, _lib.ptr(gw), _lib.ptr(gb),
                                                        _lib.DTYPE_F16 if pdtype == torch.float16 else _lib.DTYPE_F32,
                                                        _lib.ptr(coef), P, C, st))
            elif g is not None:
                _lib.check(L.s2a_bn_backward_reduce_f16(_lib.ptr(go), None, _lib.ptr(out), None, None, _lib.ptr(g), None, 0, None,
                                                        None, 0, None, P, C, st))
            if need_x:
                gx = torch.empty_like(go)
                src, mask = (g, None) if g is not None else (go, out)
                _lib.check(L.s2a_bn_backward_input_f16(_lib.ptr(src), _lib.ptr(x), _lib.ptr(mask), _lib.ptr(mean), _lib.ptr(invstd),
                                                       _lib.ptr(w), _lib.dtype_code(w), _lib.ptr(coef), _lib.ptr(gx), P, C, st))
        gr = (g if out is not None else go) if need_r else None
        return gx, gw, gb, gr, None, None, None, None, None, None


def batch_norm_train(x, bn, residual=None, relu=False):
    """relu?(bn(x) (+ residual)) of an nn.BatchNorm2d in training mode on the own kernels (BatchNormTrainFunction): batch
    statistics, running statistics and num_batches_tracked moved as the module's own forward moves them.  Raises outside
    train_bn_ok -- there is no fall-back; a single value per channel raises the ValueError torch raises."""
    _lib.require_cuda(x, residual)
    if x.dim() == 4 and x.numel() == x.shape[1] and x.numel() > 0:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
    problem = _bn_problem(x, bn, residual)
    if problem is not None:
        raise RuntimeError(f"batch_norm_train: {problem} (train_bn_ok states the limits)")
    return BatchNormTrainFunction.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                        bn.eps, bn.momentum, bool(relu))


def train_batchnorm(model, enabled=True):
    """own_grad_norm = enabled on every BottleNeck of the tree -> how many nn.BatchNorm2d layers the tree holds.  With the flag
    a grad-enabled forward of a bottleneck whose norms are in training mode, and whose every layer passes its predicate
    (train_conv_ok / train_conv_strided_ok, train_bn_ok), runs its convolutions as FusedConvFunction / FusedConvS2Function and
    its norms as BatchNormTrainFunction; every other block and every other call keeps its route.  Sets nothing else: the
    switches of train_kernels are separate.  (The stem's norm is counted and stays on the stock route: DESIGN.md 5d.)"""
    from .detector import BottleNeck
    for m in model.modules():
        if isinstance(m, BottleNeck):
            m.own_grad_norm = bool(enabled)
    return sum(1 for m in model.modules() if isinstance(m, nn.BatchNorm2d))
