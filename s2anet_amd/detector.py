"""Carrier network for the end-to-end configs: R-50 backbone (C3-C5) + FPN (P3-P7) + S2ANetHead.

The backbone and neck carry no custom arithmetic: their layers are ``torch.nn`` modules that hold
the parameters, and at f16 inference every 1x1 / 3x3 convolution of them runs on this package's own ``k_conv_f16``
(BN folded, bias / residual / ReLU fused; `fused.py`) - only FPN's two stride-2 extra levels go to the library.
Structure follows
models/backbone.py:37-175,283-354 and models/neck.py:5-96 (same module/parameter names, so a
reference ``state_dict`` loads), but the constructor is OFFLINE: no torchvision download
(backbone.py:241-255); weights are seeded random (kaiming for ResNet backbone.py:134-140,
xavier-uniform for FPN neck.py:58-62, N(0,0.01) for the head).
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .fused import Conv3Chain, FusedConv2d, bottleneck_chain_ok, bottleneck_tail, bottleneck_tail_ok, conv3_chain_ok
from .head import S2ANetHead


class BottleNeck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        return self.forward_chain(x)[0]

    def forward_chain(self, x, pre=None, nxt=None):
        """-> (block output, the NEXT block's conv1 output or None).  pre = this block's conv1 output when the previous
        block's tail or conv3 launch already produced it; nxt = the next block (run_blocks)."""
        residual = x
        if isinstance(self.conv3, FusedConv2d):           # BN folded, epilogues fused (inference)
            out = pre if pre is not None else self.conv1(x)
            if self.downsample is not None:
                residual = self.downsample(x)
            if bottleneck_tail_ok(out, self.conv2, self.conv3, residual):   # conv2 + conv3 + residual: one launch
                if isinstance(nxt, BottleNeck) and bottleneck_chain_ok(nxt.conv1):
                    return bottleneck_tail(out, self.conv2, self.conv3, residual, nxt.conv1)
                return bottleneck_tail(out, self.conv2, self.conv3, residual), None
            if isinstance(nxt, BottleNeck) and conv3_chain_ok(self.conv3, nxt.conv1):
                # conv3 + residual + ReLU and the next block's conv1 in one launch (stages 2 and 3, and into layer3.0)
                ch = Conv3Chain(nxt.conv1)
                return self.conv3(self.conv2(out), residual, chain=ch), ch.out
            return self.conv3(self.conv2(out), residual), None  # relu(conv3 + bias + residual) in one pass
        return self._forward_plain(x), None

    own_grad_norm = False       # norm.train_batchnorm(): the fourth opt-in -- a grad-enabled training forward of the unfolded
    #                             block runs on the own kernels (_forward_own_norm) when every layer passes its predicate

    def _own_norm_layers(self):
        """(conv, bn) pairs of the unfolded block: conv1, conv2, conv3 and, when there is one, the downsample"""
        pairs = [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]
        if self.downsample is not None:
            pairs.append((self.downsample[0], self.downsample[1]))
        return pairs

    def _own_norm_ok(self, x):
        """the four conditions of the own route: the flag, grad enabled, the norms in training mode, every layer inside its
        predicate.  The predicates are evaluated on x, on the shapes that follow from it and on the parameters, once per input
        geometry and parameter dtype (the answer is cached on the block)"""
        if not (self.own_grad_norm and torch.is_grad_enabled()):
            return False
        pairs = self._own_norm_layers()
        if not all(type(c) is nn.Conv2d and isinstance(b, nn.BatchNorm2d) and b.training for c, b in pairs):
            return False
        if self.downsample is not None and len(self.downsample) != 2:
            return False
        key = (tuple(x.shape), x.dtype, x.device, x.is_contiguous(memory_format=torch.channels_last)) + tuple(
            (c.weight.dtype, c.weight.device, c.bias is None, b.weight is not None and b.weight.dtype,
             b.running_mean is not None and b.running_mean.dtype, b.running_var is not None and b.running_var.dtype,
             type(b.momentum), b.affine, b.track_running_stats) for c, b in pairs)
        cached = self.__dict__.get("_own_norm_cache")
        if cached is None or cached[0] != key:
            cached = (key, self._own_norm_predicates(x))
            self.__dict__["_own_norm_cache"] = cached
        return cached[1]

    def _own_norm_predicates(self, x):
        """every layer inside its predicate, on shapes: (B, C, H, W) goes through train_shape_problem to (B, O, Ho, Wo) and that
        through bn_shape_problem; what integers cannot say is asked of x itself and of the parameters.  No tensor is made."""
        from .fused import train_shape_problem, train_tensors_problem
        from .norm import bn_layer_problem, bn_shape_problem

        def conv_bn(shape, conv, bn):
            """-> the output's shape when conv takes an f16 channels-last activation of `shape` and bn takes the result, else None"""
            B, C, H, W = shape
            O, s = conv.out_channels, conv.stride
            out = (B, O, (H - 1) // s[0] + 1, (W - 1) // s[1] + 1)
            bad = (conv.bias is not None or C != conv.in_channels or train_tensors_problem(None, conv.weight, None, C) or
                   train_shape_problem(conv.kernel_size, s, conv.padding, conv.dilation, conv.groups, C, O, B, H, W) or
                   O != bn.num_features or bn_shape_problem(B * out[2] * out[3], O) or bn_layer_problem(bn))
            return None if bad else out

        if train_tensors_problem(x, self.conv1.weight, None, self.conv1.in_channels):
            return False
        y = r = tuple(x.shape)
        for conv, bn in self._own_norm_layers()[:3]:
            y = y and conv_bn(y, conv, bn)
        r = r if self.downsample is None else conv_bn(r, *self.downsample)
        return y is not None and r == y             # (bn3's residual, x or the downsample's output, has the output's shape)

    def _forward_own_norm(self, x):
        """the unfolded block in training mode on the own kernels: conv1 -> BN + ReLU, conv2 (stride 1 or 2) -> BN + ReLU,
        conv3 -> BN + residual + ReLU in one apply launch, downsample conv -> BN (models/backbone.py:54-83)"""
        from .fused import FusedConvFunction, FusedConvS2Function
        from .norm import batch_norm_train

        def conv(c, t):
            fn = FusedConvS2Function if tuple(c.stride) == (2, 2) else FusedConvFunction
            return fn.apply(t, c.weight, None, None, False)

        out = batch_norm_train(conv(self.conv1, x), self.bn1, relu=True)
        out = batch_norm_train(conv(self.conv2, out), self.bn2, relu=True)
        residual = x
        if self.downsample is not None:
            residual = batch_norm_train(conv(self.downsample[0], x), self.downsample[1])
        return batch_norm_train(conv(self.conv3, out), self.bn3, residual, relu=True)

    def _forward_plain(self, x):
        if self._own_norm_ok(x):
            return self._forward_own_norm(x)
        residual = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            residual = self.downsample(x)
        out += residual
        return self.relu(out)


class DetectorBackbone(nn.Module):
    """ResNet-50 trunk exposing C3, C4, C5 (out_indices=(2,3,4), backbone.py:283-354)"""

    def __init__(self, layers=(3, 4, 6, 3), out_indices=(2, 3, 4)):
        super().__init__()
        self.inplanes = 64
        conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        bn1 = nn.BatchNorm2d(64)
        layer1 = self._make_layer(64, layers[0])
        layer2 = self._make_layer(128, layers[1], stride=2)
        layer3 = self._make_layer(256, layers[2], stride=2)
        layer4 = self._make_layer(512, layers[3], stride=2)
        self.backbone = nn.Sequential(
            nn.Sequential(conv1, bn1, nn.ReLU(inplace=True)),
            nn.Sequential(nn.MaxPool2d(kernel_size=3, stride=2, padding=1, ceil_mode=False), layer1),
            layer2, layer3, layer4)
        self.out_indices = out_indices
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * 4))
        layers = [BottleNeck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * 4
        layers += [BottleNeck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    @staticmethod
    def run_blocks(seq, x, pre=None, after=None, with_pre=False):
        """a stage's bottlenecks one after the other; a block's tail kernel may hand the next block its conv1 output.
        pre = conv1 output for the first block (from the previous stage's last tail), after = the block that follows
        the stage; with_pre -> (x, conv1 output for `after` or None)"""
        for i, blk in enumerate(seq):
            if not isinstance(blk, BottleNeck):
                x, pre = blk(x), None
                continue
            x, pre = blk.forward_chain(x, pre, seq[i + 1] if i + 1 < len(seq) else after)
        return (x, pre) if with_pre else x

    def _stages(self, x):
        """layer1 .. layer4 on the pooled stem output"""
        outs, pre = [], None
        first = self.backbone[1][1][0]
        if getattr(first, "own_grad_norm", False) and torch.is_grad_enabled() and x.is_cuda and \
                isinstance(first.bn1, nn.BatchNorm2d) and first.bn1.training and \
                not (x.dtype == torch.float16 and x.is_contiguous(memory_format=torch.channels_last)):
            # trunk entry of the own BatchNorm route (norm.train_batchnorm): the pooled stem output, cast once to f16
            # channels-last with stock differentiable ops (the stem itself stays on its route)
            x = x.to(torch.float16).contiguous(memory_format=torch.channels_last)
        for i in range(1, len(self.backbone)):
            seq = self.backbone[i][1] if i == 1 else self.backbone[i]
            after = self.backbone[i + 1][0] if i + 1 < len(self.backbone) else None
            x, pre = self.run_blocks(seq, x, pre, after, with_pre=True)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def forward(self, x):
        """x: the normalised float batch; or, with own_grad_entry on the stem conv (train_kernels(entry=True)) and grad
        enabled, the raw uint8 batch: the stem then trains on the own kernels (StemU8Function, / 255 inside) when the shapes
        allow (stem_limits), and on the stock route from x.to(dtype) / 255 when they do not"""
        assert 0 not in self.out_indices
        conv = self.backbone[0][0]
        if x.dtype == torch.uint8 and getattr(conv, "own_grad_entry", False) and torch.is_grad_enabled():
            if self.stem_limits(x) and conv.weight.dtype in (torch.float16, torch.float32) and conv.weight.is_cuda and \
                    (conv.bias is None or conv.bias.dtype == conv.weight.dtype):
                from .fused import StemU8Function
                return self._stages(StemU8Function.apply(x, conv.weight, conv.bias, 255.0))
            x = x.to(conv.weight.dtype) / 255
        return self._stages(self.backbone[1][0](self.backbone[0](x)))

    def stem_limits(self, imgs_u8):
        """what the fused stem kernels need, either way: the BN-folded 7x7 / s2 / p3 conv with its ReLU, the 3x3 / s2 / p1
        pool, a uint8 channels-last RGB batch on the GPU, at least 7 pixels a side, the width a multiple of 4"""
        conv, pool = self.backbone[0][0], self.backbone[1][0]
        return (isinstance(conv, FusedConv2d) and conv.fuse_relu and
                tuple(conv.weight.shape) == (64, 3, 7, 7) and conv.stride == (2, 2) and conv.padding == (3, 3) and
                isinstance(pool, nn.MaxPool2d) and pool.kernel_size == 3 and pool.stride == 2 and pool.padding == 1 and
                not pool.ceil_mode and imgs_u8.is_cuda and imgs_u8.dtype == torch.uint8 and imgs_u8.dim() == 4 and
                imgs_u8.shape[1] == 3 and imgs_u8.shape[3] % 4 == 0 and min(imgs_u8.shape[2:]) >= 7 and
                imgs_u8.permute(0, 2, 3, 1).is_contiguous())

    def stem_fusable(self, imgs_u8):
        """uint8 channels-last batch + BN-folded stem: /255, conv1, ReLU and the max-pool run as one kernel"""
        return (self.stem_limits(imgs_u8) and self.backbone[0][0].weight.dtype == torch.float16 and
                not torch.is_grad_enabled() and not os.environ.get("S2A_NO_FUSED_STEM"))

    def forward_u8(self, imgs_u8, divisor=255.0):
        """forward() on the raw uint8 batch with the fused stem (s2a_stem_u8_f16)"""
        from .fused import PackedWeightCache, stem_pack_weight, stem_u8
        conv = self.backbone[0][0]
        c = self.__dict__.get("_stem_cache")
        if c is None:
            self._stem_cache = c = PackedWeightCache()
        # filter and bias each under their own key: a bias-only update is followed too
        self._stem_w = c.lookup("stem", conv.weight, None, stem_pack_weight, conv.weight)
        self._stem_b = c.get_bias(conv.bias, conv.out_channels)
        return self._stages(stem_u8(imgs_u8, self._stem_w, self._stem_b, divisor))


class FPN(nn.Module):
    def __init__(self, in_channels=(512, 1024, 2048), out_channels=256, num_outs=5):
        super().__init__()
        self.num_ins, self.num_outs = len(in_channels), num_outs
        self.lateral_convs = nn.ModuleList(nn.Conv2d(c, out_channels, 1) for c in in_channels)
        self.fpn_convs = nn.ModuleList(nn.Conv2d(out_channels, out_channels, 3, padding=1) for _ in in_channels)
        for i in range(num_outs - self.num_ins):
            cin = in_channels[-1] if i == 0 else out_channels
            self.fpn_convs.append(nn.Conv2d(cin, out_channels, 3, stride=2, padding=1))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                nn.init.constant_(m.bias, 0)

    def forward_packed(self, inputs, layout):
        """same as forward(), but the five outputs land back to back in ONE pyramid-packed buffer
        [sum B*H*W, 256] (s2anet_amd/pyramid.py) so that the head can run each layer once for all levels"""
        from .fused import conv_f16, conv1x1_add_up2, own_conv_ok
        lat = [None] * self.num_ins
        lat[-1] = self.lateral_convs[-1](inputs[-1])
        for i in range(self.num_ins - 1, 0, -1):           # top-down: lateral conv + up-sampled coarser level, one launch
            l, x = self.lateral_convs[i - 1], inputs[i - 1]
            if (hasattr(l, "packed_args") and x.shape[2] == 2 * lat[i].shape[2] and x.shape[3] == 2 * lat[i].shape[3] and
                    lat[i].is_contiguous(memory_format=torch.channels_last) and l.out_channels % 64 == 0 and
                    own_conv_ok(x, l.in_channels, l.out_channels, l.kernel_size, l.stride, l.padding, l.dilation, l.groups)):
                w, b, o = l.packed_args()
                lat[i - 1] = conv1x1_add_up2(x, w, b, lat[i], o)
            else:
                lat[i - 1] = l(x) + F.interpolate(lat[i], scale_factor=2, mode="nearest")
        buf = layout.new(self.fpn_convs[0].out_channels, inputs[0].device)
        for i in range(self.num_outs):
            conv = self.fpn_convs[i]
            src = lat[i] if i < self.num_ins else (inputs[-1] if i == self.num_ins else prev)
            dst = layout.level(buf, i)                          # [B,C,H,W] channels-last view of the slice
            if i < self.num_ins and hasattr(conv, "packed_args"):
                w, b, o = conv.packed_args()
                prev = conv_f16(src, w, b, o, 3, 1, False, out=dst)
            elif isinstance(conv, FusedConv2d) and conv.bias is not None and src.is_contiguous(memory_format=torch.channels_last) \
                    and not own_conv_ok(src, conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride,
                                        conv.padding, conv.dilation, conv.groups):
                prev = conv(src, out=dst)       # library convolution, its bias pass writes the pyramid slice (no copy)
            else:
                prev = conv(src)
                dst.copy_(prev)
        return buf

    def _laterals_entry(self, inputs):
        """the laterals and the top-down sums with own_grad_entry (train_kernels(entry=True)): a step inside train_up2_ok is
        one FusedConvUp2Function, every other step the stock line of forward()"""
        from .fused import FusedConvUp2Function, train_up2_ok
        lat = [None] * self.num_ins
        lat[-1] = self.lateral_convs[-1](inputs[-1])
        for i in range(self.num_ins - 1, 0, -1):
            l, x = self.lateral_convs[i - 1], inputs[i - 1]
            if getattr(l, "own_grad_entry", False) and train_up2_ok(x, l, lat[i]):
                lat[i - 1] = FusedConvUp2Function.apply(x, l.weight, l.bias, lat[i])
            else:
                lat[i - 1] = l(x) + F.interpolate(lat[i], scale_factor=2, mode="nearest")
        return lat

    def forward(self, inputs):
        if any(getattr(l, "own_grad_entry", False) for l in self.lateral_convs):
            lat = self._laterals_entry(inputs)
        else:
            lat = [l(inputs[i]) for i, l in enumerate(self.lateral_convs)]
            for i in range(self.num_ins - 1, 0, -1):
                lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], scale_factor=2, mode="nearest")
        outs = [self.fpn_convs[i](lat[i]) for i in range(self.num_ins)]
        for i in range(self.num_outs - self.num_ins):
            outs.append(self.fpn_convs[self.num_ins + i](inputs[-1] if i == 0 else outs[-1]))
        return tuple(outs)


class S2ANet(nn.Module):
    """models/detector.py:9-37.  forward(imgs, post_process) -> dict like the reference."""

    def __init__(self, num_classes=15, **head_kw):
        super().__init__()
        self.stride = (8, 16, 32, 64, 128)
        self.backbone = DetectorBackbone()
        self.neck = FPN(num_outs=len(self.stride))
        self.head = S2ANetHead(num_classes=num_classes, featmap_strides=self.stride, **head_kw)

    def forward(self, imgs, targets=None, post_process=False):
        """models/detector.py:28-35: the head gets imgs_size = imgs.shape[-2:] (h, w) to scale targets to pixels"""
        if isinstance(targets, bool):
            targets, post_process = None, targets
        return self.head(self.neck(self.backbone(imgs)), targets, imgs.shape[-2:], post_process=post_process)

    def features_to_pred(self, imgs, backbone_out=None, **pyramid_kw):
        """pyramid_kw: ``anchors`` / ``trace`` of S2ANetHead.forward_pyramid (pyramid-packed path only)"""
        c = self.backbone(imgs) if backbone_out is None else backbone_out
        sizes = [tuple(c[0].shape[2:])]
        while len(sizes) < len(self.stride):                    # stride-2 3x3/pad-1 convs: ceil(n/2)
            sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
        if self.head.pyramid_ok(c[0]) and hasattr(self.neck.fpn_convs[0], "packed_args") and \
                min(sizes[-1]) >= 3 and not os.environ.get("S2A_NO_PYRAMID"):
            from .pyramid import PyramidLayout
            B = imgs.shape[0]
            key = (B, tuple(sizes))
            if getattr(self, "_layout_key", None) != key:
                self._layout_key, self._layout = key, PyramidLayout(B, sizes, self.stride)
            if pyramid_kw.get("trace") is not None:
                pyramid_kw["trace"].update(C=c, layout=self._layout)
            return self.head.forward_pyramid(self._layout, self.neck.forward_packed(c, self._layout), **pyramid_kw)
        assert not pyramid_kw, "anchors= / trace= need the pyramid-packed path"
        feats = self.neck(c)
        per_level = [self.head.forward_single(f, s) for f, s in zip(feats, self.stride)]
        return tuple(map(list, zip(*per_level)))

    @torch.no_grad()
    def detect(self, imgs_u8, max_candidates=None, return_overflow=False, **nms_kw):
        """device-resident uint8 batch [B,3,H,W] -> (dets[B,2000,6], labels[B,2000], counts[B]).
        /255 normalisation as val.py:246-247; no host synchronisation anywhere.
        max_candidates caps the (box, class) rows the batch's NMS considers (static shapes); the reference never
        drops one, so with return_overflow=True a fourth result int64[2] = [candidates found, candidates dropped]
        comes back on the device (dropped must be 0 for reference-equal results).
        nms_kw: ``dropped_total`` (device int64 accumulator) and ``return_wire`` (append the all-gather wire buffer
        float32 [B, 2000*7+1] that ``dets`` is a view of) -- see rotated.batched_multiclass_nms_rotated."""
        if self.backbone.stem_fusable(imgs_u8):
            return self.head.get_bboxes_batched(
                self.features_to_pred(imgs_u8, self.backbone.forward_u8(imgs_u8, 255.0)), max_candidates, return_overflow,
                **nms_kw)
        dt = next(self.parameters()).dtype
        x = imgs_u8.to(dt).div_(255.0)
        if imgs_u8.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        return self.head.get_bboxes_batched(self.features_to_pred(x), max_candidates, return_overflow, **nms_kw)

    def detect_scene(self, scene_u8, batch=8, subsize=1024, gap=200, rate=1.0, thresh=0.5, return_chips=False, check=True,
                     **detect_kw):
        """a whole scene uint8 [H,W,3] on the device (or a list of (scene, rate) pairs) -> merged detections in scene
        coordinates (``scene.SceneDetections``): tile grid of the reference's splitter, one gather launch per batch,
        ``detect()`` in fixed batches, per-class polygon merge on the device -- see s2anet_amd/scene.py"""
        from .scene import detect_scene
        return detect_scene(self, scene_u8, batch, subsize, gap, rate, thresh, return_chips, check, **detect_kw)


def load_reference_checkpoint(model, weights, map_location="cpu"):
    """val.py:153-183: a ``.pth`` file (or an already loaded dict) with a ``"state_dict"`` entry is
    matched to the model's own entries BY POSITION (the official-code checkpoints use other key
    names; ``intersect_dicts`` zips the two ordered dicts and asserts equal length), then loaded
    strictly.  A dict with a ``"model"`` entry holds a module (or its state_dict): loaded by name.
    Call before ``fold_batchnorm`` / ``fuse_epilogues`` (they keep values, not the BN entries)."""
    ckpt = torch.load(weights, map_location=map_location, weights_only=False) \
        if isinstance(weights, (str, os.PathLike)) else weights
    own = model.state_dict()
    if "state_dict" in ckpt:
        src = ckpt["state_dict"]
        if len(src) != len(own):
            raise AssertionError(f"checkpoint has {len(src)} entries, the model {len(own)}")
        mapped = {}
        for (k1, v1), (k2, v2) in zip(own.items(), src.items()):
            if tuple(v1.shape) != tuple(v2.shape):
                raise RuntimeError(f"size mismatch for {k1} <- {k2}: {tuple(v2.shape)} vs {tuple(v1.shape)}")
            mapped[k1] = v2
        model.load_state_dict(mapped, strict=True)
    elif "model" in ckpt:
        src = ckpt["model"]
        model.load_state_dict(src.state_dict() if hasattr(src, "state_dict") else src, strict=True)
    else:
        raise KeyError("checkpoint holds neither 'state_dict' nor 'model' (val.py:155,182)")
    return model


def fold_batchnorm(model):
    """inference-time conv+BN folding (BN in eval mode is an affine map): fewer passes over HBM"""
    def fold(conv, bn):
        w = conv.weight
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        fused = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                          conv.dilation, conv.groups, bias=True).to(w.device, w.dtype)
        fused.weight.data = w * scale.view(-1, 1, 1, 1)
        b = conv.bias if conv.bias is not None else torch.zeros_like(bn.running_mean)
        fused.bias.data = (b - bn.running_mean) * scale + bn.bias
        return fused

    for mod in model.modules():
        if isinstance(mod, BottleNeck):
            mod.conv1, mod.bn1 = FusedConv2d.from_conv(fold(mod.conv1, mod.bn1), relu=True), nn.Identity()
            mod.conv2, mod.bn2 = FusedConv2d.from_conv(fold(mod.conv2, mod.bn2), relu=True), nn.Identity()
            mod.conv3, mod.bn3 = FusedConv2d.from_conv(fold(mod.conv3, mod.bn3), relu=True), nn.Identity()
            if mod.downsample is not None:
                mod.downsample = nn.Sequential(FusedConv2d.from_conv(fold(mod.downsample[0], mod.downsample[1])))
    stem = model.backbone.backbone[0]
    model.backbone.backbone[0] = nn.Sequential(FusedConv2d.from_conv(fold(stem[0], stem[1]), relu=True), nn.Identity())
    return model


def fuse_epilogues(model):
    """swap every remaining biased nn.Conv2d (FPN, head towers, prediction heads) for FusedConv2d;
    conv+ReLU pairs inside nn.Sequential collapse into one module (names/params unchanged)"""
    from .orn import ORConv2d
    for parent in list(model.modules()):
        if isinstance(parent, nn.Sequential) and len(parent) == 2 and type(parent[0]) is nn.Conv2d \
                and isinstance(parent[1], nn.ReLU) and parent[0].bias is not None:
            parent[0] = FusedConv2d.from_conv(parent[0], relu=True)
            parent[1] = nn.Identity()
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is nn.Conv2d and child.bias is not None and not isinstance(child, ORConv2d):
                setattr(parent, name, FusedConv2d.from_conv(child, relu=False))
    return model


def build_synthetic_detector(num_classes=15, seed=1234, dtype=torch.float16, device="cuda",
                             channels_last=True, fold_bn=True, **head_kw):
    """random-init S2ANet of the reference architecture (no network access, no checkpoint).
    The last BN of every bottleneck gets gamma = 0.25 so that activations of the untrained
    50-layer trunk stay inside fp16 range (a trained network has learned scales instead)."""
    torch.manual_seed(seed)
    m = S2ANet(num_classes=num_classes, **head_kw)
    for mod in m.modules():
        if isinstance(mod, BottleNeck):
            mod.bn3.weight.data.fill_(0.25)
    m.eval()
    if fold_bn:
        fold_batchnorm(m)
        fuse_epilogues(m)
    m = m.to(device=device, dtype=dtype)
    if channels_last:
        # 4-D conv filters only (ORConv2d keeps its 5-D filter bank; its cached ARF expansion is
        # converted in ORConv2d.rotate_arf)
        for mod in m.modules():
            if isinstance(mod, nn.Conv2d) and mod.weight.dim() == 4 and mod.weight.shape[1] >= 8:
                mod.weight.data = mod.weight.data.contiguous(memory_format=torch.channels_last)
        m.head.or_conv.channels_last = True
    return m
