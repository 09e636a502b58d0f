"""S2ANet head, inference half (models/head.py:261-348, :648-725), batched.

Layer names and shapes follow the reference so that a reference ``state_dict`` loads unchanged
(``fam_reg_ls.N.0``, ``fam_cls_ls``, ``fam_reg_head``, ``fam_cls_head``, ``align_conv.deform_conv``,
``or_conv``, ``odm_reg_ls``, ``odm_cls_ls``, ``odm_cls_head``, ``odm_reg_head``).

What changed against the reference glue (same results, no per-image / per-level host work):
  * grid anchors are never built on the CPU and copied (head.py:315-326): the refined anchors
    come from ONE kernel per level (grid anchor + FAM decode fused, ``s2a_fam_refine_anchors``)
  * AlignConv consumes the refined anchors directly (no per-image get_offset loop, no offset tensor)
  * get_bboxes is batched: per-level top-k over the whole batch, one decode, ONE segmented
    rotated NMS launch sequence for all images, no host synchronisation
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .alignconv import AlignConv
from .loss import LOSS_DEFAULTS, grid_anchors, s2anet_loss
from .orn import ORConv2d, RotationInvariantPooling
from .rotated import assign_labels, assign_labels_batched, batched_multiclass_nms_rotated, multiclass_nms_rotated


def delta2bbox_rotated(rois, deltas, wh_ratio_clip=16 / 1000):
    """models/boxes.py:82-162 (is_encode_relative=True); rois/deltas [n,5] -> [n,5] f32"""
    _lib.require_cuda(rois, deltas)
    r, d = rois.float().contiguous(), deltas.float().contiguous()
    assert r.shape == d.shape and r.shape[-1] == 5
    out = torch.empty_like(r)
    n = r.numel() // 5
    with torch.cuda.device(r.device):
        _lib.check(_lib.lib().s2a_delta2bbox_rotated(_lib.ptr(r), _lib.ptr(d), n, float(wh_ratio_clip),
                                                     _lib.ptr(out), _lib.stream_ptr(r.device)))
    return out


rboxes_decode = delta2bbox_rotated   # models/boxes.py:223-247


def fam_refine_anchors(bbox_pred, stride, anchor_scale=4.0):
    """gen_grid_anchors (models/anchors.py:75-126) + fam_bbox_decode (models/head.py:27-52):
    bbox_pred[B,5,H,W] (f32/f16, NCHW or channels_last) -> refined anchors [B,H,W,5] f32"""
    _lib.require_cuda(bbox_pred)
    B, five, H, W = bbox_pred.shape
    assert five == 5
    nhwc = not bbox_pred.is_contiguous() and bbox_pred.is_contiguous(memory_format=torch.channels_last)
    p = bbox_pred if nhwc else bbox_pred.contiguous()
    out = torch.empty((B, H, W, 5), dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().s2a_fam_refine_anchors(
            _lib.ptr(p), B, H, W, float(stride), float(anchor_scale), _lib.dtype_code(p),
            _lib.LAYOUT_NHWC if nhwc else _lib.LAYOUT_NCHW, _lib.ptr(out), _lib.stream_ptr(p.device)))
    return out


def _conv_relu(cin, cout):
    return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=(3, 3), stride=(1, 1), padding=(1, 1), bias=True),
                         nn.ReLU(inplace=True))


class PyramidPred(tuple):
    """the (fam_cls, fam_bbox, odm_cls, odm_bbox, refine_anchor) per-level lists of forward(), plus the
    pyramid-packed buffers they are views of (for the fused candidate selection)"""

    def __new__(cls, layout, odm_cls, odm_bbox, anchors, *lists):
        self = super().__new__(cls, lists)
        self.packed = (layout, odm_cls, odm_bbox, anchors)
        return self


class S2ANetHead(nn.Module):
    # opt-in e4m3 tower route (s2anet_amd/fp8.py: calibrate_fp8 / fp8_towers); plain attributes, not buffers
    fp8_enabled = False
    fp8_scales = None

    def __init__(self, num_classes, in_channels=256, feat_channels=256, stacked_convs=2,
                 with_orconv=True, anchor_scales=(4,), featmap_strides=(8, 16, 32, 64, 128),
                 score_thres_before_nms=0.05, iou_thres_nms=0.5, max_before_nms_per_level=2000,
                 max_per_img=2000, compute_fam_cls=True):
        super().__init__()
        assert len(anchor_scales) == 1, "S2ANet uses one square anchor per position (head.py:66-68)"
        self.num_classes = num_classes
        self.in_channels, self.feat_channels = in_channels, feat_channels
        self.stacked_convs, self.with_orconv = stacked_convs, with_orconv
        self.anchor_scale = float(anchor_scales[0])
        self.featmap_strides = tuple(featmap_strides)
        self.score_thres_before_nms = score_thres_before_nms
        self.iou_thres_nms = iou_thres_nms
        self.max_before_nms_per_level = max_before_nms_per_level
        self.max_per_img = max_per_img
        self.compute_fam_cls = compute_fam_cls      # the reference always evaluates it (head.py:306)
        # loss settings (head.py:82-135): plain attributes, not buffers, so that the state_dict stays the reference's
        self.imgs_size = (1024, 1024)
        self.fl_gamma, self.fl_alpha = LOSS_DEFAULTS["fl_gamma"], LOSS_DEFAULTS["fl_alpha"]
        self.smoothL1_beta = LOSS_DEFAULTS["smoothL1_beta"]
        self.FPN_balance = LOSS_DEFAULTS["FPN_balance"]
        self.reg_balance, self.odm_balance = LOSS_DEFAULTS["reg_balance"], LOSS_DEFAULTS["odm_balance"]
        fam_reg, fam_cls, odm_reg, odm_cls = [], [], [], []
        for i in range(stacked_convs):
            cin = in_channels if i == 0 else feat_channels
            fam_reg.append(_conv_relu(cin, feat_channels))
            fam_cls.append(_conv_relu(cin, feat_channels))
            odm_reg.append(_conv_relu(feat_channels, feat_channels))
            c0 = feat_channels // 8 if (i == 0 and with_orconv) else feat_channels
            odm_cls.append(_conv_relu(c0, feat_channels))
        self.fam_reg_ls, self.fam_cls_ls = nn.Sequential(*fam_reg), nn.Sequential(*fam_cls)
        self.fam_reg_head = nn.Conv2d(feat_channels, 5, kernel_size=(1, 1), padding=0, bias=True)
        self.fam_cls_head = nn.Conv2d(feat_channels, num_classes, kernel_size=(1, 1), padding=0, bias=True)
        self.align_conv = AlignConv(feat_channels, feat_channels, kernel_size=3)
        if with_orconv:
            self.or_conv = ORConv2d(feat_channels, feat_channels // 8, kernel_size=3, padding=1, arf_config=(1, 8))
            self.or_pool = RotationInvariantPooling(feat_channels, 8)
        else:
            self.or_conv = nn.Conv2d(feat_channels, feat_channels, 3, padding=1)
        self.odm_reg_ls, self.odm_cls_ls = nn.Sequential(*odm_reg), nn.Sequential(*odm_cls)
        self.odm_cls_head = nn.Conv2d(feat_channels, num_classes, kernel_size=(3, 3), padding=1, bias=True)
        self.odm_reg_head = nn.Conv2d(feat_channels, 5, kernel_size=(3, 3), padding=1, bias=True)
        self.init_weights()

    def init_weights(self):
        """head.py:230-258: N(0, 0.01) everywhere, classification biases = -log((1-p)/p), p = 0.01"""
        bias_cls = float(-math.log((1 - 0.01) / 0.01))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.align_conv.init_weights()
        nn.init.constant_(self.fam_cls_head.bias, bias_cls)
        nn.init.constant_(self.odm_cls_head.bias, bias_cls)

    # ------------------------------------------------------------------ forward
    def forward_single(self, x, stride):
        """one FPN level (head.py:296-348) -> (fam_cls, fam_bbox, odm_cls, odm_bbox, refine_anchor)"""
        fam_bbox_pred = self.fam_reg_head(self.fam_reg_ls(x))
        fam_cls_pred = self.fam_cls_head(self.fam_cls_ls(x)) if self.compute_fam_cls else None
        refine_anchor = fam_refine_anchors(fam_bbox_pred.detach(), stride, self.anchor_scale)   # [B,H,W,5]
        or_feat = self.or_conv(self.align_conv(x, refine_anchor, stride))
        odm_cls_feat = self.or_pool(or_feat) if self.with_orconv else or_feat
        odm_cls_pred = self.odm_cls_head(self.odm_cls_ls(odm_cls_feat))
        odm_bbox_pred = self.odm_reg_head(self.odm_reg_ls(or_feat))
        return fam_cls_pred, fam_bbox_pred, odm_cls_pred, odm_bbox_pred, refine_anchor

    # ------------------------------------------------------------------ all levels per launch
    def pyramid_ok(self, x):
        from .fused import FusedConv2d
        return (x.is_cuda and x.dtype == torch.float16 and not torch.is_grad_enabled() and self.with_orconv and
                isinstance(self.fam_reg_head, FusedConv2d) and self.in_channels % 64 == 0 and
                self.feat_channels % 64 == 0 and self.align_conv.kernel_size == (3, 3))

    def forward_pyramid(self, layout, x, anchors=None, trace=None):
        """forward_single for ALL FPN levels at once on a pyramid-packed feature buffer x[P,256]
        (s2anet_amd/pyramid.py).  Returns per-level lists of views with the forward_single shapes.
        anchors: refined anchors [P,5] f32 to sample with instead of the ones decoded from this call's own FAM
        regression (tests: separates the sampling from the regression that feeds it); trace: dict that receives
        the packed intermediate buffers by name (tests / scripts/f16_fixture_diag.py)"""
        from . import pyramid as P

        wino = P.wino_enabled()

        # opt-in e4m3 route of the plain 256 -> 256 tower launches (s2anet_amd/fp8.py): per-tensor activation scales fixed at
        # calibration (host floats: nothing is read back)
        fp8 = self.fp8_scales if self.fp8_enabled else None

        def tower(seq, t, name=None):
            for i, blk in enumerate(seq):
                if wino and blk[0].wino_ok() and blk[0].in_channels >= 128:     # Winograd F(2,3) along x (wino_ops.hip)
                    w, b, o = blk[0].packed_args_wino()
                    t = P.conv3x3_wino(layout, t, w, b, o, relu=True)
                else:
                    w, b, o = blk[0].packed_args()
                    t = P.conv3x3(layout, t, w, b, o, relu=True)
                if trace is not None and name is not None:
                    trace[f"{name}{i}"] = t
            return t

        def quantize(t, name):
            return P.quantize_e4m3(t, 1.0 / fp8[name])

        def tower_fp8(blk, tq, name, in_name, out_name=None):
            """one tower layer on the e4m3 kernel: tq quantised with fp8[in_name]; out_name: write e4m3 with that scale
            (the next fp8 layer's input) instead of f16"""
            w, sc, b, o = blk[0].packed_args_fp8(fp8[in_name])
            t = P.conv3x3_fp8(layout, tq, w, sc, b, o, relu=True, out_e4m3=out_name is not None,
                              out_inv_scale=1.0 if out_name is None else 1.0 / fp8[out_name])
            if trace is not None:
                trace.update({f"fp8.{name}.in": tq, f"fp8.{name}.scale": sc, f"fp8.{name}.out": t})
            return t

        def tower_with_head(seq, head, t):
            """the tower's last 3x3 layer and the 1x1 head that is its only reader: one launch"""
            fusable = (head.kernel_size == (1, 1) and head.out_channels <= 32 and seq[-1][0].out_channels == 256 and
                       seq[-1][0].in_channels % 64 == 0 and not os.environ.get("S2A_NO_FUSED_HEAD"))
            if not fusable:
                w, b, o = head.packed_args()
                return P.conv1x1(tower(seq, t), w, b, o, relu=False)
            t = tower(seq[:-1], t)
            w, b, o = seq[-1][0].packed_args()
            hw, hb, _ = head.packed_args()
            return P.conv3x3_head(layout, t, w, b, o, hw, hb, relu=True)

        fam_cls = None
        if fp8 is not None:      # x quantised once for both FAM towers; their second layers stay the fused f16 3x3 + 1x1 launch
            xq = quantize(x, "x")
            fam_bbox = tower_with_head(self.fam_reg_ls[1:], self.fam_reg_head, tower_fp8(self.fam_reg_ls[0], xq, "fam_reg_ls.0", "x"))
            if self.compute_fam_cls:
                fam_cls = tower_with_head(self.fam_cls_ls[1:], self.fam_cls_head,
                                          tower_fp8(self.fam_cls_ls[0], xq, "fam_cls_ls.0", "x"))
        else:
            fam_bbox = tower_with_head(self.fam_reg_ls, self.fam_reg_head, x)               # [P,64], 5 used
            if self.compute_fam_cls:
                fam_cls = tower_with_head(self.fam_cls_ls, self.fam_cls_head, x)
        own_anchors = P.fam_refine_anchors(layout, fam_bbox, self.anchor_scale)             # [P,5] f32
        if anchors is None:
            anchors = own_anchors
        else:
            assert anchors.shape == own_anchors.shape and anchors.dtype == torch.float32 and anchors.is_contiguous()
        if getattr(self, "capture", None) is not None:      # bench.py: the operands of this step's launches
            self.capture.update(layout=layout, x=x, anchors=anchors)
        al = P.align_conv(layout, x, anchors, self.align_conv.packed_weight(torch.float16), self.feat_channels)
        wa = self.or_conv.rotate_arf()      # the cached expansion (keyed on the 5-D parameter), in train() mode as well
        orc = self.or_conv.packed_cache()
        if self.or_pool.nOrientation == 8 and wa.shape[0] % 64 == 0 and wino and wa.shape[1] % 32 == 0:
            or_feat, pooled = P.conv3x3_wino(layout, al, orc.get_wino(wa),
                                             orc.get_bias(self.or_conv.bias, wa.shape[0]), wa.shape[0],
                                             relu=False, pool=True)
        elif self.or_pool.nOrientation == 8 and wa.shape[0] % 64 == 0:                      # conv + orientation max, one launch
            or_feat, pooled = P.orconv_pool(layout, al, orc.get(wa),
                                            orc.get_bias(self.or_conv.bias, wa.shape[0]), wa.shape[0])
        else:
            or_feat = P.conv3x3(layout, al, orc.get(wa),
                                orc.get_bias(self.or_conv.bias, wa.shape[0]), wa.shape[0], relu=False)
            pooled = P.rot_inv_pool(or_feat, self.or_pool.nOrientation)                     # [P,32]
        # the real map counts: up to 16 maps run on 16 filter rows (pyramid.conv3x3); the buffers stay 64 columns wide
        if fp8 is not None:
            # the 32 -> 256 layer stays f16 and its output is quantised; odm_reg_ls[0] hands e4m3 straight to odm_reg_ls[1]
            cls_t = tower_fp8(self.odm_cls_ls[1], quantize(tower(self.odm_cls_ls[:1], pooled, "odm_cls_ls"), "odm_cls_ls0"),
                              "odm_cls_ls.1", "odm_cls_ls0")
            reg_q = tower_fp8(self.odm_reg_ls[0], quantize(or_feat, "or_feat"), "odm_reg_ls.0", "or_feat", "odm_reg_ls0")
            reg_t = tower_fp8(self.odm_reg_ls[1], reg_q, "odm_reg_ls.1", "odm_reg_ls0")
        else:
            cls_t = tower(self.odm_cls_ls, pooled, "odm_cls_ls")
            reg_t = None      # (the f16 route keeps its launch order: the regression tower follows the classification head)
        w, b, _ = self.odm_cls_head.packed_args()
        odm_cls = P.conv3x3(layout, cls_t, w, b, self.odm_cls_head.out_channels, relu=False)    # [P,64], C used
        if reg_t is None:
            reg_t = tower(self.odm_reg_ls, or_feat, "odm_reg_ls")
        w, b, _ = self.odm_reg_head.packed_args()
        odm_bbox = P.conv3x3(layout, reg_t, w, b, self.odm_reg_head.out_channels, relu=False)  # [P,64], 5 used
        n = len(layout.sizes)
        if trace is not None:
            trace.update(x=x, fam_bbox=fam_bbox, fam_cls=fam_cls, own_anchors=own_anchors, anchors=anchors, align=al,
                         or_feat=or_feat, pooled=pooled, odm_cls=odm_cls, odm_bbox=odm_bbox)
        return PyramidPred(layout, odm_cls, odm_bbox, anchors,
                           [layout.level(fam_cls, l, self.num_classes) for l in range(n)] if fam_cls is not None else [None] * n,
                [layout.level(fam_bbox, l, 5) for l in range(n)],
                [layout.level(odm_cls, l, self.num_classes) for l in range(n)],
                [layout.level(odm_bbox, l, 5) for l in range(n)],
                [layout.rows(anchors, l).view(layout.batch, *layout.sizes[l], 5) for l in range(n)])

    def forward(self, feats, targets=None, imgs_size=None, post_process=False):
        """head.py:261-293.  targets[N,7] = (image, class, x, y, w, h, angle) with x, y, w, h normalised: scaled to
        pixels IN PLACE by imgs_size (h, w) as the reference does, then compute_loss fills "loss" / "loss_items".
        A bool in the second place is post_process (the earlier forward(feats, post_process) form)."""
        if isinstance(targets, bool):
            targets, post_process = None, targets
        per_level = [self.forward_single(f, s) for f, s in zip(feats, self.featmap_strides)]
        p = tuple(map(list, zip(*per_level)))
        results = {"loss": None, "loss_items": None, "boxes_ls": None, "pred": None}
        if targets is not None:
            if imgs_size is None:
                raise ValueError("forward(feats, targets) needs imgs_size to scale the targets to pixels")
            self.imgs_size = tuple(int(v) for v in imgs_size)
            targets[:, [2, 4]] = targets[:, [2, 4]] * imgs_size[1]
            targets[:, [3, 5]] = targets[:, [3, 5]] * imgs_size[0]
            results["loss"], results["loss_items"] = self.compute_loss(p, targets)
        if post_process:
            results["boxes_ls"] = self.get_bboxes(p)
        if targets is None and not post_process:
            results["pred"] = p
        return results

    # ------------------------------------------------------------------ loss (head.py:353-646)
    def init_grid_anchors(self, featmap_sizes, device):
        """the reference's p[4]: per-level grid anchors [H*W,5] f32 (models/anchors.py:75-126)"""
        return [grid_anchors(hw, s, self.anchor_scale, device) for hw, s in zip(featmap_sizes, self.featmap_strides)]

    def _loss_pred(self, p):
        """this library's 5-list p (refined anchors at p[4]) or the reference's 6-list (grid anchors at p[4], refined
        anchors at p[5]) -> the 6-list"""
        p = list(p)
        if len(p) == 5:
            sizes = [tuple(b.shape[2:]) for b in p[1]]
            p = p[:4] + [self.init_grid_anchors(sizes, p[1][0].device), p[4]]
        if len(p) != 6:
            raise ValueError(f"p must be the 5 per-level lists of forward() or the reference's 6, got {len(p)}")
        if any(t is None for t in p[0]):
            raise ValueError("compute_loss needs the FAM classification: this head was built with compute_fam_cls=False")
        return p

    def assign_labels_fam_odm(self, p, targets):
        """head.py:439-537 for the whole batch: -> (assign_ids int64 [2,B,A] (FAM, ODM; levels concatenated per image),
        targets sorted by image [N,7] f32, row offsets int64 [B+1]).  One host synchronisation (the per-image target
        counts), then 2*B assign_labels calls."""
        p = self._loss_pred(p)
        B = p[1][0].shape[0]
        dev = p[1][0].device
        init_all = torch.cat([a.reshape(-1, 5) for a in p[4]], 0).float()
        refine_all = torch.cat([a.reshape(B, -1, 5) for a in p[5]], 1).detach().float()
        t = targets.detach().float().reshape(-1, 7)
        img = t[:, 0].long()
        order = torch.argsort(img, stable=True)
        ts = t[order]
        counts_dev = torch.bincount(img, minlength=B)[:B]
        offsets = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts_dev, 0)
        counts = counts_dev.tolist()                       # the one host sync of the assignment
        fam, odm, start = [], [], 0
        for b in range(B):
            gt = ts[start:start + counts[b], 2:7]
            start += counts[b]
            fam.append(assign_labels(init_all, gt, imgs_size=self.imgs_size))
            odm.append(assign_labels(refine_all[b], gt, imgs_size=self.imgs_size))
        return torch.stack([torch.stack(fam), torch.stack(odm)]), ts, offsets

    def _core_loss(self, p, ids, ts, offsets):
        return s2anet_loss(p[0], p[1], p[2], p[3], p[4], p[5], ids, ts, offsets, fl_gamma=self.fl_gamma,
                           fl_alpha=self.fl_alpha, smoothL1_beta=self.smoothL1_beta, FPN_balance=self.FPN_balance,
                           reg_balance=self.reg_balance, odm_balance=self.odm_balance)

    def compute_loss_device(self, p, targets, num_targets=None, pair_capacity=None):
        """compute_loss without any host read: the capturable form.  targets [G,7] in any order, rows with an image index
        outside [0, B) are padding (a static table of a replayed graph); num_targets: optional int64 device scalar, only
        the first num_targets rows take part.  One fixed launch sequence: the batched assignment of both modules and all
        images (assign_labels_batched), then the fused loss.
        -> (loss [1] f32, items [4] f32 = fam_cls, fam_reg, odm_cls, odm_reg, status [4] int64), all on the device.
        status[0] != 0 means the result is NOT valid: bit 0 = the assignment's pair list was too small (status[1] is the
        pair_capacity that fits), bit 1 = a per-image limit was exceeded; status[2] = target rows that took part."""
        p = self._loss_pred(p)
        B = p[1][0].shape[0]
        init_all = torch.cat([a.reshape(-1, 5) for a in p[4]], 0)
        refine_all = torch.cat([a.reshape(B, -1, 5) for a in p[5]], 1).detach()
        ids, ts, offsets, status = assign_labels_batched((init_all, refine_all), targets, B, imgs_size=self.imgs_size,
                                                         num_targets=num_targets, pair_capacity=pair_capacity)
        loss, items = self._core_loss(p, ids, ts, offsets)
        return loss, items, status

    def compute_loss(self, p, targets):
        """head.py:353-436: p = forward()'s 5 lists or the reference's 6; targets[N,7] (image, class, x, y, w, h,
        angle) in pixels / rad -> (loss [1] f32, loss_items float32 numpy [4] = fam_cls, fam_reg, odm_cls, odm_reg).
        One host sync: the loss_items read-back, which brings the assignment's status with it.  A pair list that was too
        small (status bit 0) costs one more run at the capacity the first one reported; a per-image limit (bit 1) or
        S2A_ASSIGN_BATCHED=0 takes the per-image route (assign_labels_fam_odm: a second sync and 2*B assign_labels
        calls)."""
        p = self._loss_pred(p)
        capacity = None
        while os.environ.get("S2A_ASSIGN_BATCHED", "1") != "0":
            loss, items, status = self.compute_loss_device(p, targets, pair_capacity=capacity)
            host = torch.cat([items.detach().double(), status.double()]).cpu().numpy()     # the one host sync
            flags = int(host[4])
            if flags == 0:
                return loss, host[:4].astype(np.float32)
            if flags & 2 or capacity is not None:
                break
            capacity = int(host[5])
        ids, ts, offsets = self.assign_labels_fam_odm(p, targets)
        loss, items = self._core_loss(p, ids, ts, offsets)
        return loss, items.detach().cpu().numpy()

    # ------------------------------------------------------------------ decode + NMS, batched
    def candidates(self, p, raw_logits=False):
        """per-level sigmoid + top-k (head.py:697-705), levels concatenated (head.py:712-714),
        final decode (head.py:717).  -> bboxes[B,n,5] f32, scores[B,n,C] f32 with n <= 5344"""
        odm_cls, odm_bbox, anchors = p[2], p[3], p[4]
        k = self.max_before_nms_per_level
        sc_l, bb_l, an_l = [], [], []
        for cls, reg, anc in zip(odm_cls, odm_bbox, anchors):
            B = cls.shape[0]
            s = cls.detach().permute(0, 2, 3, 1).reshape(B, -1, self.num_classes)
            s = s.float() if raw_logits else s.sigmoid()   # raw_logits: calibration only (same ranking)
            d = reg.detach().permute(0, 2, 3, 1).reshape(B, -1, 5)
            a = anc.reshape(B, -1, 5)
            if k > 0 and s.shape[1] > k:
                top = s.max(dim=2)[0].topk(k, dim=1)[1]
                s = s.gather(1, top[..., None].expand(-1, -1, self.num_classes))
                d = d.gather(1, top[..., None].expand(-1, -1, 5))
                a = a.gather(1, top[..., None].expand(-1, -1, 5))
            sc_l.append(s.float())
            bb_l.append(d.float())
            an_l.append(a)
        scores, deltas, anc = torch.cat(sc_l, 1), torch.cat(bb_l, 1), torch.cat(an_l, 1)
        B, n = scores.shape[:2]
        bboxes = delta2bbox_rotated(anc.reshape(-1, 5), deltas.reshape(-1, 5)).reshape(B, n, 5)
        return bboxes, scores

    def get_bboxes_batched(self, p, max_candidates=None, return_overflow=False, **nms_kw):
        """-> dets[B,max_per_img,6], labels[B,max_per_img] (-1 padded), counts[B]; no host sync.
        return_overflow: fourth result int64[2] = [NMS candidates found, candidates dropped by max_candidates];
        nms_kw: dropped_total / return_wire of batched_multiclass_nms_rotated"""
        fused = None
        if isinstance(p, PyramidPred) and not os.environ.get("S2A_NO_FUSED_CANDIDATES"):
            from . import pyramid as P
            layout, cls, reg, anc = p.packed
            fused = P.candidates(layout, cls, reg, anc, self.num_classes, self.max_before_nms_per_level)
        bboxes, scores = fused[:2] if fused is not None else self.candidates(p)
        return batched_multiclass_nms_rotated(bboxes, scores, self.score_thres_before_nms,
                                              self.iou_thres_nms, self.max_per_img, max_candidates, return_overflow,
                                              **nms_kw)

    def get_bboxes(self, p):
        """reference return shape (head.py:648-682): list of (det_bboxes[K,6], det_labels[K]) per image"""
        bboxes, scores = self.candidates(p)
        return [multiclass_nms_rotated(bboxes[b], scores[b], self.score_thres_before_nms,
                                       self.iou_thres_nms, self.max_per_img)
                for b in range(bboxes.shape[0])]
