"""Differentiable restatements of this package's composed modules in stock torch ops -- TEST INFRASTRUCTURE ONLY.

Every function takes its weights and inputs as arguments plus a ``dtype`` (float64 by default) that every step runs in.
In float64 the result and, through autograd, every gradient are the reference of tests/test_gpu_autograd_twin.py; the
same code in float32 / float16 is the stock-op baseline whose own distance from float64 sizes that test's bounds.
Nothing here calls into s2anet_amd: the functions are written from the module definitions (s2anet_amd/fused.py,
detector.py, orn.py, alignconv.py, head.py), so a link that production loses under autograd does not cancel out.

Parameter containers:
  conv        (weight, bias) -- bias may be None
  bottleneck  {"conv1": conv, "conv2": conv, "conv3": conv, "stride": int, "down": conv or None}   (BN folded)
  fpn         {"lateral": [conv, ...], "fpn": [conv, ...]}   (the entries past len(lateral) are the stride-2 extras)
  head        {state-dict name: tensor} of S2ANetHead, "or_conv.indices" included
  trunk       {"stem": conv, "stages": [[bottleneck, ...], ...]}
"""
import torch
import torch.nn.functional as F

from .dcn64 import deform_conv64

_F64 = torch.float64


def _t(v, dtype):
    return None if v is None else v.to(dtype)


class Decisions:
    """The branch every ReLU / max of one twin run takes, in call order, and where they come from.

    A ReLU whose pre-activation lies within the rounding error of zero, or a max whose two largest candidates lie that
    close together, has no branch that a lower-precision computation must take: either one is a correct result, and one
    such entry moves a gradient by far more than rounding (1e-3 of its norm for one entry of a head tower).  A run with
    `given` decisions (another run's `taken`) therefore follows them
      * only inside the band |pre-activation| <= band * rms(tensor) (for a max: top-two gap <= band * rms) when `band`
        is a number -- outside it the run keeps its own branch and counts in `disagree` how often `given` differs, which a
        test asserts to be zero;
      * everywhere when `band` is None (a lower-precision baseline that is to share the reference's branches).
    `followed` counts the in-band entries where the given branch differed from the run's own."""

    def __init__(self, given=None, band=None):
        self.given, self.band = given, band
        self.taken, self.disagree, self.followed = [], 0, 0

    def _resolve(self, own, margin, scale):
        if self.given is not None:
            g = self.given[len(self.taken)].to(own.device)
            assert g.shape == own.shape, (len(self.taken), tuple(g.shape), tuple(own.shape))
            if self.band is None:
                own = g
            else:
                amb = margin <= self.band * scale
                diff = (own != g) & (margin > 0)        # an exact tie (a window of zeros behind a ReLU) is no decision
                self.disagree += int((diff & ~amb).sum())
                self.followed += int((diff & amb).sum())
                own = torch.where(amb, g, own)
        self.taken.append(own)
        return own

    def relu(self, y):
        d = y.detach()
        mask = self._resolve(d > 0, d.abs(), d.double().pow(2).mean().sqrt())
        return y * mask.to(y.dtype)

    def select(self, cand):
        """max over the LAST dim of cand [..., k] (entries may be -inf padding)"""
        d = cand.detach()
        top = d.topk(2, -1)
        idx = self._resolve(top.indices[..., 0], top.values[..., 0] - top.values[..., 1],
                            d[torch.isfinite(d)].double().pow(2).mean().sqrt())
        return cand.gather(-1, idx.unsqueeze(-1)).squeeze(-1)


_DEC = None


class decisions:
    """with decisions(Decisions(...)): every ReLU / max of the twin functions goes through it"""

    def __init__(self, dec):
        self.dec = dec

    def __enter__(self):
        global _DEC
        self.prev, _DEC = _DEC, self.dec
        return self.dec

    def __exit__(self, *a):
        global _DEC
        _DEC = self.prev


def _relu(y):
    return F.relu(y) if _DEC is None else _DEC.relu(y)


def _windows(x, k, stride, pad):
    """x [B,C,H,W] -> the k*k candidates of every pooling window [B,C,Ho,Wo,k*k], -inf outside the image"""
    xp = F.pad(x, (pad, pad, pad, pad), value=float("-inf"))
    return xp.unfold(2, k, stride).unfold(3, k, stride).flatten(-2)


def _max_pool(x, k, stride, pad):
    return F.max_pool2d(x, k, stride, pad) if _DEC is None else _DEC.select(_windows(x, k, stride, pad))


def fused_conv(x, w, b=None, stride=1, pad=0, relu=False, residual=None, dtype=_F64):
    """relu?(conv2d(x, w, b) + residual)  (FusedConv2d)"""
    y = F.conv2d(_t(x, dtype), _t(w, dtype), _t(b, dtype), stride, pad)
    if residual is not None:
        y = y + _t(residual, dtype)
    return _relu(y) if relu else y


def bottleneck_folded(x, params, dtype=_F64):
    """BottleNeck after fold_batchnorm: relu(conv3(relu(conv2(relu(conv1(x))))) + residual), residual = x or the
    downsample conv of x (no ReLU)"""
    x = _t(x, dtype)
    st = params["stride"]
    out = fused_conv(x, *params["conv1"], 1, 0, True, dtype=dtype)
    out = fused_conv(out, *params["conv2"], st, 1, True, dtype=dtype)
    res = x if params.get("down") is None else fused_conv(x, *params["down"], st, 0, False, dtype=dtype)
    return fused_conv(out, *params["conv3"], 1, 0, True, res, dtype=dtype)


def trunk_folded(imgs, params, out_indices=(2, 3, 4), dtype=_F64):
    """DetectorBackbone after fold_batchnorm: relu(conv 7x7/2/pad 3) -> max-pool 3x3/2/pad 1 -> the stages; returns the
    outputs of the stages in out_indices (stage 1 is the first)"""
    x = fused_conv(imgs, *params["stem"], 2, 3, True, dtype=dtype)
    x = _max_pool(x, 3, 2, 1)
    outs = []
    for i, stage in enumerate(params["stages"], 1):
        for blk in stage:
            x = bottleneck_folded(x, blk, dtype)
        if i in out_indices:
            outs.append(x)
    return tuple(outs)


def fpn(inputs, params, dtype=_F64):
    """FPN.forward: 1x1 laterals, top-down nearest-2x adds, 3x3 output convs, stride-2 3x3 extras (the first on the
    last INPUT, the next on the previous extra's output, no ReLU in between)"""
    n = len(params["lateral"])
    lat = [fused_conv(inputs[i], *params["lateral"][i], dtype=dtype) for i in range(n)]
    for i in range(n - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], scale_factor=2, mode="nearest")
    outs = [fused_conv(lat[i], *params["fpn"][i], 1, 1, dtype=dtype) for i in range(n)]
    for i in range(n, len(params["fpn"])):
        outs.append(fused_conv(inputs[-1] if i == n else outs[-1], *params["fpn"][i], 2, 1, dtype=dtype))
    return tuple(outs)


def arf_expand(w5d, indices, dtype=_F64):
    """active rotating filter: w5d [O,I,nOri,kH,kW], indices uint8 [nOri,kH,kW,nRot] (1-based) ->
    [O*nRot, I*nOri, kH, kW] with out[o*nRot + k, i, indices[l, k] - 1] = w[o, i, l] over the nOri*kH*kW entries l:
    one index gather, differentiable in w5d"""
    O, I, nOri, kH, kW = w5d.shape
    nRot = indices.shape[-1]
    nE = nOri * kH * kW
    idx = indices.reshape(nE, nRot).long() - 1
    inv = torch.empty_like(idx)
    inv.scatter_(0, idx, torch.arange(nE, device=idx.device).view(nE, 1).expand(nE, nRot))   # inv[idx[l,k], k] = l
    g = _t(w5d, dtype).reshape(O, I, nE)[:, :, inv]                                          # [O,I,nE,nRot]
    return g.permute(0, 3, 1, 2).reshape(O * nRot, I * nOri, kH, kW)


def rot_pool(x, n=8, dtype=_F64):
    """RotationInvariantPooling: max over each run of n channels"""
    x = _t(x, dtype)
    if _DEC is not None:
        return _DEC.select(x.unflatten(1, (x.shape[1] // n, n)).movedim(2, -1))
    return x.unflatten(1, (x.shape[1] // n, n)).max(2)[0]


def align_offsets(anchors, stride, k=3, dtype=_F64):
    """AlignConv's sampling offsets (k_align_offsets restated): anchors [B,H,W,5] (x, y, w, h, angle; px / rad) ->
    [B, 2*k*k, H, W], channel 2t = dy, 2t + 1 = dx of tap t = ky*k + kx.  No gradient (the anchors are detached)."""
    a = anchors.detach().to(dtype)
    B, H, W, _ = a.shape
    dev = a.device
    pad = (k - 1) // 2
    t = torch.arange(k * k, device=dev)
    yy, xx = (t // k - pad).to(dtype), (t % k - pad).to(dtype)                   # [k*k]
    yc = torch.arange(H, device=dev, dtype=dtype).view(1, H, 1, 1)
    xc = torch.arange(W, device=dev, dtype=dtype).view(1, 1, W, 1)
    x_ctr, y_ctr, w, h = (a[..., i:i + 1] / stride for i in range(4))
    cs, sn = torch.cos(a[..., 4:5]), torch.sin(a[..., 4:5])
    x, y = (w / k) * xx, (h / k) * yy                                            # [B,H,W,k*k]
    off_x = (cs * x - sn * y + x_ctr) - (xc + xx)
    off_y = (sn * x + cs * y + y_ctr) - (yc + yy)
    return torch.stack([off_y, off_x], -1).reshape(B, H, W, 2 * k * k).permute(0, 3, 1, 2).contiguous()


def _offset_dtype(dtype):
    # the anchors are float32 in production whatever the feature type (pixel coordinates do not fit float16), so the
    # baseline forms the offsets in float32 too and rounds them to its own type once, as DeformConvFunction does
    return torch.float32 if dtype == torch.float16 else dtype


def align_conv(x, anchors, w, stride, dtype=_F64):
    """AlignConv.forward: relu(deform_conv(x, offsets(anchors), w)), 3 x 3, pad 1"""
    off = align_offsets(anchors, stride, 3, _offset_dtype(dtype))
    return _relu(deform_conv64(x, off, w, dtype=dtype))


def orconv_pool(x, w5d, bias, indices, pad=1, n_ori=8, dtype=_F64):
    """ORConv2d followed by RotationInvariantPooling(n_ori) -> (conv output, pooled)"""
    y = F.conv2d(_t(x, dtype), arf_expand(w5d, indices, dtype), _t(bias, dtype), 1, pad)
    return y, rot_pool(y, n_ori, dtype)


def _tower(x, P, name, dtype):
    i = 0
    while "%s.%d.0.weight" % (name, i) in P:
        x = fused_conv(x, P["%s.%d.0.weight" % (name, i)], P["%s.%d.0.bias" % (name, i)], 1, 1, True, dtype=dtype)
        i += 1
    return x


def head_single(x, stride, P, refine_anchor, dtype=_F64):
    """S2ANetHead.forward_single (with_orconv) on one level -> (fam_cls, fam_bbox, odm_cls, odm_bbox).  refine_anchor
    [B,H,W,5]: the production call's own refined anchors, detached (they carry no gradient there either), so that both
    sides sample the same points."""
    x = _t(x, dtype)
    fam_bbox = fused_conv(_tower(x, P, "fam_reg_ls", dtype), P["fam_reg_head.weight"], P["fam_reg_head.bias"], dtype=dtype)
    fam_cls = fused_conv(_tower(x, P, "fam_cls_ls", dtype), P["fam_cls_head.weight"], P["fam_cls_head.bias"], dtype=dtype)
    al = align_conv(x, refine_anchor, P["align_conv.deform_conv.weight"], stride, dtype)
    or_feat, pooled = orconv_pool(al, P["or_conv.weight"], P["or_conv.bias"], P["or_conv.indices"], dtype=dtype)
    odm_cls = fused_conv(_tower(pooled, P, "odm_cls_ls", dtype), P["odm_cls_head.weight"], P["odm_cls_head.bias"], 1, 1,
                         dtype=dtype)
    odm_bbox = fused_conv(_tower(or_feat, P, "odm_reg_ls", dtype), P["odm_reg_head.weight"], P["odm_reg_head.bias"], 1, 1,
                          dtype=dtype)
    return fam_cls, fam_bbox, odm_cls, odm_bbox


def head(feats, strides, P, refine_anchors, dtype=_F64):
    """head_single on every level -> the four per-level lists (fam_cls, fam_bbox, odm_cls, odm_bbox)"""
    per = [head_single(f, s, P, a, dtype) for f, s, a in zip(feats, strides, refine_anchors)]
    return tuple(map(list, zip(*per)))


def detector(imgs, trunk, neck, head_params, strides, refine_anchors, dtype=_F64):
    """S2ANet.forward on a float image: trunk_folded -> fpn -> head"""
    return head(fpn(trunk_folded(imgs, trunk, dtype=dtype), neck, dtype), strides, head_params, refine_anchors, dtype)


# ------------------------------------------------------------------ parameter containers from a module tree
# (attribute names only; `leaf` maps a module's tensor to the tensor the twin computes with, the identity by default)
def conv_params(m, leaf=lambda t: t):
    return (leaf(m.weight), None if m.bias is None else leaf(m.bias))


def bottleneck_params(blk, leaf=lambda t: t):
    """a BottleNeck whose BN is folded into biased convs (conv1..3, downsample[0])"""
    return {"conv1": conv_params(blk.conv1, leaf), "conv2": conv_params(blk.conv2, leaf),
            "conv3": conv_params(blk.conv3, leaf), "stride": blk.conv2.stride[0],
            "down": None if blk.downsample is None else conv_params(blk.downsample[0], leaf)}


def trunk_params(backbone, leaf=lambda t: t):
    seq = backbone.backbone
    stages = [seq[1][1]] + [seq[i] for i in range(2, len(seq))]
    return {"stem": conv_params(seq[0][0], leaf), "stages": [[bottleneck_params(b, leaf) for b in st] for st in stages]}


def fpn_params(neck, leaf=lambda t: t):
    return {"lateral": [conv_params(m, leaf) for m in neck.lateral_convs], "fpn": [conv_params(m, leaf) for m in neck.fpn_convs]}


def head_params(head, leaf=lambda t: t):
    P = {n: leaf(p) for n, p in head.named_parameters()}
    P["or_conv.indices"] = head.or_conv.indices
    return P
