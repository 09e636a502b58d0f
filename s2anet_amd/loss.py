"""S2ANet training loss (models/head.py:353-646): FAM + ODM focal classification and smooth-L1 regression.

``s2anet_loss`` is the capture-safe core: one autograd Function over both modules, all levels and all images
(csrc/loss_ops.hip).  Forward = 2 launches, backward = 1 launch, no host synchronisation: the positive counts, the
max(npos, B) normalisers and the balances stay on the device.  The assignment and the image sort of the targets come
from ``assign_labels_batched`` (s2a_assign_labels_batched: both modules and all images in one sync-free launch sequence),
so ``S2ANetHead.compute_loss_device`` = assignment + this core is capturable as a whole and replays against new targets
written into a static table; ``S2ANetHead.assign_labels_fam_odm`` (s2a_assign_labels, one call per image and module,
one host read of the target counts) is the per-image form of the same ids.

Maps are read in their NCHW layout; a map in another layout (channels_last) is copied to NCHW first.
"""
import torch

from . import _lib

LOSS_DEFAULTS = dict(fl_gamma=2.0, fl_alpha=0.5, smoothL1_beta=1.0 / 9.0, FPN_balance=(1.0, 1.0, 1.0, 1.0, 1.0),
                     reg_balance=1.0, odm_balance=1.0)


def grid_anchors(featmap_size, stride, scale=4.0, device=None):
    """AnchorGeneratorRotated.gen_grid_anchors (models/anchors.py:75-126), one square anchor per position, angle 0:
    -> [H*W, 5] f32, row-major over (y, x)"""
    H, W = featmap_size
    xs = torch.arange(W, dtype=torch.float32, device=device) * float(stride) + 0.5 * (stride - 1)
    ys = torch.arange(H, dtype=torch.float32, device=device) * float(stride) + 0.5 * (stride - 1)
    out = torch.zeros((H, W, 5), dtype=torch.float32, device=device)
    out[..., 0] = xs[None, :]
    out[..., 1] = ys[:, None]
    out[..., 2:4] = float(scale * stride)
    return out.reshape(-1, 5)


def _nchw(t):
    return t if t.is_contiguous() else t.contiguous()


class S2ANetLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, settings, n_levels, *tensors):
        L = n_levels
        maps = [_nchw(t) for t in tensors[:4 * L]]              # fam_cls, fam_bbox, odm_cls, odm_bbox (L each)
        anchors = tensors[4 * L:6 * L]                           # init (L), refine (L)
        assign_ids, targets, offsets = tensors[6 * L:6 * L + 3]
        dev = maps[0].device
        B, C = maps[0].shape[0], maps[0].shape[1]
        A = sum(m.shape[2] * m.shape[3] for m in maps[:L])
        if assign_ids.shape != (2, B, A) or assign_ids.dtype != torch.int64:
            raise ValueError(f"assign_ids must be int64 [2, {B}, {A}], got {tuple(assign_ids.shape)} {assign_ids.dtype}")
        if offsets.shape != (B + 1,) or offsets.dtype != torch.int64:
            raise ValueError(f"target_offsets must be int64 [{B + 1}]")
        ids = assign_ids.contiguous()
        tg = targets.detach().float().contiguous().reshape(-1, 7)
        grads = [torch.empty(m.shape, dtype=torch.float32, device=dev) for m in maps]
        anc = [a.detach().float().contiguous() for a in anchors]
        p = _lib.LossParams()
        p.batch, p.num_classes, p.n_levels = B, C, L
        p.fl_gamma, p.fl_alpha, p.smooth_l1_beta = settings["fl_gamma"], settings["fl_alpha"], settings["smoothL1_beta"]
        p.reg_balance, p.odm_balance = settings["reg_balance"], settings["odm_balance"]
        fpn = settings["FPN_balance"]
        for m in range(2):
            for l in range(L):
                cls, bbox = maps[(2 * m) * L + l], maps[(2 * m + 1) * L + l]
                Bc, Cc, H, W = cls.shape
                if (Bc, Cc) != (B, C) or bbox.shape != (B, 5, H, W):
                    raise ValueError(f"module {m} level {l}: cls {tuple(cls.shape)} / bbox {tuple(bbox.shape)} do not match")
                a = anc[m * L + l]
                if a.numel() == H * W * 5:
                    stride = 0
                elif a.numel() == B * H * W * 5:
                    stride = H * W * 5
                else:
                    raise ValueError(f"module {m} level {l}: anchors {tuple(a.shape)} are neither [H*W,5] nor [B,H,W,5]")
                e = p.map[m][l]
                e.cls, e.bbox, e.anchors = _lib.ptr(cls), _lib.ptr(bbox), _lib.ptr(a)
                e.grad_cls, e.grad_bbox = _lib.ptr(grads[(2 * m) * L + l]), _lib.ptr(grads[(2 * m + 1) * L + l])
                e.anchor_batch_stride, e.height, e.width = stride, H, W
                e.cls_dtype, e.bbox_dtype = _lib.dtype_code(cls), _lib.dtype_code(bbox)
                e.fpn_balance = float(fpn[l])
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        items = torch.empty((4,), dtype=torch.float32, device=dev)
        norm = torch.empty((4,), dtype=torch.float32, device=dev)
        lib = _lib.lib()
        with torch.cuda.device(dev):
            ws = _lib.workspace(lib.s2a_s2anet_loss_workspace_bytes(B, A), dev, "loss")
            _lib.check(lib.s2a_s2anet_loss_forward(p, _lib.ptr(ids), _lib.ptr(tg) if tg.numel() else None,
                                                   _lib.ptr(offsets.contiguous()), _lib.ptr(loss), _lib.ptr(items),
                                                   _lib.ptr(norm), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        ctx.mark_non_differentiable(items)
        ctx.n_levels = L
        ctx.dtypes = [m.dtype for m in maps]
        ctx.save_for_backward(norm, *grads)
        return loss, items

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, grad_items):
        norm, *grads = ctx.saved_tensors
        L = ctx.n_levels
        dev = norm.device
        want = ctx.needs_input_grad[2:2 + 4 * L]
        outs = [None] * (4 * L)
        table = (_lib.LossGradMap * (4 * L))()
        n = 0
        for j in range(4 * L):
            if not want[j]:
                continue
            outs[j] = torch.empty(grads[j].shape, dtype=ctx.dtypes[j], device=dev)
            e = table[n]
            e.src, e.dst, e.numel = _lib.ptr(grads[j]), _lib.ptr(outs[j]), grads[j].numel()
            e.dtype, e.norm_index = _lib.dtype_code(outs[j]), j // L         # fam cls, fam bbox, odm cls, odm bbox
            n += 1
        if n:
            g = grad_loss.detach().float().contiguous()
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().s2a_s2anet_loss_backward(table, n, _lib.ptr(g), _lib.ptr(norm), _lib.stream_ptr(dev)))
        return (None, None, *outs) + (None,) * (2 * L + 3)


def s2anet_loss(fam_cls, fam_bbox, odm_cls, odm_bbox, init_anchors, refine_anchors, assign_ids, targets, target_offsets,
                fl_gamma=2.0, fl_alpha=0.5, smoothL1_beta=1.0 / 9.0, FPN_balance=(1.0, 1.0, 1.0, 1.0, 1.0),
                reg_balance=1.0, odm_balance=1.0):
    """the reference's compute_loss after assignment (models/head.py:383-436), all on the device.

    fam_cls / odm_cls: per-level [B,C,H,W] logits, fam_bbox / odm_bbox: per-level [B,5,H,W] (f32 or f16, computed in
    f32); init_anchors: per-level [H*W,5] grid anchors (or [B,H,W,5]); refine_anchors: per-level [B,H,W,5];
    assign_ids: int64 [2,B,A] (FAM, ODM; levels concatenated per image; -2 ignore, -1 negative, >= 0 gt index within the
    image); targets: [G,7] (image, class, x, y, w, h, angle) in px / rad, sorted by image; target_offsets: int64 [B+1]
    row offsets of each image's targets.
    -> (loss [1], items [4] = fam_cls, fam_reg, odm_cls, odm_reg), f32 device tensors; gradients go to the four
    prediction lists only, in each map's dtype"""
    lists = (fam_cls, fam_bbox, odm_cls, odm_bbox, init_anchors, refine_anchors)
    L = len(fam_cls)
    if any(len(x) != L for x in lists):
        raise ValueError("every per-level list must have the same length")
    if not 0 < L <= _lib.LOSS_MAX_LEVELS or len(FPN_balance) < L:
        raise ValueError(f"1..{_lib.LOSS_MAX_LEVELS} levels with one FPN_balance each")
    if any(t is None for x in lists[:4] for t in x):
        raise ValueError("s2anet_loss needs all four prediction lists (fam_cls is None when the head was built "
                         "with compute_fam_cls=False)")
    flat = [t for x in lists for t in x] + [assign_ids, targets, target_offsets]
    _lib.require_cuda(*flat)
    settings = dict(fl_gamma=float(fl_gamma), fl_alpha=float(fl_alpha), smoothL1_beta=float(smoothL1_beta),
                    FPN_balance=tuple(float(f) for f in FPN_balance), reg_balance=float(reg_balance),
                    odm_balance=float(odm_balance))
    return S2ANetLossFunction.apply(settings, L, *flat)
