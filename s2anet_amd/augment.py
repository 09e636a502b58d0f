"""The reference's S2ANet training augmentation on the device (csrc/augment_ops.hip).

The recipe (data/hyps/hyp.scratch.s2anet.yaml) enables two augmentations: a turn drawn from {-180, -90, 0, 90} degrees
(`degrees: 180`, utils/augmentations.py:93-175) and a left-right flip with probability 0.5 (utils/datasets_rotation.py:
480-492); the up-down flip of the same lines is built too.  `TrainAugment` takes the raw uint8 channels-last batch and its
polygon labels [G,10] = (image, class, x1, y1 .. x4, y4) in pixels and returns the augmented batch and the [G,7] target
table (image, class, cx, cy, w, h, theta) that `S2ANetHead.compute_loss_device` reads (pixels) or, with normalize=True,
`S2ANet.forward(imgs, targets)` (normalised).  The draw runs on the device from a Philox counter that the draw launch
itself advances, so the whole of it can sit in a captured graph and still augment differently on every replay.

Not built (from_hyp refuses them): HSV jitter, translate, scale, shear, perspective, mosaic, mixup, copy-paste.  Chips
are square, the side a multiple of 4.
"""
import torch

from . import _lib

UNSUPPORTED_HYP = ("hsv_h", "hsv_s", "hsv_v", "translate", "scale", "shear", "perspective", "mosaic", "mixup", "copy_paste")
STATUS_NAMES = ("rows", "kept", "off_centre", "degenerate")


class TrainAugment:
    """degrees: 0 = no turn, anything else = a turn drawn uniformly from {0, 90, -180, -90} degrees (the reference's
    `random.choice`, whatever the value); flipud / fliplr: probabilities.  `.step` and `.seed` are int64 device scalars
    (a checkpoint carries them; `.step` counts the draws made)."""

    def __init__(self, degrees=180.0, flipud=0.0, fliplr=0.5, seed=0, device="cuda"):
        for name, p in (("flipud", flipud), ("fliplr", fliplr)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"TrainAugment: {name} is a probability (got {p})")
        self.degrees, self.flipud, self.fliplr = float(degrees), float(flipud), float(fliplr)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("s2anet_amd ops run on the GPU only (TrainAugment on a CPU device)")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.seed = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device=self.device)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)

    @classmethod
    def from_hyp(cls, hyp, seed=0, device="cuda"):
        """the reference's hyper-parameter dict; raises on an augmentation that is not built instead of skipping it"""
        on = [k for k in UNSUPPORTED_HYP if float(hyp.get(k, 0.0) or 0.0) != 0.0]
        if on:
            raise ValueError(f"TrainAugment.from_hyp: not built on the device: {', '.join(on)} (must be 0)")
        return cls(degrees=hyp.get("degrees", 0.0), flipud=hyp.get("flipud", 0.0), fliplr=hyp.get("fliplr", 0.0), seed=seed,
                   device=device)

    def draw(self, B, out=None):
        """params int32 [B,4] = (rot, flipud, fliplr, 0) for the current step; advances `.step` by one"""
        B = int(B)
        if out is None:
            out = torch.empty((B, 4), dtype=torch.int32, device=self.device)
        _lib.require_cuda(out)
        if out.device != self.step.device:
            raise ValueError(f"TrainAugment.draw: out is on {out.device}, the step counter on {self.step.device}")
        if out.dtype != torch.int32 or tuple(out.shape) != (B, 4) or not out.is_contiguous():
            raise ValueError("TrainAugment.draw: out must be a contiguous int32 [B,4] tensor")
        with torch.cuda.device(out.device):
            _lib.check(_lib.lib().s2a_augment_draw(_lib.ptr(self.step), _lib.ptr(self.seed), B, int(self.degrees != 0.0),
                                                   self.flipud, self.fliplr, _lib.ptr(out), _lib.stream_ptr(out.device)))
        return out

    def apply(self, imgs_u8, labels, params, out_imgs=None, out_targets=None, normalize=False, out_status=None):
        """imgs_u8: uint8 [B,3,S,S] channels-last (the layout `stem_limits` asks for) or [B,S,S,3] contiguous; labels f32
        [G,10]; params int32 [B,4] -> (imgs of the same shape and layout, targets f32 [G,7], status int64 [4] =
        (rows, kept, off_centre, degenerate)).  out_imgs may not overlap imgs_u8."""
        _lib.require_cuda(imgs_u8, labels, params, out_imgs, out_targets, out_status)
        for name, t in (("labels", labels), ("params", params), ("out_imgs", out_imgs), ("out_targets", out_targets),
                        ("out_status", out_status)):
            if t is not None and t.device != imgs_u8.device:
                raise ValueError(f"TrainAugment.apply: {name} is on {t.device}, imgs_u8 on {imgs_u8.device}")
        if imgs_u8.dtype != torch.uint8 or imgs_u8.dim() != 4:
            raise ValueError("TrainAugment.apply: imgs_u8 must be a uint8 batch of 4 dimensions")
        nchw = imgs_u8.shape[1] == 3 and imgs_u8.shape[3] != 3
        if imgs_u8.shape[1] == 3 and imgs_u8.shape[3] == 3:
            nchw = not imgs_u8.is_contiguous()        # [B,3,3,3]: the strides decide
        hwc = imgs_u8.permute(0, 2, 3, 1) if nchw else imgs_u8
        if hwc.shape[3] != 3 or not hwc.is_contiguous():
            raise ValueError("TrainAugment.apply: imgs_u8 must be channels-last RGB ([B,3,H,W] channels_last or [B,H,W,3])")
        B, H, W, _ = hwc.shape
        if out_imgs is None:
            out_imgs = torch.empty_like(imgs_u8)
        out_hwc = out_imgs.permute(0, 2, 3, 1) if nchw else out_imgs
        if out_imgs.dtype != torch.uint8 or out_hwc.shape != hwc.shape or not out_hwc.is_contiguous():
            raise ValueError("TrainAugment.apply: out_imgs must have the shape, dtype and layout of imgs_u8")
        if params.dtype != torch.int32 or tuple(params.shape) != (B, 4) or not params.is_contiguous():
            raise ValueError("TrainAugment.apply: params must be a contiguous int32 [B,4] tensor")
        if labels.dtype != torch.float32 or labels.dim() != 2 or labels.shape[1] != 10:
            raise ValueError("TrainAugment.apply: labels must be float32 [G,10] = (image, class, x1, y1 .. x4, y4)")
        labels = labels.contiguous()
        G = labels.shape[0]
        if out_targets is None:
            out_targets = torch.empty((G, 7), dtype=torch.float32, device=labels.device)
        if out_targets.dtype != torch.float32 or tuple(out_targets.shape) != (G, 7) or not out_targets.is_contiguous():
            raise ValueError("TrainAugment.apply: out_targets must be a contiguous float32 [G,7] tensor")
        if out_status is None:
            out_status = torch.empty(4, dtype=torch.int64, device=labels.device)
        if out_status.dtype != torch.int64 or out_status.numel() != 4 or not out_status.is_contiguous():
            raise ValueError("TrainAugment.apply: out_status must be a contiguous int64 [4] tensor")
        L = _lib.lib()
        with torch.cuda.device(imgs_u8.device):
            st = _lib.stream_ptr(imgs_u8.device)
            _lib.check(L.s2a_augment_images_u8(_lib.ptr(hwc), _lib.ptr(params), B, H, W, _lib.ptr(out_hwc), st))
            if G:
                _lib.check(L.s2a_augment_labels(_lib.ptr(labels), G, _lib.ptr(params), B, H, W, int(bool(normalize)),
                                                _lib.ptr(out_targets), _lib.ptr(out_status), st))
            else:
                out_status.zero_()
        return out_imgs, out_targets, out_status

    def __call__(self, imgs_u8, labels, params=None, out_imgs=None, out_targets=None, normalize=False, out_status=None):
        """draw, then apply; `params`: where the draw goes (int32 [B,4]), kept by the caller to see what was drawn"""
        _lib.require_cuda(imgs_u8, labels)
        params = self.draw(imgs_u8.shape[0], out=params)
        return self.apply(imgs_u8, labels, params, out_imgs, out_targets, normalize, out_status)

    def state_dict(self):
        return {"seed": self.seed.clone(), "step": self.step.clone()}

    def load_state_dict(self, state):
        self.seed.copy_(state["seed"])
        self.step.copy_(state["step"])
