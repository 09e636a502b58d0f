"""float64 references of the forward convolutions, with error scales, in plain torch -- TEST INFRASTRUCTURE ONLY.

Runs on the CPU or the GPU, on whatever device the input is on.  Every function returns the exact result y (float64) and
an elementwise scale S: the sum of the absolute values of all terms behind each output entry (products, bias, residual).
A kernel that forms an entry with rounding error u per rounding step is within about (number of roundings) * u * S of
it, whatever cancellation the sum has (the same convention as oracle/dcn64.py).

  conv64       1x1 / pad 0 and 3x3 / pad 1 at stride 1 or 2, bias, residual (also a nearest-2x up-sampled coarse map,
               the FPN top-down add of s2a_conv1x1_add_up2_f16), ReLU -- as explicit per-tap shifted matmuls, so that
               the result does not depend on the backend torch picks for float64 convolutions
  stem64       the fused stem: f16(u8 / divisor) -> conv 7x7 / 2 / pad 3 + bias -> ReLU -> max-pool 3x3 / 2 / pad 1
  rot_pool64   max over runs of 8 channels (RotationInvariantPooling)
  align64      the AlignConv forward (oracle/dcn64.py's sampling), with S and S_corner

Layout: inputs are [B,C,H,W]-shaped tensors of any memory format; outputs are [B,O,Ho,Wo]-shaped views of
channels-last float64 storage.  Work runs in chunks of images (and channels for align64) to bound memory.
"""
import torch
import torch.nn.functional as F

from .dcn64 import _columns, _corners, sample_points

_F64 = torch.float64


def _nhwc64(t):
    return t.permute(0, 2, 3, 1).to(_F64)


def _out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _conv_nhwc(x, w, stride, pad):
    """x [b,H,W,C] f64, w [O,C,k,k] f64 -> (sum of the taps, sum of their absolute values) [b,Ho,Wo,O]: one matmul
    per tap"""
    b, H, W, C = x.shape
    O, _, k, _ = w.shape
    Ho, Wo = _out_size(H, k, stride, pad), _out_size(W, k, stride, pad)
    xp = F.pad(x, (0, 0, pad, pad, pad, pad)) if pad else x
    y = x.new_zeros((b, Ho, Wo, O))
    s = x.new_zeros((b, Ho, Wo, O))
    for i in range(k):
        for j in range(k):
            xs = xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride, :]
            wt = w[:, :, i, j].t()
            y += xs @ wt
            s += xs.abs() @ wt.abs()
    return y, s


def _chunk(per_image, chunk_elems):
    return max(1, chunk_elems // max(per_image, 1))


def conv64(x, w, b=None, stride=1, ksize=None, residual=None, residual_up2=False, relu=False, chunk_elems=1 << 25):
    """relu?(conv(x, w) + b (+ residual)) in float64 -> (y, S), both [B,O,Ho,Wo].
    ksize 1 (pad 0) or 3 (pad 1); residual [B,O,Ho,Wo], or with residual_up2 the coarse map [B,O,Ho/2,Wo/2] that is
    added through a nearest 2x up-sampling.  S = conv(|x|, |w|) + |b| + |r| (ReLU does not change S)."""
    B, C, H, W = x.shape
    O = w.shape[0]
    k = w.shape[-1] if ksize is None else ksize
    assert k in (1, 3) and tuple(w.shape) == (O, C, k, k) and stride in (1, 2)
    pad = (k - 1) // 2
    Ho, Wo = _out_size(H, k, stride, pad), _out_size(W, k, stride, pad)
    w64 = w.detach().to(device=x.device, dtype=_F64)
    b64 = None if b is None else b.detach().to(device=x.device, dtype=_F64)
    y = torch.empty((B, Ho, Wo, O), dtype=_F64, device=x.device)
    S = torch.empty_like(y)
    step = _chunk(Ho * Wo * max(C, O), chunk_elems)
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        yc, sc = _conv_nhwc(_nhwc64(x[b0:b1]), w64, stride, pad)
        if b64 is not None:
            yc += b64
            sc += b64.abs()
        if residual is not None:
            r = _nhwc64(residual[b0:b1])
            if residual_up2:
                r = r.repeat_interleave(2, 1).repeat_interleave(2, 2)
            assert r.shape == yc.shape, (r.shape, yc.shape)
            yc += r
            sc += r.abs()
        if relu:
            yc.clamp_min_(0)
        y[b0:b1], S[b0:b1] = yc, sc
    return y.permute(0, 3, 1, 2), S.permute(0, 3, 1, 2)


def u8_to_f16(img_u8, divisor=255.0):
    """the stem kernel's table value: f16 of the float32 quotient u8 / divisor"""
    return (img_u8.to(torch.float32) / float(divisor)).to(torch.float16)


def stem64(img_u8, w, b=None, divisor=255.0, chunk_elems=1 << 25):
    """uint8 [B,3,H,W] -> max-pool 3x3/2/pad 1 (relu(conv 7x7/2/pad 3 (f16(u8 / divisor), w) + b)) in float64 ->
    (y, S) [B,O,Hp,Wp].  S = the max-pool of the conv's S (a max is 1-Lipschitz in the sup norm)."""
    B, C, H, W = img_u8.shape
    O = w.shape[0]
    assert C == 3 and tuple(w.shape) == (O, 3, 7, 7)
    w64 = w.detach().to(device=img_u8.device, dtype=_F64)
    b64 = None if b is None else b.detach().to(device=img_u8.device, dtype=_F64)
    Hc, Wc = _out_size(H, 7, 2, 3), _out_size(W, 7, 2, 3)
    Hp, Wp = _out_size(Hc, 3, 2, 1), _out_size(Wc, 3, 2, 1)
    y = torch.empty((B, Hp, Wp, O), dtype=_F64, device=img_u8.device)
    S = torch.empty_like(y)
    step = _chunk(Hc * Wc * O, chunk_elems)
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        yc, sc = _conv_nhwc(_nhwc64(u8_to_f16(img_u8[b0:b1], divisor)), w64, 2, 3)
        if b64 is not None:
            yc += b64
            sc += b64.abs()
        yc.clamp_min_(0)
        y[b0:b1] = F.max_pool2d(yc.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        S[b0:b1] = F.max_pool2d(sc.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    return y.permute(0, 3, 1, 2), S.permute(0, 3, 1, 2)


def rot_pool64(y, S, n=8):
    """max over runs of n channels (channel dim 1) of y and of S"""
    def pool(t):
        return t.unflatten(1, (t.shape[1] // n, n)).amax(2)
    return pool(y), pool(S)


def _reach_corners(h, w, H, W, d):
    """the in-image corners of every cell that a point within d (per axis) of (h, w) lies in, weight 1 each: rows
    floor(h - d) .. floor(h + d) + 1 (two, or three when h is within d of an integer), columns likewise"""
    r0, r1 = torch.floor(h - d), torch.floor(h + d) + 1
    c0, c1 = torch.floor(w - d), torch.floor(w + d) + 1
    out = []
    for dy in range(3):
        for dx in range(3):
            y, x = r0 + dy, c0 + dx
            ok = (y <= r1) & (x <= c1) & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
            idx = y.clamp(0, H - 1).long() * W + x.clamp(0, W - 1).long()
            out.append((idx, ok.to(_F64), ok))
    return out


def align64(x, offset, weight, pos_dtype=torch.float32, relu=False, d=0.0, chunk_elems=1 << 23):
    """the AlignConv forward relu?(deform_conv(x, offset, weight)) in float64 (oracle/dcn64.py's sampling) ->
    (y, S, S_corner), each [B,O,H,W]:
      S:        the same forward on |x| and |weight| (the bilinear weights are >= 0);
      S_corner: the same forward on |x| and |weight| with weight 1 on every in-image corner of every cell that a point
                within d (per axis, 0 <= d < 1/2) of the sample point lies in -- its own cell's four corners, and the
                neighbouring cell's too where the point lies within d of an integer row or column.
    Bilinear sampling with zero padding is continuous in (h, w) (the weights vanish at the band's edges and at the image
    border), and inside one cell its derivative along either axis is bounded by the sum of that cell's corner values.  A
    result whose sample points are off by at most d in h and in w is therefore off by at most 2 d S_corner, strictly,
    also when a moved point crosses into the neighbouring cell."""
    assert 0 <= d < 0.5
    B, C, H, W = x.shape
    O = weight.shape[0]
    HW = H * W
    w64 = weight.detach().to(device=x.device, dtype=_F64).reshape(O, C, 9)
    y = torch.zeros((B, O, HW), dtype=_F64, device=x.device)
    S, Sc = torch.zeros_like(y), torch.zeros_like(y)
    cc = max(1, min(C, chunk_elems // (9 * HW)))
    h, w = sample_points(offset.detach(), pos_dtype)
    for b in range(B):
        corners, _ = _corners(h[b], w[b], H, W)
        ones = _reach_corners(h[b], w[b], H, W, d)
        for c0 in range(0, C, cc):
            c1 = min(C, c0 + cc)
            xc = x[b, c0:c1].to(_F64).reshape(c1 - c0, HW)
            wc = w64[:, c0:c1].reshape(O, (c1 - c0) * 9)
            y[b] += wc @ _columns(xc, corners).reshape((c1 - c0) * 9, HW)
            xa, wa = xc.abs(), wc.abs()
            S[b] += wa @ _columns(xa, corners).reshape((c1 - c0) * 9, HW)
            Sc[b] += wa @ _columns(xa, ones).reshape((c1 - c0) * 9, HW)
    if relu:
        y.clamp_min_(0)
    return y.view(B, O, H, W), S.view(B, O, H, W), Sc.view(B, O, H, W)
