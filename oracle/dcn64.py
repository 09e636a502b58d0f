"""float64 deformable convolution for the AlignConv geometry in plain torch -- TEST INFRASTRUCTURE ONLY.

3 x 3 kernel, stride 1, pad 1, dilation 1, one group, one deformable group; x [B,C,H,W], offset [B,18,H,W] (channel
2t = dy, 2t + 1 = dx of tap t = 3i + j), weight [O,C,3,3].  Runs on the CPU or the GPU, on whatever device x is on.

Sampling follows the reference's kernel (models/dcn/src/deform_conv_cuda_kernel.cu):
  * a sample at (h, w) = (y - 1 + i + dy, x - 1 + j + dx) counts only inside the band -1 < h < H, -1 < w < W (:228,
    and the same test in get_gradient_weight / get_coordinate_weight, :120, :149);
  * the four corners are taken explicitly from floor(h), floor(w); a corner outside the image reads 0 (:97-108).
floor() is a constant for autograd, so the coordinate gradient at an exact integer is the one-sided difference over the
cell floor() picks, which is what get_coordinate_weight (:145-187) computes.  (grid_sample is avoided on purpose: its
normalise / unnormalise round trip can move such a point just below the integer and pick the other cell.)

The backward is autograd's, in float64, batch by batch and in channel chunks (a chunk's output is a partial sum of the
full output, so back-propagating grad_output through every chunk separately gives the full gradients; the chunks bound
the memory: 8 x 256 x 128 x 128 stays near a GB).  Next to each gradient it gives an elementwise scale S, the sum of
the absolute values of the products that make up that entry: a kernel that forms the entry with rounding error u per
product and per addition is within about (number of roundings) * u * S of it, whatever cancellation the sum has.
"""
import torch

_F64 = torch.float64


def sample_points(offset, pos_dtype=None, dtype=_F64):
    """offset [B,18,H,W] -> (h, w) [B,9,H,W] in `dtype` (float64), the sample points.  pos_dtype=torch.float32 rounds them the way a
    float32 kernel forms them, fl32(float(y - 1 + i) + dy) (deform_conv_cuda_kernel.cu:222-223 at scalar_t = float,
    and every kernel of csrc/dcn_bwd_ops.hip); d(point)/d(offset) stays 1."""
    B, _, H, W = offset.shape
    dev = offset.device
    t = torch.arange(9, device=dev)
    base_h = (torch.arange(H, device=dev, dtype=dtype).view(1, H, 1) - 1 + (t // 3).to(dtype).view(9, 1, 1)).expand(9, H, W)
    base_w = (torch.arange(W, device=dev, dtype=dtype).view(1, 1, W) - 1 + (t % 3).to(dtype).view(9, 1, 1)).expand(9, H, W)
    off = offset.to(dtype)
    h, w = base_h + off[:, 0::2], base_w + off[:, 1::2]
    if pos_dtype is not None:
        h = h + (h.detach().to(pos_dtype).to(dtype) - h.detach())
        w = w + (w.detach().to(pos_dtype).to(dtype) - w.detach())
    return h, w


def _corners(h, w, H, W):
    """the four bilinear corners of sample points h, w (any shape): [(flat index, weight, valid)] in the order (low, low),
    (low, high), (high, low), (high, high) of (row, column), plus the fractions (lh, lw) -- weights keep autograd"""
    band = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h.detach()), torch.floor(w.detach())
    lh, lw = h - hl, w - wl
    hh, hw = 1 - lh, 1 - lw
    hl, wl = hl.long(), wl.long()
    out = []
    for dy, dx, wt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
        y, x = hl + dy, wl + dx
        ok = band & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
        idx = y.clamp(0, H - 1) * W + x.clamp(0, W - 1)
        out.append((idx, torch.where(ok, wt, torch.zeros_like(wt)), ok))
    return out, (lh, lw)


def _columns(xf, corners):
    """xf [Cc, H*W] of one image, corners of its [9,H,W] points -> columns [Cc, 9*H*W]"""
    cols = None
    for idx, wt, _ in corners:
        v = xf[:, idx.reshape(-1)] * wt.reshape(1, -1).to(xf.dtype)
        cols = v if cols is None else cols + v
    return cols


def deform_conv64(x, offset, weight, pos_dtype=None, dtype=_F64):
    """differentiable forward, no chunking (small shapes): -> out [B,O,H,W].  dtype: the type every step runs in, float64
    for the reference; the same stock ops in float32 / float16 are the baseline a kernel's error is compared with
    (oracle/twin64.py)"""
    B, C, H, W = x.shape
    O = weight.shape[0]
    # float16: the sample points and the bilinear weights are formed in float32 (no float16 kernel of this package forms
    # positions in float16: at a coordinate of 16-32 its ulp is 0.016 px) and the weights are rounded to float16 once,
    # so that the float16 baseline is a single-rounding computation on the same points
    h, w = sample_points(offset, pos_dtype, torch.float32 if dtype == torch.float16 else dtype)
    xx, ww = x.to(dtype), weight.to(dtype).reshape(O, C * 9)
    outs = []
    for b in range(B):
        corners, _ = _corners(h[b], w[b], H, W)
        cols = _columns(xx[b].reshape(C, H * W), corners)
        outs.append((ww @ cols.reshape(C * 9, H * W)).view(O, H, W))
    return torch.stack(outs)


def _chunk_channels(C, HW, chunk_elems):
    return max(1, min(C, chunk_elems // (9 * HW)))


def deform_conv_backward64(x, offset, weight, grad_out, pos_dtype=None, scale=True, chunk_elems=1 << 23):
    """-> dict of float64 tensors on x's device: grad_input [B,C,H,W], grad_offset [B,18,H,W], grad_weight [O,C,3,3]
    (DeformConvFunction.backward at scale 1), and with scale=True their error scales S_input, S_offset, S_weight:
      S_input:  the backward with |weight| and |grad_out| (the bilinear weights are >= 0);
      S_weight: |grad_out| x columns sampled from |x|^T;
      S_offset: sum over channels of (|weight|^T |grad_out|) times the coordinate weight of |corner values|
                (get_coordinate_weight with |v| and the fractions' magnitudes)."""
    B, C, H, W = x.shape
    O = weight.shape[0]
    HW = H * W
    dev = x.device
    xx = x.detach().to(_F64).contiguous()
    w64 = weight.detach().to(_F64).reshape(O, C, 9)
    go = grad_out.detach().to(_F64).reshape(B, O, HW)
    r = {k: torch.zeros(s, dtype=_F64, device=dev) for k, s in
         (("grad_input", (B, C, H, W)), ("grad_offset", (B, 18, H, W)), ("grad_weight", (O, C, 3, 3)))}
    if scale:
        for k in ("input", "offset", "weight"):
            r["S_" + k] = torch.zeros_like(r["grad_" + k])
    cc = _chunk_channels(C, HW, chunk_elems)
    for b in range(B):
        ob = offset[b:b + 1].detach().to(_F64)
        for c0 in range(0, C, cc):
            c1 = min(C, c0 + cc)
            with torch.enable_grad():
                off_l = ob.clone().requires_grad_(True)
                x_l = xx[b, c0:c1].reshape(c1 - c0, HW).clone().requires_grad_(True)
                w_l = w64[:, c0:c1].reshape(O, (c1 - c0) * 9).clone().requires_grad_(True)
                h, w = sample_points(off_l, pos_dtype)
                corners, _ = _corners(h[0], w[0], H, W)
                part = w_l @ _columns(x_l, corners).reshape((c1 - c0) * 9, HW)
                gx, goff, gw = torch.autograd.grad(part, (x_l, off_l, w_l), go[b])
            r["grad_input"][b, c0:c1] = gx.view(c1 - c0, H, W)
            r["grad_offset"][b] += goff[0]
            r["grad_weight"][:, c0:c1] += gw.view(O, c1 - c0, 3, 3)
            if not scale:
                continue
            with torch.no_grad():
                h, w = sample_points(ob, pos_dtype)
            h, w = h[0], w[0]
            with torch.enable_grad():
                xa = xx[b, c0:c1].abs().reshape(c1 - c0, HW).requires_grad_(True)
                wa = w64[:, c0:c1].abs().reshape(O, (c1 - c0) * 9).requires_grad_(True)
                corners, (lh, lw) = _corners(h, w, H, W)
                part = wa @ _columns(xa, corners).reshape((c1 - c0) * 9, HW)
                sx, sw = torch.autograd.grad(part, (xa, wa), go[b].abs())
            r["S_input"][b, c0:c1] = sx.view(c1 - c0, H, W)
            r["S_weight"][:, c0:c1] += sw.view(O, c1 - c0, 3, 3)
            with torch.no_grad():
                g_abs = (wa.t() @ go[b].abs()).view(c1 - c0, 9, H, W)     # |W|^T |gO|: the column gradient's scale
                a = [torch.where(ok.reshape(1, -1), xa[:, idx.reshape(-1)], torch.zeros((), dtype=_F64, device=dev))
                     .view(c1 - c0, 9, H, W) for idx, _, ok in corners]
                hh, hw = 1 - lh, 1 - lw
                cw_h = hw * (a[0] + a[2]) + lw * (a[1] + a[3])             # bp_dir 0 (dy): |-(1-lw) v1 - lw v2 + ...|
                cw_w = hh * (a[0] + a[1]) + lh * (a[2] + a[3])             # bp_dir 1 (dx)
                r["S_offset"][b, 0::2] += (g_abs * cw_h).sum(0)
                r["S_offset"][b, 1::2] += (g_abs * cw_w).sum(0)
    return r
