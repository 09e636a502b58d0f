"""float64 deformable convolution for ANY geometry in plain torch -- TEST INFRASTRUCTURE ONLY.

The general form of oracle/dcn64.py (which stays the reference for the AlignConv geometry at production sizes: it chunks;
this one does not and is meant for small shapes).  Written from the definition of the operation:

    out[b, o, ho, wo] = sum over c in group(o), taps (i, j):
                        w[o, c', i, j] * mask[b, dg(c), t, ho, wo] * bilinear(x[b, c], h, w)   (+ bias[o])
    h = ho * sH - pH + i * dH + offset[b, dg(c) * 2T + 2t,     ho, wo]        t = i * kW + j, T = kH * kW
    w = wo * sW - pW + j * dW + offset[b, dg(c) * 2T + 2t + 1, ho, wo]
    group(o) = o // (O / groups) owns the input channels [g * C/groups, (g + 1) * C/groups); c' = c - g * C/groups
    dg(c)    = c // (C / deformable_groups)

A sample counts only inside the band -1 < h < H, -1 < w < W; its four corners come from floor(h), floor(w), a corner
outside the image reads 0.  floor() is a constant for autograd, so the coordinate gradient at an exact integer is the
one-sided difference over the cell floor() picks.  Everything is a gather and a matrix product, so one autograd backward
gives grad_input, grad_offset and grad_weight for every geometry, grouped ones included.

Next to each result comes its elementwise error scale S, the sum of the absolute values of the products behind the
entry (see oracle/dcn64.py), and M, the number of (position, tap, corner) contributions that land on each input cell.

`defect` plants one wrong reading of the definition (DEFECTS below); tests use it to show that a case can tell the
right reading from the wrong one.
"""
import torch

_F64 = torch.float64

# wrong readings of the definition a kernel could implement, and that the cases of tests/dcn_geometry_cases.py must expose
DEFECTS = ("stride_swap", "padding_swap", "dilation_swap", "tap_order", "dg_from_group", "filter_groups_swapped",
           "mask_wrong_dg", "band_closed")


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def output_size(H, W, kernel, stride, padding, dilation):
    (kH, kW), (sH, sW), (pH, pW), (dH, dW) = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
    return (H + 2 * pH - (dH * (kH - 1) + 1)) // sH + 1, (W + 2 * pW - (dW * (kW - 1) + 1)) // sW + 1


def applicable(defect, kernel, stride, padding, dilation, groups, deformable_groups, mask=False, backward=True):
    """can this geometry express the defect at all (does the wrong reading differ from the right one)?"""
    (kH, kW), s, p, d = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
    return {"stride_swap": s[0] != s[1], "padding_swap": p[0] != p[1],
            "dilation_swap": d[0] != d[1] and (kH > 1 or kW > 1),
            "tap_order": kH > 1 and kW > 1,
            # channel c -> c // (C/groups) instead of c // (C/dg): another map whenever the two counts differ
            "dg_from_group": deformable_groups > 1 and groups != deformable_groups,
            "filter_groups_swapped": groups > 1,
            "mask_wrong_dg": bool(mask) and deformable_groups > 1,
            # a sample on h = -1 has weight 0 on row 0: the forward cannot see it, the offset gradient can
            "band_closed": bool(backward)}[defect]


def sample_points(offset, kernel, stride, padding, dilation, deformable_groups, pos_dtype=None, dtype=_F64, defect=None):
    """offset [B, dg*2T, Ho, Wo] -> (h, w) [B, dg, T, Ho, Wo] in `dtype`.  pos_dtype=torch.float32 rounds them the way a
    float32 kernel forms them, fl32(float(integer base) + offset); d(point)/d(offset) stays 1."""
    (kH, kW), (sH, sW), (pH, pW), (dH, dW) = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
    if defect == "stride_swap":
        sH, sW = sW, sH
    if defect == "padding_swap":
        pH, pW = pW, pH
    if defect == "dilation_swap":
        dH, dW = dW, dH
    B, _, Ho, Wo = offset.shape
    T, dev = kH * kW, offset.device
    t = torch.arange(T, device=dev)
    i, j = t // kW, t % kW
    base_h = ((torch.arange(Ho, device=dev) * sH - pH).view(1, Ho, 1) + (i * dH).view(T, 1, 1)).to(dtype)
    base_w = ((torch.arange(Wo, device=dev) * sW - pW).view(1, 1, Wo) + (j * dW).view(T, 1, 1)).to(dtype)
    off = offset.to(dtype).reshape(B, deformable_groups, T, 2, Ho, Wo)
    if defect == "tap_order":
        off = off[:, :, j * kH + i]                      # tap (i, j) reads the channel pair j * kH + i
    h, w = base_h + off[:, :, :, 0], base_w + off[:, :, :, 1]
    if pos_dtype is not None:
        h = h + (h.detach().to(pos_dtype).to(dtype) - h.detach())
        w = w + (w.detach().to(pos_dtype).to(dtype) - w.detach())
    return h, w


def _corners(h, w, H, W, closed=False):
    """[(flat index, weight, valid)] of the four bilinear corners in the order (low, low), (low, high), (high, low),
    (high, high) of (row, column), plus the fractions (lh, lw); the weights keep autograd"""
    band = ((h >= -1) & (w >= -1) if closed else (h > -1) & (w > -1)) & (h < H) & (w < W)
    hl, wl = torch.floor(h.detach()), torch.floor(w.detach())
    lh, lw = h - hl, w - wl
    hh, hw = 1 - lh, 1 - lw
    hl, wl = hl.long(), wl.long()
    out = []
    for dy, dx, wt in ((0, 0, hh * hw), (0, 1, hh * lw), (1, 0, lh * hw), (1, 1, lh * lw)):
        y, x = hl + dy, wl + dx
        ok = band & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
        out.append((y.clamp(0, H - 1) * W + x.clamp(0, W - 1), torch.where(ok, wt, torch.zeros_like(wt)), ok))
    return out, (lh, lw)


def _dg_of_channel(C, groups, deformable_groups, dev, defect=None):
    c = torch.arange(C, device=dev)
    if defect == "dg_from_group":
        return (c // (C // groups)) % deformable_groups
    return c // (C // deformable_groups)


def _per_channel(a, dgi):
    """[B, dg, T, Ho, Wo] -> [B, C, T*Ho*Wo]: every channel gets its deformable group's entry"""
    return a[:, dgi].reshape(a.shape[0], dgi.numel(), -1)


def _forward(xx, ww, corners, dgi, mask_c, groups):
    """xx [B,C,H,W], ww [O,C/groups,kH,kW], corners of [B,dg,T,Ho,Wo] points, mask_c [B,C,T*P] or None
    -> out [B, O, P], columns [B, C, T*P]"""
    B, C = xx.shape[:2]
    O = ww.shape[0]
    xf = xx.reshape(B, C, -1)
    cols = None
    for idx, wt, _ in corners:
        v = torch.gather(xf, 2, _per_channel(idx, dgi)) * _per_channel(wt, dgi).to(xf.dtype)
        cols = v if cols is None else cols + v
    if mask_c is not None:
        cols = cols * mask_c
    K = ww[0].numel()                                     # C/groups * T
    out = torch.einsum("gok,bgkp->bgop", ww.reshape(groups, O // groups, K), cols.reshape(B, groups, K, -1))
    return out.reshape(B, O, -1), cols


def _prepare(x, offset, weight, stride, padding, dilation, groups, deformable_groups, mask, pos_dtype, dtype, defect):
    B, C, H, W = x.shape
    O, Cg, kH, kW = weight.shape
    assert Cg * groups == C and O % groups == 0 and C % deformable_groups == 0
    Ho, Wo = output_size(H, W, (kH, kW), stride, padding, dilation)
    T = kH * kW
    assert tuple(offset.shape) == (B, deformable_groups * 2 * T, Ho, Wo), (tuple(offset.shape), (Ho, Wo))
    pdt = torch.float32 if dtype == torch.float16 else dtype
    h, w = sample_points(offset, (kH, kW), stride, padding, dilation, deformable_groups, pos_dtype, pdt, defect)
    dgi = _dg_of_channel(C, groups, deformable_groups, x.device, defect)
    mask_c = None
    if mask is not None:
        assert tuple(mask.shape) == (B, deformable_groups * T, Ho, Wo)
        m = mask.to(dtype).reshape(B, deformable_groups, T, Ho, Wo)
        mask_c = _per_channel(m, (dgi + 1) % deformable_groups if defect == "mask_wrong_dg" else dgi)
    return h, w, dgi, mask_c, (B, C, H, W, O, Ho, Wo, T)


def deform_conv64_general(x, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, mask=None,
                          bias=None, pos_dtype=None, dtype=_F64, defect=None):
    """differentiable forward -> out [B, O, Ho, Wo] in `dtype` (float64: the reference; float32: the same stock ops as a
    baseline).  mask [B, dg*T, Ho, Wo] and bias [O] give the modulated form."""
    h, w, dgi, mask_c, (B, C, H, W, O, Ho, Wo, T) = _prepare(x, offset, weight, stride, padding, dilation, groups,
                                                             deformable_groups, mask, pos_dtype, dtype, defect)
    corners, _ = _corners(h, w, H, W, closed=defect == "band_closed")
    ww = weight.to(dtype)
    if defect == "filter_groups_swapped":
        ww = ww.reshape(groups, O // groups, *ww.shape[1:]).flip(0).reshape(ww.shape)
    out, _ = _forward(x.to(dtype), ww, corners, dgi, mask_c, groups)
    out = out.reshape(B, O, Ho, Wo)
    return out if bias is None else out + bias.to(dtype).view(1, O, 1, 1)


def deform_conv_general64(x, offset, weight, grad_out=None, stride=1, padding=0, dilation=1, groups=1,
                          deformable_groups=1, mask=None, bias=None, pos_dtype=None, scale=True, defect=None):
    """-> dict of float64 tensors on x's device:
      out [B,O,Ho,Wo]; with grad_out also grad_input, grad_offset, grad_weight (DeformConvFunction.backward at scale 1);
      with scale=True the error scales
        S_out:    the forward on |x|, |w|, |mask|, plus |bias|;
        S_input:  the backward with |w|, |mask| and |grad_out| (the bilinear weights are >= 0);
        S_weight: |grad_out| x columns sampled from |x| with |mask|;
        S_offset: sum over the channels of the deformable group of (|w|^T |grad_out|) |mask| times the coordinate weight
                  of |corner values| (the magnitudes of the terms of the one-sided difference);
      and the counts
        M [B,C,H,W]:          (position, tap, corner) contributions landing on each input cell (the scatter of ones);
        cw_abs [like offset]: S_offset with every column gradient set to 1: what an absolute error per column entry
                              (an underflowed float16 column) is multiplied by."""
    kw = dict(stride=stride, padding=padding, dilation=dilation, groups=groups, deformable_groups=deformable_groups)
    dev = x.device
    x64, off64, w64 = (a.detach().to(_F64) for a in (x, offset, weight))
    m64 = None if mask is None else mask.detach().to(_F64)
    b64 = None if bias is None else bias.detach().to(_F64)
    r = {}
    with torch.enable_grad():
        xl, ol, wl = (a.clone().requires_grad_(True) for a in (x64, off64, w64))
        out = deform_conv64_general(xl, ol, wl, mask=m64, bias=b64, pos_dtype=pos_dtype, defect=defect, **kw)
        r["out"] = out.detach()
        if grad_out is not None:
            go = grad_out.detach().to(_F64)
            r["grad_input"], r["grad_offset"], r["grad_weight"] = torch.autograd.grad(out, (xl, ol, wl), go)
    if not scale:
        return r
    ma = None if m64 is None else m64.abs()
    with torch.enable_grad():
        xa, wa = x64.abs().requires_grad_(True), w64.abs().requires_grad_(True)
        s_out = deform_conv64_general(xa, off64, wa, mask=ma, pos_dtype=pos_dtype, defect=defect, **kw)
        if grad_out is not None:
            r["S_input"], r["S_weight"] = torch.autograd.grad(s_out, (xa, wa), go.abs())
    r["S_out"] = s_out.detach() + (0 if b64 is None else b64.abs().view(1, -1, 1, 1))
    with torch.no_grad():
        h, w, dgi, mask_c, (B, C, H, W, O, Ho, Wo, T) = _prepare(x64, off64, w64, stride, padding, dilation, groups,
                                                                 deformable_groups, ma, pos_dtype, _F64, defect)
        corners, (lh, lw) = _corners(h, w, H, W, closed=defect == "band_closed")
        M = torch.zeros((B, C, H * W), dtype=_F64, device=dev)
        for idx, _, ok in corners:
            M.scatter_add_(2, _per_channel(idx, dgi), _per_channel(ok.to(_F64), dgi))
        r["M"] = M.view(B, C, H, W)
        if grad_out is None:
            return r
        xf = x64.abs().reshape(B, C, -1)
        a = [torch.gather(xf, 2, _per_channel(idx, dgi)) * _per_channel(ok.to(_F64), dgi) for idx, _, ok in corners]
        lh, lw = _per_channel(lh, dgi), _per_channel(lw, dgi)
        hh, hw = 1 - lh, 1 - lw
        Cg, Og, P = C // groups, O // groups, Ho * Wo
        wa = w64.abs()
        if defect == "filter_groups_swapped":
            wa = wa.reshape(groups, Og, Cg, T).flip(0)
        g_abs = torch.einsum("gok,bgop->bgkp", wa.reshape(groups, Og, Cg * T), go.abs().reshape(B, groups, Og, P))
        g_abs = g_abs.reshape(B, C, T * P)
        if mask_c is not None:
            g_abs = g_abs * mask_c

        def per_offset(cw_h, cw_w, weight_):
            s = torch.zeros((B, deformable_groups, T, 2, P), dtype=_F64, device=dev)
            s[:, :, :, 0].index_add_(1, dgi, (weight_ * cw_h).view(B, C, T, P))
            s[:, :, :, 1].index_add_(1, dgi, (weight_ * cw_w).view(B, C, T, P))
            return s.view(B, deformable_groups * 2 * T, Ho, Wo)

        r["S_offset"] = per_offset(hw * (a[0] + a[2]) + lw * (a[1] + a[3]), hh * (a[0] + a[1]) + lh * (a[2] + a[3]), g_abs)
        r["cw_abs"] = per_offset(hw * (a[0] + a[2]) + lw * (a[1] + a[3]), hh * (a[0] + a[1]) + lh * (a[2] + a[3]),
                                 torch.ones_like(g_abs))
    return r
