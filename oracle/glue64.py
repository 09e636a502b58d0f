"""float64 references of the head's small kernels (s2anet_amd/csrc/glue_ops.hip): rotated box decode, grid anchors,
AlignConv offsets, sigmoid, the top-k selection rule and the bias / residual / ReLU epilogue.

Plain numpy on the CPU.  The inputs are the kernel's own f32 / f16 inputs widened exactly to float64; every function
that has a rounding error to bound also returns the MAGNITUDE of each output: the sum of the absolute values of the
terms the float32 evaluation rounds.  A float32 evaluation of the same expression lies within

    K * 2^-24 * magnitude

of the float64 value, per element.  How K is set (tests/test_glue64_cpu.py re-measures it):

  the float32 restatements of oracle/__init__.py (numpy, one rounding per operation, no fused multiply-add) were
  compared with this module on 200 000 rows of tests/glue_cases.py:decode_rows per clip, on the AlignConv cases and on
  50 000 logits; the worst |f32 - f64| / (2^-24 * magnitude) per output kind is MEASURED_RATIO below.  K is twice that:
  the device's cosf / sinf / expf differ from numpy's by a couple of ulp and the compiler may contract a multiply-add,
  each of which moves a result by at most one more unit of the same magnitude term.  K is never tuned from a kernel's
  output.  A wrong kernel (sine and cosine swapped, a missing clamp, a wrong level stride) misses by four or more
  orders of magnitude.
"""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of float32
U16 = 2.0 ** -11            # unit roundoff of float16

# worst ratio of the float32 oracle against float64, measured on the CPU and rounded up to one decimal
# (tests/test_glue64_cpu.py measures again and asserts that it lands on these figures)
MEASURED_RATIO = {
    "centre": 3.2,          # x, y of the decode                           (measured 3.13)
    "size": 3.8,            # w, h of the decode: one expf, one product    (measured 3.74)
    "angle": 1.8,           # circular distance modulo pi                  (measured 1.79)
    "offset": 5.9,          # AlignConv offsets: five divisions, a rotation that can cancel inside |xr|  (measured 5.81)
    "sigmoid": 2.8,         # 1 / (1 + exp(-x)) on logits of [-9, 12]      (measured 2.77)
}
K = {kind: 2.0 * r for kind, r in MEASURED_RATIO.items()}
K_DECODE = np.array([K["centre"], K["centre"], K["size"], K["size"], K["angle"]])

ANGLE_LO, ANGLE_HI = -np.pi / 4, 3 * np.pi / 4


def _f64(a):
    """f16 / f32 (numpy or torch CPU) -> float64, exactly"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a).astype(np.float64)


def max_ratio32(wh_ratio_clip):
    """|log(clip)| rounded to float32, as the kernels receive it"""
    return float(np.float32(abs(np.log(float(wh_ratio_clip)))))


def decode64(rois, deltas, wh_ratio_clip):
    """delta2bbox_rotated in float64: rois, deltas [n,5] -> (out [n,5], magnitude [n,5]).
    magnitude: |dx w cos| + |dy h sin| + |x| (and the like for y), the value itself for w / h, |pi da| + |a| + pi for
    the angle.  The angle is in [-pi/4, 3pi/4); compare it with angle_distance (the wrap is a circle of length pi)."""
    r, d = _f64(rois).reshape(-1, 5), _f64(deltas).reshape(-1, 5)
    mr = max_ratio32(wh_ratio_clip)
    dw, dh = np.clip(d[:, 2], -mr, mr), np.clip(d[:, 3], -mr, mr)
    ca, sa = np.cos(r[:, 4]), np.sin(r[:, 4])
    t1, t2 = d[:, 0] * r[:, 2] * ca, d[:, 1] * r[:, 3] * sa
    t3, t4 = d[:, 0] * r[:, 2] * sa, d[:, 1] * r[:, 3] * ca
    out = np.empty_like(r)
    out[:, 0] = t1 - t2 + r[:, 0]
    out[:, 1] = t3 + t4 + r[:, 1]
    out[:, 2] = r[:, 2] * np.exp(dw)
    out[:, 3] = r[:, 3] * np.exp(dh)
    raw = np.pi * d[:, 4] + r[:, 4]
    out[:, 4] = np.mod(raw - ANGLE_LO, np.pi) + ANGLE_LO
    mag = np.empty_like(r)
    mag[:, 0] = np.abs(t1) + np.abs(t2) + np.abs(r[:, 0])
    mag[:, 1] = np.abs(t3) + np.abs(t4) + np.abs(r[:, 1])
    mag[:, 2] = np.abs(out[:, 2])
    mag[:, 3] = np.abs(out[:, 3])
    mag[:, 4] = np.abs(np.pi * d[:, 4]) + np.abs(r[:, 4]) + np.pi
    return out, mag


def angle_distance(got, ref):
    """circular distance modulo pi: min(|d|, pi - |d|), for angles at most one period apart"""
    d = np.abs(_f64(got) - _f64(ref))
    return np.minimum(d, np.abs(np.pi - d))


def decode_ratio(got, ref, mag):
    """per-element |got - ref| / (K * 2^-24 * magnitude) of a decode [n,5], the angle column as a circular distance;
    an angle outside [-pi/4 - bound, 3pi/4 + bound] counts as infinitely wrong.  No row is left out."""
    got, ref, mag = _f64(got).reshape(-1, 5), _f64(ref).reshape(-1, 5), _f64(mag).reshape(-1, 5)
    err = np.abs(got - ref)
    err[:, 4] = angle_distance(got[:, 4], ref[:, 4])
    bound = K_DECODE[None, :] * U32 * mag
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    outside = (got[:, 4] < ANGLE_LO - bound[:, 4]) | (got[:, 4] > ANGLE_HI + bound[:, 4])
    ratio[outside, 4] = np.inf
    ratio[~np.isfinite(got)] = np.inf
    return ratio


def grid_anchors64(feat_h, feat_w, stride, scale=4.0):
    """one square anchor per position, angle 0: [H*W,5], row-major over (y, x)"""
    out = np.zeros((feat_h, feat_w, 5), np.float64)
    out[..., 0] = (np.arange(feat_w, dtype=np.float64) * stride + 0.5 * (stride - 1))[None, :]
    out[..., 1] = (np.arange(feat_h, dtype=np.float64) * stride + 0.5 * (stride - 1))[:, None]
    out[..., 2] = out[..., 3] = float(np.float32(scale) * np.float32(stride))
    return out.reshape(-1, 5)


def refine64(pred, stride, anchor_scale=4.0):
    """grid anchors + FAM decode (clip 1e-6) of one level: pred [B,5,H,W] -> (out [B,H,W,5], magnitude)"""
    p = _f64(pred)
    B, five, H, W = p.shape
    assert five == 5
    anc = np.tile(grid_anchors64(H, W, stride, anchor_scale), (B, 1))
    out, mag = decode64(anc, p.transpose(0, 2, 3, 1).reshape(-1, 5), 1e-6)
    return out.reshape(B, H, W, 5), mag.reshape(B, H, W, 5)


def pyramid_anchors64(batch, sizes, strides, anchor_scale=4.0):
    """grid anchors of a pyramid-packed buffer: level l = [B, H_l, W_l] rows, levels back to back -> [P,5]"""
    return np.concatenate([np.tile(grid_anchors64(h, w, s, anchor_scale), (batch, 1)) for (h, w), s in zip(sizes, strides)])


def refine64_pyramid(pred_rows, batch, sizes, strides, anchor_scale=4.0):
    """the pyramid-packed layout: pred_rows [P, >=5] (first five columns = deltas) -> (out [P,5], magnitude)"""
    p = _f64(pred_rows)[:, :5]
    return decode64(pyramid_anchors64(batch, sizes, strides, anchor_scale), p, 1e-6)


def align_offsets64(anchors, feat_h, feat_w, stride, k=3):
    """AlignConv.get_offset in float64: anchors [B,H*W,5] -> (offset [B,2kk,H,W], magnitude); channel 2t = dy,
    2t+1 = dx, tap t = ky*k + kx.  magnitude = |xr| + |x_ctr| + |xc + xx|: the subtraction cancels."""
    a = _f64(anchors).reshape(-1, feat_h * feat_w, 5)
    B = a.shape[0]
    pad = (k - 1) // 2
    idx = np.arange(-pad, pad + 1, dtype=np.float64)
    yy, xx = (g.reshape(-1) for g in np.meshgrid(idx, idx, indexing="ij"))          # tap t = ky*k + kx
    ycg, xcg = (g.reshape(-1) for g in np.meshgrid(np.arange(feat_h, dtype=np.float64), np.arange(feat_w, dtype=np.float64),
                                                   indexing="ij"))
    x_conv, y_conv = xcg[None, :, None] + xx, ycg[None, :, None] + yy               # [1, HW, kk]
    x_ctr, y_ctr, w, h = (a[..., i, None] / stride for i in range(4))
    cs, sn = np.cos(a[..., 4, None]), np.sin(a[..., 4, None])
    x, y = w / k * xx, h / k * yy
    xr, yr = cs * x - sn * y, sn * x + cs * y
    off = np.stack([yr + y_ctr - y_conv, xr + x_ctr - x_conv], -1)                  # [B, HW, kk, (dy, dx)]
    mag = np.stack([np.abs(yr) + np.abs(y_ctr) + np.abs(y_conv), np.abs(xr) + np.abs(x_ctr) + np.abs(x_conv)], -1)

    def planes(t):
        return np.ascontiguousarray(t.reshape(B, feat_h * feat_w, 2 * k * k).transpose(0, 2, 1)).reshape(B, 2 * k * k, feat_h, feat_w)
    return planes(off), planes(mag)


def sigmoid64(x):
    """1 / (1 + exp(-x)) without overflow; -inf -> 0, +inf -> 1"""
    x = _f64(x)
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def select_topk(keys, k):
    """the rule k_pyr_topk documents: all rows strictly above the k-th largest key, then rows equal to it, lowest
    position first; returned ascending.  Every row when there are no more than k (or k <= 0)."""
    keys = np.asarray(keys)
    n = keys.shape[0]
    if k <= 0 or n <= k:
        return np.arange(n)
    kth = np.sort(keys)[n - k]
    above = np.nonzero(keys > kth)[0]
    equal = np.nonzero(keys == kth)[0][:k - above.size]
    return np.sort(np.concatenate([above, equal]))


def bias_act_ref(y, b, r, relu, dtype):
    """the epilogue kernel's own three roundings on the CPU, in its order: f32 (y + b), then + r, ReLU, ONE rounding to
    the storage type.  IEEE additions and no products: the result is fully determined, so the kernel must match it bit
    for bit.  y, r [B,C,H,W] and b [C] are taken in the storage type `dtype` (np.float16 / np.float32).
    Under ReLU a NaN becomes 0 (fmaxf(NaN, 0) = 0: the documented inference rule, DESIGN.md "Non-finite values");
    without ReLU NaN and +-inf pass through."""
    y = np.asarray(y, dtype)
    f = y.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = f + np.asarray(b, dtype).astype(np.float32).reshape(1, -1, 1, 1)
        if r is not None:
            f = f + np.asarray(r, dtype).astype(np.float32)
        if relu:
            f = np.where(f > 0, f, np.float32(0))                  # NaN > 0 is false
        return f.astype(dtype)
