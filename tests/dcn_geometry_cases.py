"""The deformable-convolution case matrix, its inputs, the counted bounds and the one comparator shared by
tests/test_dcn64_general_cpu.py (which proves on the CPU that every case can see the defects it is there for) and
tests/test_gpu_dcn_geometry.py (which holds the kernels to the float64 reference of oracle/dcn64_general.py).

Inputs are drawn on the CPU from a seeded generator, so both files see the same numbers."""
import math
import zlib

import torch

U16, U32, U64 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -53
UNIT = {torch.float16: U32, torch.float32: U32, torch.float64: U64}     # f16 kernels compute in f32
HALF_TINY = 2.0 ** -25                          # half an f16 subnormal step: the absolute error of an underflowed f16


def case(id, B=2, C=8, O=6, H=9, W=11, k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1), g=1, dg=1, wild=False):
    return dict(id=id, B=B, C=C, O=O, H=H, W=W, k=k, s=s, p=p, d=d, g=g, dg=dg, wild=wild)


# one factor at a time off the base case, always with H != W values, then combined
GEOMETRY = (
    case("base"),
    case("k1x1", k=(1, 1), p=(0, 0)), case("k5x3", k=(5, 3), p=(2, 1)), case("k2x2", k=(2, 2), p=(0, 0)),
    case("k1x3", k=(1, 3), p=(0, 1)),
    case("s2x1", s=(2, 1)), case("s1x3", s=(1, 3)), case("s3x2", s=(3, 2)),
    case("p0x0", p=(0, 0)), case("p0x2", p=(0, 2)), case("p3x1", p=(3, 1)),
    case("d2x1", d=(2, 1)), case("d1x3", d=(1, 3)),
    case("g2", O=8, g=2), case("g4", O=8, g=4), case("dg2", dg=2), case("dg4", dg=4),
    case("g2_dg4", O=8, g=2, dg=4), case("g4_dg2", O=8, g=4, dg=2),
    case("c6_o5", C=6, O=5),
    case("combined", k=(3, 5), s=(2, 1), p=(2, 0), d=(1, 2), g=2, dg=2),
)
# k_def_col2im_tiled: 3x3 / s1 / d1, (C/dg) % 8 == 0; 8 x 32 tiles, partial both ways; offsets beyond the 6-pixel halo
# (unpadded cases on the larger map: a 7 x 31 output is one tile whose window covers the whole 9 x 33 image)
TILED = (
    case("tiled_dg1_p0x0", C=16, H=17, W=45, p=(0, 0), wild=True),
    case("tiled_dg1_p1x1", C=16, H=9, W=33, p=(1, 1), wild=True),
    case("tiled_dg1_p2x3", C=16, H=9, W=33, p=(2, 3), wild=True),
    case("tiled_dg2_p0x0", C=16, H=17, W=45, p=(0, 0), dg=2, wild=True),
    case("tiled_dg2_p1x1", C=16, H=9, W=33, p=(1, 1), dg=2, wild=True),
    case("tiled_dg2_p2x3", C=16, H=17, W=45, p=(2, 3), dg=2, wild=True),
    case("tiled_g2_dg1_p2x3", C=16, H=9, W=33, p=(2, 3), g=2, wild=True),
    case("tiled_g2_dg2_p0x0", C=16, H=17, W=45, p=(0, 0), g=2, dg=2, wild=True),
)
# both neighbours of every dispatch limit, AlignConv geometry on 5 x 7 maps (and the 2 x 7 map that breaks H >= 3)
BOUNDARY = tuple(case("align_c%d_o%d" % (C, O), B=2, C=C, O=O, H=5, W=7)
                 for C, O in ((32, 64), (24, 64), (32, 48), (64, 64), (32, 16), (32, 8), (64, 32), (64, 16), (64, 272)))
THIN = case("align_c64_o32_2x7", B=2, C=64, O=32, H=2, W=7)
# im2col_step chunking (B 4 in steps of 2, B 3 in steps of 1 and 3), a 3-D call, and what DeformConv makes of a 3 x 4
# map under a 5 x 5 kernel (zero-padded to 5 x 5, the result cropped)
STEP = {4: case("step_b4", B=4, s=(2, 1), g=2, dg=2), 3: case("step_b3", B=3, O=8, p=(0, 2), g=2, dg=4)}
RANK3 = case("rank3", B=1, s=(1, 2), g=2, dg=2)
MODULE = case("module_5x5_on_3x4", H=5, W=5, k=(5, 5), p=(2, 2), dg=2)
ALL = {c["id"]: c for c in GEOMETRY + TILED + BOUNDARY + (THIN, STEP[4], STEP[3], RANK3, MODULE)}


def geom(c):
    return dict(stride=c["s"], padding=c["p"], dilation=c["d"], groups=c["g"], deformable_groups=c["dg"])


def out_hw(c):
    (kH, kW), (sH, sW), (pH, pW), (dH, dW) = c["k"], c["s"], c["p"], c["d"]
    return (c["H"] + 2 * pH - (dH * (kH - 1) + 1)) // sH + 1, (c["W"] + 2 * pW - (dW * (kW - 1) + 1)) // sW + 1


# ----------------------------------------------------------------------------- inputs
def _edge_block(gen, off, c):
    """image 0, first and last output row: samples moved onto exact integers (-1 and H included), into the bands (-1, 0)
    and (H-1, H), within a few 2^-12 of the far edge, and far outside (edge_block of test_gpu_dcn_backward_shapes.py at
    the case's geometry).  Every seventh sample of a row is put on h = -1 (w = -1 three further on) with the other
    coordinate inside the image: the points that tell the band -1 < h from -1 <= h."""
    (kH, kW), (sH, sW), (pH, pW), (dH, dW) = c["k"], c["s"], c["p"], c["d"]
    H, W, dg, T = c["H"], c["W"], c["dg"], kH * kW
    Ho, Wo = off.shape[2:]
    v = off.view(off.shape[0], dg, T, 2, Ho, Wo)
    t = torch.arange(T)
    shape = (dg, T, Wo)

    def pick(n):
        kind = torch.randint(0, 6, shape, generator=gen)
        r = torch.rand(shape, generator=gen)
        kk = torch.randint(1, 4, shape, generator=gen).float()
        return torch.where(kind == 0, torch.randint(-1, n + 1, shape, generator=gen).float(),
               torch.where(kind == 1, -0.05 - 0.9 * r,
               torch.where(kind == 2, n - 0.95 + 0.9 * r,
               torch.where(kind == 3, torch.where(r < 0.5, -30.0, n + 30.0),
               torch.where(kind == 4, n - kk * 2.0 ** -12,
                           torch.randint(0, n, shape, generator=gen).float() + 0.5)))))

    n = torch.arange(dg * T * Wo).view(shape)
    for r0 in sorted({0, Ho - 1}):
        base_h = (r0 * sH - pH + (t // kW) * dH).float().view(1, T, 1)
        base_w = ((torch.arange(Wo) * sW - pW).view(1, 1, Wo) + ((t % kW) * dW).view(1, T, 1)).float()
        th, tw = pick(H), pick(W)
        th = torch.where(n % 7 == 0, torch.tensor(-1.0), torch.where(n % 7 == 3, (n % H).float() + 0.25, th))
        tw = torch.where(n % 7 == 0, (n % W).float() + 0.25, torch.where(n % 7 == 3, torch.tensor(-1.0), tw))
        v[0, :, :, 0, r0] = th - base_h
        v[0, :, :, 1, r0] = tw - base_w


def make_inputs(c, modulated=False):
    """-> dict of float32 CPU tensors: x, offset, weight, grad_out (30 % exact zeros), and for the modulated form mask
    (in [0, 1] with exact zeros and ones) and bias"""
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()) + (1 if modulated else 0))
    B, C, O, H, W, (kH, kW), g, dg = c["B"], c["C"], c["O"], c["H"], c["W"], c["k"], c["g"], c["dg"]
    Ho, Wo = out_hw(c)
    T = kH * kW
    r = {"x": torch.randn((B, C, H, W), generator=gen),
         "weight": torch.randn((O, C // g, kH, kW), generator=gen) / math.sqrt(C // g * T)}
    if c["wild"]:
        off = 4.0 * torch.randn((B, dg * 2 * T, Ho, Wo), generator=gen)
        far = torch.rand(off.shape, generator=gen) < 0.03
        off = torch.where(far, torch.where(torch.rand(off.shape, generator=gen) < 0.5, -10.0, 10.0) + off / 8, off)
    else:
        off = 1.5 * torch.randn((B, dg * 2 * T, Ho, Wo), generator=gen)
    _edge_block(gen, off, c)
    r["offset"] = off
    go = torch.randn((B, O, Ho, Wo), generator=gen)
    r["grad_out"] = go.masked_fill(torch.rand(go.shape, generator=gen) < 0.3, 0)
    if modulated:
        m = torch.rand((B, dg * T, Ho, Wo), generator=gen)
        sel = torch.rand(m.shape, generator=gen)
        r["mask"] = torch.where(sel < 0.1, 0.0, torch.where(sel > 0.9, 1.0, m))
        r["bias"] = torch.randn((O,), generator=gen)
    return r


def as_kernel_sees(inp, dtype):
    """the values a `dtype` call hands the kernels, as float32 / float64 tensors (float16: rounded once)"""
    if dtype == torch.float16:
        return {k: v.half().float() for k, v in inp.items()}
    return {k: v.to(dtype) for k, v in inp.items()}


def beyond_halo_share(c, offset):
    """share of the samples inside the image with a corner outside the (8 + 2 + 12) x (32 + 2 + 12) window of their
    8 x 32 tile of output positions: k_def_col2im_tiled adds those straight to memory"""
    from oracle.dcn64_general import sample_points
    h, w = sample_points(offset, c["k"], c["s"], c["p"], c["d"], c["dg"], torch.float32)
    Ho, Wo = out_hw(c)
    dev = offset.device
    y0 = (torch.arange(Ho, device=dev) // 8 * 8 - c["p"][0] - 6).view(1, 1, 1, Ho, 1)
    x0 = (torch.arange(Wo, device=dev) // 32 * 32 - c["p"][1] - 6).view(1, 1, 1, 1, Wo)
    inside = (h > -1) & (w > -1) & (h < c["H"]) & (w < c["W"])
    far = (h.floor() < y0) | (h.floor() + 1 >= y0 + 22) | (w.floor() < x0) | (w.floor() + 1 >= x0 + 46)
    return (far & inside).double().mean().item()


# ----------------------------------------------------------------------------- counted bounds
def tau_forward(dtype, Cg, T):
    K = Cg * T
    return (2 * U16 if dtype == torch.float16 else 0.0) + (K + 8) * UNIT[dtype]


def tau_input(dtype, Og, max_m):
    return (2 * U16 if dtype == torch.float16 else 0.0) + (Og + max_m + 16) * UNIT[dtype]


def tau_offset(dtype, Og, Cdg):
    return (2 * U16 if dtype == torch.float16 else 0.0) + (Og + Cdg + 16) * UNIT[dtype]


def tau_weight(dtype, positions_per_chunk, chunks):
    return ((1 + chunks) * U16 if dtype == torch.float16 else 0.0) + (positions_per_chunk + chunks + 16) * UNIT[dtype]


L2_BOUND = {torch.float16: 2 * U16, torch.float32: 64 * U32, torch.float64: 64 * U64}


def generic_bounds(c, dtype, ref, chunks=1, weight=None):
    """{tensor: (tau, tiny)} of the generic forward and the unfused backward for a case (the counting is written out in
    the docstring of tests/test_gpu_dcn_geometry.py).  tiny: the absolute floor -- for float16 what an underflowed
    column entry or result (error <= 2^-25 each) adds up to in that tensor."""
    (kH, kW), g, dg = c["k"], c["g"], c["dg"]
    Cg, Og, T = c["C"] // g, c["O"] // g, kH * kW
    Ho, Wo = out_hw(c)
    f16 = dtype == torch.float16
    b = {"out": (tau_forward(dtype, Cg, T), 1e-30)}
    if f16 and weight is not None:
        b["out"] = (b["out"][0], HALF_TINY * (1 + weight.double().abs().sum((1, 2, 3)).view(1, -1, 1, 1)))
    if "grad_input" in ref:
        go_l1 = ref["go_l1"]
        b["grad_input"] = (tau_input(dtype, Og, ref["M"].max().item()), HALF_TINY * (1 + ref["M"]) if f16 else 1e-30)
        b["grad_offset"] = (tau_offset(dtype, Og, c["C"] // dg), HALF_TINY * (1 + ref["cw_abs"]) if f16 else 1e-30)
        b["grad_weight"] = (tau_weight(dtype, c["B"] // chunks * Ho * Wo, chunks),
                            HALF_TINY * (1 + chunks + go_l1.view(-1, 1, 1, 1)) if f16 else 1e-30)
    return b


SCALE = {"out": "S_out", "grad_input": "S_input", "grad_offset": "S_offset", "grad_weight": "S_weight"}


def compare(got, ref, S, tau, tiny, l2_bound):
    """THE comparator: every element within tau * S + tiny, and the tensor's relative L2 error within l2_bound.
    -> dict(ratio = largest error over bound, l2, ok).  A NaN anywhere fails."""
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    err = (got.detach().double() - ref).abs()
    bound = tau * S + tiny
    ratio = torch.nan_to_num(err / bound, nan=math.inf).max().item()
    l2 = err.norm().item() / max(ref.norm().item(), 1e-300)
    ok = bool((err <= bound).all()) and l2 <= l2_bound
    return dict(ratio=ratio, tau=tau, l2=l2, l2_bound=l2_bound, l2_ratio=l2 / l2_bound, ok=ok)


def reference(c, vals, dtype, backward=True, defect=None, scale=True):
    """the float64 reference of a case on the device `vals` are on, sampled at the points a `dtype` kernel forms
    (float32 positions for float16 / float32 kernels, float64 ones for the float64 instantiation)"""
    from oracle.dcn64_general import deform_conv_general64
    r = deform_conv_general64(vals["x"], vals["offset"], vals["weight"], vals["grad_out"] if backward else None,
                              mask=vals.get("mask"), bias=vals.get("bias"), scale=scale, defect=defect,
                              pos_dtype=None if dtype == torch.float64 else torch.float32, **geom(c))
    if backward:
        r["go_l1"] = vals["grad_out"].double().abs().sum((0, 2, 3))     # per out-channel: what a column's floor meets
    return r
