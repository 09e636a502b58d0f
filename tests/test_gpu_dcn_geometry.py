"""GPU: the deformable convolution at every geometry the package exports -- any kernel size, stride, padding, dilation,
groups, deformable groups and im2col_step, f16 / f32 / f64, forward, all three gradients and the modulated forward --
against the general float64 reference (oracle/dcn64_general.py).  The cases (tests/dcn_geometry_cases.py) are the
smallest that can still go wrong: every factor off the base case one at a time with H != W values, then combined;
partial 8 x 32 tiles of k_def_col2im_tiled with samples beyond its halo; both neighbours of every dispatch limit; edge
samples in every case; NCHW, channels-last, sliced and 3-D tensors.  tests/test_dcn64_general_cpu.py shows on the CPU
that every case rejects every wrong reading of the definition its geometry can express.

Every element of every tensor goes through one comparator (dcn_geometry_cases.compare):
    |got - ref| <= tau * S + tiny        and        ||got - ref|| / ||ref|| <= L2
S: the sum of the absolute values of the products behind the entry (the reference gives it); L2: 2 u16 (f16), 64 u32
(f32), as tests/test_gpu_dcn_backward_shapes.py, 64 u64 (f64).  tau is counted, one unit roundoff per rounding a product
of the sum sees (u = u32 for f16 and f32 kernels, which compute in f32; u64 for the f64 instantiation):

  k_dcn_generic (forward, modulated forward), K = C/g * kH * kW products per output:
      the blend (1 - lh, 1 - lw, two products and the value: 5; three additions of the four corners: 3) = 8, the mask
      multiplies inside them; K fused multiply-adds                              -> (K + 8) u
      f16: the column rounded to f16 (as the fused path), the result rounded     -> 2 u16 + (K + 8) u32
  input gradient, unfused (library GEMM -> k_def_col2im / k_def_col2im_tiled):
      the column gradient is a sum over O/g; the scatter adds up to max M contributions into a cell (atomics or LDS
      adds, any order); blend weights and products: 16 covers them               -> (O/g + max M + 16) u
      f16: the GEMM hands the columns over in f16, the result is rounded         -> + 2 u16
  offset gradient (k_def_col2im_coord): columns as above, a sum over the C/dg channels of the deformable group of four
      products each                                                              -> (O/g + C/dg + 16) u   (+ 2 u16)
  weight gradient (k_def_im2col -> library GEMM per chunk of im2col_step images, chunks added in f32):
      positions per chunk + chunks + 16 (the column's blend)                     -> (P + chunks + 16) u
      f16: f16 columns (u16), each chunk's GEMM result handed over in f16 (chunks u16; the final f16 rounding is the
      last chunk's when there is one chunk, and at most one more otherwise)      -> + (1 + chunks) u16
  tiny: 1e-30; f16: 2^-25 (half a subnormal step) for an underflowed result plus 2^-25 per underflowed f16 column
      entry times what multiplies it: sum |w| (forward), M (input), the coordinate weights (offset), sum |grad_out|
      (weight).
Calls that dispatch to the fused kernels (the fast forward, _fused_backward, the _fused_bwd_ok routes) are held to the
bounds tests/test_gpu_forward_shapes.py and tests/test_gpu_dcn_backward_shapes.py derive for those kernels, imported
from there: the point of those cases is that both neighbours of a limit agree with the same reference.

One rounding the first count missed, found by the k1x1 case: k_def_col2im formed the scatter weight as the reference
does, (ah + 1 - h), whose first addition rounds at the size of the COORDINATE (absolute error u32 * (|ah| + 1)), not of
the weight: a weight of 0.012 at row 8 carried a relative error of 4e-5.  The kernel now forms the fraction first
(ah - floor(ah), exact) as k_def_col2im_tiled and the forward do.  Error over bound of the f32 input gradient before ->
after: k1x1 3.22 -> 0.07, s3x2 0.87 -> 0.06, s1x3 0.72 -> 0.05 (f16 and f64 unchanged: 0.72 / 0.07 at most).

Set S2A_DCN_GEOMETRY_REPORT=<path> to write every measured ratio (error over bound) as JSON; the committed run is
profiles/dcn_geometry_ratios.json (699 comparisons, all inside their bounds).  The largest elementwise ratio per kernel
and dtype in that run (f16 / f32 / f64), the largest relative-L2 ratio in brackets:
  k_dcn_generic       0.70 / 0.14 / 0.15   [0.34 / 0.10 / 0.04]      k_def_im2col (weight)   0.80 / 0.07 / 0.03   [0.41 / 0.09 / 0.07]
  k_def_col2im        0.72 / 0.22 / 0.14   [0.47 / 0.03 / 0.04]      k_def_col2im_tiled      0.57 / 0.04 / -      [0.31 / 0.07 / -]
  k_def_col2im_coord  0.79 / 0.17 / 0.16   [0.36 / 0.08 / 0.03]
  fused kernels at the dispatch limits, under their own bounds: forward 0.05 / 0.01, input and offset gradient
  0.25 / 0.03, weight gradient 0.25 / 0.05
"""
import contextlib
import json
import os

import pytest
import torch

import dcn_geometry_cases as G
from test_gpu_dcn_backward_shapes import tau as tau_fused_bwd, walk as fused_walk
from test_gpu_forward_shapes import L2_DCN, L2_F32, tau as tau_fused_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAME = {F16: "f16", F32: "f32", F64: "f64"}
REPORT = []


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def values(c, dtype, modulated=False, f32_offsets=False):
    """what the kernels get, as f32 / f64 tensors on the GPU.  f16 with f32_offsets: the offsets stay unrounded (the
    forward takes them as they are); otherwise an f16 call rounds them (the backward does, _bwd_common)"""
    raw = G.make_inputs(c, modulated)
    v = G.as_kernel_sees(raw, dtype)
    if f32_offsets:
        v["offset"] = raw["offset"]
    return {k: t.to(DEV) for k, t in v.items()}


def tiled_col2im(c, dtype):
    return (c["k"] == (3, 3) and c["s"] == (1, 1) and c["d"] == (1, 1) and (c["C"] // c["dg"]) % 8 == 0 and dtype != F64)


def aligned(c):
    return (c["k"], c["s"], c["p"], c["d"], c["g"], c["dg"]) == ((3, 3), (1, 1), (1, 1), (1, 1), 1, 1)


def route(c, dtype, tensor, f32_offsets=True, simple=False):
    """the kernel a tensor of this call comes from (the dispatch rules of s2anet_amd/dcn.py and the library)"""
    C, O, big = c["C"], c["O"], c["H"] >= 3 and c["W"] >= 3
    fusable = aligned(c) and dtype != F64 and O <= 256 and big
    if tensor == "out":
        fast = aligned(c) and dtype != F64 and f32_offsets and C % (32 if dtype == F32 else 64) == 0 and O % 64 == 0
        return "fast_forward" if fast else "k_dcn_generic"
    if tensor == "grad_weight":
        return "fused_weight" if fusable and C % 64 == 0 and O % 32 == 0 else "k_def_im2col"
    if fusable and C % 32 == 0 and O % 16 == 0:
        return "fused_input"
    if tensor == "grad_offset":
        return "k_def_col2im_coord"
    return "k_def_col2im_tiled" if tiled_col2im(c, dtype) and not simple else "k_def_col2im"


def bounds_for(c, dtype, ref, weight, chunks=1, f32_offsets=True, simple=False):
    """{tensor: (kernel, tau, tiny, l2)}"""
    b = G.generic_bounds(c, dtype, ref, chunks, weight)
    out = {}
    for k, (t, tiny) in b.items():
        kern = route(c, dtype, k, f32_offsets, simple)
        l2 = G.L2_BOUND[dtype]
        if kern == "fast_forward":
            t, tiny = tau_fused_fwd("dcn16" if dtype == F16 else "dcn32_x3", c["C"] * 9), G.HALF_TINY
            l2 = L2_DCN if dtype == F16 else L2_F32
        elif kern.startswith("fused"):
            w_ = fused_walk(dtype, c["B"], c["C"], c["H"], c["W"]) if c["C"] % 64 == 0 else (1, 1)
            t = tau_fused_bwd(dtype, "f16" if dtype == F16 else "x3", k[len("grad_"):], c["C"], c["O"], *w_)
            if dtype == F16:
                tiny = G.HALF_TINY * (1 + ref["go_l1"].view(-1, 1, 1, 1)) if k == "grad_weight" else G.HALF_TINY
        out[k] = (kern, t, tiny, l2)
    return out


def check(label, c, dtype, got, ref, bounds, extra_tiny=None):
    """every tensor of `got` through the comparator; records the ratios; asserts at the end so that all are recorded"""
    bad = []
    for k, g in got.items():
        kern, t, tiny, l2 = bounds[k]
        if extra_tiny and k in extra_tiny:
            tiny = tiny + extra_tiny[k]
        m = G.compare(g, ref[k], ref[G.SCALE[k]], t, tiny, l2)
        REPORT.append(dict(test=label, case=c["id"], dtype=NAME[dtype], tensor=k, kernel=kern, ratio=m["ratio"], tau=m["tau"],
                           l2_ratio=m["l2_ratio"], ok=m["ok"]))
        print("%-44s %-22s %s %-11s %-18s ratio %.3f  l2/bound %.3f" % (label, c["id"], NAME[dtype], k, kern, m["ratio"],
                                                                       m["l2_ratio"]))
        if not m["ok"]:
            bad.append((k, kern, m))
    path = os.environ.get("S2A_DCN_GEOMETRY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)
    assert not bad, (label, c["id"], NAME[dtype], bad)


def run_autograd(c, v, dtype, needs=("x", "offset", "weight"), step=64, prepare=None, offset_dtype=None):
    """deform_conv through autograd -> {out, grad_*} for the inputs in `needs`"""
    from s2anet_amd import deform_conv
    t = {k: v[k].to(dtype) for k in ("x", "offset", "weight", "grad_out")}
    if offset_dtype is not None:
        t["offset"] = v["offset"].to(offset_dtype)
    if prepare:
        t = prepare(t)
    leaves = {k: t[k].detach().requires_grad_(k in needs) for k in ("x", "offset", "weight")}
    out = deform_conv(leaves["x"], leaves["offset"], leaves["weight"], c["s"], c["p"], c["d"], c["g"], c["dg"], step)
    order = [k for k in ("x", "offset", "weight") if k in needs]
    grads = torch.autograd.grad(out, [leaves[k] for k in order], t["grad_out"])
    got = {"out": out.detach()}
    for k, g in zip(order, grads):
        got[{"x": "grad_input", "offset": "grad_offset", "weight": "grad_weight"}[k]] = g
    return got


def pybind_args(c):
    (kH, kW), (sH, sW), (pH, pW), (dH, dW) = c["k"], c["s"], c["p"], c["d"]
    return (kW, kH, sW, sH, pW, pH, dW, dH, c["g"], c["dg"])


def run_pybind_backward(c, v, dtype, step, scale=1.0, init=None, squeeze=False):
    """the two pybind-shaped backward functions -> {grad_*}; init: what gradInput / gradWeight hold before the call"""
    from s2anet_amd.dcn import deform_conv_backward_input_cuda, deform_conv_backward_parameters_cuda
    t = {k: v[k].to(dtype) for k in ("x", "offset", "weight", "grad_out")}
    if squeeze:
        t = {k: (a[0] if k != "weight" else a) for k, a in t.items()}
    gin = torch.zeros_like(t["x"]) if init is None else torch.full_like(t["x"], init)
    goff = torch.full_like(t["offset"], float("nan"))              # overwritten, never accumulated into
    gw = torch.zeros_like(t["weight"]) if init is None else torch.full_like(t["weight"], init)
    r1 = deform_conv_backward_input_cuda(t["x"], t["offset"], t["grad_out"], gin, goff, t["weight"], None,
                                         *pybind_args(c), step)
    r2 = deform_conv_backward_parameters_cuda(t["x"], t["offset"], t["grad_out"], gw, None, None, *pybind_args(c),
                                              scale, step)
    assert r1 == 1 and r2 == 1
    if squeeze:
        gin, goff = gin.unsqueeze(0), goff.unsqueeze(0)
    return {"grad_input": gin, "grad_offset": goff, "grad_weight": gw}


DT_IDS = dict(ids=lambda d: NAME[d])


# ----------------------------------------------------------------------------- the geometry matrix
@pytest.mark.parametrize("dtype", (F32, F16, F64), **DT_IDS)
@pytest.mark.parametrize("c", G.GEOMETRY, ids=lambda c: c["id"])
def test_geometry(c, dtype):
    """forward and all three gradients; f16 with f16 offsets (k_dcn_generic<half, half>, the backward's own rounding)"""
    v = values(c, dtype)
    ref = G.reference(c, v, dtype)
    got = run_autograd(c, v, dtype)
    check("geometry", c, dtype, got, ref, bounds_for(c, dtype, ref, v["weight"], f32_offsets=False))
    if tiled_col2im(c, dtype):
        with env(S2A_COL2IM_SIMPLE="1"):
            got = run_autograd(c, v, dtype, needs=("x", "offset"))
        check("geometry:simple_col2im", c, dtype, {"grad_input": got["grad_input"]}, ref,
              bounds_for(c, dtype, ref, v["weight"], f32_offsets=False, simple=True))


@pytest.mark.parametrize("c", G.GEOMETRY, ids=lambda c: c["id"])
def test_geometry_f16_forward_f32_offsets(c):
    """k_dcn_generic<half, float>: the forward takes f32 offsets unrounded"""
    from s2anet_amd import deform_conv
    v = values(c, F16, f32_offsets=True)
    ref = G.reference(c, v, F16, backward=False)
    out = deform_conv(v["x"].half(), v["offset"], v["weight"].half(), c["s"], c["p"], c["d"], c["g"], c["dg"])
    assert out.dtype == F16
    check("forward_f16_f32_offsets", c, F16, {"out": out}, ref, bounds_for(c, F16, ref, v["weight"]))


# ----------------------------------------------------------------------------- the tiled scatter
@pytest.mark.parametrize("dtype", (F32, F16), **DT_IDS)
@pytest.mark.parametrize("c", G.TILED, ids=lambda c: c["id"])
def test_tiled_col2im(c, dtype):
    """k_def_col2im_tiled at every padding and deformable-group count, partial tiles both ways, samples beyond the halo;
    the same call on k_def_col2im (S2A_COL2IM_SIMPLE=1): each against float64"""
    assert tiled_col2im(c, dtype)
    v = values(c, dtype)
    assert G.beyond_halo_share(c, v["offset"]) > 0.002
    ref = G.reference(c, v, dtype)
    got = run_autograd(c, v, dtype)
    check("tiled", c, dtype, got, ref, bounds_for(c, dtype, ref, v["weight"], f32_offsets=False))
    with env(S2A_COL2IM_SIMPLE="1"):
        got = run_autograd(c, v, dtype, needs=("x", "offset"))
    check("tiled:simple_col2im", c, dtype, {"grad_input": got["grad_input"]}, ref,
          bounds_for(c, dtype, ref, v["weight"], f32_offsets=False, simple=True))


# ----------------------------------------------------------------------------- im2col_step and the pybind contracts
U_STORE = {F16: G.U16, F32: G.U32, F64: G.U64}


@pytest.mark.parametrize("columns_mb", (None, "0"), ids=("cache_chunks", "reference_chunks"))
@pytest.mark.parametrize("dtype", (F32, F16, F64), **DT_IDS)
@pytest.mark.parametrize("B,step", ((4, 2), (3, 1), (3, 3)))
def test_im2col_step_accumulate_and_scale(B, step, dtype, columns_mb):
    """the pybind-shaped backward functions chunk by im2col_step, ACCUMULATE into a non-zero gradInput / gradWeight,
    honour scale != 1 and return 1"""
    c = G.STEP[B]
    v = values(c, dtype)
    ref = G.reference(c, v, dtype)
    init, scale = 0.375, 0.75                                     # exact in every type; scaling by 0.75 rounds once more
    with env(S2A_DCN_COLUMNS_MB=columns_mb):
        got = run_pybind_backward(c, v, dtype, step, scale=scale, init=init)
    sref = dict(ref)
    sref["grad_weight"], sref["S_weight"] = scale * ref["grad_weight"], scale * ref["S_weight"]
    got["grad_input"] = got["grad_input"].double() - init
    got["grad_weight"] = got["grad_weight"].double() - init
    b = bounds_for(c, dtype, ref, v["weight"], chunks=B // step, f32_offsets=False)
    kern, t, tiny, l2 = b["grad_weight"]
    b["grad_weight"] = (kern, t + G.UNIT[dtype], tiny, l2)        # the multiplication by scale
    # the accumulation rounds init + gradient once in the tensor's own type
    u = U_STORE[dtype]
    extra = {"grad_input": u * (init + ref["grad_input"].abs()), "grad_weight": u * (init + sref["grad_weight"].abs())}
    check("im2col_step_%d_of_%d" % (step, B) + ("" if columns_mb is None else ":columns_mb_0"), c, dtype, got, sref, b, extra)


def test_backward_shape_errors_at_dg2():
    from s2anet_amd.dcn import deform_conv_backward_input_cuda, deform_conv_backward_parameters_cuda
    c = G.ALL["dg2"]
    v = values(c, F32)
    bad_off = v["offset"][:, :18].contiguous()                     # the channels of ONE deformable group
    gin, gw = torch.zeros_like(v["x"]), torch.zeros_like(v["weight"])
    with pytest.raises(RuntimeError, match="invalid number of channels of offset"):
        deform_conv_backward_input_cuda(v["x"], bad_off, v["grad_out"], gin, torch.zeros_like(bad_off), v["weight"], None,
                                        *pybind_args(c), 2)
    with pytest.raises(RuntimeError, match="invalid number of channels of offset"):
        deform_conv_backward_parameters_cuda(v["x"], bad_off, v["grad_out"], gw, None, None, *pybind_args(c), 1.0, 2)
    with pytest.raises(RuntimeError, match="invalid size of gradOutput"):
        deform_conv_backward_input_cuda(v["x"], v["offset"], v["grad_out"][:, :, 1:], gin, torch.zeros_like(v["offset"]),
                                        v["weight"], None, *pybind_args(c), 2)
    with pytest.raises(RuntimeError, match="invalid batch size of offset"):
        deform_conv_backward_parameters_cuda(v["x"], v["offset"][:1], v["grad_out"], gw, None, None, *pybind_args(c), 1.0, 2)
    assert not gin.any() and not gw.any()


# ----------------------------------------------------------------------------- dispatch boundaries
FWD_BOUNDARY = (("align_c32_o64", F32, True), ("align_c24_o64", F32, True), ("align_c32_o48", F32, True),
                ("align_c64_o64", F16, True), ("align_c32_o64", F16, True), ("align_c64_o64", F16, False))


@pytest.mark.parametrize("layout", ("nchw", "channels_last"))
@pytest.mark.parametrize("cid,dtype,f32_offsets", FWD_BOUNDARY,
                         ids=["%s-%s-%s" % (a, NAME[b], "off32" if o else "off16") for a, b, o in FWD_BOUNDARY])
def test_forward_dispatch_boundaries(cid, dtype, f32_offsets, layout):
    """both neighbours of every limit of fast_path_ok against the same reference, NCHW and channels-last: the fused
    kernels keep their no-copy channels-last route and output; next to them the generic kernel gets contiguous copies
    (a channels-last call there raised "the generic path supports NCHW only")"""
    from s2anet_amd import deform_conv
    c = G.ALL[cid]
    v = values(c, dtype, f32_offsets=f32_offsets and dtype == F16)
    ref = G.reference(c, v, dtype, backward=False)
    x = v["x"].to(dtype)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    off = v["offset"] if f32_offsets else v["offset"].to(dtype)
    with env(S2A_DCN_F32=None):
        out = deform_conv(x, off, v["weight"].to(dtype), 1, 1, 1, 1, 1)
    kern = route(c, dtype, "out", f32_offsets)
    assert kern == ("fast_forward" if cid in ("align_c32_o64", "align_c64_o64") and f32_offsets
                    and (dtype == F32 or c["C"] == 64) else "k_dcn_generic")
    if layout == "channels_last":
        assert out.is_contiguous(memory_format=torch.channels_last)
    else:
        assert out.is_contiguous()
    check("forward_boundary:" + layout, c, dtype, {"out": out}, ref, bounds_for(c, dtype, ref, v["weight"], f32_offsets=f32_offsets))


BWD_BOUNDARY = ("align_c32_o16", "align_c32_o8", "align_c64_o32", "align_c64_o16", "align_c64_o272")
NEEDS = {"input_offset": ("x", "offset"), "weight": ("weight",), "all": ("x", "offset", "weight")}


@pytest.mark.parametrize("needs", tuple(NEEDS))
@pytest.mark.parametrize("dtype", (F32, F16), **DT_IDS)
@pytest.mark.parametrize("cid", BWD_BOUNDARY)
def test_backward_dispatch_boundaries(cid, dtype, needs):
    """both neighbours of the limits of dcn._fused_bwd_ok for the input gradient (C % 32, O % 16, O <= 256), for the weight
    gradient and for both (_fused_backward_ok: C % 64, O % 32), under every needs_input_grad pattern: the separate entry points and the
    one-call _fused_backward all agree with the same reference"""
    c = G.ALL[cid]
    v = values(c, dtype, f32_offsets=True)            # the forward samples at f32 offsets ...
    vb = values(c, dtype)                             # ... the backward at the rounded ones (f16)
    ref = G.reference(c, vb, dtype)
    fwd = G.reference(c, v, dtype, backward=False)
    ref["out"], ref["S_out"] = fwd["out"], fwd["S_out"]
    with env(S2A_BWD_F32_WEIGHT=None, S2A_DCN_BWD_UNFUSED=None, S2A_DCN_BWD_SEPARATE=None, S2A_DCN_F32=None):
        got = run_autograd(c, v, dtype, NEEDS[needs], offset_dtype=F32)
    assert set(got) == {"out"} | {{"x": "grad_input", "offset": "grad_offset", "weight": "grad_weight"}[k] for k in NEEDS[needs]}
    check("backward_boundary:" + needs, c, dtype, got, ref, bounds_for(c, dtype, ref, v["weight"]))


@pytest.mark.parametrize("dtype", (F32, F16), **DT_IDS)
def test_backward_thin_map_breaks_h3(dtype):
    """2 x 7 at (C, O) = (64, 32): every other condition of the fused kernels holds, H >= 3 does not"""
    c = G.THIN
    v = values(c, dtype)
    ref = G.reference(c, v, dtype)
    assert route(c, dtype, "grad_input") == "k_def_col2im_tiled" and route(c, dtype, "grad_weight") == "k_def_im2col"
    got = run_pybind_backward(c, v, dtype, c["B"])
    check("backward_thin_2x7", c, dtype, got, ref, bounds_for(c, dtype, ref, v["weight"]))


# ----------------------------------------------------------------------------- layouts and ranks
def _channels_last(t):
    return dict(t, x=t["x"].contiguous(memory_format=torch.channels_last))


def _sliced(t):
    """x, offset and grad_output as non-contiguous slices of larger tensors"""
    def wrap(a):
        big = torch.full((a.shape[0], a.shape[1], a.shape[2] + 2, 2 * a.shape[3] + 1), 7.0, dtype=a.dtype, device=a.device)
        view = big[:, :, 1:-1, 1::2]
        view.copy_(a)
        assert not view.is_contiguous()
        return view
    return dict(t, x=wrap(t["x"]), offset=wrap(t["offset"]), grad_out=wrap(t["grad_out"]))


@pytest.mark.parametrize("dtype", (F32, F16, F64), **DT_IDS)
@pytest.mark.parametrize("prepare", (_channels_last, _sliced), ids=("channels_last", "sliced"))
@pytest.mark.parametrize("cid", ("s2x1", "g2", "tiled_g2_dg2_p0x0"))
def test_memory_formats(cid, prepare, dtype):
    """a channels-last or sliced input off the fused path gives the reference's values (the reference calls
    input.contiguous()); stride 2, C = 8 / 16 with groups = 2"""
    c = G.ALL[cid]
    v = values(c, dtype)
    ref = G.reference(c, v, dtype)
    got = run_autograd(c, v, dtype, prepare=prepare)
    assert got["grad_input"].shape == v["x"].shape
    check("memory_format:" + prepare.__name__.strip("_"), c, dtype, got, ref,
          bounds_for(c, dtype, ref, v["weight"], f32_offsets=False))


@pytest.mark.parametrize("dtype", (F32, F16), **DT_IDS)
def test_3d_input_through_pybind_functions(dtype):
    from s2anet_amd.dcn import deform_conv_forward_cuda
    c = G.RANK3
    v = values(c, dtype)
    ref = G.reference(c, v, dtype)
    got = run_pybind_backward(c, v, dtype, 1, squeeze=True)
    out = torch.full(ref["out"].shape[1:], float("nan"), dtype=dtype, device=DEV)
    assert deform_conv_forward_cuda(v["x"][0].to(dtype), v["weight"].to(dtype), v["offset"][0].to(dtype), out, None, None,
                                    *pybind_args(c), 1) == 1
    got["out"] = out.unsqueeze(0)
    check("rank3", c, dtype, got, ref, bounds_for(c, dtype, ref, v["weight"], f32_offsets=False))


@pytest.mark.parametrize("dtype", (F32, F16), **DT_IDS)
def test_module_on_a_map_smaller_than_its_kernel(dtype):
    """DeformConv pads a 3 x 4 map to its 5 x 5 kernel and crops the result: the reference does the same around the
    float64 operator, so the gradients are those of the padded call cropped back"""
    import torch.nn.functional as Fn
    from s2anet_amd import DeformConv
    padded = G.MODULE
    v = values(padded, dtype)
    live = torch.zeros((1, 1, 5, 5), device=DEV)
    live[:, :, :3, :4] = 1
    x, off, go = v["x"][:, :, :3, :4], v["offset"][:, :, :3, :4], v["grad_out"][:, :, :3, :4]
    vp = dict(v, x=v["x"] * live.to(v["x"].dtype), offset=v["offset"] * live.to(v["x"].dtype),
              grad_out=v["grad_out"] * live.to(v["x"].dtype))
    ref = G.reference(padded, vp, dtype)
    m = DeformConv(8, 6, 5, padding=2, deformable_groups=2).to(DEV).to(dtype)
    with torch.no_grad():
        m.weight.copy_(v["weight"])
    xl, ol = x.to(dtype).requires_grad_(True), off.to(dtype).requires_grad_(True)
    out = m(xl, ol)
    assert out.shape == go.shape
    gx, goff, gw = torch.autograd.grad(out, (xl, ol, m.weight), go.to(dtype))
    got = {"out": Fn.pad(out.detach(), (0, 1, 0, 2)), "grad_input": Fn.pad(gx, (0, 1, 0, 2)),
           "grad_offset": Fn.pad(goff, (0, 1, 0, 2)), "grad_weight": gw}
    # outside the crop the module computes nothing: the comparison there is 0 against the reference, so mask it
    for k in ("out", "grad_input", "grad_offset"):
        ref[k] = ref[k] * live
    check("module_pad_crop", padded, dtype, got, ref, bounds_for(padded, dtype, ref, v["weight"], f32_offsets=False))


# ----------------------------------------------------------------------------- modulated forward
@pytest.mark.parametrize("with_bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("dtype", (F32, F16), **DT_IDS)
@pytest.mark.parametrize("c", G.GEOMETRY, ids=lambda c: c["id"])
def test_modulated_forward(c, dtype, with_bias):
    from s2anet_amd.dcn import modulated_deform_conv_cuda_forward
    v = values(c, dtype, modulated=True)
    if not with_bias:
        v.pop("bias")
    assert (v["mask"] == 0).any() and (v["mask"] == 1).any()
    ref = G.reference(c, v, dtype, backward=False)
    out = torch.full(ref["out"].shape, float("nan"), dtype=dtype, device=DEV)
    bias = v["bias"].to(dtype) if with_bias else torch.empty(0, dtype=dtype, device=DEV)
    modulated_deform_conv_cuda_forward(v["x"].to(dtype), v["weight"].to(dtype), bias, None, v["offset"].to(dtype),
                                       v["mask"].to(dtype), out, None, c["k"][0], c["k"][1], c["s"][0], c["s"][1],
                                       c["p"][0], c["p"][1], c["d"][0], c["d"][1], c["g"], c["dg"], with_bias)
    b = bounds_for(c, dtype, ref, v["weight"], f32_offsets=False)
    kern, t, tiny, l2 = b["out"]
    b["out"] = (kern, t + G.UNIT[dtype], tiny, l2)                 # the bias addition
    check("modulated:" + ("bias" if with_bias else "nobias"), c, dtype, {"out": out}, ref, b)


def test_modulated_refuses_channels_last():
    """the documented limit (the reference's TORCH_CHECK): contiguous NCHW input only"""
    from s2anet_amd.dcn import modulated_deform_conv_cuda_forward
    c = G.ALL["base"]
    v = values(c, F32, modulated=True)
    out = torch.empty((c["B"], c["O"], *G.out_hw(c)), device=DEV)
    with pytest.raises(RuntimeError, match="input tensor has to be contiguous"):
        modulated_deform_conv_cuda_forward(v["x"].contiguous(memory_format=torch.channels_last), v["weight"], v["bias"], None,
                                           v["offset"], v["mask"], out, None, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, True)
