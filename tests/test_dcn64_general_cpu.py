"""CPU: the general-geometry float64 deformable-conv reference (oracle/dcn64_general.py) is pinned here -- against the
AlignConv-geometry reference (oracle/dcn64.py), float64 F.conv2d at zero offsets, the numpy float64 forward and the
float32 C++ backward of the oracle package, and autograd's numerical gradient -- and every case of the matrix
(tests/dcn_geometry_cases.py) is shown to reject, through the comparator and the loosest bounds the GPU tests use for it,
every wrong reading of the definition its geometry can express."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_geometry_cases as G
import oracle
from oracle.dcn64 import deform_conv64, deform_conv_backward64
from oracle.dcn64_general import DEFECTS, applicable, deform_conv64_general, deform_conv_general64

F64 = torch.float64
SMALL = G.GEOMETRY + G.TILED


def test_equals_alignconv_reference_at_its_geometry():
    c = G.ALL["base"]
    v = G.as_kernel_sees(G.make_inputs(c), F64)
    for pos in (None, torch.float32):
        r = deform_conv_general64(v["x"], v["offset"], v["weight"], v["grad_out"], pos_dtype=pos, **G.geom(c))
        a = deform_conv_backward64(v["x"], v["offset"], v["weight"], v["grad_out"], pos_dtype=pos)
        out = deform_conv64(v["x"], v["offset"], v["weight"], pos_dtype=pos)
        assert torch.allclose(r["out"], out, rtol=1e-13, atol=1e-13)
        for k in ("grad_input", "grad_offset", "grad_weight", "S_input", "S_offset", "S_weight"):
            assert torch.allclose(r[k], a[k], rtol=1e-12, atol=1e-13), k
        # the same stock ops in float32 are the baseline a kernel's error is compared with, as deform_conv64's
        b32 = deform_conv64_general(v["x"], v["offset"], v["weight"], pos_dtype=pos, dtype=torch.float32, **G.geom(c))
        a32 = deform_conv64(v["x"], v["offset"], v["weight"], pos_dtype=pos, dtype=torch.float32)
        assert b32.dtype == torch.float32 and torch.allclose(b32, a32, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c["id"])
def test_equals_conv2d_at_zero_offsets(c):
    v = G.as_kernel_sees(G.make_inputs(c, modulated=True), F64)
    off = torch.zeros_like(v["offset"])
    ref = F.conv2d(v["x"], v["weight"], None, c["s"], c["p"], c["d"], c["g"])
    for mask in (None, torch.ones_like(v["mask"])):
        got = deform_conv64_general(v["x"], off, v["weight"], mask=mask, **G.geom(c))
        assert got.shape == ref.shape and torch.allclose(got, ref, rtol=1e-12, atol=1e-12)
    got = deform_conv64_general(v["x"], off, v["weight"], mask=torch.ones_like(v["mask"]), bias=v["bias"], **G.geom(c))
    assert torch.allclose(got, ref + v["bias"].view(1, -1, 1, 1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("c", G.GEOMETRY, ids=lambda c: c["id"])
def test_equals_numpy_float64_forward(c):
    v = G.as_kernel_sees(G.make_inputs(c), F64)
    ref = oracle.deform_conv_forward_f64(v["x"].numpy(), v["offset"].numpy(), v["weight"].numpy(), c["s"], c["p"], c["d"],
                                         c["g"], c["dg"])
    got = deform_conv64_general(v["x"], v["offset"], v["weight"], **G.geom(c)).numpy()
    assert np.abs(got - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("c", [c for c in G.GEOMETRY if c["g"] == 1], ids=lambda c: c["id"])
def test_gradients_within_float32_roundoff_of_cpp_oracle(c):
    v = G.make_inputs(c)
    ref = oracle.deform_conv_backward(v["x"].numpy(), v["offset"].numpy(), v["weight"].numpy(), v["grad_out"].numpy(),
                                      c["s"], c["p"], c["d"], c["dg"])
    r = G.reference(c, v, torch.float32)
    # the C++ oracle forms the same sums in float32, element by element: the roundings counted for the float32 kernels
    bounds = G.generic_bounds(c, torch.float32, r)
    # ... except the scatter weight of the input gradient: the oracle restates the reference's (ah + 1 - h), whose first
    # addition rounds at the size of the coordinate, not of the weight: an absolute error of u32 * (|ah| + 1) per factor,
    # on each of the M contributions of a cell, times the largest column gradient
    col_max = v["weight"].double().abs().sum(0).max().item() * v["grad_out"].abs().max().item()
    slack = {"input": 2 * G.U32 * (max(c["H"], c["W"]) + 1) * col_max * r["M"], "offset": 0.0, "weight": 0.0}
    for k, o in zip(("input", "offset", "weight"), ref):
        got, S = r["grad_" + k], r["S_" + k]
        err = (got - torch.from_numpy(o).to(F64)).abs()
        assert (err <= bounds["grad_" + k][0] * S + slack[k] + 1e-12).all(), (k, (err / (S + 1e-30)).max())
        assert (got.abs() <= S * (1 + 1e-12)).all() and (got[S == 0] == 0).all(), k


def test_scatter_count_and_forward_scale():
    """M is the scatter of ones; S_out bounds |out| and is the forward on absolute values"""
    c = G.ALL["g2_dg4"]
    v = G.as_kernel_sees(G.make_inputs(c, modulated=True), F64)
    r = G.reference(c, v, F64)
    n_valid = 0
    Ho, Wo = G.out_hw(c)
    (kH, kW), (sH, sW), (pH, pW), (dH, dW) = c["k"], c["s"], c["p"], c["d"]
    off = v["offset"].view(c["B"], c["dg"], kH * kW, 2, Ho, Wo)
    for b in range(c["B"]):
        for g_ in range(c["dg"]):
            for t in range(kH * kW):
                for ho in range(Ho):
                    for wo in range(Wo):
                        h = ho * sH - pH + (t // kW) * dH + off[b, g_, t, 0, ho, wo].item()
                        w = wo * sW - pW + (t % kW) * dW + off[b, g_, t, 1, ho, wo].item()
                        if not (-1 < h < c["H"] and -1 < w < c["W"]):
                            continue
                        hl, wl = int(np.floor(h)), int(np.floor(w))
                        n_valid += sum(0 <= hl + a <= c["H"] - 1 and 0 <= wl + e <= c["W"] - 1 for a in (0, 1) for e in (0, 1))
    assert r["M"].sum().item() == n_valid * (c["C"] // c["dg"])
    assert (r["out"].abs() <= r["S_out"] * (1 + 1e-12)).all()
    for k in ("input", "offset", "weight"):
        assert (r["grad_" + k].abs() <= r["S_" + k] * (1 + 1e-12)).all(), k


def test_autograd_gradcheck_grouped():
    gen = torch.Generator().manual_seed(9)
    B, C, O, H, W, g, dg = 1, 4, 4, 4, 5, 2, 2
    kw = dict(stride=(2, 1), padding=(1, 0), dilation=(1, 2), groups=g, deformable_groups=dg)
    x = torch.randn((B, C, H, W), dtype=F64, generator=gen).requires_grad_(True)
    w = torch.randn((O, C // g, 2, 2), dtype=F64, generator=gen).requires_grad_(True)
    Ho, Wo = 3, 3                      # (4 + 2 - 2) // 2 + 1, (5 - 3) // 1 + 1
    # fractional offsets (0.3 px or more from every integer: the central differences stay in one cell), some in the bands
    off = (torch.randint(-2, 3, (B, dg * 8, Ho, Wo), generator=gen).to(F64)
           + torch.tensor([0.3, 0.5, 0.7], dtype=F64)[torch.randint(0, 3, (B, dg * 8, Ho, Wo), generator=gen)]).requires_grad_(True)
    m = torch.rand((B, dg * 4, Ho, Wo), dtype=F64, generator=gen)
    assert torch.autograd.gradcheck(lambda a, b, c_: deform_conv64_general(a, b, c_, mask=m, **kw), (x, off, w),
                                    eps=1e-6, atol=1e-7)


# ----------------------------------------------------------------------------- planted defects
def loosest_bounds(c, ref, weight):
    """the loosest bound any GPU test applies to this case: the float16 generic one, and for the AlignConv-geometry
    cases also those of the fused kernels (tests/test_gpu_dcn_backward_shapes.py, tests/test_gpu_forward_shapes.py)"""
    b = G.generic_bounds(c, torch.float16, ref, weight=weight)
    if c["id"].startswith("align_"):
        from test_gpu_dcn_backward_shapes import tau as tau_bwd
        from test_gpu_forward_shapes import tau as tau_fwd
        b["out"] = (max(b["out"][0], tau_fwd("dcn16", c["C"] * 9)), b["out"][1])
        for k in ("input", "offset", "weight"):
            if "grad_" + k in b:
                t = tau_bwd(torch.float16, "f16", k, c["C"], c["O"], c["B"] * 4, 1)
                b["grad_" + k] = (max(b["grad_" + k][0], t), b["grad_" + k][1])
    return b


def rejected(c, v, ref, defect, backward):
    bad = G.reference(c, v, torch.float16, backward=backward, defect=defect, scale=False)
    bounds = loosest_bounds(c, ref, v["weight"])
    l2 = max(G.L2_BOUND[torch.float16], 4 * G.U16)             # L2_DCN of the fused f16 forward is the loosest
    return {k: not G.compare(bad[k], ref[k], ref[G.SCALE[k]], *bounds[k], l2)["ok"] for k in bounds}


@pytest.mark.parametrize("c", tuple(G.ALL.values()), ids=lambda c: c["id"])
def test_planted_defects_are_rejected(c):
    v = G.as_kernel_sees(G.make_inputs(c), torch.float16)
    ref = G.reference(c, v, torch.float16)
    same = rejected(c, v, ref, None, True)
    assert not any(same.values()), same                      # the comparator accepts the reference itself
    n = 0
    for defect in DEFECTS:
        if not applicable(defect, c["k"], c["s"], c["p"], c["d"], c["g"], c["dg"]):
            continue
        n += 1
        rej = rejected(c, v, ref, defect, True)
        if defect == "band_closed":                          # a sample on -1 weighs 0: only the offset gradient sees it
            assert rej["grad_offset"], (c["id"], defect, rej)
        else:
            assert all(rej.values()), (c["id"], defect, rej)
    assert n >= 1


@pytest.mark.parametrize("c", G.GEOMETRY, ids=lambda c: c["id"])
def test_planted_defects_are_rejected_modulated(c):
    v = G.as_kernel_sees(G.make_inputs(c, modulated=True), torch.float16)
    ref = G.reference(c, v, torch.float16, backward=False)
    assert (v["mask"] == 0).any() and (v["mask"] == 1).any()
    for defect in DEFECTS:
        if applicable(defect, c["k"], c["s"], c["p"], c["d"], c["g"], c["dg"], mask=True, backward=False):
            rej = rejected(c, v, ref, defect, False)
            assert rej["out"], (c["id"], defect)


def test_every_defect_is_expressed_somewhere():
    for defect in DEFECTS:
        assert any(applicable(defect, c["k"], c["s"], c["p"], c["d"], c["g"], c["dg"], mask=True) for c in G.GEOMETRY), defect


@pytest.mark.parametrize("c", G.TILED, ids=lambda c: c["id"])
def test_tiled_cases_leave_the_halo(c):
    for dtype in (torch.float32, torch.float16):
        assert G.beyond_halo_share(c, G.as_kernel_sees(G.make_inputs(c), dtype)["offset"]) > 0.002
