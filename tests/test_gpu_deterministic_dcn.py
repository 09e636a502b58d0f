"""GPU: the fused f16 deformable-conv backward in deterministic mode (s2anet_amd.deterministic): the input gradient summed
in 64-bit fixed point (include/s2anet_hip.h, "Deterministic training mode").

Inputs, float64 reference and bounds are those of tests/test_gpu_dcn_backward_shapes.py (make_case with its wild offsets,
reference, run_fused, compare: the same tau as the default f16 path, no constant of this file's own).  Shapes: partial
tiles both ways with overlapping windows, the smallest map the kernel takes, a thin map, and 128 tiles whose windows
overlap many times.  Set S2A_DETERMINISTIC_REPORT=<path> to write every measured figure as JSON.

(1, 32, 16, 3, 3): the fused weight gradient needs channels % 64 == 0 and out_channels % 32 == 0, so this shape has an
input and an offset gradient only (deform_conv_backward_input_cuda, the same kernel through the input entry)."""
import ctypes
import json
import math
import os

import pytest
import torch

from test_gpu_dcn_backward_shapes import HALO, TILE, compare, make_case, reference, run_fused, walk
from workspace_guard import GuardedWorkspaces

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16 = torch.float16
SHAPES = {"partial_9x21": (2, 64, 64, 9, 21), "smallest_3x3": (1, 32, 16, 3, 3), "thin_4x40": (1, 64, 64, 4, 40),
          "tiles128_64x64": (2, 64, 64, 64, 64)}          # (B, C, O, H, W)
REPORT = []
_CASES = {}


def record(**row):
    REPORT.append(row)
    path = os.environ.get("S2A_DETERMINISTIC_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)


def case(name):
    """inputs and the float64 reference of a shape: made once, shared, never modified"""
    if name not in _CASES:
        B, C, O, H, W = SHAPES[name]
        x, off, w, go, wild0, _ = make_case(900 + len(_CASES), B, C, O, H, W, 8, F16)
        _CASES[name] = (x, off, w, go, reference(x, off, w, go))
    return _CASES[name]


def has_weight_grad(name):
    _, C, O, _, _ = SHAPES[name]
    return C % 64 == 0 and O % 32 == 0


def run(name, x, off, w, go):
    """the gradients of one call in the CURRENT mode: (input, offset, weight) through s2a_deform_conv_backward_typed, or
    (input, offset) through the input entry where the shape has no fused weight gradient"""
    if has_weight_grad(name):
        return run_fused(x, off, w, go, "f16")
    from s2anet_amd.dcn import deform_conv_backward_input_cuda
    gin, goff = torch.zeros_like(x), torch.zeros_like(off, dtype=F16)
    deform_conv_backward_input_cuda(x, off.to(F16), go, gin, goff, w, None, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, x.shape[0])
    return gin, goff


def accumulating(x, off, w, go, init):
    """s2a_deform_conv_backward with an f32 grad_input that already holds `init`: -> (grad_input f32, grad_offset, grad_weight f32)"""
    from s2anet_amd import _lib
    L = _lib.lib()
    B, C, H, W = x.shape
    O = w.shape[0]
    gin, goff = init.clone(), torch.empty((B, 18, H, W), dtype=F16, device=DEV)
    gw = torch.zeros((O, C, 3, 3), dtype=torch.float32, device=DEV)
    ws = torch.empty((L.s2a_deform_conv_backward_workspace_bytes(_lib.DTYPE_F16, B, C, H, W, O),), dtype=torch.uint8, device=DEV)
    _lib.check(L.s2a_deform_conv_backward(_lib.DTYPE_F16, _lib.ptr(x), _lib.ptr(off.to(F16).contiguous()), _lib.ptr(go), _lib.ptr(w),
                                          _lib.ptr(gin), _lib.ptr(goff), _lib.ptr(gw), 1.0, B, C, H, W, O, _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr(torch.device(DEV))))
    return gin, goff, gw


def equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.dtype == F16 else torch.int32),
                                                                     b.view(torch.int16 if b.dtype == F16 else torch.int32))


# ----------------------------------------------------------------------------- 1. accuracy
@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_within_the_default_path_bound(name):
    import s2anet_amd as S
    B, C, O, H, W = SHAPES[name]
    x, off, w, go, ref = case(name)
    with S.deterministic(True):
        got = run(name, x, off, w, go)
    res = compare(got, ref, F16, "f16", C, O, walk(F16, B, C, H, W) if has_weight_grad(name) else (1, 1))
    record(test="accuracy", shape=name, **{k: {m: v[m] for m in ("ratio", "tau", "glob", "l2", "ok")} for k, v in res.items()})
    for g, m in res.items():
        print(name, g, m)
        assert m["ok"], (name, g, m)


# ----------------------------------------------------------------------------- 2. two calls
@pytest.mark.parametrize("name", list(SHAPES))
def test_two_calls_are_bit_equal(name):
    import s2anet_amd as S
    x, off, w, go, _ = case(name)
    with S.deterministic(True):
        a, b = run(name, x, off, w, go), run(name, x, off, w, go)
        for i, (p, q) in enumerate(zip(a, b)):
            assert equal_bits(p, q), (name, "typed", i)
        if has_weight_grad(name):
            init = torch.randn(x.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
            a, b = accumulating(x, off, w, go, init), accumulating(x, off, w, go, init)
            for i, (p, q) in enumerate(zip(a, b)):
                assert equal_bits(p, q), (name, "accumulating", i)
            # and it accumulates: init + gradient, one rounding of the exact sum
            plain = accumulating(x, off, w, go, torch.zeros_like(init))[0]
            assert ((a[0].double() - (init.double() + plain.double())).abs() <= 2.0 ** -23 * (init.abs() + plain.abs()).double()).all()


# ----------------------------------------------------------------------------- 3. order independence
@pytest.mark.parametrize("name", ["partial_9x21", "tiles128_64x64"])
def test_batch_order_does_not_change_an_image_gradient(name):
    """[a, b] and [b, a]: the workgroups of an image run at other times next to other neighbours, every sum must keep its bits"""
    import s2anet_amd as S
    x, off, w, go, _ = case(name)
    flip = lambda t: t.flip(0).contiguous()                                          # noqa: E731
    with S.deterministic(True):
        fwd = run(name, x, off, w, go)
        rev = run(name, flip(x), flip(off), w, flip(go))
    assert equal_bits(fwd[0], flip(rev[0])), "grad_input"
    assert equal_bits(fwd[1], flip(rev[1])), "grad_offset"


# ----------------------------------------------------------------------------- 4. control (recorded, not asserted)
def test_control_default_mode_repeat_is_recorded():
    import s2anet_amd as S
    x, off, w, go, _ = case("tiles128_64x64")
    assert S.deterministic() is False
    a, b = run_fused(x, off, w, go, "f16"), run_fused(x, off, w, go, "f16")
    differs = int((a[0].view(torch.int16) != b[0].view(torch.int16)).sum())
    record(test="control_default_mode_two_runs", shape="tiles128_64x64", grad_input_entries_that_differ=differs,
           grad_input_entries=a[0].numel())
    print("default mode, two runs at 64 x 64: %d of %d grad_input entries differ" % (differs, a[0].numel()))
    assert equal_bits(a[1], b[1]) and equal_bits(a[2], b[2])                         # (what the default mode does promise)


# ----------------------------------------------------------------------------- 5. non-finite values and the range
def planted_case():
    """partial_9x21 with the samples of ONE position of the last image set by hand: all four corners of every tap inside the
    image with non-zero weights (the float64 reference multiplies a zero weight with the planted value, the kernels skip
    it), taps 6-8 ten columns to the left, outside the position's 12 x 24 window: the stray path"""
    B, C, O, H, W = SHAPES["partial_9x21"]
    x, off, w, go, _ = case("partial_9x21")
    b, y, xq, o0 = B - 1, 1, 18, 7
    off = off.clone()
    off[b, 0::2, y, xq] = 0.25
    off[b, 1::2, y, xq] = torch.tensor([-0.5] * 6 + [-10.5] * 3, device=DEV)
    th, tw = TILE[F16]
    ox = xq // tw * tw - 3                                                           # window origin (k_dcn_bwd_input: ox = tx0 - 3)
    assert xq - 1 + 2 - 10.5 < ox - 1 and HALO == 4
    return x, off, w, go.clone(), (b, o0, y, xq)


def classes(t):
    return torch.isnan(t).to(torch.int8) * 4 + torch.isposinf(t).to(torch.int8) + torch.isneginf(t).to(torch.int8) * 2


@pytest.mark.parametrize("value", [math.inf, -math.inf, math.nan], ids=["+inf", "-inf", "nan"])
def test_a_planted_non_finite_value_reaches_its_cells_and_no_other(value):
    import s2anet_amd as S
    x, off, w, go, at = planted_case()
    with S.deterministic(True):
        base = run_fused(x, off, w, go, "f16")[0]
        go[at] = value
        got = run_fused(x, off, w, go, "f16")[0]
    ref = reference(x, off, w, go)["grad_input"]
    hit = ~torch.isfinite(ref)
    assert 64 * 16 <= int(hit.sum()) < ref.numel() // 4                              # every channel of 16+ cells, a small part of the tensor
    assert torch.isfinite(base).all()
    assert torch.equal(classes(got)[hit], classes(ref)[hit]), "class of the affected entries"
    assert torch.equal(got.view(torch.int16)[~hit], base.view(torch.int16)[~hit]), "an entry no planted value reached moved"
    record(test="planted", value=str(value), affected=int(hit.sum()), nan=int(torch.isnan(got).sum()),
           posinf=int(torch.isposinf(got).sum()), neginf=int(torch.isneginf(got).sum()))


def test_a_finite_contribution_beyond_the_range_counts_as_infinite():
    """filter row o0 = 1024 everywhere, grad_output of o0 zero but for 32768 at one position whose samples sit at (.5, .5):
    every contribution of that position is 0.25 * 2^25 = 2^23 >= 2^20, the documented class is +inf (-inf for -32768) in
    the 4 x 4 cells its corners touch, and nothing else moves"""
    import s2anet_amd as S
    x, off, w, go, (b, o0, y, xq) = planted_case()
    off[b, :, y, xq] = 0.5
    w = w.clone()
    w[o0] = 1024.0
    go[:, o0] = 0
    for sign, want in ((1.0, torch.isposinf), (-1.0, torch.isneginf)):
        with S.deterministic(True):
            base = run_fused(x, off, w, go, "f16")[0]
            go[b, o0, y, xq] = sign * 32768.0
            got = run_fused(x, off, w, go, "f16")[0]
            go[b, o0, y, xq] = 0
        touched = torch.zeros_like(got, dtype=torch.bool)
        touched[b, :, y - 1:y + 3, xq - 1:xq + 3] = True
        assert torch.isfinite(base).all()
        assert want(got[touched]).all(), sign
        assert torch.equal(got.view(torch.int16)[~touched], base.view(torch.int16)[~touched]), sign


# ----------------------------------------------------------------------------- 6. workspace contract of the mode
@pytest.mark.parametrize("entry", ["s2a_deform_conv_backward_typed", "s2a_deform_conv_backward_input_f16"])
def test_workspace_contract_in_the_mode(entry):
    import s2anet_amd as S
    from s2anet_amd import _lib
    L = _lib.lib()
    B, C, O, H, W = SHAPES["partial_9x21"]
    x, off, w, go, _ = case("partial_9x21")
    off16 = off.to(F16).contiguous()
    typed = entry.endswith("typed")
    pat = 12344.0

    def outputs():
        gin = torch.full((B, C, H, W), pat, dtype=F16, device=DEV) if typed else torch.zeros((B, C, H, W), device=DEV)
        return gin, torch.full((B, 18, H, W), pat, dtype=F16, device=DEV), torch.zeros((O, C, 3, 3), device=DEV)

    def call(outs, ws_ptr, ws_bytes):
        gin, goff, gw = outs
        tail = (B, C, H, W, O, ws_ptr, ws_bytes, _lib.stream_ptr(torch.device(DEV)))
        if typed:
            rc = L.s2a_deform_conv_backward_typed(_lib.DTYPE_F16, _lib.ptr(x), _lib.ptr(off16), _lib.ptr(go), _lib.ptr(w), _lib.ptr(gin),
                                                  _lib.ptr(goff), _lib.ptr(gw), 1.0, *tail)
        else:
            rc = L.s2a_deform_conv_backward_input_f16(_lib.ptr(x), _lib.ptr(off16), _lib.ptr(go), _lib.ptr(w), _lib.ptr(gin), _lib.ptr(goff), *tail)
        torch.cuda.synchronize()
        return rc

    with S.deterministic(True):
        q = (lambda: L.s2a_deform_conv_backward_workspace_bytes(_lib.DTYPE_F16, B, C, H, W, O)) if typed else \
            (lambda: L.s2a_deform_conv_backward_input_workspace_bytes(B, C, H, W, O))
        need = q()
        runs = []
        for fill in (0x00, 0xA5):
            gw_ = GuardedWorkspaces(fill)
            ws = gw_(need, torch.device(DEV), entry)
            assert ws.numel() == need
            outs = outputs()
            assert call(outs, _lib.ptr(ws), ws.numel()) == _lib.OK, L.s2a_last_error()
            gw_.check()
            runs.append(outs)
        for i, (p, r) in enumerate(zip(*runs)):
            assert equal_bits(p, r), (entry, "output %d depends on the scratch contents" % i)
        assert not (runs[0][0] == pat).any() and not (runs[0][1] == pat).any()
        gw_ = GuardedWorkspaces(0xA5)
        ws = gw_(need, torch.device(DEV), entry)
        for what, p, n in (("one byte short", _lib.ptr(ws), need - 1), ("NULL", ctypes.c_void_p(0), need)):
            outs = outputs()
            before = [t.clone() for t in outs]
            rc = call(outs, p, n)
            msg = L.s2a_last_error().decode()
            assert rc == _lib.EWORKSPACE and entry[len("s2a_"):] in msg and "workspace" in msg, (what, rc, msg)
            assert all(torch.equal(a, b) for a, b in zip(outs, before)), (what, "a refused call wrote an output")
            assert gw_.untouched(), (what, "a refused call wrote the workspace")
    # the default mode's query is smaller, and its bytes are refused in the mode
    small = q()
    assert small < need
    with S.deterministic(True):
        ws = torch.empty((small,), dtype=torch.uint8, device=DEV)
        assert call(outputs(), _lib.ptr(ws), small) == _lib.EWORKSPACE


# ----------------------------------------------------------------------------- 7. refusals
def test_routes_without_a_deterministic_form_raise_and_leave_the_buffers_alone():
    import s2anet_amd as S
    from s2anet_amd import _lib
    from s2anet_amd.dcn import deform_conv_backward_input_cuda
    L = _lib.lib()
    x, off, w, go, _ = case("partial_9x21")
    B, C, H, W = x.shape
    O = w.shape[0]
    x32, off32, w32, go32 = x.float(), off.float(), w.float(), go.float()
    args = (3, 3, 1, 1, 1, 1, 1, 1, 1, 1, B)
    with S.deterministic(True):
        # the f32 fused kernel, through the reference-shaped function: raised in front of the first launch
        gin, goff = torch.full_like(x32, 7.0), torch.full_like(off32, 7.0)
        with pytest.raises(RuntimeError, match="has no deterministic implementation"):
            deform_conv_backward_input_cuda(x32, off32, go32, gin, goff, w32, None, *args)
        torch.cuda.synchronize()
        assert (gin == 7.0).all() and (goff == 7.0).all()
        # the C entry itself
        ws = torch.full((L.s2a_deform_conv_backward_input_f32_workspace_bytes(B, C, H, W, O),), 0xA5, dtype=torch.uint8, device=DEV)
        rc = L.s2a_deform_conv_backward_input_f32(_lib.ptr(x32), _lib.ptr(off32), _lib.ptr(go32), _lib.ptr(w32), _lib.ptr(gin), _lib.ptr(goff),
                                                  B, C, H, W, O, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert rc == _lib.EINVAL and "deterministic" in L.s2a_last_error().decode()
        assert (gin == 7.0).all() and (goff == 7.0).all() and (ws == 0xA5).all()
        # the unfused route: a map under 3 x 3 (f16), and f32 through autograd (both gradients, and the input's alone)
        xs = x[:, :, :2, :5].contiguous()
        gin, goff = torch.full_like(xs, 7.0), torch.full((B, 18, 2, 5), 7.0, dtype=F16, device=DEV)
        with pytest.raises(RuntimeError, match="has no deterministic implementation"):
            deform_conv_backward_input_cuda(xs, off[:, :, :2, :5].to(F16).contiguous(), go[:, :, :2, :5].contiguous(), gin, goff, w, None, *args)
        assert (gin == 7.0).all() and (goff == 7.0).all()
        for wgrad in (True, False):
            xg, wg = x32.clone().requires_grad_(True), w32.clone().requires_grad_(wgrad)
            out = S.deform_conv(xg, off32, wg, 1, 1)
            with pytest.raises(RuntimeError, match="has no deterministic implementation"):
                out.backward(go32)
            assert xg.grad is None and wg.grad is None
        ac = S.AlignConv(C, O, 3).to(DEV)                                           # f32 AlignConv: the same refusal
        xg = x32.clone().requires_grad_(True)
        anchors = torch.rand((B, H, W, 5), device=DEV) * 20 + 4
        out = ac(xg, anchors, 8)
        with pytest.raises(RuntimeError, match="has no deterministic implementation"):
            out.backward(go32)
        assert xg.grad is None and ac.deform_conv.weight.grad is None
        # weight-only backwards are unaffected: f32 AlignConv on detached features, bit-equal to the default mode
        out = ac(x32, anchors, 8)
        out.backward(go32)
        g_on = ac.deform_conv.weight.grad.clone()
    ac.deform_conv.weight.grad = None
    ac(x32, anchors, 8).backward(go32)
    assert torch.equal(g_on, ac.deform_conv.weight.grad)
