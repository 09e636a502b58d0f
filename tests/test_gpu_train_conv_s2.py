"""The stride-2 layers on the own training route (s2anet_amd.train_kernels(model, True, strided=True), FusedConvS2Function):
forward, the parity-class input gradient, the strided weight gradient, bias gradient and ReLU mask, against float64.

Accuracy: the bound, the constants and the helpers of tests/test_gpu_autograd_twin.py; per tensor (output or gradient, no
entry excluded)   e = |t - t64|_2 / |t64|_2,   e_prod <= FACTOR e_stock + 2 u(dtype of t),
e_stock being the SAME module with both switches off (library convolution + stock epilogue ops; under torch.autocast for
f32 masters).  The float64 side is oracle.conv64 with stride = 2 for the forward and float64 autograd behind production's
ReLU mask for the gradients; outside BAND[F16] * rms the mask must agree with the sign of the float64 pre-activation (the
rule of tests/test_gpu_train_conv.py).

Shapes: the smallest at which the kernels can go wrong (CASES)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import nonfinite_cases as N
from oracle import twin64 as T
from oracle.conv64 import conv64
from test_gpu_autograd_twin import (BAND, DEV, F16, F32, F64, FACTOR, U, channels_last_filters, check, folded_trunk, named_leaves,
                                    randn, set_pattern)

pytestmark = pytest.mark.gpu

CASES = {  # name: (k, B, C, O, H, W, relu, residual, bias)
    # odd x odd: partial 4 x 16 tiles both ways in the weight gradient, partial quad tiles in the input gradient
    "3x3_relu_2x64x128_9x21": (3, 2, 64, 128, 9, 21, True, False, True),
    # even x even: the input gradient's g[i+1] and g[j+1] fall outside the map; O = 256 takes the forward's other instantiation
    "3x3_1x128x256_10x22": (3, 1, 128, 256, 10, 22, False, False, True),
    # mixed parity; a residual of the OUTPUT's shape
    "3x3_relu_res_2x64x128_10x21": (3, 2, 64, 128, 10, 21, True, True, True),
    # one group of 256 out channels and a 128 rest in the weight gradient
    "3x3_1x128x384_7x9": (3, 1, 128, 384, 7, 9, False, False, True),
    # 60 position tiles on 32 slices: more tiles than slices, not divisible by the slice count
    "3x3_4x64x128_40x72": (3, 4, 64, 128, 40, 72, False, False, True),
    # a single output: only the centre tap / only ky, kx in {1, 2} meet the image
    "3x3_1x64x128_1x1": (3, 1, 64, 128, 1, 1, False, False, True),
    "3x3_1x64x128_2x2": (3, 1, 64, 128, 2, 2, False, False, True),
    # 60 output positions: not a multiple of the 64-position tile nor of the bias pass's rows
    "1x1_relu_res_3x512x128_7x9": (1, 3, 512, 128, 7, 9, True, True, True),
    # even dims; O with a 64 rest
    "1x1_nobias_2x64x320_6x8": (1, 2, 64, 320, 6, 8, False, False, False),
}
SIDE_LIMIT = {  # a map side of 32000: outside the library's limits and outside train_shape_problem; x is 4 and 8 MB
    "1x1_1x64x64_32000x1": (1, 1, 64, 64, 32000, 1, False, False, True),
    "3x3_1x64x128_2x32000": (3, 1, 64, 128, 2, 32000, False, False, True),
}
PATTERNS = {"ALL": "xwbr", "X": "x", "PAR": "wb", "BIAS": "b", "RES": "r"}
TENSORS = {"x": "x", "w": "weight", "b": "bias", "r": "residual"}


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def make(case, master, seed=11):
    from s2anet_amd.fused import FusedConv2d
    k, B, C, O, H, W, relu, res, bias = CASES.get(case) or SIDE_LIMIT[case]
    torch.manual_seed(seed)
    m = FusedConv2d(C, O, k, 2, k // 2, bias=bias, relu=relu).to(DEV, F32 if master else F16)
    if bias:
        with torch.no_grad():
            m.bias.normal_(0, 0.5)
    Ho, Wo = out_hw(H, W)
    x = randn((B, C, H, W), F16, 1, cl=True)
    r = randn((B, O, Ho, Wo), F16, 2, cl=True) if res else None
    cot = randn((B, O, Ho, Wo), F16, 3, cl=True)
    return m, x, r, cot


def run(m, x, r, cot, pattern, own, autocast=False, strided=True):
    """forward + backward with the pattern's requires_grad -> {"out", "x", "weight", "bias", "residual"} (None: no gradient).
    own: both switches on (train_kernels(m, True, strided=True)) or both off; strided=False: train_kernels(m, own) alone"""
    import s2anet_amd as S
    what = PATTERNS[pattern]
    S.train_kernels(m, False, strided=True)
    if strided:
        S.train_kernels(m, own, strided=True)
    else:
        S.train_kernels(m, own)
    m.weight.requires_grad_("w" in what)
    if m.bias is not None:
        m.bias.requires_grad_("b" in what)
    m.zero_grad(set_to_none=True)
    x_ = x.detach().requires_grad_("x" in what)
    r_ = None if r is None else r.detach().requires_grad_("r" in what)
    with torch.enable_grad(), torch.autocast("cuda", torch.float16, enabled=autocast):
        y = m(x_, r_)
    assert y.dtype == F16 and y.shape == cot.shape
    if y.requires_grad:
        y.backward(cot)
    return {"out": y.detach(), "x": x_.grad, "weight": m.weight.grad, "bias": None if m.bias is None else m.bias.grad,
            "residual": None if r_ is None else r_.grad}


def reference(m, x, r, cot, mask):
    """float64: the forward by oracle.conv64 (stride 2), the gradients by float64 autograd behind the GIVEN ReLU mask; also
    the float64 pre-activation"""
    k, relu = m.kernel_size[0], m.fuse_relu
    w64 = m.weight.detach().to(F64).requires_grad_(True)
    b64 = None if m.bias is None else m.bias.detach().to(F64).requires_grad_(True)
    x64 = x.detach().to(F64).requires_grad_(True)
    r64 = None if r is None else r.detach().to(F64).requires_grad_(True)
    out64, _ = conv64(x.detach(), m.weight.detach(), None if m.bias is None else m.bias.detach(), stride=2, ksize=k,
                      residual=None if r is None else r.detach(), relu=relu)
    with torch.enable_grad():
        pre = F.conv2d(x64, w64, b64, 2, k // 2)
        if r64 is not None:
            pre = pre + r64
        y = pre * mask.to(F64) if relu else pre
        y.backward(cot.to(F64))
    return {"out": out64, "x": x64.grad, "weight": w64.grad, "bias": None if b64 is None else b64.grad,
            "residual": None if r64 is None else r64.grad}, pre.detach()


def rel(a, ref):
    return float((a.to(F64) - ref.to(F64)).norm() / ref.to(F64).norm())


def verify(tag, m, x, r, cot, master, patterns=tuple(PATTERNS), autocast_on=False):
    """autocast_on: the run with the switches on is under autocast too (a layer whose route then is the stock one)"""
    bad = []
    for pattern in patterns:
        what = PATTERNS[pattern]
        if not any((c == "x") or (c == "w") or (c == "b" and m.bias is not None) or (c == "r" and r is not None) for c in what):
            continue                                        # (BIAS without a bias, RES without a residual)
        prod = run(m, x, r, cot, pattern, True, autocast=autocast_on)
        stock = run(m, x, r, cot, pattern, False, autocast=master)
        mask = prod["out"] > 0
        ref, pre = reference(m, x, r, cot, mask)
        if m.fuse_relu:
            clear = pre.abs() > BAND[F16] * pre.pow(2).mean().sqrt()
            n = int((clear & (mask != (pre > 0))).sum())
            if n:
                bad.append("%s: %d ReLU entries outside the band take another branch than float64" % (pattern, n))
        for name in ["out"] + [TENSORS[c] for c in "xwbr"]:
            wanted = name == "out" or [c for c in what if TENSORS[c] == name]
            got = prod[name]
            if not wanted or ref[name] is None:
                if name != "out" and got is not None:
                    bad.append("%s: grad(%s) was not requested but is not None" % (pattern, name))
                continue
            leaf = {"out": prod["out"], "x": x, "weight": m.weight, "bias": m.bias, "residual": r}[name]
            if got is None or got.dtype != leaf.dtype or tuple(got.shape) != tuple(leaf.shape):
                bad.append("%s: %s is %s" % (pattern, name, None if got is None else (got.dtype, tuple(got.shape))))
                continue
            e_prod, e_stock = rel(got, ref[name]), rel(stock[name], ref[name])
            bound = FACTOR * e_stock + 2 * U[got.dtype]
            print("%-44s %-5s %-9s e_prod %.3e e_stock %.3e bound %.3e ratio %.3f" % (tag, pattern, name, e_prod, e_stock, bound,
                                                                                     e_prod / bound))
            if not e_prod <= bound:
                bad.append("%s: %s e_prod %.3e > %g * %.3e + 2u = %.3e" % (pattern, name, e_prod, FACTOR, e_stock, bound))
    assert not bad, tag + ":\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
@pytest.mark.parametrize("case", list(CASES))
def test_accuracy_every_pattern(case, master):
    import s2anet_amd as S
    m, x, r, cot = make(case, master)
    assert S.train_conv_strided_ok(x, m, r) and not S.train_conv_ok(x, m, r)
    verify("%s/%s" % (case, "f32" if master else "f16"), m, x, r, cot, master)


# ----------------------------------------------------------------------------- route
def _boom(*a, **kw):
    raise AssertionError("F.conv2d reached on the own training route")


@pytest.mark.parametrize("case", ["3x3_relu_res_2x64x128_10x21", "1x1_nobias_2x64x320_6x8"])
def test_route_strided_never_reaches_the_library(case, monkeypatch):
    from s2anet_amd import fused
    m, x, r, cot = make(case, True)
    monkeypatch.setattr(fused.F, "conv2d", _boom)
    got = run(m, x, r, cot, "ALL", True)
    assert got["x"] is not None and got["weight"] is not None
    assert tuple(got["x"].shape) == tuple(x.shape) and got["x"].is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("case", list(SIDE_LIMIT))
def test_behind_the_side_limit_the_stock_route_runs(case, monkeypatch):
    """a map side of 32000 is outside the library's limits: the predicate says so, and the grad-enabled step takes the stock
    route (under autocast, as every stock step of f32 masters) instead of raising from the C entry point; output and
    gradients meet the bound of the accuracy cases.  The stock route is F.conv2d whatever serves it: here torch's own GEMM
    convolution, because MIOpen builds its solvers for a 2 x 32000 map on first use, 7 to 17 s of host time for 1 ms of work"""
    import s2anet_amd as S
    from s2anet_amd import fused
    monkeypatch.setattr(torch.backends.cudnn, "enabled", False)
    m, x, r, cot = make(case, True)
    S.train_kernels(m, True, strided=True)
    assert not S.train_conv_ok(x, m, r) and not S.train_conv_strided_ok(x, m, r)
    monkeypatch.setattr(fused.FusedConvFunction, "apply", _boom)
    monkeypatch.setattr(fused.FusedConvS2Function, "apply", _boom)
    verify(case, m, x, r, cot, True, patterns=("ALL",), autocast_on=True)


@pytest.mark.parametrize("case", ["3x3_relu_res_2x64x128_10x21", "1x1_nobias_2x64x320_6x8"])
def test_route_first_switch_alone_leaves_the_library_bit_for_bit(case, monkeypatch):
    from s2anet_amd import fused
    m, x, r, cot = make(case, False)
    # (both runs are the library's: reproducible only in deterministic mode and once its solver choice has settled)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    run(m, x, r, cot, "ALL", False)
    off = run(m, x, r, cot, "ALL", False)
    real, calls = fused.F.conv2d, []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(fused.F, "conv2d", counted)
    on = run(m, x, r, cot, "ALL", True, strided=False)          # train_kernels(m) alone
    assert m.own_grad and not m.own_grad_strided and calls, "the library convolution was not reached"
    for name in off:
        assert (on[name] is None and off[name] is None) or torch.equal(on[name], off[name]), name


# ----------------------------------------------------------------------------- every byte is written (C ABI)
FRONT, BACK = 4096, 65536                   # the canaries of tests/workspace_guard.py
FILLS = (0xA5, 0xFF)                        # 0xFF..: NaN in f16 and in f32


def guarded(nbytes, fill):
    buf = torch.full((FRONT + nbytes + BACK,), fill, dtype=torch.uint8, device=DEV)
    view = buf[FRONT:FRONT + nbytes]
    assert view.data_ptr() % 256 == 0
    return buf, view


def canaries_intact(buf, nbytes, fill):
    torch.cuda.synchronize()
    return bool((buf[:FRONT] == fill).all()) and bool((buf[FRONT + nbytes:] == fill).all())


def _packed(w):
    from s2anet_amd import _lib
    O, C, k, _ = w.shape
    fwd = torch.empty((w.numel(),), dtype=F16, device=DEV)
    dg = torch.empty_like(fwd)
    _lib.check(_lib.lib().s2a_conv_pack_weight_train(_lib.ptr(w), _lib.dtype_code(w), O, C, k, _lib.ptr(fwd), _lib.ptr(dg),
                                                     _lib.stream_ptr(DEV)))
    return dg


ABI_CASES = ["3x3_1x128x256_10x22", "3x3_relu_2x64x128_9x21", "3x3_1x64x128_1x1", "1x1_relu_res_3x512x128_7x9",
             "1x1_nobias_2x64x320_6x8"]


@pytest.mark.parametrize("case", ABI_CASES)
def test_input_gradient_writes_all_of_gx_and_nothing_else(case):
    from s2anet_amd import _lib
    L = _lib.lib()
    k, B, C, O, H, W = CASES[case][:6]
    m, x, r, cot = make(case, False)
    dg = _packed(m.weight.detach().contiguous())
    g = cot.permute(0, 2, 3, 1).contiguous()
    n = B * H * W * C * 2
    got = []
    for fill in FILLS:
        buf, view = guarded(n, fill)
        _lib.check(L.s2a_conv_backward_input_s2_f16(_lib.ptr(g), _lib.ptr(dg), ctypes.c_void_p(view.data_ptr()), B, C, H, W, O, k,
                                                    _lib.stream_ptr(DEV)))
        assert canaries_intact(buf, n, fill), "bytes beside gx were written"
        got.append(view.clone().view(torch.int16).view(B, H, W, C))
    assert torch.equal(got[0], got[1]), "gx depends on what the buffer held: not every element is written"
    gx = got[0].view(F16)
    x64 = x.to(F64).requires_grad_(True)
    F.conv2d(x64, m.weight.detach().to(F64), None, 2, k // 2).backward(cot.to(F64))
    want = x64.grad.permute(0, 2, 3, 1)
    # WHAT was written: f16 products are exact in f32 and the f32 sums round far below f16's unit, so the one rounding
    # to f16 is the error: at most u per entry, hence per tensor; 2 u leaves room for the sums
    assert rel(gx, want) <= 2 * U[F16], rel(gx, want)
    if k == 1:
        odd = torch.ones((H, W), dtype=torch.bool, device=DEV)
        odd[0::2, 0::2] = False
        assert int((got[0][:, odd] != 0).sum()) == 0, "a pixel with an odd row or column is not an exact +0"


@pytest.mark.parametrize("case", ABI_CASES)
def test_weight_gradient_writes_all_of_partial_and_nothing_else(case):
    from s2anet_amd import _lib
    L = _lib.lib()
    k, B, C, O, H, W = CASES[case][:6]
    m, x, r, cot = make(case, False)
    xs = x.permute(0, 2, 3, 1).contiguous()
    g = cot.permute(0, 2, 3, 1).contiguous()
    slices = L.s2a_conv_backward_weight_s2_slices(B, C, H, W, O, k)
    assert slices > 0
    count = O * C * k * k
    n = slices * count * 4
    got, sums = [], []
    for fill in FILLS:
        buf, view = guarded(n, fill)
        for wrong in (slices + 1, slices - 1):               # refused, nothing touched
            rc = L.s2a_conv_backward_weight_s2_f16(_lib.ptr(xs), _lib.ptr(g), ctypes.c_void_p(view.data_ptr()), wrong, B, C, H, W, O,
                                                   k, _lib.stream_ptr(DEV))
            torch.cuda.synchronize()
            assert rc == _lib.EINVAL and bool((buf == fill).all())
        _lib.check(L.s2a_conv_backward_weight_s2_f16(_lib.ptr(xs), _lib.ptr(g), ctypes.c_void_p(view.data_ptr()), slices, B, C, H, W,
                                                     O, k, _lib.stream_ptr(DEV)))
        assert canaries_intact(buf, n, fill), "bytes beside partial were written"
        got.append(view.clone().view(torch.int32).view(slices, count))
        obuf, oview = guarded(count * 4, fill)
        _lib.check(L.s2a_conv_backward_weight_s2_reduce(ctypes.c_void_p(view.data_ptr()), slices, count,
                                                        ctypes.c_void_p(oview.data_ptr()), _lib.DTYPE_F32, _lib.stream_ptr(DEV)))
        assert canaries_intact(obuf, count * 4, fill)
        sums.append(oview.clone().view(F32).view(O, C, k, k))
    assert torch.equal(got[0], got[1]), "partial depends on what the buffer held: not every element is written"
    assert torch.equal(sums[0].view(torch.int32), sums[1].view(torch.int32))
    part = got[0].view(F32)
    assert bool(torch.isfinite(part).all())
    Ho, Wo = out_hw(H, W)
    tiles = B * ((Ho + 3) // 4) * ((Wo + 15) // 16) if k == 3 else (B * Ho * Wo + 63) // 64
    for s in range(min(tiles, slices), slices):              # a slice without a tile holds exact zeros
        assert int((got[0][s] != 0).sum()) == 0, s
    acc = torch.zeros((count,), dtype=F32, device=DEV)
    for s in range(slices):                                  # the reduce is the slices' sum in slice order
        acc = acc + part[s]
    assert torch.equal(acc.view(O, C, k, k), sums[0])
    w64 = m.weight.detach().to(F64).requires_grad_(True)
    F.conv2d(x.to(F64), w64, None, 2, k // 2).backward(cot.to(F64))
    # WHAT was written: f16 products are exact in f32, only the f32 sums round.  A chain of n adds of random terms is off by
    # about sqrt(n / 2) u of its result; n <= 110 positions here (7.4 u), and 64 u is eight times that
    assert rel(sums[0], w64.grad) <= 64 * U[F32], rel(sums[0], w64.grad)


# ----------------------------------------------------------------------------- reproducible
@pytest.mark.parametrize("case", ["3x3_relu_res_2x64x128_10x21", "3x3_1x128x384_7x9", "1x1_relu_res_3x512x128_7x9"])
def test_two_fresh_runs_are_bit_equal(case):
    runs = []
    for _ in range(2):
        m, x, r, cot = make(case, True)
        runs.append(run(m, x, r, cot, "ALL", True))
    for name, a in runs[0].items():
        assert (a is None and runs[1][name] is None) or torch.equal(a, runs[1][name]), name


# ----------------------------------------------------------------------------- capturable
def test_forward_and_backward_in_one_graph():
    """3x3 / s2 + ReLU, then 1x1 / s1 + residual + ReLU whose residual is a 1x1 / s2 branch of the input (a stage's first
    bottleneck in small), f32 masters: forward + backward captured once, replayed after in-place changes of input and
    weights, bit-equal to eager on the same values"""
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d
    torch.manual_seed(17)
    l1 = FusedConv2d(64, 128, 3, 2, 1, relu=True).to(DEV, F32)
    l2 = FusedConv2d(128, 128, 1, relu=True).to(DEV, F32)
    ld = FusedConv2d(64, 128, 1, 2, 0).to(DEV, F32)
    net = torch.nn.ModuleList([l1, l2, ld])
    assert S.train_kernels(net, True, strided=True) == 3
    x = randn((2, 64, 10, 21), F16, 1, cl=True, grad=True)
    cot = randn((2, 128, 5, 11), F16, 3, cl=True)
    leaves = [x] + list(net.parameters())

    def step():
        y = l2(l1(x), ld(x))
        y.backward(cot)
        return y

    def eager():
        for t in leaves:
            t.grad = None
        with torch.enable_grad():
            y = step()
        return [y.detach().clone()] + [t.grad.clone() for t in leaves]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.enable_grad():      # warm-up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    for t in leaves:
        t.grad = torch.zeros_like(t)                        # static buffers the captured backward accumulates into
    static = [t.grad for t in leaves]
    graph = torch.cuda.CUDAGraph()
    with torch.enable_grad(), torch.cuda.graph(graph):
        y_static = step()
    for round_ in range(2):
        with torch.no_grad():
            if round_:                                      # in-place changes: the replay must pack the new filters
                x.copy_(randn(tuple(x.shape), F16, 21, cl=True))
                for i, p in enumerate(net.parameters()):
                    p.mul_(1.25).add_(randn(tuple(p.shape), F32, 30 + i, scale=0.01))
            for g in static:
                g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = [y_static.clone()] + [g.clone() for g in static]
        for t, g in zip(leaves, static):
            assert t.grad is g
        want = eager()
        for t, g in zip(leaves, static):                    # (eager() replaced the buffers: put them back)
            t.grad = g
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (round_, i)


# ----------------------------------------------------------------------------- non-finite values
# name: (k, B, C, O, H, W, relu, residual, NaN in x at (b, c, y, x), inf in the cotangent at (b, oy, ox))
NONFINITE = {
    # even x even: the cotangent's inf sits on the last output row and column, whose lower / right neighbours do not exist
    "3x3_relu_2x64x128_10x22": (3, 2, 64, 128, 10, 22, True, False, (0, 10, 4, 10), (1, 4, 10)),
    "1x1_res_3x128x64_7x9": (1, 3, 128, 64, 7, 9, False, True, (1, 10, 2, 4), (2, 3, 4)),
}


def nonfinite_fixture(case):
    k, B, C, O, H, W, relu, res, (nb, nc, ny, nx), (ib, iy, ix) = NONFINITE[case]
    Ho, Wo = out_hw(H, W)
    x = N._randn((B, C, H, W), 1)
    w = N._randn((O, C, k, k), 2, 0.05).float()
    b = N._randn((O,), 3, 0.5).float()
    r = N._randn((B, O, Ho, Wo), 4) if res else None
    cot = N._randn((B, O, Ho, Wo), 5)
    pre = F.conv2d(x.to(F64), w.to(F64), b.to(F64), 2, k // 2) + (0 if r is None else r.to(F64))
    x[nb, nc, ny, nx] = N.NANV
    cot[ib, int(pre[ib, :, iy, ix].argmax()), iy, ix] = N.INF          # (the channel the ReLU passes whatever the rounding)
    assert bool(torch.isfinite(F.conv2d(x.to(F64), w.to(F64), None, 2, k // 2)[ib, :, iy, ix]).all())   # the plants do not meet
    p = dict(x=x, w=w, b=b, r=r, cot=cot)
    return {"planted": p, "sanitised": {n: N.sanitised(t) for n, t in p.items()}, "geom": (k, relu)}


def nonfinite_reference(t, k, relu, mask):
    """nonfinite_cases.conv_reference at stride 2"""
    x64, w64, b64 = (t[n].detach().to("cpu", F64).requires_grad_(True) for n in ("x", "w", "b"))
    r64 = None if t["r"] is None else t["r"].detach().to("cpu", F64).requires_grad_(True)
    with torch.enable_grad():
        pre = F.conv2d(x64, w64, b64, 2, k // 2)
        if r64 is not None:
            pre = pre + r64
        y = pre
        if relu:
            keep = torch.where(torch.isfinite(pre.detach()), mask.to("cpu"), ~(pre.detach() <= 0))
            y = torch.where(keep, pre, torch.zeros_like(pre))
        y.backward(t["cot"].detach().to("cpu", F64))
    return {"out": y.detach(), "x": x64.grad, "weight": w64.grad, "bias": b64.grad, "residual": None if r64 is None else r64.grad}


def nonfinite_module(t, geom, master):
    from s2anet_amd.fused import FusedConv2d
    k, relu = geom
    O, C = t["w"].shape[:2]
    m = FusedConv2d(C, O, k, 2, k // 2, bias=True, relu=relu).to(DEV, F32 if master else F16)
    with torch.no_grad():
        m.weight.copy_(t["w"])
        m.bias.copy_(t["b"])
    cl = dict(memory_format=torch.channels_last)
    return m, t["x"].to(DEV).contiguous(**cl), None if t["r"] is None else t["r"].to(DEV).contiguous(**cl), \
        t["cot"].to(DEV).contiguous(**cl)


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
@pytest.mark.parametrize("case", list(NONFINITE))
def test_nonfinite_values_keep_float64s_class_and_stay_local(case, master):
    assert N.FACTOR == FACTOR and N.U == U
    fx = nonfinite_fixture(case)
    k, relu = fx["geom"]
    mp, xp, rp, cp = nonfinite_module(fx["planted"], fx["geom"], master)
    ms, xs, rs, cs = nonfinite_module(fx["sanitised"], fx["geom"], master)
    prod_p = run(mp, xp, rp, cp, "ALL", True)
    prod_s = run(ms, xs, rs, cs, "ALL", True)
    stock_s = run(ms, xs, rs, cs, "ALL", False, autocast=master)
    ref_p = nonfinite_reference(fx["planted"], k, relu, prod_p["out"] > 0)
    ref_s = nonfinite_reference(fx["sanitised"], k, relu, prod_s["out"] > 0)
    bad = []
    for name in ("out", "x", "weight", "bias", "residual"):
        if ref_p[name] is None:
            assert prod_p[name] is None
            continue
        assert prod_p[name] is not None and prod_s[name] is not None, name
        if name in ("out", "x", "weight"):
            assert N.counts(ref_p[name])[0] < ref_p[name].numel(), "the plants do not reach " + name
        bad += N.contract("%s/%s/%s" % (case, "f32" if master else "f16", name), prod_p[name], prod_s[name], stock_s[name],
                          ref_p[name], ref_s[name])
    assert not bad, case + ":\n  " + "\n  ".join(bad)


# ----------------------------------------------------------------------------- composed
def _fresh_bits(build):
    """two fresh builds + runs of the same case -> their outputs and gradients, which must be bit-equal"""
    runs = []
    for _ in range(2):
        leaves, prod = build()
        for t in leaves.values():
            t.grad = None
        with torch.enable_grad():
            outs = prod()
            outs = [outs] if isinstance(outs, torch.Tensor) else list(outs)
            gen = torch.Generator(device=DEV).manual_seed(5)
            torch.autograd.backward(outs, [torch.randn(o.shape, device=DEV, generator=gen, dtype=F32).to(o.dtype) for o in outs])
        runs.append([o.detach().clone() for o in outs] + [t.grad.clone() for t in leaves.values() if t.grad is not None])
    assert len(runs[0]) == len(runs[1]) > 1
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i


def _under_no_library(monkeypatch, fn):
    """fn() with F.conv2d raising -- for production's forward only: the twins are written in stock ops"""
    from s2anet_amd import fused

    def wrapped():
        with monkeypatch.context() as mp:
            mp.setattr(fused.F, "conv2d", _boom)
            return fn()
    return wrapped


def test_bottleneck_with_a_strided_conv2_and_downsample(monkeypatch):
    """layer2[0] of the folded f16 trunk (1x1, 3x3 / s2, 1x1 + residual, 1x1 / s2 downsample) on 17 x 21, the size
    tests/test_gpu_autograd_twin.py argues for: every convolution under grad on the own kernels"""
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d

    def build():
        block = folded_trunk(F16).backbone[2][0]
        assert isinstance(block.conv3, FusedConv2d) and block.downsample is not None
        assert tuple(block.conv2.stride) == (2, 2) and tuple(block.downsample[0].stride) == (2, 2)
        assert all(isinstance(m, FusedConv2d) for m in (block.conv1, block.conv2, block.downsample[0]))
        assert S.train_kernels(block, True, strided=True) >= 4
        x = randn((2, 256, 17, 21), F16, 3, cl=True)
        set_pattern("ALL", [x], block)
        return block, x, dict(named_leaves(block), x=x)

    block, x, leaves = build()
    check("train_conv_s2/bottleneck/f16/ALL", F16, leaves, _under_no_library(monkeypatch, lambda: block(x)),
          lambda tw, dt: T.bottleneck_folded(tw(x), T.bottleneck_params(block, tw), dt), module=block)

    def fresh():
        b, xx, lv = build()
        return lv, _under_no_library(monkeypatch, lambda: b(xx))
    _fresh_bits(fresh)


def test_fpn_with_its_two_strided_extra_levels(monkeypatch):
    import s2anet_amd as S
    from s2anet_amd.detector import FPN, fuse_epilogues
    from s2anet_amd.fused import FusedConv2d

    def build():
        torch.manual_seed(31)
        neck = FPN(in_channels=(64, 128, 256), out_channels=128)
        for m in neck.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.normal_(m.bias, 0, 0.3)
        neck = channels_last_filters(fuse_epilogues(neck).to(DEV, F16))
        convs = list(neck.lateral_convs) + list(neck.fpn_convs)
        assert all(isinstance(m, FusedConv2d) for m in convs) and len(neck.fpn_convs) == 5
        assert all(tuple(m.stride) == (2, 2) for m in list(neck.fpn_convs)[3:])
        assert S.train_kernels(neck, True, strided=True) == len(convs)
        xs = [randn((2, c, h, w), F16, 4 + i, cl=True) for i, (c, h, w) in enumerate(((64, 16, 20), (128, 8, 10), (256, 4, 5)))]
        set_pattern("ALL", xs, neck)
        return neck, xs, dict(named_leaves(neck), **{"x%d" % i: x for i, x in enumerate(xs)})

    neck, xs, leaves = build()
    check("train_conv_s2/fpn/f16/ALL", F16, leaves, _under_no_library(monkeypatch, lambda: neck(xs)),
          lambda tw, dt: T.fpn([tw(x) for x in xs], T.fpn_params(neck, tw), dt), module=neck)

    def fresh():
        n, xx, lv = build()
        return lv, _under_no_library(monkeypatch, lambda: n(xx))
    _fresh_bits(fresh)
