"""FusedConv2d with own_grad (s2anet_amd.train_kernels): forward, input gradient, weight gradient, bias gradient and ReLU
mask on the project's kernels, against float64.

Accuracy: the bound of tests/test_gpu_autograd_twin.py with its constants, per tensor (output or gradient, no entry excluded)
      e = |t - t64|_2 / |t64|_2,        e_prod <= FACTOR e_stock + 2 u(dtype of t),
where e_stock is the SAME module with own_grad off (the route every grad-enabled forward took before: library
convolution + stock epilogue ops), in the same dtype; for f32 masters, under torch.autocast("cuda", torch.float16).
The float64 side is oracle.conv64 for the forward and float64 autograd for the gradients.  The float64 backward takes
production's ReLU mask (out > 0) as given; separately, wherever the float64 pre-activation exceeds BAND[F16] * rms in
magnitude the mask must agree with its sign.

Shapes: the smallest at which the kernels can go wrong (CASES)."""
import pytest
import torch
import torch.nn.functional as F

from oracle.conv64 import conv64
from test_gpu_autograd_twin import BAND, DEV, F16, F32, F64, FACTOR, U, check, head_case, make_head, randn

pytestmark = pytest.mark.gpu

CASES = {  # name: (k, B, C, O, H, W, relu, residual, bias)
    # partial 4 x 16 tiles both ways, several tiles across
    "3x3_relu_res_2x64x64_9x21": (3, 2, 64, 64, 9, 21, True, True, True),
    # a single partial tile; O crosses one 256 group with a 64-wide remainder; most position slices own no tile
    "3x3_1x128x320_3x5": (3, 1, 128, 320, 3, 5, False, False, True),
    # 200 position tiles on 85 slices: more tiles than slices, not divisible by the slice count
    "3x3_4x64x64_40x72": (3, 4, 64, 64, 40, 72, False, False, True),
    # 189 positions: not a multiple of the 64-position tile (nor of the bias pass's 32 rows)
    "1x1_relu_res_3x512x128_7x9": (1, 3, 512, 128, 7, 9, True, True, True),
    "1x1_nobias_2x64x320_5x5": (1, 2, 64, 320, 5, 5, False, False, False),
}
SIDE_LIMIT = {  # a map side of 32000: outside the library's limits and outside train_shape_problem; x is 4 and 8 MB
    "1x1_1x64x64_32000x1": (1, 1, 64, 64, 32000, 1, False, False, True),
    "3x3_1x64x128_2x32000": (3, 1, 64, 128, 2, 32000, False, False, True),
}
PATTERNS = {"ALL": "xwbr", "X": "x", "PAR": "wb", "BIAS": "b", "RES": "r"}
TENSORS = {"x": "x", "w": "weight", "b": "bias", "r": "residual"}


def make(case, master, seed=11):
    from s2anet_amd.fused import FusedConv2d
    k, B, C, O, H, W, relu, res, bias = CASES.get(case) or SIDE_LIMIT[case]
    torch.manual_seed(seed)
    m = FusedConv2d(C, O, k, 1, k // 2, bias=bias, relu=relu).to(DEV, F32 if master else F16)
    if bias:
        with torch.no_grad():
            m.bias.normal_(0, 0.5)
    x = randn((B, C, H, W), F16, 1, cl=True)
    r = randn((B, O, H, W), F16, 2, cl=True) if res else None
    cot = randn((B, O, H, W), F16, 3, cl=True)
    return m, x, r, cot


def run(m, x, r, cot, pattern, own, autocast=False):
    """forward + backward with the pattern's requires_grad -> {"out", "x", "weight", "bias", "residual"} (None: no gradient)"""
    import s2anet_amd as S
    what = PATTERNS[pattern]
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
    """float64: the forward by oracle.conv64, the gradients by float64 autograd behind the GIVEN ReLU mask; also the
    float64 pre-activation"""
    k, relu = m.kernel_size[0], m.fuse_relu
    w64 = m.weight.detach().to(F64).requires_grad_(True)
    b64 = None if m.bias is None else m.bias.detach().to(F64).requires_grad_(True)
    x64 = x.detach().to(F64).requires_grad_(True)
    r64 = None if r is None else r.detach().to(F64).requires_grad_(True)
    out64, _ = conv64(x.detach(), m.weight.detach(), None if m.bias is None else m.bias.detach(), 1, k,
                      None if r is None else r.detach(), relu=relu)
    with torch.enable_grad():
        pre = F.conv2d(x64, w64, b64, 1, k // 2)
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
    assert S.train_conv_ok(x, m, r)
    verify("%s/%s" % (case, "f32" if master else "f16"), m, x, r, cot, master)


def _boom(*a, **kw):
    raise AssertionError("a route was reached that this step must not take")


@pytest.mark.parametrize("case", ["3x3_relu_res_2x64x64_9x21", "1x1_nobias_2x64x320_5x5"])
def test_route_eligible_never_reaches_the_library(case, monkeypatch):
    from s2anet_amd import fused
    m, x, r, cot = make(case, True)
    monkeypatch.setattr(fused.F, "conv2d", _boom)
    got = run(m, x, r, cot, "ALL", True)
    assert got["x"] is not None and got["weight"] is not None


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


@pytest.mark.parametrize("which", ["stride2", "narrow15", "nchw"])
def test_route_ineligible_falls_through_bit_for_bit(which, monkeypatch):
    from s2anet_amd import fused
    from s2anet_amd.fused import FusedConv2d
    torch.manual_seed(13)
    geom = {"stride2": (64, 128, 1, 2, 0), "narrow15": (64, 15, 3, 1, 1), "nchw": (64, 64, 3, 1, 1)}[which]
    m = FusedConv2d(*geom, relu=True).to(DEV, F16)
    x = randn((2, 64, 9, 11), F16, 1, cl=which != "nchw")
    ho = (9 + 2 * geom[4] - geom[2]) // geom[3] + 1
    wo = (11 + 2 * geom[4] - geom[2]) // geom[3] + 1
    cot = randn((2, geom[1], ho, wo), F16, 3, cl=which != "nchw")
    import s2anet_amd as S
    assert not S.train_conv_ok(x, m, None)
    # both runs are the library's: its weight gradient is reproducible only in deterministic mode, and only once its
    # solver choice for the shape has settled (a first call may take another solver than the calls after it)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    run(m, x, None, cot, "ALL", False)
    off = run(m, x, None, cot, "ALL", False)
    real, calls = fused.F.conv2d, []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(fused.F, "conv2d", counted)
    on = run(m, x, None, cot, "ALL", True)
    assert calls, "the library convolution was not reached"
    for name in off:
        assert (on[name] is None and off[name] is None) or torch.equal(on[name], off[name]), name


@pytest.mark.parametrize("case", ["3x3_relu_res_2x64x64_9x21", "3x3_1x128x320_3x5", "1x1_relu_res_3x512x128_7x9"])
def test_two_fresh_runs_are_bit_equal(case):
    runs = []
    for _ in range(2):
        m, x, r, cot = make(case, True)
        runs.append(run(m, x, r, cot, "ALL", True))
    for name, a in runs[0].items():
        assert (a is None and runs[1][name] is None) or torch.equal(a, runs[1][name]), name


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
def test_weights_are_followed_without_a_cache(master):
    m, x, r, cot = make("3x3_relu_res_2x64x64_9x21", master)
    verify("follow/first", m, x, r, cot, master, ("ALL",))
    with torch.no_grad():
        m.weight.mul_(-1.5)
        m.bias.add_(0.25)
    verify("follow/no_grad_inplace", m, x, r, cot, master, ("ALL",))
    m.weight.data.copy_(randn(tuple(m.weight.shape), m.weight.dtype, 7, scale=0.05))       # moves no version counter
    m.bias.data.copy_(randn(tuple(m.bias.shape), m.bias.dtype, 8, scale=0.5))
    verify("follow/data_copy", m, x, r, cot, master, ("ALL",))


def test_forward_and_backward_in_one_graph():
    """3x3 + ReLU, then 1x1 + residual + ReLU, f32 masters: forward + backward captured once, replayed after in-place
    changes of input and weights, bit-equal to eager on the same values"""
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d
    torch.manual_seed(17)
    l1 = FusedConv2d(64, 64, 3, 1, 1, relu=True).to(DEV, F32)
    l2 = FusedConv2d(64, 64, 1, relu=True).to(DEV, F32)
    net = torch.nn.ModuleList([l1, l2])
    assert S.train_kernels(net) == 2
    x = randn((2, 64, 9, 21), F16, 1, cl=True, grad=True)
    cot = randn((2, 64, 9, 21), F16, 3, cl=True)
    leaves = [x] + list(net.parameters())

    def step():
        y = l2(l1(x), x)
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


def test_head_composition_through_the_twin_harness():
    import s2anet_amd as S
    head = make_head(F16, True)
    assert S.train_kernels(head) > 0
    leaves, prod, twin = head_case(head, F16, "ALL", True)
    check("train_conv/head/f16/ALL", F16, leaves, prod, twin, module=head)
