"""Training-mode BatchNorm on the own kernels (s2anet_amd.batch_norm_train / train_batchnorm, csrc/bn_ops.hip) against float64.

Accuracy, per tensor and with no entry excluded (the bound and constants of tests/test_gpu_autograd_twin.py):
    e = |t - t64|_2 / |t64|_2 <= FACTOR * e_stock + 2 u(dtype of t)
for the output, dx, grad_gamma, grad_beta, the residual's gradient, and running_mean / running_var after the step.  e_stock is
the SAME nn.BatchNorm2d with the stock add and ReLU on the same f16 channels-last tensors; float64 starts from the same f16
values.  The ReLU mask is judged as in tests/test_gpu_train_conv.py: the float64 backward takes production's mask (out > 0),
and wherever the float64 pre-activation exceeds BAND[F16] * rms in magnitude the mask must agree with its sign.

Shapes: tests/test_batchnorm_cpu.py:SHAPES -- the issue's six, one more for "more tiles than slices" (at 64 channels the
plan has 256 slices, and 40 x 72 only 180 tiles), and 3 x 117 x 117, the one whose lanes own more than four rows (the
unrolled loop of k_bn_stats; per channel and per element that walk is held by tests/test_gpu_bn_geometry.py).

The capture test runs two blocks: layer1[0] as the trunk has it (64 -> 64 -> 256, stride 1, with downsample) and a stride-2
block with downsample at 64 -> 128 -> 512.  A 64 -> 64 -> 256 block at stride 2 is outside train_conv_strided_ok (the 3x3 / s2
forward kernel needs O % 128 == 0) and keeps the stock route, so it cannot stand for the own one."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import twin64 as T
from test_batchnorm_cpu import SHAPES
from test_gpu_autograd_twin import BAND, DEV, F16, F32, F64, FACTOR, U, channels_last_filters, check, named_leaves, randn, set_pattern

pytestmark = pytest.mark.gpu

VARIANTS = {"relu_res": (True, True), "relu": (True, False), "plain": (False, False)}     # name: (relu, residual)
PATTERNS = {"ALL": "xwbr", "X": "x", "PAR": "wb", "RES": "r"}
CL = torch.channels_last


def make_x(name, seed=1):
    B, C, H, W = SHAPES[name]
    x = randn((B, C, H, W), F32, seed)
    if name == "offset":
        x = 8.0 + x / 16.0                                   # channel means 8, std 1/16: E[x^2] - mean^2 cancels in f32
    elif name == "constant_channel":
        x[:, 5] = 0.75                                       # var = 0, invstd = eps^-1/2
    else:
        x = x * 0.8 + randn((1, C, 1, 1), F32, seed + 50)    # a mean of the order of the spread
    return x.to(F16).contiguous(memory_format=CL)


def make(name, master, seed=11):
    B, C, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.5)
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    bn = bn.to(DEV).train()
    if not master:
        bn = bn.half()
    x = make_x(name)
    r = randn((B, C, H, W), F16, 2, cl=True)
    cot = randn((B, C, H, W), F16, 3, cl=True)
    return bn, x, r, cot


def run(bn0, x, r, cot, relu, pattern, own):
    """one training step of a COPY of bn0 -> {"out", "x", "weight", "bias", "residual", "running_mean", "running_var", "nbt"}"""
    import s2anet_amd as S
    what = PATTERNS[pattern]
    bn = copy.deepcopy(bn0)
    bn.weight.requires_grad_("w" in what)
    bn.bias.requires_grad_("b" in what)
    x_ = x.detach().clone(memory_format=torch.preserve_format).requires_grad_("x" in what)
    r_ = None if r is None else r.detach().clone(memory_format=torch.preserve_format).requires_grad_("r" in what)
    with torch.enable_grad():
        if own:
            assert S.train_bn_ok(x_, bn, r_)
            y = S.batch_norm_train(x_, bn, r_, relu)
        else:
            y = bn(x_)
            if r_ is not None:
                y = y + r_
            y = F.relu(y) if relu else y
    assert y.dtype == F16 and y.shape == cot.shape and y.is_contiguous(memory_format=CL)
    if y.requires_grad:
        y.backward(cot)
    return {"out": y.detach(), "x": x_.grad, "weight": bn.weight.grad, "bias": bn.bias.grad, "residual": None if r_ is None else r_.grad,
            "running_mean": bn.running_mean.detach(), "running_var": bn.running_var.detach(), "nbt": int(bn.num_batches_tracked)}


def reference(bn, x, r, cot, relu, mask):
    """float64 from the same f16 / parameter values: forward, gradients behind the GIVEN ReLU mask, running statistics"""
    x64 = x.detach().to(F64).requires_grad_(True)
    w64, b64 = bn.weight.detach().to(F64).requires_grad_(True), bn.bias.detach().to(F64).requires_grad_(True)
    r64 = None if r is None else r.detach().to(F64).requires_grad_(True)
    with torch.enable_grad():
        pre = F.batch_norm(x64, None, None, w64, b64, True, 0.0, bn.eps)
        if r64 is not None:
            pre = pre + r64
        y = pre * mask.to(F64) if relu else pre
        y.backward(cot.to(F64))
    P = x.numel() // x.shape[1]
    xd = x.detach().to(F64)
    mean, var = xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)
    m = bn.momentum
    return {"out": F.relu(pre.detach()) if relu else pre.detach(), "x": x64.grad, "weight": w64.grad, "bias": b64.grad,
            "residual": None if r64 is None else r64.grad,
            "running_mean": (1 - m) * bn.running_mean.detach().to(F64) + m * mean,
            "running_var": (1 - m) * bn.running_var.detach().to(F64) + m * var * P / (P - 1)}, pre.detach()


def rel(a, ref):
    return float((a.to(F64) - ref.to(F64)).norm() / ref.to(F64).norm())


GRADS = {"x": "x", "w": "weight", "b": "bias", "r": "residual"}


def verify(tag, bn, x, r, cot, relu):
    bad = []
    for pattern, what in PATTERNS.items():
        if what == "r" and r is None:
            continue
        prod = run(bn, x, r, cot, relu, pattern, True)
        stock = run(bn, x, r, cot, relu, pattern, False)
        mask = prod["out"] > 0
        ref, pre = reference(bn, x, r, cot, relu, mask)
        if relu:
            clear = pre.abs() > BAND[F16] * pre.pow(2).mean().sqrt()
            n = int((clear & (mask != (pre > 0))).sum())
            if n:
                bad.append("%s: %d ReLU entries outside the band take another branch than float64" % (pattern, n))
        if prod["nbt"] != 1 or stock["nbt"] != 1:
            bad.append("%s: num_batches_tracked %d (stock %d)" % (pattern, prod["nbt"], stock["nbt"]))
        leaf = {"out": prod["out"], "x": x, "weight": bn.weight, "bias": bn.bias, "residual": r, "running_mean": bn.running_mean,
                "running_var": bn.running_var}
        for name in ("out", "x", "weight", "bias", "residual", "running_mean", "running_var"):
            wanted = name in ("out", "running_mean", "running_var") or any(GRADS[c] == name for c in what)
            got = prod[name]
            if not wanted or ref[name] is None:
                if got is not None:
                    bad.append("%s: grad(%s) was not requested but is not None" % (pattern, name))
                continue
            if got is None or got.dtype != leaf[name].dtype or tuple(got.shape) != tuple(leaf[name].shape):
                bad.append("%s: %s is %s" % (pattern, name, None if got is None else (got.dtype, tuple(got.shape))))
                continue
            if not bool(torch.isfinite(got).all()):
                bad.append("%s: %s is not finite" % (pattern, name))
                continue
            e_prod, e_stock = rel(got, ref[name]), rel(stock[name], ref[name])
            bound = FACTOR * e_stock + 2 * U[got.dtype]
            print("%-40s %-4s %-12s e_prod %.3e e_stock %.3e bound %.3e ratio %.3f" % (tag, pattern, name, e_prod, e_stock, bound,
                                                                                    e_prod / bound))
            if not e_prod <= bound:
                bad.append("%s: %s e_prod %.3e > %g * %.3e + 2u = %.3e" % (pattern, name, e_prod, FACTOR, e_stock, bound))
    assert not bad, tag + ":\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("master", [True, False], ids=["f32_masters", "f16_params"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_accuracy_every_pattern(name, variant, master):
    relu, res = VARIANTS[variant]
    bn, x, r, cot = make(name, master)
    assert bn.weight.dtype == (F32 if master else F16) and bn.running_var.dtype == bn.weight.dtype
    verify("%s/%s/%s" % (name, variant, "f32" if master else "f16"), bn, x, r if res else None, cot, relu)


def test_f16_parameters_with_f32_statistics():
    bn, x, r, cot = make("ragged", False)
    bn.running_mean, bn.running_var = bn.running_mean.float(), bn.running_var.float()
    verify("ragged/relu_res/f16_params_f32_stats", bn, x, r, cot, True)


def test_constant_channel_has_the_epsilon_invstd_and_finite_gradients():
    bn, x, r, cot = make("constant_channel", True)
    got = run(bn, x, r, cot, True, "ALL", True)
    def f32(v):
        return float(torch.tensor(v, dtype=F32))
    m = bn.momentum                                          # (the update is formed in double and rounded once)
    assert float(got["running_var"][5]) == f32((1.0 - m) * float(bn.running_var[5]) + m * 0.0)
    assert float(got["running_mean"][5]) == f32((1.0 - m) * float(bn.running_mean[5]) + m * 0.75)
    assert bool(torch.isfinite(got["x"]).all()) and float(got["weight"][5]) == 0.0       # xhat is exactly 0 on that channel
    pre = bn.bias[5].detach() + r[:, 5].float()              # (x - mean) = 0: beta + residual in f32, one rounding
    assert torch.equal(got["out"][:, 5], F.relu(pre).to(F16))


def test_one_value_per_channel_raises_torchs_value_error():
    import s2anet_amd as S
    bn = nn.BatchNorm2d(64).to(DEV).train()
    x = torch.zeros((1, 64, 1, 1), dtype=F16, device=DEV).contiguous(memory_format=CL)
    assert not S.train_bn_ok(x, bn)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        S.batch_norm_train(x, bn)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        S.BatchNormTrainFunction.apply(x, bn.weight, bn.bias, None, bn.running_mean, bn.running_var, bn.num_batches_tracked, 1e-5, 0.1, False)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        bn(x)                                                # torch's own
    assert int(bn.num_batches_tracked) <= 1 and torch.equal(bn.running_mean, torch.zeros_like(bn.running_mean))
    with pytest.raises(RuntimeError, match="train_bn_ok"):
        S.batch_norm_train(x.float().expand(2, 64, 1, 1).contiguous(memory_format=CL), bn)     # outside the limits: no fall-back


# ----------------------------------------------------------------------------- blocks
def make_block(kind, master=True, seed=5):
    """an unfolded bottleneck in training mode, channels-last filters, randomised norms; kind: "layer1_0" (64 -> 64 -> 256,
    stride 1, downsample), "s2_down" (64 -> 128 -> 512, stride 2, downsample), "plain" (256 -> 64 -> 256, no downsample)"""
    from s2anet_amd.detector import BottleNeck
    inp, planes, stride = {"layer1_0": (64, 64, 1), "s2_down": (64, 128, 2), "plain": (256, 64, 1)}[kind]
    torch.manual_seed(seed)
    down = None
    if kind != "plain":
        down = nn.Sequential(nn.Conv2d(inp, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
    blk = BottleNeck(inp, planes, stride, down)
    g = torch.Generator().manual_seed(seed + 1)
    for m in blk.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
    blk.bn3.weight.data.mul_(0.25)
    blk = channels_last_filters(blk.to(DEV, F32 if master else F16)).train()
    return blk, inp


def _boom(*a, **kw):
    raise AssertionError("a library convolution / batch norm was reached on the own route")


@pytest.mark.parametrize("kind", ["layer1_0", "s2_down", "plain"])
def test_own_route_never_reaches_the_library(kind, monkeypatch):
    import s2anet_amd as S
    blk, inp = make_block(kind)
    assert S.train_batchnorm(blk) == (4 if kind != "plain" else 3)
    x = randn((2, inp, 12, 20), F16, 3, cl=True, grad=True)
    assert blk._own_norm_ok(x)
    monkeypatch.setattr(F, "batch_norm", _boom)
    monkeypatch.setattr(F, "conv2d", _boom)
    monkeypatch.setattr(torch, "batch_norm", _boom)
    monkeypatch.setattr(torch, "conv2d", _boom)
    with torch.enable_grad():
        y = blk(x)
        y.backward(torch.ones_like(y))
    assert x.grad is not None and all(p.grad is not None for p in blk.parameters())
    assert all(int(m.num_batches_tracked) == 1 for m in blk.modules() if isinstance(m, nn.BatchNorm2d))
    with pytest.raises(AssertionError, match="was reached"):
        blk(x.float())                                       # the control: an f32 input is outside and takes the stock route


@pytest.mark.parametrize("kind", ["layer1_0", "s2_down"])
def test_own_norm_ok_creates_no_tensor(kind):
    """the block's question is answered on shapes and parameters: not one byte is allocated, not even for a moment"""
    import s2anet_amd as S
    blk, inp = make_block(kind)
    S.train_batchnorm(blk)
    x = randn((2, inp, 24, 24), F16, 3, cl=True, grad=True)
    blk.__dict__.pop("_own_norm_cache", None)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.enable_grad():
        ok = blk._own_norm_ok(x)
    assert ok is True
    assert torch.cuda.memory_allocated() == before and torch.cuda.max_memory_allocated() == before


def _step(blk, x, cot):
    for p in blk.parameters():
        p.grad = None
    x.grad = None
    with torch.enable_grad():
        y = blk(x)
    y.backward(cot)
    return y


def _state(blk, x, y):
    out = [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in blk.parameters()]
    return out + [b.detach().clone() for b in blk.buffers()]


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_two_fresh_runs_are_bit_equal(det):
    import s2anet_amd as S
    runs = []
    with S.deterministic(det):
        for _ in range(2):
            blk, inp = make_block("s2_down")
            S.train_batchnorm(blk)
            x = randn((2, inp, 12, 20), F16, 3, cl=True, grad=True)
            y = _step(blk, x, randn((2, 512, 6, 10), F16, 4, cl=True))
            runs.append(_state(blk, x, y))
    assert len(runs[0]) == len(runs[1]) > 10
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b) or (torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())), i
    for name in SHAPES:                                      # and the op alone, every shape
        bn, x, r, cot = make(name, True)
        a, b = run(bn, x, r, cot, True, "ALL", True), run(bn, x, r, cot, True, "ALL", True)
        assert all(torch.equal(a[k], b[k]) for k in a if k != "nbt"), name


@pytest.mark.parametrize("kind", ["layer1_0", "s2_down"])
def test_captured_step_replays_bit_equal_to_eager(kind):
    """forward + backward of the unfolded block captured in a CUDAGraph, replayed three times on changed inputs: every replay
    equals the eager step on a twin block bit for bit, running statistics and num_batches_tracked after k steps included"""
    import s2anet_amd as S
    blk, inp = make_block(kind)
    eager = copy.deepcopy(blk)
    S.train_batchnorm(blk)
    S.train_batchnorm(eager)
    shape = (2, inp, 12, 20)
    xs = [randn(shape, F16, 30 + i, cl=True) for i in range(4)]
    x = xs[0].clone(memory_format=torch.preserve_format).requires_grad_(True)
    stride = 2 if kind == "s2_down" else 1
    cot = randn((2, blk.conv3.out_channels, 12 // stride, 20 // stride), F16, 4, cl=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up: allocator, lazy inits, the route's cached decision
        _step(blk, x, cot)
    torch.cuda.current_stream().wait_stream(side)
    _step(eager, xs[0].clone(memory_format=torch.preserve_format).requires_grad_(True), cot)
    graph = torch.cuda.CUDAGraph()
    for p in blk.parameters():
        p.grad = None
    x.grad = None
    with torch.cuda.graph(graph):
        with torch.enable_grad():
            y = blk(x)
        y.backward(cot)
    for k in range(1, 4):
        with torch.no_grad():
            x.copy_(xs[k])
        graph.replay()
        xe = xs[k].clone(memory_format=torch.preserve_format).requires_grad_(True)
        ye = _step(eager, xe, cot)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(_state(blk, x, y), _state(eager, xe, ye))):
            assert torch.equal(a, b), (k, i)
        assert all(int(m.num_batches_tracked) == k + 1 for m in blk.modules() if isinstance(m, nn.BatchNorm2d))


def test_eval_and_no_grad_forwards_are_bit_equal_to_the_flag_off(monkeypatch):
    import s2anet_amd as S
    # (both sides are the library's: reproducible only in deterministic mode and once its solver choice has settled, as in
    # tests/test_gpu_train_conv_s2.py)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    for kind in ("layer1_0", "s2_down"):
        blk, inp = make_block(kind, master=False)
        twin = copy.deepcopy(blk)
        S.train_batchnorm(blk)
        x = randn((2, inp, 12, 20), F16, 3, cl=True)
        with torch.no_grad():
            settle = copy.deepcopy(twin)
            settle(x), settle.eval()(x)
        with torch.no_grad():                                # training-mode norms, no grad: the stock route, statistics move
            assert not blk._own_norm_ok(x) and torch.equal(blk(x), twin(x))
        assert torch.equal(blk.bn2.running_var, twin.bn2.running_var)
        blk.eval(), twin.eval()
        xg = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        with torch.enable_grad():                            # eval-mode norms under grad: the stock route again
            assert not blk._own_norm_ok(xg) and torch.equal(blk(xg), twin(x))
        blk.train()
        with torch.enable_grad():
            assert blk._own_norm_ok(xg)


# ----------------------------------------------------------------------------- the trunk, through the twin harness
def _bn_twin(y, bn, tw, dt):
    return F.batch_norm(y, None, None, tw(bn.weight).to(dt), tw(bn.bias).to(dt), True, 0.0, bn.eps)


def bottleneck_twin(x, blk, tw, dt):
    """the unfolded BottleNeck in training mode in stock ops (detector.BottleNeck._forward_plain), every step in dt"""
    def conv(c, t):
        return F.conv2d(t, tw(c.weight).to(dt), None, c.stride, c.padding)
    out = T._relu(_bn_twin(conv(blk.conv1, x), blk.bn1, tw, dt))
    out = T._relu(_bn_twin(conv(blk.conv2, out), blk.bn2, tw, dt))
    out = _bn_twin(conv(blk.conv3, out), blk.bn3, tw, dt)
    res = x if blk.downsample is None else _bn_twin(conv(blk.downsample[0], x), blk.downsample[1], tw, dt)
    return T._relu(out + res)


class NormRecorder:
    """stands in for the harness' Recorder on the own route, which calls no nn.ReLU module: notes out > 0 of every
    batch_norm_train(..., relu=True) in call order -- bn1, bn2, bn3 of each block, the order of bottleneck_twin's ReLUs"""

    def __init__(self, module):
        from s2anet_amd import norm
        self.taken, self.norm, self.real = [], norm, norm.batch_norm_train

        def recording(x, bn, residual=None, relu=False):
            out = self.real(x, bn, residual, relu)
            if relu:
                self.taken.append(out.detach() > 0)
            return out
        norm.batch_norm_train = recording

    def remove(self):
        self.norm.batch_norm_train = self.real


def test_unfolded_trunk_layer1_and_layer2_0_against_the_float64_twin(monkeypatch):
    """layer1 + layer2[0] of build_synthetic_detector(fold_bn=False) in training mode, f32 masters, batch 2 at 96 x 96 (a
    24 x 24 pooled stem output), through the twin harness under its bound"""
    import s2anet_amd as S
    import test_gpu_autograd_twin as H
    from s2anet_amd.detector import DetectorBackbone, build_synthetic_detector
    model = build_synthetic_detector(dtype=F32, device=DEV, fold_bn=False)
    bb = model.backbone.backbone
    blocks = list(bb[1][1]) + [bb[2][0]]
    mod = nn.Sequential(*blocks).train()
    assert len(blocks) == 4 and S.train_batchnorm(mod) == 3 * 4 + 2
    x = randn((2, 64, 24, 24), F16, 3, cl=True)
    set_pattern("ALL", [x], mod)
    leaves = dict(named_leaves(mod), x=x)
    assert all(b._own_norm_ok(x if i == 0 else randn((2, 256, 24, 24), F16, 9, cl=True)) for i, b in enumerate(blocks))
    monkeypatch.setattr(H, "Recorder", NormRecorder)

    def prod():
        with monkeypatch.context() as mp:
            mp.setattr(F, "conv2d", _boom)
            mp.setattr(F, "batch_norm", _boom)
            return DetectorBackbone.run_blocks(mod, x)

    def twin(tw, dt):
        y = tw(x).to(dt)
        for b in blocks:
            y = bottleneck_twin(y, b, tw, dt)
        return y
    check("train_bn/trunk/layer1+layer2.0/f32_masters/ALL", F16, leaves, prod, twin, module=mod)


def test_trunk_entry_casts_the_pooled_stem_output_once(monkeypatch):
    """with the flag on, a grad-enabled training forward of the f32 trunk hands layer 1 an f16 channels-last tensor and every
    block takes the own route; with it off, or in eval mode, nothing is cast"""
    import s2anet_amd as S
    from s2anet_amd.detector import BottleNeck, DetectorBackbone
    torch.manual_seed(3)
    bb = DetectorBackbone(layers=(1, 1, 1, 1))
    for m in bb.modules():
        if isinstance(m, BottleNeck):
            m.bn3.weight.data.fill_(0.25)
    bb = channels_last_filters(bb.to(DEV, F32)).train()
    imgs = torch.rand((2, 3, 96, 96), device=DEV).contiguous(memory_format=CL)
    seen, real = [], BottleNeck._forward_plain

    def noting(self, x):                                     # (run_blocks calls forward_chain, not the module: no hook sees it)
        seen.append((x.dtype, self._own_norm_ok(x)))
        return real(self, x)
    monkeypatch.setattr(BottleNeck, "_forward_plain", noting)
    with torch.enable_grad():
        outs = bb(imgs)
    assert all(o.dtype == F32 for o in outs) and seen == [(F32, False)] * 4
    del seen[:]
    assert S.train_batchnorm(bb) == 1 + 4 * 4
    with torch.enable_grad():
        outs = bb(imgs)
        sum(o.float().sum() for o in outs).backward()
    assert all(o.dtype == F16 and o.is_contiguous(memory_format=CL) for o in outs) and seen == [(F16, True)] * 4
    assert all(p.grad is not None and p.grad.dtype == F32 for p in bb.parameters())
    del seen[:]
    bb.eval()
    with torch.enable_grad():
        outs = bb(imgs)
    assert all(o.dtype == F32 for o in outs) and seen == [(F32, False)] * 4


# ----------------------------------------------------------------------------- fold_batchnorm after one step
def test_fold_batchnorm_after_one_own_step_against_the_stock_stepped_twin():
    """one SGD step of a (1, 1, 1, 1) trunk from the pooled stem output on: own route, stock route, and float64; then
    fold_batchnorm of all three.  Every folded filter and bias of the own-stepped model is within the bound of float64's,
    e_stock being the stock-stepped model's distance"""
    import s2anet_amd as S
    from s2anet_amd.detector import BottleNeck, DetectorBackbone, fold_batchnorm
    from s2anet_amd.fused import FusedConv2d

    def build():
        torch.manual_seed(21)
        net = nn.Module()
        net.backbone = DetectorBackbone(layers=(1, 1, 1, 1))
        g = torch.Generator().manual_seed(22)
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.data = torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5
                m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
        for m in net.modules():
            if isinstance(m, BottleNeck):
                m.bn3.weight.data.mul_(0.25)
        return net.train()

    x = randn((2, 64, 24, 24), F16, 3, cl=True)
    folded = {}
    for route in ("own", "stock", "f64"):
        net = build().to(DEV, F64 if route == "f64" else F32)
        if route != "f64":
            channels_last_filters(net)
        if route == "own":
            assert S.train_batchnorm(net) == 17
        params = [p for n, p in net.named_parameters() if not n.startswith("backbone.backbone.0.")]
        xin = x.to(F64) if route == "f64" else x
        # (stock: f32 masters over the same f16 tensors need autocast, as in tests/test_gpu_train_conv.py)
        with torch.enable_grad(), torch.autocast("cuda", F16, enabled=route == "stock"):
            outs = net.backbone._stages(xin)
            loss = sum((o.double() * randn(o.shape, F64, 40 + i).to(o.device)).sum() for i, o in enumerate(outs)) / 1000
            loss.backward()
        with torch.no_grad():
            for p in params:
                p -= 0.05 * p.grad
        assert all(int(b.bn1.num_batches_tracked) == 1 and int(b.bn3.num_batches_tracked) == 1
                   for b in net.modules() if isinstance(b, BottleNeck))
        net.eval()
        fold_batchnorm(net)
        folded[route] = {n: p.detach() for n, p in net.named_parameters() if not n.startswith("backbone.backbone.0.")}
        assert all(isinstance(m.conv1, FusedConv2d) for m in net.modules() if isinstance(m, BottleNeck))
    assert len(folded["own"]) == 2 * 17 - 2 and set(folded["own"]) == set(folded["f64"])
    bad = []
    for n, ref in folded["f64"].items():
        e_prod, e_stock = rel(folded["own"][n], ref), rel(folded["stock"][n], ref)
        bound = FACTOR * e_stock + 2 * U[F32]
        print("%-50s e_prod %.3e e_stock %.3e ratio %.3f" % (n, e_prod, e_stock, e_prod / bound))
        if not e_prod <= bound:
            bad.append("%s: e_prod %.3e > %g * %.3e + 2u" % (n, e_prod, FACTOR, e_stock))
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------- the C entry points on guarded buffers
class Guarded:
    """typed buffers of exactly the stated size inside one allocation pre-filled with a byte, with canaries around each"""
    FRONT = BACK = 4096

    def __init__(self, fill):
        self.fill, self.bufs = fill, {}

    def new(self, name, shape, dtype):
        n = int(torch.tensor(shape).prod()) * torch.empty((), dtype=dtype).element_size()
        whole = torch.full((self.FRONT + n + self.BACK,), self.fill, dtype=torch.uint8, device=DEV)
        view = whole[self.FRONT:self.FRONT + n].view(dtype).view(shape)
        assert view.data_ptr() % 16 == 0
        self.bufs[name] = (whole, n, view)
        return view

    def check(self):
        torch.cuda.synchronize()
        for name, (whole, n, _) in self.bufs.items():
            assert bool((whole[:self.FRONT] == self.fill).all()) and bool((whole[self.FRONT + n:] == self.fill).all()), \
                "%s: a canary byte was written" % name


def _raw_passes(fill, name, relu, res, pdtype):
    """the four passes through the C ABI on guarded outputs -> {name: tensor}, canaries checked"""
    from s2anet_amd import _lib
    L = _lib.lib()
    B, C, H, W = SHAPES[name]
    P = B * H * W
    bn, x, r, cot = make(name, pdtype == F32)
    xs = x.permute(0, 2, 3, 1).reshape(P, C)
    rs = r.permute(0, 2, 3, 1).reshape(P, C) if res else None
    go = cot.permute(0, 2, 3, 1).reshape(P, C)
    assert xs.data_ptr() == x.data_ptr()
    g = Guarded(fill)
    n = L.s2a_bn_slices(P, C)
    partial, mean, invstd = g.new("partial", (n, 2, C), F32), g.new("mean", (C,), F32), g.new("invstd", (C,), F32)
    out = g.new("out", (P, C), F16)
    rm, rv = g.new("running_mean", (C,), pdtype), g.new("running_var", (C,), pdtype)
    rm.copy_(bn.running_mean), rv.copy_(bn.running_var)
    partial2, coef = g.new("partial_bwd", (n, 2, C), F32), g.new("coef", (2, C), F32)
    gw, gb = g.new("grad_weight", (C,), pdtype), g.new("grad_bias", (C,), pdtype)
    gmask, gx = g.new("g", (P, C), F16), g.new("grad_input", (P, C), F16)
    st, code, ptr = _lib.stream_ptr(DEV), _lib.dtype_code(bn.weight), _lib.ptr
    w, b = bn.weight.detach(), bn.bias.detach()
    _lib.check(L.s2a_bn_train_stats_f16(ptr(xs), P, C, bn.eps, bn.momentum, ptr(partial), n, ptr(mean), ptr(invstd), ptr(rm), ptr(rv),
                                        code, st))
    _lib.check(L.s2a_bn_train_apply_f16(ptr(xs), ptr(mean), ptr(invstd), ptr(w), ptr(b), code, ptr(rs), ptr(out), P, C, int(relu), st))
    _lib.check(L.s2a_bn_backward_reduce_f16(ptr(go), ptr(xs), ptr(out) if relu else None, ptr(mean), ptr(invstd),
                                            ptr(gmask) if relu else None, ptr(partial2), n, ptr(gw), ptr(gb), code, ptr(coef), P, C, st))
    _lib.check(L.s2a_bn_backward_input_f16(ptr(gmask if relu else go), ptr(xs), None, ptr(mean), ptr(invstd), ptr(w), code, ptr(coef),
                                           ptr(gx), P, C, st))
    g.check()
    outs = {k: v[2] for k, v in g.bufs.items()}
    if not relu:
        assert bool((g.bufs["g"][0] == fill).all())          # not asked for: not touched
        del outs["g"]
    return outs


@pytest.mark.parametrize("pdtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("relu,res", [(True, True), (False, False)], ids=["relu_res", "plain"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_output_byte_is_written_and_nothing_beside_it(name, relu, res, pdtype):
    """outputs and `partial` pre-filled with 0xA5 and with 0xFF (NaN in every float format): the same bits come out of both
    runs, so no byte of them kept its fill; the canaries around each keep theirs"""
    a, b = _raw_passes(0xA5, name, relu, res, pdtype), _raw_passes(0xFF, name, relu, res, pdtype)
    assert set(a) == set(b) and len(a) >= 11
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
        assert not bool(torch.isnan(b[k]).any()), k


# ----------------------------------------------------------------------------- non-finite values
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("where", ["x", "grad_out"])
def test_planted_non_finite_value_gives_float64s_class_map(where, value):
    """one NaN / +-inf planted in x or in grad_out: every tensor has float64's map of finite / NaN / +inf / -inf entries, the
    other channels keep their bits, and the ReLU keeps a NaN"""
    bn, x, r, cot = make("ragged", True)
    clean = run(bn, x, r, cot, True, "ALL", True)
    x2, cot2 = x.clone(memory_format=torch.preserve_format), cot.clone(memory_format=torch.preserve_format)
    # at the channel's largest clean output: the ReLU passes there, so a planted gradient is not masked away (the float64
    # reference multiplies by the mask, and 0 * NaN is not the 0 a select gives)
    ib, ih, iw = (int(v) for v in torch.unravel_index(clean["out"][:, 7].argmax(), clean["out"][:, 7].shape))
    assert float(clean["out"][ib, 7, ih, iw]) > 0
    (x2 if where == "x" else cot2)[ib, 7, ih, iw] = value
    got = run(bn, x2, r, cot2, True, "ALL", True)
    mask = (got["out"] > 0) | got["out"].isnan()             # torch's ReLU backward: a NaN output passes the gradient
    ref, _ = reference(bn, x2, r, cot2, True, mask)
    if where == "x":
        assert bool(got["out"][:, 7].isnan().all())          # the ReLU keeps the NaN of the whole channel

    def classes(t):
        t = t.to(F64)
        return torch.where(t.isnan(), 3, torch.where(t == float("inf"), 2, torch.where(t == float("-inf"), 1, 0)))
    for name in ("out", "x", "weight", "bias", "residual", "running_mean", "running_var"):
        assert torch.equal(classes(got[name]), classes(ref[name])), (name, int((classes(got[name]) != classes(ref[name])).sum()))
        keep = [c for c in range(x.shape[1]) if c != 7]
        a, b = (got[name][:, keep], clean[name][:, keep]) if got[name].dim() == 4 else (got[name][keep], clean[name][keep])
        assert torch.equal(a, b), name
    assert not bool(torch.isfinite(got["weight"][7]))
