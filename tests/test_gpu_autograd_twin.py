"""Composed modules under autograd against the float64 twin (oracle/twin64.py).

The forward kernels are checked launch by launch and the backward kernels shape by shape; this file checks the WIRING:
production runs under torch.enable_grad() with a requires_grad pattern, fixed random cotangents are back-propagated
(vector-Jacobian products), and every output and every gradient is compared with the twin, which is written in stock
ops from the module definitions and shares no autograd graph with production.

Patterns:  ALL  everything requires grad          IN   only the inputs, the module is frozen
           PAR  inputs detached, parameters train  BIAS only the biases train

Structure, per case:
  * out.requires_grad equals the twin's;
  * a leaf that requires grad and whose twin gradient is non-zero has a gradient of its own dtype and shape;
  * a leaf that does not require grad has grad None;
  * a tensor whose twin gradient is exactly zero is exactly zero or None in production.
Accuracy, per tensor (output or gradient, no entry excluded):  e = |t - twin64|_2 / |twin64|_2,
      e_prod <= 4 e_stock + 2 u,        u = 2^-24 (f32) / 2^-11 (f16),
where e_stock is the same ratio of the twin run in the production dtype with stock ops on the GPU, measured in the same
test.  The factor 4 is what this project already allows its f16 AlignConv over a single-rounding convolution (L2_DCN
against L2_CONV in test_gpu_forward_shapes.py: other summation orders, the packed-half blend); 2 u is the final rounding
of the result.  ReLU / max decisions that flip between precisions occur in e_stock as well, hence an L2 ratio.
For f16 cases the twin gets the f16-rounded values.

Knife-edge decisions (every case with a ReLU or a max inside a module: convolutions, bottlenecks, AlignConv, head, detector).  One ReLU entry that takes the other
branch than float64 moves a gradient by 1e-3 ... 1e-2 of its norm, far more than rounding.  In f32, with 1e6 - 1e7 ReLU /
max entries per graph, about one entry per run has a float64 pre-activation inside the rounding error of zero; which one
depends on the library convolutions' summation order, which differs from run to run.  In f16 about 1 % of the entries
do, a handful per small level, and their count in production and in the baseline are two small Poisson draws.  Neither
branch is wrong there.  Production's branches are therefore recorded (forward hooks), and the float64 twin follows them
at the entries whose own pre-activation (top-two gap of a max) is within BAND * rms(tensor) -- and only there; an entry
OUTSIDE the band on which production and float64 differ is a structure violation.  The baseline takes the twin's
branches, so e_stock is rounding only and the bound keeps its meaning.  BAND = (L2 forward error of the deepest tensors in
u) x 5 (the largest of 1e6 entries over their rms) x 3 (margin): the outputs' measured e_prod is 1e-6 = 17 u in f32 and
7e-4 = 1.4 u in f16, hence 256 u (f32: 1e-5 of the entries can be affected) and 32 u (f16: 1 %).
Set S2A_AUTOGRAD_REPORT=<path> to write every
(case, tensor, e_prod, e_stock) as JSON."""
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import twin64 as T
from oracle.dcn64 import deform_conv64

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F16, F32, F64 = torch.float16, torch.float32, torch.float64
U = {F32: 2.0 ** -24, F16: 2.0 ** -11}
FACTOR = 4.0
BAND = {F32: 256 * 2.0 ** -24, F16: 32 * 2.0 ** -11}
_REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report_file():
    yield
    path = os.environ.get("S2A_AUTOGRAD_REPORT")
    if path:
        real = [r for r in _REPORT if not r["case"].startswith("planted")]
        worst = max((r["ratio"] for r in real), default=0.0)
        parts = max((r["ratio"] for r in real if not r["case"].startswith("detector")), default=0.0)
        with open(path, "w") as f:
            head = {"bound": "e_prod <= 4 e_stock + 2 u", "worst_ratio": worst, "worst_ratio_without_whole_detector": parts,
                    "rows_real": len(real), "rows_planted": len(_REPORT) - len(real)}
            f.write(json.dumps(head)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r) for r in _REPORT) + "\n]}\n")


# ----------------------------------------------------------------------------- the comparison
class Twin:
    """maps a production tensor to the twin's own leaf: same values in `dtype`, same requires_grad, no shared graph"""

    def __init__(self, dtype):
        self.dtype, self.map = dtype, {}

    def __call__(self, t):
        if t is None or not t.is_floating_point():
            return t
        e = self.map.get(id(t))
        if e is None:
            v = t.detach().to(self.dtype).contiguous().clone().requires_grad_(t.requires_grad)
            self.map[id(t)] = e = (t, v)
        return e[1]


class Recorder:
    """forward hooks that note, in call order, the branch production takes at every ReLU (FusedConv2d with a fused ReLU,
    nn.ReLU, AlignConv's own ReLU) and every max (MaxPool2d window, orientation pooling), in twin64.Decisions' form"""

    def __init__(self, module):
        from s2anet_amd.alignconv import AlignConv
        from s2anet_amd.fused import FusedConv2d
        from s2anet_amd.orn import RotationInvariantPooling
        self.taken, self.handles = [], []
        inner = {id(m) for a in module.modules() if isinstance(a, AlignConv) for m in a.modules() if m is not a}

        def relu(mod, inp, out):
            self.taken.append(out.detach() > 0)

        def pool(mod, inp, out):
            k, st, pd = mod.kernel_size, mod.stride, mod.padding
            self.taken.append(T._windows(inp[0].detach(), k, st, pd).argmax(-1))

        def rot(mod, inp, out):
            x = inp[0].detach()
            self.taken.append(x.unflatten(1, (x.shape[1] // mod.nOrientation, mod.nOrientation)).movedim(2, -1).argmax(-1))

        for m in module.modules():
            if id(m) in inner:
                continue
            if isinstance(m, (AlignConv, nn.ReLU)) or (isinstance(m, FusedConv2d) and m.fuse_relu):
                self.handles.append(m.register_forward_hook(relu))
            elif isinstance(m, nn.MaxPool2d):
                self.handles.append(m.register_forward_hook(pool))
            elif isinstance(m, RotationInvariantPooling):
                self.handles.append(m.register_forward_hook(rot))

    def remove(self):
        for h in self.handles:
            h.remove()


def _flat(outs):
    if isinstance(outs, torch.Tensor):
        return [outs]
    r = []
    for o in outs:
        if o is not None:
            r += _flat(o)
    return r


def _rel(a, ref):
    return float((a.to(F64) - ref).norm() / ref.norm())


def _backward(outs, cots):
    sel = [(o, c.to(o.dtype)) for o, c in zip(outs, cots) if o.requires_grad]
    if sel:
        torch.autograd.backward([o for o, _ in sel], [c for _, c in sel])


def compare(case, dtype, leaves, prod_fn, twin_fn, seed=0, module=None):
    """leaves {name: production leaf}; prod_fn() -> outputs; twin_fn(tw, dtype) -> the same outputs from tw(leaf) values.
    module: the production module tree whose ReLU / max branches the float64 twin follows inside BAND.
    -> (violations [str], rows): nothing is asserted here"""
    for t in leaves.values():
        t.grad = None
    rec = Recorder(module) if module is not None else None
    bad = []
    with torch.enable_grad():
        try:
            outs = _flat(prod_fn())
        finally:
            if rec is not None:
                rec.remove()
        tw64, tws = Twin(F64), Twin(dtype)
        if rec is None:
            o64, ost = _flat(twin_fn(tw64, F64)), _flat(twin_fn(tws, dtype))
        else:
            with T.decisions(T.Decisions(rec.taken, BAND[dtype])) as d64:
                o64 = _flat(twin_fn(tw64, F64))
            assert len(d64.taken) == len(rec.taken), (len(d64.taken), len(rec.taken))
            with T.decisions(T.Decisions(d64.taken, None)):
                ost = _flat(twin_fn(tws, dtype))
            print("%s: %d ReLU / max tensors, %d in-band entries follow production, %d differ outside the band" % (
                case, len(rec.taken), d64.followed, d64.disagree))
            if d64.disagree:
                bad.append("decisions: %d ReLU / max entries outside the band take another branch than float64" % d64.disagree)
    assert len(outs) == len(o64) == len(ost)
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
    cots = [torch.randn(o.shape, device=DEV, generator=gen, dtype=F32).to(dtype) for o in o64]
    rows, u = [], U[dtype]

    def accuracy(name, got, stock, ref):
        e_prod, e_stock = _rel(got, ref), _rel(stock, ref)
        bound = FACTOR * e_stock + 2 * u
        rows.append({"case": case, "tensor": name, "e_prod": e_prod, "e_stock": e_stock, "ratio": e_prod / bound})
        if not e_prod <= bound:
            bad.append("%s: e_prod %.3e > 4 * %.3e + 2u = %.3e (x%.1f)" % (name, e_prod, e_stock, bound, e_prod / bound))

    for i, (o, r, s) in enumerate(zip(outs, o64, ost)):
        name = "out%d" % i
        if tuple(o.shape) != tuple(r.shape) or o.dtype != dtype:
            bad.append("%s: shape / dtype %s %s, twin %s" % (name, tuple(o.shape), o.dtype, tuple(r.shape)))
            continue
        if o.requires_grad != r.requires_grad:
            bad.append("%s: requires_grad %s, twin %s" % (name, o.requires_grad, r.requires_grad))
        if float(r.detach().norm()) == 0:
            if float(o.detach().abs().max()) != 0:
                bad.append("%s: twin is exactly zero, production is not" % name)
            continue
        accuracy(name, o.detach(), s.detach(), r.detach())
    _backward(outs, cots)
    _backward(o64, cots)
    _backward(ost, cots)
    for name, t in leaves.items():
        g = t.grad
        if not t.requires_grad:
            if g is not None:
                bad.append("grad(%s): leaf does not require grad but has one" % name)
            continue
        r, s = tw64(t).grad, tws(t).grad
        if r is None or float(r.norm()) == 0:
            if g is not None and float(g.abs().max()) != 0:
                bad.append("grad(%s): twin gradient is exactly zero, production's is not" % name)
            continue
        if g is None:
            bad.append("grad(%s): None, twin gradient has norm %.3e" % (name, float(r.norm())))
            continue
        if g.dtype != t.dtype or tuple(g.shape) != tuple(t.shape):
            bad.append("grad(%s): %s %s for a leaf %s %s" % (name, g.dtype, tuple(g.shape), t.dtype, tuple(t.shape)))
            continue
        accuracy("grad(%s)" % name, g, s if s is not None else torch.zeros_like(r), r)
    for t in leaves.values():
        t.grad = None
    return bad, rows


def check(case, dtype, leaves, prod_fn, twin_fn, seed=0, module=None):
    bad, rows = compare(case, dtype, leaves, prod_fn, twin_fn, seed, module)
    _REPORT.extend(rows)
    for r in rows:
        print("%-60s %-40s e_prod %.3e e_stock %.3e ratio %.3f" % (case, r["tensor"], r["e_prod"], r["e_stock"], r["ratio"]))
    assert not bad, case + ":\n  " + "\n  ".join(bad)


def rejected(case, dtype, leaves, prod_fn, twin_fn, seed=0):
    """a planted defect: must violate a rule; -> the largest factor over the accuracy bound (inf for a structure rule)"""
    bad, rows = compare(case, dtype, leaves, prod_fn, twin_fn, seed)
    worst = max((r["ratio"] for r in rows), default=0.0)
    structural = [b for b in bad if "e_prod" not in b]
    _REPORT.extend(dict(r, case="planted:" + case) for r in rows if r["ratio"] > 1)
    print("planted %s: %d violations, worst accuracy ratio x%.1f, structure: %s" % (case, len(bad), worst, structural))
    assert bad, "planted defect %s was not noticed" % case
    return worst, structural


# ----------------------------------------------------------------------------- inputs
def randn(shape, dtype, seed, scale=1.0, cl=False, grad=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = (torch.randn(shape, device=DEV, generator=g, dtype=F32) * scale).to(dtype)
    if cl:
        t = t.contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(grad)


def set_pattern(pattern, inputs, module, frozen=()):
    """requires_grad of the inputs and of the module's parameters; frozen: parameter-name prefixes kept frozen (IN)"""
    for t in inputs:
        t.requires_grad_(pattern in ("ALL", "IN"))
    for n, p in module.named_parameters():
        if pattern == "ALL":
            p.requires_grad_(True)
        elif pattern == "IN":
            p.requires_grad_(not any(n.startswith(f) for f in frozen) if frozen else False)
        elif pattern == "PAR":
            p.requires_grad_(True)
        else:
            p.requires_grad_(n.endswith("bias"))


def channels_last_filters(module):
    for m in module.modules():
        if isinstance(m, nn.Conv2d) and m.weight.dim() == 4 and m.weight.shape[1] >= 8:
            m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    return module


def rotated_anchors(B, H, W, stride, seed):
    from s2anet_amd.loss import grid_anchors
    g = torch.Generator(device=DEV).manual_seed(seed)
    anc = grid_anchors((H, W), stride, 4.0, DEV).view(1, H, W, 5).repeat(B, 1, 1, 1)
    anc[..., :2] += torch.randn((B, H, W, 2), device=DEV, generator=g) * 3
    anc[..., 4] = torch.rand((B, H, W), device=DEV, generator=g) * 3.0 - 0.7
    return anc


def named_leaves(module, prefix=""):
    return {prefix + n: p for n, p in module.named_parameters()}


# ----------------------------------------------------------------------------- 1. FusedConv2d
FUSED_GEOM = {  # name: (cin, cout, k, stride, pad, relu, residual)
    "3x3": (64, 64, 3, 1, 1, False, False), "3x3_relu": (64, 64, 3, 1, 1, True, False),
    "3x3_res": (64, 64, 3, 1, 1, False, True), "3x3_relu_res": (64, 64, 3, 1, 1, True, True),
    "1x1_s2": (64, 128, 1, 2, 0, False, False), "3x3_head15": (64, 15, 3, 1, 1, False, False),
}


def fused_conv_case(geom, cl, dtype, pattern, hw=(9, 11), forward=None):
    from s2anet_amd.fused import FusedConv2d
    cin, cout, k, st, pad, relu, res = geom
    torch.manual_seed(11)
    m = FusedConv2d(cin, cout, k, st, pad, relu=relu).to(DEV, dtype)
    with torch.no_grad():
        m.bias.normal_(0, 0.5)
    if cl:
        m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    x = randn((2, cin, *hw), dtype, 1, cl=cl)
    ho, wo = (hw[0] + 2 * pad - k) // st + 1, (hw[1] + 2 * pad - k) // st + 1
    r = randn((2, cout, ho, wo), dtype, 2, cl=cl) if res else None
    set_pattern(pattern, [x] + ([r] if res else []), m)
    leaves = dict(named_leaves(m), x=x)
    if res:
        leaves["residual"] = r
    prod = (lambda: m(x, r)) if forward is None else (lambda: forward(m, x, r))
    return m, leaves, prod, (lambda tw, dt: T.fused_conv(tw(x), tw(m.weight), tw(m.bias), st, pad, relu, tw(r), dtype=dt))


@pytest.mark.parametrize("pattern", ["ALL", "IN", "PAR", "BIAS"])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("geom", list(FUSED_GEOM))
def test_fused_conv(geom, cl, dtype, pattern):
    m, leaves, prod, twin = fused_conv_case(FUSED_GEOM[geom], cl, dtype, pattern)
    check("fused_conv/%s/%s/%s/%s" % (geom, "nhwc" if cl else "nchw", dtype, pattern), dtype, leaves, prod, twin, module=m)


@pytest.mark.parametrize("pattern", ["ALL", "IN", "PAR", "BIAS"])
def test_fused_conv_six_channels_stock_epilogue(pattern):
    """6 maps: no 16-byte channel vectors, bias_act_ takes its stock-op fallback whatever the layout"""
    m, leaves, prod, twin = fused_conv_case((6, 6, 3, 1, 1, True, True), True, F32, pattern)
    check("fused_conv/6ch/nhwc/f32/%s" % pattern, F32, leaves, prod, twin, module=m)


def test_bias_act_out_buffer_with_a_gradient_wanted_is_refused():
    """out= writes a caller's buffer through its pointer: with a gradient wanted it raises instead of dropping it"""
    from s2anet_amd.fused import bias_act_
    y = randn((2, 8, 3, 5), F32, 1, cl=True)
    out = torch.empty_like(y)
    bias = randn((8,), F32, 2, grad=True)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="no backward"):
        bias_act_(y, bias, None, True, out=out)
    with torch.no_grad():
        assert bias_act_(y.clone(), bias, None, True, out=out) is out
        assert torch.equal(out, torch.relu(y + bias.view(1, -1, 1, 1)))


# ----------------------------------------------------------------------------- 2. folded bottlenecks
def folded_trunk(dtype):
    """layer1 (two blocks) and layer2's first block of the trunk, BN statistics randomised, folded, channels-last"""
    from s2anet_amd.detector import BottleNeck, DetectorBackbone, fold_batchnorm
    torch.manual_seed(21)
    net = nn.Module()
    net.backbone = DetectorBackbone(layers=(2, 1, 1, 1))
    g = torch.Generator().manual_seed(22)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_mean.data = torch.randn(m.bias.shape, generator=g) * 0.1
            m.running_var.data = torch.rand(m.bias.shape, generator=g) + 0.5
    for m in net.modules():
        if isinstance(m, BottleNeck):
            m.bn3.weight.data.mul_(0.25)
    net.eval()
    fold_batchnorm(net)
    return channels_last_filters(net.to(DEV, dtype)).backbone


@pytest.mark.parametrize("pattern", ["ALL", "IN", "PAR"])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("which", ["planes64", "planes128_s2_down", "run_blocks_2"])
def test_folded_bottleneck(which, dtype, pattern):
    from s2anet_amd.detector import DetectorBackbone
    from s2anet_amd.fused import FusedConv2d
    bb = folded_trunk(dtype)
    layer1, layer2 = bb.backbone[1][1], bb.backbone[2]
    if which == "planes64":
        blocks, cin = [layer1[1]], 256
    elif which == "planes128_s2_down":
        blocks, cin = [layer2[0]], 256
    else:
        blocks, cin = [layer1[0], layer1[1]], 64
    assert all(isinstance(b.conv3, FusedConv2d) for b in blocks)
    assert (blocks[0].downsample is not None) == (which != "planes64")
    mod = nn.Sequential(*blocks)
    # 9 x 11 at the block's OUTPUT: the stride-2 block gets 17 x 21.  (On 9 x 11 its conv2 would have 5 x 6 x 2 x 128 =
    # 7 680 outputs; in f16 a handful of them sit within an ulp of the ReLU's kink and flip against float64, each worth
    # about 1 % of a gradient's norm -- with so few, their count in production and in the baseline is two small Poisson
    # draws and the ratio of the two errors is noise.)
    hw = (17, 21) if which == "planes128_s2_down" else (9, 11)
    x = randn((2, cin, *hw), dtype, 3, cl=True)
    set_pattern(pattern, [x], mod)
    leaves = dict(named_leaves(mod), x=x)

    def prod():
        return DetectorBackbone.run_blocks(mod, x) if which == "run_blocks_2" else blocks[0](x)

    def twin(tw, dt):
        y = tw(x)
        for b in blocks:
            y = T.bottleneck_folded(y, T.bottleneck_params(b, tw), dt)
        return y
    check("bottleneck/%s/%s/%s" % (which, dtype, pattern), dtype, leaves, prod, twin, module=mod)


# ----------------------------------------------------------------------------- 3. FPN
@pytest.mark.parametrize("pattern", ["ALL", "PAR"])
def test_fpn_fused_epilogues(pattern):
    from s2anet_amd.detector import FPN, fuse_epilogues
    from s2anet_amd.fused import FusedConv2d
    torch.manual_seed(31)
    neck = FPN(in_channels=(64, 128, 256), out_channels=64)
    for m in neck.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.normal_(m.bias, 0, 0.3)
    neck = channels_last_filters(fuse_epilogues(neck).to(DEV, F32))
    assert all(isinstance(m, FusedConv2d) for m in list(neck.lateral_convs) + list(neck.fpn_convs))
    xs = [randn((2, c, h, w), F32, 4 + i, cl=True) for i, (c, h, w) in enumerate(((64, 16, 20), (128, 8, 10), (256, 4, 5)))]
    set_pattern(pattern, xs, neck)
    leaves = dict(named_leaves(neck), **{"x%d" % i: x for i, x in enumerate(xs)})
    check("fpn/f32/%s" % pattern, F32, leaves, lambda: neck(xs),
          lambda tw, dt: T.fpn([tw(x) for x in xs], T.fpn_params(neck, tw), dt), module=neck)


# ----------------------------------------------------------------------------- 4. AlignConv
ALIGN_CASES = {  # name: (cin, cout, H, W, dtype, S2A_DCN_F32, fused)
    "fused_f32_x3": (64, 64, 12, 16, F32, None, True), "fused_f32_mfma32": (64, 64, 12, 16, F32, "mfma32", True),
    "fused_f16": (64, 64, 12, 16, F16, None, True), "unfused_2x3": (64, 64, 2, 3, F32, None, False),
    "generic_16to8_7x9": (16, 8, 7, 9, F32, None, False),
}


def align_case(name, pattern):
    import s2anet_amd as S
    cin, cout, H, W, dtype, _, fused = ALIGN_CASES[name]
    torch.manual_seed(41)
    ac = S.AlignConv(cin, cout, 3).to(DEV, dtype)
    with torch.no_grad():
        ac.deform_conv.weight.normal_(0, 0.05)
    stride = 8
    anc = rotated_anchors(2, H, W, stride, 5)
    x = randn((2, cin, H, W), dtype, 6)
    assert ac.fused_ok(x) == fused
    set_pattern(pattern, [x], ac)
    w = ac.deform_conv.weight
    return ac, dtype, {"x": x, "weight": w}, (lambda: ac(x, anc, stride)), \
        (lambda tw, dt: T.align_conv(tw(x), anc, tw(w), stride, dt))


@pytest.mark.parametrize("pattern", ["ALL", "IN", "PAR"])
@pytest.mark.parametrize("name", list(ALIGN_CASES))
def test_align_conv(name, pattern, monkeypatch):
    if ALIGN_CASES[name][5]:
        monkeypatch.setenv("S2A_DCN_F32", ALIGN_CASES[name][5])
    else:
        monkeypatch.delenv("S2A_DCN_F32", raising=False)
    ac, dtype, leaves, prod, twin = align_case(name, pattern)
    check("align_conv/%s/%s" % (name, pattern), dtype, leaves, prod, twin, module=ac)


# ----------------------------------------------------------------------------- 5. deform_conv
@pytest.mark.parametrize("subset", range(1, 8), ids=lambda s: "".join(n for i, n in enumerate("xow") if s >> i & 1))
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_deform_conv_every_requires_grad_subset(dtype, subset):
    """bit 0: input, bit 1: offset, bit 2: weight.  weight only = the head-only fine-tune on detached features (the
    separate weight-only entry); input / offset without weight = the separate input entry"""
    import s2anet_amd as S
    x = randn((2, 64, 13, 21), dtype, 7, grad=bool(subset & 1))
    off = randn((2, 18, 13, 21), dtype, 8, scale=1.5, grad=bool(subset & 2))
    w = randn((32, 64, 3, 3), dtype, 9, scale=0.05, grad=bool(subset & 4))
    check("deform_conv/%s/%d" % (dtype, subset), dtype, {"x": x, "offset": off, "weight": w},
          lambda: S.deform_conv(x, off, w, 1, 1), lambda tw, dt: deform_conv64(tw(x), tw(off), tw(w), dtype=dt))


# ----------------------------------------------------------------------------- 6. ORConv2d + RotationInvariantPooling
def orconv_case(dtype, train):
    import s2anet_amd as S
    torch.manual_seed(51)
    conv = S.ORConv2d(64, 8, kernel_size=3, padding=1, arf_config=(1, 8)).to(DEV)
    with torch.no_grad():
        conv.bias.normal_(0, 0.3)
    conv = conv.to(dtype).train(train)
    pool = S.RotationInvariantPooling(64, 8)
    x = randn((2, 64, 9, 11), dtype, 10)

    def prod():
        y = conv(x)
        return y, pool(y)
    return conv, x, {"x": x, "weight": conv.weight, "bias": conv.bias}, prod, \
        (lambda tw, dt: T.orconv_pool(tw(x), tw(conv.weight), tw(conv.bias), conv.indices, dtype=dt))


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype,pattern", [(F32, "ALL"), (F32, "IN"), (F32, "PAR"), (F16, "ALL")])
def test_orconv_pool(dtype, pattern, train):
    conv, x, leaves, prod, twin = orconv_case(dtype, train)
    set_pattern(pattern, [x], conv)
    check("orconv_pool/%s/%s/%s" % (dtype, pattern, "train" if train else "eval"), dtype, leaves, prod, twin)


def test_orconv_frozen_then_trainable_again():
    """the frozen forward caches the ARF expansion; with requires_grad back on, the differentiable expansion must be used"""
    conv, x, leaves, prod, twin = orconv_case(F32, True)
    set_pattern("IN", [x], conv)
    check("orconv_pool/flip/frozen", F32, leaves, prod, twin)
    assert conv._arf_cache is not None
    set_pattern("ALL", [x], conv)
    check("orconv_pool/flip/trainable_again", F32, leaves, prod, twin)
    with torch.no_grad():                                  # an update in between: the frozen route must follow it
        conv.weight.mul_(1.5)
    set_pattern("IN", [x], conv)
    check("orconv_pool/flip/frozen_after_update", F32, leaves, prod, twin)


# ----------------------------------------------------------------------------- 7. the head
LEVELS = ((16, 20), (8, 10), (4, 5), (2, 3), (1, 2))          # a 128 x 160 image


def make_head(dtype, fused):
    from s2anet_amd.detector import fuse_epilogues
    from s2anet_amd.head import S2ANetHead
    torch.manual_seed(61)
    head = S2ANetHead(15, in_channels=64, feat_channels=64).train()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, nn.Conv2d) and m.weight.shape[-1] == 3:
                m.weight.normal_(0, 0.05)
        head.align_conv.deform_conv.weight.normal_(0, 0.05)
    if fused:
        fuse_epilogues(head)
    head = head.to(DEV, dtype)
    if fused:
        channels_last_filters(head)
        head.or_conv.channels_last = True
    return head


def head_case(head, dtype, pattern, cl):
    feats = [randn((2, 64, h, w), dtype, 70 + i, cl=cl) for i, (h, w) in enumerate(LEVELS)]
    set_pattern(pattern, feats, head, frozen=("align_conv.",))
    leaves = dict(named_leaves(head), **{"feat%d" % i: f for i, f in enumerate(feats)})
    got = {}

    def prod():
        p = head(feats)["pred"]
        got["anchors"] = [a.detach() for a in p[4]]
        return p[:4]

    def twin(tw, dt):
        return T.head([tw(f) for f in feats], head.featmap_strides, T.head_params(head, tw), got["anchors"], dt)
    return leaves, prod, twin


@pytest.mark.parametrize("form,dtype,pattern", [("plain", F32, "ALL"), ("plain", F32, "PAR"), ("plain", F32, "IN"),
                                                ("fused", F32, "ALL"), ("fused", F32, "PAR"), ("fused", F32, "IN"),
                                                ("fused", F16, "ALL")])
def test_head(form, dtype, pattern):
    """IN here: only align_conv is frozen (its filter gets no gradient, the features still do, through it)"""
    head = make_head(dtype, form == "fused")
    leaves, prod, twin = head_case(head, dtype, pattern, form == "fused")
    assert not head.align_conv.fused_ok(torch.empty((2, 64, 2, 3))) and head.align_conv.fused_ok(torch.empty((2, 64, 4, 5)))
    check("head/%s/%s/%s" % (form, dtype, pattern), dtype, leaves, prod, twin, module=head)


# ----------------------------------------------------------------------------- 8. the whole detector
def test_whole_detector():
    """model(imgs) of the folded f32 detector on a 2 x 3 x 128 x 160 image.  Cotangents go on the four differentiable
    prediction lists (fam_cls, fam_bbox, odm_cls, odm_bbox); the fifth list, the refined anchors, carries no gradient and
    is handed to the twin.  Compared: the stem, one bottleneck per stage (two of them with a downsample), every FPN
    lateral bias, every head parameter.  About 1e7 ReLU / max entries: the twin follows production's branch inside BAND
    (module docstring) and nowhere else."""
    from s2anet_amd.detector import build_synthetic_detector
    model = build_synthetic_detector(dtype=F32, device=DEV)
    imgs = torch.rand((2, 3, 128, 160), device=DEV, generator=torch.Generator(device=DEV).manual_seed(81))
    for p in model.parameters():
        p.requires_grad_(True)
    bb = model.backbone.backbone
    leaves = {"stem.weight": bb[0][0].weight, "stem.bias": bb[0][0].bias}
    for name, blk in (("layer1.0", bb[1][1][0]), ("layer2.1", bb[2][1]), ("layer3.0", bb[3][0]), ("layer4.2", bb[4][2])):
        leaves.update(named_leaves(blk, name + "."))
    assert "layer1.0.downsample.0.weight" in leaves and "layer3.0.downsample.0.bias" in leaves
    for i, l in enumerate(model.neck.lateral_convs):
        leaves["neck.lateral%d.bias" % i] = l.bias
    leaves.update(named_leaves(model.head, "head."))
    got = {}

    def prod():
        p = model(imgs)["pred"]
        got["anchors"] = [a.detach() for a in p[4]]
        assert [tuple(a.shape[1:3]) for a in p[4]] == list(LEVELS)
        return p[:4]

    def twin(tw, dt):
        return T.detector(tw(imgs), T.trunk_params(model.backbone, tw), T.fpn_params(model.neck, tw),
                          T.head_params(model.head, tw), model.stride, got["anchors"], dt)
    check("detector/f32/ALL", F32, leaves, prod, twin, module=model)


# ----------------------------------------------------------------------------- 9. planted defects
def test_planted_alignconv_backward_without_relu_mask(monkeypatch):
    from torch.autograd.function import once_differentiable
    from s2anet_amd import alignconv as A
    from s2anet_amd.dcn import _fused_backward
    monkeypatch.delenv("S2A_DCN_F32", raising=False)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):                        # AlignConvFunction.backward without the out <= 0 mask
        x, anchors, weight, out = ctx.saved_tensors
        B, C, H, W = x.shape
        offset = A.align_offsets(anchors.detach().reshape(B, H * W, 5), (H, W), ctx.stride, 3)
        gin, _, gw = _fused_backward(x, offset, weight.type_as(x), grad_output.contiguous())
        return gin, None, gw.to(weight.dtype), None
    monkeypatch.setattr(A.AlignConvFunction, "backward", backward)
    _, dtype, leaves, prod, twin = align_case("fused_f32_x3", "ALL")
    worst, _ = rejected("align_conv/no_relu_mask", dtype, leaves, prod, twin)
    assert worst > 100


def test_planted_rot_pool_backward_routes_to_next_orientation(monkeypatch):
    from s2anet_amd import orn
    real = orn.rot_inv_pool_backward

    def shifted(x, grad_output, n_orientation=8):
        g = real(x, grad_output, n_orientation)
        return g.unflatten(1, (g.shape[1] // n_orientation, n_orientation)).roll(1, 2).flatten(1, 2)
    monkeypatch.setattr(orn, "rot_inv_pool_backward", shifted)
    conv, x, leaves, prod, twin = orconv_case(F32, True)
    set_pattern("ALL", [x], conv)
    worst, _ = rejected("orconv_pool/next_orientation", F32, leaves, prod, twin)
    assert worst > 100


def test_planted_raw_epilogue_under_grad(monkeypatch):
    """the grad-enabled FusedConv2d branch as it was: F.conv2d, then the raw in-place epilogue that autograd cannot see"""
    from s2anet_amd import fused

    def forward(m, x, r):
        y = F.conv2d(x, m.weight, None, m.stride, m.padding, m.dilation, m.groups)
        return fused._bias_act_raw(y, m.bias, r, m.fuse_relu)
    for pattern, geom in (("ALL", "3x3_relu_res"), ("BIAS", "3x3")):
        _, leaves, prod, twin = fused_conv_case(FUSED_GEOM[geom], True, F32, pattern, forward=forward)
        worst, structural = rejected("fused_conv/raw_epilogue/%s" % pattern, F32, leaves, prod, twin)
        assert structural                                   # bias.grad is None / the output does not require grad
