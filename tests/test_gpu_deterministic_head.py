"""GPU: the S2ANet head's training step in deterministic mode (s2anet_amd.deterministic + train_kernels): every layer of
the head on the project's kernels -- the narrow prediction convs and odm_cls_ls[0] at the zero-padded width, ORConv2d
through FusedConvFunction on the expanded filter, AlignConv's input gradient in fixed point -- so that forward + loss +
backward is bit-equal from run to run and from a captured graph to eager.

A head with feat_channels = 256 (so that the 32 -> 256 layer behind the orientation pooling exists), 15 classes,
fuse_epilogues, levels 16 x 20, 8 x 10, 4 x 5, 3 x 3 (every map takes AlignConv's fused route: the mode refuses the
unfused one), batch 2, f16 parameters or f32 masters under f16 features.  in_channels is 256 as well, not 64: S2ANetHead
applies align_conv, built feat_channels -> feat_channels, to the level's INPUT (models/head.py does the same), so a head
whose two widths differ is not a valid module.

Accuracy: the verify machinery of tests/test_gpu_train_conv.py for the padded layers and the check machinery of
tests/test_gpu_autograd_twin.py for ORConv2d and the whole head, with their constants (FACTOR, U)."""
import math

import pytest
import torch
import torch.nn as nn

from oracle import twin64 as T
from test_gpu_autograd_twin import DEV, F16, F32, channels_last_filters, check, named_leaves, randn, set_pattern
from test_gpu_train_conv import run, verify

pytestmark = pytest.mark.gpu

LEVELS = ((16, 20), (8, 10), (4, 5), (3, 3))                # a 128 x 160 image, strides 8 .. 64
IMG = (128, 160)
B = 2
LOSS_SCALE = 1024.0                                         # f16 training runs under a loss scale: without one the negatives' focal
                                                            # gradients (1e-6 per logit) underflow to exact zeros on the way to the features


def make_head(master, seed=61):
    from s2anet_amd.detector import fuse_epilogues
    from s2anet_amd.head import S2ANetHead
    torch.manual_seed(seed)
    head = S2ANetHead(15, in_channels=256, feat_channels=256).train()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, nn.Conv2d) and m.weight.shape[-1] == 3:
                m.weight.normal_(0, 0.02)
        head.align_conv.deform_conv.weight.normal_(0, 0.02)
    fuse_epilogues(head)
    head = head.to(DEV, F32 if master else F16)
    channels_last_filters(head)
    head.or_conv.channels_last = True
    head.imgs_size = IMG
    return head


def make_feats(grad=True, seed=70):
    return [randn((B, 256, h, w), F16, seed + i, cl=True, grad=grad) for i, (h, w) in enumerate(LEVELS)]


def make_targets(seed, n=14, rows=24):
    """a static table of `rows` rows, the first n real (image, class, x, y, w, h, angle in pixels / rad), the rest padding"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.full((rows, 7), -1.0, device=DEV)
    t[:n, 0] = torch.randint(0, B, (n,), device=DEV, generator=g).float()
    t[:n, 1] = torch.randint(0, 15, (n,), device=DEV, generator=g).float()
    t[:n, 2] = 16 + torch.rand((n,), device=DEV, generator=g) * (IMG[1] - 32)
    t[:n, 3] = 16 + torch.rand((n,), device=DEV, generator=g) * (IMG[0] - 32)
    t[:n, 4:6] = 12 + torch.rand((n, 2), device=DEV, generator=g) * 60
    t[:n, 6] = (torch.rand((n,), device=DEV, generator=g) - 0.25) * math.pi
    return t


def boom(*a, **kw):
    raise AssertionError("the library convolution was reached")


def no_library_conv(monkeypatch):
    """F.conv2d raises: s2anet_amd.fused.F and s2anet_amd.orn.F are torch.nn.functional itself, so nn.Conv2d.forward raises too"""
    from s2anet_amd import fused, orn
    monkeypatch.setattr(fused.F, "conv2d", boom)
    monkeypatch.setattr(orn.F, "conv2d", boom)


def train_step(head, feats, table):
    p = head(feats)["pred"]
    loss, items, status = head.compute_loss_device(p, table)
    (loss * LOSS_SCALE).backward()
    return loss, items, status


# ----------------------------------------------------------------------------- 1. no library convolution
@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
def test_no_library_convolution_in_the_head(master, monkeypatch):
    import s2anet_amd as S
    head = make_head(master)
    feats = make_feats()
    assert S.train_kernels(head) >= 8                          # (counts FusedConv2d only; ORConv2d is set as well)
    assert head.or_conv.own_grad is True
    no_library_conv(monkeypatch)
    with S.deterministic(True):
        loss, items, status = train_step(head, feats, make_targets(1))
    assert int(status[0]) == 0 and int(status[2]) == 14 and bool(torch.isfinite(loss).all())
    for n, p in head.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
    for i, f in enumerate(feats):
        assert f.grad is not None and f.grad.shape == f.shape and bool(torch.isfinite(f.grad).all()), i
        # (the 128- and 256-pixel anchors of the two coarse levels leave a 128 x 160 image and are ignored by the assignment:
        # those levels may legitimately receive an all-zero gradient)
        assert i >= 2 or float(f.grad.abs().max()) > 0, i


# ----------------------------------------------------------------------------- 2. per-layer accuracy
PADDED = {  # name: (k, C, O, relu): the widths train_conv_ok refuses and train_pad_widths takes
    "fam_reg_head_1x1_64x5": (1, 64, 5, False), "fam_cls_head_1x1_64x15": (1, 64, 15, False),
    "odm_reg_head_3x3_64x5": (3, 64, 5, False), "odm_cls_head_3x3_64x15": (3, 64, 15, False),
    "odm_cls_ls0_3x3_32x256_relu": (3, 32, 256, True), "narrow_both_3x3_32x15": (3, 32, 15, False),
}
MAPS = {3: ((2, 9, 21), (2, 3, 5)), 1: ((3, 7, 9),)}       # (B, H, W): partial tiles / one partial tile; 189 positions


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
@pytest.mark.parametrize("layer", list(PADDED))
def test_padded_layer_accuracy_every_pattern(layer, master, monkeypatch):
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d, train_pad_widths
    k, C, O, relu = PADDED[layer]
    for (b, H, W) in MAPS[k]:
        torch.manual_seed(11)
        m = FusedConv2d(C, O, k, 1, k // 2, relu=relu).to(DEV, F32 if master else F16)
        with torch.no_grad():
            m.bias.normal_(0, 0.5)
        x = randn((b, C, H, W), F16, 1, cl=True)
        cot = randn((b, O, H, W), F16, 3, cl=True)
        assert not S.train_conv_ok(x, m, None)
        with S.deterministic(True):
            assert train_pad_widths(x, m) == (max(C, 64), max(O, 64))
            with monkeypatch.context() as mp:               # the route really is the own one
                no_library_conv(mp)
                got = run(m, x, None, cot, "ALL", True)
                assert got["x"] is not None and got["weight"].shape == m.weight.shape and got["bias"].shape == m.bias.shape
            verify("det/%s/%dx%dx%d/%s" % (layer, b, H, W, "f32" if master else "f16"), m, x, None, cot, master,
                   ("ALL", "X", "PAR", "BIAS"))
            again = run(m, x, None, cot, "ALL", True)
            for name, t in got.items():
                assert (t is None and again[name] is None) or torch.equal(t, again[name]), (layer, name)


def orconv_case(master, H, W):
    import s2anet_amd as S
    torch.manual_seed(51)
    conv = S.ORConv2d(64, 8, kernel_size=3, padding=1, arf_config=(1, 8)).to(DEV)
    with torch.no_grad():
        conv.bias.normal_(0, 0.3)
    conv = conv.to(F32 if master else F16).train()
    pool = S.RotationInvariantPooling(64, 8)
    x = randn((B, 64, H, W), F16, 10, cl=True)

    def prod():
        y = conv(x)
        return y, pool(y)
    return conv, x, {"x": x, "weight": conv.weight, "bias": conv.bias}, prod, \
        (lambda tw, dt: T.orconv_pool(tw(x), tw(conv.weight), tw(conv.bias), conv.indices, dtype=dt))


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
@pytest.mark.parametrize("pattern", ["ALL", "IN", "PAR", "BIAS"])
@pytest.mark.parametrize("hw", [(9, 21), (3, 5)], ids=["9x21", "3x5"])
def test_orconv_accuracy_every_pattern(hw, pattern, master, monkeypatch):
    """IN is the X pattern of the conv tests: only the input requires grad"""
    import s2anet_amd as S
    conv, x, leaves, prod, twin = orconv_case(master, *hw)
    S.train_kernels(conv)
    set_pattern(pattern, [x], conv)
    with S.deterministic(True):
        with monkeypatch.context() as mp, torch.enable_grad():
            no_library_conv(mp)
            y, _ = prod()
            assert y.dtype == F16 and y.requires_grad
        check("det/orconv/%dx%d/%s/%s" % (*hw, pattern, "f32" if master else "f16"), F16, leaves, prod, twin)


# ----------------------------------------------------------------------------- 3. the head against the float64 twin
def test_head_through_the_twin_harness_in_the_mode():
    import s2anet_amd as S
    head = make_head(False)
    assert S.train_kernels(head) > 0
    feats = make_feats(grad=False)
    set_pattern("ALL", feats, head, frozen=("align_conv.",))
    leaves = dict(named_leaves(head), **{"feat%d" % i: f for i, f in enumerate(feats)})
    got = {}

    def prod():
        p = head(feats)["pred"]
        got["anchors"] = [a.detach() for a in p[4]]
        return p[:4]

    def twin(tw, dt):
        return T.head([tw(f) for f in feats], head.featmap_strides, T.head_params(head, tw), got["anchors"], dt)
    with S.deterministic(True):
        check("det/head/f16/ALL", F16, leaves, prod, twin, module=head)


# ----------------------------------------------------------------------------- 4. two fresh runs
def fresh_step(master):
    import s2anet_amd as S
    head = make_head(master)
    S.train_kernels(head)
    feats = make_feats()
    with S.deterministic(True):
        loss, items, status = train_step(head, feats, make_targets(2))
    assert int(status[0]) == 0
    out = {"loss": loss.detach(), "items": items.detach()}
    out.update({"grad(%s)" % n: p.grad for n, p in head.named_parameters()})
    out.update({"grad(feat%d)" % i: f.grad for i, f in enumerate(feats)})
    return out


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
def test_two_fresh_steps_are_bit_equal(master):
    a, b = fresh_step(master), fresh_step(master)
    assert set(a) == set(b) and len(a) > 20
    for name in a:
        assert a[name] is not None and torch.equal(a[name], b[name]), name


# ----------------------------------------------------------------------------- 5. one captured graph
def test_captured_step_replays_bit_equal_to_eager():
    """forward + compute_loss_device + backward captured once in the mode; replayed after in-place changes of features,
    targets and weights; every gradient, the features' included, equals eager on the same values.  The mode is switched
    OFF around the replays: a captured graph keeps the mode it was captured in."""
    import s2anet_amd as S
    head = make_head(True)
    S.train_kernels(head)
    feats = make_feats()
    table = make_targets(3)
    leaves = feats + list(head.parameters())

    def eager():
        for t in leaves:
            t.grad = None
        with torch.enable_grad(), S.deterministic(True):
            loss, items, status = train_step(head, feats, table)
        return [loss.detach().clone(), items.detach().clone(), status.clone()] + [t.grad.clone() for t in leaves]

    with S.deterministic(True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.enable_grad():
            train_step(head, feats, table)
        torch.cuda.current_stream().wait_stream(side)
        for t in leaves:
            t.grad = torch.zeros_like(t)
        static = [t.grad for t in leaves]
        graph = torch.cuda.CUDAGraph()
        with torch.enable_grad(), torch.cuda.graph(graph):
            s_loss, s_items, s_status = train_step(head, feats, table)
    assert S.deterministic() is False
    for round_ in range(2):
        with torch.no_grad():
            if round_:
                for i, f in enumerate(feats):
                    f.copy_(randn(tuple(f.shape), F16, 170 + i, cl=True))
                table.copy_(make_targets(4, n=9))
                for i, p in enumerate(head.parameters()):
                    p.mul_(1.125).add_(randn(tuple(p.shape), F32, 200 + i, scale=0.002))
            for g in static:
                g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = [s_loss.detach().clone(), s_items.detach().clone(), s_status.clone()] + [g.clone() for g in static]
        want = eager()
        for t, g in zip(leaves, static):
            t.grad = g
        assert int(got[2][0]) == 0 and int(got[2][2]) == (9 if round_ else 14)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (round_, i)


# ----------------------------------------------------------------------------- 6. mode off
def test_mode_off_leaves_no_trace(monkeypatch):
    import s2anet_amd as S
    from s2anet_amd import fused
    from s2anet_amd.fused import FusedConv2d
    torch.manual_seed(13)
    m = FusedConv2d(64, 15, 3, 1, 1, relu=True).to(DEV, F16)
    x = randn((2, 64, 9, 11), F16, 1, cl=True)
    cot = randn((2, 15, 9, 11), F16, 3, cl=True)
    with S.deterministic(True):
        with monkeypatch.context() as mp:
            no_library_conv(mp)
            run(m, x, None, cot, "ALL", True)                  # (the padded own route)
    assert S.deterministic() is False
    real, calls = fused.F.conv2d, []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(fused.F, "conv2d", counted)
    on = run(m, x, None, cot, "ALL", True)
    assert calls, "mode off: the narrow layer must reach the library as before"
    assert not S.train_conv_ok(x, m, None)
    assert on["out"].shape == cot.shape and on["weight"] is not None
