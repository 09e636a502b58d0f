"""GPU: the 16-row form of the pyramid-packed 3x3 prediction convs (s2a_conv3x3_narrow_pyramid_f16, k_conv3x3_narrow_f16).

A ragged pyramid (batch 2, levels 20x28, 10x14, 5x7, 3x3, C = 256: partial tiles in x and y, levels smaller than a tile)
and a one-level pyramid (9x17, C = 64, batch 1: one chunk per tile, the lt.n == 1 table), O in {1, 5, 15, 16}, ReLU on
and off, N(0, 1) inputs, N(0, 1 / K) filters:
  * columns < O carry the bits of the 64-row launch (S2A_CONV_NARROW=0), columns O..63 the bit pattern 0x0000, and a second
    launch into a NaN-filled buffer gives the same bits;
  * against float64 (oracle/conv64.py): |err| <= (u16 + (K + 17) u32) S + 2^-25 elementwise and relative L2 <= 2 u16, the
    bounds of tests/test_gpu_forward_shapes.py for this layer kind;
  * S2A_CONV_NARROW_WGS = 1 and 3 (a workgroup walks tiles of several levels and images, the last run is short): same bits;
  * routing: O = 17, a residual, C = 32 go to s2a_conv3x3_pyramid_f16; the head's two prediction convs reach the new symbol
    once each (with 15 and 5 maps); forward_pyramid keeps every packed buffer's bits and S2ANet.detect gives the same
    detections, labels and counts with the switch on and off (256 x 256, where P7 is too small for the packed head and the
    per-level path runs, and 384 x 384, where it is taken; S2A_OWN_CONV_ALWAYS=1, see there).
The float64 references are computed once per (pyramid, O) and shared."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16, U32 = 2.0 ** -11, 2.0 ** -24
TINY = 2.0 ** -25
NARROW, WIDE = "s2a_conv3x3_narrow_pyramid_f16", "s2a_conv3x3_pyramid_f16"

PYRAMIDS = {"ragged": (2, [(20, 28), (10, 14), (5, 7), (3, 3)], 256), "one_level": (1, [(9, 17)], 64)}
OS = [1, 5, 15, 16]
_cache = {}


def case(pyr, O):
    """operands, packed filter, 64-entry bias and the float64 reference (pre-activation) of one (pyramid, O)"""
    key = (pyr, O)
    if key not in _cache:
        from oracle.conv64 import conv64
        from s2anet_amd.fused import conv_pack_weight
        from s2anet_amd.pyramid import PyramidLayout
        B, sizes, C = PYRAMIDS[pyr]
        g = torch.Generator().manual_seed(100 * O + C)
        layout = PyramidLayout(B, sizes, [8 * 2 ** i for i in range(len(sizes))])
        x = torch.randn(layout.pixels, C, generator=g).to(DEV).half()
        w = (torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(DEV).half()
        b = (torch.randn(O, generator=g) * 0.5).to(DEV).half()
        b64 = torch.zeros(64, dtype=torch.float16, device=DEV)
        b64[:O] = b
        ref = [conv64(layout.level(x, l), w, b, 1, 3) for l in range(len(sizes))]
        _cache[key] = dict(layout=layout, x=x, w=w, b=b, b64=b64, packed=conv_pack_weight(w), ref=ref, C=C)
    return _cache[key]


def launch(c, O, relu):
    """pyramid.conv3x3 into a NaN-filled [P,64] buffer"""
    from s2anet_amd import pyramid as P
    out = torch.full((c["layout"].pixels, 64), float("nan"), dtype=torch.float16, device=DEV)
    got = P.conv3x3(c["layout"], c["x"], c["packed"], c["b64"], O, relu, out=out)
    assert got is out
    return out


class CountingLib:
    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("s2a_"):
            return fn

        def call(*a):
            self.calls.append((name, a))
            return fn(*a)
        return call

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)


@pytest.fixture
def counting(monkeypatch):
    from s2anet_amd import _lib
    proxy = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", proxy)
    return proxy


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for k in ("S2A_CONV_NARROW", "S2A_CONV_NARROW_WGS", "S2A_CONV_OG", "S2A_CONV_PH"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("pyr", list(PYRAMIDS))
def test_bits_of_the_64_row_launch_and_float64_bounds(pyr, O, relu, monkeypatch, counting):
    c = case(pyr, O)
    got = launch(c, O, relu)
    assert counting.count(NARROW) == 1 and counting.count(WIDE) == 0
    monkeypatch.setenv("S2A_CONV_NARROW", "0")
    parent = launch(c, O, relu)
    monkeypatch.delenv("S2A_CONV_NARROW")
    assert not torch.isnan(parent).any()
    assert torch.equal(got[:, :O], parent[:, :O]), (got[:, :O].float() - parent[:, :O].float()).abs().max().item()
    assert torch.equal(got.view(torch.int16)[:, O:], torch.zeros_like(got.view(torch.int16)[:, O:]))
    assert torch.equal(parent.view(torch.int16)[:, O:], torch.zeros_like(got.view(torch.int16)[:, O:]))
    assert torch.equal(launch(c, O, relu).view(torch.int16), got.view(torch.int16))      # every element written again
    # the OG / PH switches of the 64-row launch do not reach this route
    for k, v in (("S2A_CONV_OG", "1"), ("S2A_CONV_OG", "2"), ("S2A_CONV_PH", "1"), ("S2A_CONV_PH", "2")):
        monkeypatch.setenv(k, v)
        assert torch.equal(launch(c, O, relu).view(torch.int16), got.view(torch.int16)), (k, v)
        monkeypatch.delenv(k)
    K = 9 * c["C"]
    tau = U16 + (K + 17) * U32
    e2 = y2 = 0.0
    worst = 0.0
    layout = c["layout"]
    for l, (y, S) in enumerate(c["ref"]):
        yl = y.clamp_min(0) if relu else y
        err = (layout.level(got, l, O).double() - yl).abs()
        worst = max(worst, ((err - TINY).clamp_min(0) / S.clamp_min(1e-300)).max().item())
        assert int((~(err <= tau * S + TINY)).sum()) == 0, (l, worst, tau)
        e2 += err.square().sum().item()
        y2 += yl.square().sum().item()
    l2 = e2 ** 0.5 / max(y2 ** 0.5, 1e-300)
    print("narrow %s O=%d relu=%d: max err/S %.3g (tau %.3g), relative L2 %.3g (bound %.3g)" % (pyr, O, relu, worst, tau, l2, 2 * U16))
    assert l2 <= 2 * U16
    assert (got[:, :O] != 0).float().mean().item() > 0.2


@pytest.mark.parametrize("wgs", ["1", "3"])
@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("pyr", list(PYRAMIDS))
def test_persistent_workgroups_cross_levels_and_images(pyr, O, wgs, monkeypatch):
    c = case(pyr, O)
    for relu in (False, True):
        ref = launch(c, O, relu)
        monkeypatch.setenv("S2A_CONV_NARROW_WGS", wgs)
        got = launch(c, O, relu)
        monkeypatch.delenv("S2A_CONV_NARROW_WGS")
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (relu, wgs)


def test_more_than_16_maps_a_residual_or_32_inputs_take_the_64_row_launch(counting):
    from s2anet_amd import pyramid as P
    from s2anet_amd.fused import conv_pack_weight
    c = case("ragged", 5)
    layout = c["layout"]
    g = torch.Generator().manual_seed(7)
    w17 = (torch.randn(17, 256, 3, 3, generator=g) / 48).to(DEV).half()
    b64 = torch.zeros(64, dtype=torch.float16, device=DEV)
    a = P.conv3x3(layout, c["x"], conv_pack_weight(w17), b64, 17, False)
    assert a.shape == (layout.pixels, 64) and counting.count(WIDE) == 1 and counting.count(NARROW) == 0
    assert torch.equal(a, P.conv3x3(layout, c["x"], conv_pack_weight(w17), b64, 64, False))
    counting.calls.clear()
    res = torch.randn(layout.pixels, 64, generator=g).to(DEV).half()
    r = P.conv3x3(layout, c["x"], c["packed"], c["b64"], 5, False, residual=res)
    assert r.shape == (layout.pixels, 64) and counting.count(WIDE) == 1 and counting.count(NARROW) == 0
    plain = launch(c, 5, False)
    assert counting.count(NARROW) == 1
    assert torch.equal(r[:, :5], (plain[:, :5].float() + res[:, :5].float()).half())     # rnd16(rnd16(acc + b) + r)
    counting.calls.clear()
    x32 = torch.randn(layout.pixels, 32, generator=g).to(DEV).half()
    w32 = (torch.randn(5, 32, 3, 3, generator=g) / 17).to(DEV).half()
    o = P.conv3x3(layout, x32, conv_pack_weight(w32), b64, 5, False)
    assert o.shape == (layout.pixels, 64) and counting.count(WIDE) == 1 and counting.count(NARROW) == 0
    assert torch.equal(o, P.conv3x3(layout, x32, conv_pack_weight(w32), b64, 64, False))


@pytest.fixture(scope="module")
def detector():
    from s2anet_amd.detector import build_synthetic_detector
    model = build_synthetic_detector(device=DEV)
    model.head.odm_cls_head.bias.data.fill_(-2.0)       # a score spread that leaves detections (as smoke() does)
    model.head.odm_cls_head.weight.data.mul_(20.0)
    return model


def images(size):
    return torch.randint(0, 256, (2, 3, size, size), dtype=torch.uint8, device=DEV,
                         generator=torch.Generator(DEV).manual_seed(size)).contiguous(memory_format=torch.channels_last)


def test_head_reaches_the_new_symbol_once_per_prediction_conv(detector, counting):
    with torch.no_grad():
        detector.detect(images(384))
    torch.cuda.synchronize()
    used = sorted(int(a[6]) for n, a in counting.calls if n == NARROW)
    assert used == [5, 15], used
    # what still goes to the 64-row entry point are the towers (64 maps or more), not a prediction conv
    wide = [int(a[7]) for n, a in counting.calls if n == WIDE]
    assert wide and all(o >= 64 and o % 64 == 0 for o in wide), wide


def test_head_predictions_do_not_depend_on_the_switch(detector, monkeypatch):
    """forward_pyramid on random features: every packed buffer of the head, the two predictions included, keeps its bits"""
    from s2anet_amd.pyramid import PyramidLayout
    head = detector.head
    layout = PyramidLayout(2, [(20, 28), (10, 14), (5, 7), (3, 4), (3, 3)], head.featmap_strides)
    x = torch.randn(layout.pixels, head.in_channels, generator=torch.Generator().manual_seed(3)).to(DEV).half()
    on, off = {}, {}
    with torch.no_grad():
        head.forward_pyramid(layout, x, trace=on)
        monkeypatch.setenv("S2A_CONV_NARROW", "0")
        head.forward_pyramid(layout, x, trace=off)
    for k, cols in (("odm_cls", 64), ("odm_bbox", 64), ("or_feat", 256), ("pooled", 32), ("anchors", 5), ("fam_bbox", 5)):
        a, b = on[k][:, :cols], off[k][:, :cols]      # (the fused FAM heads write 32 of their 64 columns)
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a,
                           b.view(torch.int16) if b.dtype == torch.float16 else b), k
    assert on["odm_cls"].shape == (layout.pixels, 64) and (on["odm_cls"][:, :15] != 0).any()
    assert not on["odm_cls"][:, 15:].view(torch.int16).any() and not on["odm_bbox"][:, 5:].view(torch.int16).any()


@pytest.mark.parametrize("size", [256, 384])
def test_detections_do_not_depend_on_the_switch(detector, size, monkeypatch, counting):
    # FPN's two library convolutions (P6 / P7) do not repeat their bits from call to call -- detect() of the parent commit
    # differs from itself on these images -- so every layer runs on the own kernels here, as in tests/test_gpu_conv3_chain.py
    monkeypatch.setenv("S2A_OWN_CONV_ALWAYS", "1")
    imgs = images(size)
    with torch.no_grad():
        on = detector.detect(imgs)
        n_on = counting.count(NARROW)
        monkeypatch.setenv("S2A_CONV_NARROW", "0")
        off = detector.detect(imgs)
    torch.cuda.synchronize()
    assert n_on == (2 if size == 384 else 0)            # 256 x 256: P7 is 2 x 2, the head runs per level
    assert int(on[2].min()) > 0
    for a, b, name in zip(on, off, ("detections", "labels", "counts")):
        assert torch.equal(a, b), name
