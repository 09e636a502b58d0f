"""GPU: the opt-in e4m3 tower route of S2ANetHead.forward_pyramid (s2anet_amd/fp8.py).

Synthetic detector (He-initialised towers: O(1) activations), head layout batch 2 with levels 20x28, 10x14, 5x7, 3x4, 3x3.
  * mode off (also after calibration): no fp8 symbol is called; enabled then disabled: every packed output has the bits of a
    twin that was never enabled; enabling before calibration raises;
  * mode on: exactly five s2a_conv3x3_pyramid_fp8 and three s2a_quantize_e4m3 calls; every fp8 launch is checked ON ITS OWN
    traced input against oracle/conv64.py with the bounds of tests/test_gpu_conv_fp8.py (no fake-quant chain: a rounding
    flip in an intermediate is not an error), every quantise launch bit for bit against the torch cast; detect() on a
    384 x 384 uint8 batch of 2 gives finite outputs and counts within the caps;
  * HIP graph: detect() with the mode on, captured once and replayed on a new input, equals eager execution bit for bit --
    its head and post-processing on a feature pyramid, and the whole call on a uint8 batch with S2A_OWN_CONV_ALWAYS=1;
  * weight cache: after weight.mul_(1.5) under no_grad, and after load_state_dict, the fp8 layer's output equals that of a
    twin layer built from the updated weight; a re-calibration with another scale changes the cache entry."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
CONV, QUANT, PACK = "s2a_conv3x3_pyramid_fp8", "s2a_quantize_e4m3", "s2a_conv_pack_weight_fp8"
SIZES = [(20, 28), (10, 14), (5, 7), (3, 4), (3, 3)]
PACKED = (("odm_cls", 15), ("odm_bbox", 5), ("or_feat", 256), ("pooled", 32), ("anchors", 5), ("fam_bbox", 5), ("fam_cls", 15),
          ("align", 256))


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


def make_model():
    from s2anet_amd.detector import build_synthetic_detector
    from s2anet_amd.fused import FusedConv2d
    model = build_synthetic_detector(device=DEV)
    g = torch.Generator().manual_seed(77)
    for seq in (model.head.fam_reg_ls, model.head.fam_cls_ls, model.head.odm_reg_ls, model.head.odm_cls_ls):
        for blk in seq:
            conv = blk[0]
            assert isinstance(conv, FusedConv2d)
            fan_in = conv.weight[0].numel()
            conv.weight.data.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            conv.bias.data.copy_(torch.randn(conv.bias.shape, generator=g) * 0.05)
    model.head.odm_cls_head.bias.data.fill_(-2.0)       # a score spread that leaves detections (as smoke() does)
    model.head.odm_cls_head.weight.data.mul_(20.0)
    return model


@pytest.fixture(scope="module")
def model():
    return make_model()


@pytest.fixture(scope="module")
def layout():
    from s2anet_amd.pyramid import PyramidLayout
    return PyramidLayout(2, SIZES, (8, 16, 32, 64, 128))


def features(layout, seed=3):
    return torch.randn(layout.pixels, 256, generator=torch.Generator().manual_seed(seed)).to(DEV).half()


@pytest.fixture
def calibrated(model, layout):
    """the module's model, calibrated on the test features and switched on; switched off again afterwards"""
    import s2anet_amd as S
    S.calibrate_fp8(model.head, [(layout, features(layout)), (layout, features(layout, 4))])
    S.fp8_towers(model.head)
    yield model
    S.fp8_towers(model.head, False)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t


def run(head, layout, x):
    tr = {}
    with torch.no_grad():
        head.forward_pyramid(layout, x, trace=tr)
    torch.cuda.synchronize()
    return tr


def test_enabling_before_calibration_raises():
    import s2anet_amd as S
    from s2anet_amd.detector import fuse_epilogues
    from s2anet_amd.head import S2ANetHead
    head = fuse_epilogues(S2ANetHead(num_classes=15).eval()).to(DEV).half()
    assert S.fp8.fp8_supported(head)
    with pytest.raises(RuntimeError, match="calibrate"):
        S.fp8_towers(head)
    assert head.fp8_enabled is False


def test_mode_off_calls_no_fp8_symbol_and_keeps_the_bits_of_a_twin(model, layout, counting):
    import s2anet_amd as S
    x = features(layout)
    twin_model = make_model()                               # never enabled, never calibrated
    twin = run(twin_model.head, layout, x)
    counting.calls.clear()
    scales = S.calibrate_fp8(model, [torch.randint(0, 256, (2, 3, 384, 384), dtype=torch.uint8, device=DEV)
                                     .contiguous(memory_format=torch.channels_last)])
    assert sorted(scales) == sorted(S.fp8.FP8_TENSORS) and all(0 < v < 1e4 for v in scales.values())
    S.calibrate_fp8(model.head, [(layout, x)])
    off = run(model.head, layout, x)
    assert not [n for n, _ in counting.calls if n in (CONV, QUANT, PACK)]
    S.fp8_towers(model)
    on = run(model.head, layout, x)
    assert counting.count(CONV) == 5
    S.fp8_towers(model, False)
    counting.calls.clear()
    back = run(model.head, layout, x)
    assert not [n for n, _ in counting.calls if n in (CONV, QUANT, PACK)]
    for k, cols in PACKED:
        for name, tr in (("calibrated, off", off), ("enabled then disabled", back)):
            assert torch.equal(bits(tr[k][:, :cols]), bits(twin[k][:, :cols])), (k, name)
    assert not torch.equal(bits(on["odm_bbox"][:, :5]), bits(twin["odm_bbox"][:, :5]))      # the route really differs
    assert not [k for k in off if k.startswith("fp8.")] and list(model.head.state_dict()) == list(twin_model.head.state_dict())


def test_mode_on_every_fp8_launch_against_float64_on_its_own_input(calibrated, layout, counting):
    from oracle.conv64 import conv64
    from s2anet_amd.fp8 import FP8_LAYERS, quantize_weight_e4m3
    head = calibrated.head
    sc = head.fp8_scales
    x = features(layout)
    counting.calls.clear()
    tr = run(head, layout, x)
    assert counting.count(CONV) == 5 and counting.count(QUANT) == 3
    # the three quantise launches, bit for bit: x (shared by both FAM towers), or_feat, the 32 -> 256 layer's output
    assert tr["fp8.fam_reg_ls.0.in"] is tr["fp8.fam_cls_ls.0.in"]
    for name, src, s in (("fam_reg_ls.0", tr["x"], sc["x"]), ("odm_reg_ls.0", tr["or_feat"], sc["or_feat"]),
                         ("odm_cls_ls.1", tr["odm_cls_ls0"], sc["odm_cls_ls0"])):
        want = (src.float().cpu() * (1.0 / s)).clamp(-448, 448).to(F8).view(torch.uint8)
        assert torch.equal(tr[f"fp8.{name}.in"].cpu(), want), name
    # odm_reg_ls[1] reads what odm_reg_ls[0] wrote: no quantise launch in between
    assert tr["fp8.odm_reg_ls.1.in"] is tr["fp8.odm_reg_ls.0.out"] and tr["fp8.odm_reg_ls.0.out"].dtype == torch.uint8
    layers = {"fam_reg_ls.0": (head.fam_reg_ls[0][0], "x", None), "fam_cls_ls.0": (head.fam_cls_ls[0][0], "x", None),
              "odm_reg_ls.0": (head.odm_reg_ls[0][0], "or_feat", "odm_reg_ls0"),
              "odm_reg_ls.1": (head.odm_reg_ls[1][0], "odm_reg_ls0", None),
              "odm_cls_ls.1": (head.odm_cls_ls[1][0], "odm_cls_ls0", None)}
    assert sorted(layers) == sorted(FP8_LAYERS)
    K = 9 * 256
    f32_term = 2 * (K + 3) * 2.0 ** -24
    for name, (conv, s_in, s_out) in layers.items():
        wq, s_w = quantize_weight_e4m3(conv.weight)
        scale = tr[f"fp8.{name}.scale"]
        assert torch.equal(scale, s_w * float(sc[s_in])), name
        xq, out = tr[f"fp8.{name}.in"], tr[f"fp8.{name}.out"]
        assert int(((xq & 0x7f) == 0x7f).sum()) == 0
        x64 = xq.cpu().view(F8).double()
        w64 = wq.cpu().view(F8).double() * scale.double().cpu().view(-1, 1, 1, 1)
        worst = 0.0
        for l in range(len(SIZES)):
            y, S = conv64(layout.level(x64, l), w64, conv.bias.double().cpu(), 1, 3, relu=True)
            if s_out is None:
                assert out.dtype == torch.float16
                err = (layout.level(out, l).cpu().double() - y).abs()
                bound = (2.0 ** -11 + f32_term) * S + 2.0 ** -25
            else:
                inv = float(torch.tensor(1.0 / sc[s_out], dtype=torch.float32))
                t = (y * inv).clamp(-448, 448)
                err = (layout.level(out, l).contiguous().cpu().view(F8).double() - t).abs()
                bound = 2.0 ** -4 * t.abs() + 2.0 ** -10 + f32_term * S * inv
            worst = max(worst, (err / bound).max().item())
            assert int((~(err <= bound)).sum()) == 0, (name, l, worst)
        print("fp8 head launch %s: max err/bound %.3g" % (name, worst))
        assert (out != 0).float().mean().item() > 0.2, name
    # the calibration saw these features: the quantised tensors use the top of the range and nothing is clipped away
    # (two batches of N(0, 1) features: their maxima are within a few per cent of each other)
    assert int(tr["fp8.fam_reg_ls.0.in"].cpu().view(F8).float().abs().max()) >= 320


def test_mode_on_detect_runs_with_finite_outputs(calibrated):
    imgs = torch.randint(0, 256, (2, 3, 384, 384), dtype=torch.uint8, device=DEV,
                         generator=torch.Generator(DEV).manual_seed(384)).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        dets, labels, counts = calibrated.detect(imgs)
    torch.cuda.synchronize()
    assert dets.shape == (2, 2000, 6) and labels.shape == (2, 2000) and counts.shape == (2,)
    assert bool(torch.isfinite(dets).all()) and int(counts.min()) >= 0 and int(counts.max()) <= calibrated.head.max_per_img
    for b in range(2):
        k = int(counts[b])
        assert bool((labels[b, :k] >= 0).all()) and bool((labels[b, :k] < 15).all()) and bool((labels[b, k:] == -1).all())


def test_mode_on_hip_graph_replay_equals_eager(calibrated, layout):
    head = calibrated.head
    feats = [features(layout, 20 + i) for i in range(2)]

    def go(x):
        return head.get_bboxes_batched(head.forward_pyramid(layout, x), max_candidates=50000, return_overflow=True)
    with torch.no_grad():
        eager = [tuple(t.clone() for t in go(x)) for x in feats]
        static_x = feats[0].clone()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # warm the side stream's workspaces before capturing on it
            go(static_x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_out = go(static_x)
        static_x.copy_(feats[1])
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(static_out, eager[1]):
            assert torch.equal(got, ref)
    assert int(eager[1][2].sum()) > 0 and not torch.equal(eager[0][0], eager[1][0])


def test_mode_on_whole_detect_hip_graph_replay_equals_eager(calibrated, monkeypatch):
    """the whole detect() (trunk included) on a uint8 batch in a static buffer; every convolution on the own kernels
    (S2A_OWN_CONV_ALWAYS=1: the library's small-grid convolutions do not repeat their bits from call to call)"""
    monkeypatch.setenv("S2A_OWN_CONV_ALWAYS", "1")
    g = torch.Generator().manual_seed(12)
    imgs = [torch.randint(0, 256, (2, 3, 384, 384), dtype=torch.uint8, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
            for _ in range(2)]
    with torch.no_grad():
        eager = [tuple(t.clone() for t in calibrated.detect(i)) for i in imgs]
        static_img = imgs[0].clone(memory_format=torch.channels_last)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            calibrated.detect(static_img)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = calibrated.detect(static_img)
        static_img.copy_(imgs[1])
        graph.replay()
        torch.cuda.synchronize()
        for got, ref, name in zip(out, eager[1], ("detections", "labels", "counts")):
            assert torch.equal(got, ref), name
    assert int(eager[1][2].min()) > 0 and not torch.equal(eager[0][0], eager[1][0])


def test_weight_cache_follows_updates_and_recalibration(calibrated, layout):
    import s2anet_amd as S
    from s2anet_amd import pyramid as P
    from s2anet_amd.fused import FusedConv2d
    head = calibrated.head
    conv = head.odm_reg_ls[1][0]
    x = features(layout)
    saved = {k: v.clone() for k, v in conv.state_dict().items()}
    scales = dict(head.fp8_scales)

    def twin_out(tr):
        t = FusedConv2d(256, 256, 3, padding=1, relu=True).to(DEV).half()
        t.load_state_dict(conv.state_dict())
        w, sc, b, o = t.packed_args_fp8(head.fp8_scales["odm_reg_ls0"])
        out = P.conv3x3_fp8(layout, tr["fp8.odm_reg_ls.1.in"], w, sc, b, o, relu=True)
        torch.cuda.synchronize()
        return out
    try:
        first = run(head, layout, x)
        assert torch.equal(bits(first["fp8.odm_reg_ls.1.out"]), bits(twin_out(first)))
        with torch.no_grad():
            conv.weight.mul_(1.5)
        second = run(head, layout, x)
        assert torch.equal(second["fp8.odm_reg_ls.1.in"], first["fp8.odm_reg_ls.1.in"])
        assert not torch.equal(bits(second["fp8.odm_reg_ls.1.out"]), bits(first["fp8.odm_reg_ls.1.out"]))
        assert torch.equal(bits(second["fp8.odm_reg_ls.1.out"]), bits(twin_out(second)))
        g = torch.Generator().manual_seed(9)
        conv.load_state_dict({"weight": (torch.randn(256, 256, 3, 3, generator=g) / 48).half(),
                              "bias": (torch.randn(256, generator=g) * 0.1).half()})
        third = run(head, layout, x)
        assert not torch.equal(bits(third["fp8.odm_reg_ls.1.out"]), bits(second["fp8.odm_reg_ls.1.out"]))
        assert torch.equal(bits(third["fp8.odm_reg_ls.1.out"]), bits(twin_out(third)))
        # re-calibration: another input scale of this layer -> another cache entry (its key holds the scale)
        entry = conv._packed.slots["fp8"]
        assert entry[3] == scales["odm_reg_ls0"]
        S.calibrate_fp8(head, None, scales=dict(scales, odm_reg_ls0=scales["odm_reg_ls0"] * 2))
        fourth = run(head, layout, x)
        entry2 = conv._packed.slots["fp8"]
        assert entry2 is not entry and entry2[3] == scales["odm_reg_ls0"] * 2
        assert torch.equal(fourth["fp8.odm_reg_ls.1.scale"], third["fp8.odm_reg_ls.1.scale"] * 2)
        assert torch.equal(bits(fourth["fp8.odm_reg_ls.1.out"]), bits(twin_out(fourth)))
        # drop_weight_caches forgets the entry; the next forward packs again, same bits
        S.drop_weight_caches(head)
        assert "fp8" not in conv._packed.slots
        assert torch.equal(bits(run(head, layout, x)["fp8.odm_reg_ls.1.out"]), bits(fourth["fp8.odm_reg_ls.1.out"]))
    finally:
        conv.load_state_dict(saved)
        S.calibrate_fp8(head, None, scales=scales)
