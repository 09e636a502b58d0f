"""GPU: every instantiation of the dense f16 convolution (k_conv_f16 behind s2a_conv_nhwc_f16), the pyramid-packed
launches and the fused trunk forms, called directly at the tile-edge geometries of tests/conv_geometry_cases.py and held
to the float64 reference of oracle/conv64.py.

Every case sets all four tile-shape switches, so the instantiation it runs is route(ksize, stride, C, O, switches) -- in
the test id -- whatever the tile-count thresholds say at these sizes.  Per launch:
  1. |got - y64| <= tau * S + 2^-25 elementwise and relative L2 error <= 2 u16 (conv_geometry_cases.compare; the bounds
     of tests/test_gpu_forward_shapes.py, K = taps * C);
  2. x, the residual and the coarse map are views into NaN-filled buffers (64 KiB of NaN on each side): a read outside
     the tensor is a NaN in the output, not a plausible zero;
  3. `out` is such a view too: afterwards every element of the view is written and every band element is still NaN;
  4. a second call into a freshly NaN-filled `out` gives the same bits;
  5. behind a ReLU more than 20 % of the outputs are nonzero.
Fused launches are checked stage by stage from the f16 values the kernel rounded to at that stage, and against the
separate launches bit for bit where the code claims it; tile shapes of one layer give equal bits where it claims that.

Set S2A_CONV_GEOMETRY_REPORT=<path> to write the worst ratios (error over bound) per instantiation and fused form as
JSON; the committed run is profiles/conv_geometry_ratios.json (1 944 comparisons, all inside their bounds).  The largest
elementwise ratio per family in that run, the largest relative-L2 ratio in brackets: 3x3 stride 1 0.49 [0.31], 3x3 stride 2
0.37 [0.30], 1x1 0.77 [0.31], pyramid launches 0.74 [0.28], bottleneck_tail 0.80 [0.29], s2a_conv1x1_chain_f16 0.50 [0.29],
conv1x1_add_up2 0.59 [0.30].  The planted defects this file was run against are listed in docs/HISTORY.md."""
import json
import os

import pytest
import torch

import conv_geometry_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {}
BIAS_RELU, PLAIN, BIAS_RES_RELU, RES = G.EPILOGUES


def note(key, case_id, m):
    """keep the worst ratios per key; returns m["ok"]"""
    r = REPORT.setdefault(key, dict(ratio=0.0, ratio_case=None, l2_ratio=0.0, l2_case=None, comparisons=0))
    r["comparisons"] += 1
    if m["ratio"] >= r["ratio"]:
        r["ratio"], r["ratio_case"] = m["ratio"], case_id
    if m["l2_ratio"] >= r["l2_ratio"]:
        r["l2_ratio"], r["l2_case"] = m["l2_ratio"], case_id
    print("%-34s %-52s ratio %.3f  l2/bound %.3f  nonzero %.2f" % (key, case_id, m["ratio"], m["l2_ratio"], m["nonzero"]))
    path = os.environ.get("S2A_CONV_GEOMETRY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(sorted(REPORT.items())), f, indent=1)
    return m["ok"]


def set_switches(monkeypatch, sw):
    assert set(sw) == set(G.SWITCHES)
    for k, v in sw.items():
        monkeypatch.setenv(k, v)
    for k in ("S2A_CONV_OG", "S2A_CONV_NARROW", "S2A_CONV_NARROW_WGS"):
        monkeypatch.delenv(k, raising=False)


def on_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def finished(*guards):
    """after the launches: synchronised; inputs' and outputs' bands untouched"""
    torch.cuda.synchronize()
    for g in guards:
        assert g.bands_untouched(), "a NaN band around a tensor was written"


def launch(c, epi, gx, gr, wp, bias, written=True):
    """conv_f16 into a fresh guarded `out` -> the f16 result [B,O,Ho,Wo] (a copy), every element written (checked
    unless the input itself holds a NaN), bands NaN"""
    from s2anet_amd.fused import conv_f16
    Ho, Wo = G.out_hw(c["H"], c["W"], c["s"])
    go = G.Guarded((c["B"], Ho, Wo, c["O"]), DEV)
    r = conv_f16(G.nchw(gx.t), wp, bias if epi["bias"] else None, c["O"], c["k"], c["s"], epi["relu"],
                 G.nchw(gr.t) if epi["res"] else None, out=G.nchw(go.t))
    assert r.data_ptr() == go.t.data_ptr()
    finished(go)
    assert go.all_written() or not written, "an output element was not written"
    return G.nchw(go.t.clone())


# ----------------------------------------------------------------------------- the fourteen instantiations
@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["id"])
def test_instantiation(c, monkeypatch):
    from s2anet_amd.fused import conv_pack_weight
    set_switches(monkeypatch, c["sw"])
    inp = on_dev(G.make_inputs(c))
    gx, gr = G.Guarded(inp["x"], DEV), G.Guarded(inp["res"], DEV)
    seen = dict(x=gx.t, w=inp["w"], bias=inp["bias"], res=gr.t)
    wp = conv_pack_weight(inp["w"])
    bad = []
    for e in c["epis"]:
        epi = G.EPILOGUES[e]
        got = launch(c, epi, gx, gr, wp, inp["bias"])
        again = launch(c, epi, gx, gr, wp, inp["bias"])
        assert torch.equal(again, got), (epi["name"], "the second launch gives other bits")
        y, S = G.reference(c, seen, epi)
        m = G.compare(got, y, S, G.kind_of(epi), c["K"])
        if not note(G.inst_name(c["inst"]), c["id"] + ":" + epi["name"], m):
            bad.append((epi["name"], m))
        if epi["relu"]:
            assert m["nonzero"] > 0.2, (epi["name"], m["nonzero"])
    finished(gx, gr)
    assert not bad, (c["id"], bad)


C32_CASES = tuple(c for c in G.CASES if c["C"] == 32 and c["grid_x"] > 1)


@pytest.mark.parametrize("c", C32_CASES, ids=lambda c: c["id"])
def test_c32_reads_no_neighbouring_channels(c, monkeypatch):
    """C = 32 fills half a chunk (qlim = C / 8), and the filter's other half is zero: a kernel that read 64 channels
    would fetch the next pixel's values and multiply them by zero -- invisible on finite data.  One NaN pixel shows it:
    the outputs that are NaN must be exactly those whose window holds that pixel."""
    from s2anet_amd.fused import conv_pack_weight
    set_switches(monkeypatch, c["sw"])
    inp = on_dev(G.make_inputs(c))
    B, H, W, k, s = c["B"], c["H"], c["W"], c["k"], c["s"]
    Ho, Wo = G.out_hw(H, W, s)
    py, px = min(H - 1, 2 * s), min(W - 1, 4 * s)
    inp["x"][B - 1, py, px, :] = G.NAN
    gx, gr = G.Guarded(inp["x"], DEV), G.Guarded(inp["res"], DEV)
    got = launch(c, PLAIN, gx, gr, conv_pack_weight(inp["w"]), inp["bias"], written=False)
    pad = (k - 1) // 2
    oy, ox = torch.arange(Ho, device=DEV).view(-1, 1) * s, torch.arange(Wo, device=DEV).view(1, -1) * s
    want = torch.zeros((B, c["O"], Ho, Wo), dtype=torch.bool, device=DEV)
    want[B - 1] = ((oy - py).abs() <= pad) & ((ox - px).abs() <= pad)
    assert bool(want.any()) and torch.equal(got.isnan(), want)


# ----------------------------------------------------------------------------- tile shapes of one layer: equal bits
def _dedup(seq):
    return tuple(dict.fromkeys(seq))


BITS_3X3 = tuple((C, O, g) for C, O in ((192, 320), (128, 384), (192, 512))
                 for g in _dedup(G.geoms_3x3(4) + G.geoms_3x3(8) + G.geoms_3x3(16)))
BITS_1X1 = tuple((s, g) for s in (1, 2) for g in _dedup(G.geoms_1x1(64, s) + G.geoms_1x1(128, s)))


def _bits_inputs(tag, B, H, W, C, O, k, s):
    Ho, Wo = G.out_hw(H, W, s)
    inp = on_dev(G.draw(G._gen(tag), B, H, W, C, O, k, Ho, Wo))
    return inp, G.Guarded(inp["x"], DEV), G.Guarded(inp["res"], DEV)


@pytest.mark.parametrize("C,O,g", BITS_3X3, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_3x3_tile_shapes_give_equal_bits(C, O, g, monkeypatch):
    """4 x 16, 8 x 16 and 16 x 16 (filter through LDS) tiles of one 3x3 / stride 1 layer: the same bits, with and
    without a residual (the claims of test_narrow_conv3x3_filter_through_lds_matches,
    test_conv3x3_wide_layer_filter_through_lds_matches and test_conv3x3_half_tiles_match at the edge geometries)"""
    from s2anet_amd.fused import conv_pack_weight
    B, H, W = g
    inp, gx, gr = _bits_inputs("bits3-%d-%d-%s" % (C, O, g), B, H, W, C, O, 3, 1)
    wp = conv_pack_weight(inp["w"])
    og = G.og_of(O)
    forms = [G.switches()]
    forms.append(G.switches(ph=2) if og == 4 else G.switches(ph_narrow=2))
    if og >= 2:
        forms.append(G.switches(half3=1))
    outs = {}
    for sw in forms:
        set_switches(monkeypatch, sw)
        inst = G.route(3, 1, C, O, sw)
        c = dict(B=B, H=H, W=W, s=1, k=3, O=O)
        outs[inst] = [launch(c, epi, gx, gr, wp, inp["bias"]) for epi in (BIAS_RELU, BIAS_RES_RELU, RES)]
    assert len(outs) == len(forms)
    first = next(iter(outs.values()))
    for inst, o in outs.items():
        assert all(torch.equal(a, b) for a, b in zip(o, first)), (inst, "differs from", next(iter(outs)))


@pytest.mark.parametrize("s,g", BITS_1X1, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "s%d" % v)
def test_1x1_tile_shapes_give_equal_bits(s, g, monkeypatch):
    """64- and 128-position tiles of a full-width 1x1 (test_conv1x1_half_tiles_match at the edge geometries)"""
    from s2anet_amd.fused import conv_pack_weight
    B, H, W = g
    C, O = 192, 512
    inp, gx, gr = _bits_inputs("bits1-%d-%s" % (s, g), B, H, W, C, O, 1, s)
    wp = conv_pack_weight(inp["w"])
    outs = []
    for half in (0, 1):
        set_switches(monkeypatch, G.switches(half1=half))
        c = dict(B=B, H=H, W=W, s=s, k=1, O=O)
        outs.append([launch(c, epi, gx, gr, wp, inp["bias"]) for epi in (PLAIN, BIAS_RES_RELU)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ----------------------------------------------------------------------------- pyramid-packed launches
class GuardedLayout:
    """a PyramidLayout whose new() hands out guarded NaN-filled buffers (the wrappers allocate their outputs with it)"""

    def __init__(self, B, levels):
        from s2anet_amd.pyramid import PyramidLayout
        self.layout = PyramidLayout(B, levels, [8.0 * 2 ** i for i in range(len(levels))])
        self.made = []
        self.layout.new = self.new

    def new(self, channels, device, dtype=torch.float16):
        assert dtype == torch.float16
        g = G.Guarded((self.layout.pixels, channels), device)
        self.made.append(g)
        return g.t

    def take(self):
        made, self.made = self.made, []
        return made


def pyramid_instantiation(C, O, ph):
    og = G.og_of(O)
    return (9, og, 2 if (ph == 2 and og == 4 and C % 64 == 0) else 1, 1, 0)


def ph_values(O):
    return (1, 2) if O == 256 else (1,)


def per_level(key, cid, layout, got, y_of_level, kind, K, channels=None):
    """every level of a packed result through the comparator -> the list of failures"""
    bad = []
    for l in range(len(layout.sizes)):
        y, S = y_of_level(l)
        m = G.compare(layout.level(got, l, channels), y, S, kind, K)
        if not note(key, "%s:level%d" % (cid, l), m):
            bad.append((l, m))
    return bad


@pytest.mark.parametrize("pc", G.pyramid_cases(G.PYRAMID_CONV_PAIRS), ids=lambda pc: pc["id"])
def test_pyramid_conv3x3(pc, monkeypatch):
    from oracle.conv64 import conv64
    from s2anet_amd import pyramid as P
    from s2anet_amd.fused import conv_pack_weight
    B, C, O = pc["B"], pc["C"], pc["O"]
    gl = GuardedLayout(B, pc["levels"])
    lay = gl.layout
    inp = on_dev(G.pyramid_inputs(pc["id"], pc["levels"], B, C, O))
    gx, gr = G.Guarded(inp["x"], DEV), G.Guarded(inp["res"], DEV)
    wp = conv_pack_weight(inp["w"])
    bad, bits = [], {}
    for ph in ph_values(O):
        set_switches(monkeypatch, G.switches(ph=ph))
        key = "pyramid.conv3x3:" + G.inst_name(pyramid_instantiation(C, O, ph))
        for epi in (BIAS_RELU, RES):
            outs = []
            for rep in range(2):
                go = G.Guarded((lay.pixels, O), DEV)
                P.conv3x3(lay, gx.t, wp, inp["bias"] if epi["bias"] else None, O, epi["relu"],
                          residual=gr.t if epi["res"] else None, out=go.t)
                finished(go)
                assert go.all_written(), "an output element was not written"
                outs.append(go.t.clone())
            assert torch.equal(outs[0], outs[1])
            bits.setdefault(epi["name"], []).append(outs[0])
            bad += per_level(key, "%s:%s" % (pc["id"], epi["name"]), lay, outs[0],
                             lambda l: conv64(lay.level(gx.t, l), inp["w"], inp["bias"] if epi["bias"] else None, 1, 3,
                                              residual=lay.level(gr.t, l) if epi["res"] else None, relu=epi["relu"]),
                             G.kind_of(epi), 9 * C)
            if epi["relu"]:
                assert (outs[0] != 0).double().mean().item() > 0.2
    finished(gx, gr)
    assert all(torch.equal(v[0], o) for v in bits.values() for o in v), "S2A_CONV_PH=1 and 2 give different bits"
    assert not bad, (pc["id"], bad)


@pytest.mark.parametrize("pc", G.pyramid_cases(G.PYRAMID_POOL_PAIRS), ids=lambda pc: pc["id"])
def test_pyramid_orconv_pool(pc, monkeypatch):
    """out within the conv bound; pooled equal to rot_pool64 of the float64 conv within the same bound, and equal bit for
    bit to the max over runs of eight of the kernel's own out"""
    from oracle.conv64 import conv64, rot_pool64
    from s2anet_amd import pyramid as P
    from s2anet_amd.fused import conv_pack_weight
    B, C, O = pc["B"], pc["C"], pc["O"]
    gl = GuardedLayout(B, pc["levels"])
    lay = gl.layout
    inp = on_dev(G.pyramid_inputs("pool-" + pc["id"], pc["levels"], B, C, O))
    gx = G.Guarded(inp["x"], DEV)
    wp = conv_pack_weight(inp["w"])
    bad, bits = [], []
    for ph in ph_values(O):
        set_switches(monkeypatch, G.switches(ph=ph))
        key = "pyramid.orconv_pool:" + G.inst_name(pyramid_instantiation(C, O, ph))
        runs = []
        for rep in range(2):
            out, pooled = P.orconv_pool(lay, gx.t, wp, inp["bias"], O)
            made = gl.take()
            assert len(made) == 2 and made[0].t.data_ptr() == out.data_ptr() and made[1].t.data_ptr() == pooled.data_ptr()
            finished(*made)
            assert made[0].all_written() and made[1].all_written(), "an output element was not written"
            runs.append((out.clone(), pooled.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        out, pooled = runs[0]
        assert torch.equal(pooled, out.view(lay.pixels, O // 8, 8).amax(-1))
        bits.append(runs[0])
        refs = [conv64(lay.level(gx.t, l), inp["w"], inp["bias"], 1, 3) for l in range(len(lay.sizes))]
        bad += per_level(key, pc["id"] + ":out", lay, out, lambda l: refs[l], "conv", 9 * C)
        bad += per_level(key, pc["id"] + ":pooled", lay, pooled, lambda l: rot_pool64(*refs[l]), "conv", 9 * C)
    finished(gx)
    assert all(torch.equal(a, b) for r in bits for a, b in zip(r, bits[0])), "S2A_CONV_PH=1 and 2 give different bits"
    assert not bad, (pc["id"], bad)


HEAD_CASES = tuple(dict(id="%s-b%d-c%dh%d" % (name, B, C, nh), levels=G.PYRAMIDS[name], B=B, C=C, nh=nh)
                   for name in G.PYRAMIDS for B in G.PYRAMID_BATCHES for C, nh in G.PYRAMID_HEAD_CHANNELS)


@pytest.mark.parametrize("pc", HEAD_CASES, ids=lambda pc: pc["id"])
def test_pyramid_conv3x3_head(pc, monkeypatch):
    """tower + 1x1 head in one launch: the tower held to float64, the head to conv64 of the kernel's own f16 tower
    values (keep_tower=True); keep_tower=False gives the same head bits"""
    from oracle.conv64 import conv64
    from s2anet_amd import pyramid as P
    from s2anet_amd.fused import conv_pack_weight
    B, C, nh, O = pc["B"], pc["C"], pc["nh"], 256
    gl = GuardedLayout(B, pc["levels"])
    lay = gl.layout
    inp = on_dev(G.pyramid_inputs("head-" + pc["id"], pc["levels"], B, C, O,
                                  extra=(("hw", (nh, O, 1, 1), 1.0 / 16), ("hb", (nh,), 1.0))))
    gx = G.Guarded(inp["x"], DEV)
    wp, hwp = conv_pack_weight(inp["w"]), conv_pack_weight(inp["hw"])
    hb = torch.cat([inp["hb"], inp["hb"].new_zeros(64 - nh)])
    bad, bits = [], []
    for ph in (1, 2):
        set_switches(monkeypatch, G.switches(ph=ph))
        key = "pyramid.conv3x3_head:" + G.inst_name(pyramid_instantiation(C, O, ph))
        runs = []
        for rep in range(2):
            head, tower = P.conv3x3_head(lay, gx.t, wp, inp["bias"], O, hwp, hb, relu=True, keep_tower=True)
            made = gl.take()
            assert len(made) == 2 and made[0].t.data_ptr() == head.data_ptr() and made[1].t.data_ptr() == tower.data_ptr()
            finished(*made)
            assert made[1].all_written() and not bool(head[:, :32].isnan().any()), "an output element was not written"
            runs.append((head[:, :32].clone(), tower.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        head, tower = runs[0]
        only = P.conv3x3_head(lay, gx.t, wp, inp["bias"], O, hwp, hb, relu=True)
        finished(*gl.take())
        assert torch.equal(only[:, :32], head), "keep_tower=False gives other head bits"
        assert bool((head[:, nh:] == 0).all())
        assert (tower != 0).double().mean().item() > 0.2
        bits.append(runs[0])
        bad += per_level(key, pc["id"] + ":tower", lay, tower,
                         lambda l: conv64(lay.level(gx.t, l), inp["w"], inp["bias"], 1, 3, relu=True), "conv", 9 * C)
        bad += per_level(key, pc["id"] + ":head", lay, head,
                         lambda l: conv64(lay.level(tower, l), inp["hw"], inp["hb"], 1, 1), "conv", O, channels=nh)
    finished(gx)
    assert all(torch.equal(a, b) for r in bits for a, b in zip(r, bits[0])), "S2A_CONV_PH=1 and 2 give different bits"
    assert not bad, (pc["id"], bad)


# ----------------------------------------------------------------------------- fused trunk forms
@pytest.fixture(scope="module")
def tail_layers():
    """conv2 (3x3, 64 -> 64), conv3 (1x1, 64 -> 256) and the next block's conv1 with 64 and with 128 maps"""
    from s2anet_amd.fused import FusedConv2d
    gen = G._gen("tail-layers")

    def layer(C, O, k):
        m = FusedConv2d(C, O, k, padding=(k - 1) // 2, relu=True)
        with torch.no_grad():
            m.weight.copy_(torch.randn(m.weight.shape, generator=gen) / (k * k * C) ** 0.5)
            m.bias.copy_(torch.randn(m.bias.shape, generator=gen))
        return m.to(DEV).half().requires_grad_(False)
    return dict(conv2=layer(64, 64, 3), conv3=layer(64, 256, 1), chain={64: layer(256, 64, 1), 128: layer(256, 128, 1)})


def tail_entry(x, c2, c3, res, chain, B, H, W):
    """s2a_conv3x3_tail1x1_f16 itself into guarded outputs -> (Guarded out, Guarded chain_out | None)"""
    from s2anet_amd import _lib
    w2, b2, _ = c2.packed_args()
    w3, b3, _ = c3.packed_args()
    wc = bc = gn = None
    go = G.Guarded((B, H, W, 256), DEV)
    if chain is not None:
        wc, bc, _ = chain.packed_args()
        gn = G.Guarded((B, H, W, chain.out_channels), DEV)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().s2a_conv3x3_tail1x1_f16(
            _lib.ptr(x), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(w3), _lib.ptr(b3), _lib.ptr(res), _lib.ptr(go.t),
            _lib.ptr(None if gn is None else wc), _lib.ptr(bc), _lib.ptr(None if gn is None else gn.t),
            0 if chain is None else chain.out_channels, B, 64, 64, 256, H, W, _lib.stream_ptr(x.device)))
    return go, gn


@pytest.mark.parametrize("B", G.TAIL_BATCHES)
@pytest.mark.parametrize("H,W", G.TAIL_SIZES)
def test_bottleneck_tail(H, W, B, tail_layers, monkeypatch):
    """s2a_conv3x3_tail1x1_f16 stage by stage: the 64-map intermediate is the separate 3x3 launch (bit identity with the
    two launches asserted), the tail against conv64 (1x1) of it plus the residual, the chained conv1 against conv64 of
    the tail's own output; 8 x 16 and 16 x 16 tiles give the same bits"""
    from oracle.conv64 import conv64
    from s2anet_amd.fused import bottleneck_tail, conv_f16
    c2, c3 = tail_layers["conv2"], tail_layers["conv3"]
    cid = "b%dx%dx%d" % (B, H, W)
    d = on_dev(G.draw(G._gen("tail-" + cid), B, H, W, 64, 256, 1, H, W))
    gx, gr = G.Guarded(d["x"], DEV), G.Guarded(d["res"], DEV)
    x, bad = G.nchw(gx.t), []
    for with_res, nchain in G.TAIL_FORMS:
        res = G.nchw(gr.t) if with_res else None
        chain = None if nchain is None else tail_layers["chain"][nchain]
        form = "%s:res%d:chain%s" % (cid, with_res, nchain)
        bits = []
        for ph in (1, 2):
            set_switches(monkeypatch, G.switches(ph_narrow=ph))
            key = "bottleneck_tail:ph%d" % ph
            r = bottleneck_tail(x, c2, c3, res, chain)
            out, nxt = (r, None) if chain is None else r
            go, gn = tail_entry(x, c2, c3, res, chain, B, H, W)
            finished(go, *([] if gn is None else [gn]))
            assert go.all_written() and torch.equal(G.nchw(go.t), out), "the second launch gives other bits"
            if chain is not None:
                assert gn.all_written() and torch.equal(G.nchw(gn.t), nxt), "the second launch gives other chain bits"
            w2, b2, _ = c2.packed_args()
            w3, b3, _ = c3.packed_args()
            mid = conv_f16(x, w2, b2, 64, 3, 1, True)
            assert torch.equal(out, conv_f16(mid, w3, b3, 256, 1, 1, True, res)), "tail differs from the two launches"
            y, S = conv64(x, c2.weight, c2.bias, 1, 3, relu=True)
            ok = note(key + ":mid", form, G.compare(mid, y, S, "conv", 9 * 64))
            y, S = conv64(mid, c3.weight, c3.bias, 1, 1, residual=res, relu=True)
            ok &= note(key + ":tail", form, G.compare(out, y, S, "conv_res" if with_res else "conv", 64))
            assert (mid != 0).double().mean().item() > 0.2 and (out != 0).double().mean().item() > 0.2
            if chain is not None:
                wc, bc, _ = chain.packed_args()
                assert torch.equal(nxt, conv_f16(out, wc, bc, nchain, 1, 1, True)), "chain differs from the separate conv1"
                y, S = conv64(out, chain.weight, chain.bias, 1, 1, relu=True)
                ok &= note(key + ":chain", form, G.compare(nxt, y, S, "conv", 256))
                assert (nxt != 0).double().mean().item() > 0.2
            if not ok:
                bad.append((form, ph))
            bits.append((out, nxt))
        assert torch.equal(bits[0][0], bits[1][0]) and (chain is None or torch.equal(bits[0][1], bits[1][1])), \
            "S2A_CONV_PH_NARROW=1 and 2 give different bits"
    finished(gx, gr)
    assert not bad, bad


@pytest.mark.parametrize("g", G.CHAIN_GEOMS, ids=lambda g: "b%dx%dx%d" % g)
@pytest.mark.parametrize("K,O,O3", G.CHAIN_SHAPES)
def test_conv1x1_chain(K, O, O3, g, monkeypatch):
    """s2a_conv1x1_chain_f16 called directly: out and chain_out against float64 (the chain on the kernel's own out), equal
    to the stand-alone launches bit for bit"""
    from oracle.conv64 import conv64
    from s2anet_amd import _lib
    from s2anet_amd.fused import conv_f16, conv_pack_weight
    B, H, W = g
    cid = "k%do%do%d-b%dx%dx%d" % (K, O, O3, B, H, W)
    set_switches(monkeypatch, G.switches())
    gen = G._gen("chain-" + cid)
    d = on_dev(G.draw(gen, B, H, W, K, O, 1, H, W))
    dc = on_dev(G.draw(gen, 1, 1, 1, O, O3, 1, 1, 1))
    gx, gr = G.Guarded(d["x"], DEV), G.Guarded(d["res"], DEV)
    x = G.nchw(gx.t)
    p3, pc = conv_pack_weight(d["w"]), conv_pack_weight(dc["w"])
    bad = []
    for with_res in (False, True):
        res = G.nchw(gr.t) if with_res else None
        runs = []
        for rep in range(2):
            go, gn = G.Guarded((B, H, W, O), DEV), G.Guarded((B, H, W, O3), DEV)
            with torch.cuda.device(x.device):
                _lib.check(_lib.lib().s2a_conv1x1_chain_f16(_lib.ptr(x), _lib.ptr(p3), _lib.ptr(d["bias"]), _lib.ptr(res),
                                                            _lib.ptr(go.t), _lib.ptr(pc), _lib.ptr(dc["bias"]), _lib.ptr(gn.t),
                                                            O3, B, K, O, H, W, _lib.stream_ptr(x.device)))
            finished(go, gn)
            assert go.all_written() and gn.all_written(), "an output element was not written"
            runs.append((G.nchw(go.t.clone()), G.nchw(gn.t.clone())))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        out, nxt = runs[0]
        alone = conv_f16(x, p3, d["bias"], O, 1, 1, True, res)
        assert torch.equal(out, alone) and torch.equal(nxt, conv_f16(alone, pc, dc["bias"], O3, 1, 1, True))
        form = "%s:res%d" % (cid, with_res)
        y, S = conv64(x, d["w"], d["bias"], 1, 1, residual=res, relu=True)
        ok = note("conv1x1_chain:out", form, G.compare(out, y, S, "conv_res" if with_res else "conv", K))
        y, S = conv64(out, dc["w"], dc["bias"], 1, 1, relu=True)
        ok &= note("conv1x1_chain:chain", form, G.compare(nxt, y, S, "conv", O))
        assert (out != 0).double().mean().item() > 0.2 and (nxt != 0).double().mean().item() > 0.2
        if not ok:
            bad.append(form)
    finished(gx, gr)
    assert not bad, bad


@pytest.mark.parametrize("B", G.UP2_BATCHES)
@pytest.mark.parametrize("C,O", G.UP2_CHANNELS)
@pytest.mark.parametrize("H,W", G.UP2_SIZES)
def test_conv1x1_add_up2(H, W, C, O, B):
    """the FPN top-down step: conv1x1(x) + bias + the coarse map through a nearest 2x up-sampling, the coarse map inside
    NaN bands like a residual"""
    from oracle.conv64 import conv64
    from s2anet_amd import _lib
    from s2anet_amd.fused import conv1x1_add_up2, conv_pack_weight
    cid = "c%do%d-b%dx%dx%d" % (C, O, B, H, W)
    d = on_dev(G.draw(G._gen("up2-" + cid), B, H, W, C, O, 1, H // 2, W // 2))
    gx, gc = G.Guarded(d["x"], DEV), G.Guarded(d["res"], DEV)
    x, coarse = G.nchw(gx.t), G.nchw(gc.t)
    wp = conv_pack_weight(d["w"])
    got = conv1x1_add_up2(x, wp, d["bias"], coarse, O)
    go = G.Guarded((B, H, W, O), DEV)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().s2a_conv1x1_add_up2_f16(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(d["bias"]), _lib.ptr(coarse),
                                                      _lib.ptr(go.t), B, C, H, W, O, _lib.stream_ptr(x.device)))
    finished(go, gx, gc)
    assert go.all_written() and torch.equal(G.nchw(go.t), got), "the second launch gives other bits"
    y, S = conv64(x, d["w"], d["bias"], 1, 1, residual=coarse, residual_up2=True)
    m = G.compare(got, y, S, "conv_res", C)
    assert note("conv1x1_add_up2:" + G.inst_name((1, G.og_of(O), 1, 1, 0)), cid, m), (cid, m)
