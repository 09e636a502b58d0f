"""The dense-convolution case table (tests/conv_geometry_cases.py) checked without a GPU: the float64 reference against
torch's own float64 convolution, the bound against an emulation of the kernel's arithmetic, what the table reaches, the
shapes the entry point refuses, and route() -- the table's statement of which instantiation a call launches -- against the
library's own answer (s2a_conv_nhwc_f16_form): with the switches of every case, with none at the default thresholds, and
over the values a switch can be set to."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_geometry_cases as G


@pytest.fixture(scope="module")
def walked():
    """every case under every epilogue it runs: conv64 against conv2d, the emulation against the bound -- computed once"""
    rows = []
    for c in G.CASES:
        inp = G.make_inputs(c)
        x64, w64 = G.nchw(inp["x"]).double(), inp["w"].double()
        plain = F.conv2d(x64, w64, None, c["s"], (c["k"] - 1) // 2)
        for e in c["epis"]:
            epi = G.EPILOGUES[e]
            y, S = G.reference(c, inp, epi)
            want = plain
            if epi["bias"]:
                want = want + inp["bias"].double().view(1, -1, 1, 1)
            if epi["res"]:
                want = want + G.nchw(inp["res"]).double()
            if epi["relu"]:
                want = want.clamp_min(0)
            scale = max(want.abs().max().item(), 1.0)
            m = G.compare(G.emulate(c, inp, epi), y, S, G.kind_of(epi), c["K"])
            rows.append(dict(case=c["id"], epi=epi, ref_err=(y - want).abs().max().item() / scale,
                             S_min=(S - y.abs()).min().item(), m=m))
    return rows


def test_bounds_restate_the_forward_shapes_formulas():
    from test_gpu_forward_shapes import L2_CONV, TINY, tau
    assert G.TINY == TINY and G.L2_BOUND == L2_CONV
    for K in sorted({c["K"] for c in G.CASES} | {64, 256, 9 * 32, 9 * 64, 9 * 256, 128, 192, 512, 1024}):
        for kind in ("conv", "conv_res"):
            assert G.tau(kind, K) == tau(kind, K), (kind, K)


def test_conv64_agrees_with_torch_float64(walked):
    """conv64 (per-tap matmuls) against torch.nn.functional.conv2d in float64 with the bias, the residual and ReLU added
    by hand, to 1e-12 relative, for every case and epilogue; S dominates |y|"""
    assert len(walked) >= len(G.CASES)
    for r in walked:
        assert r["ref_err"] <= 1e-12, (r["case"], r["epi"]["name"], r["ref_err"])
        assert r["S_min"] >= -1e-12, (r["case"], r["epi"]["name"])


def test_conv64_up2_residual_agrees_with_torch_float64():
    """the nearest-2x coarse map of conv1x1_add_up2, added by hand"""
    from oracle.conv64 import conv64
    for (H, W) in G.UP2_SIZES:
        for (C, O) in G.UP2_CHANNELS:
            d = G.draw(G._gen("up2-cpu-%dx%d-%d-%d" % (H, W, C, O)), 3, H, W, C, O, 1, H // 2, W // 2)
            y, S = conv64(G.nchw(d["x"]), d["w"], d["bias"], 1, 1, residual=G.nchw(d["res"]), residual_up2=True)
            up = F.interpolate(G.nchw(d["res"]).double(), scale_factor=2, mode="nearest")
            want = F.conv2d(G.nchw(d["x"]).double(), d["w"].double(), d["bias"].double()) + up
            assert (y - want).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)
            assert bool((S >= y.abs() - 1e-12).all())


def test_emulated_kernel_arithmetic_stays_inside_the_bounds(walked):
    """f16 operands, f32 convolution, bias in f32, one f16 rounding (two behind a residual): inside the elementwise and
    the L2 bound for every case, and more than 20 % of the outputs behind a ReLU are nonzero.
    Worst ratios of the emulation over the table (error over bound): elementwise 0.77 (conv) / 0.61 (conv_res),
    relative L2 0.24 (conv) / 0.31 (conv_res) of 2 u16 -- the bound leaves a factor of about 1.3 elementwise (a single
    rounding can use all of u16) and of 3 in L2."""
    worst = {}
    for r in walked:
        kind = G.kind_of(r["epi"])
        w = worst.setdefault(kind, [0.0, 0.0])
        w[0], w[1] = max(w[0], r["m"]["ratio"]), max(w[1], r["m"]["l2_ratio"])
        assert r["m"]["ok"], (r["case"], r["epi"]["name"], r["m"])
        if r["epi"]["relu"]:
            assert r["m"]["nonzero"] > 0.2, (r["case"], r["epi"]["name"], r["m"]["nonzero"])
    print("worst emulation ratios (elementwise, l2):", {k: [round(v, 3) for v in w] for k, w in worst.items()})
    assert set(worst) == {"conv", "conv_res"}


def test_table_reaches_every_instantiation_and_tile_count():
    listed = {(9, 4, 1, 2, 0), (9, 2, 1, 2, 0), (9, 2, 2, 1, 0), (9, 1, 2, 1, 0), (9, 4, 2, 1, 0), (9, 4, 1, 1, 1),
              (9, 2, 1, 1, 1), (9, 4, 1, 1, 0), (9, 2, 1, 1, 0), (9, 1, 1, 1, 0), (1, 4, 1, 2, 0), (1, 4, 1, 1, 0),
              (1, 2, 1, 1, 0), (1, 1, 1, 1, 0)}
    assert len(listed) == 14 and set(G.ALL_INSTANTIATIONS) == listed
    reached = {}
    for c in G.CASES:
        assert G.route(c["k"], c["s"], c["C"], c["O"], c["sw"]) == c["inst"]
        assert set(c["sw"]) == set(G.SWITCHES)
        reached.setdefault(c["inst"], []).append(c)
    assert set(reached) == listed
    assert {c["grid_x"] for c in G.CASES} >= set(G.GRID_X_WANTED)
    for inst, cs in reached.items():
        # every (C, O) pair of an instantiation at two launches or more; every epilogue; blockIdx.y > 0; B = 1 and 3
        pairs = {}
        for c in cs:
            pairs[(c["C"], c["O"])] = pairs.get((c["C"], c["O"]), 0) + 1
        assert min(pairs.values()) >= 2, (inst, pairs)
        assert {e for c in cs for e in c["epis"]} == set(range(len(G.EPILOGUES))), inst
        assert any(c["O"] > 64 * inst[1] for c in cs), inst
        assert {c["B"] for c in cs} >= {1, 3}, inst
        needs64 = inst[2] == 2
        assert {c["C"] for c in cs} == set(G.CHANNELS) - ({32} if needs64 else set()), inst
        if inst[0] == 1:
            assert {c["s"] for c in cs} == {1, 2}, inst
    assert {c["O"] for c in G.CASES} == {64, 128, 256, 320, 384, 512}
    assert len({c["id"] for c in G.CASES}) == len(G.CASES)
    print("cases %d, launches per pass %d" % (len(G.CASES), sum(len(c["epis"]) for c in G.CASES)))


def test_tile_geometry_of_the_table():
    """the geometries sit where they are meant to: exactly one tile, one past it, and the counted grids"""
    for spec in G.INSTANTIATIONS:
        inst, s = spec["inst"], spec["strides"][0]
        (one, past) = G.pair_geoms(inst)
        assert G.grid_x(inst, *one, s) == 1, inst
        assert G.grid_x(inst, *past, s) == (4 if inst[0] == 9 else 2), inst
        if inst in G.COUNTED:
            assert [G.grid_x(inst, *g, s) for g in G.geoms_count(inst, s)] == [7, 8, 9, 13], inst
    for P in (64, 128):
        assert [B * H * W for B, H, W in G.geoms_1x1(P, 1)] == [1, P - 1, P, P + 1, 189]
        assert [B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) for B, H, W in G.geoms_1x1(P, 2)] == [1, P - 1, P, P + 1, 189, 189]
    assert G.PYRAMIDS["eight"] == ((33, 17), (17, 9), (9, 5), (5, 3), (3, 2), (2, 1), (1, 1), (1, 1))


def test_guarded_views_are_aligned_and_banded():
    v = torch.arange(3 * 5 * 7 * 32, dtype=torch.float16).view(3, 5, 7, 32)
    g = G.Guarded(v, "cpu")
    assert torch.equal(g.t, v) and g.bands_untouched() and g.all_written()
    assert g.lo * 2 >= 65536 and (g.buf.numel() - g.hi) * 2 >= 65536 and (g.t.data_ptr() - g.buf.data_ptr()) % 16 == 0
    assert G.nchw(g.t).is_contiguous(memory_format=torch.channels_last)
    o = G.Guarded((2, 3, 64), "cpu")
    assert not o.all_written() and o.bands_untouched()
    o.buf[o.hi] = 0
    assert not o.bands_untouched()


# ----------------------------------------------------------------------------- the library's own answer
def _query(B, C, H, W, O, k, s):
    """s2a_conv_nhwc_f16_form -> (return code, (TAPS, OG, PH, SD, HT), TAIL)"""
    from s2anet_amd import _lib
    f = (ctypes.c_int32 * 6)(*([-1] * 6))
    rc = _lib.lib().s2a_conv_nhwc_f16_form(B, C, H, W, O, k, s, f)
    return rc, (f[0], f[1], f[2], f[3], f[5]), f[4]


def _set_switches(monkeypatch, sw):
    for name in G.SWITCHES:
        if name in sw:
            monkeypatch.setenv(name, sw[name])
        else:
            monkeypatch.delenv(name, raising=False)


def test_query_answers_the_instantiation_of_every_case(monkeypatch):
    """(a) with a case's switches set, the library routes it to the instantiation the table says it runs"""
    for c in G.CASES:
        _set_switches(monkeypatch, c["sw"])
        assert _query(c["B"], c["C"], c["H"], c["W"], c["O"], c["k"], c["s"]) == (0, c["inst"], 0), c["id"]
    print("query against the table: %d cases" % len(G.CASES))


# geometries (B, H, W) on both sides of each default threshold, with what is counted there at stride 1:
#   16 x 16 tiles, O = 64 / 128 (from 256 on: filter through LDS): 240 | 256, B = 3: 255 | 258
#   16 x 16 tiles, O = 256 (from 512 on): 511 | 512, B = 3: 510 | 513
#   8 x 16 workgroups, O = 128 / 256 (below 256: 4 x 16 tiles): 255 | 256, B = 3: 255 | 258
#   128-position workgroups of a 1x1, O = 256 (below 256: 64 positions): 255 | 256, B = 3: 255 | 258; the last pair at stride 2
#   and two maps far below every threshold
THRESHOLD_GEOMS = {
    "tiles16_256": ((1, 240, 256), (1, 241, 256), (3, 80, 272), (3, 32, 688)),
    "tiles16_512": ((1, 112, 1168), (1, 256, 512), (3, 160, 272), (3, 144, 304)),
    "wgs8x16_256": ((1, 120, 272), (1, 128, 256), (3, 40, 272), (3, 16, 688)),
    "wgs128_256": ((1, 255, 128), (1, 256, 128), (3, 85, 128), (3, 86, 128), (1, 510, 256), (1, 512, 256)),
    "small": ((1, 8, 16), (1, 1, 1)),
}
GRID_CHANNELS, GRID_OUT = (32, 64, 192), (64, 128, 256, 512)


def test_threshold_geometries_sit_on_both_sides():
    def count(g, rows):
        B, H, W = g
        return B * ((W + 15) // 16) * ((H + rows - 1) // rows)
    T = THRESHOLD_GEOMS
    assert [count(g, 16) for g in T["tiles16_256"]] == [240, 256, 255, 258]
    assert [count(g, 16) for g in T["tiles16_512"]] == [511, 512, 510, 513]
    assert [count(g, 8) for g in T["wgs8x16_256"]] == [255, 256, 255, 258]
    assert max(count(g, 16) for g in T["wgs8x16_256"]) < 256          # (the 16 x 16 rules stay out of the way)
    assert [(B * H * W + 127) // 128 for B, H, W in T["wgs128_256"][:4]] == [255, 256, 255, 258]
    assert [(B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) + 127) // 128 for B, H, W in T["wgs128_256"][4:]] == [255, 256]
    for gs in T.values():
        for B, H, W in gs:
            assert B * H * W * max(GRID_CHANNELS) * 2 < 2 ** 31 and B * H * W * max(GRID_OUT) * 2 < 2 ** 31 and max(H, W) < 32000


def test_default_routes_equal_the_query(monkeypatch):
    """(b) no switch set: route()'s four thresholds against the library over ksize x stride x C x O x the geometries
    above (3x3 at stride 2 with O = 64 is refused and left to the refusal test).  Default routing reaches all fourteen
    instantiations: none needs a switch."""
    _set_switches(monkeypatch, {})
    reached, points = set(), 0
    for k in (1, 3):
        for s in (1, 2):
            for C in GRID_CHANNELS:
                for O in GRID_OUT:
                    if k == 3 and s == 2 and O % 128:
                        continue
                    for gs in THRESHOLD_GEOMS.values():
                        for B, H, W in gs:
                            want = G.route(k, s, C, O, {}, B, H, W)
                            assert _query(B, C, H, W, O, k, s) == (0, want, 0), (k, s, C, O, B, H, W)
                            reached.add(want)
                            points += 1
    assert reached == set(G.ALL_INSTANTIATIONS) and len(reached) == 14
    # each threshold decides between the two forms it is there for, at the sizes it was set for
    T = THRESHOLD_GEOMS
    for below, above in (T["tiles16_256"][:2], T["tiles16_256"][2:]):
        assert G.route(3, 1, 64, 64, {}, *below) == (9, 1, 1, 1, 0) and G.route(3, 1, 64, 64, {}, *above) == (9, 1, 2, 1, 0)
        assert G.route(3, 1, 64, 128, {}, *below) == (9, 2, 1, 1, 0) and G.route(3, 1, 64, 128, {}, *above) == (9, 2, 2, 1, 0)
    for below, above in (T["tiles16_512"][:2], T["tiles16_512"][2:]):
        assert G.route(3, 1, 64, 256, {}, *below) == (9, 4, 1, 1, 0) and G.route(3, 1, 64, 256, {}, *above) == (9, 4, 2, 1, 0)
    for below, above in (T["wgs8x16_256"][:2], T["wgs8x16_256"][2:]):
        for O, og in ((128, 2), (256, 4)):
            assert G.route(3, 1, 64, O, {}, *below) == (9, og, 1, 1, 1) and G.route(3, 1, 64, O, {}, *above) == (9, og, 1, 1, 0)
    for s, (below, above) in ((1, T["wgs128_256"][:2]), (1, T["wgs128_256"][2:4]), (2, T["wgs128_256"][4:])):
        assert G.route(1, s, 64, 256, {}, *below) == (1, 4, 1, 2, 0) and G.route(1, s, 64, 256, {}, *above) == (1, 4, 1, 1, 0)
    print("default routes: %d points" % points)


def _atoi(v):
    """the C library's atoi on the values used below"""
    import re
    m = re.match(r"\s*[+-]?\d+", v)
    return int(m.group(0)) if m else 0


def test_switch_values_are_parsed_as_documented(monkeypatch):
    """(c) S2A_CONV_PH, S2A_CONV_PH_NARROW: a set value is 2 when atoi gives 2 and 1 otherwise, the empty string included;
    S2A_CONV3_HALF, S2A_CONV1_HALF: on when atoi gives non-zero.  Each at a shape below and one above its threshold, where
    the two settings launch different forms."""
    T = THRESHOLD_GEOMS
    shapes = {"S2A_CONV_PH_NARROW": (3, 1, 64, 128, T["tiles16_256"][:2]), "S2A_CONV_PH": (3, 1, 64, 256, T["tiles16_512"][:2]),
              "S2A_CONV3_HALF": (3, 1, 64, 256, T["wgs8x16_256"][:2]), "S2A_CONV1_HALF": (1, 1, 64, 256, T["wgs128_256"][:2])}
    points = 0
    for name, (k, s, C, O, geoms) in shapes.items():
        for B, H, W in geoms:
            seen = set()
            for v in ("", "0", "1", "2", "3", "x"):
                if name in ("S2A_CONV_PH", "S2A_CONV_PH_NARROW"):
                    meant = "2" if _atoi(v) == 2 else "1"
                else:
                    meant = "1" if _atoi(v) != 0 else "0"
                _set_switches(monkeypatch, {name: v})
                want = G.route(k, s, C, O, {name: meant}, B, H, W)
                assert _query(B, C, H, W, O, k, s) == (0, want, 0), (name, v, B, H, W)
                seen.add(want)
                points += 1
            assert len(seen) == 2, (name, seen)
    print("switch values: %d points" % points)


def test_query_refuses_what_the_call_refuses(monkeypatch):
    """(d) the sizes the entry point refuses are refused by the query with the same code and text; an empty batch is
    answered with the form of the sizes; the bound on the output of a fused residual is the call's alone"""
    from s2anet_amd import _lib
    L = _lib.lib()
    _set_switches(monkeypatch, {})
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    #          B, C, H, W, O, k, s
    refused = ((1, 64, 8, 8, 96, 3, 1, "multiple of 64"), (1, 64, 8, 8, 64, 3, 2, "stride 2"), (1, 64, 8, 8, 192, 3, 2, "stride 2"),
               (1, 48, 8, 8, 64, 3, 1, "multiple of 64"), (1, 64, 8, 8, 64, 5, 1, "kernel size"), (1, 64, 8, 8, 64, 3, 3, "stride"),
               (1, 64, 0, 8, 64, 3, 1, "bad shape"), (-1, 64, 8, 8, 64, 3, 1, "bad shape"),
               (1, 64, 4096, 4096, 64, 1, 1, "32-bit offsets"), (1, 64, 1, 32000, 64, 3, 1, "32-bit offsets"))
    for *sizes, text in refused:
        B, C, H, W, O, k, s = sizes
        assert L.s2a_conv_nhwc_f16(one, one, one, z, one, B, C, H, W, O, k, s, 1, z) == _lib.EINVAL
        said = L.s2a_last_error().decode()
        assert text in said, (sizes, said)
        rc, form, tail = _query(*sizes)
        assert rc == _lib.EINVAL and L.s2a_last_error().decode() == said, (sizes, said)
        assert form == (-1,) * 5 and tail == -1                       # nothing written
    assert _query(0, 64, 8, 8, 256, 3, 1) == (0, G.route(3, 1, 64, 256, {}, 0, 8, 8), 0)
    assert _query(1, 64, 1, 32000, 64, 1, 1)[0] == 0                  # (a 1x1 has no limit on the map's side)
    # 64 -> 512 on 2048 x 1024: x is 256 MiB, the output 2 GiB.  Only a call with a residual refuses it; the query, as a
    # call without one (which gets as far as its NULL tensor), answers
    big = (1, 64, 2048, 1024, 512, 1, 1)
    assert L.s2a_conv_nhwc_f16(one, one, one, one, one, *big, 1, z) == _lib.EINVAL and "fused residual" in L.s2a_last_error().decode()
    assert L.s2a_conv_nhwc_f16(z, one, one, z, one, *big, 1, z) == _lib.EINVAL and "NULL tensor" in L.s2a_last_error().decode()
    assert _query(*big) == (0, G.route(1, 1, 64, 512, {}, 1, 2048, 1024), 0)


def test_refused_shapes_come_back_as_argument_errors():
    """O = 96 and a 3x3 at stride 2 with O = 64 or 192 (tests/test_cabi_cpu.py holds C = 48, ksize 5, stride 3 and the
    misaligned x): refused before any HIP call"""
    from s2anet_amd import _lib
    L = _lib.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert L.s2a_conv_nhwc_f16(one, one, one, z, one, 1, 64, 8, 8, 96, 3, 1, 1, z) == -1
    assert "multiple of 64" in L.s2a_last_error().decode()
    for O in (64, 192):
        assert L.s2a_conv_nhwc_f16(one, one, one, z, one, 1, 64, 8, 8, O, 3, 2, 1, z) == -1
        assert "stride 2" in L.s2a_last_error().decode()
