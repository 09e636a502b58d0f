"""The dense-convolution case table (tests/conv_geometry_cases.py) checked without a GPU: the float64 reference against
torch's own float64 convolution, the bound against an emulation of the kernel's arithmetic, what the table reaches, and
the shapes the entry point refuses."""
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
