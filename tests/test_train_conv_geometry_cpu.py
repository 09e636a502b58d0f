"""The training-kernel case table (tests/train_conv_geometry_cases.py) checked without a GPU: what the table reaches, by
name; its restatement of ksplit / slices / workspace against the library's own answers; the exactness the GPU file relies
on, proved from the data of every case (the sum of the terms' magnitudes stays under 2^20 units of 2^-4, and the terms summed
in f32 in two random orders equal float64); the fall-back bound against 1/32; and the references against autograd and
against the formulas of tests/test_train_conv_cpu.py and tests/test_train_conv_s2_cpu.py."""
import torch
import torch.nn.functional as F

import train_conv_geometry_cases as T

F16, F32, F64 = T.F16, T.F32, T.F64

WANTED = [
    # the stride-1 weight gradient around its own ksplit, k = 3 and k = 1
    "tiles = slices - 1, k = 3, s1", "tiles = slices, k = 3, s1", "tiles = slices + 1, k = 3, s1", "tiles = 2 slices + 1, k = 3, s1",
    "tiles = slices - 1, k = 1, s1", "tiles = slices, k = 1, s1", "tiles = slices + 1, k = 1, s1", "tiles = 2 slices + 1, k = 1, s1",
    "slices without a tile, k = 3, s1", "slices without a tile, k = 1, s1",
    "partial last tile row and column past the slices, k = 3, s1", "B > 1, k = 3, s1", "a 1x1 tile spans images, s1",
    # out-channel groups
    "idle mwave waves", "a full 256-group and a 64 rest", "two full 256-groups",
    # the strided weight gradient around its 32 slices
    "tiles = slices - 1, k = 3, s2", "tiles = slices, k = 3, s2", "tiles = slices + 1, k = 3, s2", "tiles = 2 slices + 1, k = 3, s2",
    "tiles = slices - 1, k = 1, s2", "tiles = slices, k = 1, s2", "tiles = slices + 1, k = 1, s2", "tiles = 2 slices + 1, k = 1, s2",
    "slices without a tile, k = 3, s2", "slices without a tile, k = 1, s2", "a 1x1 tile spans images, s2",
    "H odd, W odd", "H odd, W even", "H even, W odd", "H even, W even",
    "Wo = 16 on the 33-pixel patch row", "Wo = 17 on the 33-pixel patch row", "partial tile, k = 3, s2", "sparse g",
    # the strided input gradient
    "edge-free s2 input tile", "partial s2 input tile", "B > 1, k = 3, s2", "B > 1, k = 1, s2",
    # the preparation pass
    "prep rows = 1", "prep rows = 31", "prep rows = 32", "prep rows = 33 with empty workgroups", "prep rows = 34 with empty workgroups",
    "prep at the 256-workgroup cap",
]


def test_table_reaches_every_mechanism_by_name():
    have = T.mechanisms()
    missing = [w for w in WANTED if w not in have]
    assert not missing, missing
    assert T.prep_geometry(8193) == (256, 33, 7) and T.prep_geometry(8192) == (256, 32, 0) and T.prep_geometry(8449)[1] == 34
    assert T.prep_geometry(8191) == (256, 32, 0) and T.prep_geometry(33) == (2, 17, 0) and T.prep_geometry(1) == (1, 1, 0)
    ids = [c["id"] for c in T.WGRAD_CASES + T.DGRAD_S2 + T.DGRAD_S1]
    assert len(ids) == len(set(ids))
    # the counts the issue names
    by = {(c["fam"], c["C"], c["O"]): [] for c in T.WGRAD_CASES}
    for c in T.WGRAD_CASES:
        by[(c["fam"], c["C"], c["O"])].append(c["tiles"])
    assert T.ksplit(64, 64, 3) == 85 and {84, 85, 86, 171} <= set(by[("w3", 64, 64)])
    assert T.ksplit(128, 512, 3) == 21 and {20, 21, 22, 43} <= set(by[("w3", 128, 512)])
    assert T.ksplit(512, 512, 1) == 32 and {31, 32, 33, 65} <= set(by[("w1", 512, 512)])
    assert T.ksplit(64, 64, 1) == 512 and 513 in by[("w1", 64, 64)]
    assert {31, 32, 33, 65} <= set(by[("ws3", 64, 128)]) and {31, 32, 33, 65} <= set(by[("ws1", 64, 64)])
    for c in T.WGRAD_CASES + T.DGRAD_S2 + T.DGRAD_S1:        # no tensor above 8 MB; a row of x inside the guard band
        Ho, Wo = T.out_hw(c["H"], c["W"], c["s"])
        assert c["B"] * c["H"] * c["W"] * c["C"] * 2 <= 8 << 20 and c["B"] * Ho * Wo * c["O"] * 2 <= 8 << 20, c["id"]
        assert c["W"] * c["C"] * 2 <= T.BAND or c["k"] == 1, c["id"]
    # one Gaussian copy per kernel per (C, O)
    assert {(c["fam"], c["C"], c["O"]) for c in T.GAUSS_WGRAD} == set(by)
    assert {(c["fam"], c["C"], c["O"]) for c in T.GAUSS_DGRAD} == {(c["fam"], c["C"], c["O"]) for c in T.DGRAD_S2 + T.DGRAD_S1}


def test_ksplit_slices_and_workspace_restate_the_library():
    from s2anet_amd import _lib
    L = _lib.lib()
    for c in T.WGRAD_CASES:
        shape = (c["B"], c["C"], c["H"], c["W"], c["O"], c["k"])
        if c["s"] == 2:
            assert L.s2a_conv_backward_weight_s2_slices(*shape) == c["slices"] == T.s2_slices(c["C"], c["O"], c["k"]), c["id"]
        else:
            assert c["slices"] == T.ksplit(c["C"], c["O"], c["k"])
            assert L.s2a_conv_backward_weight_f16_workspace_bytes(*shape) == T.workspace_bytes(c["C"], c["O"], c["k"]), c["id"]
    # the workspace is the only place the library shows ksplit: where ksplit * nowner is above the launch's aim it IS the size
    for C, O, k in ((64, 64, 3), (64, 64, 1), (128, 512, 3), (512, 512, 1), (64, 320, 3), (1024, 512, 3), (2048, 1024, 1)):
        got = L.s2a_conv_backward_weight_f16_workspace_bytes(1, C, 8, 8, O, k)
        assert got == T.workspace_bytes(C, O, k), (C, O, k)
        assert got >= T.ksplit(C, O, k) * T.nowner(C, O, k) * min(O, 256) * k * 64 * 4


def _two_orders(gs, xs, gen):
    """sum over the rows of gs[n,O]^T xs[n,C] in f32, rows in two random orders"""
    out = []
    for _ in range(2):
        p = torch.randperm(gs.shape[0], generator=gen)
        out.append(gs[p].float().t() @ xs[p].float())
    return out


def test_weight_gradient_cases_are_exact_in_any_order_and_the_fallback_bound_sees_one_term():
    """every dyadic weight-gradient case: at most MAX_TERMS terms, sum of magnitudes under 2^20 sixteenths (so every partial
    sum in any order is an f32 number), the f32 sums in two random orders equal float64, the reference is autograd's, and the
    fall-back bound stays below 1/32 -- except in the one case with 1 025 nonzero positions (513 tiles on 512 slices need
    them), where it is 0.10 and would not separate a single term"""
    blind = []
    for c in T.WGRAD_CASES:
        x, g = T.wgrad_inputs(c)
        assert bool(((x * 4).abs() >= 1).all()) and bool(((x * 4) == (x * 4).round()).all()) and float(x.abs().max()) <= 2
        gw, S, n = T.wgrad_ref(x, g, c["k"], c["s"])
        Ho, Wo = T.out_hw(c["H"], c["W"], c["s"])
        dense = c["B"] * Ho * Wo <= T.DENSE_MAX
        assert n <= T.MAX_TERMS and (n == c["B"] * Ho * Wo if dense else n <= max(T.SPARSE_MAX, 2 * c["slices"] + 2)), (c["id"], n)
        assert float(S.max()) * 16 < 2 ** 20, c["id"]
        T.as_f32_exactly(gw)
        gen = T.gen_of(c["id"] + ":orders")
        pad = c["k"] // 2
        at = (g != 0).any(-1).nonzero()
        gs = g[at[:, 0], at[:, 1], at[:, 2]]
        xp = F.pad(x, (0, 0, pad, pad, pad, pad))
        ky, kx = int(torch.randint(0, c["k"], (1,), generator=gen)), int(torch.randint(0, c["k"], (1,), generator=gen))
        xs = xp[at[:, 0], c["s"] * at[:, 1] + ky, c["s"] * at[:, 2] + kx]
        for got in _two_orders(gs, xs, gen):
            assert torch.equal(got.double(), gw[:, :, ky, kx]), c["id"]
        if c["B"] * c["H"] * c["W"] * c["C"] <= 1 << 18:          # autograd where it is cheap: every geometry case
            assert torch.equal(T.wgrad_autograd(x, g, c["k"], c["s"]), gw), c["id"]
        if not dense:                                            # the sparse g holds the corners the table promises
            flat = (g != 0).any(-1).view(-1).nonzero().view(-1).tolist()
            for t in (0, c["tiles"] - 1):
                assert set(T.tile_corners(t, c["B"], Ho, Wo, c["k"])) <= set(flat), c["id"]
            for s in range(min(c["slices"], c["tiles"])):
                assert any(set(T.tile_corners(t, c["B"], Ho, Wo, c["k"])) <= set(flat) for t in range(s, c["tiles"], c["slices"])), c["id"]
        b = float(T.bound(n, c["slices"], S, gw, False).max())
        if not b < 1 / 32:
            blind.append((c["id"], n, round(b, 3)))
    assert [i for i, _, _ in blind] == ["w1-k1s1-c64o64-b3x1x10923"], blind


def test_input_gradient_cases_are_exact_in_any_order():
    """every dyadic input-gradient case: O * taps-of-the-class terms <= MAX_TERMS, sum of magnitudes under 2^20 sixteenths,
    f32 autograd in two channel orders equals float64.  The fall-back bound stays below 1/32 only up to about 500 terms:
    above it (O >= 256 at k = 3, O = 320 at k = 1) it could not separate one term -- asserted as such, not hidden."""
    for c in T.DGRAD_S2 + T.DGRAD_S1:
        g, w = T.dgrad_inputs(c)
        gx, S = T.dgrad_ref(g, w, c["H"], c["W"], c["s"])
        assert c["terms"] <= T.MAX_TERMS and float(S.max()) * 16 < 2 ** 20, c["id"]
        T.as_f32_exactly(gx)
        gen = T.gen_of(c["id"] + ":orders")
        for _ in range(2):
            p = torch.randperm(c["O"], generator=gen)
            x0 = torch.zeros((c["B"], c["C"], c["H"], c["W"]), requires_grad=True)
            F.conv2d(x0, w[p].float(), None, c["s"], c["k"] // 2).backward(T.nchw(g[..., p].float()))
            assert torch.equal(x0.grad.permute(0, 2, 3, 1).double(), gx), c["id"]
        b = float(T.bound(c["terms"], 0, S, gx, False).max())
        assert b < 1 / 32 or c["terms"] > 512, (c["id"], c["terms"], b)


def test_prep_pool_and_pack_inputs_are_what_the_issue_asks_for():
    for P in T.PREP_P:
        for O in T.PREP_O:
            go, out = T.prep_inputs(P, O)
            assert int((out == 0).sum()) >= 16 and bool(torch.signbit(out[out == 0]).any()) and bool((~torch.signbit(out[out == 0])).any())
            assert bool(out.isnan().any()) and bool(((out > 0) & (out < 2.0 ** -14)).any())
            g = torch.where(out <= 0, torch.zeros_like(go), go)
            s64 = g.double().sum(0)
            T.as_f32_exactly(s64)
            assert float(g.double().abs().sum(0).max()) * 4 < 2 ** 20
            gen = T.gen_of("prep-orders-%d-%d" % (P, O))
            for _ in range(2):
                acc = torch.zeros((O,), dtype=F32)
                for chunk in g[torch.randperm(P, generator=gen)].float().split(97):
                    acc = acc + chunk.sum(0)
                assert torch.equal(acc.double(), s64)
    for O, C, k in T.PACK_SIZES:
        w = T.pack_master(O, C, k, F32)
        h = w.half()
        assert bool(h.isinf().any()) and bool(((h != 0) & (h.abs() < 2.0 ** -14)).any())
        assert bool((w == 1 + 2.0 ** -11).any()) and bool((w == 65520.0).any())         # ties: 1 + u and f16's overflow threshold
        assert float(h[w == 65519.0][0]) == 65504.0 and bool(h[w == 65520.0].isinf().all()) and float(h[w == 2.0 ** -25][0]) == 0.0
        assert torch.equal(T.dgrad_filter(h)[3, 5], h[5, 3].flip(0, 1))
    for shape in T.POOL_SHAPES:
        g = T.dyadic(T.gen_of("pool-%d-%d-%d-%d" % shape), shape)
        want = g.double().view(shape[0], shape[1] // 2, 2, shape[2] // 2, 2, shape[3]).sum((2, 4))
        assert torch.equal(T.sum_pool_f32(g).double(), want)
    assert 1 * 3 * 5 * (72 // 8) == 135


def test_references_are_the_formulas_of_the_older_cpu_files():
    from test_train_conv_cpu import dgrad_filter, weight_grad_formula
    from test_train_conv_s2_cpu import input_grad_3x3_s2, weight_grad_s2
    gen = T.gen_of("identities")
    for k in (3, 1):
        for (B, H, W) in ((2, 5, 17), (1, 4, 16), (3, 9, 1)):
            x, g = T.gauss(gen, (B, H, W, 64)), T.gauss(gen, (B, H, W, 64))
            ref = T.wgrad_ref(x, g, k, 1)[0]
            auto = T.wgrad_autograd(x, g, k, 1)
            form = weight_grad_formula(T.nchw(x).double(), T.nchw(g).double(), k)
            assert torch.allclose(ref, auto, rtol=1e-12, atol=1e-12) and torch.allclose(form, auto, rtol=1e-12, atol=1e-12)
        for (B, H, W) in ((2, 9, 21), (1, 10, 22), (1, 1, 1), (1, 2, 2)):
            Ho, Wo = T.out_hw(H, W, 2)
            x, g, w = T.gauss(gen, (B, H, W, 64)), T.gauss(gen, (B, Ho, Wo, 128)), T.gauss(gen, (128, 64, k, k))
            auto = T.wgrad_autograd(x, g, k, 2)
            assert torch.allclose(T.wgrad_ref(x, g, k, 2)[0], auto, rtol=1e-12, atol=1e-12)
            assert torch.allclose(weight_grad_s2(T.nchw(x).double(), T.nchw(g).double(), k), auto, rtol=1e-12, atol=1e-12)
            gx = T.dgrad_ref(g, w, H, W, 2)[0]
            if k == 3:
                cls = input_grad_3x3_s2(T.nchw(g).double(), w.double(), H, W)
                assert torch.allclose(cls.permute(0, 2, 3, 1), gx, rtol=1e-12, atol=1e-12)
            else:
                odd = gx.clone()
                odd[:, 0::2, 0::2] = 0
                assert int((odd != 0).sum()) == 0 and not bool(torch.signbit(odd).any())
        w = T.gauss(gen, (128, 64, k, k))
        assert torch.equal(T.dgrad_filter(w), dgrad_filter(w))
        # the stride-1 input gradient IS the convolution of g with the header's filter
        g = T.gauss(gen, (2, 5, 17, 128))
        conv = F.conv2d(T.nchw(g).double(), T.dgrad_filter(w).double(), None, 1, k // 2).permute(0, 2, 3, 1)
        assert torch.allclose(conv, T.dgrad_ref(g, w, 5, 17, 1)[0], rtol=1e-12, atol=1e-12)


def test_the_shared_tables_are_not_sampled():
    """the GPU file parametrises over these very tuples"""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_train_conv_geometry.py")).read()
    for name in ("WGRAD_S1", "WGRAD_S2", "DGRAD_S2", "DGRAD_S1", "GAUSS_WGRAD", "GAUSS_DGRAD", "PACK_SIZES", "PREP_P", "PREP_O",
                 "PREP_CALLS", "POOL_SHAPES", "INF_CASES"):
        assert "T." + name in src, name
    assert "skip" not in src and "xfail" not in src
    ast.parse(src)
