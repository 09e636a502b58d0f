"""GPU: the training kernels of the dense convolutions (s2anet_amd/csrc/conv_bwd_ops.hip) called through their C entry points
at the tile-edge geometries of tests/train_conv_geometry_cases.py and held to float64 PER ELEMENT.

The inputs are exact by construction (operands k / 4, at most 4 096 terms per output element: every f32 partial sum in any
order is exact -- tests/test_train_conv_geometry_cpu.py proves it from the data), so an f32 result must EQUAL the float64 sum
and an f16 result be that sum rounded once: one dropped, doubled or misplaced term is a failed torch.equal.  A Gaussian copy
of one case per kernel per (C, O) carries the general numerics: |err| <= (n + slices + 17) u32 S + 2^-25 (+ u16 |y| for f16).

Every input and every output is a view into a larger buffer with >= 64 KiB of fill on each side (NaN around the inputs).
Every output is launched into twice, over a NaN fill (0xFF bytes) and over 0xA5 bytes: the two results must have equal bits
(every element is written), every band must keep its fill (nothing else is written) and no result of finite inputs may hold a
NaN (nothing outside an input was read).

Set S2A_TRAIN_CONV_GEOMETRY_REPORT=<path> to write the Gaussian copies' worst ratios (error over bound) per family as JSON;
the committed run is profiles/train_conv_geometry.json.  The planted defects this file was run against are in docs/HISTORY.md."""
import ctypes
import json
import os

import pytest
import torch

import train_conv_geometry_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32, F64 = T.F16, T.F32, T.F64
U8 = torch.uint8
REPORT = {}
SCRATCH = "scratch"               # a workspace: bands checked, contents not compared


def abi():
    from s2anet_amd import _lib
    return _lib, _lib.lib()


class Bytes:
    """nbytes of `fill` bytes between two bands of BAND fill bytes, the view 16-byte aligned; values: copied in (an input)"""

    def __init__(self, nbytes, fill, values=None):
        self.n, self.fill = int(nbytes), fill
        self.buf = torch.full((2 * T.BAND + self.n + 16,), fill, dtype=U8, device=DEV)
        self.flat = self.buf[T.BAND:T.BAND + self.n]
        assert self.flat.data_ptr() % 16 == 0 and T.BAND >= 65536
        if values is not None:
            self.flat.copy_(values.contiguous().view(-1).view(U8))
        self.ptr = ctypes.c_void_p(self.flat.data_ptr())

    def view(self, dtype, shape):
        return self.flat.view(dtype).view(shape)

    def bands_untouched(self):
        return bool((self.buf[:T.BAND] == self.fill).all()) and bool((self.buf[T.BAND + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def vp(g):
    """pointer of a Guarded input (or NULL)"""
    return ctypes.c_void_p(g.t.data_ptr() if g is not None else 0)


def esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def bits(t):
    return t.view({1: U8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def twice(launch, outs, inputs=()):
    """launch(bufs) once over NaN bytes and once over 0xA5 bytes; outs: name -> (dtype, shape[, SCRATCH]).  Asserts: every
    band intact, equal bits from both launches, no NaN -> the results on the CPU"""
    got = []
    for fill in (T.NAN_BYTE, T.OTHER_BYTE):
        bufs = {n: Bytes(torch.Size(o[1]).numel() * esize(o[0]), fill) for n, o in outs.items()}
        launch(bufs)
        torch.cuda.synchronize()
        for n, b in bufs.items():
            assert b.bands_untouched(), "bytes beside %s were written" % n
        for g in inputs:
            assert g.bands_untouched(), "an input's band was written"
        got.append({n: bufs[n].view(o[0], o[1]).clone().cpu() for n, o in outs.items() if SCRATCH not in o})
    for n, a in got[0].items():
        assert torch.equal(bits(a), bits(got[1][n])), "%s depends on what the buffer held: not every element is written" % n
        assert not bool(a.isnan().any()), "%s holds a NaN: something outside an input was read" % n
    return got[0]


def note(family, case_id, ratio, ok):
    r = REPORT.setdefault(family, dict(ratio=0.0, ratio_case=None, comparisons=0))
    r["comparisons"] += 1
    if ratio >= r["ratio"]:
        r["ratio"], r["ratio_case"] = ratio, case_id
    print("%-8s %-40s ratio %.3f" % (family, case_id, ratio))
    path = os.environ.get("S2A_TRAIN_CONV_GEOMETRY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(sorted(REPORT.items())), f, indent=1)
    return ok


def dims(c):
    return tuple(c[n] for n in ("B", "C", "H", "W", "O", "k"))


# ----------------------------------------------------------------------------- 1, 2: the stride-1 weight gradient
def weight_s1(c, gx, gg):
    """s2a_conv_backward_weight_f16 into guarded outputs, both gradient dtypes -> {dtype: [O,C,k,k] on the CPU}"""
    _lib, L = abi()
    B, C, H, W, O, k = dims(c)
    wsb = L.s2a_conv_backward_weight_f16_workspace_bytes(B, C, H, W, O, k)
    assert wsb == T.workspace_bytes(C, O, k)
    res = {}
    for dt, code in ((F32, _lib.DTYPE_F32), (F16, _lib.DTYPE_F16)):
        def launch(b):
            _lib.check(L.s2a_conv_backward_weight_f16(vp(gx), vp(gg), b["gw"].ptr, code, B, C, H, W, O, k, b["ws"].ptr, wsb,
                                                      _lib.stream_ptr()))
        res[dt] = twice(launch, {"gw": (dt, (O, C, k, k)), "ws": (U8, (wsb,), SCRATCH)}, (gx, gg))["gw"]
    return res


@pytest.mark.parametrize("c", T.WGRAD_S1, ids=lambda c: c["id"])
def test_weight_gradient(c):
    x, g = T.wgrad_inputs(c)
    gw, S, n = T.wgrad_ref(x, g, c["k"], 1)
    got = weight_s1(c, T.Guarded(x, DEV), T.Guarded(g, DEV))
    for dt in (F32, F16):
        assert T.exact(got[dt], gw), (c["id"], dt, T.mismatches(got[dt], gw))


# ----------------------------------------------------------------------------- 3: the strided weight gradient and its reduce
def weight_s2(c, gx, gg):
    """s2a_conv_backward_weight_s2_f16 and both reduces -> partial [slices, O C k k] f32, the f32 and the f16 sum"""
    _lib, L = abi()
    B, C, H, W, O, k = dims(c)
    slices = L.s2a_conv_backward_weight_s2_slices(B, C, H, W, O, k)
    assert slices == c["slices"]
    count = O * C * k * k

    def launch(b):
        _lib.check(L.s2a_conv_backward_weight_s2_f16(vp(gx), vp(gg), b["partial"].ptr, slices, B, C, H, W, O, k, _lib.stream_ptr()))
        for name, code in (("sum32", _lib.DTYPE_F32), ("sum16", _lib.DTYPE_F16)):
            _lib.check(L.s2a_conv_backward_weight_s2_reduce(b["partial"].ptr, slices, count, b[name].ptr, code, _lib.stream_ptr()))
    return twice(launch, {"partial": (F32, (slices, count)), "sum32": (F32, (O, C, k, k)), "sum16": (F16, (O, C, k, k))}, (gx, gg))


def check_slices(c, got):
    part = got["partial"]
    for s in range(min(c["tiles"], c["slices"]), c["slices"]):          # a slice without a tile holds exact zeros
        assert int((bits(part[s]) != 0).sum()) == 0, (c["id"], s)
    acc = torch.zeros_like(part[0])
    for s in range(c["slices"]):                                         # the reduce is the slices' sum in slice order
        acc = acc + part[s]
    assert torch.equal(acc.view(got["sum32"].shape), got["sum32"]) and torch.equal(acc.to(F16).view(got["sum16"].shape), got["sum16"])


@pytest.mark.parametrize("c", T.WGRAD_S2, ids=lambda c: c["id"])
def test_strided_weight_gradient(c):
    x, g = T.wgrad_inputs(c)
    gw, S, n = T.wgrad_ref(x, g, c["k"], 2)
    got = weight_s2(c, T.Guarded(x, DEV), T.Guarded(g, DEV))
    check_slices(c, got)
    assert torch.equal(got["partial"].double().sum(0).view(gw.shape), gw), c["id"]      # (every partial sum is exact)
    for name in ("sum32", "sum16"):
        assert T.exact(got[name], gw), (c["id"], name, T.mismatches(got[name], gw))


@pytest.mark.parametrize("c", T.GAUSS_WGRAD, ids=lambda c: c["id"])
def test_weight_gradient_gaussian(c):
    x, g = T.wgrad_inputs(c, "gauss")
    gw, S, n = T.wgrad_ref(x, g, c["k"], c["s"])
    Ho, Wo = T.out_hw(c["H"], c["W"], c["s"])
    assert n == c["B"] * Ho * Wo <= T.DENSE_MAX
    gx, gg = T.Guarded(x, DEV), T.Guarded(g, DEV)
    if c["s"] == 1:
        got = weight_s1(c, gx, gg)
    else:
        r = weight_s2(c, gx, gg)
        check_slices(c, r)
        got = {F32: r["sum32"], F16: r["sum16"]}
    bad = []
    for dt in (F32, F16):
        ratio, ok = T.bounded(got[dt], gw, S, n, c["slices"])
        if not note("%s.%s" % (c["fam"], "f32" if dt == F32 else "f16"), c["id"], ratio, ok):
            bad.append((dt, ratio))
    assert not bad, (c["id"], bad)


# ----------------------------------------------------------------------------- 4, 5: the input gradients
def pack_train(w, fwd, dgrad):
    """s2a_conv_pack_weight_train of a master on the device (a Guarded f16 or a Bytes f32) into two pointers"""
    _lib, L = abi()
    master, dtype, (O, C, k) = w
    _lib.check(L.s2a_conv_pack_weight_train(master, _lib.DTYPE_F32 if dtype == F32 else _lib.DTYPE_F16, O, C, k, fwd, dgrad,
                                            _lib.stream_ptr()))


def input_gradient(c, gg, gw):
    """the filter through s2a_conv_pack_weight_train, then s2a_conv_backward_input_s2_f16 (stride 2) or s2a_conv_nhwc_f16 on
    the output gradient with channels = O, out_channels = C (stride 1, as production computes it) -> gx [B,H,W,C] f16"""
    _lib, L = abi()
    B, C, H, W, O, k = dims(c)

    def launch(b):
        pack_train((vp(gw), F16, (O, C, k)), b["fwd"].ptr, b["dgrad"].ptr)
        if c["s"] == 2:
            _lib.check(L.s2a_conv_backward_input_s2_f16(vp(gg), b["dgrad"].ptr, b["gx"].ptr, B, C, H, W, O, k, _lib.stream_ptr()))
        else:
            _lib.check(L.s2a_conv_nhwc_f16(vp(gg), b["dgrad"].ptr, None, None, b["gx"].ptr, B, O, H, W, C, k, 1, 0, _lib.stream_ptr()))
    n = O * C * k * k
    return twice(launch, {"fwd": (F16, (n,)), "dgrad": (F16, (n,)), "gx": (F16, (B, H, W, C))}, (gg, gw))["gx"]


@pytest.mark.parametrize("c", T.DGRAD_S2 + T.DGRAD_S1, ids=lambda c: c["id"])
def test_input_gradient(c):
    g, w = T.dgrad_inputs(c)
    ref, S = T.dgrad_ref(g, w, c["H"], c["W"], c["s"])
    got = input_gradient(c, T.Guarded(g, DEV), T.Guarded(w, DEV))
    assert T.exact(got, ref), (c["id"], T.mismatches(got, ref))
    if c["s"] == 2 and c["k"] == 1:
        odd = torch.ones((c["H"], c["W"]), dtype=torch.bool)
        odd[0::2, 0::2] = False
        assert int((bits(got)[:, odd] != 0).sum()) == 0, "a pixel with an odd row or column is not +0"


@pytest.mark.parametrize("c", T.GAUSS_DGRAD, ids=lambda c: c["id"])
def test_input_gradient_gaussian(c):
    g, w = T.dgrad_inputs(c, "gauss")
    ref, S = T.dgrad_ref(g, w, c["H"], c["W"], c["s"])
    got = input_gradient(c, T.Guarded(g, DEV), T.Guarded(w, DEV))
    ratio, ok = T.bounded(got, ref, S, c["terms"], 0)
    assert note(c["fam"], c["id"], ratio, ok), (c["id"], ratio)


# ----------------------------------------------------------------------------- 6: the filter pack
def pack_f16(w):
    """s2a_conv_pack_weight_f16 of an f16 [O,C,k,k] filter -> packed halfs on the CPU"""
    _lib, L = abi()
    O, C, k, _ = w.shape
    wd = w.to(DEV).contiguous()
    out = torch.empty((w.numel(),), dtype=F16, device=DEV)
    _lib.check(L.s2a_conv_pack_weight_f16(_lib.ptr(wd), O, C, k, _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("with_dgrad", [True, False], ids=["dgrad", "no_dgrad"])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32_master", "f16_master"])
@pytest.mark.parametrize("size", T.PACK_SIZES, ids=lambda s: "o%dc%dk%d" % s)
def test_pack_weight_train(size, dtype, with_dgrad):
    O, C, k = size
    w = T.pack_master(O, C, k, dtype)
    if dtype == F32:
        master = Bytes(w.numel() * 4, T.NAN_BYTE, w.to(DEV))
        handle = master.ptr
    else:
        master = T.Guarded(w, DEV)
        handle = vp(master)
    outs = {"fwd": (F16, (w.numel(),))}
    if with_dgrad:
        outs["dgrad"] = (F16, (w.numel(),))
    got = twice(lambda b: pack_train((handle, dtype, size), b["fwd"].ptr, b["dgrad"].ptr if with_dgrad else None), outs, (master,))
    h = w.to(F16)
    assert torch.equal(bits(got["fwd"]), bits(pack_f16(h))), "packed_fwd is not s2a_conv_pack_weight_f16 of w.half()"
    if with_dgrad:
        assert torch.equal(bits(got["dgrad"]), bits(pack_f16(T.dgrad_filter(h)))), "packed_dgrad is not the header's filter"


# ----------------------------------------------------------------------------- 7: the preparation pass
@pytest.mark.parametrize("O", T.PREP_O)
@pytest.mark.parametrize("P", T.PREP_P)
def test_backward_prep(P, O):
    _lib, L = abi()
    go, out = T.prep_inputs(P, O)
    ggo, gout = T.Guarded(go, DEV), T.Guarded(out, DEV)
    wsb = L.s2a_conv_backward_prep_f16_workspace_bytes(P, O)
    assert wsb >= T.prep_geometry(P)[0] * O * 4
    masked = torch.where(out <= 0, torch.zeros_like(go), go)
    for with_out, want_g, gb_dtype in T.PREP_CALLS:
        outs = {"ws": (U8, (wsb,), SCRATCH)}
        if want_g:
            outs["g"] = (F16, (P, O))
        if gb_dtype is not None:
            outs["gb"] = (gb_dtype, (O,))

        def launch(b):
            _lib.check(L.s2a_conv_backward_prep_f16(vp(ggo), vp(gout if with_out else None), b["g"].ptr if want_g else None,
                                                    b["gb"].ptr if gb_dtype is not None else None,
                                                    _lib.DTYPE_F32 if gb_dtype == F32 else _lib.DTYPE_F16, P, O, b["ws"].ptr, wsb,
                                                    _lib.stream_ptr()))
        got = twice(launch, outs, (ggo, gout))
        tag = (P, O, with_out, want_g, gb_dtype)
        if want_g:
            assert torch.equal(bits(got["g"]), bits(masked)), tag
        if gb_dtype is not None:
            s64 = (masked if with_out else go).double().sum(0)
            assert T.exact(got["gb"], s64), (tag, T.mismatches(got["gb"], s64))
    # nothing to write: no launch, nothing touched; a masked gradient without the forward output: refused, nothing touched
    for with_out, want_g, rc in ((True, False, _lib.OK), (False, False, _lib.OK), (False, True, _lib.EINVAL)):
        g, ws = Bytes(P * O * 2, T.OTHER_BYTE), Bytes(wsb, T.OTHER_BYTE)
        assert L.s2a_conv_backward_prep_f16(vp(ggo), vp(gout if with_out else None), g.ptr if want_g else None, None,
                                            _lib.DTYPE_F32, P, O, ws.ptr, wsb, _lib.stream_ptr()) == rc
        torch.cuda.synchronize()
        assert g.untouched() and ws.untouched()


# ----------------------------------------------------------------------------- 8: the 2 x 2 sum pool
def sum_pool(g):
    _lib, L = abi()
    B, H, W, O = g.shape
    gg = T.Guarded(g, DEV)
    return twice(lambda b: _lib.check(L.s2a_sum_pool2x2_f16(vp(gg), b["out"].ptr, B, H, W, O, _lib.stream_ptr())),
                 {"out": (F16, (B, H // 2, W // 2, O))}, (gg,))["out"]


@pytest.mark.parametrize("shape", T.POOL_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_sum_pool_dyadic_is_exact(shape):
    g = T.dyadic(T.gen_of("pool-%d-%d-%d-%d" % shape), shape)
    B, H, W, O = shape
    want = g.double().view(B, H // 2, 2, W // 2, 2, O).sum((2, 4))
    got = sum_pool(g)
    assert T.exact(got, want), T.mismatches(got, want)


def test_sum_pool_gaussian_is_the_headers_order():
    g = T.gauss(T.gen_of("pool-gauss"), T.POOL_GAUSS, 8.0)
    assert torch.equal(bits(sum_pool(g)), bits(T.sum_pool_f32(g)))


# ----------------------------------------------------------------------------- 9: zero times infinity at partial tiles
def same_class(got, ref, tag):
    """finite where float64 is finite, and equal; float64's class (NaN, +inf, -inf) elsewhere"""
    want = ref.to(F32).to(got.dtype)
    fin = torch.isfinite(ref)
    assert torch.equal(ref[fin].to(F32).double(), ref[fin])
    assert torch.equal(got[fin], want[fin]), (tag, "a value float64 leaves finite differs", int((got[fin] != want[fin]).sum()))
    assert torch.equal(got[~fin].isnan(), want[~fin].isnan()), (tag, "NaN where float64 has an infinity, or the reverse")
    inf = ~fin & ~ref.isnan()
    assert torch.equal(got[inf], want[inf]), (tag, "an infinity of the other sign")


@pytest.mark.parametrize("case", T.INF_CASES, ids=lambda s: "s%d-c%do%d-b%dx%dx%d" % s)
def test_weight_gradient_zero_times_infinity_at_partial_tiles(case):
    s, C, O, B, H, W = case
    c = dict(id="inf-s%d-%dx%d" % (s, H, W), k=3, s=s, C=C, O=O, B=B, H=H, W=W, slices=T.ksplit(C, O, 3) if s == 1 else T.s2_slices(C, O, 3))
    c["tiles"] = T.ntiles(B, *T.out_hw(H, W, s), 3)
    x, g = T.wgrad_inputs(c)
    c0 = T.INF_CHANNEL
    x[:, H - 1, :, c0] = float("inf")
    x[:, :, W - 1, c0] = float("inf")
    ref = T.wgrad_autograd(x, g, 3, s)
    plain = T.wgrad_ref(x, g, 3, s)[0]
    rest = [i for i in range(C) if i != c0]
    assert bool(torch.isfinite(ref[:, rest]).all()) and torch.equal(ref[:, rest], plain[:, rest])
    assert bool(torch.isfinite(ref[:, c0, 0, 0]).all()) and not bool(torch.isfinite(ref[:, c0]).all())
    gx, gg = T.Guarded(x, DEV), T.Guarded(g, DEV)
    _lib, L = abi()
    wsb = L.s2a_conv_backward_weight_f16_workspace_bytes(B, C, H, W, O, 3) if s == 1 else 0
    count = O * C * 9
    for dt, code in ((F32, _lib.DTYPE_F32), (F16, _lib.DTYPE_F16)):
        got = []
        for fill in (T.NAN_BYTE, T.OTHER_BYTE):
            out = Bytes(count * esize(dt), fill)
            if s == 1:
                ws = Bytes(wsb, fill)
                _lib.check(L.s2a_conv_backward_weight_f16(vp(gx), vp(gg), out.ptr, code, B, C, H, W, O, 3, ws.ptr, wsb, _lib.stream_ptr()))
            else:
                ws = Bytes(c["slices"] * count * 4, fill)
                _lib.check(L.s2a_conv_backward_weight_s2_f16(vp(gx), vp(gg), ws.ptr, c["slices"], B, C, H, W, O, 3, _lib.stream_ptr()))
                _lib.check(L.s2a_conv_backward_weight_s2_reduce(ws.ptr, c["slices"], count, out.ptr, code, _lib.stream_ptr()))
            torch.cuda.synchronize()
            assert out.bands_untouched() and ws.bands_untouched() and gx.bands_untouched() and gg.bands_untouched()
            got.append(out.view(dt, (O, C, 3, 3)).clone().cpu())
        assert torch.equal(bits(got[0]), bits(got[1]))
        same_class(got[0], ref, (c["id"], dt))


@pytest.mark.parametrize("geom", [(1, 10, 22), (1, 9, 21), (2, 10, 21)], ids=lambda g: "b%dx%dx%d" % g)
def test_strided_input_gradient_leaves_out_an_infinite_tap_of_a_missing_neighbour(geom):
    """the quads on the bottom / right edge have no neighbour g[i+1] / g[j+1]: the kernel keeps the accumulator instead of
    adding w . 0, which only an infinite filter tap can tell apart (inf * 0 is NaN).  The five taps that go with a neighbour
    are +inf for one (o0, c0); float64 autograd says which entries of gx[..., c0] stay finite"""
    B, H, W = geom
    c = T.dcase("dinf", 3, 2, 64, 128, B, H, W)
    g, w = T.dgrad_inputs(c)
    o0, c0 = 77, T.INF_CHANNEL
    for ky, kx in ((1, 0), (0, 1), (0, 0), (0, 2), (2, 0)):
        w[o0, c0, ky, kx] = float("inf")
    x0 = torch.zeros((B, 64, H, W), dtype=F64, requires_grad=True)
    torch.nn.functional.conv2d(x0, w.double(), None, 2, 1).backward(T.nchw(g).double())
    ref = x0.grad.permute(0, 2, 3, 1)
    assert bool(torch.isfinite(ref[..., c0]).any()) and not bool(torch.isfinite(ref[..., c0]).all())
    gg, gw = T.Guarded(g, DEV), T.Guarded(w, DEV)
    _lib, L = abi()
    got = []
    for fill in (T.NAN_BYTE, T.OTHER_BYTE):
        fwd, dg, gx = Bytes(w.numel() * 2, fill), Bytes(w.numel() * 2, fill), Bytes(B * H * W * 64 * 2, fill)
        pack_train((vp(gw), F16, (128, 64, 3)), fwd.ptr, dg.ptr)
        _lib.check(L.s2a_conv_backward_input_s2_f16(vp(gg), dg.ptr, gx.ptr, B, 64, H, W, 128, 3, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert all(b.bands_untouched() for b in (fwd, dg, gx, gg, gw))
        got.append(gx.view(F16, (B, H, W, 64)).clone().cpu())
    assert torch.equal(bits(got[0]), bits(got[1]))
    same_class(got[0], ref, geom)
