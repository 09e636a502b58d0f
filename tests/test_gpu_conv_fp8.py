"""GPU: the e4m3 kernels of csrc/conv_fp8_ops.hip (s2a_quantize_e4m3, s2a_conv_pack_weight_fp8, s2a_conv3x3_pyramid_fp8).

Shapes: a ragged pyramid (batch 2, levels 20x28, 10x14, 5x7, 3x3, C = 256: partial tiles in x and y, a level smaller than
a tile, two 128-channel chunks) and a one-level pyramid (batch 1, 9x17, C = 128: a single chunk, the one-level table).

  * exact integers: x_q in [-8, 8], w_q in [-4, 4] (all exact in e4m3), power-of-two scales, integer bias: every partial
    sum is an exact f32 integer (max |sum| ~ 2.5e3), so the f16 output must have the BITS of float64 -> f16.  Pins the
    operand lane maps, the tap order, the padding and the level table.
  * general data: random e4m3 operands, random f32 scale and bias, against oracle/conv64.py in float64 with
    w = deq(w_q) scale[o]:  f16 out |err| <= (2^-11 + 2 (K + 3) 2^-24) S + 2^-25;  e4m3 out, with t = clamp(y out_inv_scale,
    +-448): |deq(got) - t| <= 2^-4 |t| + 2^-10 + 2 (K + 3) 2^-24 S out_inv_scale.  (Products of two e4m3 values are exact in
    f32; the factor 2 over one rounding per accumulation step covers a rounding mode inside the matrix unit.)
    The output sits in a NaN-filled buffer between guard rows: every element is overwritten, the guards keep their bits, a
    second launch gives the same bits.
  * quantise: bit-equal to (x.float() * inv_scale).clamp(-448, 448).to(float8_e4m3fn) on random f16 and on a vector of
    edge values (zero, +-448, just above, ties, subnormal ties, +-inf, NaN)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PYRAMIDS = {"ragged": (2, [(20, 28), (10, 14), (5, 7), (3, 3)], 256), "one_level": (1, [(9, 17)], 128)}
O = 256
GUARD = 16
F8 = torch.float8_e4m3fn
_cache = {}


def to_e4m3(t):
    """float tensor -> uint8 e4m3fn bytes (CPU cast: the reference conversion)"""
    return t.float().cpu().clamp(-448, 448).to(F8).view(torch.uint8)


def deq(q):
    return q.cpu().view(F8).double()


def make_layout(pyr):
    from s2anet_amd.pyramid import PyramidLayout
    B, sizes, C = PYRAMIDS[pyr]
    return PyramidLayout(B, sizes, [8 * 2 ** i for i in range(len(sizes))]), C


def pack(wq):
    from s2anet_amd import _lib
    out = torch.empty(wq.numel(), dtype=torch.uint8, device=DEV)
    w = wq.to(DEV).contiguous()
    _lib.check(_lib.lib().s2a_conv_pack_weight_fp8(_lib.ptr(w), w.shape[0], w.shape[1], _lib.ptr(out), _lib.stream_ptr(w.device)))
    return out


def reference(layout, xq, wq, scale, bias):
    """float64 conv of the dequantised operands with w = deq(w_q) scale[o] -> per-level [(y, S)] on the CPU"""
    from oracle.conv64 import conv64
    x64 = deq(xq)
    w64 = deq(wq) * scale.double().cpu().view(-1, 1, 1, 1)
    return [conv64(layout.level(x64, l), w64, bias.double().cpu(), 1, 3) for l in range(len(layout.sizes))]


def case(pyr, kind):
    key = (pyr, kind)
    if key not in _cache:
        layout, C = make_layout(pyr)
        g = torch.Generator().manual_seed(len(pyr) * 7 + (kind == "int"))
        if kind == "int":
            xq = to_e4m3(torch.randint(-8, 9, (layout.pixels, C), generator=g))
            wq = to_e4m3(torch.randint(-4, 5, (O, C, 3, 3), generator=g))
            scale = 2.0 ** torch.randint(-3, 1, (O,), generator=g).float()
            bias = torch.randint(-20, 21, (O,), generator=g).float()
        else:
            xq = to_e4m3(torch.randn(layout.pixels, C, generator=g))
            wq = to_e4m3(torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** 0.5)
            scale = torch.rand(O, generator=g) * 1.5 + 0.5
            bias = torch.randn(O, generator=g) * 0.5
        assert int(((xq & 0x7f) == 0x7f).sum()) == 0 and int(((wq & 0x7f) == 0x7f).sum()) == 0
        _cache[key] = dict(layout=layout, C=C, xq=xq.to(DEV), packed=pack(wq), scale=scale.to(DEV), bias=bias.to(DEV),
                           ref=reference(layout, xq, wq, scale, bias))
    return _cache[key]


def launch(c, relu, out_e4m3=False, out_inv_scale=1.0):
    """into a NaN-filled buffer with guard rows before and behind -> (whole buffer, the [P,O] view)"""
    from s2anet_amd import pyramid as P
    rows = c["layout"].pixels
    if out_e4m3:
        buf = torch.full((rows + 2 * GUARD, O), 0x7f, dtype=torch.uint8, device=DEV)       # 0x7f: e4m3fn NaN
    else:
        buf = torch.full((rows + 2 * GUARD, O), float("nan"), dtype=torch.float16, device=DEV)
    view = buf[GUARD:GUARD + rows]
    got = P.conv3x3_fp8(c["layout"], c["xq"], c["packed"], c["scale"], c["bias"], O, relu, out_e4m3, out_inv_scale, out=view)
    assert got is view
    torch.cuda.synchronize()
    return buf, view


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t


def check_guards(buf, out_e4m3):
    raw = bits(buf)
    fill = raw.new_full((1,), 0x7f) if out_e4m3 else bits(torch.full((1,), float("nan"), dtype=torch.float16, device=DEV))
    assert bool((raw[:GUARD] == fill).all()) and bool((raw[-GUARD:] == fill).all()), "a guard row was written"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pyr", list(PYRAMIDS))
def test_exact_integer_operands_give_the_bits_of_float64(pyr, relu):
    c = case(pyr, "int")
    buf, got = launch(c, relu)
    check_guards(buf, False)
    assert not torch.isnan(got).any()
    layout = c["layout"]
    biggest = 0.0
    for l, (y, S) in enumerate(c["ref"]):
        want = (y.clamp_min(0) if relu else y).to(torch.float16)
        have = layout.level(got, l).cpu()
        biggest = max(biggest, S.max().item())
        bad = bits(have.contiguous()) != bits(want.contiguous())
        assert int(bad.sum()) == 0, (l, int(bad.sum()), (have.double() - want.double()).abs().max().item())
    assert biggest < 2 ** 24            # every partial sum is an exact f32 integer (times a power of two)
    assert (got != 0).float().mean().item() > 0.3


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pyr", list(PYRAMIDS))
def test_general_data_f16_out_against_float64(pyr, relu):
    c = case(pyr, "rand")
    buf, got = launch(c, relu)
    check_guards(buf, False)
    assert not torch.isnan(got).any()                                   # every element of [P,O] was written
    buf2, _ = launch(c, relu)
    assert torch.equal(bits(buf2), bits(buf))                           # and a second launch gives the same bits
    K = 9 * c["C"]
    tau = 2.0 ** -11 + 2 * (K + 3) * 2.0 ** -24
    layout, worst = c["layout"], 0.0
    for l, (y, S) in enumerate(c["ref"]):
        yl = y.clamp_min(0) if relu else y
        err = (layout.level(got, l).cpu().double() - yl).abs()
        bound = tau * S + 2.0 ** -25
        worst = max(worst, (err / bound).max().item())
        print("fp8 conv %s relu=%d level %d: max err/bound %.3g" % (pyr, relu, l, (err / bound).max().item()))
        assert int((~(err <= bound)).sum()) == 0, (l, worst)
    assert (got != 0).float().mean().item() > 0.3


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pyr", list(PYRAMIDS))
def test_general_data_e4m3_out_against_float64(pyr, relu):
    c = case(pyr, "rand")
    inv = 100.0                                                         # |y| reaches ~6: the top of the range saturates
    buf, got = launch(c, relu, True, inv)
    check_guards(buf, True)
    assert int(((got & 0x7f) == 0x7f).sum()) == 0                       # every element written, none of them NaN
    buf2, _ = launch(c, relu, True, inv)
    assert torch.equal(buf2, buf)
    K = 9 * c["C"]
    layout, worst, saturated = c["layout"], 0.0, 0
    for l, (y, S) in enumerate(c["ref"]):
        t = ((y.clamp_min(0) if relu else y) * inv).clamp(-448, 448)
        have = deq(layout.level(got, l).contiguous())
        err = (have - t).abs()
        bound = 2.0 ** -4 * t.abs() + 2.0 ** -10 + 2 * (K + 3) * 2.0 ** -24 * S * inv
        worst = max(worst, (err / bound).max().item())
        saturated += int((have.abs() == 448).sum())
        assert int((~(err <= bound)).sum()) == 0, (l, worst)
    print("fp8 conv %s relu=%d e4m3 out: max err/bound %.3g, %d saturated" % (pyr, relu, worst, saturated))
    assert saturated > 0 and (got != 0).float().mean().item() > 0.3


def test_exact_integer_operands_e4m3_out_is_one_rounding_of_float64():
    """integer case: v is an exact integer (times a power of two) -- the e4m3 output must be e4m3_rne(clamp(v / 2)) of the
    float64 value, bit for bit (one rounding, saturation at 448)"""
    c = case("one_level", "int")
    _, got = launch(c, True, True, 0.5)
    y, _ = c["ref"][0]
    want = to_e4m3(y.clamp_min(0) * 0.5)
    assert torch.equal(c["layout"].level(got, 0).cpu().contiguous(), want.contiguous())
    assert int((want == 0x7e).sum()) > 0                                # some values saturate (0x7e = 448)


def test_quantise_is_bit_equal_to_the_torch_cast():
    from s2anet_amd import pyramid as P
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(1488, 256, generator=g) * torch.exp(torch.randn(1488, 1, generator=g) * 3)).half()
    for inv in (1.0, 3.7, 448 / 5.3, 1e-3):
        got = P.quantize_e4m3(x.to(DEV), inv).cpu()
        want = (x.float() * inv).clamp(-448, 448).to(F8).view(torch.uint8)
        assert torch.equal(got, want), (inv, int((got != want).sum()))
    assert got.shape == x.shape


def test_quantise_edge_values():
    from s2anet_amd import pyramid as P
    s = 0.25
    vals = [0.0, -0.0, 448.0, -448.0, 449.0, 464.0, 480.0, -480.0, 1000.0, 17.0, 19.0, -17.0, -19.0, 2.0 ** -10, 1.5 * 2.0 ** -9,
            -(2.0 ** -10), 2.0 ** -9, 2.5 * 2.0 ** -9, 0.9 * 2.0 ** -10, 2.0 ** -6, 1.0625, 1.1875,
            float("inf"), float("-inf"), float("nan"), 431.0, 432.0, 447.0]
    x = torch.zeros(2, 16, dtype=torch.float16)
    x.view(-1)[:len(vals)] = (torch.tensor(vals, dtype=torch.float64) * s).half()
    assert torch.equal(x.view(-1)[:9].float() / s, torch.tensor(vals[:9]))      # exact in f16
    got = P.quantize_e4m3(x.to(DEV), 1 / s).cpu()
    want = (x.float() * (1 / s)).clamp(-448, 448).to(F8).view(torch.uint8)
    assert torch.equal(got, want), (got.view(-1)[:len(vals)].tolist(), want.view(-1)[:len(vals)].tolist())
    d = got.view(F8).float().view(-1)
    assert d[2] == 448 and d[4] == 448 and d[8] == 448 and d[7] == -448 and d[22] == 448 and d[23] == -448
    assert torch.isnan(d[24]) and d[9] == 16 and d[10] == 20 and d[13] == 0 and d[14] == 2.0 ** -8
