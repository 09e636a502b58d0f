"""The dense f16 convolution case matrix (s2anet_amd/csrc/conv_ops.hip), its inputs, the bounds and the one comparator
shared by tests/test_conv_geometry_cpu.py (which checks the table, the reference and the bound without a GPU) and
tests/test_gpu_conv_geometry.py (which holds every instantiation of k_conv_f16, the pyramid-packed launches and the fused
trunk forms to the float64 reference of oracle/conv64.py).

A case fixes all four tile-shape switches, so the instantiation it runs is a function of (ksize, stride, C, O, switches)
alone: route() below, the tests' own statement of the dispatch, which tests/test_conv_geometry_cpu.py holds to the library's
answer (s2a_conv_nhwc_f16_form), the default thresholds included.  The geometries are the smallest at which each mechanism of a tile
kernel can still go wrong, chosen per instantiation from its tile shape; inputs are drawn on the CPU from a generator
seeded by the case id, so both files see the same numbers.

Bound (the formulas of tests/test_gpu_forward_shapes.py, restated; the CPU test asserts they agree), K = taps * C:
    |got - y| <= tau * S + 2^-25        and        ||got - y|| / ||y|| <= 2 u16
    conv      exact f16 products summed in f32 (K u32), + bias in f32, ONE f16 rounding, ReLU on the rounded value
                                                                                      -> u16 + (K + 17) u32
    conv_res  rnd16(rnd16(acc + b) + r): the residual / up-2 coarse epilogue rounds twice -> 2 u16 + (K + 17) u32
K is used at border pixels too (fewer taps: an upper bound, and S shrinks there)."""
import math
import zlib

import torch

U16, U32 = 2.0 ** -11, 2.0 ** -24
TINY = 2.0 ** -25                 # half an f16 subnormal step: the absolute floor of an underflowed result
L2_BOUND = 2 * U16
GUARD = 32768                     # f16 elements of NaN on each side of a guarded tensor: 64 KiB
NAN = float("nan")


def tau(kind, K):
    return {"conv": U16 + (K + 17) * U32, "conv_res": 2 * U16 + (K + 17) * U32}[kind]


# ----------------------------------------------------------------------------- routes
SWITCHES = ("S2A_CONV_PH_NARROW", "S2A_CONV_PH", "S2A_CONV3_HALF", "S2A_CONV1_HALF")


def switches(ph_narrow=1, ph=1, half3=0, half1=0):
    return {"S2A_CONV_PH_NARROW": str(ph_narrow), "S2A_CONV_PH": str(ph), "S2A_CONV3_HALF": str(half3),
            "S2A_CONV1_HALF": str(half1)}


def og_of(O):
    return 4 if O % 256 == 0 else (2 if O % 128 == 0 else 1)


def route(ksize, stride, C, O, sw, B=None, H=None, W=None):
    """the k_conv_f16<TAPS, OG, PH, SD, false, HT> that s2a_conv_nhwc_f16 launches -> (TAPS, OG, PH, SD, HT).  A switch
    absent from sw is decided by the entry point's threshold on the launch's workgroup count, which needs B, H, W:
    16 x 16 tiles from 256 (OG 1, 2) / 512 (OG 4) workgroups on, 4 x 16 tiles and 64-position 1x1 tiles below 256
    workgroups of the 8 x 16 / 128-position form"""
    assert set(sw) <= set(SWITCHES) and ksize in (1, 3) and stride in (1, 2)
    assert (C % 64 == 0 or C == 32) and O % 64 == 0 and not (ksize == 3 and stride == 2 and O % 128)
    og = og_of(O)
    groups = (O + 64 * og - 1) // (64 * og)
    Ho, Wo = out_hw(H, W, stride) if set(sw) != set(SWITCHES) else (None, None)

    def tiles(rows):
        return B * ((Wo + 15) // 16) * ((Ho + rows - 1) // rows) * groups

    def tall(name, least):
        return sw[name] == "2" if name in sw else tiles(16) >= least

    def half(name, wgs):
        return int(sw[name]) != 0 if name in sw else wgs() < 256

    if ksize == 3 and stride == 2:
        return (9, 4 if og == 4 else 2, 1, 2, 0)
    if ksize == 3:
        if og < 4 and C % 64 == 0 and tall("S2A_CONV_PH_NARROW", 256):
            return (9, og, 2, 1, 0)
        if og == 4 and C % 64 == 0 and tall("S2A_CONV_PH", 512):
            return (9, 4, 2, 1, 0)
        if og >= 2 and half("S2A_CONV3_HALF", lambda: tiles(8)):
            return (9, og, 1, 1, 1)
        return (9, og, 1, 1, 0)
    if og == 4 and half("S2A_CONV1_HALF", lambda: (B * Ho * Wo + 127) // 128 * groups):
        return (1, 4, 1, 2, 0)            # (SD = 2 selects the 64-position tile of a 1x1; its stride is cstride)
    return (1, og, 1, 1, 0)


def tile_rows(inst):
    """rows of the rows x 16 output tile of a 3x3 instantiation"""
    taps, og, ph, sd, ht = inst
    assert taps == 9
    return 4 if (sd == 2 or ht) else 8 * ph


def tile_positions(inst):
    """consecutive output positions of the whole batch per workgroup of a 1x1 instantiation"""
    taps, og, ph, sd, ht = inst
    assert taps == 1
    return 64 if sd == 2 else 128


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def grid_x(inst, B, H, W, stride):
    """gridDim.x of the launch (launch_conv)"""
    Ho, Wo = out_hw(H, W, stride)
    if inst[0] == 9:
        R = tile_rows(inst)
        return B * ((Wo + 15) // 16) * ((Ho + R - 1) // R)
    P = tile_positions(inst)
    return (B * Ho * Wo + P - 1) // P


def inst_name(inst):
    return "k%d.og%d.ph%d.sd%d.ht%d" % inst


# ----------------------------------------------------------------------------- epilogues
EPILOGUES = (dict(name="bias_relu", bias=True, res=False, relu=True),
             dict(name="plain", bias=False, res=False, relu=False),
             dict(name="bias_res_relu", bias=True, res=True, relu=True),
             dict(name="res", bias=False, res=True, relu=False))


def kind_of(epi):
    return "conv_res" if epi["res"] else "conv"


# ----------------------------------------------------------------------------- geometries (B, H, W)
def geoms_3x3(R):
    """3x3 / stride 1 on R x 16 tiles: only the centre tap inside; a one-pixel-wide map crossing a tile boundary either
    way; under one tile both ways (B = 3: the halo rows of the middle image border real data of its neighbours);
    exactly one tile; one row and one column into the next tile; (2R - 1) x 31"""
    return ((1, 1, 1), (1, 1, 17), (1, 17, 1), (1, 3, 5), (3, 3, 5), (1, R, 16), (1, R + 1, 17), (3, R + 1, 17),
            (1, 2 * R - 1, 31))


# 3x3 / stride 2, 4 x 16 output tiles from 9 x 33 patches; odd and even H, W: both roundings of Ho = (H - 1) / 2 + 1
GEOMS_3X3_S2 = ((1, 1, 1), (1, 2, 2), (1, 3, 3), (3, 3, 3), (1, 8, 32), (1, 9, 33), (3, 9, 33), (1, 7, 66))


def geoms_1x1(P, stride):
    """1x1 on P consecutive positions of the whole batch: B * Ho * Wo = 1, P - 1, P, P + 1, and B = 3 of 7 x 9 outputs
    (189 positions: a tile boundary inside the second image, an image boundary inside a tile); at stride 2 from an odd
    and from an even map"""
    if stride == 1:
        return ((1, 1, 1), (1, 1, P - 1), (1, 8, P // 8), (1, 1, P + 1), (3, 7, 9))
    return ((1, 1, 1), (1, 2, 2 * (P - 1)), (1, 15, 2 * (P // 8)), (1, 1, 2 * P + 1), (3, 13, 17), (3, 14, 18))


def geoms_count(inst, stride):
    """launches whose gridDim.x is 7, 8, 9 and 13 (xcd_remap permutes workgroups differently for n % 8 != 0); 3x3: one
    row of tiles, the nine as three images of three tiles"""
    if inst[0] == 9:
        wo = lambda n: 16 * n - 3
        wi = (lambda n: wo(n)) if stride == 1 else (lambda n: 2 * wo(n) - 1)
        return ((1, 1, wi(7)), (1, 1, wi(8)), (3, 1, wi(3)), (1, 1, wi(13)))
    P = tile_positions(inst)
    return tuple((1, 1, n * P - 5) for n in (7, 8, 9, 13))


def pair_geoms(inst):
    """exactly one tile, and one past it"""
    if inst[0] == 9 and inst[3] == 2:
        return ((1, 8, 32), (1, 9, 33))
    if inst[0] == 9:
        R = tile_rows(inst)
        return ((1, R, 16), (1, R + 1, 17))
    P = tile_positions(inst)
    return ((1, 8, P // 8), (1, 1, P + 1))


# ----------------------------------------------------------------------------- the table
CHANNELS = (32, 64, 128, 192, 512)      # half-filled chunk; one chunk; two; three (the loop ends on the odd buffer); steady state


def _pairs(oa, ob, with32=True):
    """every C once, the two O of the instantiation in turn"""
    cs = CHANNELS if with32 else CHANNELS[1:]
    return tuple((c, (oa, ob)[i % 2]) for i, c in enumerate(cs))


# instantiation -> ksize, strides, switches, the (C, O) every geometry runs at, the (C, O) pairs that run at two
# geometries.  O = 64 / 320: og 1 with one / five groups; 128 / 384: og 2 with one / three; 256 / 512: og 4 with one / two
# (blockIdx.y > 0 for every OG).  C = 32 only where the entry point lets it through (the filter-through-LDS forms need
# C % 64 == 0).
INSTANTIATIONS = (
    dict(inst=(9, 4, 1, 2, 0), k=3, strides=(2,), sw=switches(), home=(128, 512), pairs=_pairs(256, 512)),
    dict(inst=(9, 2, 1, 2, 0), k=3, strides=(2,), sw=switches(), home=(192, 384), pairs=_pairs(128, 384)),
    dict(inst=(9, 2, 2, 1, 0), k=3, strides=(1,), sw=switches(ph_narrow=2), home=(128, 384), pairs=_pairs(128, 384, False)),
    dict(inst=(9, 1, 2, 1, 0), k=3, strides=(1,), sw=switches(ph_narrow=2), home=(192, 320), pairs=_pairs(64, 320, False)),
    dict(inst=(9, 4, 2, 1, 0), k=3, strides=(1,), sw=switches(ph=2), home=(128, 512), pairs=_pairs(256, 512, False)),
    dict(inst=(9, 4, 1, 1, 1), k=3, strides=(1,), sw=switches(half3=1), home=(192, 512), pairs=_pairs(256, 512)),
    dict(inst=(9, 2, 1, 1, 1), k=3, strides=(1,), sw=switches(half3=1), home=(128, 384), pairs=_pairs(128, 384)),
    dict(inst=(9, 4, 1, 1, 0), k=3, strides=(1,), sw=switches(), home=(192, 512), pairs=_pairs(256, 512)),
    dict(inst=(9, 2, 1, 1, 0), k=3, strides=(1,), sw=switches(), home=(128, 384), pairs=_pairs(128, 384)),
    dict(inst=(9, 1, 1, 1, 0), k=3, strides=(1,), sw=switches(), home=(192, 320), pairs=_pairs(64, 320)),
    dict(inst=(1, 4, 1, 2, 0), k=1, strides=(1, 2), sw=switches(half1=1), home=(192, 512), pairs=_pairs(256, 512)),
    dict(inst=(1, 4, 1, 1, 0), k=1, strides=(1, 2), sw=switches(), home=(128, 512), pairs=_pairs(256, 512)),
    dict(inst=(1, 2, 1, 1, 0), k=1, strides=(1, 2), sw=switches(), home=(192, 384), pairs=_pairs(128, 384)),
    dict(inst=(1, 1, 1, 1, 0), k=1, strides=(1, 2), sw=switches(), home=(128, 320), pairs=_pairs(64, 320)),
)
ALL_INSTANTIATIONS = tuple(i["inst"] for i in INSTANTIATIONS)
# one instantiation per family carries the tile-count launches
COUNTED = ((9, 4, 1, 1, 0), (9, 1, 2, 1, 0), (9, 2, 1, 2, 0), (1, 1, 1, 1, 0), (1, 4, 1, 2, 0))
GRID_X_WANTED = (1, 7, 8, 9, 13)


def _case(spec, stride, C, O, B, H, W, epis, why):
    inst = route(spec["k"], stride, C, O, spec["sw"])
    assert inst == spec["inst"], (spec["inst"], inst, C, O)
    cid = "%s-%dx%ds%d-c%do%d-b%dx%dx%d" % (inst_name(inst), spec["k"], spec["k"], stride, C, O, B, H, W)
    return dict(id=cid, inst=inst, k=spec["k"], s=stride, sw=spec["sw"], C=C, O=O, B=B, H=H, W=W, epis=tuple(epis), why=why,
                grid_x=grid_x(inst, B, H, W, stride), K=spec["k"] ** 2 * C)


def _build():
    cases = {}

    def add(c):
        old = cases.get(c["id"])
        if old is not None:             # the same launch from two rules: the union of the epilogues
            c = dict(old, epis=tuple(sorted(set(old["epis"]) | set(c["epis"]))), why=old["why"] + "+" + c["why"])
        cases[c["id"]] = c

    every = range(len(EPILOGUES))
    for spec in INSTANTIATIONS:
        inst = spec["inst"]
        for stride in spec["strides"]:
            if inst[0] == 9:
                geos = GEOMS_3X3_S2 if stride == 2 else geoms_3x3(tile_rows(inst))
            else:
                geos = geoms_1x1(tile_positions(inst), stride)
            for B, H, W in geos:
                add(_case(spec, stride, *spec["home"], B, H, W, every, "geometry"))
        if inst in COUNTED:
            for B, H, W in geoms_count(inst, spec["strides"][0]):
                add(_case(spec, spec["strides"][0], *spec["home"], B, H, W, (0, 2), "count"))
        for C, O in spec["pairs"]:
            (one, past) = pair_geoms(inst)
            add(_case(spec, spec["strides"][0], C, O, *one, (0, 3), "pair"))
            add(_case(spec, spec["strides"][0], C, O, *past, (1, 2), "pair"))
    return tuple(cases.values())


CASES = _build()


# ----------------------------------------------------------------------------- inputs
def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def draw(gen, B, H, W, C, O, k, Ho, Wo):
    """f16 CPU tensors: x [B,H,W,C] ~ N(0,1), w [O,C,k,k] ~ N(0,1) / sqrt(taps C) (outputs of order 1), bias [O] and
    residual [B,Ho,Wo,O] ~ N(0,1)"""
    return dict(x=torch.randn((B, H, W, C), generator=gen).half(),
                w=(torch.randn((O, C, k, k), generator=gen) / math.sqrt(k * k * C)).half(),
                bias=torch.randn((O,), generator=gen).half(),
                res=torch.randn((B, Ho, Wo, O), generator=gen).half())


def make_inputs(c):
    Ho, Wo = out_hw(c["H"], c["W"], c["s"])
    return draw(_gen(c["id"]), c["B"], c["H"], c["W"], c["C"], c["O"], c["k"], Ho, Wo)


def nchw(t):
    """[B,H,W,C] storage -> the channels-last [B,C,H,W] view the entry points take"""
    return t.permute(0, 3, 1, 2)


class Guarded:
    """a tensor as a view into a larger f16 buffer filled with NaN: >= 64 KiB of NaN on each side, the view at a
    16-byte-aligned element offset.  A read outside the tensor shows up as a NaN, a write outside it as a non-NaN in a
    band -- inside one allocation, so a wrong index is a failed assertion and not a fault.
    values: an f16 tensor (copied in), or a shape (the view stays NaN: an output)."""

    def __init__(self, values, device):
        shape = tuple(values.shape) if torch.is_tensor(values) else tuple(values)
        self.n = math.prod(shape)
        self.lo = GUARD
        self.hi = self.lo + self.n
        self.buf = torch.full((self.hi + GUARD + 8,), NAN, dtype=torch.float16, device=device)
        self.flat = self.buf[self.lo:self.hi]
        assert self.flat.data_ptr() % 16 == 0
        if torch.is_tensor(values):
            self.flat.copy_(values.reshape(-1))
        self.t = self.flat.view(shape)

    def bands_untouched(self):
        return bool(self.buf[:self.lo].isnan().all()) and bool(self.buf[self.hi:].isnan().all())

    def all_written(self):
        return not bool(self.flat.isnan().any())


# ----------------------------------------------------------------------------- reference, comparator, emulation
def reference(c, inp, epi):
    """oracle.conv64 of a case under an epilogue, on the device the inputs are on -> (y, S) [B,O,Ho,Wo] float64"""
    from oracle.conv64 import conv64
    return conv64(nchw(inp["x"]), inp["w"], inp["bias"] if epi["bias"] else None, c["s"], c["k"],
                  residual=nchw(inp["res"]) if epi["res"] else None, relu=epi["relu"])


def compare(got, y, S, kind, K):
    """THE comparator: every element within tau * S + 2^-25 and the relative L2 error within 2 u16.
    -> dict(ratio = largest error over bound, l2_ratio, ok).  A NaN anywhere fails."""
    assert tuple(got.shape) == tuple(y.shape), (tuple(got.shape), tuple(y.shape))
    err = (got.detach().double() - y).abs()
    bound = tau(kind, K) * S + TINY
    ratio = torch.nan_to_num(err / bound, nan=math.inf).max().item()
    l2 = err.norm().item() / max(y.norm().item(), 1e-300)
    l2 = l2 if math.isfinite(l2) else math.inf
    ok = bool((err <= bound).all()) and l2 <= L2_BOUND
    return dict(ratio=ratio, l2=l2, l2_ratio=l2 / L2_BOUND, ok=ok, nonzero=(got != 0).double().mean().item())


def emulate(c, inp, epi):
    """the kernel's arithmetic on the CPU: f16 operands, an f32 convolution, the bias in f32, one f16 rounding, the
    second rounding behind the residual, ReLU on the rounded value -> f16 [B,O,Ho,Wo]"""
    import torch.nn.functional as F
    acc = F.conv2d(nchw(inp["x"]).float(), inp["w"].float(), None, c["s"], (c["k"] - 1) // 2)
    if epi["bias"]:
        acc = acc + inp["bias"].float().view(1, -1, 1, 1)
    v = acc.half()
    if epi["res"]:
        v = (v.float() + nchw(inp["res"]).float()).half()
    return v.clamp_min(0) if epi["relu"] else v


# ----------------------------------------------------------------------------- pyramid-packed launches
def _halving(h, w, n):
    out = [(h, w)]
    while len(out) < n:
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return tuple(out)


# one level (the entry point's lt.n == 1 -> 2 patch-up); two levels; eight, 33 x 17 down to 1 x 1 halving and rounding up
PYRAMIDS = {"one": ((5, 7),), "two": ((17, 9), (1, 1)), "eight": _halving(33, 17, 8)}
PYRAMID_BATCHES = (1, 3)
PYRAMID_CONV_PAIRS = ((32, 256), (64, 128), (256, 64), (256, 256))       # (C, O); O = 256 runs S2A_CONV_PH both ways
PYRAMID_POOL_PAIRS = ((32, 64), (64, 256), (256, 128), (256, 256))
PYRAMID_HEAD_CHANNELS = ((32, 5), (64, 15), (256, 5))                     # (C, head maps); the tower has 256


def pyramid_cases(pairs):
    return tuple(dict(id="%s-b%d-c%do%d" % (name, B, C, O), levels=PYRAMIDS[name], B=B, C=C, O=O)
                 for name in PYRAMIDS for B in PYRAMID_BATCHES for C, O in pairs)


def pyramid_inputs(cid, levels, B, C, O, extra=()):
    """packed f16 CPU tensors: x [P,C], w [O,C,3,3], bias [O], res [P,O]; extra: (name, shape, scale) draws behind them"""
    gen = _gen("pyramid-" + cid)
    P = B * sum(h * w for h, w in levels)
    r = dict(x=torch.randn((P, C), generator=gen).half(), w=(torch.randn((O, C, 3, 3), generator=gen) / math.sqrt(9 * C)).half(),
             bias=torch.randn((O,), generator=gen).half(), res=torch.randn((P, O), generator=gen).half())
    for name, shape, scale in extra:
        r[name] = (torch.randn(shape, generator=gen) * scale).half()
    return r


# ----------------------------------------------------------------------------- fused trunk forms
TAIL_SIZES = ((1, 1), (3, 5), (8, 16), (9, 17))
TAIL_BATCHES = (1, 3)
TAIL_FORMS = ((False, None), (True, None), (False, 64), (True, 64), (True, 128), (False, 128))      # (residual, chain maps)
CHAIN_SHAPES = ((128, 512, 128), (128, 512, 256), (256, 1024, 256))       # (K, O, O3) of s2a_conv1x1_chain_f16
CHAIN_GEOMS = ((1, 1, 1), (1, 1, 127), (1, 8, 16), (1, 1, 129), (3, 7, 9))     # 1, 127, 128, 129 and 3 x 63 positions
UP2_SIZES = ((2, 2), (2, 34), (16, 16), (18, 34))
UP2_CHANNELS = ((64, 64), (64, 256), (192, 64), (192, 256))
UP2_BATCHES = (1, 3)
