"""The case table of the dense convolutions' TRAINING kernels (s2anet_amd/csrc/conv_bwd_ops.hip), its inputs, the float64
references and the comparators shared by tests/test_train_conv_geometry_cpu.py (table, references and the exactness proof,
no GPU) and tests/test_gpu_train_conv_geometry.py (the C entry points on guarded buffers).

Inputs are exact by construction: every operand is k / 4, 1 <= |k| <= 8 (`dyadic`), so a product is a multiple of 2^-4 of
magnitude <= 4, and with at most MAX_TERMS = 4096 nonzero terms per output element every partial sum, in any order, is a
multiple of 2^-4 below 2^14: 18 bits, exact in f32.  An f32 result must therefore EQUAL the float64 sum and an f16 result be
that sum rounded once (`exact`); one dropped, doubled or misplaced term moves a result by >= 1/16 whatever the map size.  Maps
above DENSE_MAX positions take a sparse g (`sparse_positions`): nonzero at the first and last valid position of the first tile,
of the last tile and of the last tile of every slice, filled up with random positions to SPARSE_MAX.  (One case cannot keep
SPARSE_MAX: 513 tiles on 512 slices need two positions a slice, 1 025 in all; its term count stays under MAX_TERMS.)  The bias
gradient of the preparation pass sums single operands (multiples of 2^-2 of magnitude <= 2): 8 449 of them stay under 2^15,
17 bits.

Should the f16 MFMA not keep 24 bits in its running sum, a family is held to `bound` instead:
    |err| <= (n + slices + 17) u32 * S + 2^-25   (+ u16 |y| for an f16 output),   S = sum |g x| from float64,
which test_train_conv_geometry_cpu.py shows to stay below 1/32, half the smallest term, for every dyadic weight-gradient case
but the 1 025-position one and for every input-gradient case of at most 512 terms (above that the bound could not separate a
single term; on an MI355X no family needed it: every dyadic case is exact).  The Gaussian copies (GAUSS_*) are held to the same
bound with n the number of positions (input gradients: of terms).

ksplit(), s2_slices() and workspace_bytes() restate the launch geometry of conv_bwd_ops.hip; the CPU file holds them to the
library's own answers."""
import math
import zlib

import torch
import torch.nn.functional as F

from conv_geometry_cases import GUARD, TINY, U16, U32, Guarded      # noqa: F401  (Guarded: re-exported to the GPU file)

F16, F32, F64 = torch.float16, torch.float32, torch.float64
MAX_TERMS = 4096
DENSE_MAX = 600
SPARSE_MAX = 512
BAND = 2 * GUARD                  # bytes of fill on each side of a byte-typed guarded buffer: 64 KiB
NAN_BYTE, OTHER_BYTE = 0xFF, 0xA5        # 0xFF..: NaN in f16 and in f32; the second launch's fill


# ----------------------------------------------------------------------------- launch geometry, restated
def out_hw(H, W, stride):
    return ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if stride == 2 else (H, W)


def nowner(C, O, k):
    return (C // 64) * ((O + 255) // 256) * k


def ksplit(C, O, k):
    """position slices of the stride-1 weight gradient: the workgroups aimed at (256 / 512) over the owners"""
    return max(1, (256 if k == 3 else 512) // nowner(C, O, k))


def s2_slices(C, O, k):
    return min(ksplit(C, O, k), 32)


def ntiles(B, Hp, Wp, k):
    """position tiles on the map the positions live on: 4 x 16 of one image (3x3), 64 consecutive of the batch (1x1)"""
    return B * ((Hp + 3) // 4) * ((Wp + 15) // 16) if k == 3 else (B * Hp * Wp + 63) // 64


def workspace_bytes(C, O, k):
    blocks = max(ksplit(C, O, k) * nowner(C, O, k), 256 if k == 3 else 512)
    return (blocks * min(O, 256) * k * 64 * 4 + 255) // 256 * 256


def tile_corners(t, B, Hp, Wp, k):
    """first and last valid position of tile t, as flat indices into [B, Hp, Wp]"""
    if k == 1:
        return t * 64, min(t * 64 + 63, B * Hp * Wp - 1)
    tyn, txn = (Hp + 3) // 4, (Wp + 15) // 16
    b, r = divmod(t, tyn * txn)
    y0, x0 = (r // txn) * 4, (r % txn) * 16
    y1, x1 = min(y0 + 3, Hp - 1), min(x0 + 15, Wp - 1)
    return (b * Hp + y0) * Wp + x0, (b * Hp + y1) * Wp + x1


def sparse_positions(gen, B, Hp, Wp, k, slices):
    """sorted flat positions at which a sparse g is nonzero"""
    nt = ntiles(B, Hp, Wp, k)
    tiles = {0, nt - 1} | {s + slices * ((nt - 1 - s) // slices) for s in range(min(slices, nt))}
    need = sorted({p for t in tiles for p in tile_corners(t, B, Hp, Wp, k)})
    P = B * Hp * Wp
    extra = max(0, min(SPARSE_MAX, P) - len(need))
    if extra:
        free = torch.ones((P,), dtype=torch.bool)
        free[torch.tensor(need)] = False
        free = free.nonzero().view(-1)
        need = sorted(need + free[torch.randperm(free.numel(), generator=gen)[:extra]].tolist())
    return need


# ----------------------------------------------------------------------------- inputs
def gen_of(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def dyadic(gen, shape):
    """f16 values k / 4, 1 <= |k| <= 8, random sign: no zeros"""
    k = torch.randint(1, 9, tuple(shape), generator=gen)
    s = torch.randint(0, 2, tuple(shape), generator=gen) * 2 - 1
    return (k * s).to(F16) / 4


def gauss(gen, shape, scale=1.0):
    return (torch.randn(tuple(shape), generator=gen) * scale).to(F16)


def wgrad_inputs(c, kind="dyadic"):
    """x [B,H,W,C], g [B,Ho,Wo,O] f16 on the CPU; g sparse when the map has more than DENSE_MAX positions"""
    gen = gen_of(c["id"] + ":" + kind)
    draw = dyadic if kind == "dyadic" else gauss
    B, H, W, C, O, k, s = (c[n] for n in ("B", "H", "W", "C", "O", "k", "s"))
    Ho, Wo = out_hw(H, W, s)
    x = draw(gen, (B, H, W, C))
    if B * Ho * Wo <= DENSE_MAX:
        return x, draw(gen, (B, Ho, Wo, O))
    assert kind == "dyadic"
    at = torch.tensor(sparse_positions(gen, B, Ho, Wo, k, c["slices"]))
    g = torch.zeros((B * Ho * Wo, O), dtype=F16)
    g[at] = dyadic(gen, (at.numel(), O))
    return x, g.view(B, Ho, Wo, O)


def dgrad_inputs(c, kind="dyadic"):
    """g [B,Ho,Wo,O], w [O,C,k,k] f16 on the CPU"""
    gen = gen_of(c["id"] + ":" + kind)
    B, H, W, C, O, k, s = (c[n] for n in ("B", "H", "W", "C", "O", "k", "s"))
    Ho, Wo = out_hw(H, W, s)
    if kind == "dyadic":
        return dyadic(gen, (B, Ho, Wo, O)), dyadic(gen, (O, C, k, k))
    return gauss(gen, (B, Ho, Wo, O)), gauss(gen, (O, C, k, k), 1 / math.sqrt(k * k * O))


# ----------------------------------------------------------------------------- references (float64, on the CPU)
def wgrad_ref(x, g, k, stride):
    """gw[o,c,ky,kx] = sum over (b,oy,ox) of g[b,oy,ox,o] x[b, s oy + ky - pad, s ox + kx - pad, c], zero padding, over the
    positions at which g is nonzero -> (gw, S = the same sum of magnitudes, n = those positions' count), float64"""
    pad = k // 2
    O, C = g.shape[3], x.shape[3]
    at = (g != 0).any(-1).nonzero()
    b, oy, ox = at[:, 0], at[:, 1], at[:, 2]
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    gs = g[b, oy, ox].to(F64)
    gw, S = torch.zeros((O, C, k, k), dtype=F64), torch.zeros((O, C, k, k), dtype=F64)
    for ky in range(k):
        for kx in range(k):
            xs = xp[b, stride * oy + ky, stride * ox + kx].to(F64)
            gw[:, :, ky, kx] = gs.t() @ xs
            S[:, :, ky, kx] = gs.abs().t() @ xs.abs()
    return gw, S, int(at.shape[0])


def nchw(t):
    return t.permute(0, 3, 1, 2)


def wgrad_autograd(x, g, k, stride):
    """float64 autograd of F.conv2d for the filter -> [O,C,k,k]"""
    w = torch.zeros((g.shape[3], x.shape[3], k, k), dtype=F64, requires_grad=True)
    with torch.enable_grad():
        F.conv2d(nchw(x).to(F64), w, None, stride, k // 2).backward(nchw(g).to(F64))
    return w.grad


def dgrad_ref(g, w, H, W, stride):
    """float64 autograd of F.conv2d(x, w, None, stride, k // 2) for x -> (gx [B,H,W,C], S), NHWC"""
    k = w.shape[2]

    def run(g64, w64):
        x = torch.zeros((g.shape[0], w.shape[1], H, W), dtype=F64, requires_grad=True)
        with torch.enable_grad():
            F.conv2d(x, w64, None, stride, k // 2).backward(nchw(g64))
        return x.grad.permute(0, 2, 3, 1).contiguous()
    return run(g.to(F64), w.to(F64)), run(g.to(F64).abs(), w.to(F64).abs())


def dgrad_filter(w):
    """the header's formula: w'[c,o,ky,kx] = w[o,c,k-1-ky,k-1-kx]"""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def sum_pool_f32(g):
    """the header's order over f32, one rounding: ((g[2i,2j] + g[2i,2j+1]) + g[2i+1,2j]) + g[2i+1,2j+1]; g [B,H,W,O] f16"""
    f = g.float()
    return (((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2]).to(F16)


# ----------------------------------------------------------------------------- comparators
def as_f32_exactly(ref64):
    """the float64 sum as f32, asserting that nothing was rounded"""
    want = ref64.to(F32)
    assert torch.equal(want.to(F64), ref64), "the float64 reference is no f32 number: the inputs are not exact by construction"
    return want


def exact(got, ref64):
    """an f32 result equals the float64 sum, an f16 result is that sum rounded once; a NaN anywhere fails"""
    assert tuple(got.shape) == tuple(ref64.shape), (tuple(got.shape), tuple(ref64.shape))
    want = as_f32_exactly(ref64)
    return torch.equal(got, want.to(F16) if got.dtype == F16 else want)


def bound(n, slices, S, y, f16_out):
    b = (n + slices + 17) * U32 * S + TINY
    return b + U16 * y.abs() if f16_out else b


def bounded(got, ref64, S, n, slices):
    """-> (largest error over bound, all inside); a NaN anywhere fails"""
    assert tuple(got.shape) == tuple(ref64.shape), (tuple(got.shape), tuple(ref64.shape))
    err = (got.to(F64) - ref64).abs()
    b = bound(n, slices, S, ref64, got.dtype == F16)
    ratio = torch.nan_to_num(err / b, nan=math.inf).max().item()
    return ratio, bool((err <= b).all())


def mismatches(got, ref64):
    """for a failure message: how many elements differ and the first few"""
    want = ref64.to(got.dtype)
    bad = (got != want).nonzero()
    return "%d of %d differ; first %s got %s want %s" % (bad.shape[0], got.numel(), bad[:3].tolist(),
                                                      [got[tuple(i)].item() for i in bad[:3]],
                                                      [want[tuple(i)].item() for i in bad[:3]])


# ----------------------------------------------------------------------------- the table
def _wcase(fam, k, s, C, O, B, H, W, marks=()):
    Ho, Wo = out_hw(H, W, s)
    slices = ksplit(C, O, k) if s == 1 else s2_slices(C, O, k)
    nt = ntiles(B, Ho, Wo, k)
    m = set(marks)
    m.add("k%d s%d" % (k, s))
    for d, name in ((-1, "slices - 1"), (0, "slices"), (1, "slices + 1")):
        if nt == slices + d:
            m.add("tiles = %s, k = %d, s%d" % (name, k, s))
    if nt == 2 * slices + 1:
        m.add("tiles = 2 slices + 1, k = %d, s%d" % (k, s))
    if nt > slices:
        m.add("more tiles than slices, k = %d, s%d" % (k, s))
    if nt < slices:
        m.add("slices without a tile, k = %d, s%d" % (k, s))
    if O % 256 in (64, 192):
        m.add("idle mwave waves")
    if O % 256 == 64 and O > 256:
        m.add("a full 256-group and a 64 rest")
    if O == 512:
        m.add("two full 256-groups")
    if k == 3 and (Ho % 4 or Wo % 16):
        m.add("partial tile, k = 3, s%d" % s)
    if k == 3 and Ho % 4 and Wo % 16 and nt > slices:
        m.add("partial last tile row and column past the slices, k = 3, s%d" % s)
    if B > 1:
        m.add("B > 1, k = %d, s%d" % (k, s))
    if B * Ho * Wo > DENSE_MAX:
        m.add("sparse g")
    if k == 1 and B > 1 and (Ho * Wo) % 64:
        m.add("a 1x1 tile spans images, s%d" % s)
    if s == 2:
        m.add("H %s, W %s" % ("odd" if H % 2 else "even", "odd" if W % 2 else "even"))
        if k == 3 and Wo in (16, 17):
            m.add("Wo = %d on the 33-pixel patch row" % Wo)
    return dict(id="%s-k%ds%d-c%do%d-b%dx%dx%d" % (fam, k, s, C, O, B, H, W), fam=fam, k=k, s=s, C=C, O=O, B=B, H=H, W=W,
                slices=slices, tiles=nt, marks=frozenset(m))


# 1. s2a_conv_backward_weight_f16, k = 3
W3_PAIRS = ((64, 64), (128, 64), (64, 192), (64, 256), (64, 320), (128, 512))
W3_GEOMS = ((1, 1, 1), (1, 1, 16), (1, 1, 17), (1, 4, 16), (1, 5, 16), (1, 3, 15), (1, 4, 33), (1, 9, 1), (3, 5, 17))
# tile counts ksplit - 1, ksplit, ksplit + 1, 2 ksplit + 1.  (64, 64): ksplit 85 -> 6 x 14, 17 x 5 (65 x 65: a partial last
# tile row and column), 43 images of 2 x 1, 3 images of 3 x 19; (128, 512): ksplit 21 -> 5 x 4 (partial both ways), 3 x 7,
# 2 images of 1 x 11, 43 images of one.  No row of x is wider than 64 KiB.
W3_COUNTS = {(64, 64): ((1, 24, 209), (1, 65, 65), (43, 5, 3), (3, 9, 301)),
             (128, 512): ((1, 18, 50), (1, 9, 100), (2, 2, 175), (43, 2, 3))}
# 2. the same, k = 1: 1, 63, 64, 65 and 189 positions
W1_PAIRS = ((64, 64), (512, 128), (64, 320), (512, 512))
W1_GEOMS = ((1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 5, 13), (3, 7, 9))
# (512, 512): ksplit 32 -> 31 tiles; 2 047, 2 048, 2 049 positions (32, 32, 33 tiles); 65 tiles.  (64, 64): 513 tiles on 512 slices
W1_COUNTS = {(512, 512): ((1, 31, 64), (1, 23, 89), (2, 32, 32), (3, 1, 683), (1, 41, 100)), (64, 64): ((3, 1, 10923),)}
# 3. s2a_conv_backward_weight_s2_f16 + _reduce
S2_H, S2_W = (1, 2, 7, 8, 9, 10), (1, 2, 31, 32, 33, 34)
S2_GRID = tuple((1, h, w) for h in S2_H for w in S2_W)
S2_DIAG = tuple((2, h, w) for h, w in zip(S2_H, S2_W))
WS3_PAIRS = ((64, 128), (128, 256), (128, 384))             # the first runs the whole grid, the others its diagonal at B = 2
WS1_PAIRS = ((64, 64), (512, 128), (64, 320))
# 31, 32, 33 and 65 tiles on 32 slices: output maps of 31 images of one tile, 2 x (2 x 8), 3 x 11, 5 x 13 (k = 3); of 1 922,
# 2 048, 2 079 and 4 100 positions (k = 1)
WS3_COUNTS = ((31, 3, 5), (2, 13, 251), (1, 18, 322), (1, 34, 400))
WS1_COUNTS = ((1, 61, 124), (2, 63, 64), (1, 65, 125), (1, 81, 200))
WS1_SPAN = (3, 13, 17)                                       # 3 images of 7 x 9 outputs: a tile spans three images


def _wgrad_cases():
    out = []
    for C, O in W3_PAIRS:
        out += [_wcase("w3", 3, 1, C, O, *g) for g in W3_GEOMS + W3_COUNTS.get((C, O), ())]
    for C, O in W1_PAIRS:
        out += [_wcase("w1", 1, 1, C, O, *g) for g in W1_GEOMS + W1_COUNTS.get((C, O), ())]
    for i, (C, O) in enumerate(WS3_PAIRS):
        out += [_wcase("ws3", 3, 2, C, O, *g) for g in (S2_GRID + WS3_COUNTS if i == 0 else S2_DIAG)]
    for i, (C, O) in enumerate(WS1_PAIRS):
        out += [_wcase("ws1", 1, 2, C, O, *g) for g in (S2_GRID + WS1_COUNTS + (WS1_SPAN,) if i == 0 else S2_DIAG)]
    return tuple(out)


WGRAD_CASES = _wgrad_cases()
WGRAD_S1 = tuple(c for c in WGRAD_CASES if c["s"] == 1)
WGRAD_S2 = tuple(c for c in WGRAD_CASES if c["s"] == 2)


def _first_dense(cases, fam):
    """one case per (C, O) of a family: the dense one with the most positions"""
    best = {}
    for c in cases:
        Ho, Wo = out_hw(c["H"], c["W"], c["s"])
        P = c["B"] * Ho * Wo
        if c["fam"] == fam and P <= DENSE_MAX and P > best.get((c["C"], c["O"]), (0, None))[0]:
            best[(c["C"], c["O"])] = (P, c)
    return tuple(v[1] for v in best.values())


GAUSS_WGRAD = sum((_first_dense(WGRAD_CASES, f) for f in ("w3", "w1", "ws3", "ws1")), ())


# 4. s2a_conv_backward_input_s2_f16; 5. the stride-1 input gradient through s2a_conv_nhwc_f16
def dcase(fam, k, s, C, O, B, H, W):
    Ho, Wo = out_hw(H, W, s)
    m = {"k%d s%d" % (k, s)}
    if s == 2:
        m.add("H %s, W %s" % ("odd" if H % 2 else "even", "odd" if W % 2 else "even"))
        tyn, txn = (Ho + 3) // 4, (Wo + 15) // 16
        if any(4 * i + 4 < Ho and 16 * j + 16 < Wo for i in range(tyn) for j in range(txn)):
            m.add("edge-free s2 input tile")
        if Ho % 4 or Wo % 16:
            m.add("partial s2 input tile")
    if B > 1:
        m.add("B > 1, k = %d, s%d" % (k, s))
    return dict(id="%s-k%ds%d-c%do%d-b%dx%dx%d" % (fam, k, s, C, O, B, H, W), fam=fam, k=k, s=s, C=C, O=O, B=B, H=H, W=W,
                terms=(O * (4 if s == 2 else 9) if k == 3 else O), marks=frozenset(m))


D3_PAIRS = tuple((C, O) for C in (64, 128, 192) for O in (128, 256, 384))
D1_PAIRS = tuple((C, O) for C in (64, 128, 192) for O in (64, 320))
D_FREE = (1, 18, 66)                                         # 9 x 33 quads: the first tile has no edge quad
DS1_PAIRS = ((64, 128), (64, 320), (512, 128))
DS1_GEOMS = ((1, 5, 17), (3, 4, 16))


def _dgrad_cases():
    out = []
    for k, pairs in ((3, D3_PAIRS), (1, D1_PAIRS)):
        for i, (C, O) in enumerate(pairs):
            out += [dcase("d%d" % k, k, 2, C, O, *g) for g in (S2_GRID if i == 0 else S2_DIAG) + (D_FREE,)]
    return tuple(out)


DGRAD_S2 = _dgrad_cases()
DGRAD_S1 = tuple(dcase("ds", k, 1, C, O, *g) for C, O in DS1_PAIRS for k in (1, 3) for g in DS1_GEOMS)
GAUSS_DGRAD = tuple(c for c in DGRAD_S2 if (c["B"], c["H"], c["W"]) == (2, 9, 33)) + \
    tuple(c for c in DGRAD_S2 if (c["B"], c["H"], c["W"]) == (1, 9, 33)) + tuple(c for c in DGRAD_S1 if c["B"] == 1)

# 6. s2a_conv_pack_weight_train: (O, C, k)
PACK_SIZES = ((64, 64, 1), (64, 128, 3), (320, 64, 3), (128, 512, 1))
# what the f32 masters must hold besides Gaussian values: ties (round to even: down, up), values around f16's largest
# (65 504; 65 520 is the tie that rounds to inf), subnormal results with a tie among them, both signs
PACK_PLANTS = (1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 65519.0, 65520.0, 70000.0, -70000.0, 3e-6, -3e-6,
               2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -24, 1e-9)


def pack_master(O, C, k, dtype):
    gen = gen_of("pack-%d-%d-%d" % (O, C, k))
    w = torch.randn((O, C, k, k), generator=gen) / math.sqrt(k * k * C)
    if dtype == F32:
        at = torch.randperm(w.numel(), generator=gen)[:len(PACK_PLANTS)]
        w.view(-1)[at] = torch.tensor(PACK_PLANTS, dtype=F32)
    return w.to(dtype)


# 7. s2a_conv_backward_prep_f16: one row per workgroup ... the 256-workgroup cap, 33-row workgroups, 34-row workgroups
PREP_P = (1, 31, 32, 33, 8191, 8192, 8193, 8449)
PREP_O = (64, 128, 320)
# (out given, g wanted, bias gradient dtype or None) of a call that launches
PREP_CALLS = ((True, True, F32), (True, True, F16), (True, True, None), (True, False, F32), (True, False, F16),
              (False, False, F32), (False, False, F16))
PREP_SPECIALS = (0.0, -0.0, 2.0 ** -24, 2.0 ** -15, float("nan"), -(2.0 ** -24))


def prep_geometry(P):
    """(workgroups, rows per workgroup, workgroups that own no row) of k_conv_bwd_prep"""
    nb = min(max((P + 31) // 32, 1), 256)
    rows = (P + nb - 1) // nb
    return nb, rows, sum(1 for b in range(nb) if b * rows >= P)


def prep_inputs(P, O):
    """grad_out dyadic; out dyadic (half of it below 0) with each of PREP_SPECIALS at eight random places"""
    gen = gen_of("prep-%d-%d" % (P, O))
    go = dyadic(gen, (P, O))
    out = dyadic(gen, (P, O))
    n = P * O
    at = torch.randperm(n, generator=gen)[:min(n, 8 * len(PREP_SPECIALS))]
    out.view(-1)[at] = torch.tensor(PREP_SPECIALS, dtype=F16).repeat(8)[:at.numel()]
    return go, out


# 8. s2a_sum_pool2x2_f16: (B, H, W, O)
POOL_SHAPES = ((1, 2, 2, 8), (1, 6, 10, 72), (3, 2, 34, 256), (2, 8, 8, 256))
POOL_GAUSS = (1, 6, 10, 72)

# 9. zero times infinity at partial tiles: (stride, C, O, B, H, W), k = 3
INF_CASES = ((1, 64, 64, 1, 5, 17), (1, 64, 64, 1, 4, 16), (2, 64, 128, 1, 10, 22), (2, 64, 128, 1, 9, 21))
INF_CHANNEL = 5


def mechanisms():
    """every named mechanism the tables reach"""
    m = set()
    for c in WGRAD_CASES + DGRAD_S2 + DGRAD_S1:
        m |= c["marks"]
    for P in PREP_P:
        nb, rows, empty = prep_geometry(P)
        m.add("prep rows = %d%s" % (rows, " with empty workgroups" if empty else ""))
        if nb == 256:
            m.add("prep at the 256-workgroup cap")
    return m
