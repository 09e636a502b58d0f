"""CPU: the float64 forward references (oracle/conv64.py) that hold the benchmarked forward's launches are pinned here:
conv64 against F.conv2d in float64 (1x1 / 3x3, stride 1 / 2, odd and even sizes, residual, up-2 residual, ReLU), stem64
against F.conv2d + relu + max_pool2d, the stem's u8 table against torch's half division, rot_pool64, and every error
scale (S, S_corner) against brute-force sums at sampled entries."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.conv64 import align64, conv64, rot_pool64, stem64, u8_to_f16
from oracle.dcn64 import deform_conv64, sample_points

F64 = torch.float64


def rnd(g, *shape, scale=1.0):
    return (torch.randn(shape, generator=g, dtype=F64) * scale).half()


CASES = [  # B, C, H, W, O, k, stride
    (2, 16, 9, 13, 24, 3, 1), (1, 8, 10, 12, 16, 3, 1), (2, 16, 9, 13, 32, 3, 2), (1, 8, 10, 12, 8, 3, 2),
    (2, 24, 7, 11, 16, 1, 1), (1, 16, 10, 8, 32, 1, 2), (2, 16, 9, 13, 16, 1, 2), (1, 4, 1, 1, 8, 3, 1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%dC%dH%dW%dO%dk%ds%d" % c)
def test_conv64_vs_conv2d(case):
    B, C, H, W, O, k, st = case
    g = torch.Generator().manual_seed(sum(case))
    x, w, b = rnd(g, B, C, H, W), rnd(g, O, C, k, k, scale=0.2), rnd(g, O)
    x = x.contiguous(memory_format=torch.channels_last)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=st, padding=(k - 1) // 2)
    r = rnd(g, *ref.shape)
    for relu in (False, True):
        for res in (None, r):
            y, S = conv64(x, w, b, st, k, residual=res, relu=relu)
            want = ref + (0 if res is None else res.double())
            want = want.clamp_min(0) if relu else want
            assert y.shape == want.shape and S.shape == want.shape
            assert torch.allclose(y, want, rtol=1e-12, atol=1e-12), (case, relu, res is None)
    y, S = conv64(x, w, None, st, k)                     # no bias
    assert torch.allclose(y, F.conv2d(x.double(), w.double(), None, stride=st, padding=(k - 1) // 2), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", [(2, 16, 8, 12, 32), (1, 8, 6, 10, 16)])
def test_conv64_residual_up2(shape):
    """the FPN top-down step: 1x1 + bias + nearest-2x up-sampled coarse map"""
    B, C, H, W, O = shape
    g = torch.Generator().manual_seed(3)
    x, w, b = rnd(g, B, C, H, W), rnd(g, O, C, 1, 1, scale=0.3), rnd(g, O)
    coarse = rnd(g, B, O, H // 2, W // 2)
    y, S = conv64(x, w, b, 1, 1, residual=coarse, residual_up2=True)
    up = F.interpolate(coarse.double(), scale_factor=2, mode="nearest")
    assert torch.allclose(y, F.conv2d(x.double(), w.double(), b.double()) + up, rtol=1e-12, atol=1e-12)
    assert torch.allclose(S, F.conv2d(x.double().abs(), w.double().abs(), b.double().abs()) + up.abs(), rtol=1e-12)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5]], ids=("3x3s1", "3x3s2", "1x1s2"))
def test_conv64_scale_brute_force(case):
    """S at sampled entries (corners, edges and the interior) = the sum of |products| + |bias| + |residual|, term by
    term"""
    B, C, H, W, O, k, st = case
    g = torch.Generator().manual_seed(7)
    x, w, b = rnd(g, B, C, H, W), rnd(g, O, C, k, k, scale=0.2), rnd(g, O)
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    r = rnd(g, B, O, Ho, Wo)
    y, S = conv64(x, w, b, st, k, residual=r, relu=True)
    xd, wd = x.double(), w.double()
    rng = np.random.default_rng(1)
    picks = [(0, 0, 0, 0), (B - 1, O - 1, Ho - 1, Wo - 1), (0, 1, Ho - 1, 0), (B - 1, 2, 0, Wo - 1)]
    picks += [tuple(int(rng.integers(0, n)) for n in (B, O, Ho, Wo)) for _ in range(24)]
    for bi, o, i, j in picks:
        s = abs(b[o].item()) + abs(r[bi, o, i, j].item())
        v = b[o].item() + r[bi, o, i, j].item()
        for c in range(C):
            for di in range(k):
                for dj in range(k):
                    yy, xx = i * st - pad + di, j * st - pad + dj
                    if 0 <= yy < H and 0 <= xx < W:
                        p = xd[bi, c, yy, xx].item() * wd[o, c, di, dj].item()
                        v += p
                        s += abs(p)
        assert S[bi, o, i, j].item() == pytest.approx(s, rel=1e-12, abs=1e-15)
        assert y[bi, o, i, j].item() == pytest.approx(max(v, 0.0), rel=1e-9, abs=1e-12)


def test_u8_table_is_torch_half_division():
    u = torch.arange(256, dtype=torch.uint8)
    t = u8_to_f16(u)
    assert torch.equal(t, u.half() / 255)                              # torch's half division
    assert torch.equal(t, (u.double() / 255).half())                   # and the correctly rounded quotient


@pytest.mark.parametrize("hw", [(32, 48), (30, 36), (17, 20)])
def test_stem64_vs_conv2d_relu_maxpool(hw):
    H, W = hw
    g = torch.Generator().manual_seed(H * W)
    img = torch.randint(0, 256, (2, 3, H, W), generator=g, dtype=torch.uint8).contiguous(memory_format=torch.channels_last)
    w, b = rnd(g, 64, 3, 7, 7, scale=0.1), rnd(g, 64, scale=0.3)
    y, S = stem64(img, w, b)
    xf = (img.half() / 255).double()
    conv = F.conv2d(xf, w.double(), b.double(), stride=2, padding=3)
    want = F.max_pool2d(F.relu(conv), 3, 2, 1)
    assert y.shape == want.shape and torch.allclose(y, want, rtol=1e-12, atol=1e-12)
    sconv = F.conv2d(xf.abs(), w.double().abs(), b.double().abs(), stride=2, padding=3)
    assert torch.allclose(S, F.max_pool2d(sconv, 3, 2, 1), rtol=1e-12, atol=1e-15)
    assert (y > 0).double().mean() > 0.2


def test_rot_pool64():
    g = torch.Generator().manual_seed(2)
    y = torch.randn((2, 64, 5, 6), generator=g, dtype=F64)
    S = y.abs() + 1
    py, pS = rot_pool64(y, S)
    assert torch.equal(py, y.view(2, 8, 8, 5, 6).amax(2)) and torch.equal(pS, S.view(2, 8, 8, 5, 6).amax(2))
    assert torch.equal(py[:, 3], y[:, 24:32].amax(1))


def edge_offsets(g, B, H, W):
    """samples on exact integers (-1 and H included), in the bands (-1, 0) and (H-1, H), far outside, and ordinary
    fractional points"""
    kind = torch.randint(0, 6, (B, 9, H, W), generator=g)
    t = torch.arange(9)
    ys = (torch.arange(H).view(1, 1, H, 1) - 1 + (t // 3).view(1, 9, 1, 1)).double()
    xs = (torch.arange(W).view(1, 1, 1, W) - 1 + (t % 3).view(1, 9, 1, 1)).double()

    def pick(n, base):
        r = torch.rand(kind.shape, generator=g, dtype=F64)
        return torch.where(kind == 0, torch.randint(-1, n + 1, kind.shape, generator=g).double(),
               torch.where(kind == 1, -0.05 - 0.9 * r,
               torch.where(kind == 2, n - 0.95 + 0.9 * r,
               torch.where(kind == 3, torch.where(r < 0.5, -30.0, n + 30.0),
               torch.where(kind == 4, torch.randint(0, n, kind.shape, generator=g).double() + 0.25,
                           base + 4 * (r - 0.5))))))
    off = torch.empty((B, 18, H, W), dtype=F64)
    off[:, 0::2] = pick(H, ys) - ys
    off[:, 1::2] = pick(W, xs) - xs
    return off.float()


@pytest.mark.parametrize("d", (0.0, 2.0 ** -6, 0.3))
def test_align64_against_deform_conv64_and_brute_force(d):
    B, C, O, H, W = 2, 12, 8, 7, 9
    g = torch.Generator().manual_seed(5)
    x, w = rnd(g, B, C, H, W), rnd(g, O, C, 3, 3, scale=0.2)
    off = edge_offsets(g, B, H, W)
    y, S, Sc = align64(x, off, w, relu=True, d=d, chunk_elems=9 * H * W * 5)       # channel chunks of 5
    assert torch.allclose(y, deform_conv64(x, off, w, pos_dtype=torch.float32).clamp_min(0), rtol=1e-12, atol=1e-14)
    assert (Sc >= S).all() and (S >= y.abs() - 1e-12).all()
    h, ww = sample_points(off, torch.float32)
    xd, wd = x.double(), w.double()
    rng = np.random.default_rng(3)
    picks = [tuple(int(rng.integers(0, n)) for n in (B, O, H, W)) for _ in range(40)]
    picks += [(0, 0, 0, 0), (B - 1, O - 1, H - 1, W - 1)]
    kinds = set()
    for bi, o, i, j in picks:
        s = sc = 0.0
        for t in range(9):
            hp, wp = h[bi, t, i, j].item(), ww[bi, t, i, j].item()

            def a(yy, xx):
                return sum(abs(xd[bi, c, yy, xx].item() * wd[o, c, t // 3, t % 3].item()) for c in range(C))
            # S_corner: every in-image corner of the cells a point within d of (hp, wp) lies in (band or not)
            for yy in range(int(np.floor(hp - d)), int(np.floor(hp + d)) + 2):
                for xx in range(int(np.floor(wp - d)), int(np.floor(wp + d)) + 2):
                    if 0 <= yy < H and 0 <= xx < W:
                        sc += a(yy, xx)
            if not (-1 < hp < H and -1 < wp < W):
                kinds.add("outside")
                continue
            edge = hp < 0 or wp < 0 or hp > H - 1 or wp > W - 1
            kinds.add("integer" if hp == int(hp) or wp == int(wp) else ("band" if edge else "inner"))
            hl, wl = int(np.floor(hp)), int(np.floor(wp))
            lh, lw = hp - hl, wp - wl
            for dy, dx, cw in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
                yy, xx = hl + dy, wl + dx
                if 0 <= yy < H and 0 <= xx < W:
                    s += cw * a(yy, xx)
        assert S[bi, o, i, j].item() == pytest.approx(s, rel=1e-12, abs=1e-15)
        assert Sc[bi, o, i, j].item() == pytest.approx(sc, rel=1e-12, abs=1e-15)
    assert {"outside", "integer", "band", "inner"} <= kinds, kinds


@pytest.mark.parametrize("d", (2.0 ** -6, 0.3))
def test_align64_coordinate_bound(d):
    """moving every sample point by at most d in h and in w moves the result by at most 2 d S_corner(d), also where a
    point crosses an integer row or column (the edge offsets put many samples exactly on integers and on the band's
    edges)"""
    B, C, O, H, W = 1, 8, 4, 6, 7
    g = torch.Generator().manual_seed(9)
    x, w = rnd(g, B, C, H, W), rnd(g, O, C, 3, 3, scale=0.3)
    off = edge_offsets(g, B, H, W).double()
    y0, _, Sc = align64(x, off, w, pos_dtype=None, d=d)
    for k in range(8):
        moved = off + d * (2 * torch.rand(off.shape, generator=g, dtype=F64) - 1)
        if k < 2:                                    # every coordinate moved by exactly -d / +d
            moved = off + (d if k else -d)
        y1, _, _ = align64(x, moved, w, pos_dtype=None)
        diff = (y1 - y0).abs()
        assert (diff <= 2 * d * Sc + 1e-12).all(), k
