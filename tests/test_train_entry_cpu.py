"""The entry of the training step on the own kernels (train_kernels(..., entry=True): StemU8Function, FusedConvUp2Function)
without a GPU:

  * the float64 identities the kernels are built on, against autograd: the stem's filter and bias gradient written with the
    pooled tap `sel` and the ReLU mask `m` (include/s2anet_hip.h, s2a_stem_backward_f16) equals the gradient of
    max_pool2d(relu(conv2d(img / 255, w, b, 2, 3)), 3, 2, 1); the 2 x 2 sum-pool equals the gradient of the nearest
    up-sampling;
  * the switch (own_grad_entry) and the CPU fall-through of DetectorBackbone.forward and FPN.forward;
  * every argument check of the new C entry points: S2A_EINVAL with its message, made before any HIP call (this file runs
    where there is no device), and the slices query;
  * the exported *_workspace_bytes symbols are still the 20 of tests/test_workspace_queries_cpu.py.

stem_reference() and sum_pool_reference() are the float64 side of tests/test_gpu_train_entry.py as well."""
import ctypes
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64
STEM_COLS = 64 * 147 + 64


def stem_out_hw(H, W):
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (Hc, Wc), ((Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1)


def sel_from_indices(idx, Wc):
    """max_pool2d's flat indices into the conv map [B,O,Hp,Wp] -> the tap 3 dy + dx of the 3x3 / s2 / p1 window"""
    Hp, Wp = idx.shape[2:]
    py = torch.arange(Hp, device=idx.device).view(1, 1, Hp, 1)
    px = torch.arange(Wp, device=idx.device).view(1, 1, 1, Wp)
    dy, dx = idx // Wc - (2 * py - 1), idx % Wc - (2 * px - 1)
    assert int(dy.min()) >= 0 and int(dy.max()) <= 2 and int(dx.min()) >= 0 and int(dx.max()) <= 2
    return (3 * dy + dx).to(torch.uint8)


def stem_reference(x64, sel, m, cot):
    """the two formulas of s2a_stem_backward_f16 over float64: x64 [B,3,H,W] the values the forward multiplied, sel
    [B,O,Hp,Wp] the pooled taps, m [B,O,Hp,Wp] bool the ReLU mask, cot [B,O,Hp,Wp] -> (gW [O,3,7,7], gB [O]).
    A masked term is selected away (torch.where), a pixel outside the image enters as zero."""
    B, _, H, W = x64.shape
    O, Hp, Wp = sel.shape[1:]
    dev = x64.device
    g = torch.where(m, cot.to(F64), torch.zeros((), dtype=F64, device=dev))
    s = sel.long()
    y = 2 * torch.arange(Hp, device=dev).view(1, 1, Hp, 1) - 1 + s // 3             # the conv pixel sel names
    x = 2 * torch.arange(Wp, device=dev).view(1, 1, 1, Wp) - 1 + s % 3
    xp = F.pad(x64, (3, 3, 3, 3))
    bi = torch.arange(B, device=dev).view(B, 1, 1, 1).expand(B, O, Hp, Wp)
    gw = torch.zeros((O, 3, 7, 7), dtype=F64, device=dev)
    for ky in range(7):
        for kx in range(7):
            v = xp[bi, :, 2 * y + ky, 2 * x + kx]                                    # [B,O,Hp,Wp,3]
            gw[:, :, ky, kx] = torch.einsum("bopq,bopqc->oc", g, v)
    return gw, g.sum((0, 2, 3))


def sum_pool_reference(g, dtype=None):
    """s2a_sum_pool2x2_f16's formula on [B,O,H,W]: ((g[2i,2j] + g[2i,2j+1]) + g[2i+1,2j]) + g[2i+1,2j+1]"""
    g = g if dtype is None else g.to(dtype)
    return ((g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2]) + g[:, :, 1::2, 0::2]) + g[:, :, 1::2, 1::2]


# ----------------------------------------------------------------------------- float64 identities
@pytest.mark.parametrize("H,W", [(8, 8), (72, 100), (9, 12)])
def test_stem_formulas_are_autograds(H, W):
    B, O = 2, 5
    gen = torch.Generator().manual_seed(100 * H + W)
    img = torch.randint(0, 256, (B, 3, H, W), generator=gen, dtype=torch.uint8)
    w = (torch.randn((O, 3, 7, 7), generator=gen, dtype=F64) * 0.2).requires_grad_(True)
    b = torch.randn((O,), generator=gen, dtype=F64) * 0.3 - 2.0
    b[0] = -100.0                                                   # one map the ReLU masks everywhere
    b.requires_grad_(True)
    x64 = img.to(F64) / 255
    conv = F.conv2d(x64, w, b, 2, 3)
    out, idx = F.max_pool2d(F.relu(conv), 3, 2, 1, return_indices=True)
    (Hc, Wc), (Hp, Wp) = stem_out_hw(H, W)
    assert tuple(conv.shape[2:]) == (Hc, Wc) and tuple(out.shape[2:]) == (Hp, Wp)
    cot = torch.randn(out.shape, generator=gen, dtype=F64)
    out.backward(cot)
    gw, gb = stem_reference(x64, sel_from_indices(idx, Wc), out.detach() > 0, cot)
    assert int((out.detach() > 0).sum()) > 0 and int((out.detach() <= 0).sum()) > 0      # both branches of the mask
    assert torch.allclose(gw, w.grad, rtol=1e-12, atol=1e-12), float((gw - w.grad).abs().max())
    assert torch.allclose(gb, b.grad, rtol=1e-12, atol=1e-12), float((gb - b.grad).abs().max())


@pytest.mark.parametrize("H,W", [(6, 10), (2, 2), (14, 18)])
def test_sum_pool_is_the_gradient_of_the_nearest_upsampling(H, W):
    gen = torch.Generator().manual_seed(H * 50 + W)
    coarse = torch.randn((2, 3, H // 2, W // 2), generator=gen, dtype=F64, requires_grad=True)
    g = torch.randn((2, 3, H, W), generator=gen, dtype=F64)
    F.interpolate(coarse, scale_factor=2, mode="nearest").backward(g)
    got = sum_pool_reference(g)
    assert torch.allclose(got, coarse.grad, rtol=1e-13, atol=1e-13), float((got - coarse.grad).abs().max())


# ----------------------------------------------------------------------------- the switch
def test_train_kernels_sets_and_clears_the_entry_flag():
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d
    assert FusedConv2d.own_grad_entry is False
    net = torch.nn.ModuleList([FusedConv2d(3, 64, 7, 2, 3, relu=True), FusedConv2d(64, 64, 1), torch.nn.Conv2d(4, 4, 1)])
    assert S.train_kernels(net) == 2
    assert all(m.own_grad and m.own_grad_entry is False and m.own_grad_strided is False for m in net[:2])
    assert S.train_kernels(net, True, entry=True) == 2
    assert all(m.own_grad_entry is True and m.own_grad_strided is False for m in net[:2])
    assert S.train_kernels(net, True, strided=True) == 2                                 # not mentioned: not touched
    assert all(m.own_grad_entry is True and m.own_grad_strided is True for m in net[:2])
    assert S.train_kernels(net, False, entry=True) == 2
    assert all(m.own_grad is False and m.own_grad_entry is False and m.own_grad_strided is True for m in net[:2])
    assert not hasattr(net[2], "own_grad_entry")


def test_cpu_forwards_fall_through():
    """on the CPU no limit of the own routes holds: a uint8 batch is divided by 255 and takes the stock stem, the top-down
    steps run the stock line -- the same bits as with the switch off"""
    import s2anet_amd as S
    from s2anet_amd.detector import FPN, DetectorBackbone, fold_batchnorm, fuse_epilogues

    class Carrier(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = DetectorBackbone(layers=(1, 1, 1, 1))
    torch.manual_seed(3)
    trunk = fold_batchnorm(Carrier().eval()).backbone
    gen = torch.Generator().manual_seed(4)
    img = torch.randint(0, 256, (1, 3, 32, 36), generator=gen, dtype=torch.uint8)
    off = trunk(img.float() / 255)
    assert S.train_kernels(trunk, True, entry=True) > 0 and trunk.backbone[0][0].own_grad_entry
    assert not trunk.stem_limits(img)
    on = trunk(img)
    assert all(torch.equal(a, b) for a, b in zip(on, off)) and on[0].requires_grad
    sum(t.sum() for t in on).backward()
    assert trunk.backbone[0][0].weight.grad is not None
    with torch.no_grad(), pytest.raises(RuntimeError):                                   # without grad: today's behaviour (no uint8 conv)
        trunk(img)

    neck = fuse_epilogues(FPN(in_channels=(64, 128, 256), out_channels=64))
    xs = [torch.randn((1, c, h, w), generator=gen) for c, h, w in ((64, 8, 12), (128, 4, 6), (256, 2, 3))]
    off = neck(xs)
    assert S.train_kernels(neck, True, entry=True) == 8
    assert not S.train_up2_ok(xs[0], neck.lateral_convs[0], off[1])
    on = neck(xs)
    assert len(on) == 5 and all(torch.equal(a, b) for a, b in zip(on, off))


# ----------------------------------------------------------------------------- the C ABI
def _err():
    from s2anet_amd import _lib
    return _lib.lib().s2a_last_error().decode()


P, ODD = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)         # never dereferenced: every call below is refused first
NULL = ctypes.c_void_p(0)
OK_IMG = (2, 72, 100)

BAD_IMAGES = [((2, 6, 100), "bad shape"), ((2, 72, 4), "bad shape"), ((-1, 72, 100), "bad shape"),
              ((2, 72, 102), "multiple of 4"), ((1 << 20, 1024, 1024), "too large")]


def _fwd(L, img_shape, divisor=255.0, img=P, w=P, b=P, out=P, sel=P):
    return L.s2a_stem_u8_f16_train(img, w, b, out, sel, *img_shape, divisor, NULL)


def _bwd(L, img_shape, slices, divisor=255.0, img=P, out=P, sel=P, go=P, partial=P):
    return L.s2a_stem_backward_f16(img, out, sel, go, partial, slices, *img_shape, divisor, NULL)


@pytest.mark.parametrize("shape,words", BAD_IMAGES, ids=["-".join(map(str, a)) for a, _ in BAD_IMAGES])
def test_bad_images_are_refused_by_forward_backward_and_query(shape, words):
    from s2anet_amd import _lib
    L = _lib.lib()
    assert L.s2a_stem_backward_slices(*shape) == 0
    assert _fwd(L, shape) == _lib.EINVAL and "stem_train" in _err() and words in _err(), _err()
    assert _bwd(L, shape, 1) == _lib.EINVAL and "stem_backward" in _err() and words in _err(), _err()


def test_stem_divisor_null_and_misaligned_pointers_are_refused():
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_stem_backward_slices(*OK_IMG)
    assert n > 0
    for d in (0.0, -1.0):
        assert _fwd(L, OK_IMG, d) == _lib.EINVAL and "divisor" in _err()
        assert _bwd(L, OK_IMG, n, d) == _lib.EINVAL and "divisor" in _err()
    for name in ("img", "w", "out", "sel"):                             # (the bias may be NULL: no bias)
        assert _fwd(L, OK_IMG, **{name: NULL}) == _lib.EINVAL and "NULL tensor" in _err(), name
    for name, bad in (("img", ctypes.c_void_p(0x10002)), ("w", ODD), ("out", ODD), ("sel", ODD), ("b", ctypes.c_void_p(0x10001))):
        assert _fwd(L, OK_IMG, **{name: bad}) == _lib.EINVAL and "misaligned" in _err(), name
    for name in ("img", "out", "sel", "go", "partial"):
        assert _bwd(L, OK_IMG, n, **{name: NULL}) == _lib.EINVAL and "NULL tensor" in _err(), name
    for name, bad in (("img", ctypes.c_void_p(0x10002)), ("out", ODD), ("sel", ODD), ("go", ODD), ("partial", ODD)):
        assert _bwd(L, OK_IMG, n, **{name: bad}) == _lib.EINVAL and "misaligned" in _err(), name
    assert _fwd(L, (0,) + OK_IMG[1:], img=NULL, w=NULL, out=NULL, sel=NULL) == _lib.OK     # nothing to write


def test_a_slice_count_other_than_the_querys_is_refused():
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_stem_backward_slices(*OK_IMG)
    for s in (0, -1, n - 1, n + 1, 2 * n):
        assert _bwd(L, OK_IMG, s) == _lib.EINVAL and "slices is %d" % s in _err() and "answers %d" % n in _err(), _err()
    assert _bwd(L, (0,) + OK_IMG[1:], 0) == _lib.EINVAL and "empty batch" in _err()


def _tiles(B, H, W):
    _, (Hp, Wp) = stem_out_hw(H, W)
    return B * ((Hp + 7) // 8) * ((Wp + 7) // 8)


@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 72, 100), (1, 516, 516), (8, 1024, 1024), (2, 384, 384), (1, 9, 12)])
def test_slices_query_is_positive_and_repeats(shape):
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_stem_backward_slices(*shape)
    assert 0 < n <= 256 and n == min(_tiles(*shape), 256) and L.s2a_stem_backward_slices(*shape) == n
    assert n * STEM_COLS * 4 < (1 << 31)
    assert L.s2a_stem_backward_slices(0, *shape[1:]) == 0


def test_516_is_the_smallest_square_with_more_tiles_than_slices_and_no_even_split():
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_stem_backward_slices(1, 516, 516)
    assert _tiles(1, 516, 516) == 289 > n == 256 and 289 % n != 0
    for side in range(8, 516, 4):                                    # (the width must be a multiple of 4)
        assert _tiles(1, side, side) <= L.s2a_stem_backward_slices(1, side, side), side


def test_sum_pool_argument_checks():
    from s2anet_amd import _lib
    L = _lib.lib()
    sp = L.s2a_sum_pool2x2_f16
    for args, words in (((P, P, 1, 0, 8, 64), "bad shape"), ((P, P, -1, 8, 8, 64), "bad shape"), ((P, P, 1, 8, 8, 0), "bad shape"),
                        ((P, P, 1, 7, 8, 64), "exactly twice"), ((P, P, 1, 8, 9, 64), "exactly twice"),
                        ((P, P, 1, 8, 8, 60), "multiple of 8"), ((P, P, 8, 2048, 2048, 64), "too large"),
                        ((NULL, P, 1, 8, 8, 64), "NULL tensor"), ((P, NULL, 1, 8, 8, 64), "NULL tensor"),
                        ((ODD, P, 1, 8, 8, 64), "16-byte aligned"), ((P, ODD, 1, 8, 8, 64), "16-byte aligned")):
        assert sp(*args, NULL) == _lib.EINVAL and "sum_pool2x2" in _err() and words in _err(), (args, _err())
    assert sp(NULL, NULL, 0, 8, 8, 64, NULL) == _lib.OK                                  # nothing to write


def test_no_new_workspace_query_and_no_opaque_workspace():
    from s2anet_amd import _lib
    _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len(set(re.findall(r"\b(s2a_\w+_workspace_bytes)\b", out))) == 20
    for n in ("s2a_stem_u8_f16_train", "s2a_stem_backward_slices", "s2a_stem_backward_f16", "s2a_sum_pool2x2_f16"):
        assert re.search(r"\b%s\b" % n, out), n
        assert n in _lib.SYMBOLS and ctypes.c_size_t not in _lib.SYMBOLS[n][1]
