"""The stride-2 training route (train_kernels(..., strided=True), FusedConvS2Function) without a GPU:

  * the float64 identities the kernels are built on, against autograd of F.conv2d(x, w, None, 2, k // 2): the four
    parity classes of the 3x3 / s2 / p1 input gradient, the 1x1 / s2 spread with exact zeros, both weight gradients;
  * the switch (own_grad_strided) and the CPU fall-through;
  * every argument check of the new C entry points: S2A_EINVAL with its message, made before any HIP call (this file runs
    where there is no device), and the slices query;
  * the exported *_workspace_bytes symbols are still the 20 of tests/test_workspace_queries_cpu.py: the new entry points
    take no opaque workspace."""
import ctypes
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64
SIZES = [(9, 21), (10, 22), (9, 22), (10, 21), (1, 1), (2, 2), (3, 2), (1, 4)]
B, C, O = 2, 3, 5


def _case(k, H, W, seed=0):
    g = torch.Generator().manual_seed(100 * H + W + seed)
    x = torch.randn((B, C, H, W), generator=g, dtype=F64, requires_grad=True)
    w = torch.randn((O, C, k, k), generator=g, dtype=F64, requires_grad=True)
    y = F.conv2d(x, w, None, 2, k // 2)
    cot = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(cot)
    return x.detach(), w.detach(), cot, x.grad, w.grad


def _g_at(g, di, dj, n_i, n_j):
    """g[b, :, i + di, j + dj] for i < n_i, j < n_j, with g outside its map taking no part (zeros stand for 'left out')"""
    Ho, Wo = g.shape[2:]
    out = g.new_zeros((g.shape[0], g.shape[1], n_i, n_j))
    hi, wj = min(n_i, Ho - di), min(n_j, Wo - dj)
    if hi > 0 and wj > 0:
        out[:, :, :hi, :wj] = g[:, :, di:di + hi, dj:dj + wj]
    return out


def input_grad_3x3_s2(g, w, H, W):
    """the four parity classes of include/s2anet_hip.h (s2a_conv_backward_input_s2_f16), tap sums in the kernel's order"""
    gx = g.new_zeros((g.shape[0], w.shape[1], H, W))
    classes = {(0, 0): [(1, 1, 0, 0)],
               (0, 1): [(1, 0, 0, 1), (1, 2, 0, 0)],
               (1, 0): [(0, 1, 1, 0), (2, 1, 0, 0)],
               (1, 1): [(0, 0, 1, 1), (0, 2, 1, 0), (2, 0, 0, 1), (2, 2, 0, 0)]}
    for (py, px), taps in classes.items():
        n_i, n_j = len(range(py, H, 2)), len(range(px, W, 2))
        if n_i == 0 or n_j == 0:
            continue
        acc = g.new_zeros((g.shape[0], w.shape[1], n_i, n_j))
        for ky, kx, di, dj in taps:
            acc = acc + torch.einsum("oc,boij->bcij", w[:, :, ky, kx], _g_at(g, di, dj, n_i, n_j))
        gx[:, :, py::2, px::2] = acc
    return gx


def weight_grad_s2(x, g, k):
    """gw[o,c,ky,kx] = sum g[b,oy,ox,o] x[b, 2 oy + ky - pad, 2 ox + kx - pad, c], zero padding"""
    pad = k // 2
    Ho, Wo = g.shape[2:]
    xp = F.pad(x, (pad, pad, pad, pad))
    gw = x.new_zeros((g.shape[1], x.shape[1], k, k))
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, :, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2]
            gw[:, :, ky, kx] = torch.einsum("boij,bcij->oc", g, xs)
    return gw


@pytest.mark.parametrize("H,W", SIZES)
def test_four_class_input_gradient_is_autograds(H, W):
    x, w, cot, gx, _ = _case(3, H, W)
    assert tuple(cot.shape[2:]) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    got = input_grad_3x3_s2(cot, w, H, W)
    assert torch.allclose(got, gx, rtol=1e-12, atol=1e-12), float((got - gx).abs().max())


@pytest.mark.parametrize("H,W", SIZES)
def test_1x1_spread_is_autograds_with_exact_zeros_elsewhere(H, W):
    x, w, cot, gx, _ = _case(1, H, W)
    even = torch.einsum("oc,boij->bcij", w[:, :, 0, 0], cot)
    assert torch.allclose(gx[:, :, 0::2, 0::2], even, rtol=1e-12, atol=1e-12)
    rest = gx.clone()
    rest[:, :, 0::2, 0::2] = 0
    assert int((rest != 0).sum()) == 0 and not bool(torch.signbit(rest).any())          # exact +0 at every other pixel


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("H,W", SIZES)
def test_strided_weight_gradient_is_autograds(k, H, W):
    x, w, cot, _, gw = _case(k, H, W)
    got = weight_grad_s2(x, cot, k)
    assert torch.allclose(got, gw, rtol=1e-12, atol=1e-12), float((got - gw).abs().max())


# ----------------------------------------------------------------------------- the switch
def _net():
    from s2anet_amd.fused import FusedConv2d
    return torch.nn.ModuleList([FusedConv2d(64, 128, 3, 2, 1, relu=True), FusedConv2d(64, 128, 1, 2, 0), FusedConv2d(64, 64, 3, 1, 1)])


def test_train_kernels_sets_and_clears_the_strided_flag():
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d
    assert FusedConv2d.own_grad_strided is False
    net = _net()
    assert S.train_kernels(net) == 3
    assert all(m.own_grad and m.own_grad_strided is False for m in net)                  # the default leaves it off
    assert S.train_kernels(net, True, strided=True) == 3
    assert all(m.own_grad and m.own_grad_strided is True for m in net)
    assert S.train_kernels(net, True) == 3                                               # not mentioned: not touched
    assert all(m.own_grad_strided is True for m in net)
    assert S.train_kernels(net, False, strided=True) == 3
    assert all(m.own_grad is False and m.own_grad_strided is False for m in net)


def test_cpu_forward_falls_through():
    import s2anet_amd as S
    net = _net()
    S.train_kernels(net, True, strided=True)
    x = torch.randn((1, 64, 6, 8), requires_grad=True)
    for m in net[:2]:
        assert not S.train_conv_strided_ok(x, m)
        y = m(x)
        want = F.conv2d(x, m.weight, m.bias, 2, m.padding)
        assert torch.equal(y, F.relu(want) if m.fuse_relu else want)
        y.sum().backward()
        assert x.grad is not None and m.weight.grad is not None


# ----------------------------------------------------------------------------- the C ABI
def _err():
    from s2anet_amd import _lib
    return _lib.lib().s2a_last_error().decode()


P, ODD = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10008)         # never dereferenced: every call below is refused first
NULL = ctypes.c_void_p(0)
OK_SHAPE = (2, 64, 9, 21, 128)

# (B, C, H, W, O, ksize) -> the message's key words
BAD_SHAPES = [
    ((2, 64, 9, 21, 128, 2), "kernel size must be 1 or 3"),
    ((2, 64, 9, 21, 128, 5), "kernel size must be 1 or 3"),
    ((2, 64, 0, 21, 128, 3), "bad shape"),
    ((2, 64, 9, -1, 128, 3), "bad shape"),
    ((-1, 64, 9, 21, 128, 3), "bad shape"),
    ((2, 0, 9, 21, 128, 3), "bad shape"),
    ((2, 96, 9, 21, 128, 3), "multiples of 64"),
    ((2, 64, 9, 21, 96, 1), "multiples of 64"),
    ((2, 64, 9, 21, 192, 3), "out_channels % 128"),
    ((2, 64, 9, 21, 64, 3), "out_channels % 128"),
    ((8, 64, 2048, 2048, 128, 3), "too large"),                      # x: 2^32 bytes
    ((1, 64, 64, 64, 1 << 20, 1), "too large"),                      # g: 2^31 bytes
    ((1, 8192, 2, 2, 8192, 3), "too large"),                         # the filter in f32: 2.4e9 bytes
]


def _input(L, shape, k, g=P, w=P, gx=P):
    return L.s2a_conv_backward_input_s2_f16(g, w, gx, *shape, k, NULL)


def _weight(L, shape, k, slices, x=P, g=P, partial=P):
    return L.s2a_conv_backward_weight_s2_f16(x, g, partial, slices, *shape, k, NULL)


@pytest.mark.parametrize("args,words", BAD_SHAPES, ids=["-".join(map(str, a)) for a, _ in BAD_SHAPES])
def test_bad_shapes_are_refused_by_all_three(args, words):
    from s2anet_amd import _lib
    L = _lib.lib()
    shape, k = args[:5], args[5]
    assert L.s2a_conv_backward_weight_s2_slices(*shape, k) == 0
    assert _input(L, shape, k) == _lib.EINVAL and "conv_backward_input_s2" in _err() and words in _err(), _err()
    assert _weight(L, shape, k, 1) == _lib.EINVAL and "conv_backward_weight_s2" in _err() and words in _err(), _err()


@pytest.mark.parametrize("k", [3, 1])
def test_null_and_misaligned_pointers_are_refused(k):
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_conv_backward_weight_s2_slices(*OK_SHAPE, k)
    for i in range(3):
        for bad, words in ((NULL, "NULL tensor"), (ODD, "16-byte aligned")):
            ptrs = [P, P, P]
            ptrs[i] = bad
            assert _input(L, OK_SHAPE, k, *ptrs) == _lib.EINVAL and words in _err(), (i, _err())
            assert _weight(L, OK_SHAPE, k, n, *ptrs) == _lib.EINVAL and words in _err(), (i, _err())


@pytest.mark.parametrize("k", [3, 1])
def test_a_slice_count_other_than_the_querys_is_refused(k):
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_conv_backward_weight_s2_slices(*OK_SHAPE, k)
    for s in (0, -1, n - 1, n + 1, 2 * n):
        assert _weight(L, OK_SHAPE, k, s) == _lib.EINVAL and "slices is %d" % s in _err() and "answers %d" % n in _err(), _err()
    assert _weight(L, (0,) + OK_SHAPE[1:], k, 0) == _lib.EINVAL and "empty batch" in _err()
    assert _input(L, (0,) + OK_SHAPE[1:], k, NULL, NULL, NULL) == _lib.OK              # nothing to write


def test_reduce_argument_checks():
    from s2anet_amd import _lib
    L = _lib.lib()
    red = L.s2a_conv_backward_weight_s2_reduce
    for args, words in (((P, 0, 64, P, _lib.DTYPE_F32), "bad shape"), ((P, 4, -1, P, _lib.DTYPE_F32), "bad shape"),
                        ((P, 4, 1 << 29, P, _lib.DTYPE_F32), "too large"), ((P, 4, 64, P, _lib.DTYPE_F64), "dtype must be f32 or f16"),
                        ((NULL, 4, 64, P, _lib.DTYPE_F32), "NULL tensor"), ((P, 4, 64, NULL, _lib.DTYPE_F16), "NULL tensor"),
                        ((ODD, 4, 64, P, _lib.DTYPE_F32), "16-byte aligned"), ((P, 4, 64, ODD, _lib.DTYPE_F16), "16-byte aligned")):
        assert red(*args, NULL) == _lib.EINVAL and "conv_backward_weight_s2_reduce" in _err() and words in _err(), (args, _err())
    assert red(NULL, 4, 0, NULL, _lib.DTYPE_F32, NULL) == _lib.OK                        # nothing to write


# the trunk's and the neck's stride-2 layers at the benchmark's shapes, and the cases of tests/test_gpu_train_conv_s2.py
VALID = [(8, 128, 256, 256, 128, 3), (8, 256, 128, 128, 256, 3), (8, 512, 64, 64, 512, 3), (8, 256, 256, 256, 512, 1),
         (8, 512, 128, 128, 1024, 1), (8, 1024, 64, 64, 2048, 1), (8, 2048, 32, 32, 256, 3), (8, 256, 16, 16, 256, 3),
         (2, 64, 9, 21, 128, 3), (1, 128, 7, 9, 384, 3), (4, 64, 40, 72, 128, 3), (1, 64, 1, 1, 128, 3), (2, 64, 6, 8, 320, 1)]


@pytest.mark.parametrize("args", VALID, ids=["-".join(map(str, a)) for a in VALID])
def test_slices_query_is_positive_and_repeats(args):
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_conv_backward_weight_s2_slices(*args)
    assert 0 < n <= 32 and L.s2a_conv_backward_weight_s2_slices(*args) == n
    Bn, Cn, H, W, On, k = args
    assert n * On * Cn * k * k * 4 < (1 << 31)                                          # a partial a caller can allocate
    assert L.s2a_conv_backward_weight_s2_slices(2 * Bn, Cn, H + 1, W + 3, On, k) == n   # shapes of the FILTER only move it
    assert L.s2a_conv_backward_weight_s2_slices(0, Cn, H, W, On, k) == 0


def test_the_40x72_case_has_more_tiles_than_slices_and_no_even_split():
    from s2anet_amd import _lib
    n = _lib.lib().s2a_conv_backward_weight_s2_slices(4, 64, 40, 72, 128, 3)
    tiles = 4 * ((20 + 3) // 4) * ((36 + 15) // 16)                                     # 4 x 16 tiles of the 20 x 36 output map
    assert tiles > n and tiles % n != 0, (tiles, n)


def test_no_new_workspace_query_and_no_opaque_workspace():
    from s2anet_amd import _lib
    _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len(set(re.findall(r"\b(s2a_\w+_workspace_bytes)\b", out))) == 20
    new = [n for n in _lib.SYMBOLS if "_s2_" in n]
    assert sorted(new) == ["s2a_conv_backward_input_s2_f16", "s2a_conv_backward_weight_s2_f16",
                           "s2a_conv_backward_weight_s2_reduce", "s2a_conv_backward_weight_s2_slices"]
    for n in new:
        assert re.search(r"\b%s\b" % n, out), n
        assert ctypes.c_size_t not in _lib.SYMBOLS[n][1]
