"""CPU: the two identities the training kernels of FusedConv2d implement, the train_kernels switch, and the argument
checks of the three C entries (s2a_conv_pack_weight_train, s2a_conv_backward_prep_f16, s2a_conv_backward_weight_f16)."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

F64 = torch.float64


def dgrad_filter(w):
    """w'[c, o, ky, kx] = w[o, c, k-1-ky, k-1-kx]: what s2a_conv_pack_weight_train packs as the input-gradient filter"""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def weight_grad_formula(x, g, k):
    """gw[o, c, ky, kx] = sum over (b, y, x) of g[b, o, y, x] * x[b, c, y + ky - pad, x + kx - pad], zero padding"""
    pad = k // 2
    B, C, H, W = x.shape
    xp = F.pad(x, (pad, pad, pad, pad))
    gw = torch.zeros((g.shape[1], C, k, k), dtype=x.dtype)
    for ky in range(k):
        for kx in range(k):
            gw[:, :, ky, kx] = torch.einsum("boyx,bcyx->oc", g, xp[:, :, ky:ky + H, kx:kx + W])
    return gw


@pytest.mark.parametrize("k", [3, 1])
def test_input_and_weight_gradient_identities(k):
    gen = torch.Generator().manual_seed(3 + k)
    x = torch.randn((2, 5, 6, 7), dtype=F64, generator=gen, requires_grad=True)
    w = torch.randn((4, 5, k, k), dtype=F64, generator=gen, requires_grad=True)
    g = torch.randn((2, 4, 6, 7), dtype=F64, generator=gen)
    F.conv2d(x, w, None, 1, k // 2).backward(g)
    gx = F.conv2d(g, dgrad_filter(w.detach()), None, 1, k // 2)
    assert torch.allclose(gx, x.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(weight_grad_formula(x.detach(), g, k), w.grad, rtol=1e-12, atol=1e-12)


def test_train_kernels_switch_and_cpu_fall_through():
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d
    torch.manual_seed(5)
    assert FusedConv2d(64, 64, 3, 1, 1).own_grad is False
    net = nn.Sequential(FusedConv2d(64, 64, 3, 1, 1, relu=True), nn.ReLU(), nn.Conv2d(64, 64, 1),
                        nn.Sequential(FusedConv2d(64, 128, 1)))
    assert S.train_kernels(net) == 2 and all(m.own_grad for m in net.modules() if isinstance(m, FusedConv2d))
    assert S.train_kernels(net, False) == 2 and not any(m.own_grad for m in net.modules() if isinstance(m, FusedConv2d))
    assert S.train_kernels(nn.ReLU()) == 0
    # flag on, CPU tensors: ineligible, the call falls through to the stock route and equals nn.Conv2d's
    m = FusedConv2d(64, 64, 3, 1, 1, relu=True)
    ref = nn.Conv2d(64, 64, 3, 1, 1)
    ref.load_state_dict(m.state_dict())
    assert S.train_kernels(m) == 1
    x = torch.randn(2, 64, 5, 6, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    assert not S.train_conv_ok(x, m, None)
    y, y2 = m(x), F.relu(ref(x2))
    cot = torch.randn_like(y)
    y.backward(cot)
    y2.backward(cot)
    assert torch.equal(y, y2) and torch.equal(x.grad, x2.grad)
    assert torch.equal(m.weight.grad, ref.weight.grad) and torch.equal(m.bias.grad, ref.bias.grad)


def _abi():
    from s2anet_amd import _lib
    L = _lib.lib()
    return _lib, L, ctypes.c_void_p(0), ctypes.c_void_p(16), ctypes.c_void_p(18), (lambda: L.s2a_last_error().decode())


def test_pack_weight_train_argument_checks_without_touching_the_gpu():
    _lib, L, z, one, odd, msg = _abi()

    def call(w=one, dt=_lib.DTYPE_F32, O=64, C=64, k=3, fwd=one, dg=one):
        return L.s2a_conv_pack_weight_train(w, dt, O, C, k, fwd, dg, z)
    assert call(k=2) == _lib.EINVAL and "kernel size" in msg()
    assert call(dt=_lib.DTYPE_F64) == _lib.EINVAL and "dtype" in msg()
    for O, C in ((32, 64), (64, 96), (0, 64), (64, -64)):
        assert call(O=O, C=C) == _lib.EINVAL and "bad shape" in msg(), (O, C)
    assert call(O=1 << 14, C=1 << 14) == _lib.EINVAL and "32-bit" in msg()
    assert call(w=z) == _lib.EINVAL and "NULL" in msg()
    assert call(fwd=z) == _lib.EINVAL and "NULL" in msg()
    for kw in (dict(w=odd), dict(fwd=odd), dict(dg=odd)):
        assert call(**kw) == _lib.EINVAL and "aligned" in msg(), kw


def test_backward_prep_argument_checks_without_touching_the_gpu():
    _lib, L, z, one, odd, msg = _abi()

    def call(go=one, out=one, g=one, gb=one, dt=_lib.DTYPE_F32, P=100, O=64, ws=one, nbytes=1 << 20):
        return L.s2a_conv_backward_prep_f16(go, out, g, gb, dt, P, O, ws, nbytes, z)
    for P, O in ((-1, 64), (10, 0), (10, 72)):
        assert call(P=P, O=O) == _lib.EINVAL and "bad shape" in msg(), (P, O)
    assert call(P=1 << 24, O=64) == _lib.EINVAL and "32-bit" in msg()
    assert call(dt=_lib.DTYPE_F64) == _lib.EINVAL and "dtype" in msg()
    assert call(out=z) == _lib.EINVAL and "forward output" in msg()
    assert call(go=z) == _lib.EINVAL and "NULL" in msg()
    for kw in (dict(go=odd), dict(out=odd), dict(g=odd), dict(gb=odd), dict(ws=odd)):
        assert call(**kw) == _lib.EINVAL and "aligned" in msg(), kw
    assert call(ws=z) == _lib.EWORKSPACE and "workspace" in msg()
    assert call(nbytes=16) == _lib.EWORKSPACE and "workspace" in msg()
    assert call(P=0) == _lib.OK
    assert call(g=z, gb=z) == _lib.OK and call(out=z, g=z, gb=z) == _lib.OK        # nothing to write: no launch
    assert L.s2a_conv_backward_prep_f16_workspace_bytes(100, 64) >= 4 * 64 * 4
    assert L.s2a_conv_backward_prep_f16_workspace_bytes(100, 72) == 0


def test_backward_weight_argument_checks_without_touching_the_gpu():
    _lib, L, z, one, odd, msg = _abi()

    def call(x=one, g=one, gw=one, dt=_lib.DTYPE_F32, B=1, C=64, H=8, W=8, O=64, k=3, ws=one, nbytes=1 << 40):
        return L.s2a_conv_backward_weight_f16(x, g, gw, dt, B, C, H, W, O, k, ws, nbytes, z)
    assert call(k=5) == _lib.EINVAL and "kernel size" in msg()
    for kw in (dict(B=-1), dict(C=0), dict(H=0), dict(W=-3), dict(O=0)):
        assert call(**kw) == _lib.EINVAL and "bad shape" in msg(), kw
    for kw in (dict(C=32), dict(O=96), dict(C=65)):
        assert call(**kw) == _lib.EINVAL and "multiples of 64" in msg(), kw
    assert call(B=1 << 12, H=1 << 10, W=1 << 10) == _lib.EINVAL and "32-bit" in msg()
    assert call(O=2048, B=64, H=128, W=128) == _lib.EINVAL and "32-bit" in msg()       # the output gradient is too large
    assert call(dt=_lib.DTYPE_F64) == _lib.EINVAL and "dtype" in msg()
    for kw in (dict(x=z), dict(g=z), dict(gw=z)):
        assert call(**kw) == _lib.EINVAL and "NULL" in msg(), kw
    for kw in (dict(x=odd), dict(g=odd), dict(gw=odd), dict(ws=odd)):
        assert call(**kw) == _lib.EINVAL and "aligned" in msg(), kw
    assert call(ws=z) == _lib.EWORKSPACE and "workspace" in msg()
    assert call(nbytes=1024) == _lib.EWORKSPACE and "workspace" in msg()
    assert call(B=0) == _lib.OK
    for k in (3, 1):            # O above 256 goes in out-channel groups; the split depends on the shapes only
        n = L.s2a_conv_backward_weight_f16_workspace_bytes(2, 128, 9, 21, 320, k)
        assert n >= 2 * 2 * k * 256 * k * 64 * 4 and n == L.s2a_conv_backward_weight_f16_workspace_bytes(2, 128, 9, 21, 320, k)
    assert L.s2a_conv_backward_weight_f16_workspace_bytes(2, 96, 9, 21, 64, 3) == 0
