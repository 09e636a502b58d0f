"""oracle/twin64.py, the float64 twin of tests/test_gpu_autograd_twin.py, checked on the CPU:
  1. torch.autograd.gradcheck of every twin function at tiny float64 shapes (the twin's autograd is the GPU test's
     gradient reference, so it has to be the derivative of what the twin computes);
  2. the folded bottleneck and the FPN against stock nn.Conv2d / nn.BatchNorm2d(eval) / nn.ReLU modules in float64
     (the fold is an affine re-parametrisation: outputs and input gradients agree to float64 rounding);
  3. the index gather, the offsets and the pooling against the oracle's own restatements."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import gradcheck

import oracle
from oracle import twin64 as T

F64 = torch.float64


def rnd(*shape, scale=1.0, grad=True, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    return (torch.randn(*shape, dtype=F64) * scale).requires_grad_(grad)


def anchors_for(B, H, W, stride, seed=0):
    """rotated, shifted anchors around the grid (x, y, w, h, angle)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.from_numpy(oracle.grid_anchors(H, W, stride)).view(1, H, W, 5).repeat(B, 1, 1, 1).clone()
    a[..., :2] += torch.randn((B, H, W, 2), generator=g) * 3
    a[..., 4] = torch.rand((B, H, W), generator=g) * 3.0 - 0.7
    return a


# ----------------------------------------------------------------------------- 1. gradcheck
def test_gradcheck_fused_conv():
    torch.manual_seed(0)
    x, w, b = rnd(2, 3, 5, 4), rnd(4, 3, 3, 3), rnd(4)
    r = rnd(2, 4, 5, 4)
    assert gradcheck(lambda x, w, b, r: T.fused_conv(x, w, b, 1, 1, True, r), (x, w, b, r))
    x2, w2, b2 = rnd(2, 3, 5, 4), rnd(4, 3, 1, 1), rnd(4)
    assert gradcheck(lambda x, w, b: T.fused_conv(x, w, b, 2, 0, False), (x2, w2, b2))


def _bottleneck_leaves(cin, planes, stride, down):
    p = {"conv1": (rnd(planes, cin, 1, 1, scale=0.5), rnd(planes, scale=0.3)),
         "conv2": (rnd(planes, planes, 3, 3, scale=0.3), rnd(planes, scale=0.3)),
         "conv3": (rnd(4 * planes, planes, 1, 1, scale=0.5), rnd(4 * planes, scale=0.3)),
         "stride": stride, "down": (rnd(4 * planes, cin, 1, 1, scale=0.5), rnd(4 * planes, scale=0.3)) if down else None}
    return p


def _flat_convs(p):
    out = []
    for k in ("conv1", "conv2", "conv3", "down"):
        if p.get(k) is not None:
            out += list(p[k])
    return out


def _rebuild_bottleneck(p, flat):
    q, i = dict(p), 0
    for k in ("conv1", "conv2", "conv3", "down"):
        if p.get(k) is not None:
            q[k] = (flat[i], flat[i + 1])
            i += 2
    return q


def test_gradcheck_bottleneck_folded():
    torch.manual_seed(1)
    for cin, stride, down in ((8, 1, False), (4, 2, True)):
        p = _bottleneck_leaves(cin, 2, stride, down)
        x = rnd(2, cin, 5, 4)
        assert gradcheck(lambda x, *flat: T.bottleneck_folded(x, _rebuild_bottleneck(p, flat)), (x, *_flat_convs(p)))


def test_gradcheck_trunk_folded():
    torch.manual_seed(2)
    stem = (rnd(4, 3, 7, 7, scale=0.2), rnd(4, scale=0.2))
    p1, p2 = _bottleneck_leaves(4, 1, 1, True), _bottleneck_leaves(4, 1, 2, True)
    imgs = rnd(1, 3, 12, 10)

    def f(imgs, sw, sb, *flat):
        n = len(_flat_convs(p1))
        tr = {"stem": (sw, sb), "stages": [[_rebuild_bottleneck(p1, flat[:n])], [_rebuild_bottleneck(p2, flat[n:])]]}
        return T.trunk_folded(imgs, tr, out_indices=(1, 2))
    assert gradcheck(f, (imgs, *stem, *_flat_convs(p1), *_flat_convs(p2)))


def _fpn_leaves(cins, co):
    lat = [(rnd(co, c, 1, 1, scale=0.4), rnd(co, scale=0.3)) for c in cins]
    out = [(rnd(co, co, 3, 3, scale=0.3), rnd(co, scale=0.3)) for _ in cins]
    out.append((rnd(co, cins[-1], 3, 3, scale=0.3), rnd(co, scale=0.3)))
    out.append((rnd(co, co, 3, 3, scale=0.3), rnd(co, scale=0.3)))
    return lat, out


def test_gradcheck_fpn():
    torch.manual_seed(3)
    cins, co = (2, 3), 2
    lat, out = _fpn_leaves(cins, co)
    xs = [rnd(1, 2, 6, 4), rnd(1, 3, 3, 2)]
    flat = [t for c in lat + out for t in c]

    def f(x0, x1, *flat):
        convs = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]
        return T.fpn([x0, x1], {"lateral": convs[:2], "fpn": convs[2:]})
    assert gradcheck(f, (*xs, *flat))


def test_gradcheck_arf_expand_and_rot_pool():
    torch.manual_seed(4)
    idx = torch.from_numpy(oracle.arf_indices(1, 8, 3))
    w = rnd(2, 3, 1, 3, 3)
    assert gradcheck(lambda w: T.arf_expand(w, idx), (w,))
    x = rnd(2, 16, 3, 2)
    assert gradcheck(lambda x: T.rot_pool(x, 8), (x,))
    b = rnd(16)
    xi = rnd(1, 3, 4, 3)
    assert gradcheck(lambda x, w, b: T.orconv_pool(x, w, b, idx), (xi, w, b))


def test_gradcheck_deform_conv64_and_align_conv():
    torch.manual_seed(5)
    B, C, O, H, W = 1, 2, 3, 4, 5
    x, w = rnd(B, C, H, W), rnd(O, C, 3, 3)
    off = rnd(B, 18, H, W, scale=1.3)
    from oracle.dcn64 import deform_conv64
    assert gradcheck(deform_conv64, (x, off, w))
    anc = anchors_for(B, H, W, 8, seed=1)
    assert gradcheck(lambda x, w: T.align_conv(x, anc, w, 8), (x, w))
    # a map smaller than the kernel (the head's last levels), where DeformConv pads and crops
    x2 = rnd(1, C, 1, 2)
    anc2 = anchors_for(1, 1, 2, 128, seed=2)
    assert gradcheck(lambda x, w: T.align_conv(x, anc2, w, 128), (x2, w))


def _head_leaves(cin, cf, ncls):
    torch.manual_seed(6)
    P = {}
    for name, c0 in (("fam_reg_ls", cin), ("fam_cls_ls", cin), ("odm_reg_ls", cf), ("odm_cls_ls", cf // 8)):
        for i in range(2):
            P["%s.%d.0.weight" % (name, i)] = rnd(cf, c0 if i == 0 else cf, 3, 3, scale=0.2)
            P["%s.%d.0.bias" % (name, i)] = rnd(cf, scale=0.2)
    for name, o, k in (("fam_reg_head", 5, 1), ("fam_cls_head", ncls, 1), ("odm_cls_head", ncls, 3), ("odm_reg_head", 5, 3)):
        P[name + ".weight"], P[name + ".bias"] = rnd(o, cf, k, k, scale=0.2), rnd(o, scale=0.2)
    P["align_conv.deform_conv.weight"] = rnd(cf, cin, 3, 3, scale=0.2)
    P["or_conv.weight"], P["or_conv.bias"] = rnd(cf // 8, cf, 1, 3, 3, scale=0.2), rnd(cf, scale=0.2)
    return P


def test_gradcheck_head_single():
    P = _head_leaves(8, 8, 2)
    idx = torch.from_numpy(oracle.arf_indices(1, 8, 3))
    names = sorted(P)
    x = rnd(1, 8, 3, 4)
    anc = anchors_for(1, 3, 4, 8, seed=3)

    def f(x, *vals):
        Q = dict(zip(names, vals))
        Q["or_conv.indices"] = idx
        return T.head_single(x, 8, Q, anc)
    # ~6 000 parameter entries: the random-projection form checks the same Jacobian in a handful of evaluations
    assert gradcheck(f, (x, *[P[n] for n in names]), fast_mode=True)


# ----------------------------------------------------------------------------- 2. against stock modules
def _bn(c, g):
    bn = nn.BatchNorm2d(c).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g, dtype=F64) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g, dtype=F64) * 0.2)
        bn.running_mean.copy_(torch.randn(c, generator=g, dtype=F64) * 0.2)
        bn.running_var.copy_(torch.rand(c, generator=g, dtype=F64) + 0.5)
    return bn.eval()


def _fold(conv, bn):
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    b = conv.bias if conv.bias is not None else torch.zeros_like(bn.running_mean)
    return ((conv.weight * s.view(-1, 1, 1, 1)).detach(), ((b - bn.running_mean) * s + bn.bias).detach())


def test_bottleneck_twin_equals_stock_modules():
    g = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    for cin, planes, stride, down in ((16, 4, 1, False), (8, 4, 2, True)):
        c1, c2 = nn.Conv2d(cin, planes, 1, bias=False).double(), nn.Conv2d(planes, planes, 3, stride, 1, bias=False).double()
        c3 = nn.Conv2d(planes, 4 * planes, 1, bias=False).double()
        b1, b2, b3 = _bn(planes, g), _bn(planes, g), _bn(4 * planes, g)
        relu = nn.ReLU()
        ds = (nn.Conv2d(cin, 4 * planes, 1, stride, bias=False).double(), _bn(4 * planes, g)) if down else None
        x = rnd(2, cin, 7, 5)
        out = b3(c3(relu(b2(c2(relu(b1(c1(x))))))))
        ref = relu(out + (ds[1](ds[0](x)) if down else x))
        go = torch.randn(ref.shape, dtype=F64)
        (gx_ref,) = torch.autograd.grad(ref, x, go)
        p = {"conv1": _fold(c1, b1), "conv2": _fold(c2, b2), "conv3": _fold(c3, b3), "stride": stride,
             "down": _fold(*ds) if down else None}
        y = T.bottleneck_folded(x, p)
        (gx,) = torch.autograd.grad(y, x, go)
        assert torch.allclose(y, ref, rtol=1e-11, atol=1e-11)
        assert torch.allclose(gx, gx_ref, rtol=1e-11, atol=1e-11)


def test_fpn_twin_equals_stock_modules():
    torch.manual_seed(8)
    cins, co = (4, 6, 8), 4
    lat = [nn.Conv2d(c, co, 1).double() for c in cins]
    out = [nn.Conv2d(co, co, 3, padding=1).double() for _ in cins]
    out += [nn.Conv2d(cins[-1], co, 3, 2, 1).double(), nn.Conv2d(co, co, 3, 2, 1).double()]
    xs = [rnd(2, 4, 8, 12), rnd(2, 6, 4, 6), rnd(2, 8, 2, 3)]
    la = [l(x) for l, x in zip(lat, xs)]
    la[1] = la[1] + F.interpolate(la[2], scale_factor=2, mode="nearest")
    la[0] = la[0] + F.interpolate(la[1], scale_factor=2, mode="nearest")
    ref = [out[i](la[i]) for i in range(3)]
    ref.append(out[3](xs[-1]))
    ref.append(out[4](ref[-1]))
    got = T.fpn(xs, T.fpn_params(type("N", (), {"lateral_convs": lat, "fpn_convs": out})))
    assert [tuple(t.shape[2:]) for t in got] == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    gos = [torch.randn(t.shape, dtype=F64) for t in ref]
    g_ref = torch.autograd.grad(ref, xs, gos)
    g_got = torch.autograd.grad(got, xs, gos)
    for a, b in zip(list(got) + list(g_got), ref + list(g_ref)):
        assert torch.allclose(a, b, rtol=1e-11, atol=1e-11)


# ----------------------------------------------------------------------------- 3. against the oracle's restatements
def test_arf_expand_equals_oracle():
    rng = np.random.default_rng(9)
    for n_ori, n_rot in ((1, 8), (8, 8), (4, 4)):
        idx = oracle.arf_indices(n_ori, n_rot, 3)
        w = rng.standard_normal((3, 2, n_ori, 3, 3)).astype(np.float32)
        ref = oracle.arf_forward(w, idx)
        got = T.arf_expand(torch.from_numpy(w), torch.from_numpy(idx), torch.float32).numpy()
        assert np.array_equal(got, ref)


def test_align_offsets_equals_oracle():
    B, H, W, stride = 2, 5, 7, 16
    anc = anchors_for(B, H, W, stride, seed=10)
    got = T.align_offsets(anc, stride).numpy()
    for b in range(B):
        ref = oracle.align_offsets(anc[b].reshape(-1, 5).numpy(), H, W, stride)        # float32 arithmetic
        assert np.abs(got[b] - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    assert T.align_offsets(anc, stride, dtype=torch.float32).dtype == torch.float32


def test_rot_pool_equals_oracle_and_any_layout():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 16, 3, 5)).astype(np.float32)
    ref = oracle.rot_inv_pool(x, 8)
    t = torch.from_numpy(x)
    assert np.array_equal(T.rot_pool(t, 8, torch.float32).numpy(), ref)
    assert np.array_equal(T.rot_pool(t.contiguous(memory_format=torch.channels_last), 8, torch.float32).numpy(), ref)


def test_lower_precision_twin_is_the_same_code():
    """the f32 / f16 baseline is the same function at another dtype: close to float64, in its own type"""
    torch.manual_seed(12)
    x, w, b = rnd(2, 8, 5, 6, grad=False), rnd(8, 8, 3, 3, scale=0.1, grad=False), rnd(8, grad=False)
    y64 = T.fused_conv(x, w, b, 1, 1, True)
    y32 = T.fused_conv(x.float(), w.float(), b.float(), 1, 1, True, dtype=torch.float32)
    assert y32.dtype == torch.float32 and float((y32.double() - y64).norm() / y64.norm()) < 1e-6
    anc = anchors_for(2, 5, 6, 8, seed=13)
    a64 = T.align_conv(x, anc, w, 8)
    a32 = T.align_conv(x.float(), anc, w.float(), 8, dtype=torch.float32)
    assert a32.dtype == torch.float32 and float((a32.double() - a64).norm() / a64.norm()) < 1e-5
