"""CPU: the host side of the opt-in e4m3 tower route (s2anet_amd/fp8.py, csrc/conv_fp8_ops.hip).

  * quantize_weight_e4m3: every byte is a finite e4m3fn value, |w - s_w deq(w_q)| <= 2^-4 |w| + s_w 2^-10 (half an ulp of a
    normal e4m3 value relative to it, half a subnormal step in absolute terms), an all-zero filter gets scale 1;
  * the three entry points refuse C = 64, O = 32 and NULL tensors with S2A_EINVAL before any HIP call;
  * header, library and binding declare the three symbols."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

SYMS = ("s2a_quantize_e4m3", "s2a_conv_pack_weight_fp8", "s2a_conv3x3_pyramid_fp8")


def test_quantize_weight_e4m3_error_bound_and_zero_filter():
    from s2anet_amd.fp8 import dequantize_e4m3, quantize_weight_e4m3
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 128, 3, 3, generator=g) * 0.01
    w[3] = 0                                   # an all-zero filter
    w[5] *= 1e-4                               # a tiny one
    w[7, 0, 0, 0] = 3.0                        # one outlier: the rest of the filter lands in e4m3's subnormal range
    w[9] = w[9].half().float()
    wq, s = quantize_weight_e4m3(w)
    assert wq.dtype == torch.uint8 and wq.shape == w.shape and s.dtype == torch.float32 and s.shape == (64,)
    assert int(((wq & 0x7f) == 0x7f).sum()) == 0            # 0x7f / 0xff are e4m3fn's only non-finite encodings (NaN)
    assert s[3].item() == 1.0 and not wq[3].any()
    assert torch.equal(s[[0, 7]], (w[[0, 7]].abs().amax(dim=(1, 2, 3)) / 448))
    deq = dequantize_e4m3(wq).double()
    assert deq.abs().max().item() <= 448
    s64 = s.double().view(-1, 1, 1, 1)
    err = (w.double() - s64 * deq).abs()
    bound = 2.0 ** -4 * w.double().abs() + s64 * 2.0 ** -10
    assert bool((err <= bound).all()), (err - bound).max().item()
    # the largest entry of a filter maps to +-448 exactly
    assert torch.equal(deq.abs().amax(dim=(1, 2, 3))[[0, 5, 7]], torch.full((3,), 448.0, dtype=torch.float64))
    # f16 filters (the model's dtype) take the same route
    wq16, s16 = quantize_weight_e4m3(w[9:10].half())
    assert torch.equal(wq16, wq[9:10]) and torch.equal(s16, s[9:10])


def test_argument_checks_return_codes_without_touching_the_gpu():
    from s2anet_amd import _lib
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(1 << 20)     # never dereferenced: the checks fail first
    odd = ctypes.c_void_p((1 << 20) + 2)

    def msg():
        return L.s2a_last_error().decode()
    pyr = _lib.Pyramid()
    pyr.n_levels = 1
    pyr.height[0], pyr.width[0], pyr.stride[0] = 9, 17, 8.0
    P = ctypes.byref(pyr)

    def conv(x=one, w=one, s=one, b=one, out=one, C=256, O=256, pyramid=P):
        return L.s2a_conv3x3_pyramid_fp8(x, w, s, b, out, 0, 1.0, 1, C, O, 1, pyramid, z)
    assert conv(C=64) == _lib.EINVAL and "multiple of 128" in msg()
    assert conv(C=192) == _lib.EINVAL and "multiple of 128" in msg()
    assert conv(O=32) == _lib.EINVAL and "multiple of 64" in msg()
    for k in ("x", "w", "s", "b", "out"):
        assert conv(**{k: z}) == _lib.EINVAL and "NULL" in msg(), k
    assert conv(x=odd) == _lib.EINVAL and "aligned" in msg()
    bad = _lib.Pyramid()
    bad.n_levels = 0
    assert conv(pyramid=ctypes.byref(bad)) == _lib.EINVAL and "level table" in msg()
    # quantise: channels a multiple of 16, NULL
    assert L.s2a_quantize_e4m3(one, one, 4, 24, 1.0, z) == _lib.EINVAL and "multiple of 16" in msg()
    assert L.s2a_quantize_e4m3(z, one, 4, 64, 1.0, z) == _lib.EINVAL and "NULL" in msg()
    assert L.s2a_quantize_e4m3(one, z, 4, 64, 1.0, z) == _lib.EINVAL and "NULL" in msg()
    assert L.s2a_quantize_e4m3(one, one, 0, 64, 1.0, z) == _lib.OK            # nothing to do
    # filter pack
    assert L.s2a_conv_pack_weight_fp8(one, 256, 64, one, z) == _lib.EINVAL and "multiple of 128" in msg()
    assert L.s2a_conv_pack_weight_fp8(one, 32, 128, one, z) == _lib.EINVAL and "multiple of 64" in msg()
    assert L.s2a_conv_pack_weight_fp8(z, 256, 256, one, z) == _lib.EINVAL and "NULL" in msg()
    assert L.s2a_conv_pack_weight_fp8(one, 256, 256, z, z) == _lib.EINVAL and "NULL" in msg()


def test_header_library_and_binding_declare_the_symbols():
    from s2anet_amd import _lib
    txt = open(os.path.join(ROOT, "include", "s2anet_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.lib()
    for n in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in _lib.SYMBOLS and hasattr(L, n), n


def test_switch_raises_before_calibration_and_surface_is_exported():
    import s2anet_amd as S
    from s2anet_amd.head import S2ANetHead
    head = S2ANetHead(num_classes=15)
    assert head.fp8_enabled is False and head.fp8_scales is None
    with pytest.raises(RuntimeError, match="calibrate"):
        S.fp8_towers(head)
    assert S.fp8_towers(head, False) is head and head.fp8_enabled is False
    keys = list(head.state_dict())
    S.calibrate_fp8(head, None, scales={"x": 0.5, "or_feat": 0.25, "odm_reg_ls0": 0.125, "odm_cls_ls0": 1.0})
    assert head.fp8_scales["or_feat"] == 0.25 and list(head.state_dict()) == keys      # plain attributes
    with pytest.raises(RuntimeError, match="fused head"):
        S.fp8_towers(head)                     # plain nn.Conv2d towers: the route needs FusedConv2d layers
    with pytest.raises(ValueError):
        S.calibrate_fp8(head, None, scales={"x": 0.0, "or_feat": 0.25, "odm_reg_ls0": 0.125, "odm_cls_ls0": 1.0})
