"""CPU: fused.train_shape_problem and norm.bn_shape_problem -- the one statement, on the Python side, of what the dense training
kernels take -- against the library's own pointer-free queries (s2a_conv_nhwc_f16_form, s2a_conv_backward_weight_f16_workspace_bytes,
s2a_conv_backward_weight_s2_slices, s2a_bn_slices).  No HIP call is made and no pointer to a tensor is passed.  The grids reach
into the corners where the two sides once differed: a map side of 32000, a filter of 2^31 bytes, 2^24 channels."""
import ctypes
import itertools

import pytest

WIDTHS = (32, 64, 128, 192, 8192, 16384)
MAPS = ((1, 1, 1), (1, 7, 9), (2, 16, 16), (1, 31999, 1), (1, 32000, 1), (1, 1, 32000), (1, 2, 32000), (8, 256, 256),
        (64, 512, 512))
CONV_GRID = tuple(itertools.product(WIDTHS, WIDTHS, (1, 3), (1, 2), MAPS))          # C, O, k, stride, (B, H, W)

BN_P = (1, 2, 3, 31, 32, 33, 1 << 20, (1 << 24) - 1, 1 << 24, (1 << 30) // 64 - 1, (1 << 30) // 64)
BN_C = (32, 64, 96, 128, 2048, (1 << 24) - 64, 1 << 24)


def _form_ok(L, B, C, H, W, O, k, s):
    form = (ctypes.c_int32 * 6)()
    return L.s2a_conv_nhwc_f16_form(B, C, H, W, O, k, s, form) == 0


def _library_takes(B, C, H, W, O, k, s):
    """the conjunction of the queries: forward, input gradient, weight gradient and pack at stride 1; forward and the strided
    backward's shared shape check at stride 2"""
    from s2anet_amd import _lib
    L = _lib.lib()
    if s == 1:
        return (_form_ok(L, B, C, H, W, O, k, 1) and _form_ok(L, B, O, H, W, C, k, 1) and
                L.s2a_conv_backward_weight_f16_workspace_bytes(B, C, H, W, O, k) > 0 and O * C * k * k * 4 < (1 << 31))
    return _form_ok(L, B, C, H, W, O, k, 2) and L.s2a_conv_backward_weight_s2_slices(B, C, H, W, O, k) > 0


def _predicate_takes(B, C, H, W, O, k, s, **other):
    from s2anet_amd.fused import train_shape_problem
    geometry = dict(ksize=(k, k), stride=(s, s), padding=(k // 2, k // 2), dilation=(1, 1), groups=1)
    geometry.update(other)
    why = train_shape_problem(C=C, O=O, B=B, H=H, W=W, **geometry)
    assert why is None or (isinstance(why, str) and why)
    return why is None


def test_conv_predicate_is_the_library_on_the_grid():
    assert len(CONV_GRID) == 1296
    taken = {1: 0, 2: 0}
    for C, O, k, s, (B, H, W) in CONV_GRID:
        lib = _library_takes(B, C, H, W, O, k, s)
        assert _predicate_takes(B, C, H, W, O, k, s) == lib, ("wider" if not lib else "narrower", C, O, k, s, B, H, W)
        taken[s] += lib
    # the grid's own counts: a change means the library's limits moved, and someone must look at both sides
    assert taken == {1: 202, 2: 156}, taken


def test_batchnorm_predicate_is_the_library_on_the_grid():
    from s2anet_amd import _lib
    from s2anet_amd.norm import bn_shape_problem
    L = _lib.lib()
    taken = 0
    for P, C in itertools.product(BN_P, BN_C):
        lib = L.s2a_bn_slices(P, C) > 0
        assert (bn_shape_problem(P, C) is None) == lib, (P, C)
        taken += lib
    assert len(BN_P) * len(BN_C) == 77 and taken == 24, taken


@pytest.mark.parametrize("k,s", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_each_departure_from_the_geometry_is_refused(k, s):
    at = dict(B=2, C=64, H=16, W=16, O=128, k=k, s=s)
    assert _predicate_takes(**at) and _library_takes(2, 64, 16, 16, 128, k, s)
    p = k // 2
    for other in (dict(ksize=(5, 5)), dict(ksize=(k, 5)), dict(padding=(p + 1, p + 1)), dict(padding=(p, p + 1)),
                  dict(padding=(abs(p - 1), abs(p - 1))), dict(dilation=(2, 2)), dict(dilation=(1, 2)), dict(groups=2),
                  dict(stride=(1, 2)), dict(stride=(2, 1)), dict(stride=(3, 3))):
        assert not _predicate_takes(**at, **other), other
    assert _predicate_takes(**at, ksize=[k, k], stride=[s, s], padding=[p, p], dilation=[1, 1])       # lists as tuples
