"""CPU: dcn._fused_bwd_ok -- the one statement, on the Python side, of what the fused deformable-conv backward kernels take --
against the argument checks of the library itself (fused_bwd_run of csrc/dcn_bwd_ops.hip).  The library is probed with
never-dereferenced pointers and a workspace of 0 bytes: S2A_EWORKSPACE means every argument check passed, S2A_EINVAL that
the shape was refused; no call gets as far as a launch."""
import ctypes
import itertools

import pytest
import torch

DTYPES = (torch.float16, torch.float32)
CHANNELS = (8, 16, 32, 48, 64, 96, 128, 4096, 4128, 4160, 6784, 6848)
OUT_CHANNELS = (8, 16, 24, 32, 48, 64, 256, 272, 288)
MAPS = ((2, 7), (7, 2), (3, 3), (5, 7))
WANTS = ((True, False), (False, True), (True, True))               # (input, weight)
GRID = tuple(itertools.product(DTYPES, CHANNELS, OUT_CHANNELS, MAPS, WANTS))


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("S2A_DCN_BWD_UNFUSED", "S2A_DCN_BWD_SEPARATE", "S2A_DCN_COLUMNS_MB"):
        monkeypatch.delenv(name, raising=False)


def _library_answer(dtype, C, O, H, W, want_input, want_weight):
    from s2anet_amd import _lib
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)          # never dereferenced: the checks fail first
    code = _lib.DTYPE_F16 if dtype == torch.float16 else _lib.DTYPE_F32
    return _lib.lib().s2a_deform_conv_backward_typed(code, one, one, one, one, one if want_input else z, one,
                                                     one if want_weight else z, 1.0, 1, C, H, W, O, one, 0, z)


def test_predicate_against_the_library_on_the_grid():
    from s2anet_amd import _lib
    from s2anet_amd.dcn import _ALIGN_GEOMETRY, _fused_bwd_ok
    assert len(GRID) == 2592
    assert not _lib.deterministic()
    for dtype, C, O, (H, W), (want_input, want_weight) in GRID:
        ok = _fused_bwd_ok(dtype, _ALIGN_GEOMETRY, C, O, H, W, want_input, want_weight)
        rc = _library_answer(dtype, C, O, H, W, want_input, want_weight)
        point = (dtype, C, O, H, W, want_input, want_weight)
        if ok:
            assert rc == _lib.EWORKSPACE, point                    # never wider than the library
        elif C <= 4096:
            assert rc == _lib.EINVAL, point                        # and below the cap not narrower either


def test_the_channel_cap_is_narrower_than_the_library():
    """whoever lifts dcn._FUSED_WGRAD_MAX_CHANNELS meets this line: the library takes the weight gradient up to C = 6784,
    the predicate stops at 4096 because no test runs the fused weight gradient above it"""
    from s2anet_amd import _lib
    from s2anet_amd.dcn import _ALIGN_GEOMETRY, _FUSED_WGRAD_MAX_CHANNELS, _fused_bwd_ok
    assert _FUSED_WGRAD_MAX_CHANNELS == 4096
    for dtype in DTYPES:
        for want_input in (False, True):
            assert not _fused_bwd_ok(dtype, _ALIGN_GEOMETRY, 4160, 32, 5, 7, want_input, True)
            assert _library_answer(dtype, 4160, 32, 5, 7, want_input, True) == _lib.EWORKSPACE
        assert _fused_bwd_ok(dtype, _ALIGN_GEOMETRY, 4160, 32, 5, 7, True, False)      # the input gradient has no cap


def test_predicate_refuses_other_types_and_geometries():
    from s2anet_amd.dcn import _ALIGN_GEOMETRY, _fused_bwd_ok
    shape = (64, 32, 5, 7)
    for wants in WANTS:
        assert _fused_bwd_ok(torch.float16, _ALIGN_GEOMETRY, *shape, *wants)
        assert _fused_bwd_ok(torch.float32, list(_ALIGN_GEOMETRY), *shape, *wants)
        assert not _fused_bwd_ok(torch.float64, _ALIGN_GEOMETRY, *shape, *wants)
        assert not _fused_bwd_ok(torch.bfloat16, _ALIGN_GEOMETRY, *shape, *wants)
        # kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group: each single departure
        for i, other in enumerate((1, 5, 2, 2, 0, 2, 2, 2, 2, 2)):
            geometry = _ALIGN_GEOMETRY[:i] + (other,) + _ALIGN_GEOMETRY[i + 1:]
            assert not _fused_bwd_ok(torch.float16, geometry, *shape, *wants), geometry


def test_unfused_switch_refuses_everywhere(monkeypatch):
    from s2anet_amd.dcn import _ALIGN_GEOMETRY, _fused_bwd_ok
    monkeypatch.setenv("S2A_DCN_BWD_UNFUSED", "1")
    for dtype, C, O, (H, W), wants in GRID:
        assert not _fused_bwd_ok(dtype, _ALIGN_GEOMETRY, C, O, H, W, *wants)
