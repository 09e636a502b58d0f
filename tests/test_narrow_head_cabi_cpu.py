"""CPU: s2a_conv3x3_narrow_pyramid_f16 refuses bad arguments with S2A_EINVAL before any HIP call, and an empty batch is
nothing to do (the conventions of tests/test_cabi_cpu.py)."""
import ctypes

import pytest


@pytest.fixture
def call(monkeypatch):
    from s2anet_amd import _lib
    monkeypatch.delenv("S2A_CONV_NARROW", raising=False)
    monkeypatch.delenv("S2A_CONV_NARROW_WGS", raising=False)
    L = _lib.lib()
    pyr = _lib.Pyramid()
    pyr.n_levels = 2
    pyr.height[0], pyr.width[0], pyr.stride[0] = 8, 8, 8.0
    pyr.height[1], pyr.width[1], pyr.stride[1] = 3, 3, 16.0
    one = ctypes.c_void_p(1 << 20)      # never dereferenced: the checks fail first

    def f(x=one, w=one, b=one, out=one, batch=1, channels=256, used=5, pyramid=pyr):
        rc = L.s2a_conv3x3_narrow_pyramid_f16(x, w, b, out, batch, channels, used, 0, ctypes.byref(pyramid), ctypes.c_void_p(0))
        return rc, L.s2a_last_error().decode()
    return f


def test_null_and_misaligned_tensors(call):
    z = ctypes.c_void_p(0)
    for kw in (dict(x=z), dict(w=z), dict(out=z)):
        rc, msg = call(**kw)
        assert rc == -1 and "NULL" in msg, kw
    for name, off in (("x", 2), ("w", 8), ("out", 4), ("b", 2)):
        rc, msg = call(**{name: ctypes.c_void_p((1 << 20) + off)})
        assert rc == -1 and "aligned" in msg, name


@pytest.mark.parametrize("used", [0, 17, -1])
def test_out_channels_used_range(call, used):
    rc, msg = call(used=used)
    assert rc == -1 and "1..16" in msg


@pytest.mark.parametrize("channels", [32, 0, 96])
def test_channels_must_be_a_multiple_of_64(call, channels):
    rc, msg = call(channels=channels)
    assert rc == -1 and ("multiple of 64" in msg or "bad shape" in msg)


def test_bad_level_table(call):
    from s2anet_amd import _lib
    for n, h in ((0, 8), (9, 8), (1, 0)):
        pyr = _lib.Pyramid()
        pyr.n_levels = n
        pyr.height[0], pyr.width[0], pyr.stride[0] = h, 8, 8.0
        rc, msg = call(pyramid=pyr)
        assert rc == -1 and "level table" in msg, (n, h)


def test_input_too_large_for_32_bit_offsets(call):
    rc, msg = call(batch=1 << 20)
    assert rc == -1 and "32-bit" in msg


def test_empty_batch_is_ok(call):
    z = ctypes.c_void_p(0)
    assert call(x=z, w=z, b=z, out=z, batch=0)[0] == 0
    assert call(batch=-1)[0] == -1


def test_switch_off_keeps_the_checks(call, monkeypatch):
    """S2A_CONV_NARROW=0 hands the call to the 64-row launch: the range checks of this entry point still come first, and
    that launch's own checks refuse the rest"""
    monkeypatch.setenv("S2A_CONV_NARROW", "0")
    assert call(used=17)[0] == -1 and call(channels=32)[0] == -1
    rc, msg = call(x=ctypes.c_void_p(0))
    assert rc == -1 and "NULL" in msg
    assert call(batch=0)[0] == 0
