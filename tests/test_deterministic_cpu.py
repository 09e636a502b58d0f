"""CPU: the deterministic-mode switch (s2a_set_deterministic / s2anet_amd.deterministic) -- default, setter, context
manager, environment initialisation -- what the workspace queries of the fused deformable-conv backward answer in the
mode, and the refusals of the entries that have no deterministic form, all in front of the first HIP call."""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import ROOT

F32, F16 = 0, 1
RAGGED = (2, 64, 5, 7, 64)


@pytest.fixture(autouse=True)
def _mode_off_before_and_after():
    import s2anet_amd as S
    assert S.deterministic() is False, "a test before this one left the mode on"
    yield
    assert S.deterministic() is False, "this test left the mode on"


def test_default_off_and_the_setter_returns_the_previous_value():
    import s2anet_amd as S
    from s2anet_amd import _lib
    L = _lib.lib()
    assert "deterministic" in S.__all__
    assert L.s2a_get_deterministic() == 0 and S.deterministic() is False
    assert L.s2a_set_deterministic(1) == 0 and L.s2a_get_deterministic() == 1 and S.deterministic() is True
    assert L.s2a_set_deterministic(7) == 1 and L.s2a_get_deterministic() == 1          # any non-zero value is "on"
    assert L.s2a_set_deterministic(0) == 1 and L.s2a_get_deterministic() == 0
    g = S.deterministic(True)
    assert g.previous is False and S.deterministic() is True
    g = S.deterministic(False)
    assert g.previous is True and S.deterministic() is False


def test_context_manager_restores_the_flag_also_after_an_exception():
    import s2anet_amd as S
    with S.deterministic(True):
        assert S.deterministic() is True
        with S.deterministic(False):
            assert S.deterministic() is False
        assert S.deterministic() is True
    assert S.deterministic() is False
    with pytest.raises(ValueError):
        with S.deterministic(True):
            assert S.deterministic() is True
            raise ValueError("inside")
    assert S.deterministic() is False


@pytest.mark.parametrize("value,want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_sets_the_initial_value(value, want):
    env = {k: v for k, v in os.environ.items() if k != "S2A_DETERMINISTIC"}
    if value is not None:
        env["S2A_DETERMINISTIC"] = value
    r = subprocess.run([sys.executable, "-c", "import s2anet_amd as S; print(S.deterministic())"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(want)


def _queries(L):
    return {"input": L.s2a_deform_conv_backward_input_workspace_bytes(*RAGGED),
            "both_f16": L.s2a_deform_conv_backward_workspace_bytes(F16, *RAGGED),
            "both_f32": L.s2a_deform_conv_backward_workspace_bytes(F32, *RAGGED),
            "input_f32": L.s2a_deform_conv_backward_input_f32_workspace_bytes(*RAGGED),
            "weight": L.s2a_deform_conv_backward_weight_workspace_bytes(*RAGGED),
            "weight_f32": L.s2a_deform_conv_backward_weight_f32_workspace_bytes(*RAGGED)}


def test_queries_answer_for_the_current_mode():
    import s2anet_amd as S
    from s2anet_amd import _lib
    L = _lib.lib()
    off = _queries(L)
    with S.deterministic(True):
        on = _queries(L)
        # sizes the entries refuse have no workspace in either mode
        assert L.s2a_deform_conv_backward_input_workspace_bytes(2, 64, 2, 7, 64) == 0
        assert L.s2a_deform_conv_backward_input_workspace_bytes(-1, 64, 5, 7, 64) == 0
        assert L.s2a_deform_conv_backward_workspace_bytes(2, *RAGGED) == 0
        assert L.s2a_deform_conv_backward_workspace_bytes(F16, 2, 0, 5, 7, 64) == 0
    assert _queries(L) == off                                       # back to the default answers, to the byte
    B, C, H, W, _ = RAGGED
    cells = B * C * H * W
    pad = lambda n: (n + 255) // 256 * 256
    # 8-byte cells + one class byte per element in the room of the 4-byte accumulator
    for k in ("input", "both_f16"):
        assert on[k] > off[k] and on[k] - off[k] == pad(9 * cells) - pad(4 * cells), (k, on[k], off[k])
    # nothing else has an accumulator to widen
    for k in ("both_f32", "input_f32", "weight", "weight_f32"):
        assert on[k] == off[k], k


def test_entries_without_a_deterministic_form_refuse_before_any_launch():
    import s2anet_amd as S
    from s2anet_amd import _lib
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(1 << 20)                                   # never dereferenced: the checks fail first
    B, C, H, W, O = RAGGED
    big = 1 << 40

    def msg():
        return L.s2a_last_error().decode()

    def input_f32(gin=one):
        return L.s2a_deform_conv_backward_input_f32(one, one, one, one, gin, one, B, C, H, W, O, one, big, z)

    def typed(dt, gin, gw):
        return L.s2a_deform_conv_backward_typed(dt, one, one, one, one, gin, one, gw, 1.0, B, C, H, W, O, one, 0, z)

    p = _lib.DcnParams(B, C, H, W, O, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, F32, F32, _lib.LAYOUT_NCHW, 0)
    with S.deterministic(True):
        assert input_f32() == _lib.EINVAL and "deterministic" in msg()
        assert input_f32(z) == _lib.EINVAL and "NULL" in msg()       # the NULL checks still come first
        assert typed(F32, one, z) == _lib.EINVAL and "deterministic" in msg()
        assert typed(F32, one, one) == _lib.EINVAL and "deterministic" in msg()
        # weight-only (no atomics) and the f16 forms are not refused for the mode: they get as far as the workspace check
        assert typed(F32, z, one) == _lib.EWORKSPACE and "too small" in msg()
        assert typed(F16, one, one) == _lib.EWORKSPACE and "too small" in msg()
        assert L.s2a_deformable_col2im(one, one, one, ctypes.byref(p), z) == _lib.EINVAL and "deterministic" in msg()
        assert L.s2a_deformable_col2im(z, one, one, ctypes.byref(p), z) == _lib.EINVAL and "NULL" in msg()
        assert L.s2a_deformable_col2im(one, one, one, None, z) == _lib.EINVAL
    # mode off: the same calls get past that check (and stop at the next one that needs no GPU)
    assert typed(F32, one, one) == _lib.EWORKSPACE and "too small" in msg()
    rc = L.s2a_deform_conv_backward_input_f32(one, one, one, one, one, one, B, C, H, W, O, one, 0, z)
    assert rc == _lib.EWORKSPACE and "too small" in msg()


def test_python_routes_refuse_on_cpu_reachable_checks():
    """train_pad_widths answers None for anything but a CUDA f16 channels-last activation: the padded route is never taken
    on the CPU, in either mode"""
    import torch
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d, train_pad_widths
    m = FusedConv2d(64, 15, 3, 1, 1)
    x = torch.zeros(1, 64, 5, 5)
    with S.deterministic(True):
        assert train_pad_widths(x, m) is None
        assert S.train_kernels(torch.nn.ModuleList([m, S.ORConv2d(64, 8, 3, padding=1, arf_config=(1, 8))])) == 1
