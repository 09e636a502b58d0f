"""GPU: AlignConvFunction.backward computes the gradients that are wanted and no other.  B = 2, C = 64, 5 x 7, stride 8:
the smallest sizes inside both gradients' limits (dcn._fused_bwd_ok) that leave a ragged tile in each kernel, with O = 64,
the smallest out_channels the function's forward (s2a_align_conv_forward) takes.  The library object is wrapped in a
proxy that records every entry point called with its arguments; no kernel is touched.

The kept gradient comes from the same kernel as when both are wanted, so: the filter gradient (fixed-order reduce) is
bit-equal in both types, the f16 input gradient is bit-equal in deterministic mode, and the f32 input gradient (float
atomics, never reproducible) stays within the elementwise bound tests/test_gpu_dcn_backward_shapes.py derives for that
kernel -- each run is within tau * S + tiny of the float64 reference, two runs within twice that of each other."""
import pytest
import torch

from test_gpu_dcn_backward_shapes import reference, refined_anchors, tau

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, C, O, H, W, STRIDE = 2, 64, 64, 5, 7, 8
PATTERNS = {"all": (True, True), "x_frozen": (False, True), "filter_frozen": (True, False)}    # (x, filter) want a gradient
IDS = {torch.float16: "f16", torch.float32: "f32"}


def gradients_taken(name, args):
    """-> (input, weight): does this library call take a non-NULL output pointer for that gradient?"""
    given = lambda p: bool(getattr(p, "value", p))
    if name in ("s2a_deform_conv_backward", "s2a_deform_conv_backward_typed"):
        return given(args[5]), given(args[7])
    if name in ("s2a_deform_conv_backward_input_f16", "s2a_deform_conv_backward_input_f32", "s2a_deformable_col2im",
                "s2a_deformable_col2im_coord"):
        return True, False
    if name in ("s2a_deform_conv_backward_weight_f16", "s2a_deform_conv_backward_weight_f32", "s2a_deformable_im2col"):
        return False, True
    return False, False


class Recorder:
    """stands in for the object _lib.lib() returns: every function called through it is logged as (name, args)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


@pytest.fixture
def recorder(monkeypatch):
    from s2anet_amd import _lib
    for name in ("S2A_DCN_BWD_UNFUSED", "S2A_DCN_BWD_SEPARATE", "S2A_BWD_F32_WEIGHT", "S2A_DCN_F32"):
        monkeypatch.delenv(name, raising=False)
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def tensors(dtype):
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn((B, C, H, W), device=DEV, generator=gen).to(dtype)
    w = (torch.randn((O, C, 3, 3), device=DEV, generator=gen) / (9 * C) ** 0.5).to(dtype)
    anchors = refined_anchors(gen, B, H, W, STRIDE)
    cot = torch.randn((B, O, H, W), device=DEV, generator=gen).to(dtype)
    return x, w, anchors, cot


def run(rec, dtype, pattern):
    """forward + backward of AlignConvFunction -> (x.grad, filter.grad, out, the calls of the backward)"""
    from s2anet_amd import AlignConvFunction
    x, w, anchors, cot = tensors(dtype)
    want_x, want_w = PATTERNS[pattern]
    x.requires_grad_(want_x)
    w.requires_grad_(want_w)
    out = AlignConvFunction.apply(x, anchors, w, STRIDE)
    del rec.calls[:]
    out.backward(cot)
    torch.cuda.synchronize()
    return x.grad, w.grad, out.detach(), list(rec.calls)


@pytest.mark.parametrize("dtype", tuple(IDS), ids=tuple(IDS.values()))
def test_frozen_patterns_take_only_the_wanted_gradient(recorder, dtype):
    gx_all, gw_all, out, calls = run(recorder, dtype, "all")
    taken = [gradients_taken(*c) for c in calls]
    assert any(i for i, _ in taken) and any(w for _, w in taken), [n for n, _ in calls]
    assert gx_all is not None and gw_all is not None

    gx, gw, _, calls = run(recorder, dtype, "x_frozen")
    assert not any(gradients_taken(*c)[0] for c in calls), [n for n, _ in calls]
    assert any(gradients_taken(*c)[1] for c in calls)
    assert gx is None and torch.equal(gw, gw_all)

    gx, gw, _, calls = run(recorder, dtype, "filter_frozen")
    assert not any(gradients_taken(*c)[1] for c in calls), [n for n, _ in calls]
    assert any(gradients_taken(*c)[0] for c in calls)
    assert gw is None and gx.shape == gx_all.shape and gx.dtype == dtype
    if dtype == torch.float32:
        from s2anet_amd.alignconv import align_offsets
        x, w, anchors, cot = tensors(dtype)
        off = align_offsets(anchors.reshape(B, H * W, 5), (H, W), STRIDE)
        ref = reference(x, off, w, cot.masked_fill(out <= 0, 0))
        bound = tau(dtype, "x3", "input", C, O, 0, 0) * ref["S_input"] + 1e-30
        for name, g in (("all", gx_all), ("filter_frozen", gx)):
            err = (g.double() - ref["grad_input"]).abs()
            print("f32 input gradient, %s: max err / bound = %.3g" % (name, (err / bound).max().item()))
        assert bool(((gx.double() - gx_all.double()).abs() <= 2 * bound).all())


def test_f16_input_gradient_is_bit_equal_in_deterministic_mode(recorder):
    import s2anet_amd as S
    with S.deterministic(True):
        gx_all, gw_all, _, _ = run(recorder, torch.float16, "all")
        gx, _, _, calls = run(recorder, torch.float16, "filter_frozen")
        assert not any(gradients_taken(*c)[1] for c in calls)
        _, gw, _, _ = run(recorder, torch.float16, "x_frozen")
    assert torch.equal(gx, gx_all) and torch.equal(gw, gw_all)
