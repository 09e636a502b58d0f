"""The head's small kernels (s2anet_amd/csrc/glue_ops.hip) against the float64 references of oracle/glue64.py:

  decode family   k_delta2bbox, k_fam_refine (f32 / f16, NCHW / channels-last), k_fam_refine_pyramid, the decode of
                  k_pyr_gather, k_align_offsets: every element within K * 2^-24 * magnitude (K, the magnitude terms and
                  how K was set: oracle/glue64.py; angles as a circular distance modulo pi, no row left out)
  selection       k_pyr_keys / k_pyr_topk / k_pyr_gather through pyramid.candidates on every key route (precomputed
                  keys, the four-in-flight vector loop, the plain loop for more than 16 classes): the selected rows equal
                  glue64.select_topk, scores within one f16 rounding of an f32 sigmoid of float64's
  epilogue        k_bias_act: bit-equal to glue64.bias_act_ref (IEEE additions only: fully determined)
  k_rbox_to_poly  within the centre bound of oracle.rbox_to_poly

The inputs and case tables are tests/glue_cases.py; tests/test_glue64_cpu.py holds the float32 oracle to the same bounds
on the same rows without a GPU.  S2A_GLUE_REPORT=<path> writes each kernel's worst error-to-bound ratio as JSON (the
committed run: profiles/glue_ratios.json).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import glue64 as G
import glue_cases as GC

pytestmark = pytest.mark.gpu

RATIOS = {}


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def note(kernel, ratio):
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("S2A_GLUE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"what": "worst |kernel - float64| / bound per kernel (tests/test_gpu_glue.py); bit-equal checks count 0",
                       "K": G.K, "worst_ratio": {k: round(v, 4) for k, v in sorted(RATIOS.items())}}, f, indent=1)
            f.write("\n")


def check_decode(kernel, got, ref, mag, where=None):
    ratio = G.decode_ratio(got, ref, mag)
    print(kernel, where, "worst error / bound per column:", np.round(ratio.max(0), 3))
    note(kernel, ratio.max())
    assert ratio.max() <= 1.0, (kernel, where, ratio.max(0), np.unravel_index(ratio.argmax(), ratio.shape))


# ---------------------------------------------------------------------------------------------- decode family
@pytest.mark.parametrize("n", GC.DECODE_SIZES)
def test_delta2bbox_vs_float64(n):
    """1, 255, 257 and 5000 rows (off a multiple of the 256-thread block, more than one block) at both clips; saturated
    dw / dh on both sides; 32 rows at, 1e-6 and 1e-3 from the norm_angle wrap"""
    from s2anet_amd.head import delta2bbox_rotated
    r, d = GC.decode_rows(n, seed=n)
    for clip in GC.DECODE_CLIPS:
        got = delta2bbox_rotated(cu(r), cu(d), clip).cpu().numpy()
        assert got.shape == (n, 5)
        ref, mag = G.decode64(r, d, clip)
        check_decode("k_delta2bbox", got, ref, mag, (n, clip))


@pytest.mark.parametrize("stride", GC.REFINE_STRIDES)
@pytest.mark.parametrize("shape", GC.REFINE_SHAPES)
def test_fam_refine_vs_float64(shape, stride):
    """grid anchors + decode, f32 and f16, NCHW and channels-last (the same f16-representable values for all four, so
    one float64 reference serves them); zero deltas must give the grid anchors back exactly"""
    from s2anet_amd.head import fam_refine_anchors
    B, H, W = shape
    pred = GC.refine_pred(shape, seed=stride)                            # [B,H,W,5]
    ref, mag = G.refine64(pred.transpose(0, 3, 1, 2), stride)
    nchw = cu(pred.transpose(0, 3, 1, 2))                                # contiguous NCHW
    for dtype in (torch.float32, torch.float16):
        for fmt in ("nchw", "nhwc"):
            t = nchw.to(dtype)
            if fmt == "nhwc":
                t = t.contiguous(memory_format=torch.channels_last)
            got = fam_refine_anchors(t, stride).cpu().numpy()
            assert got.shape == (B, H, W, 5)
            check_decode("k_fam_refine", got, ref, mag, (shape, stride, str(dtype), fmt))
            zero = fam_refine_anchors(torch.zeros_like(t), stride).cpu().numpy().astype(np.float64)
            assert np.array_equal(zero.reshape(B, H * W, 5), np.broadcast_to(G.grid_anchors64(H, W, stride), (B, H * W, 5)))


@pytest.mark.parametrize("pyr", [GC.PYRAMID5, GC.PYRAMID8], ids=["5levels", "8levels"])
def test_fam_refine_pyramid_vs_float64(pyr):
    """the packed kernel's level lookup (position, stride and side of every level) on ragged and on eight tiny levels,
    rows of 64 columns: against float64, not against the per-level kernel that shares decode_one with it"""
    from s2anet_amd import pyramid as P
    batch, sizes, strides = pyr
    layout = P.PyramidLayout(batch, sizes, strides)
    pred5 = GC.refine_pred((layout.pixels,), seed=len(sizes))
    pred = np.full((layout.pixels, GC.PYRAMID_ROW_STRIDE), np.nan, np.float16)     # columns >= 5 are never read
    pred[:, :5] = pred5
    got = P.fam_refine_anchors(layout, cu(pred), 4.0).cpu().numpy()
    ref, mag = G.refine64_pyramid(pred5, batch, sizes, strides)
    check_decode("k_fam_refine_pyramid", got, ref, mag, len(sizes))
    pred[:, :5] = 0
    zero = P.fam_refine_anchors(layout, cu(pred), 4.0).cpu().numpy().astype(np.float64)
    assert np.array_equal(zero, G.pyramid_anchors64(batch, sizes, strides))


@pytest.mark.parametrize("case", GC.ALIGN_CASES, ids=lambda c: "%dx%d_s%d_k%d" % c)
def test_align_offsets_vs_float64(case):
    """rotated anchors far off the grid; the channel order (2t = dy, 2t+1 = dx) is held by the bound itself"""
    from s2anet_amd.alignconv import align_offsets
    H, W, stride, ks = case
    a = GC.align_anchors(H, W, stride)
    got = align_offsets(cu(a), (H, W), stride, ks).cpu().numpy().astype(np.float64)
    ref, mag = G.align_offsets64(a, H, W, stride, ks)
    assert got.shape == ref.shape
    ratio = np.abs(got - ref) / (G.K["offset"] * G.U32 * mag)
    print("k_align_offsets", case, "worst error / bound:", round(ratio.max(), 3))
    note("k_align_offsets", ratio.max())
    assert ratio.max() <= 1.0, (case, np.unravel_index(ratio.argmax(), ratio.shape))


# ---------------------------------------------------------------------------------------------- candidate selection
CLIP = 16 / 1000


def _raw_candidates(layout, cls, reg, anc, C, k, bb, sc, sel):
    from s2anet_amd import _lib
    with torch.cuda.device(cls.device):
        return _lib.lib().s2a_pyramid_candidates(_lib.ptr(cls), _lib.ptr(reg), _lib.ptr(anc), layout.batch, ctypes.byref(layout.c),
                                                 int(C), int(k), float(CLIP), _lib.ptr(bb), _lib.ptr(sc), _lib.ptr(sel),
                                                 _lib.stream_ptr(cls.device))


def _canaries(B, n, C):
    return (torch.full((B, n, 5), float("nan"), device=dev()), torch.full((B, n, C), float("nan"), device=dev()),
            torch.full((B, n), -1, dtype=torch.int32, device=dev()))


def _segments(layout, sizes, k):
    out0, n = GC.out_slots(sizes, k)
    for l, (h, w) in enumerate(sizes):
        for b in range(layout.batch):
            yield l, b, layout.pix0[l] + b * h * w, h * w, out0[l], min(h * w, k)


@pytest.mark.parametrize("case", GC.CAND_CASES, ids=lambda c: c[0])
def test_candidates_vs_float64(case):
    """pyramid.candidates on the case table of tests/glue_cases.py (route of every case: glue_cases.topk_route), each with
    five kinds of keys: all distinct, a handful of values, all equal (the first k positions), all negative, and +-inf /
    f16 subnormals / 65504 (the sign branch of f16_key).  Per (image, level) the selected rows equal select_topk; the
    scores are f16 values within 2^-11 s + K 2^-24 s of sigmoid64 (one f16 rounding on top of an f32 sigmoid); the
    boxes are within the decode bound; two calls into NaN-filled outputs write every element with the same bits.
    No -0.0 / +0.0 mix in the keys: the kernel orders them, a float comparison does not, and the reference's topk
    defines no order among equal scores."""
    from s2anet_amd import pyramid as P
    name, B, C, sizes, k = case
    layout = P.PyramidLayout(B, sizes, tuple(8 * 2 ** i for i in range(len(sizes))))
    route = GC.topk_route(B, sizes, C, k)
    reg, anc = GC.cand_reg_anchors(layout.pixels, seed=len(name))
    reg_d, anc_d = cu(reg), cu(anc)
    n = GC.out_slots(sizes, k)[1]
    for kind in GC.KEY_KINDS:
        cls = GC.cand_logits(B, C, sizes, kind, seed=len(name))
        cls_d = cu(cls)
        out = P.candidates(layout, cls_d, reg_d, anc_d, C, k, CLIP)
        assert out is not None
        bb, sc, sel = (t.cpu().numpy() for t in out)
        assert bb.shape == (B, n, 5) and sc.shape == (B, n, C) and sel.shape == (B, n)
        want = np.empty((B, n), np.int64)
        for l, b, r0, hw, o0, m in _segments(layout, sizes, k):
            keys = cls[r0:r0 + hw, :C].astype(np.float64).max(1)
            want[b, o0:o0 + m] = G.select_topk(keys, k) + r0
            assert np.array_equal(sel[b, o0:o0 + m], want[b, o0:o0 + m]), (name, route, kind, l, b)
        assert np.array_equal(sc.astype(np.float16).astype(np.float32), sc), "scores are f16 values"
        s64 = G.sigmoid64(cls[want.reshape(-1), :C]).reshape(B, n, C)
        bound = G.U16 * s64 + G.K["sigmoid"] * G.U32 * s64
        err = np.abs(sc.astype(np.float64) - s64)
        assert (err <= bound).all(), (name, kind, (err - bound).max())
        note("k_pyr_gather (scores)", (err[bound > 0] / bound[bound > 0]).max())
        ref, mag = G.decode64(anc[want.reshape(-1)], reg[want.reshape(-1), :5], CLIP)
        check_decode("k_pyr_gather (boxes)", bb, ref, mag, (name, kind))
        # twice into NaN / -1 filled outputs
        twice = []
        for rep in range(2):
            o = _canaries(B, n, C)
            assert _raw_candidates(layout, cls_d, reg_d, anc_d, C, k, *o) == 0
            twice.append([t.cpu().numpy() for t in o])
        for first, second, lib_out in zip(twice[0], twice[1], (bb, sc, sel)):
            assert not np.isnan(first).any() and (first.dtype != np.int32 or (first >= 0).all()), (name, kind, "an element was not written")
            assert first.tobytes() == second.tobytes() == lib_out.tobytes(), (name, kind)
    note("k_pyr_topk (rows differing from select_topk)", 0.0)


@pytest.mark.parametrize("case", [GC.CAND_CASES[1], GC.CAND_CASES[3], GC.CAND_CASES[5]], ids=lambda c: c[0])
def test_candidates_with_nan_logits_keep_their_structure(case):
    """16 NaN logits planted (one route each).  Where a NaN ranks is not pinned by the reference (its sigmoid is NaN and
    torch.topk's treatment of NaN is its own), so only the structure is asserted: exactly min(HW, k) distinct,
    ascending, in-range rows per (image, level)."""
    from s2anet_amd import pyramid as P
    name, B, C, sizes, k = case
    layout = P.PyramidLayout(B, sizes, tuple(8 * 2 ** i for i in range(len(sizes))))
    cls = GC.cand_logits(B, C, sizes, "distinct", seed=3)
    rng = np.random.default_rng(8)
    rows = rng.choice(layout.pixels, 16, replace=False)
    cls[rows, rng.integers(0, C, 16)] = np.nan
    cls[rows[:4], :C] = np.nan                                             # four rows wholly NaN
    reg, anc = GC.cand_reg_anchors(layout.pixels)
    out = P.candidates(layout, cu(cls), cu(reg), cu(anc), C, k, CLIP)
    sel = out[2].cpu().numpy()
    for l, b, r0, hw, o0, m in _segments(layout, sizes, k):
        got = sel[b, o0:o0 + m]
        assert got.shape == (m,) and (np.diff(got) > 0).all() and got[0] >= r0 and got[-1] < r0 + hw, (name, l, b)


def test_candidates_refuse_a_level_past_the_lds_cap():
    """24 577 positions with k = 2000: pyramid.candidates answers None, and the C entry returns its argument error
    without touching the outputs"""
    from s2anet_amd import _lib, pyramid as P
    layout = P.PyramidLayout(1, [(1, GC.TOPK_MAX_N + 1)], (8,))
    cls = torch.zeros((layout.pixels, 64), dtype=torch.float16, device=dev())
    reg = torch.zeros_like(cls)
    anc = torch.ones((layout.pixels, 5), device=dev())
    assert P.candidates(layout, cls, reg, anc, 15, 2000) is None
    o = _canaries(1, 2000, 15)
    rc = _raw_candidates(layout, cls, reg, anc, 15, 2000, *o)
    assert rc != 0
    with pytest.raises(RuntimeError, match="24576"):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert torch.isnan(o[0]).all() and torch.isnan(o[1]).all() and (o[2] == -1).all()
    # at the cap itself the level is taken (test_candidates_vs_float64[cap_keys])
    assert P.candidates(P.PyramidLayout(1, [(1, GC.TOPK_MAX_N)], (8,)), cls[:-1], reg[:-1], anc[:-1], 15, 2000) is not None


# ---------------------------------------------------------------------------------------------- epilogue
def _same_bits(got, ref):
    """equal bit for bit, a NaN matching any NaN"""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    gn, rn = np.isnan(got), np.isnan(ref)
    u = np.uint16 if got.dtype == np.float16 else np.uint32
    return np.array_equal(gn, rn) and np.array_equal(got.view(u)[~gn], ref.view(u)[~rn])


def _epilogue_inputs(shape, np_dtype, plant, seed):
    """NHWC arrays y, r [B,H,W,C] and bias [C] in the storage type; plant: +inf, -inf and NaN in y (channels 2-4 of the
    first position), NaN and +inf in r (channels 2, 3 of the last position), NaN and +inf in the bias (channels 1, C-1)"""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((B, H, W, C), dtype=np.float32) * 2).astype(np_dtype)
    r = (rng.standard_normal((B, H, W, C), dtype=np.float32) * 2).astype(np_dtype)
    bias = rng.standard_normal(C, dtype=np.float32).astype(np_dtype)
    if plant:
        y[0, 0, 0, 2:5] = (np.inf, -np.inf, np.nan)
        r[-1, -1, -1, 2:4] = (np.nan, np.inf)
        y[-1, -1, -1, 3] = -np.inf                                       # -inf + inf residual: NaN
        bias[1], bias[C - 1] = np.nan, np.inf
    return y, r, bias


def _run_epilogue(shape, np_dtype, configs, plant, seed=0):
    from s2anet_amd.fused import _bias_act_raw, bias_act_
    y, r, bias = _epilogue_inputs(shape, np_dtype, plant, seed)
    nchw = (0, 3, 1, 2)
    y_d, r_d, b_d = cu(y).permute(*nchw), cu(r).permute(*nchw), cu(bias)
    assert y_d.is_contiguous(memory_format=torch.channels_last) and y_d.shape == tuple(shape)
    for residual, relu, into in configs:
        ref = G.bias_act_ref(y.transpose(nchw), bias, r.transpose(nchw) if residual else None, relu, np_dtype).transpose(0, 2, 3, 1)
        res = r_d if residual else None
        with torch.no_grad():
            if into:
                src = y_d.clone(memory_format=torch.preserve_format)
                out = torch.full_like(src, 7.0, memory_format=torch.preserve_format)
                ret = _bias_act_raw(src, b_d, res, relu, out=out)
                assert ret is out and _same_bits(src.permute(0, 2, 3, 1).cpu().numpy(), y), "out=: y must stay as it was"
            else:
                out = y_d.clone(memory_format=torch.preserve_format)
                assert out.is_contiguous(memory_format=torch.channels_last)
                ret = bias_act_(out, b_d, res, relu)
                assert ret is out
        got = out.permute(0, 2, 3, 1).cpu().numpy()
        assert _same_bits(got, ref), (shape, np_dtype.__name__, residual, relu, into, int((got != ref).sum()))
        if residual:
            assert _same_bits(r_d.permute(0, 2, 3, 1).cpu().numpy(), r), "the residual is read only"
        if plant:                                                        # the documented classes, spelled out
            C = shape[1]
            if relu:
                assert not np.isnan(got).any() and (got >= 0).all()
                assert got[0, 0, 0, 4] == 0 and got[0, 0, 0, 3] == 0 and np.isposinf(got[0, 0, 0, 2])   # NaN -> 0, -inf -> 0
                assert (got[..., 1] == 0).all()                          # NaN bias: the whole channel is 0
            else:
                assert np.isnan(got[0, 0, 0, 4]) and np.isneginf(got[0, 0, 0, 3]) and np.isposinf(got[0, 0, 0, 2])
                assert np.isnan(got[..., 1]).all() and np.isposinf(got[..., C - 1]).all()
                if residual:
                    assert np.isnan(got[-1, -1, -1, 2]) and np.isnan(got[-1, -1, -1, 3])
    note("k_bias_act (elements differing from bias_act_ref)", 0.0)


ALL_CONFIGS = [(res, relu, into) for res in (False, True) for relu in (False, True) for into in (False, True)]


@pytest.mark.parametrize("dtype", ["f16", "f32"])
@pytest.mark.parametrize("shape", GC.EPILOGUE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bias_act_bit_equal(shape, dtype):
    """with and without residual and ReLU, in place (bias_act_) and into another buffer (_bias_act_raw(out=)); channel
    vector counts that are hoisted (a power of two <= 256), not hoisted (3, 40) and above 256; non-finite values in y, the
    bias and the residual from 24 channels on"""
    np_dtype = np.float16 if dtype == "f16" else np.float32
    if shape == (1, 8, 1, 1) and dtype == "f32":
        shape = (1, 4, 1, 1)
    _run_epilogue(shape, np_dtype, ALL_CONFIGS, plant=False)
    if shape[1] >= 24:
        _run_epilogue(shape, np_dtype, ALL_CONFIGS, plant=True, seed=1)


def test_bias_act_bit_equal_past_the_grid_cap():
    """f16 1x64x524x524: 2 196 608 vectors on the capped grid of 2048 workgroups (524 288 threads): one full trip of the
    four-stream loop for every thread, then the tail loop for the first 99 456"""
    _run_epilogue(GC.EPILOGUE_LARGE, np.float16, [(True, True, False), (False, False, True), (True, False, True), (False, True, False)],
                  plant=True)


def test_bias_act_bit_equal_in_the_second_trip():
    """f16 1x64x680x680: 3 699 200 vectors > 7 x 524 288, so the first 29 184 threads make a second trip of the four-stream
    loop while the others finish in the tail loop (the 524 x 524 case stops after one trip)"""
    B, C, H, W = GC.EPILOGUE_SECOND_TRIP
    assert B * C * H * W // 8 > 7 * 2048 * 256
    _run_epilogue(GC.EPILOGUE_SECOND_TRIP, np.float16, [(True, True, False), (False, False, True)], plant=True)


# ---------------------------------------------------------------------------------------------- rbox_to_poly
def _poly_rows(n, seed):
    rng = np.random.default_rng(seed)
    b = np.empty((n, 6), np.float32)
    b[:, 0:2] = rng.uniform(0, 1024, (n, 2))
    b[:, 2:4] = rng.uniform(4, 512, (n, 2))
    b[:, 4] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, n)
    b[:, 5] = np.nan                                                     # the score column of a detection: never read
    h = np.float32(np.pi / 2)
    special = [0.0, -np.pi / 4, h, h + np.float32(1e-3), h - np.float32(1e-3), 3 * np.pi / 4 - 1e-6]
    m = min(n, len(special)) if n > 1 else 0
    b[:m, 4] = np.asarray(special[:m], np.float32)
    return b


@pytest.mark.parametrize("n", [1, 257, 2006])
def test_rbox_to_poly_vs_oracle(n):
    """2 000 random rows + the angles 0, -pi/4, f32(pi/2), f32(pi/2) +- 1e-3, 3pi/4 - 1e-6; rows of 5 and of 6 columns (a
    [:, :5] view of detections); every coordinate within K 2^-24 (|c| + |w| + |h|), c the centre coordinate it belongs to
    (x for the x of a vertex, y for its y), same vertex order; rows within 1e-4 rad of the 90 degree branch are compared
    as an unordered vertex set (at most 1 % of the rows).  The comparator is the float32 oracle (cv2.boxPoints restated):
    both sides carry at most the measured float32 error, K is twice that."""
    from s2anet_amd.formats import rbox_to_poly
    b6 = _poly_rows(n, seed=n)
    ref = oracle.rbox_to_poly(b6[:, :5]).astype(np.float64)
    c64 = b6.astype(np.float64)
    bound = np.empty((n, 8))
    bound[:, 0::2] = (G.K["centre"] * G.U32 * (np.abs(c64[:, 0]) + c64[:, 2] + c64[:, 3]))[:, None]
    bound[:, 1::2] = (G.K["centre"] * G.U32 * (np.abs(c64[:, 1]) + c64[:, 2] + c64[:, 3]))[:, None]
    near = np.abs(b6[:, 4].astype(np.float64) - np.pi / 2) < 1e-4
    assert near.mean() <= 0.01 or n < 100
    view = cu(b6)[:, :5]
    assert view.stride(0) == 6
    for boxes in (cu(b6[:, :5].copy()), view):
        got = rbox_to_poly(boxes).cpu().numpy().astype(np.float64)
        assert got.shape == (n, 8)
        ratio = np.abs(got - ref) / bound
        for i in np.nonzero(near)[0]:                                    # any rotation of the vertex list
            ratio[i] = min((np.abs(np.roll(got[i], 2 * s) - ref[i]) / bound[i] for s in range(4)), key=np.max)
        note("k_rbox_to_poly", ratio.max())
        assert ratio.max() <= 1.0, (n, np.unravel_index(ratio.argmax(), ratio.shape), ratio.max())
