"""GPU: every own-kernel launch of the forward that bench.py times, at the benchmark's own shapes, against float64.

Two geometries run S2ANet.detect() with the Python entry points that launch own kernels wrapped (Recorder below):
  (A) bench.py's input: build_synthetic_detector(seed=1234), batch 8 of 1024^2 u8 chips drawn as bench.py draws them,
      odm_cls_head scaled as calibrate_cls_bias does (logit std 1.5); default switches;
  (B) ragged maps: batch 2 of 800 x 1344 with S2A_OWN_CONV_ALWAYS=1 (layer-4 grids and P6 / P7 on k_conv_f16 too).
Each wrapper calls the original and checks that launch at once (memory stays flat):
  1. elementwise |got - y64| <= tau * S + 2^-25, S the sum of |terms| behind the entry (oracle/conv64.py), tau below;
  2. relative L2 error <= 2 u16 (conv) / L2_DCN (AlignConv f16) / L2_F32 (AlignConv f32): errors spread too thin
     for the elementwise bound;
  3. a second launch into NaN-filled outputs is bitwise equal (every output written, deterministically);
  4. the tile-shape switches forced both ways give the same bits where the code claims it (S2A_CONV_PH, _PH_NARROW,
     S2A_CONV3_HALF, S2A_CONV1_HALF, S2A_DCN_HALF_TAIL), the elementwise bound for S2A_CONV_OG;
  5. real signal: > 20 % nonzero outputs behind a ReLU, no reference value beyond the f16 range.
Fused launches are checked stage by stage from the f16 values the kernel rounded to at that stage.  The C-ABI symbols
are wrapped too: every compute call must belong to a checked launch or to the allow-list.  Planted defects show that
the bounds bite at these magnitudes.  Set S2A_FWD_SHAPES_REPORT=<path> to write every launch's numbers as JSON."""
import contextlib
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16, U32 = 2.0 ** -11, 2.0 ** -24
TINY = 2.0 ** -25                 # half an f16 subnormal step: the absolute floor of an underflowed result
F16_MAX = 65504.0
L2_CONV = 2 * U16
# AlignConv f16: six roundings behind each product (bilinear weight to f16, one product and three FMAs of the packed-half
# blend, the f16 result), each at most u16 relative and independent, RMS about u16 / sqrt(3) each: sqrt(6 / 3) u16 = 1.4
# u16 expected; the bound leaves a factor of about 3
L2_DCN = 4 * U16
# coordinate slack per axis between align_offsets (the points of the reference) and the kernel's anchor_offset: the same
# operations in the same order, but another kernel -- the compiler may contract xr / yr into FMAs differently, and its
# cosf / sinf may differ by an ulp: a few f32 ulps of coordinates below 256 (ulp 2^-16 .. 2^-15).  2^-12 = 8 ulps or more.
DP = 2.0 ** -12
# AlignConv f32: the output is a sum of K = 2304 products formed in f32.  Each addition rounds by at most u32 of its
# partial sum, with a random sign (RMS u32 / sqrt(3)); the partial sums grow like sqrt(k) times the RMS term, so the
# accumulated error is about u32 / sqrt(3) * sqrt(K / 2) = 20 u32 of |y| (= sqrt(K) RMS terms) for a sequential order
# (less for the MFMA's partial trees).  The blend's four roundings and the x3 kernel's dropped cross terms (< 3 u32 per
# product, independent) add about 2 u32.  Expected <= 22 u32; the bound leaves a factor of about 3.
L2_F32 = 64 * U32
REPORT = []


def tau(kind, K):
    """elementwise bound / S, one unit roundoff per rounding a term of the sum sees (u = u16 = 2^-11, v = u32 = 2^-24,
    K products per output):
    conv      exact f16 products summed in f32 (K v), + bias in f32, ONE f16 rounding, ReLU on the rounded value
                                                                                   -> u + (K + 17) v
    conv_res  rnd16(rnd16(acc + b) + r): the residual / up-2 coarse epilogue rounds twice (k_conv_f16: its residual pass
              and its fused tail)                                                     -> 2u + (K + 17) v
    stem      as conv (K = 147; the zero-padded K steps add nothing), ReLU and the max-pool exact, through the pooled S
                                                                                   -> u + (K + 17) v
    dcn16     f16 bilinear weights (u), one product and three FMAs in packed half (4u, blend_pk), exact f16 products
              summed in f32 (K v), f16 result (u)                                  -> 6u + (K + 16) v
    dcn32_x3  f32 blend (4 roundings), three bf16 planes per operand (dropped cross terms), f32 sums -> (K + 24) v
    dcn32_mfma32  f32 blend (4 roundings), f32 products and sums                  -> (K + 20) v
    AlignConv bounds add 2 DP S_corner for the coordinates (oracle/conv64.py:align64)."""
    return {"conv": U16 + (K + 17) * U32, "conv_res": 2 * U16 + (K + 17) * U32, "stem": U16 + (K + 17) * U32,
            "dcn16": 6 * U16 + (K + 16) * U32, "dcn32_x3": (K + 24) * U32, "dcn32_mfma32": (K + 20) * U32}[kind]


def _report_write():
    path = os.environ.get("S2A_FWD_SHAPES_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)


class Meter:
    """one launch (or stage) against its reference, accumulated over levels.  Every test is written so that a NaN (in
    the output or in the reference) fails it on its own: NaN compares false, and the ratios turn NaN into inf."""

    def __init__(self, kind, K, l2_bound=L2_CONV):
        self.kind, self.K, self.t, self.l2_bound = kind, K, tau(kind, K), l2_bound
        self.ratio, self.ratio_raw, self.e2, self.y2, self.bad, self.nz, self.n, self.ymax = 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0.0

    @staticmethod
    def _max(t):
        return torch.nan_to_num(t, nan=math.inf).max().item()

    def add(self, got, y, S, extra=None):
        err = (got.double() - y).abs()
        slack = TINY if extra is None else extra + TINY
        self.bad += int((~(err <= self.t * S + slack)).sum())
        self.ratio = max(self.ratio, self._max((err - slack).clamp_min(0) / S.clamp_min(1e-300)))
        self.ratio_raw = max(self.ratio_raw, self._max((err - TINY).clamp_min(0) / S.clamp_min(1e-300)))
        self.e2 += err.square().sum().item()
        self.y2 += y.square().sum().item()
        self.nz += int((got != 0).sum())
        self.n += got.numel()
        self.ymax = max(self.ymax, self._max(y.abs()))

    def l2(self):
        if not (math.isfinite(self.e2) and math.isfinite(self.y2)):
            return math.inf
        return math.sqrt(self.e2) / max(math.sqrt(self.y2), 1e-300)

    def ok_elem(self):
        return self.bad == 0

    def ok_l2(self):
        return self.l2() <= self.l2_bound

    def rejected_by(self):
        """the checks that reject this comparison (a planted defect must be rejected by at least one)"""
        return [k for k, ok in (("elementwise", self.ok_elem()), ("l2", self.ok_l2())) if not ok]

    def summary(self):
        return dict(kind=self.kind, K=self.K, tau=self.t, max_err_over_S=self.ratio,
                    max_err_over_S_without_coordinate_term=self.ratio_raw, l2=self.l2(), l2_bound=self.l2_bound,
                    entries_over_bound=self.bad, nonzero=self.nz / max(self.n, 1), ref_absmax=self.ymax)


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def nan_like(t):
    return torch.full_like(t, float("nan"))


# C-ABI calls that are not a checked launch: weight packing, the ARF expansion of the ORConv filter, fam_refine,
# candidates, NMS
ALLOW = {"s2a_conv_pack_weight_f16", "s2a_stem_pack_weight_f16", "s2a_stem_packed_elems", "s2a_dcn_pack_weight",
         "s2a_dcn_packed_elems", "s2a_arf_forward", "s2a_fam_refine_anchors_pyramid", "s2a_pyramid_candidates_count",
         "s2a_pyramid_candidates", "s2a_multiclass_candidates_workspace_bytes", "s2a_multiclass_candidates",
         "s2a_nms_rotated_workspace_bytes", "s2a_nms_rotated_segmented_dets", "s2a_last_error"}
ALLOW_LIBRARY_CONV = {"s2a_bias_act_nhwc_to"}          # (A) only: the epilogue behind FPN's two library convolutions


class _LibProxy:
    def __init__(self, real, rec):
        self._real, self._rec = real, rec

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("s2a_"):
            return fn
        rec = self._rec

        def call(*a):
            rec.note(name)
            return fn(*a)
        return call


class Recorder:
    """wraps the own-kernel entry points and the C-ABI for the duration of one forward; checks every launch"""

    def __init__(self, model, tag, allow_library_conv, imgs):
        from s2anet_amd.fused import FusedConv2d, PackedWeightCache
        self.model, self.tag, self.imgs = model, tag, imgs
        self.allow = ALLOW | (ALLOW_LIBRARY_CONV if allow_library_conv else set())
        self.depth, self.attributed, self.allowed, self.unattributed = 0, {}, {}, []
        self.failures, self.entries, self.keep, self.counts = [], [], {}, {}
        self.wmap = {}
        for n, m in model.named_modules():
            if isinstance(m, FusedConv2d) and tuple(m.kernel_size) in ((1, 1), (3, 3)) and \
                    (m.in_channels % 64 == 0 or m.in_channels == 32):
                pw, _, _ = m.packed_args()
                self.wmap[pw.data_ptr()] = (n, m.weight, m.bias)
        oc = model.head.or_conv
        wa = oc.rotate_arf()
        if not hasattr(oc, "_packed"):
            oc._packed = PackedWeightCache()
        self.wmap[oc._packed.get(wa).data_ptr()] = ("head.or_conv", wa, oc.bias)
        self.align_w = model.head.align_conv.packed_weight(torch.float16)

    # ------------------------------------------------------------------ plumbing
    def note(self, name):
        if self.depth > 0:
            self.attributed[name] = self.attributed.get(name, 0) + 1
        elif name in self.allow:
            self.allowed[name] = self.allowed.get(name, 0) + 1
        else:
            self.unattributed.append(name)

    def __enter__(self):
        from s2anet_amd import _lib, detector, fused, pyramid
        self._lib_mod = _lib
        self._real = _lib.lib()
        _lib._lib = _LibProxy(self._real, self)
        self.orig = {}
        targets = [(fused, "stem_u8", self.check_stem), (fused, "conv_f16", self.check_conv),
                   (fused, "conv1x1_add_up2", self.check_up2), (detector, "bottleneck_tail", self.check_tail),
                   (pyramid, "conv3x3", self.check_pyr_conv), (pyramid, "conv3x3_head", self.check_head),
                   (pyramid, "orconv_pool", self.check_orpool), (pyramid, "align_conv", self.check_align),
                   (pyramid, "conv1x1", self.check_pyr_conv1x1)]
        self._patched = []
        for mod, name, chk in targets:
            orig = getattr(mod, name)
            self.orig[name] = orig
            self._patched.append((mod, name, orig))
            setattr(mod, name, self._wrap(name, orig, chk))
        return self

    def __exit__(self, *exc):
        for mod, name, orig in self._patched:
            setattr(mod, name, orig)
        self._lib_mod._lib = self._real
        return False

    def _wrap(self, name, orig, chk):
        def f(*args, **kw):
            self.depth += 1
            try:
                got = orig(*args, **kw)
                self.counts[name] = self.counts.get(name, 0) + 1
                chk(got, *args, **kw)
            finally:
                self.depth -= 1
            return got
        return f

    def weights(self, packed):
        key = packed.data_ptr()
        if key not in self.wmap:
            raise AssertionError("%s: a launch with a packed filter that belongs to no module" % self.tag)
        return self.wmap[key]

    def finish(self, label, meters, relu, extra=None):
        """record one launch: meters = {stage: Meter}; extra = more report fields (bit_* must be True)"""
        e = dict(geometry=self.tag, launch=label, stages={k: m.summary() for k, m in meters.items()}, **(extra or {}))
        ok = True
        for k, m in meters.items():
            if not m.ok_elem():
                self.failures.append("%s %s/%s: %d entries over tau*S (max err/S %.3g, tau %.3g)" %
                                     (self.tag, label, k, m.bad, m.ratio, m.t))
                ok = False
            if not m.ok_l2():
                self.failures.append("%s %s/%s: relative L2 %.3g > %.3g" % (self.tag, label, k, m.l2(), m.l2_bound))
                ok = False
            if m.ymax > F16_MAX:
                self.failures.append("%s %s/%s: reference beyond the f16 range (%.4g)" % (self.tag, label, k, m.ymax))
                ok = False
            if relu.get(k, False) and m.nz <= 0.2 * m.n:
                self.failures.append("%s %s/%s: only %.1f %% nonzero behind a ReLU" % (self.tag, label, k, 100.0 * m.nz / m.n))
                ok = False
        for k, v in (extra or {}).items():
            if k.startswith("bit_") and v is not True:
                self.failures.append("%s %s: %s = %s" % (self.tag, label, k, v))
                ok = False
        e["ok"] = ok
        self.entries.append(e)
        REPORT.append(e)
        _report_write()

    def variants(self, run, ref, switches):
        """run() under each (var, value): bitwise equal to ref -> {"var=value": bool}"""
        res = {}
        for var, vals in switches:
            for v in vals:
                with env(**{var: v}):
                    got = run()
                if isinstance(ref, tuple):
                    res["%s=%s" % (var, v)] = all(torch.equal(a, b) for a, b in zip(got, ref))
                else:
                    res["%s=%s" % (var, v)] = torch.equal(got, ref)
        return res

    # ------------------------------------------------------------------ per-entry-point checks
    def check_stem(self, got, imgs, packed_weight, bias, divisor=255.0):
        from oracle.conv64 import stem64
        from s2anet_amd import _lib
        conv = self.model.backbone.backbone[0][0]
        assert imgs.data_ptr() == self.imgs.data_ptr()
        y, S = stem64(imgs, conv.weight, conv.bias, divisor)
        m = Meter("stem", 147)
        m.add(got, y, S)
        B, _, H, W = imgs.shape
        again = nan_like(got)
        _lib.check(_lib.lib().s2a_stem_u8_f16(_lib.ptr(imgs), _lib.ptr(packed_weight), _lib.ptr(bias), _lib.ptr(again),
                                              B, H, W, float(divisor), _lib.stream_ptr(imgs.device)))
        Hp, Wp = got.shape[2:]
        tiles = B * ((Wp + 7) // 8) * ((Hp + 7) // 8)
        self.keep["stem"] = dict(out=got, y=y, S=S)
        self.finish("stem", {"out": m}, {"out": True},
                    dict(shape=[B, 3, H, W, 64], tiles=tiles, tiles_per_wg=-(-tiles // min(tiles, 512)),
                         bit_nan_rerun=torch.equal(again, got)))

    def check_conv(self, got, x, packed_weight, bias, out_channels, ksize, stride=1, relu=False, residual=None, **kw):
        from oracle.conv64 import conv64
        name, w, b = self.weights(packed_weight)
        B, C, H, W = x.shape
        O = w.shape[0]
        y, S = conv64(x, w, b, stride, ksize, residual=residual, relu=relu)
        m = Meter("conv_res" if residual is not None else "conv", w.shape[1] * ksize * ksize)
        m.add(got, y, S)
        phys = max(64, O)
        Ho, Wo = got.shape[2:]

        def run():
            buf = torch.empty((B, phys, Ho, Wo), dtype=torch.float16, device=x.device,
                              memory_format=torch.channels_last).fill_(float("nan"))
            return self.orig["conv_f16"](x, packed_weight, bias, out_channels, ksize, stride, relu, residual, out=buf)
        again = run()
        sw = []
        if ksize == 3 and stride == 1:
            sw = [("S2A_CONV_PH_NARROW", ("1", "2")), ("S2A_CONV_PH", ("1", "2")), ("S2A_CONV3_HALF", ("0", "1"))]
        elif ksize == 1:
            sw = [("S2A_CONV1_HALF", ("0", "1"))]
        var = self.variants(run, got, sw)
        if name == "backbone.backbone.3.1.conv2":
            self.keep["l3c2"] = dict(x=x, w=w, out=got, y=y, S=S, m=m)
        if name == "backbone.backbone.4.1.conv1":
            self.keep["l4c1"] = dict(x=x, w=w, b=b, out=got, relu=relu)
        if ksize == 3 and stride == 1 and Wo % 16 != 0 and Wo > 16 and "ragged" not in self.keep:
            self.keep["ragged"] = dict(out=got, y=y, S=S, m=m, name=name)
        self.finish("conv_f16:%s" % name, {"out": m}, {"out": relu},
                    dict(shape=[B, C, H, W, O], ksize=ksize, stride=stride, residual=residual is not None,
                         bit_nan_rerun=torch.equal(again, got), variants=var, **{"bit_" + k: v for k, v in var.items()}))

    def check_up2(self, got, x, packed_weight, bias, coarse, out_channels):
        from oracle.conv64 import conv64
        from s2anet_amd import _lib
        name, w, b = self.weights(packed_weight)
        B, C, H, W = x.shape
        y, S = conv64(x, w, b, 1, 1, residual=coarse, residual_up2=True)
        m = Meter("conv_res", C)
        m.add(got, y, S)
        again = nan_like(got)
        _lib.check(_lib.lib().s2a_conv1x1_add_up2_f16(_lib.ptr(x), _lib.ptr(packed_weight), _lib.ptr(bias), _lib.ptr(coarse),
                                                      _lib.ptr(again), B, C, H, W, out_channels, _lib.stream_ptr(x.device)))
        if "up2" not in self.keep:
            self.keep["up2"] = dict(coarse=coarse, out=got, y=y, S=S, m=m)
        self.finish("conv1x1_add_up2:%s" % name, {"out": m}, {},
                    dict(shape=[B, C, H, W, out_channels], bit_nan_rerun=torch.equal(again, got)))

    def check_tail(self, res, x, conv2, conv3, residual=None, chain=None):
        """s2a_conv3x3_tail1x1_f16 stage by stage: the 64-map intermediate = the separate conv_f16(3x3, ReLU) launch
        (the header claims bit-identity with the two stand-alone launches: asserted), the tail against conv64(1x1) of it
        plus the residual, the chained conv1 against conv64 of the tail output"""
        from oracle.conv64 import conv64
        from s2anet_amd import _lib
        out, nxt = (res, None) if chain is None else res
        B, C, H, W = x.shape
        w2, b2, _ = conv2.packed_args()
        w3, b3, _ = conv3.packed_args()
        conv_f16 = self.orig["conv_f16"]
        mid = conv_f16(x, w2, b2, 64, 3, 1, True)
        meters = {}
        y, S = conv64(x, conv2.weight, conv2.bias, 1, 3, relu=True)
        meters["mid"] = Meter("conv", 64 * 9)
        meters["mid"].add(mid, y, S)
        del y, S
        two = conv_f16(mid, w3, b3, 256, 1, 1, True, residual)
        y, S = conv64(mid, conv3.weight, conv3.bias, 1, 1, residual=residual, relu=True)
        meters["tail"] = Meter("conv_res" if residual is not None else "conv", 64)
        meters["tail"].add(out, y, S)
        del y, S
        extra = dict(shape=[B, C, H, W, 256], chain=0 if chain is None else chain.out_channels,
                     bit_tail_equals_two_launches=torch.equal(out, two))
        wc = bc = None
        if chain is not None:
            wc, bc, _ = chain.packed_args()
            y, S = conv64(out, chain.weight, chain.bias, 1, 1, relu=True)
            meters["chain"] = Meter("conv", 256)
            meters["chain"].add(nxt, y, S)
            del y, S
            extra["bit_chain_equals_separate_conv1"] = torch.equal(nxt, conv_f16(out, wc, bc, chain.out_channels, 1, 1, True))

        def run():
            o = nan_like(out)
            n = None if chain is None else nan_like(nxt)
            _lib.check(_lib.lib().s2a_conv3x3_tail1x1_f16(
                _lib.ptr(x), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(w3), _lib.ptr(b3), _lib.ptr(residual), _lib.ptr(o),
                _lib.ptr(wc), _lib.ptr(bc), _lib.ptr(n), 0 if chain is None else chain.out_channels, B, 64, 64, 256, H, W,
                _lib.stream_ptr(x.device)))
            return o if chain is None else (o, n)
        ref = out if chain is None else (out, nxt)
        again = run()
        extra["bit_nan_rerun"] = (torch.equal(again, out) if chain is None else
                                  torch.equal(again[0], out) and torch.equal(again[1], nxt))
        var = self.variants(run, ref, [("S2A_CONV_PH_NARROW", ("1", "2"))])
        extra.update(variants=var, **{"bit_" + k: v for k, v in var.items()})
        names = {id(m): n for n, m in self.model.named_modules()}
        self.finish("bottleneck_tail:%s" % names.get(id(conv2), "?"), meters, {k: True for k in meters}, extra)

    def check_pyr_conv(self, got, layout, x, packed_w, bias, out_channels, relu, residual=None, out=None):
        from oracle.conv64 import conv64
        assert residual is None
        name, w, b = self.weights(packed_w)
        O = w.shape[0]
        orig = self.orig["conv3x3"]

        def run():
            return orig(layout, x, packed_w, bias, out_channels, relu, out=nan_like(got))
        again = run()
        var = self.variants(run, got, [("S2A_CONV_PH", ("1", "2"))])
        og = {}
        for v in ("1", "2"):
            with env(S2A_CONV_OG=v):
                og[v] = run()
        meters = {"out": Meter("conv", x.shape[1] * 9)}
        for v in og:
            meters["S2A_CONV_OG=" + v] = Meter("conv", x.shape[1] * 9)
        for l in range(len(layout.sizes)):
            y, S = conv64(layout.level(x, l), w, b, 1, 3, relu=relu)
            meters["out"].add(layout.level(got, l, O), y, S)
            for v, g in og.items():
                meters["S2A_CONV_OG=" + v].add(layout.level(g, l, O), y, S)
            del y, S
        self.finish("pyramid.conv3x3:%s" % name, meters, {"out": relu},
                    dict(shape=[layout.batch, x.shape[1], layout.sizes, O], bit_nan_rerun=torch.equal(again, got),
                         variants=var, **{"bit_" + k: v for k, v in var.items()}))

    def check_pyr_conv1x1(self, got, x, packed_w, bias, out_channels, relu, residual=None):
        raise AssertionError("pyramid.conv1x1 ran: the fused tower + head launch was expected (no check written for it)")

    def check_head(self, head_out, layout, x, packed_w, bias, out_channels, head_w, head_b, relu=True, keep_tower=False):
        """tower + 1x1 head in one launch: the tower (keep_tower) bit-identical to pyramid.conv3x3 and within its bound,
        the head (columns 0..31 written) against conv64(1x1) of the f16 tower"""
        from oracle.conv64 import conv64
        from s2anet_amd import _lib
        assert not keep_tower
        name, w, b = self.weights(packed_w)
        hname, hw, hb = self.weights(head_w)
        C = x.shape[1]

        def run():
            h, t = nan_like(head_out), layout.new(out_channels, x.device).fill_(float("nan"))
            _lib.check(_lib.lib().s2a_conv3x3_head_pyramid_f16(
                _lib.ptr(x), _lib.ptr(packed_w), _lib.ptr(bias), _lib.ptr(t), _lib.ptr(head_w), _lib.ptr(head_b),
                _lib.ptr(h), layout.batch, C, out_channels, int(bool(relu)), ctypes.byref(layout.c),
                _lib.stream_ptr(x.device)))
            return h[:, :32], t
        h2, tower = run()
        tower_sep = self.orig["conv3x3"](layout, x, packed_w, bias, out_channels, relu)
        # S2A_CONV_OG does not apply to the fused head (it needs OG = 4, conv3x3_pyramid_impl): the same bits
        var = self.variants(run, (h2, tower), [("S2A_CONV_PH", ("1", "2")), ("S2A_CONV_OG", ("1", "2"))])
        mt, mh = Meter("conv", C * 9), Meter("conv", hw.shape[1])
        for l in range(len(layout.sizes)):
            y, S = conv64(layout.level(x, l), w, b, 1, 3, relu=relu)
            tl = layout.level(tower, l)
            mt.add(tl, y, S)
            del y, S
            y, S = conv64(tl, hw, hb, 1, 1)
            mh.add(layout.level(head_out, l, hw.shape[0]), y, S)
            del y, S
        self.finish("pyramid.conv3x3_head:%s+%s" % (name, hname), {"tower": mt, "head": mh}, {"tower": relu},
                    dict(shape=[layout.batch, C, layout.sizes, out_channels, hw.shape[0]],
                         bit_nan_rerun=torch.equal(h2, head_out[:, :32]), bit_tower_equals_conv3x3=torch.equal(tower, tower_sep),
                         variants=var, **{"bit_" + k: v for k, v in var.items()}))

    def check_orpool(self, res, layout, x, packed_w, bias, out_channels, n_orientation=8):
        """ORConv + orientation max-pool: pooled == the max over runs of 8 of the kernel's own out (bitwise); both
        within their bounds (rot_pool64)"""
        from oracle.conv64 import conv64, rot_pool64
        from s2anet_amd import _lib
        out, pooled = res
        name, w, b = self.weights(packed_w)
        C = x.shape[1]

        def run():
            o, p = nan_like(out), nan_like(pooled)
            _lib.check(_lib.lib().s2a_orconv_pool_pyramid_f16(_lib.ptr(x), _lib.ptr(packed_w), _lib.ptr(bias), _lib.ptr(o),
                                                              _lib.ptr(p), layout.batch, C, out_channels,
                                                              ctypes.byref(layout.c), _lib.stream_ptr(x.device)))
            return o, p
        again = run()
        var = self.variants(run, (out, pooled), [("S2A_CONV_PH", ("1", "2"))])
        og = {}
        for v in ("1", "2"):
            with env(S2A_CONV_OG=v):
                og[v] = run()
        meters = {"out": Meter("conv", C * 9), "pooled": Meter("conv", C * 9)}
        for v in og:
            meters["out:S2A_CONV_OG=" + v] = Meter("conv", C * 9)
            meters["pooled:S2A_CONV_OG=" + v] = Meter("conv", C * 9)
        for l in range(len(layout.sizes)):
            y, S = conv64(layout.level(x, l), w, b, 1, 3)
            py, pS = rot_pool64(y, S)
            meters["out"].add(layout.level(out, l), y, S)
            meters["pooled"].add(layout.level(pooled, l), py, pS)
            for v, (o, p) in og.items():
                meters["out:S2A_CONV_OG=" + v].add(layout.level(o, l), y, S)
                meters["pooled:S2A_CONV_OG=" + v].add(layout.level(p, l), py, pS)
            if l == 0:
                self.keep["orpool"] = dict(layout=layout, out=out, pooled=pooled, py=py, pS=pS)
            del y, S, py, pS
        own_pool = out.view(out.shape[0], out_channels // 8, 8).amax(-1)
        self.finish("pyramid.orconv_pool:%s" % name, meters, {},
                    dict(shape=[layout.batch, C, layout.sizes, out_channels],
                         bit_pooled_is_max_of_own_out=torch.equal(pooled, own_pool),
                         bit_nan_rerun=torch.equal(again[0], out) and torch.equal(again[1], pooled),
                         variants=var, **{"bit_" + k: v for k, v in var.items()}))

    def check_align(self, got, layout, x, anchors, packed_w, out_channels, relu=True):
        """k_dcn_patch on every level: sample points from the GPU's own align_offsets (the kernel's anchor_offset
        operation order), checked against oracle.align_offsets; reference deform_conv64 at f32 points"""
        import oracle
        from oracle.conv64 import align64
        from s2anet_amd import _lib
        from s2anet_amd.alignconv import align_offsets
        assert packed_w.data_ptr() == self.align_w.data_ptr()
        w = self.model.head.align_conv.deform_conv.weight
        B, C = layout.batch, x.shape[1]

        def run():
            o = nan_like(got)
            _lib.check(_lib.lib().s2a_align_conv_pyramid_f16(_lib.ptr(x), _lib.ptr(anchors), _lib.ptr(packed_w), _lib.ptr(o),
                                                             B, C, out_channels, int(bool(relu)), ctypes.byref(layout.c),
                                                             _lib.stream_ptr(x.device)))
            return o
        again = run()
        var = self.variants(run, got, [("S2A_DCN_HALF_TAIL", ("0", "1"))])
        m = Meter("dcn16", C * 9, L2_DCN)
        off_dev = 0.0
        for l, ((H, W), s) in enumerate(zip(layout.sizes, layout.strides)):
            a = layout.rows(anchors, l).view(B, H * W, 5)
            off = align_offsets(a, (H, W), s)
            for bi in sorted({0, B - 1}):
                ref_off = oracle.align_offsets(a[bi].cpu().numpy(), H, W, s)
                off_dev = max(off_dev, float(np.abs(off[bi].cpu().numpy() - ref_off).max()))
            y, S, Sc = align64(layout.level(x, l), off, w, relu=relu, d=DP)
            m.add(layout.level(got, l), y, S, extra=2 * DP * Sc)
            if l == 0:
                self.keep["align_p3"] = dict(y=y, S=S, Sc=Sc, run=run, layout=layout)
            del y, S, Sc
        self.keep["align_inputs"] = dict(layout=layout, x=x, anchors=anchors)
        if off_dev > DP:
            self.failures.append("%s align_offsets differ from oracle.align_offsets by %.3g px > %.3g" % (self.tag, off_dev, DP))
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        tiles = sum(B * ((W + 15) // 16) * ((H + 7) // 8) for H, W in layout.sizes)
        self.finish("pyramid.align_conv", {"out": m}, {"out": relu},
                    dict(shape=[B, C, layout.sizes, out_channels], tiles=tiles,
                         half_tail=bool(tiles > ncu and 0 < 2 * (tiles % ncu) <= ncu), offsets_vs_oracle_px=off_dev,
                         delta_p=DP, bit_nan_rerun=torch.equal(again, got), variants=var,
                         **{"bit_" + k: v for k, v in var.items()}))


# ----------------------------------------------------------------------------- the two geometries
def bench_images():
    g = torch.Generator(device="cpu").manual_seed(1234)
    t = torch.randint(0, 256, (8, 3, 1024, 1024), dtype=torch.uint8, generator=g).to(DEV)
    return t.contiguous(memory_format=torch.channels_last)


def ragged_images():
    g = torch.Generator(device="cpu").manual_seed(99)
    t = torch.randint(0, 256, (2, 3, 800, 1344), dtype=torch.uint8, generator=g).to(DEV)
    return t.contiguous(memory_format=torch.channels_last)


@pytest.fixture(scope="module")
def model():
    from s2anet_amd.detector import build_synthetic_detector
    m = build_synthetic_detector(num_classes=15, seed=1234, dtype=torch.float16, device=DEV)
    imgs = bench_images()
    with torch.no_grad():                                # bench.py's calibrate_cls_bias: logit std 1.5
        p = m.features_to_pred(imgs, m.backbone.forward_u8(imgs, 255.0))
        raw = torch.cat([l.float().reshape(-1) for l in p[2]])
        std = raw.std().item()
        assert math.isfinite(std), std
        if std > 0:                                      # (a constant classifier has nothing to scale)
            m.head.odm_cls_head.weight.mul_(1.5 / std)
    REPORT.append(dict(calibration_logit_std=std))
    return m


def record(model, imgs, tag, allow_library_conv):
    with torch.no_grad():                               # (ORConv2d.rotate_arf caches its filter only without grad)
        rec = Recorder(model, tag, allow_library_conv, imgs)
    with rec, torch.no_grad():
        dets, labels, counts = model.detect(imgs)
        torch.cuda.synchronize()
    rec.counts["detections"] = int(counts.sum())
    return rec


@pytest.fixture(scope="module")
def geometry_a(model):
    for k in ("S2A_OWN_CONV_ALWAYS", "S2A_CONV_WINO", "S2A_NO_OWN_CONV"):
        assert not os.environ.get(k), k
    return record(model, bench_images(), "A", True)


@pytest.fixture(scope="module")
def geometry_b(model):
    with env(S2A_OWN_CONV_ALWAYS="1"):
        return record(model, ragged_images(), "B", False)


KINDS = ("stem_u8", "conv_f16", "conv1x1_add_up2", "bottleneck_tail", "conv3x3", "conv3x3_head", "orconv_pool", "align_conv")


def assert_clean(rec):
    assert not rec.unattributed, ("C-ABI calls outside every checked launch", sorted(set(rec.unattributed)))
    assert not rec.failures, rec.failures[:20]
    assert all(e["ok"] for e in rec.entries)
    for k in KINDS:
        assert rec.counts.get(k, 0) > 0, (k, rec.counts)
    assert "conv1x1" not in rec.counts
    REPORT.append(dict(geometry=rec.tag, counts=rec.counts, allowed=rec.allowed, attributed=rec.attributed))
    _report_write()


def test_benchmark_forward_every_launch(geometry_a):
    rec = geometry_a
    assert_clean(rec)
    stem = [e for e in rec.entries if e["launch"] == "stem"][0]
    assert stem["tiles_per_wg"] == 16, stem                    # 8192 tiles on 512 persistent workgroups
    al = [e for e in rec.entries if e["launch"] == "pyramid.align_conv"][0]
    assert al["tiles"] == 1368 and al["half_tail"], al
    kinds = {(e["ksize"], e["stride"], e["shape"][4]) for e in rec.entries if e["launch"].startswith("conv_f16")}
    assert {(3, 1, 128), (3, 1, 256), (3, 2, 128), (1, 1, 256), (1, 2, 512)} <= kinds, kinds
    assert rec.allowed.get("s2a_bias_act_nhwc_to", 0) == 2, rec.allowed      # P6 / P7 on the library
    assert any(e["launch"] == "pyramid.conv3x3:head.odm_cls_ls.0.0" and e["shape"][1] == 32 for e in rec.entries)


def test_ragged_forward_every_launch(geometry_b):
    rec = geometry_b
    assert_clean(rec)
    assert "s2a_bias_act_nhwc_to" not in rec.allowed           # S2A_OWN_CONV_ALWAYS: P6 / P7 on conv_f16 too
    assert any(e["launch"] == "conv_f16:neck.fpn_convs.3" for e in rec.entries)


# ----------------------------------------------------------------------------- f32 AlignConv at the head's shapes
@pytest.mark.parametrize("geom", ("A", "B"))
@pytest.mark.parametrize("kernel", ("x3", "mfma32"))
def test_alignconv_f32_head_shapes(request, model, geom, kernel):
    """S.AlignConv in f32 on the recorded FPN levels and refined anchors (P3 [8,256,128,128] .. P7 at (A)).
    Planted at P3 of (A): tap 4's sample points rounded to multiples of 2^-6 px on one 8 x 16 tile of the last image --
    the reference built from them must be rejected (the report says by which check)"""
    import s2anet_amd as S
    from oracle.conv64 import align64
    from s2anet_amd.alignconv import align_offsets
    rec = request.getfixturevalue("geometry_a" if geom == "A" else "geometry_b")
    inp = rec.keep["align_inputs"]
    layout, x, anchors = inp["layout"], inp["x"], inp["anchors"]
    m = S.AlignConv(256, 256, 3).to(DEV).float()
    w = model.head.align_conv.deform_conv.weight.detach().float()
    with torch.no_grad():
        m.deform_conv.weight.copy_(w)
    B = layout.batch
    meters, defect = {}, None
    for l, ((H, W), s) in enumerate(zip(layout.sizes, layout.strides)):
        xl = layout.level(x, l).float()
        a = layout.rows(anchors, l).view(B, H, W, 5)
        with torch.no_grad(), env(S2A_DCN_F32="mfma32" if kernel == "mfma32" else "x3"):
            out = m(xl, a, s)
        off = align_offsets(a.reshape(B, H * W, 5), (H, W), s)
        y, Sv, Sc = align64(xl, off, w, relu=True, d=DP)
        mt = meters["P%d" % (l + 3)] = Meter("dcn32_" + kernel, 256 * 9, L2_F32)
        mt.add(out, y, Sv, extra=2 * DP * Sc)
        del y, Sv, Sc
        if geom == "A" and l == 0:
            # the f32 points the kernel forms, fl32(base + offset), exact in f64; tap t rounded to 2^-6 px on the tile
            t, y0, x0 = 4, 64, 64
            base = [(torch.arange(H, device=DEV).view(H, 1) - 1 + t // 3).float().expand(H, W),
                    (torch.arange(W, device=DEV).view(1, W) - 1 + t % 3).float().expand(H, W)]
            t_all = torch.arange(9, device=DEV)
            bh = (torch.arange(H, device=DEV).view(1, H, 1) - 1 + (t_all // 3).view(9, 1, 1)).float()
            bw = (torch.arange(W, device=DEV).view(1, 1, W) - 1 + (t_all % 3).view(9, 1, 1)).float()
            pts = torch.empty((B, 18, H, W), dtype=torch.float64, device=DEV)
            pts[:, 0::2] = (bh + off[:, 0::2]).double()
            pts[:, 1::2] = (bw + off[:, 1::2]).double()
            for ch in (2 * t, 2 * t + 1):
                tile = pts[B - 1, ch, y0:y0 + 8, x0:x0 + 16]
                pts[B - 1, ch, y0:y0 + 8, x0:x0 + 16] = torch.round(tile * 64) / 64
            bad = torch.empty_like(pts)
            bad[:, 0::2] = pts[:, 0::2] - bh.double()
            bad[:, 1::2] = pts[:, 1::2] - bw.double()
            moved = (pts[B - 1, 2 * t:2 * t + 2, y0:y0 + 8, x0:x0 + 16] -
                     torch.stack(base)[:, y0:y0 + 8, x0:x0 + 16].double() - off[B - 1, 2 * t:2 * t + 2, y0:y0 + 8,
                                                                                   x0:x0 + 16].double()).abs().max().item()
            yd, Sd, Scd = align64(xl, bad, w, pos_dtype=None, relu=True, d=DP)
            md = Meter("dcn32_" + kernel, 256 * 9, L2_F32)
            md.add(out, yd, Sd, extra=2 * DP * Scd)
            defect = dict(max_point_move_px=moved, rejected_by=md.rejected_by(), **md.summary())
            del yd, Sd, Scd
    REPORT.append(dict(geometry=geom, launch="AlignConv_f32", kernel=kernel, shape=[B, 256, layout.sizes, 256],
                       stages={k: v.summary() for k, v in meters.items()}))
    if defect is not None:
        REPORT.append(dict(geometry=geom, launch="defect:alignconv_f32_tap4_points_2^-6_one_tile_P3", kernel=kernel,
                           **defect))
    _report_write()
    for k, mt in meters.items():
        assert mt.ok_elem() and mt.ok_l2(), (geom, kernel, k, mt.summary())
    if defect is not None:
        assert defect["max_point_move_px"] > 0 and defect["rejected_by"], ("planted 2^-6 px points not rejected", defect)


# ----------------------------------------------------------------------------- planted defects
def _meter(out, y, S, kind, K, l2_bound=L2_CONV, extra=None):
    m = Meter(kind, K, l2_bound)
    m.add(out, y, S, extra)
    return m


def test_planted_defects_a(geometry_a):
    """each defect planted for one recorded launch of the real forward, as an altered float64 reference from the launch's
    real inputs or on the kernel's output: the comparison must reject it"""
    import torch.nn.functional as F
    from oracle.conv64 import _conv_nhwc, conv64, stem64, u8_to_f16
    rec, res = geometry_a, {}
    # 1. layer-3 conv2: the 64-channel chunk 64..127 of tap (1, 1) missing on one 8 x 16 output tile
    k = rec.keep["l3c2"]
    part = torch.einsum("bchw,oc->bohw", k["x"][0:1, 64:128, 0:8, 16:32].double(), k["w"][:, 64:128, 1, 1].double())
    y = k["y"].clone()
    t = y[0:1, :, 0:8, 16:32]
    y[0:1, :, 0:8, 16:32] = torch.where(t > 0, (t - part).clamp_min(0), t)
    m = _meter(k["out"], y, k["S"], k["m"].kind, k["m"].K)
    res["l3c2_missing_chunk"] = m.summary()
    assert not m.ok_elem(), m.summary()
    # 3. conv1x1_add_up2: one (odd) output row's coarse term read at (y + 1) >> 1
    k = rec.keep["up2"]
    y = k["y"].clone()
    row = 2 * (y.shape[2] // 4) + 1
    c = k["coarse"].double()
    y[:, :, row] += (c[:, :, (row + 1) >> 1] - c[:, :, row >> 1]).repeat_interleave(2, -1)
    m = _meter(k["out"], y, k["S"], "conv_res", k["m"].K)
    res["up2_coarse_row"] = m.summary()
    assert not m.ok_elem(), m.summary()
    # 4a. the stem with its pool window shifted by one pixel on the last tile row (image 0)
    k = rec.keep["stem"]
    conv = rec.model.backbone.backbone[0][0]
    img = rec.imgs[0:1]
    yc, _ = _conv_nhwc(u8_to_f16(img).permute(0, 2, 3, 1).double(), conv.weight.double(), 2, 3)
    yc = (yc + conv.bias.double()).clamp_min(0).permute(0, 3, 1, 2)
    Hp = k["y"].shape[2]
    r0 = (Hp - 1) // 8 * 8
    shifted = F.max_pool2d(F.pad(yc[:, :, 1:], (0, 0, 0, 1)), 3, 2, 1)
    y = k["y"][0:1].clone()
    y[:, :, r0:] = shifted[:, :, r0:Hp]
    m = _meter(k["out"][0:1], y, k["S"][0:1], "stem", 147)
    res["stem_pool_shift_last_tile_row"] = m.summary()
    assert not m.ok_elem(), m.summary()
    del yc, shifted
    # 4b. the stem with R and B swapped on one tile's input
    swapped = img.clone()
    swapped[:, [0, 2], 32:64, 64:96] = img[:, [2, 0], 32:64, 64:96]
    y, S = stem64(swapped, conv.weight, conv.bias)
    m = _meter(k["out"][0:1], y, S, "stem", 147)
    res["stem_rb_swap_one_tile"] = m.summary()
    assert not m.ok_elem(), m.summary()
    # 5. orconv_pool pooling strided channels (c, c + 32, ...) on one block of 128 positions
    k = rec.keep["orpool"]
    pooled = k["pooled"].clone()
    pooled[:128] = k["out"][:128].view(128, 8, 32).amax(1)
    m = _meter(k["layout"].level(pooled, 0), k["py"], k["pS"], "conv", 256 * 9)
    res["orconv_pool_strided"] = m.summary()
    assert not m.ok_elem(), m.summary()
    # 6. a layer-4 1x1 (K = 2048) with one input channel dropped -- a typical one: the median-energy channel among those
    #    that are not all zero after the ReLU; the L2 check catches it
    k = rec.keep["l4c1"]
    energy = k["x"].double().square().sum((0, 2, 3))
    live = torch.nonzero(energy > 0).flatten()
    ch = int(live[energy[live].argsort()[live.numel() // 2]])
    xd = k["x"].clone()
    xd[:, ch] = 0
    y, S = conv64(xd, k["w"], k["b"], 1, 1, relu=k["relu"])
    m = _meter(k["out"], y, S, "conv", 2048)
    res["l4c1_dropped_channel"] = dict(channel=ch, live_channels=live.numel(),
                                       energy_share=(energy[ch] / energy.sum()).item(), rejected_by=m.rejected_by(),
                                       **m.summary())
    assert not m.ok_l2(), m.summary()
    # 7. the pyramid AlignConv with binary16 coordinates (S2A_DCN_HALF_COORDS=1) fails the f32-coordinate bounds on P3
    k = rec.keep["align_p3"]
    with env(S2A_DCN_HALF_COORDS="1"):
        hc = k["run"]()
    m = _meter(k["layout"].level(hc, 0), k["y"], k["S"], "dcn16", 256 * 9, L2_DCN, extra=2 * DP * k["Sc"])
    res["align_half_coords_P3"] = dict(rejected_by=m.rejected_by(), **m.summary())
    REPORT.append(dict(geometry="A", launch="planted_defects", defects=res))
    _report_write()
    assert not (m.ok_elem() and m.ok_l2()), m.summary()


def test_planted_defect_ragged_tile_b(geometry_b):
    """2. on the ragged last tile column of a (B) launch, the tile's output replaced by its left neighbour's"""
    k = geometry_b.keep["ragged"]
    out = k["out"].clone()
    Wo = out.shape[3]
    c0 = Wo // 16 * 16
    out[:, :, 0:8, c0:] = k["out"][:, :, 0:8, c0 - 16:c0 - 16 + (Wo - c0)]
    m = _meter(out, k["y"], k["S"], k["m"].kind, k["m"].K)
    REPORT.append(dict(geometry="B", launch="defect:ragged_tile_from_left_neighbour:" + k["name"], **m.summary()))
    _report_write()
    assert not m.ok_elem(), m.summary()
