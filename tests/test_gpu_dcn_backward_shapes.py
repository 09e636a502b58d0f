"""GPU: the fused deformable-conv backward (dcn._fused_backward -> s2a_deform_conv_backward_typed, the call
AlignConvFunction.backward makes) at the head's shapes -- C = O = 256 on every FPN level, the batch-8 P3 call bench.py
times, a ragged pyramid, other channel counts, the thinnest legal maps -- against the float64 reference
(oracle/dcn64.py), in f16 and f32 (both f32 weight kernels); planted defects that the comparison must catch; AlignConv
end to end through autograd; a HIP-graph captured training step replayed on new inputs.

Every gradient entry is held to |got - ref| <= tau * S + tiny, S the sum of the absolute values of the products that
make it up (oracle/dcn64.py), tau counted from unit roundoff per dtype, kernel and gradient (tau() below); the global
bounds of the older tests hold too, and a relative L2 bound that sees errors spread too thin for the elementwise one.
Set S2A_DCN_SHAPES_REPORT=<path> to write every measured ratio as JSON."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16, U32 = 2.0 ** -11, 2.0 ** -24
TILE = {torch.float16: (4, 16), torch.float32: (4, 8)}     # kBTH x kBTW / kFTH x kFTW (weight tiles: 4 x 16, 4 x 8)
HALO = 4                                                   # kBHalo, kFHalo
GLOBAL = {(torch.float32, k): 1e-4 for k in ("input", "offset", "weight")}
GLOBAL.update({(torch.float16, "input"): 4e-3, (torch.float16, "offset"): 4e-3, (torch.float16, "weight"): 6e-3})
# relative L2 error: f16 -- every product carries one f16 rounding of a column / bilinear weight / fraction and the result
# one more, each at most U16 relative and independent, so the L2 error stays near U16 / sqrt(3) per rounding; f32 -- sums
# of up to a few thousand terms in f32
L2 = {torch.float16: 2 * U16, torch.float32: 64 * U32}
REPORT = []


def tau(dtype, kernel, grad, C, O, tiles_per_wg, ksplit):
    """elementwise bound / S from unit roundoff: one u per rounding a product of the sum sees.
    f16 input:  f16 bilinear weights (u16) x f32 column gradient (O/16 MFMA steps) summed in f32, one f16 rounding of the
                result (u16)                                                      -> 2 u16 + (O + 64) u32
    f16 offset: f16 fractions and corner values (u16), f16 result (u16), f32 sums -> 2 u16 + (O + C + 64) u32
    f16 weight: f16 columns (blend of f16 weights: 2 u16), exact f16 products summed in f32 along the tile walk and the
                ksplit reduction, the result handed back in f16 (u16)            -> 3 u16 + (tiles * 64 / 16 + ksplit + 16) u32
    f32 input / offset: the same sums in f32                                      -> (O + 64) u32 / (O + C + 64) u32
    f32 weight x3: three bf16 planes per operand (the dropped cross terms < 3 u32 per product); mfma32: f32 products;
                the walk as above with four positions per MFMA step             -> (tiles * 32 / 4 + ksplit + 16) u32 (+ 4 u32 x3)"""
    if dtype == torch.float16:
        return {"input": 2 * U16 + (O + 64) * U32, "offset": 2 * U16 + (O + C + 64) * U32,
                "weight": 3 * U16 + (tiles_per_wg * 4 + ksplit + 16) * U32}[grad]
    return {"input": (O + 64) * U32, "offset": (O + C + 64) * U32,
            "weight": (tiles_per_wg * 8 + ksplit + 16 + (4 if kernel == "x3" else 0)) * U32}[grad]


def walk(dtype, B, C, H, W):
    """(tiles per weight workgroup, ksplit) of the weight kernels (fused_bwd_run: ksplit = min(tiles, 256 / owners))"""
    th, tw = TILE[dtype]
    tiles = B * -(-H // th) * -(-W // tw)
    ksplit = max(1, min(tiles, min(torch.cuda.get_device_properties(0).multi_processor_count, 256) // (3 * (C // 64))))
    return -(-tiles // ksplit), ksplit


# ----------------------------------------------------------------------------- inputs
def refined_anchors(gen, B, H, W, stride):
    """tests/test_gpu_loss.py:full_size_batch's refined anchors (jittered centres), sizes 0.5 - 8 x (4 * stride), angles
    -0.7 .. 2.3"""
    from s2anet_amd.loss import grid_anchors
    a = grid_anchors((H, W), stride, 4.0, DEV).view(1, H, W, 5).repeat(B, 1, 1, 1)
    a[..., :2] += torch.randn((B, H, W, 2), device=DEV, generator=gen) * (4.0 * stride) * 0.1
    a[..., 2:4] = 4.0 * stride * (0.5 + 7.5 * torch.rand((B, H, W, 2), device=DEV, generator=gen))
    a[..., 4] = -0.7 + 3.0 * torch.rand((B, H, W), device=DEV, generator=gen)
    return a


def edge_block(gen, off, rows):
    """samples of image 0, its first and last `rows` rows, moved onto exact integers (-1 and H included), into the bands
    (-1, 0) and (H-1, H), within a few 2^-12 of the far edge (the fraction 1 - 2^-12 that f16 cannot hold), and far
    outside"""
    _, _, H, W = off.shape
    t = torch.arange(9, device=DEV)
    for r0 in sorted({0, H - rows}):
        ys = (torch.arange(r0, r0 + rows, device=DEV).view(1, rows, 1) - 1 + (t // 3).view(9, 1, 1)).float()
        xs = (torch.arange(W, device=DEV).view(1, 1, W) - 1 + (t % 3).view(9, 1, 1)).float()
        shape = (9, rows, W)

        def pick(n):
            kind = torch.randint(0, 6, shape, device=DEV, generator=gen)
            r = torch.rand(shape, device=DEV, generator=gen)
            k = torch.randint(1, 4, shape, device=DEV, generator=gen).float()
            return torch.where(kind == 0, torch.randint(-1, n + 1, shape, device=DEV, generator=gen).float(),
                   torch.where(kind == 1, -0.05 - 0.9 * r,
                   torch.where(kind == 2, n - 0.95 + 0.9 * r,
                   torch.where(kind == 3, torch.where(r < 0.5, -30.0, n + 30.0),
                   torch.where(kind == 4, n - k * 2.0 ** -12,
                               torch.randint(0, n, shape, device=DEV, generator=gen).float() + 0.5)))))
        off[0, 0::2, r0:r0 + rows] = pick(H) - ys
        off[0, 1::2, r0:r0 + rows] = pick(W) - xs


def make_case(seed, B, C, O, H, W, stride, dtype, wild=True):
    """-> x, offset (f32 holding what the kernel gets), weight, grad_output (masked by the library's forward output like
    AlignConvFunction), wild-row start, the offsets before the f16 rounding.  Offsets: align_offsets of refined anchors;
    the last image's lower half gets N(0, 6 px) on top (the wild set); image 0's top and bottom rows hold the edge
    block."""
    from s2anet_amd import deform_conv
    from s2anet_amd.alignconv import align_offsets
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((B, C, H, W), device=DEV, generator=gen).to(dtype)
    w = (torch.randn((O, C, 3, 3), device=DEV, generator=gen) / math.sqrt(9 * C)).to(dtype)
    off = align_offsets(refined_anchors(gen, B, H, W, stride).view(B, H * W, 5), (H, W), stride)
    wild0 = H // 2
    if wild:
        off[B - 1, :, wild0:] += 6.0 * torch.randn((18, H - wild0, W), device=DEV, generator=gen)
    edge_block(gen, off, max(1, min(H // 4, 8)))
    raw = off
    if dtype == torch.float16:
        off = off.half().float()                       # dcn._fused_backward hands the kernel f16 offsets
    out = deform_conv(x, off.to(dtype), w, 1, 1, 1, 1, 1)
    go = torch.randn((B, O, H, W), device=DEV, generator=gen).to(dtype).masked_fill(out <= 0, 0)
    return x, off, w, go, wild0, raw


def far_share(off, dtype, rows):
    """share of the samples of `rows` that land more than HALO pixels outside their tile (the global-atomic path)"""
    B, _, H, W = off.shape
    th, tw = TILE[dtype]
    t = torch.arange(9, device=DEV)
    y = torch.arange(H, device=DEV).view(1, 1, H, 1)
    xq = torch.arange(W, device=DEV).view(1, 1, 1, W)
    h = (y - 1 + (t // 3).view(1, 9, 1, 1)).double() + off[:, 0::2].double()
    w = (xq - 1 + (t % 3).view(1, 9, 1, 1)).double() + off[:, 1::2].double()
    y0, x0 = (y // th) * th, (xq // tw) * tw
    far = (h < y0 - HALO) | (h > y0 + th - 1 + HALO) | (w < x0 - HALO) | (w > x0 + tw - 1 + HALO)
    return far[..., rows, :].double().mean().item()


# ----------------------------------------------------------------------------- comparison
def reference(x, off, w, go):
    from oracle.dcn64 import deform_conv_backward64
    r = deform_conv_backward64(x, off, w, go, pos_dtype=torch.float32)
    r["go_l1"] = go.double().abs().sum((0, 2, 3))                    # per out-channel: the f16 columns' underflow floor
    return r


def run_fused(x, off, w, go, kernel):
    from s2anet_amd.dcn import _fused_backward
    old = os.environ.get("S2A_BWD_F32_WEIGHT")
    try:
        if kernel == "mfma32":
            os.environ["S2A_BWD_F32_WEIGHT"] = "mfma32"
        else:
            os.environ.pop("S2A_BWD_F32_WEIGHT", None)
        return _fused_backward(x, off.to(x.dtype), w, go)
    finally:
        if old is None:
            os.environ.pop("S2A_BWD_F32_WEIGHT", None)
        else:
            os.environ["S2A_BWD_F32_WEIGHT"] = old


def compare(got, ref, dtype, kernel, C, O, walk_):
    """-> {grad: metrics}, each with ok = all three bounds hold"""
    res = {}
    for g, name in zip(got, ("input", "offset", "weight")):
        r, S = ref["grad_" + name], ref["S_" + name]
        err = (g.double() - r).abs()
        t = tau(dtype, kernel, name, C, O, *walk_)
        # absolute floor: half an f16 subnormal step for an underflowed result; for the f16 weight gradient also per column
        # entry (a blend below 2^-25 is 0 in f16), summed over the positions with the gradOutput they meet
        tiny = 1e-30
        if dtype == torch.float16:
            tiny = 2.0 ** -25 * (1 + ref["go_l1"].view(-1, 1, 1, 1)) if name == "weight" else 2.0 ** -25
        ratio = torch.where(S > 0, err / S, torch.where(err > 0, math.inf, 0.0)).max().item()
        glob = err.max().item() / max(r.abs().max().item(), 1e-30)
        l2 = (err.norm() / max(r.norm().item(), 1e-30)).item()
        ok_e = bool((err <= t * S + tiny).all())
        res[name] = dict(ratio=ratio, tau=t, glob=glob, glob_bound=GLOBAL[(dtype, name)], l2=l2, l2_bound=L2[dtype],
                         ok=ok_e and glob <= GLOBAL[(dtype, name)] and l2 <= L2[dtype])
    return res


def record(case, dtype, kernel, res, **extra):
    REPORT.append(dict(case=case, dtype=str(dtype).replace("torch.", ""), kernel=kernel,
                       **{k: v for k, v in res.items()}, **extra))
    path = os.environ.get("S2A_DCN_SHAPES_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)


def kernels(dtype):
    return ("f16",) if dtype == torch.float16 else ("x3", "mfma32")


def check_level(case, x, off, w, go, dtype):
    """both f32 weight kernels / the f16 one against the reference; weight gradient bit-identical on a second call.
    -> {kernel: gradients}"""
    B, C, H, W = x.shape
    O = w.shape[0]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ref = reference(x, off, w, go)
    ref_peak = torch.cuda.max_memory_allocated() - base
    gots = {}
    for k in kernels(dtype):
        got = gots[k] = run_fused(x, off, w, go, k)
        res = compare(got, ref, dtype, k, C, O, walk(dtype, B, C, H, W))
        again = run_fused(x, off, w, go, k)
        same = torch.equal(got[2], again[2])
        record(case, dtype, k, res, shape=[B, C, O, H, W], weight_repeat_bitequal=same, ref_peak_bytes=ref_peak)
        for name, m in res.items():
            assert m["ok"], (case, k, name, m)
        assert same, (case, k)
    return gots


DTYPES = (torch.float16, torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "f32"))
def test_pyramid_1024(dtype):
    for lvl, (s, n) in enumerate(((8, 128), (16, 64), (32, 32), (64, 16), (128, 8))):
        x, off, w, go, _, _ = make_case(100 + lvl, 2, 256, 256, n, n, s, dtype)
        check_level("pyr1024_P%d" % (lvl + 3), x, off, w, go, dtype)


def planted(x, off, w, go, dtype):
    """the defects the comparison must catch: (name, offset, grad_output) handed to the reference instead"""
    B, _, H, W = x.shape
    th, tw = TILE[dtype]
    lost = go.clone()
    y0, x0 = (H // th // 2) * th, (W // tw // 2) * tw
    lost[B - 1, :, y0:y0 + th, x0:x0 + tw] = 0                       # one tile of the last image lost in the walk
    row = go.clone()
    row[:, :, (H - 1) // th * th:] = 0                               # the last (partial) tile row dropped
    q = torch.round(off * 256) / 256                                 # offsets rounded to 2^-8 px
    return (("lost_tile", off, lost), ("last_tile_row", off, row), ("offsets_2^-8", q, go))


def check_defects(case, x, off, w, go, dtype, gots):
    B, C, H, W = x.shape
    O = w.shape[0]
    for name, d_off, d_go in planted(x, off, w, go, dtype):
        ref = reference(x, d_off, w, d_go)
        for k, got in gots.items():
            res = compare(got, ref, dtype, k, C, O, walk(dtype, B, C, H, W))
            record(case + ":defect:" + name, dtype, k, res)
            for g, m in res.items():
                assert not m["ok"], ("defect not detected", case, name, k, g, m)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "f32"))
def test_benchmarked_call_p3_batch8(dtype):
    """8 x 256 x 128 x 128, the shape bench.py times: ~98 (f16) / ~195 (f32) tiles per weight workgroup"""
    x, off, w, go, wild0, raw = make_case(7, 8, 256, 256, 128, 128, 8, dtype)
    share = far_share(off[-1:], dtype, slice(wild0, None))
    assert share > 0.01, share                                       # the global-atomic path is really taken
    gots = check_level("P3x8", x, off, w, go, dtype)
    record("P3x8:wild_far_share", dtype, "-", {}, far_share=share)
    check_defects("P3x8", x, off, w, go, dtype, gots)
    if dtype == torch.float16:
        # the fused forward samples at f32 offsets, this backward at f16-rounded ones: how far apart the two gradients are
        from oracle.dcn64 import deform_conv_backward64
        a = deform_conv_backward64(x, raw, w, go, pos_dtype=torch.float32, scale=False)
        b = deform_conv_backward64(x, off, w, go, pos_dtype=torch.float32, scale=False)
        rel = {k: ((a[k] - b[k]).norm() / a[k].norm()).item() for k in a}
        record("P3x8:f16_offset_vs_f32_offset", dtype, "-", {}, rel_l2=rel)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "f32"))
def test_ragged_pyramid_1000x600(dtype):
    """partial tiles in every kernel; in f16 H*W % 8 != 0 sends the transposes to the scalar path"""
    levels = ((8, 125, 75), (16, 63, 38), (32, 32, 19), (64, 16, 10), (128, 8, 5))
    for lvl, (s, h, w_) in enumerate(levels):
        x, off, w, go, _, _ = make_case(200 + lvl, 3, 256, 256, h, w_, s, dtype)
        gots = check_level("ragged_P%d" % (lvl + 3), x, off, w, go, dtype)
        if lvl == 0:
            check_defects("ragged_P3", x, off, w, go, dtype, gots)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "f32"))
def test_other_channel_counts(dtype):
    """O = 160: the f32 non-EXACT input kernel; C = 512 / 1024: 24 and 48 weight owners"""
    for i, (C, O) in enumerate(((256, 160), (512, 256), (1024, 64))):
        x, off, w, go, _, _ = make_case(300 + i, 2, C, O, 40, 52, 8, dtype)
        check_level("C%d_O%d" % (C, O), x, off, w, go, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "f32"))
def test_thin_maps(dtype):
    for i, (h, w_) in enumerate(((3, 3), (3, 200), (200, 3))):
        x, off, w, go, _, _ = make_case(400 + i, 1, 256, 256, h, w_, 8, dtype)
        check_level("thin_%dx%d" % (h, w_), x, off, w, go, dtype)


# ----------------------------------------------------------------------------- through autograd
def alignconv_case(seed, B, C, O, H, W, stride, dtype):
    from s2anet_amd import AlignConv
    gen = torch.Generator(device=DEV).manual_seed(seed)
    m = AlignConv(C, O, 3).to(DEV).to(dtype)
    with torch.no_grad():
        m.deform_conv.weight.copy_(torch.randn((O, C, 3, 3), device=DEV, generator=gen) / math.sqrt(9 * C))
    x = torch.randn((B, C, H, W), device=DEV, generator=gen).to(dtype).contiguous(memory_format=torch.channels_last)
    anchors = refined_anchors(gen, B, H, W, stride)
    go = torch.randn((B, O, H, W), device=DEV, generator=gen).to(dtype)
    return m, x, anchors, go


def alignconv_reference(x, anchors, w, go, out, stride):
    """what AlignConvFunction.backward hands the deformable-conv backward: align_offsets of the anchors (f16-rounded for
    an f16 x), grad_output masked by the library's forward output"""
    from s2anet_amd.alignconv import align_offsets
    B, C, H, W = x.shape
    off = align_offsets(anchors.reshape(B, H * W, 5), (H, W), stride)
    if x.dtype == torch.float16:
        off = off.half().float()
    return reference(x, off, w, go.masked_fill(out <= 0, 0))


@pytest.mark.parametrize("dtype,C,O", ((torch.float16, 256, 256), (torch.float32, 256, 256), (torch.float32, 96, 64)),
                         ids=("f16", "f32", "f32-unfused-C96"))
def test_alignconv_autograd_end_to_end(dtype, C, O):
    """AlignConv with grad enabled and a channels_last x; C = 96 takes the unfused fallback (alignconv.py:94-100)"""
    B, H, W, stride = 2, 64, 64, 16
    m, x, anchors, go = alignconv_case(500 + C, B, C, O, H, W, stride, dtype)
    x.requires_grad_(True)
    out = m(x, anchors, stride)
    out.backward(go)
    w = m.deform_conv.weight
    ref = alignconv_reference(x.detach(), anchors, w.detach(), go, out.detach(), stride)
    kern = "f16" if dtype == torch.float16 else ("x3" if C % 64 == 0 else "unfused")
    res = compare((x.grad, torch.zeros_like(ref["grad_offset"]), w.grad), ref, dtype, kern, C, O, walk(dtype, B, C, H, W))
    record("alignconv_autograd_C%d" % C, dtype, kern, {k: res[k] for k in ("input", "weight")})
    for k in ("input", "weight"):
        assert res[k]["ok"], (k, res[k])


# ----------------------------------------------------------------------------- HIP graph
@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "f32"))
def test_graph_captured_backward_replays_on_new_inputs(dtype):
    """AlignConv forward + torch.autograd.grad captured at P3, B = 2, C = O = 256; three replays after copying new x,
    grad_output and anchors in: each against eager and the float64 reference; a repeated replay on the same inputs
    gives the same gradients (the accumulator is cleared inside the graph, k_bwd_zero4)"""
    B, C, O, H, W, stride = 2, 256, 256, 128, 128, 8
    m, sx, sa, sgo = alignconv_case(600, B, C, O, H, W, stride, dtype)
    sx.requires_grad_(True)
    w = m.deform_conv.weight

    def step():
        out = m(sx, sa, stride)
        gx, gw = torch.autograd.grad(out, (sx, w), sgo)
        return out, gx, gw

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_gx, g_gw = step()
    for rep in range(3):
        _, x, a, go = alignconv_case(610 + rep, B, C, O, H, W, stride, dtype)
        with torch.no_grad():
            sx.copy_(x)
            sa.copy_(a)
            sgo.copy_(go)
        graph.replay()
        torch.cuda.synchronize()
        out, gx, gw = g_out.clone(), g_gx.clone(), g_gw.clone()
        graph.replay()                                  # the same inputs again: nothing may be left from the last replay
        torch.cuda.synchronize()
        e_out, e_gx, e_gw = step()                      # eager on the same inputs
        assert torch.equal(out, e_out), rep
        assert torch.equal(gw, e_gw), rep
        assert torch.equal(g_gw, gw), rep
        ref = alignconv_reference(sx.detach(), sa, w.detach(), sgo, e_out.detach(), stride)
        res = compare((gx, torch.zeros_like(ref["grad_offset"]), gw), ref, dtype, kernels(dtype)[0], C, O,
                      walk(dtype, B, C, H, W))
        record("graph_replay_%d" % rep, dtype, kernels(dtype)[0], {k: res[k] for k in ("input", "weight")})
        assert res["input"]["ok"] and res["weight"]["ok"], (rep, res)
        # the input gradient's atomics may add in another order: eager and the second replay agree within rounding
        t = tau(dtype, "", "input", C, O, 1, 1)
        for other in (e_gx, g_gx):
            assert ((other.double() - gx.double()).abs() <= 2 * t * ref["S_input"] + 2.0 ** -24).all(), rep
