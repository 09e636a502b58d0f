"""Non-finite values on the training path: f16 training with a loss scale relies on an overflowed value reaching the
gradients as inf / NaN, so that TrainUpdate finds it, skips the step and backs the scale off.  tests/test_gpu_optim.py
checks that last link; this file checks the links before it: the training convolutions (FusedConvFunction), the fused
AlignConv under grad, the orientation pooling and the loss, and the whole chain once.  AlignConv's input gradient is
summed with float atomics, so for that one tensor locality reads "the independent set stays finite and within the
bound" (nonfinite_cases.contract, exact_locality=False); its output and weight gradient take the rules as they are.

Fixtures, entry classes, the float64 references and the per-tensor contract (class map, locality, dependent finite
entries) are in tests/nonfinite_cases.py; their side conditions are held by tests/test_train_nonfinite_cpu.py.  The
float64 side runs on the CPU from the same f16-rounded inputs.  At finite entries ReLU decisions follow production's
output, as test_gpu_train_conv.reference does; at non-finite ones torch's rule holds: an entry passes unless out <= 0,
so it passes at a NaN.  The sanitised run is itself checked against float64 with test_gpu_train_conv.verify."""
import pytest
import torch

import nonfinite_cases as N
import test_gpu_autograd_twin as TW
import test_gpu_train_conv as TC

pytestmark = pytest.mark.gpu
DEV = TW.DEV
F16, F32, F64 = torch.float16, torch.float32, torch.float64


def test_constants_are_the_projects():
    assert N.FACTOR == TW.FACTOR and N.U == TW.U


# ----------------------------------------------------------------------------- FusedConv2d
def conv_module(t, geom, master):
    from s2anet_amd.fused import FusedConv2d
    k, relu = geom
    O, C = t["w"].shape[:2]
    m = FusedConv2d(C, O, k, 1, k // 2, bias=True, relu=relu).to(DEV, F32 if master else F16)
    with torch.no_grad():
        m.weight.copy_(t["w"])
        m.bias.copy_(t["b"])
    cl = dict(memory_format=torch.channels_last)
    return m, t["x"].to(DEV).contiguous(**cl), None if t["r"] is None else t["r"].to(DEV).contiguous(**cl), \
        t["cot"].to(DEV).contiguous(**cl)


def conv_violations(tag, fx, master, pattern):
    """the contract of nonfinite_cases.contract for the output and every gradient of the pattern -> violations"""
    k, relu = fx["geom"]
    mp, xp, rp, cp = conv_module(fx["planted"], fx["geom"], master)
    ms, xs, rs, cs = conv_module(fx["sanitised"], fx["geom"], master)
    prod_p = TC.run(mp, xp, rp, cp, pattern, True)
    prod_s = TC.run(ms, xs, rs, cs, pattern, True)
    stock_s = TC.run(ms, xs, rs, cs, pattern, False, autocast=master)
    ref_p, _ = N.conv_reference(fx["planted"], k, relu, prod_p["out"] > 0)
    ref_s, _ = N.conv_reference(fx["sanitised"], k, relu, prod_s["out"] > 0)
    bad = []
    wanted = ["out"] + [N.TENSOR_OF[c] for c in TC.PATTERNS[pattern] if not (c == "r" and rp is None)]
    for name in ("out", "x", "weight", "bias", "residual"):
        if name not in wanted:
            if prod_p[name] is not None:
                bad.append("%s: grad(%s) was not requested but is not None" % (pattern, name))
            continue
        if prod_p[name] is None or prod_s[name] is None:
            bad.append("%s: %s is None" % (pattern, name))
            continue
        bad += N.contract("%s/%s/%s" % (tag, pattern, name), prod_p[name], prod_s[name], stock_s[name], ref_p[name], ref_s[name])
    return bad, (ms, xs, rs, cs)


def conv_check(tag, fx, master, pattern):
    bad, sane = conv_violations(tag, fx, master, pattern)
    TC.verify(tag + "/sanitised", *sane, master, (pattern,))          # anchors the sanitised run in float64
    assert not bad, tag + ":\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
@pytest.mark.parametrize("case,where", N.FORWARD_PLANTS, ids=["%s-%s" % cw for cw in N.FORWARD_PLANTS])
def test_fused_conv_forward_plants(case, where, master):
    conv_check("%s/%s/%s" % (case, where, "f32" if master else "f16"), N.conv_fixture(case, where), master, "ALL")


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
@pytest.mark.parametrize("pattern", N.BACKWARD_PATTERNS)
def test_fused_conv_backward_plants(pattern, master):
    conv_check("cot/%s" % ("f32" if master else "f16"), N.conv_fixture(N.FIRST, "cot"), master, pattern)


# ----------------------------------------------------------------------------- AlignConv
def align_run(t, anchors, dtype, fused):
    """forward + backward of AlignConv on the differentiable fused route, or of the unfused route (align_offsets ->
    deform_conv -> relu), which is the stock side of the bound -> {"out", "x", "weight"}"""
    import s2anet_amd as S
    from s2anet_amd.alignconv import AlignConvFunction, align_offsets
    O, C = t["w"].shape[:2]
    ac = S.AlignConv(C, O, 3).to(DEV, dtype)
    with torch.no_grad():
        ac.deform_conv.weight.copy_(t["w"])
    x = t["x"].to(DEV, dtype).requires_grad_(True)
    anc = anchors.to(DEV)
    B, _, H, W = x.shape
    with torch.enable_grad():
        if fused:
            assert ac.fused_ok(x)
            out = ac(x, anc, N.ALIGN_STRIDE)
            assert type(out.grad_fn).__name__.startswith(AlignConvFunction.__name__)
        else:
            offset = align_offsets(anc.reshape(B, H * W, 5), (H, W), N.ALIGN_STRIDE)
            out = torch.relu(S.deform_conv(x, offset, ac.deform_conv.weight, 1, 1))
    out.backward(t["cot"].to(DEV, dtype))
    return {"out": out.detach(), "x": x.grad, "weight": ac.deform_conv.weight.grad}


# (case, S2A_DCN_F32): the f32 forward runs on the f32 matrix instruction with mfma32, where the class map is exact; by
# default it splits its operands into three bf16 planes, which turns an infinite pre-activation into NaN (documented in
# include/s2anet_hip.h): that deviation is PINNED here (align_reference(inf_is_nan=True)), no more than that is allowed
ALIGN_MODES = [("f16_64to64", None), ("f32_32to64", "mfma32"), ("f32_32to64", None)]


@pytest.mark.parametrize("plant", list(N.ALIGN_PLANTS))
@pytest.mark.parametrize("case,mode", ALIGN_MODES, ids=["f16", "f32_mfma32", "f32_x3_pinned"])
def test_align_conv_plants(case, mode, plant, monkeypatch):
    if mode:
        monkeypatch.setenv("S2A_DCN_F32", mode)
    else:
        monkeypatch.delenv("S2A_DCN_F32", raising=False)
    dtype = N.ALIGN_CASES[case][0]
    pin = dtype == F32 and mode is None
    fx = N.align_fixture(case, plant)
    h, w = N.align_points(fx["anchors"])
    assert float(torch.minimum((h - h.round()).abs().min(), (w - w.round()).abs().min())) > 1e-3
    prod_p = align_run(fx["planted"], fx["anchors"], dtype, True)
    prod_s = align_run(fx["sanitised"], fx["anchors"], dtype, True)
    stock_s = align_run(fx["sanitised"], fx["anchors"], dtype, False)
    ref_p, _ = N.align_reference(fx["planted"], fx["anchors"], prod_p["out"] > 0, inf_is_nan=pin)
    ref_s, _ = N.align_reference(fx["sanitised"], fx["anchors"], prod_s["out"] > 0)
    tag = "align/%s/%s/%s" % (case, mode or "x3", plant)
    bad = []
    for name in ("out", "x", "weight"):
        got = prod_p[name]
        assert got is not None and got.dtype == dtype and tuple(got.shape) == tuple(ref_p[name].shape), name
        bad += N.contract("%s/%s" % (tag, name), got, prod_s[name], stock_s[name], ref_p[name], ref_s[name],
                          exact_locality=name != "x")
        # the sanitised run against float64, whole tensor, with the project's bound
        e_prod, e_stock = TC.rel(prod_s[name].cpu(), ref_s[name]), TC.rel(stock_s[name].cpu(), ref_s[name])
        if not e_prod <= N.FACTOR * e_stock + 2 * N.U[dtype]:
            bad.append("%s/%s: sanitised run e_prod %.3e > %g * %.3e + 2u" % (tag, name, e_prod, N.FACTOR, e_stock))
    assert not bad, tag + ":\n  " + "\n  ".join(bad)


# ----------------------------------------------------------------------------- orientation pooling
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_rot_inv_pool_routes_like_torch_max(dtype, channels_last):
    import s2anet_amd as S
    x0, go = N.pool_fixture()
    v64, g64, _ = N.pool_reference(x0, go)
    x = x0.to(DEV, dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    with torch.enable_grad():
        y = S.rot_inv_pool(x, 8)
    assert y.grad_fn is not None and y.dtype == dtype
    y.backward(go.to(DEV, dtype))
    assert torch.equal(N.classes(y), N.classes(v64))
    assert N.same(y, v64), "forward values differ from torch.max(dim) in float64"      # (all values are exact in f16)
    assert x.grad.dtype == dtype and N.counts(x.grad)[0] == x.grad.numel()
    wrong = int((x.grad.detach().cpu().double() != g64).sum())
    assert wrong == 0, "%d gradient entries are routed to another orientation than torch.max(dim)" % wrong


# ----------------------------------------------------------------------------- loss
def loss_case(dtype):
    import test_gpu_loss as TL
    g, p = TL.golden_p(dtype)
    head = TL.make_head()
    targets = torch.from_numpy(g["targets"]).to(DEV)
    ids, ts, off = head.assign_labels_fam_odm(p, targets)
    return p, ids, ts, off


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", list(N.LOSS_SCENARIOS))
def test_loss_plants(name, dtype):
    from s2anet_amd import s2anet_loss
    p, ids, ts, off = loss_case(dtype)
    shapes = [tuple(t.shape[2:]) for t in p[0]]
    plants, ids_c = N.loss_plants(name, ids.cpu(), ts.cpu(), off.cpu(), shapes)
    with torch.no_grad():
        for k, lvl, at, v in plants:
            p[k][lvl][at] = v
    maps = [t for lst in p[:4] for t in lst]
    loss, items = s2anet_loss(*p, ids_c.to(DEV), ts, off)
    loss.backward()
    got = [t.grad.detach().cpu() for t in maps]
    p64 = [[t.detach().cpu().double().requires_grad_(True) for t in lst] for lst in p[:4]] + [[a.cpu() for a in lst] for lst in p[4:]]
    rl, ritems = N.loss_reference(p64, ids_c, ts.cpu(), off.cpu())
    rl.sum().backward()
    items, ritems = items.detach().cpu().double(), ritems.detach()
    print(name, dtype, "items", items.tolist(), "float64", ritems.tolist())
    fin = torch.isfinite(ritems)
    assert torch.equal(torch.isfinite(items), fin), (items, ritems)
    assert [k for k in range(4) if not bool(fin[k])] == list(N.LOSS_SCENARIOS[name][4])
    assert bool(((items - ritems)[fin].abs() <= 2e-5 * ritems[fin].abs() + 1e-7).all()), (items, ritems)   # test_gpu_loss's
    assert bool(torch.isfinite(loss.detach()).all()) == bool(fin.all())
    bad = []
    for j, (a, t) in enumerate(zip(got, [t for lst in p64[:4] for t in lst])):
        r = t.grad
        assert a.dtype == dtype
        a = a.double()
        rfin = torch.isfinite(r)
        if not torch.equal(torch.isfinite(a), rfin):
            bad.append("map %d: %d entries non-finite in float64 but finite in production, %d the other way" % (
                j, int((~rfin & torch.isfinite(a)).sum()), int((rfin & ~torch.isfinite(a)).sum())))
            continue
        if bool(rfin.any()):
            # grads_close of test_gpu_loss.py over the finite entries only.  An f16 map's gradient is the f32 value v rounded
            # once (test_f16_maps_and_determinism holds it bit-equal to .half() of the f32 run): |v - r| <= tol gives
            # |half(v) - r| <= tol + half an f16 ulp at r, no more; the half ulp is taken from the f16 grid itself.
            # (Comparing with half(r) instead needs a WHOLE ulp: v and r can lie on two sides of a rounding boundary.)
            tol = 1e-4 * r[rfin].abs() + 1e-6 * r[rfin].abs().max()
            if dtype == F16:
                r16 = r[rfin].to(F16).abs()
                tol = tol + 0.5 * (torch.nextafter(r16, torch.full_like(r16, N.INF)).double() - r16.double())
            n = int(((a[rfin] - r[rfin]).abs() > tol).sum())
            if n:
                bad.append("map %d: %d finite gradient entries off" % (j, n))
    for k, lvl, at, v in plants:
        if not N.LOSS_SCENARIOS[name][4] and float(got[5 * k + lvl][at]) != 0.0:
            bad.append("a plant that does not enter the loss has gradient %r" % float(got[5 * k + lvl][at]))
    assert not bad, name + ":\n  " + "\n  ".join(bad)


# ----------------------------------------------------------------------------- the chain
def chain_step(overflow, own):
    """layer 1 -> layer 2 -> <out, cot> through TrainUpdate.scale_loss -> backward -> step(); f32 masters"""
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d
    f = N.chain_fixture(overflow)
    l1 = FusedConv2d(64, 64, 3, 1, 1, relu=True).to(DEV, F32)
    l2 = FusedConv2d(64, 64, 1, relu=True).to(DEV, F32)
    with torch.no_grad():
        for m, w, b in ((l1, "w1", "b1"), (l2, "w2", "b2")):
            m.weight.copy_(f[w])
            m.bias.copy_(f[b])
    net = torch.nn.ModuleList([l1, l2])
    assert S.train_kernels(net, own) == 2
    params = list(net.parameters())
    upd = S.TrainUpdate([{"params": params, "lr": 0.01, "weight_decay": 1e-4}], loss_scale=1024.0)
    before = [q.detach().clone() for q in params]
    x = f["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    cot = f["cot"].to(DEV).contiguous(memory_format=torch.channels_last)
    assert S.train_conv_ok(x, l1) and S.train_conv_ok(x, l2)
    with torch.enable_grad(), torch.autocast("cuda", F16, enabled=not own):
        y = l2(l1(x))
        assert y.dtype == F16
        loss = (y.float() * cot.float()).sum()
        upd.scale_loss(loss).backward()
    upd.step()
    torch.cuda.synchronize()
    stats = upd.stats.cpu().tolist()
    print("chain overflow=%s own=%s: loss %r stats %s scale %r out classes %s" % (
        overflow, own, float(loss.detach()), stats, float(upd.scale), N.counts(y)))
    unchanged = all(torch.equal(a, q.detach()) for a, q in zip(before, params))
    still = all(int((upd.momentum_buffer(q) != 0).sum()) == 0 for q in params)
    return stats, float(upd.scale), unchanged, still, y.detach()


@pytest.mark.parametrize("own", [True, False], ids=["train_kernels_on", "train_kernels_off"])
def test_chain_overflow_is_found_and_the_step_skipped(own):
    stats, scale, unchanged, still, y = chain_step(True, own)
    assert stats[2] == 1.0 and stats[3] == 1.0, "found_inf / skip not raised: %s" % stats
    assert unchanged and still, "a skipped step moved parameters or momentum buffers"
    assert scale == 512.0
    if own:
        _, _, out2 = N.chain_reference(N.chain_fixture(True))
        assert torch.equal(N.classes(y), N.classes(out2))


@pytest.mark.parametrize("own", [True, False], ids=["train_kernels_on", "train_kernels_off"])
def test_chain_without_the_overflow_is_not_skipped(own):
    stats, scale, unchanged, still, y = chain_step(False, own)
    assert stats[2] == 0.0 and stats[3] == 0.0 and scale == 1024.0
    assert not unchanged and not still
    assert N.counts(y)[0] == y.numel()


# ----------------------------------------------------------------------------- planted defects
def test_planted_training_forward_through_the_inference_relu(monkeypatch):
    """FusedConvFunction.forward with the ReLU fused into the launch (NaN -> 0, documented for inference)"""
    from s2anet_amd import _lib, fused

    @staticmethod
    def forward(ctx, x, weight, bias, residual, relu):
        O, C, k, _ = weight.shape
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        w = weight.detach().contiguous()
        fwd = torch.empty((w.numel(),), dtype=F16, device=x.device)
        dgrad = torch.empty_like(fwd) if need_x else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().s2a_conv_pack_weight_train(_lib.ptr(w), _lib.dtype_code(w), O, C, k, _lib.ptr(fwd),
                                                             _lib.ptr(dgrad), _lib.stream_ptr(x.device)))
        out = fused.conv_f16(x, fwd, None if bias is None else bias.detach(), O, k, 1, relu, residual)
        ctx.save_for_backward(x if need_w else None, out if relu else None, dgrad)
        ctx.geom = (tuple(x.shape), O, k, weight.dtype, None if bias is None else bias.dtype)
        return out
    monkeypatch.setattr(fused.FusedConvFunction, "forward", forward)
    bad, _ = conv_violations("planted/inference_relu", N.conv_fixture(N.FIRST, "x"), True, "ALL")
    print(bad)
    assert any("out: class map differs" in b and "NaN -> finite" in b for b in bad), bad


def test_planted_backward_mask_out_greater_than_zero(monkeypatch):
    """the backward sees NaN outputs as 0: its mask then acts as `out > 0` and drops the gradient at a NaN output"""
    from s2anet_amd import fused
    real = fused.FusedConvFunction.forward

    class Ctx:
        """the autograd context with save_for_backward intercepted: the saved output loses its NaNs, everything else
        (needs_input_grad, geom) goes to the real context"""

        def __init__(self, ctx):
            object.__setattr__(self, "ctx", ctx)

        def __getattr__(self, name):
            return getattr(object.__getattribute__(self, "ctx"), name)

        def __setattr__(self, name, value):
            setattr(object.__getattribute__(self, "ctx"), name, value)

        def save_for_backward(self, x, out, dgrad):
            out = None if out is None else torch.nan_to_num(out, nan=0.0, posinf=N.INF)
            object.__getattribute__(self, "ctx").save_for_backward(x, out, dgrad)

    @staticmethod
    def forward(ctx, x, weight, bias, residual, relu):
        return real(Ctx(ctx), x, weight, bias, residual, relu)
    monkeypatch.setattr(fused.FusedConvFunction, "forward", forward)
    bad, _ = conv_violations("planted/mask_gt", N.conv_fixture(N.FIRST, "x"), True, "ALL")
    print(bad)
    assert any("bias: dependent finite entries e_prod" in b for b in bad), bad
    assert any("/x: " in b for b in bad) and not any("/out: " in b for b in bad), bad
