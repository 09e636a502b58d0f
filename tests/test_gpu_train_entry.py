"""GPU: the entry of the training step on the own kernels (s2anet_amd.train_kernels(model, True, entry=True)): the stem from
the uint8 batch (StemU8Function: s2a_stem_u8_f16_train, s2a_stem_backward_f16) and FPN's top-down steps
(FusedConvUp2Function: s2a_conv1x1_add_up2_f16, s2a_sum_pool2x2_f16), then the whole detector in deterministic mode.

Accuracy: the bound and the constants of tests/test_gpu_autograd_twin.py; per tensor (output or gradient, no entry excluded)
    e = |t - t64|_2 / |t64|_2,   e_prod <= FACTOR e_stock + 2 u(dtype of t).
Stem: the float64 backward (test_train_entry_cpu.stem_reference, the two formulas of include/s2anet_hip.h) takes production's
pooled taps and ReLU mask as given (the convention of tests/test_gpu_train_conv.py); e_stock is the stock route (F.conv2d on
img.half() / 255, ReLU, F.max_pool2d; under torch.autocast for f32 masters) against the same formulas under the stock run's
OWN indices and mask.  Where float64 is clear about it (the window's maximum leads the runner-up, the pre-activation is away
from zero, by more than BAND[F16] * rms) production's tap and mask must be float64's.

Shapes: 8 x 8 (one pooled 2 x 2 corner of one tile), 72 x 100 (partial tiles both ways, two images), 516 x 516 (289 tiles on
256 slices: the smallest square with more tiles than slices; 289 is no multiple of 256)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_autograd_twin import BAND, DEV, F16, F32, F64, FACTOR, U, channels_last_filters, folded_trunk, randn
from test_train_entry_cpu import STEM_COLS, sel_from_indices, stem_out_hw, stem_reference, sum_pool_reference
from workspace_guard import GuardedWorkspaces

pytestmark = pytest.mark.gpu

STEM_CASES = {"8x8": (1, 8, 8), "72x100": (2, 72, 100), "516x516": (1, 516, 516)}
MASKED = 3                                   # a map whose bias keeps every pre-activation below zero


def rel(a, ref):
    return float((a.to(F64) - ref.to(F64)).norm() / ref.to(F64).norm())


def make_image(B, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), device=DEV, generator=g, dtype=torch.uint8).permute(0, 3, 1, 2)


def make_stem(case, master, bias, seed=5):
    """-> (image uint8 [B,3,H,W] channels-last, weight, bias or None, cotangent [B,64,Hp,Wp] f16 channels-last)"""
    B, H, W = STEM_CASES[case]
    img = make_image(B, H, W, seed)
    dt = F32 if master else F16
    w = randn((64, 3, 7, 7), F32, seed + 1, scale=0.1).to(dt)
    b = None
    if bias:
        b = randn((64,), F32, seed + 2, scale=0.5)
        b[MASKED] = -40.0
        b = b.to(dt)
    _, (Hp, Wp) = stem_out_hw(H, W)
    cot = randn((B, 64, Hp, Wp), F16, seed + 3, cl=True)
    return img, w, b, cot


def lut64(img):
    """the values the forward multiplies: f16(u / 255) (an f32 division, one rounding), as float64"""
    return (img.float() / 255).half().to(F64)


def raw_forward(img, w, b, out=None, sel=None):
    """s2a_stem_u8_f16_train itself -> (out [B,64,Hp,Wp] f16 channels-last, sel [B,Hp,Wp,64] uint8)"""
    from s2anet_amd import _lib
    from s2anet_amd.fused import stem_pack_weight
    B, _, H, W = img.shape
    _, (Hp, Wp) = stem_out_hw(H, W)
    given = out is not None                     # (guarded byte buffers of the caller: handed back as they are)
    if not given:
        out = torch.empty((B, Hp, Wp, 64), dtype=F16, device=DEV)
        sel = torch.empty((B, Hp, Wp, 64), dtype=torch.uint8, device=DEV)
    b16 = None if b is None else b.detach().half().contiguous()
    _lib.check(_lib.lib().s2a_stem_u8_f16_train(_lib.ptr(img), _lib.ptr(stem_pack_weight(w)), _lib.ptr(b16), ctypes.c_void_p(out.data_ptr()),
                                                ctypes.c_void_p(sel.data_ptr()), B, H, W, 255.0, _lib.stream_ptr(DEV)))
    return (out, sel) if given else (out.permute(0, 3, 1, 2), sel)


def run_own(img, w, b, cot, what):
    import s2anet_amd as S
    w_ = w.detach().clone().requires_grad_("w" in what)
    b_ = None if b is None else b.detach().clone().requires_grad_("b" in what)
    with torch.enable_grad():
        y = S.StemU8Function.apply(img, w_, b_, 255.0)
        assert y.dtype == F16 and y.is_contiguous(memory_format=torch.channels_last) and y.requires_grad
        y.backward(cot)
    return {"out": y.detach(), "weight": w_.grad, "bias": None if b_ is None else b_.grad}


def run_stock(img, w, b, cot, what, master):
    """the stock route -> (results, its own pooled taps, its own mask)"""
    w_ = w.detach().clone().requires_grad_("w" in what)
    b_ = None if b is None else b.detach().clone().requires_grad_("b" in what)
    x = img.half() / 255
    with torch.enable_grad(), torch.autocast("cuda", torch.float16, enabled=master):
        conv = F.conv2d(x, w_, b_, 2, 3)
        y, idx = F.max_pool2d(F.relu(conv), 3, 2, 1, return_indices=True)
        y.backward(cot)
    return ({"out": y.detach(), "weight": w_.grad, "bias": None if b_ is None else b_.grad},
            sel_from_indices(idx, conv.shape[3]), y.detach() > 0)


PARAMS = [(m, b) for m in (False, True) for b in (True, False)]
PARAM_IDS = ["%s-%s" % ("f32_masters" if m else "f16_params", "bias" if b else "nobias") for m, b in PARAMS]


# ----------------------------------------------------------------------------- forward bits, taps, mask, gradients
@pytest.mark.parametrize("master,bias", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("case", list(STEM_CASES))
def test_stem_forward_bits_selection_and_gradients(case, master, bias):
    from s2anet_amd.fused import stem_pack_weight, stem_u8
    img, w, b, cot = make_stem(case, master, bias)
    bad = []
    patterns = ("wb", "w", "b") if bias else ("w",)
    first = None
    for what in patterns:
        prod = run_own(img, w, b, cot, what)
        if first is None:
            first = prod
            # forward bits: the inference kernel's
            want = stem_u8(img, stem_pack_weight(w), b)
            assert torch.equal(prod["out"].view(torch.int16), want.view(torch.int16)), "out differs from s2a_stem_u8_f16"
            out_raw, sel = raw_forward(img, w, b)
            assert torch.equal(out_raw.view(torch.int16), want.view(torch.int16))
            sel = sel.permute(0, 3, 1, 2)
            assert int(sel.max()) <= 8
            mask = prod["out"] > 0
            # float64 where it is clear: the pooled tap and the sign of the pooled pre-activation
            x64 = lut64(img)
            pre = F.conv2d(x64, w.detach().half().to(F64), None if b is None else b.detach().half().to(F64), 2, 3)
            rms = float(pre.pow(2).mean().sqrt())
            Bn, _, Hc, Wc = pre.shape
            _, (Hp, Wp) = stem_out_hw(*img.shape[2:])

            def windows(t):                                 # tap 3 dy + dx of every window; -inf outside the conv map
                t = F.pad(t, (1, 1, 1, 1), value=float("-inf")).reshape(Bn * 64, 1, Hc + 2, Wc + 2)
                return F.unfold(t, 3, stride=2).view(Bn, 64, 9, Hp, Wp)
            top = windows(F.relu(pre)).topk(2, dim=2)       # what the pool sees
            clear = (top.values[:, :, 0] - top.values[:, :, 1]) > BAND[F16] * rms
            n = int((clear & (sel.long() != top.indices[:, :, 0])).sum())
            if n:
                bad.append("%d pooled taps differ from float64's where the maximum leads by more than the band" % n)
            pooled = windows(pre).amax(2)                   # the pre-activation behind the pooled output
            clear = pooled.abs() > BAND[F16] * rms
            n = int((clear & (mask != (pooled > 0))).sum())
            if n:
                bad.append("%d mask entries outside the band take another branch than float64" % n)
            if bias:
                assert not bool(mask[:, MASKED].any()) and bool(mask.any())
        else:
            assert torch.equal(prod["out"], first["out"])
        stock, sel_s, mask_s = run_stock(img, w, b, cot, what, master)
        ref = dict(zip(("weight", "bias"), stem_reference(x64, sel, mask, cot)))
        ref_s = dict(zip(("weight", "bias"), stem_reference(x64, sel_s, mask_s, cot)))
        for name, c in (("weight", "w"), ("bias", "b")):
            got = prod[name]
            if c not in what:
                if got is not None:
                    bad.append("%s: grad(%s) was not requested but is not None" % (what, name))
                continue
            leaf = w if name == "weight" else b
            if got is None or got.dtype != leaf.dtype or tuple(got.shape) != tuple(leaf.shape):
                bad.append("%s: grad(%s) is %s" % (what, name, None if got is None else (got.dtype, tuple(got.shape))))
                continue
            e_prod, e_stock = rel(got, ref[name]), rel(stock[name], ref_s[name])
            bound = FACTOR * e_stock + 2 * U[got.dtype]
            print("%-28s %-3s %-7s e_prod %.3e e_stock %.3e bound %.3e ratio %.3f" % (case + "/" + PARAM_IDS[PARAMS.index((master, bias))],
                                                                                     what, name, e_prod, e_stock, bound, e_prod / bound))
            if not e_prod <= bound:
                bad.append("%s: %s e_prod %.3e > %g * %.3e + 2u = %.3e" % (what, name, e_prod, FACTOR, e_stock, bound))
    assert not bad, case + ":\n  " + "\n  ".join(bad)


def test_stem_tie_rule_is_atens():
    """a zero filter under bias 1: every tap of every window ties at 1, the first tap inside the map stays"""
    for case in ("8x8", "72x100"):
        B, H, W = STEM_CASES[case]
        img = make_image(B, H, W, 9)
        out, sel = raw_forward(img, torch.zeros((64, 3, 7, 7), dtype=F16, device=DEV), torch.ones((64,), dtype=F16, device=DEV))
        (Hc, Wc), _ = stem_out_hw(H, W)
        ones, idx = F.max_pool2d(torch.ones((B, 64, Hc, Wc), device=DEV), 3, 2, 1, return_indices=True)
        assert torch.equal(out.float(), ones)
        assert torch.equal(sel.permute(0, 3, 1, 2), sel_from_indices(idx, Wc)), case


# ----------------------------------------------------------------------------- every byte is written (C ABI)
@pytest.mark.parametrize("case", list(STEM_CASES))
def test_stem_entries_write_their_buffers_in_full_and_nothing_else(case):
    from s2anet_amd import _lib
    L = _lib.lib()
    img, w, b, cot = make_stem(case, False, True)
    B, _, H, W = img.shape
    _, (Hp, Wp) = stem_out_hw(H, W)
    n = B * Hp * Wp * 64
    slices = L.s2a_stem_backward_slices(B, H, W)
    assert slices == min(B * ((Hp + 7) // 8) * ((Wp + 7) // 8), 256)
    g = cot.permute(0, 2, 3, 1).contiguous()
    outs, sels, parts = [], [], []
    for fill in (0xA5, 0xFF):                               # 0xFF..: NaN in f16 and in f32
        gw = GuardedWorkspaces(fill)
        o_v, s_v, p_v = gw(n * 2, DEV, "out"), gw(n, DEV, "sel"), gw(slices * STEM_COLS * 4, DEV, "partial")
        raw_forward(img, w, b, o_v, s_v)
        gw.check()
        outs.append(o_v.clone())
        sels.append(s_v.clone())
        for wrong in (slices + 1, slices - 1):              # refused, nothing touched
            rc = L.s2a_stem_backward_f16(_lib.ptr(img), _lib.ptr(o_v), _lib.ptr(s_v), _lib.ptr(g), _lib.ptr(p_v), wrong, B, H, W,
                                         255.0, _lib.stream_ptr(DEV))
            torch.cuda.synchronize()
            assert rc == _lib.EINVAL and bool((p_v == fill).all())
        _lib.check(L.s2a_stem_backward_f16(_lib.ptr(img), _lib.ptr(o_v), _lib.ptr(s_v), _lib.ptr(g), _lib.ptr(p_v), slices, B, H, W,
                                           255.0, _lib.stream_ptr(DEV)))
        gw.check()
        parts.append(p_v.clone())
    assert torch.equal(outs[0], outs[1]), "out depends on what the buffer held: not every element is written"
    assert torch.equal(sels[0], sels[1]), "sel depends on what the buffer held: not every element is written"
    assert torch.equal(parts[0], parts[1]), "partial depends on what the buffer held: not every element is written"
    part = parts[0].view(F32).view(slices, STEM_COLS)
    assert bool(torch.isfinite(part).all())
    # the reduce is the slices' sum in slice order, and it is the gradient
    acc = torch.zeros((STEM_COLS,), dtype=F32, device=DEV)
    for s in range(slices):
        acc = acc + part[s]
    red = torch.empty((STEM_COLS,), dtype=F32, device=DEV)
    _lib.check(L.s2a_conv_backward_weight_s2_reduce(_lib.ptr(part), slices, STEM_COLS, _lib.ptr(red), _lib.DTYPE_F32, _lib.stream_ptr(DEV)))
    assert torch.equal(acc, red)
    sel = sels[0].view(B, Hp, Wp, 64).permute(0, 3, 1, 2)
    out = outs[0].view(F16).view(B, Hp, Wp, 64).permute(0, 3, 1, 2)
    gw64, gb64 = stem_reference(lut64(img), sel, out > 0, cot)
    # WHAT was written: f16 products are exact in f32, only the f32 sums round.  A chain of n adds of random terms is off by
    # about sqrt(n / 2) u of its result; n <= 129 * 129 windows here (91 u), and 512 u is under six times that
    assert rel(red[:64 * 147].view(64, 3, 7, 7), gw64) <= 512 * U[F32]
    assert rel(red[64 * 147:], gb64) <= 512 * U[F32]


def test_stem_slices_hold_their_tiles():
    """slices = min(tiles, 256), so every slice owns a tile; in the 516 x 516 case slice s < 33 holds the sums of tiles s and
    s + 256 and every other slice those of tile s alone: checked on the bias sums"""
    from s2anet_amd import _lib
    L = _lib.lib()
    img, w, b, cot = make_stem("516x516", False, True)
    out, sel = raw_forward(img, w, b)
    g = cot.permute(0, 2, 3, 1).contiguous()
    part = torch.empty((256, STEM_COLS), dtype=F32, device=DEV)
    _lib.check(L.s2a_stem_backward_f16(_lib.ptr(img), _lib.ptr(out.permute(0, 2, 3, 1)), _lib.ptr(sel), _lib.ptr(g), _lib.ptr(part), 256,
                                       1, 516, 516, 255.0, _lib.stream_ptr(DEV)))
    # the bias sums of slice s: the masked cotangent summed over tiles s and s + 256 (17 tiles a row, 8 x 8 windows a tile)
    gm = torch.where(out > 0, cot, torch.zeros_like(cot)).to(F64)[0]                  # [64,129,129]
    gm = F.pad(gm, (0, 7, 0, 7)).view(64, 17, 8, 17, 8).sum((2, 4)).reshape(64, 289)  # per tile, tile = ty * 17 + tx
    want = gm[:, :256].clone()
    want[:, :33] += gm[:, 256:]
    got = part[:, 64 * 147:].t().to(F64)
    assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max())


# ----------------------------------------------------------------------------- reproducible, capturable
@pytest.mark.parametrize("case", ["72x100", "516x516"])
def test_stem_two_fresh_runs_are_bit_equal(case):
    runs = []
    for _ in range(2):
        img, w, b, cot = make_stem(case, True, True)
        runs.append(run_own(img, w, b, cot, "wb"))
    for name, a in runs[0].items():
        assert torch.equal(a, runs[1][name]), name


def test_stem_forward_and_backward_in_one_graph():
    import s2anet_amd as S
    img, w, b, cot = make_stem("72x100", True, True)
    w.requires_grad_(True)
    b.requires_grad_(True)
    leaves = [w, b]

    def step():
        y = S.StemU8Function.apply(img, w, b, 255.0)
        y.backward(cot)
        return y

    def eager():
        for t in leaves:
            t.grad = None
        with torch.enable_grad():
            y = step()
        return [y.detach().clone()] + [t.grad.clone() for t in leaves]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.enable_grad():
        step()
    torch.cuda.current_stream().wait_stream(side)
    for t in leaves:
        t.grad = torch.zeros_like(t)
    static = [t.grad for t in leaves]
    graph = torch.cuda.CUDAGraph()
    with torch.enable_grad(), torch.cuda.graph(graph):
        y_static = step()
    for round_ in range(2):
        with torch.no_grad():
            img.copy_(make_image(*STEM_CASES["72x100"], 40 + round_))          # new image bytes in the static batch
            if round_:
                w.mul_(1.25)
            for g in static:
                g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = [y_static.clone()] + [g.clone() for g in static]
        want = eager()
        for t, g in zip(leaves, static):
            t.grad = g
        for i, (a, c) in enumerate(zip(got, want)):
            assert torch.equal(a, c), (round_, i)
        assert float(got[1].abs().max()) > 0


# ----------------------------------------------------------------------------- routing
def _boom(*a, **kw):
    raise AssertionError("a stock op was reached on the own training route")


def test_route_switch_on_never_reaches_the_stock_stem(monkeypatch):
    import s2anet_amd as S
    from s2anet_amd import fused
    trunk = folded_trunk(F16)
    S.train_kernels(trunk, True, strided=True, entry=True)
    img = make_image(2, 72, 100, 3)
    assert trunk.stem_limits(img)
    monkeypatch.setattr(fused.F, "conv2d", _boom)
    monkeypatch.setattr(fused.F, "max_pool2d", _boom)
    for p in trunk.parameters():
        p.requires_grad_(True)
    with torch.enable_grad():
        outs = trunk(img)
        sum(o.float().sum() for o in outs).backward()
    conv = trunk.backbone[0][0]
    assert conv.weight.grad is not None and conv.weight.grad.dtype == F16 and float(conv.weight.grad.abs().max()) > 0
    assert conv.bias.grad is not None
    # outside the limits (a width that is no multiple of 4): / 255 and the stock route
    monkeypatch.undo()
    odd = make_image(1, 40, 42, 4)
    assert not trunk.stem_limits(odd)
    with torch.enable_grad():
        a = trunk(odd)
    trunk.backbone[0][0].own_grad_entry = False              # (the third switch alone: the rest of the trunk keeps its route)
    with torch.enable_grad():
        b = trunk(odd.to(F16) / 255)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_route_switch_off_keeps_todays_route_bit_for_bit(monkeypatch):
    import s2anet_amd as S
    from s2anet_amd import fused
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    trunk = folded_trunk(F16)
    conv = trunk.backbone[0][0]
    x = (make_image(2, 72, 100, 3).to(F16) / 255).contiguous(memory_format=torch.channels_last)
    real_conv, real_pool, calls = fused.F.conv2d, fused.F.max_pool2d, []

    def run():
        conv.zero_grad(set_to_none=True)
        with torch.enable_grad():
            outs = trunk(x)
            sum(o.float().sum() for o in outs).backward()
        return [o.detach() for o in outs] + [conv.weight.grad.clone(), conv.bias.grad.clone()]
    S.train_kernels(trunk, True)
    for p in trunk.parameters():
        p.requires_grad_(True)
    run()
    off = run()
    S.train_kernels(trunk, True, entry=True)                 # the switch on, a FLOAT batch: today's route
    monkeypatch.setattr(fused.F, "conv2d", lambda *a, **k: (calls.append("conv"), real_conv(*a, **k))[1])
    monkeypatch.setattr(fused.F, "max_pool2d", lambda *a, **k: (calls.append("pool"), real_pool(*a, **k))[1])
    on = run()
    assert "conv" in calls and "pool" in calls
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    S.train_kernels(trunk, True, entry=False)                # entry not mentioned: the flag stays
    assert conv.own_grad_entry is True
    with pytest.raises(RuntimeError):                        # a uint8 batch without grad (and outside detect()): as today
        with torch.no_grad():
            trunk(make_image(2, 72, 100, 3))


# ----------------------------------------------------------------------------- non-finite values
def test_stem_nonfinite_values_follow_torch():
    img, w, b, cot = make_stem("72x100", True, True)
    clean = run_own(img, w, b, cot, "wb")
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    # a NaN filter entry: its map is NaN wherever it is multiplied (everywhere: 0 * NaN at the border too); +inf bias: +inf
    w2, b2 = w.clone(), b.clone()
    w2[5, 1, 3, 3] = float("nan")
    b2[7] = float("inf")
    got = run_own(img, w2, b2, cot, "wb")
    assert bool(torch.isnan(got["out"][:, 5]).all()), "the inference epilogue's NaN -> 0 on the training route"
    assert bool((got["out"][:, 7] == float("inf")).all())
    rest = [c for c in range(64) if c not in (5, 7)]
    assert torch.equal(got["out"][:, rest], clean["out"][:, rest])
    assert torch.equal(got["weight"][rest], clean["weight"][rest]) and torch.equal(got["bias"][rest], clean["bias"][rest])
    assert bool(torch.isfinite(got["weight"][5]).all())      # the gradient passes at a NaN output: finite cotangent, finite image
    assert float(got["weight"][5].abs().max()) > 0
    # a NaN / inf cotangent under a passing window reaches both gradients of its map, and only them
    pos = (clean["out"][0, 11] > 0).nonzero()[0]
    pos2 = (clean["out"][1, 12] > 0).nonzero()[0]
    cot2 = cot.clone()
    cot2[0, 11, pos[0], pos[1]] = float("nan")
    cot2[1, 12, pos2[0], pos2[1]] = float("inf")
    got = run_own(img, w, b, cot2, "wb")
    assert bool(torch.isnan(got["bias"][11])) and bool(torch.isnan(got["weight"][11]).any())
    assert float(got["bias"][12]) == float("inf") and not bool(torch.isfinite(got["weight"][12]).all())
    rest = [c for c in range(64) if c not in (11, 12)]
    assert torch.equal(got["weight"][rest], clean["weight"][rest]) and torch.equal(got["bias"][rest], clean["bias"][rest])
    # under a masked window nothing contributes: not the image, not an inf or NaN cotangent (selected away, not multiplied)
    cot3 = cot.clone()
    cot3[0, MASKED, 2, 3] = float("inf")
    cot3[1, MASKED, 4, 1] = float("nan")
    got = run_own(img, w, b, cot3, "wb")
    assert int((got["weight"][MASKED] != 0).sum()) == 0 and float(got["bias"][MASKED]) == 0
    for name in ("weight", "bias"):
        assert torch.equal(got[name], clean[name]), name


# ----------------------------------------------------------------------------- FPN top-down
UP2_CASES = {"2x64x64_6x10": (2, 64, 64, 6, 10), "1x512x256_2x2": (1, 512, 256, 2, 2), "3x128x64_14x18": (3, 128, 64, 14, 18)}
UP2_PATTERNS = {"ALL": "xwbc", "X": "x", "PAR": "wb", "COARSE": "c"}


def make_up2(case, master, seed=13):
    from s2anet_amd.fused import FusedConv2d
    B, C, O, H, W = UP2_CASES[case]
    torch.manual_seed(seed)
    m = FusedConv2d(C, O, 1).to(DEV, F32 if master else F16)
    with torch.no_grad():
        m.bias.normal_(0, 0.5)
    x = randn((B, C, H, W), F16, seed + 1, cl=True)
    coarse = randn((B, O, H // 2, W // 2), F16, seed + 2, cl=True)
    cot = randn((B, O, H, W), F16, seed + 3, cl=True)
    return m, x, coarse, cot


def run_up2(m, x, coarse, cot, what, own, autocast=False):
    import s2anet_amd as S
    m.weight.requires_grad_("w" in what)
    m.bias.requires_grad_("b" in what)
    m.zero_grad(set_to_none=True)
    x_ = x.detach().requires_grad_("x" in what)
    c_ = coarse.detach().requires_grad_("c" in what)
    with torch.enable_grad():
        if own:
            assert S.train_up2_ok(x_, m, c_)
            y = S.FusedConvUp2Function.apply(x_, m.weight, m.bias, c_)
        else:
            with torch.autocast("cuda", torch.float16, enabled=autocast):
                lat = m(x_)
            y = lat + F.interpolate(c_, scale_factor=2, mode="nearest")    # (on f16, as FPN.forward sees it: autocast would widen it)
    assert y.dtype == F16 and y.shape == cot.shape
    y.backward(cot)
    return {"out": y.detach(), "x": x_.grad, "weight": m.weight.grad, "bias": m.bias.grad, "coarse": c_.grad}


@pytest.mark.parametrize("master", [False, True], ids=["f16_params", "f32_masters"])
@pytest.mark.parametrize("case", list(UP2_CASES))
def test_top_down_accuracy_every_pattern(case, master):
    m, x, coarse, cot = make_up2(case, master)
    x64, c64 = x.to(F64).requires_grad_(True), coarse.to(F64).requires_grad_(True)
    w64, b64 = m.weight.detach().to(F64).requires_grad_(True), m.bias.detach().to(F64).requires_grad_(True)
    with torch.enable_grad():
        y64 = F.conv2d(x64, w64, b64) + F.interpolate(c64, scale_factor=2, mode="nearest")
        y64.backward(cot.to(F64))
    ref = {"out": y64.detach(), "x": x64.grad, "weight": w64.grad, "bias": b64.grad, "coarse": c64.grad}
    names = {"x": "x", "w": "weight", "b": "bias", "c": "coarse"}
    bad = []
    for pattern, what in UP2_PATTERNS.items():
        m.own_grad = m.own_grad_entry = True
        prod = run_up2(m, x, coarse, cot, what, True)
        m.own_grad = m.own_grad_entry = False
        stock = run_up2(m, x, coarse, cot, what, False, autocast=master)
        for name in ["out"] + list(names.values()):
            wanted = name == "out" or [c for c in what if names[c] == name]
            got = prod[name]
            if not wanted:
                if got is not None:
                    bad.append("%s: grad(%s) was not requested but is not None" % (pattern, name))
                continue
            leaf = {"out": prod["out"], "x": x, "weight": m.weight, "bias": m.bias, "coarse": coarse}[name]
            if got is None or got.dtype != leaf.dtype or tuple(got.shape) != tuple(leaf.shape):
                bad.append("%s: %s is %s" % (pattern, name, None if got is None else (got.dtype, tuple(got.shape))))
                continue
            e_prod, e_stock = rel(got, ref[name]), rel(stock[name], ref[name])
            bound = FACTOR * e_stock + 2 * U[got.dtype]
            print("%-28s %-6s %-7s e_prod %.3e e_stock %.3e bound %.3e ratio %.3f" % (case + ("/f32" if master else "/f16"), pattern, name,
                                                                                     e_prod, e_stock, bound, e_prod / bound))
            if not e_prod <= bound:
                bad.append("%s: %s e_prod %.3e > %g * %.3e + 2u = %.3e" % (pattern, name, e_prod, FACTOR, e_stock, bound))
        if "c" in what:                                     # the sum-pool: header's formula in f32, bit for bit
            want = sum_pool_reference(cot, F32).to(F16)
            assert torch.equal(prod["coarse"], want), pattern
            assert prod["coarse"].is_contiguous(memory_format=torch.channels_last)
    assert not bad, case + ":\n  " + "\n  ".join(bad)


def test_sum_pool_writes_all_of_out_and_nothing_else():
    from s2anet_amd import _lib
    L = _lib.lib()
    B, O, H, W = 3, 64, 14, 18
    g = randn((B, H, W, O), F16, 3)
    n = B * (H // 2) * (W // 2) * O * 2
    got = []
    for fill in (0xA5, 0xFF):
        gw = GuardedWorkspaces(fill)
        v = gw(n, DEV, "out")
        _lib.check(L.s2a_sum_pool2x2_f16(_lib.ptr(g), _lib.ptr(v), B, H, W, O, _lib.stream_ptr(DEV)))
        gw.check()
        got.append(v.clone())
    assert torch.equal(got[0], got[1])
    want = sum_pool_reference(g.permute(0, 3, 1, 2), F32).to(F16).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(got[0].view(F16).view(B, H // 2, W // 2, O), want)


def make_neck(sizes):
    import s2anet_amd as S
    from s2anet_amd.detector import FPN, fuse_epilogues
    torch.manual_seed(31)
    neck = FPN(in_channels=(64, 128, 256), out_channels=128)
    for m in neck.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.normal_(m.bias, 0, 0.3)
    neck = channels_last_filters(fuse_epilogues(neck).to(DEV, F16))
    xs = [randn((2, c, h, w), F16, 4 + i, cl=True, grad=True) for i, (c, (h, w)) in enumerate(zip((64, 128, 256), sizes))]
    assert S.train_kernels(neck, True, strided=True) == 8
    return neck, xs


def neck_step(neck, xs):
    for x in xs:
        x.grad = None
    neck.zero_grad(set_to_none=True)
    with torch.enable_grad():
        outs = neck(xs)
        gen = torch.Generator(device=DEV).manual_seed(5)
        torch.autograd.backward(list(outs), [torch.randn(o.shape, device=DEV, generator=gen).to(F16) for o in outs])
    return [o.detach() for o in outs] + [x.grad for x in xs] + [p.grad for p in neck.parameters()]


def test_fpn_route_never_reaches_interpolate_and_odd_levels_fall_through(monkeypatch):
    import s2anet_amd as S
    from s2anet_amd import detector
    neck, xs = make_neck(((16, 20), (8, 10), (4, 5)))
    off = neck_step(neck, xs)
    S.train_kernels(neck, True, entry=True)
    with monkeypatch.context() as mp:
        mp.setattr(detector.F, "interpolate", _boom)
        on = neck_step(neck, xs)
        again = neck_step(neck, xs)
    assert all(torch.equal(a, b) for a, b in zip(on, again))
    for a, b in zip(on, off):                               # the same sums, other roundings: close, and checked per tensor above
        assert a.shape == b.shape and rel(a, b) < 0.02
    # a level that is no exact double (5 x 6 over 3 x 3) is outside the own step's limits and reaches the stock line, which
    # refuses it as it always did
    neck, xs = make_neck(((10, 12), (5, 6), (3, 3)))
    for entry in (False, True):
        S.train_kernels(neck, True, entry=entry)
        with pytest.raises(RuntimeError, match="must match the size"):
            neck(xs)
    # a level outside the limits for its layout (NCHW storage) falls through to the stock line, bit for bit
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    neck, xs = make_neck(((16, 20), (8, 10), (4, 5)))
    xs[1] = xs[1].detach().contiguous().requires_grad_(True)
    assert not xs[1].is_contiguous(memory_format=torch.channels_last)
    with torch.enable_grad():
        neck(xs)
        off = [o.detach() for o in neck(xs)]
    S.train_kernels(neck, True, entry=True)
    real, calls = detector.F.interpolate, []
    monkeypatch.setattr(detector.F, "interpolate", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.enable_grad():
        on = [o.detach() for o in neck(xs)]
    assert len(calls) >= 1
    for a, b in zip(on[1:], off[1:]):                       # from the fallen-through level upwards: the stock bits
        assert torch.equal(a, b)
    if len(calls) == 2:                                     # (its sum came back in NCHW: the step below it fell through as well)
        assert torch.equal(on[0], off[0])


# ----------------------------------------------------------------------------- the whole detector, deterministic mode
from test_gpu_deterministic_head import LOSS_SCALE, make_targets  # noqa: E402

DET_IMG = 384                                               # P3 .. P7 = 48, 24, 12, 6, 3: P7 is 3 x 3


def make_detector(seed=1234):
    import s2anet_amd as S
    from s2anet_amd.detector import build_synthetic_detector
    model = build_synthetic_detector(seed=seed).train()
    model.head.imgs_size = (DET_IMG, DET_IMG)
    S.train_kernels(model, True, strided=True, entry=True)
    for p in model.parameters():
        p.requires_grad_(True)
    return model


def det_step(model, imgs, table):
    p = model(imgs)["pred"]
    loss, items, status = model.head.compute_loss_device(p, table)
    (loss * LOSS_SCALE).backward()
    return loss, items, status


def fresh_detector_step():
    import s2anet_amd as S
    model = make_detector()
    imgs = make_image(2, DET_IMG, DET_IMG, 77)
    with S.deterministic(True), torch.enable_grad():
        loss, items, status = det_step(model, imgs, make_targets(2))
    assert int(status[0]) == 0
    out = {"loss": loss.detach(), "items": items.detach()}
    out.update({"grad(%s)" % n: p.grad for n, p in model.named_parameters()})
    return out


def test_detector_two_fresh_steps_are_bit_equal(monkeypatch):
    from s2anet_amd import detector, fused
    monkeypatch.setattr(fused.F, "max_pool2d", _boom)
    monkeypatch.setattr(detector.F, "interpolate", _boom)
    a, b = fresh_detector_step(), fresh_detector_step()
    assert set(a) == set(b) and len(a) > 100
    for name in a:
        assert a[name] is not None, name
        assert torch.equal(a[name], b[name]), name
    stem = a["grad(backbone.backbone.0.0.weight)"]
    assert bool(torch.isfinite(stem).all()) and float(stem.abs().max()) > 0


def test_detector_captured_step_replays_bit_equal_to_eager():
    import s2anet_amd as S
    model = make_detector()
    imgs = make_image(2, DET_IMG, DET_IMG, 77).contiguous(memory_format=torch.channels_last)
    table = make_targets(3)
    leaves = list(model.parameters())

    def eager():
        for t in leaves:
            t.grad = None
        with torch.enable_grad(), S.deterministic(True):
            loss, items, status = det_step(model, imgs, table)
        return [loss.detach().clone(), items.detach().clone(), status.clone()] + [t.grad.clone() for t in leaves]

    with S.deterministic(True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.enable_grad():
            det_step(model, imgs, table)
        torch.cuda.current_stream().wait_stream(side)
        for t in leaves:
            t.grad = torch.zeros_like(t)
        static = [t.grad for t in leaves]
        graph = torch.cuda.CUDAGraph()
        with torch.enable_grad(), torch.cuda.graph(graph):
            s_loss, s_items, s_status = det_step(model, imgs, table)
    for round_ in range(2):
        with torch.no_grad():
            if round_:
                imgs.copy_(make_image(2, DET_IMG, DET_IMG, 78))
                table.copy_(make_targets(4, n=9))
            for g in static:
                g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = [s_loss.detach().clone(), s_items.detach().clone(), s_status.clone()] + [g.clone() for g in static]
        want = eager()
        for t, g in zip(leaves, static):
            t.grad = g
        assert int(got[2][0]) == 0
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (round_, i)
