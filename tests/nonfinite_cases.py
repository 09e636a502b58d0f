"""Fixtures and float64 references for the non-finite tests of the training path (test_gpu_train_nonfinite.py on the
GPU, test_train_nonfinite_cpu.py for the fixtures' side conditions).  Everything here runs on the CPU from seeded CPU
generators, so both files see the same numbers.

Entry classes: every entry is FINITE, PINF, NINF or NAN (classes()).  No tensor that may hold a NaN is ever compared
bare: comparisons go through class maps, through masks of finite entries, or through same() (torch.equal on
nan_to_num'd float64 copies with three distinct sentinels).

The per-tensor contract (contract()), for the output and for every gradient, no entry excluded:
  1. the class map equals the float64 reference's, entry for entry;
  2. locality: an entry is INDEPENDENT when its float64 reference is finite and bit-identical between the planted input
     and the sanitised one (plants replaced by 0); every independent entry is equal between production's two runs;
  3. the other finite entries (DEPENDENT: relu(-inf) = 0, gradients whose ReLU mask changed) are within
     FACTOR * e_stock + 2u of float64 as an L2 ratio over those entries, e_stock being the stock route's ratio on the
     SANITISED input over the same entries; where the reference is exactly 0 production is exactly 0.
"Equal" in 2. is equality of values: the two zeros of a ReLU output compare equal."""
import math

import torch
import torch.nn.functional as F

F16, F32, F64 = torch.float16, torch.float32, torch.float64
U = {F32: 2.0 ** -24, F16: 2.0 ** -11}          # the constants of test_gpu_autograd_twin.py (asserted equal in the GPU file)
FACTOR = 4.0
FINITE, PINF, NINF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+inf", "-inf", "NaN")
INF, NANV = float("inf"), float("nan")
LIMIT = 1024.0                                   # no finite reference entry above it: rounding to f16 creates no infinity


# ----------------------------------------------------------------------------- classes
def classes(t):
    """int8 class map of t (any dtype, any device) on the CPU"""
    t = t.detach().to("cpu", F64)
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[t == INF] = PINF
    c[t == -INF] = NINF
    c[t != t] = NAN
    return c


def counts(t):
    c = classes(t)
    return [int((c == k).sum()) for k in range(4)]


def sanitised(t):
    return None if t is None else torch.where(torch.isfinite(t), t, torch.zeros_like(t))


def same(a, b):
    """torch.equal on float64 copies whose NaN / +inf / -inf became three distinct sentinels"""
    kw = dict(nan=1e300, posinf=2e300, neginf=-2e300)
    a, b = a.detach().to("cpu", F64), b.detach().to("cpu", F64)
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, **kw), torch.nan_to_num(b, **kw))


def partition(ref_p, ref_s):
    """-> (independent, dependent finite, non-finite) masks of the planted reference ref_p against the sanitised ref_s"""
    fin = torch.isfinite(ref_p)
    ind = fin & (torch.nan_to_num(ref_p, nan=1e300, posinf=2e300, neginf=-2e300) == ref_s)
    return ind, fin & ~ind, ~fin


def _l2(a, ref, at):
    d, r = (a[at] - ref[at]).norm(), ref[at].norm()
    return float(d / r) if float(r) > 0 else (0.0 if float(d) == 0 else INF)


def _l2_stock(a, ref, at):
    """e_stock over a set.  Where the sanitised reference vanishes over the whole set (a residual gradient behind a ReLU
    that blocks it without the plant) no ratio exists; e_stock is then 0 and the bound is 2u alone, never infinite."""
    return _l2(a, ref, at) if float(ref[at].norm()) > 0 else 0.0


def contract(name, got_p, got_s, stock_s, ref_p, ref_s, exact_locality=True):
    """the three rules for one tensor -> list of violations.  got_p / got_s: production on the planted / sanitised input;
    stock_s: the stock route on the sanitised input; ref_p / ref_s: float64 references (CPU).
    exact_locality=False, for a tensor that is summed with float atomics (AlignConv's input gradient: two runs on the
    SAME input are not bit-equal): rule 2 becomes "every independent entry is finite, and the independent set is within
    FACTOR * e_stock + 2u of float64", with e_stock over the same entries of the sanitised run."""
    bad = []
    u = U[got_p.dtype]
    gp, gs, st = (t.detach().to("cpu", F64) for t in (got_p, got_s, stock_s))
    cg, cr = classes(gp), classes(ref_p)
    if not torch.equal(cg, cr):
        moves = ["%d x %s -> %s" % (int(((cr == a) & (cg == b)).sum()), CLASS_NAMES[a], CLASS_NAMES[b])
                 for a in range(4) for b in range(4) if a != b and bool(((cr == a) & (cg == b)).any())]
        bad.append("%s: class map differs from float64 (reference -> production): %s" % (name, ", ".join(moves)))
    ind, dep, _ = partition(ref_p, ref_s)
    if exact_locality:
        leak = ind & ~(torch.nan_to_num(gp, nan=1e300, posinf=2e300, neginf=-2e300) == gs)
        if bool(leak.any()):
            bad.append("%s: %d of %d independent entries differ between the planted and the sanitised run" % (
                name, int(leak.sum()), int(ind.sum())))
    elif bool(ind.any()):
        leak = ind & ~torch.isfinite(gp)
        if bool(leak.any()):
            bad.append("%s: %d of %d independent entries are not finite" % (name, int(leak.sum()), int(ind.sum())))
        else:
            ei, es = _l2(gp, ref_p, ind), _l2_stock(st, ref_s, ind)
            if not ei <= FACTOR * es + 2 * u:
                bad.append("%s: independent entries e_prod %.3e > %g * %.3e + 2u" % (name, ei, FACTOR, es))
    zero = dep & (ref_p == 0)
    if bool((zero & ~(gp == 0)).any()):
        bad.append("%s: %d dependent entries are exactly 0 in float64 but not in production" % (name, int((zero & ~(gp == 0)).sum())))
    e_prod = e_stock = bound = 0.0
    if bool(dep.any()) and float(ref_p[dep].norm()) > 0:
        e_prod, e_stock = _l2(gp, ref_p, dep), _l2_stock(st, ref_s, dep)
        bound = FACTOR * e_stock + 2 * u
        if not e_prod <= bound:
            bad.append("%s: dependent finite entries e_prod %.3e > %g * %.3e + 2u = %.3e" % (name, e_prod, FACTOR, e_stock, bound))
    print("%-40s classes %s independent %d dependent %d e_prod %.3e e_stock %.3e bound %.3e%s" % (
        name, counts(ref_p), int(ind.sum()), int(dep.sum()), e_prod, e_stock, bound, "  VIOLATED" if bad else ""))
    return bad


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    """seeded CPU normal values that are exact in f16 (f32 masters and f16 parameters then hold the same numbers)"""
    return (torch.randn(shape, generator=_gen(seed)) * scale).to(F16)


# ----------------------------------------------------------------------------- FusedConv2d
# name: (k, B, C, O, H, W, relu, residual, plants in x [(b, c, y, x, value)])
# plants: the (0, 0) corner; the last channel of the last pixel of the last image; a pixel on the edge of a partial tile
# (3x3: 4 x 16 position tiles, 1x1: 64 consecutive positions); two opposite infinities in two channels of one pixel
CONV_CASES = {
    "3x3_relu_res_2x64x64_9x21": (3, 2, 64, 64, 9, 21, True, True,
                                  [(0, 3, 0, 0, INF), (1, 63, 8, 20, -INF), (0, 10, 8, 16, NANV), (1, 5, 4, 10, INF), (1, 40, 4, 10, -INF)]),
    "1x1_relu_3x128x64_7x9": (1, 3, 128, 64, 7, 9, True, False,
                              [(0, 3, 0, 0, INF), (2, 127, 6, 8, -INF), (1, 10, 0, 1, NANV), (1, 5, 3, 4, INF), (1, 40, 3, 4, -INF)]),
    "3x3_1x64x128_3x5": (3, 1, 64, 128, 3, 5, False, False,
                         [(0, 3, 0, 0, INF), (0, 63, 2, 4, -INF), (0, 10, 2, 0, NANV), (0, 5, 1, 2, INF), (0, 40, 1, 2, -INF)]),
}
FIRST = "3x3_relu_res_2x64x64_9x21"
# (case, where the plants go): "x" the five plants above; "w" / "b" / "r" a NaN in one filter (centre tap), bias, residual entry
FORWARD_PLANTS = [(c, "x") for c in CONV_CASES] + [(FIRST, "w"), (FIRST, "b"), (FIRST, "r")]
# classes the float64 OUTPUT must contain (a ReLU leaves no -inf)
FORWARD_EXPECT = {(FIRST, "x"): {FINITE, PINF, NAN}, ("1x1_relu_3x128x64_7x9", "x"): {FINITE, PINF, NAN},
                  ("3x3_1x64x128_3x5", "x"): {FINITE, PINF, NINF, NAN}, (FIRST, "w"): {FINITE, NAN}, (FIRST, "b"): {FINITE, NAN},
                  (FIRST, "r"): {FINITE, NAN}}
BACKWARD_PATTERNS = ("ALL", "X", "PAR", "BIAS")
TENSOR_OF = {"x": "x", "w": "weight", "b": "bias", "r": "residual"}


def conv_fixture(case, where):
    """-> {"planted": {x, w, b, r, cot}, "sanitised": {...}, "geom": (k, relu)}; CPU tensors: x, r, cot f16 NCHW-shaped,
    w / b f32 holding f16-exact values.  where = "x" | "w" | "b" | "r" (forward plants) or "cot" (backward plants)"""
    k, B, C, O, H, W, relu, res, plants = CONV_CASES[case]
    x = _randn((B, C, H, W), 1)
    w = _randn((O, C, k, k), 2, 0.05).float()
    b = _randn((O,), 3, 0.5).float()
    r = _randn((B, O, H, W), 4) if res else None
    cot = _randn((B, O, H, W), 5)
    if where == "x":
        for bi, c, y, xx, v in plants:
            x[bi, c, y, xx] = v
    elif where == "w":
        w[5, 9, k // 2, k // 2] = NANV
    elif where == "b":
        b[7] = NANV
    elif where == "r":
        r[B - 1, 20, H - 1, W - 1] = NANV
    elif where == "cot":
        # a finite forward on x >= 0 with many exact zeros (inf * 0 occurs in the weight gradient); the cotangent carries
        # +inf at (0, W - 1), -inf in the middle and NaN at (H - 1, 0), each in the out channel whose float64
        # pre-activation is the largest there (the ReLU passes it whatever the rounding)
        x = torch.relu(x)
        pre = conv_reference(dict(x=x, w=w, b=b, r=r, cot=cot), k, relu)[1]
        for bi, y, xx, v in ((0, 0, W - 1, INF), (B - 1, H // 2, W // 2, -INF), (B - 1, H - 1, 0, NANV)):
            cot[bi, int(pre[bi, :, y, xx].argmax()), y, xx] = v
    else:
        raise KeyError(where)
    p = dict(x=x, w=w, b=b, r=r, cot=cot)
    return {"planted": p, "sanitised": {n: sanitised(t) for n, t in p.items()}, "geom": (k, relu)}


def conv_reference(t, k, relu, mask=None):
    """float64 on the CPU: relu?(conv(x) + b (+ r)) and the gradients of <out, cot> -> ({out, x, weight, bias, residual},
    pre-activation).  The ReLU SELECTS (torch.where, never a product with a 0 / 1 mask) by torch's rule: an entry passes,
    forward and backward, unless pre <= 0, so it passes at NaN.  mask (bool, the shape of out): the decisions to take at
    the entries whose float64 pre-activation is finite (production's out > 0, as test_gpu_train_conv.reference does)."""
    x64, w64, b64 = (t[n].detach().to("cpu", F64).requires_grad_(True) for n in ("x", "w", "b"))
    r64 = None if t["r"] is None else t["r"].detach().to("cpu", F64).requires_grad_(True)
    with torch.enable_grad():
        pre = F.conv2d(x64, w64, b64, 1, k // 2)
        if r64 is not None:
            pre = pre + r64
        y = pre
        if relu:
            keep = ~(pre.detach() <= 0)
            if mask is not None:
                keep = torch.where(torch.isfinite(pre.detach()), mask.to("cpu"), keep)
            y = torch.where(keep, pre, torch.zeros_like(pre))
        y.backward(t["cot"].detach().to("cpu", F64))
    return {"out": y.detach(), "x": x64.grad, "weight": w64.grad, "bias": b64.grad,
            "residual": None if r64 is None else r64.grad}, pre.detach()


# ----------------------------------------------------------------------------- the chain: two layers, loss, update
CHAIN_PIXEL, CHAIN_CHANNELS, CHAIN_VALUE = (0, 4, 10), (5, 40), 60000.0


def chain_fixture(overflow):
    """layer 1: 3x3 64 -> 64 + ReLU, its weights on CHAIN_CHANNELS are 1.0; layer 2: 1x1 64 -> 64 + ReLU.  With `overflow`
    the two channels hold 60 000 at one pixel: every layer-1 pre-activation in its 3 x 3 neighbourhood is >= 1.2e5, 1.8 x
    f16's largest finite value, and leaves layer 1 as +inf; layer 2 sums inf * w over weights of both signs: NaN."""
    x = _randn((2, 64, 9, 21), 21)
    w1 = _randn((64, 64, 3, 3), 22, 0.05).float()
    w1[:, list(CHAIN_CHANNELS)] = 1.0
    b1 = _randn((64,), 23, 0.5).float()
    w2 = _randn((64, 64, 1, 1), 24, 0.05).float()
    b2 = _randn((64,), 25, 0.5).float()
    cot = _randn((2, 64, 9, 21), 26, 1.0 / 64)
    bi, y, xx = CHAIN_PIXEL
    for c in CHAIN_CHANNELS:
        x[bi, c, y, xx] = CHAIN_VALUE if overflow else 1.0
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, cot=cot)


def chain_reference(f):
    """float64 layer-1 pre-activation, and what the f16 network holds after each layer: (pre1, out1 as f16 -> f64, out2)"""
    pre1 = F.conv2d(f["x"].to(F64), f["w1"].to(F64), f["b1"].to(F64), 1, 1)
    out1 = torch.relu(pre1).to(F16).to(F64)                              # f16 storage: > 65504 + half an ulp becomes +inf
    pre2 = F.conv2d(out1, f["w2"].to(F64), f["b2"].to(F64))
    return pre1, out1, torch.where(pre2 <= 0, torch.zeros_like(pre2), pre2)


# ----------------------------------------------------------------------------- orientation pooling
POOL_SHAPE = (2, 32, 5, 7)                      # 4 groups of 8 orientations


def pool_fixture():
    """-> (x f32 [2, 32, 5, 7] with f16-exact values, cotangent [2, 4, 5, 7]).  Group g holds channels 8 g .. 8 g + 7."""
    x = _randn(POOL_SHAPE, 31).float()
    go = _randn((POOL_SHAPE[0], POOL_SHAPE[1] // 8) + POOL_SHAPE[2:], 32).float()
    x[0, 0 * 8 + 0, 0, 0] = NANV                  # NaN at orientation 0, 3, 7 of different groups
    x[0, 1 * 8 + 3, 1, 2] = NANV
    x[1, 2 * 8 + 7, 4, 6] = NANV
    x[1, 3 * 8 + 2, 2, 3] = NANV                  # a NaN next to a larger finite value at a later orientation
    x[1, 3 * 8 + 5, 2, 3] = 100.0
    x[0, 2 * 8 + 4, 3, 3] = NANV                  # two NaNs in one group: the first one is the maximum
    x[0, 2 * 8 + 6, 3, 3] = NANV
    x[0, 1 * 8 + 6, 4, 0] = INF                   # +inf wins
    x[1, 0 * 8 + 1, 0, 5] = -INF                  # -inf never wins against finite values
    x[1, 1 * 8:2 * 8, 3, 1] = -INF                # a whole group of -inf: orientation 0
    x[0, 3 * 8 + 1, 2, 2] = INF                   # two +inf: the first
    x[0, 3 * 8 + 4, 2, 2] = INF
    x[1, 0 * 8 + 2, 4, 4] = INF                   # +inf, then a NaN: the NaN
    x[1, 0 * 8 + 6, 4, 4] = NANV
    return x, go


def pool_reference(x, go):
    """torch.max(dim) in float64 on the CPU -> (values, gradient, routed orientation)"""
    N, C, H, W = x.shape
    x64 = x.detach().to("cpu", F64).requires_grad_(True)
    with torch.enable_grad():
        v, i = x64.view(N, C // 8, 8, H, W).max(2)
        v.backward(go.detach().to("cpu", F64))
    return v.detach(), x64.grad, i


# ----------------------------------------------------------------------------- loss
def loss_reference(p6, ids, ts, offsets, fl_gamma=2.0, fl_alpha=0.5, smoothL1_beta=1.0 / 9.0, FPN_balance=(1.0,) * 5,
                   reg_balance=1.0, odm_balance=1.0):
    """test_gpu_loss.ref_loss64 with SELECTION instead of products: the reference picks the valid anchors and the positives
    by index (models/head.py:586-638), so a map entry of an ignored anchor, or a delta of a negative, takes no part in the
    value and gets an exact-zero gradient whatever it holds.  (A product with a 0 / 1 mask, or a torch.where around an
    expression of the whole map, turns a NaN there into a NaN loss or gradient.)  Runs where its inputs are."""
    B, C = p6[1][0].shape[0], p6[0][0].shape[1]
    dev = p6[0][0].device
    ts, offsets = ts.double(), offsets.long()
    items = []
    for m in range(2):
        cls_l, box_l, anc_l = p6[2 * m], p6[2 * m + 1], p6[4 + m]
        cls = torch.cat([c.double().permute(0, 2, 3, 1).reshape(B, -1, C) for c in cls_l], 1)
        box = torch.cat([b.double().permute(0, 2, 3, 1).reshape(B, -1, 5) for b in box_l], 1)
        anc = torch.cat([a.detach().double().reshape(-1, a.shape[-3] * a.shape[-2] if a.dim() == 4 else a.shape[0], 5)
                         .expand(B, -1, 5) for a in anc_l], 1)
        w = torch.cat([torch.full((c.shape[2] * c.shape[3],), float(FPN_balance[l]), dtype=F64, device=dev)
                       for l, c in enumerate(cls_l)])[None].expand(B, -1)
        idm = ids[m]
        pos, valid = idm >= 0, idm != -2
        row = (offsets[:B, None] + idm.clamp(min=0)).clamp(max=max(ts.shape[0] - 1, 0))
        gt = ts[row] if ts.shape[0] else torch.zeros(B, idm.shape[1], 7, dtype=F64, device=dev)
        t = torch.zeros(cls.shape, dtype=F64, device=dev)
        t.scatter_(2, gt[..., 1].long().clamp(0, C - 1)[..., None], 1.0)
        t = t * pos[..., None]
        cv, tv = cls[valid], t[valid]                                   # [valid anchors, C]
        p = torch.sigmoid(cv)
        bce = cv.clamp(min=0) - cv * tv + torch.log1p(torch.exp(-cv.abs()))
        p_t = tv * p + (1 - tv) * (1 - p)
        focal = bce * (tv * fl_alpha + (1 - tv) * (1 - fl_alpha)) * (1.0 - p_t) ** fl_gamma
        cls_sum = (focal.sum(-1) * w[valid]).sum()
        anc, gt = anc[pos], gt[pos]                                     # [positives, ...]
        ox, oy = gt[..., 2] - anc[..., 0], gt[..., 3] - anc[..., 1]
        ca, sa = torch.cos(anc[..., 4]), torch.sin(anc[..., 4])
        da = torch.remainder(gt[..., 6] - anc[..., 4] + math.pi / 4, math.pi) - math.pi / 4
        tgt = torch.stack([(ca * ox + sa * oy) / anc[..., 2], (-sa * ox + ca * oy) / anc[..., 3],
                           torch.log(gt[..., 4].clamp(min=1e-30) / anc[..., 2]),
                           torch.log(gt[..., 5].clamp(min=1e-30) / anc[..., 3]), da / math.pi], -1)
        d = (box[pos] - tgt.detach()).abs()
        sl1 = torch.where(d < smoothL1_beta, 0.5 * d * d / smoothL1_beta, d - 0.5 * smoothL1_beta)
        reg_sum = (sl1.sum(-1) * w[pos]).sum()
        n = max(int(pos.sum()), B)
        bal = odm_balance if m == 1 else 1.0
        items += [cls_sum / n * bal, reg_sum / n * reg_balance * bal]
    items = torch.stack(items)
    return items.sum().reshape(1), items


# scenario: (module, which map, which anchor kind, value, items that turn non-finite [fam_cls, fam_reg, odm_cls, odm_reg])
LOSS_SCENARIOS = {
    "nan_class_logit_of_a_positive": (0, "cls", "positive", NANV, (0,)),
    "nan_other_logit_of_a_positive": (1, "cls", "positive_other", NANV, (2,)),
    "nan_logit_of_a_negative": (0, "cls", "negative", NANV, (0,)),
    "nan_delta_of_a_positive": (0, "bbox", "positive", NANV, (1,)),
    "pinf_delta_of_a_positive": (1, "bbox", "positive", INF, (3,)),
    "ninf_delta_of_a_positive": (0, "bbox", "positive", -INF, (1,)),
    "nan_and_inf_that_do_not_enter": (0, "both", "outside", NANV, ()),
}


def loss_plants(name, ids, ts, offsets, shapes):
    """where the scenario's plants go, from the assignment alone -> [(list index 0..3 of fam_cls / fam_bbox / odm_cls /
    odm_bbox, level, (b, channel, y, x), value)] and the ids to use (one anchor of level 0 is set to ignored for the
    scenario that needs one).  ids [2, B, A] int64 CPU; shapes: [(H, W)] per level"""
    m, which, kind, value, _ = LOSS_SCENARIOS[name]
    ids = ids.clone()
    starts = [0]
    for h, w in shapes:
        starts.append(starts[-1] + h * w)

    def place(b, a):
        lvl = max(l for l in range(len(shapes)) if starts[l] <= a)
        pos = a - starts[lvl]
        return lvl, b, pos // shapes[lvl][1], pos % shapes[lvl][1]

    def first(mask):
        at = mask.nonzero()
        assert at.shape[0] > 0, name
        return int(at[0, 0]), int(at[0, 1])

    plants = []
    if kind in ("positive", "positive_other"):
        b, a = first(ids[m] >= 0)
        lvl, b, y, x = place(b, a)
        if which == "cls":
            c = int(ts[int(offsets[b]) + int(ids[m, b, a]), 1])
            plants.append((2 * m, lvl, (b, c if kind == "positive" else (c + 1) % 15, y, x), value))
        else:
            plants.append((2 * m + 1, lvl, (b, 2, y, x), value))
    elif kind == "negative":
        b, a = first(ids[m] == -1)
        lvl, b, y, x = place(b, a)
        plants.append((2 * m, lvl, (b, 4, y, x), value))
    else:
        b, a = first(ids[m] == -1)                       # a delta of a negative: NaN and inf
        lvl, b, y, x = place(b, a)
        plants += [(2 * m + 1, lvl, (b, 0, y, x), NANV), (2 * m + 1, lvl, (b, 3, y, x), INF)]
        for mm in range(2):                              # every map entry kind of an ignored anchor (the second negative)
            at = (ids[mm] == -1).nonzero()
            b, a = int(at[1, 0]), int(at[1, 1])
            ids[mm, b, a] = -2
            lvl, b, y, x = place(b, a)
            plants += [(2 * mm, lvl, (b, 1, y, x), NANV), (2 * mm, lvl, (b, 7, y, x), INF),
                       (2 * mm + 1, lvl, (b, 1, y, x), NANV), (2 * mm + 1, lvl, (b, 4, y, x), -INF)]
    return plants, ids


# ----------------------------------------------------------------------------- AlignConv (differentiable route)
# name: (dtype, C, O); the map is ragged: 2 x C x 7 x 11, stride 8
ALIGN_CASES = {"f16_64to64": (F16, 64, 64), "f32_32to64": (F32, 32, 64)}
ALIGN_HW, ALIGN_STRIDE = (7, 11), 8
# NaN and +inf in x at the (0, 0) corner pixel and at an interior pixel, both ways round; a NaN in one filter entry
ALIGN_PLANTS = {"nan_corner_inf_interior": [(0, 3, 0, 0, NANV), (1, 9, 3, 5, INF)],
                "inf_corner_nan_interior": [(0, 3, 0, 0, INF), (1, 9, 3, 5, NANV)],
                "nan_filter": "w"}


def align_anchors(B, H, W, stride, seed):
    """grid anchors (side 4 strides) moved by N(0, 3 px), sides scaled by exp(N(0, 0.2)), angles in [-0.7, 2.3): the taps
    of border positions fall outside the image.  Positions with a sampling coordinate within 2e-3 of an integer are moved
    until none is left (a zero bilinear weight is otherwise legitimately ambiguous)."""
    from oracle import twin64 as T
    from oracle.dcn64 import sample_points
    g = _gen(seed)
    a = torch.zeros(B, H, W, 5)
    a[..., 0] = (torch.arange(W).float() * stride + 0.5 * (stride - 1)).view(1, 1, W)
    a[..., 1] = (torch.arange(H).float() * stride + 0.5 * (stride - 1)).view(1, H, 1)
    a[..., :2] += torch.randn((B, H, W, 2), generator=g) * 3
    a[..., 2:4] = 4.0 * stride * torch.exp(torch.randn((B, H, W, 2), generator=g) * 0.2)
    a[..., 4] = torch.rand((B, H, W), generator=g) * 3.0 - 0.7
    for _ in range(200):
        h, w = sample_points(T.align_offsets(a, stride, dtype=F32), F32)
        near = ((h - h.round()).abs() < 2e-3) | ((w - w.round()).abs() < 2e-3)
        bad = near.any(1)                                            # [B, H, W]
        if not bool(bad.any()):
            return a
        a[..., 0] += bad.float() * 0.137
        a[..., 1] += bad.float() * 0.071
    raise AssertionError("align_anchors: could not move every sampling point off the integers")


def align_fixture(case, plant):
    """-> {"planted": {x, w, cot}, "sanitised": {...}, "anchors": [B, H, W, 5] f32}; values exact in f16"""
    dtype, C, O = ALIGN_CASES[case]
    H, W = ALIGN_HW
    x = _randn((2, C, H, W), 41).float()
    w = _randn((O, C, 3, 3), 42, 0.05).float()
    cot = _randn((2, O, H, W), 43).float()
    what = ALIGN_PLANTS[plant]
    if what == "w":
        w[5, 9, 1, 2] = NANV
    else:
        for bi, c, y, xx, v in what:
            x[bi, c, y, xx] = v
    p = dict(x=x, w=w, cot=cot)
    return {"planted": p, "sanitised": {n: sanitised(t) for n, t in p.items()}, "anchors": align_anchors(2, H, W, ALIGN_STRIDE, 44)}


def align_points(anchors):
    """the sampling points (h, w) [B, 9, H, W] in float64, formed in float32 as every kernel forms them"""
    from oracle import twin64 as T
    from oracle.dcn64 import sample_points
    return sample_points(T.align_offsets(anchors, ALIGN_STRIDE, dtype=F32), F32)


def align_reference(t, anchors, mask=None, inf_is_nan=False):
    """float64 on the CPU: relu(deform_conv(x, offsets(anchors), w)) and the gradients of <out, cot> -> ({out, x, weight},
    pre-activation).  oracle.dcn64's geometry (band, floor, corners), but a corner outside the image is DROPPED
    (torch.where), never read at a clamped index and multiplied by a zero weight: the reference's kernel reads no such
    corner (deform_conv_cuda_kernel.cu:97-108).  The ReLU selects as in conv_reference.
    inf_is_nan pins the documented deviation of the default f32 forward (include/s2anet_hip.h, s2a_dcn_pack_weight: the
    operands are split into three bf16 planes, and inf - bf16(inf) is NaN): an infinite pre-activation counts as NaN,
    in the output and, since a NaN passes the ReLU's backward, in the mask."""
    from oracle.dcn64 import _corners
    h, wv = align_points(anchors)
    x64 = t["x"].detach().to("cpu", F64).requires_grad_(True)
    w64 = t["w"].detach().to("cpu", F64).requires_grad_(True)
    B, C, H, W = x64.shape
    O = w64.shape[0]
    with torch.enable_grad():
        outs = []
        for b in range(B):
            corners, _ = _corners(h[b], wv[b], H, W)
            xf = x64[b].reshape(C, H * W)
            cols = 0
            for idx, wt, ok in corners:
                v = torch.where(ok.reshape(1, -1), xf[:, idx.reshape(-1)], torch.zeros((), dtype=F64))
                cols = cols + v * wt.reshape(1, -1)
            outs.append((w64.reshape(O, C * 9) @ cols.reshape(C * 9, H * W)).view(O, H, W))
        pre = torch.stack(outs)
        keep = ~(pre.detach() <= 0)
        if mask is not None:
            keep = torch.where(torch.isfinite(pre.detach()), mask.to("cpu"), keep)
        if inf_is_nan:
            keep = keep | torch.isinf(pre.detach())
        y = torch.where(keep, pre, torch.zeros_like(pre))
        y.backward(t["cot"].detach().to("cpu", F64))
    out = y.detach()
    if inf_is_nan:
        out = torch.where(torch.isinf(pre.detach()), torch.full_like(out, NANV), out)
    return {"out": out, "x": x64.grad, "weight": w64.grad}, pre.detach()
