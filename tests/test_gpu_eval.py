"""GPU: all-class DOTA Task-1 evaluation on the device (s2a_eval_task1, evaluate_task1, Task1Evaluator) against the
reference script's golden curves, the CPU oracle's voc_eval restatement per class, mark_tp_fp, and itself (padding,
two runs, HIP-graph replay, the detector's own output).

One CPU reference serves every comparison (cpu_reference): per class the rows are ordered by
np.argsort(-score, kind="stable") -- with distinct scores that is the order of oracle.voc_eval_arrays' own argsort --
and handed to oracle.voc_eval_arrays with surrogate scores n, n - 1, ..., 1 in that order, so the oracle's curves,
ovmax and argmax come back in the order the device uses.  The max-F1 point is val.py:357-386 applied in NumPy to the
oracle's curves.

Bounds: everything is compared bit for bit except the area-rule AP, which the device sums in another order than
np.sum: D_c terms of at most 1 with partial sums of at most 1, each addition off by at most 2^-53 in either order, so
|difference| <= D_c * 2^-52.
"""

import numpy as np
import pytest
import torch

import oracle
from conftest import golden, rand_rboxes

pytestmark = pytest.mark.gpu

# the sizes at which the kernels of eval_ops.hip change path
MATCH_BLOCK = 128        # k_eval_match: rows of the (class, image) order per workgroup (kPolyThreads)
GT_CHUNK = 64            # k_eval_match: ground truths of a group staged in LDS at a time (kEvalChunk)
SCAN_TILE = 1024         # k_eval_mark / k_eval_cum: rank positions per workgroup (kEvalScanTile)
CLASS_TILE = 4096        # k_eval_class: positions per step of the suffix maximum / area sum / F1 arg-max (kEvalClassTile)
TILE_SCAN_STEP = 1024    # k_eval_tile_scan: tile totals per step of its one workgroup (1024 * SCAN_TILE = 2^20 rows)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ------------------------------------------------------------------------------------------------ data + reference
KEYS = ("dp", "ds", "dl", "di", "gp", "gl", "gi", "gd")


def polys_of(rng, n, span):
    return np.round(oracle.rboxes_to_polys(rand_rboxes(rng, n, span=span)), 1) if n else np.zeros((0, 8))


def make_data(rng, C, I, n_gt, n_fa, dup=(0, 3), span=500.0, difficult=0.2, det_sizes=None, gt_groups=None):
    """ground truths of random class / image; detections = jittered ground truths (dup[0]..dup[1]-1 each) + n_fa false
    alarms, distinct scores; rows shuffled.  det_sizes {class: exact number of detections}; gt_groups [(class, image,
    n)]: extra ground-truth groups of exactly n boxes."""
    gp = polys_of(rng, n_gt, span)
    gl, gi = rng.integers(0, C, n_gt), rng.integers(0, I, n_gt)
    for c, im, n in gt_groups or ():
        keep = ~((gl == c) & (gi == im))
        gp, gl, gi = gp[keep], gl[keep], gi[keep]
        gp = np.concatenate([gp, polys_of(rng, n, span)])
        gl, gi = np.concatenate([gl, np.full(n, c)]), np.concatenate([gi, np.full(n, im)])
    G = gl.size
    rep = rng.integers(dup[0], dup[1], G)
    src = np.repeat(np.arange(G), rep)
    dp = np.round(gp[src] + rng.normal(0, 2.5, (src.size, 8)), 1)
    dl, di = gl[src], gi[src]
    fa = polys_of(rng, n_fa, span)
    dp = np.concatenate([dp, fa])
    dl, di = np.concatenate([dl, rng.integers(0, C, n_fa)]), np.concatenate([di, rng.integers(0, I, n_fa)])
    if det_sizes is not None:
        parts = []
        for c in range(C):
            at = np.nonzero(dl == c)[0]
            want = det_sizes.get(c, at.size)
            if at.size < want:                                     # more false alarms of that class
                extra = want - at.size
                dp = np.concatenate([dp, polys_of(rng, extra, span)])
                dl, di = np.concatenate([dl, np.full(extra, c)]), np.concatenate([di, rng.integers(0, I, extra)])
                at = np.nonzero(dl == c)[0]
            parts.append(rng.permutation(at)[:want])
        keep = np.concatenate(parts)
        dp, dl, di = dp[keep], dl[keep], di[keep]
    D = dl.size
    sh, gsh = rng.permutation(D), rng.permutation(G)
    return dict(dp=dp[sh], ds=(rng.permutation(D) + 1.0) / (D + 1.0), dl=dl[sh].astype(np.int32), di=di[sh].astype(np.int32),
                gp=gp[gsh], gl=gl[gsh].astype(np.int32), gi=gi[gsh].astype(np.int32),
                gd=(rng.random(G) < difficult).astype(np.uint8)[gsh])


def max_f1_point(rec, prec, sorted_scores):
    """val.py:357-386"""
    f1 = 2 * rec * prec / (rec + prec + 1e-16)
    i = f1.argmax()
    return dict(precision=prec[i], recall=rec[i], f1=f1[i], conf=sorted_scores[i], num_det_at_f1=i + 1)


def cpu_reference(data, C, I, ovthresh=0.5, is_filter_difficult=True, use_07_metric=True):
    out = []
    for c in range(C):
        d, g = np.nonzero(data["dl"] == c)[0], np.nonzero(data["gl"] == c)[0]
        order = np.argsort(-data["ds"][d], kind="stable")
        sur = np.empty(d.size)
        sur[order] = np.arange(d.size, 0, -1)
        diff = data["gd"][g].astype(bool)
        r = dict(order=d[order], ndet=d.size, npos=int((~diff).sum()) if is_filter_difficult else g.size)
        if d.size:
            with np.errstate(all="ignore"):
                rec, prec, ap, _, (ov, am) = oracle.voc_eval_arrays(
                    data["dp"][d], sur, data["di"][d], data["gp"][g], data["gi"][g], data["gd"][g], I, ovthresh=ovthresh,
                    is_filter_difficult=is_filter_difficult, use_07_metric=use_07_metric)
            r.update(rec=rec, prec=prec, ap=ap, ovmax=ov, argmax=np.where(am >= 0, g[np.maximum(am, 0)] if g.size else -1, -1))
            if r["npos"]:
                r.update(max_f1_point(rec, prec, data["ds"][d][order]))
        out.append(r)
    return out


def run_device(data, C, I, **kw):
    from s2anet_amd.evaluate import evaluate_task1
    res = evaluate_task1(*(cu(data[k]) for k in KEYS), C, I, curves=True, **kw)
    torch.cuda.synchronize()
    return res


def host(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ("ap", "precision", "recall", "f1", "conf", "num_det_at_f1", "npos", "ndet", "valid")}
    out.update({k: v.cpu().numpy() for k, v in res.curves.items()})
    return out


def assert_equals_reference(h, ref, use_07_metric=True, tag=""):
    seg = h["seg_start"]
    assert seg[0] == 0 and seg[-1] == sum(r["ndet"] for r in ref), tag
    n_real = seg[-1]
    assert (h["order"][n_real:] == -1).all() and (h["argmax"][n_real:] == -1).all(), tag
    for k in ("ovmax", "tp_cum", "fp_cum", "rec", "prec"):
        assert (h[k][n_real:] == 0).all(), (tag, k)
    for c, r in enumerate(ref):
        s, e = seg[c], seg[c + 1]
        assert e - s == r["ndet"] == h["ndet"][c] and h["npos"][c] == r["npos"], (tag, c)
        assert h["valid"][c] == (1 if r["npos"] else 0), (tag, c)
        assert np.array_equal(h["order"][s:e], r["order"]), (tag, c)
        if r["ndet"]:
            assert np.array_equal(h["ovmax"][s:e], r["ovmax"]) and np.array_equal(h["argmax"][s:e], r["argmax"]), (tag, c)
        if r["ndet"] == 0 or r["npos"] == 0:
            for k in ("ap", "precision", "recall", "f1", "conf", "num_det_at_f1"):
                assert h[k][c] == 0, (tag, c, k)
            continue
        assert np.array_equal(h["rec"][s:e], r["rec"]) and np.array_equal(h["prec"][s:e], r["prec"]), (tag, c)
        assert np.array_equal(h["tp_cum"][s:e], np.round(r["rec"] * r["npos"]).astype(np.int64)), (tag, c)
        if use_07_metric:
            assert h["ap"][c] == r["ap"], (tag, c, h["ap"][c], r["ap"])
        else:
            assert abs(h["ap"][c] - r["ap"]) <= r["ndet"] * 2.0 ** -52, (tag, c, h["ap"][c], r["ap"])
        for k in ("precision", "recall", "f1", "conf", "num_det_at_f1"):
            assert h[k][c] == r[k], (tag, c, k, h[k][c], r[k])


def interleave(rng, sizes):
    """a random merge of blocks that keeps the order inside every block -> for each block its positions"""
    tags = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(tags)
    return [np.nonzero(tags == b)[0] for b in range(len(sizes))]


# ------------------------------------------------------------------------------------------------ 1. reference fixture
def test_golden_class_among_decoys(rng):
    """tests/golden/voc_eval.npz (the reference script's own voc_eval) as class 3 of 5; the other classes hold the SAME
    polygons on the same images (detections and ground truths), which must not leak into class 3"""
    from test_oracle_pinned import VOC_CASES
    g = golden("voc_eval.npz")
    C, I, n_d, n_g = 5, int(g["num_images"]), g["det_scores"].size, g["gt_image"].size
    others = [c for c in range(C) if c != 3]
    dpos, gpos = interleave(rng, [n_d] * 5), interleave(rng, [n_g] * 5)
    data = dict(dp=np.zeros((5 * n_d, 8)), ds=np.zeros(5 * n_d), dl=np.zeros(5 * n_d, np.int32), di=np.zeros(5 * n_d, np.int32),
                gp=np.zeros((5 * n_g, 8)), gl=np.zeros(5 * n_g, np.int32), gi=np.zeros(5 * n_g, np.int32), gd=np.zeros(5 * n_g, np.uint8))
    for b, c in enumerate([3] + others):
        decoy = c != 3
        data["dp"][dpos[b]] = g["det_polys"] + (rng.normal(0, 1.0, (n_d, 8)) if decoy else 0)
        data["ds"][dpos[b]] = rng.permutation(g["det_scores"]) if decoy else g["det_scores"]
        data["dl"][dpos[b]], data["di"][dpos[b]] = c, g["det_image"]
        data["gp"][gpos[b]] = g["gt_polys"]
        data["gl"][gpos[b]], data["gi"][gpos[b]] = c, g["gt_image"]
        data["gd"][gpos[b]] = rng.permutation(g["gt_difficult"]) if decoy else g["gt_difficult"]
    for tag, kw in VOC_CASES:
        kw = dict(dict(use_07_metric=False), **kw)
        h = host(run_device(data, C, I, **kw))
        s, e = h["seg_start"][3], h["seg_start"][4]
        assert e - s == n_d
        assert np.array_equal(h["rec"][s:e], g["rec_" + tag]) and np.array_equal(h["prec"][s:e], g["prec_" + tag]), tag
        print(tag, "ap", h["ap"][3], "golden", float(g["ap_" + tag]), "diff", h["ap"][3] - float(g["ap_" + tag]))
        if kw["use_07_metric"]:
            assert h["ap"][3] == float(g["ap_" + tag]), tag
        else:
            assert abs(h["ap"][3] - float(g["ap_" + tag])) <= n_d * 2.0 ** -52, tag
        assert np.array_equal(h["order"][s:e], dpos[0][np.argsort(-g["det_scores"])]), tag


# ------------------------------------------------------------------------------------------------ 2. oracle, many classes
@pytest.fixture(scope="module")
def many_classes():
    rng = np.random.default_rng(20)
    C, I = 15, 40
    data = make_data(rng, C, I, n_gt=900, n_fa=3100, dup=(0, 3))
    keep = data["dl"] != 5                                          # class 5: ground truth but no detection
    for k in ("dp", "ds", "dl", "di"):
        data[k] = data[k][keep]
    keep = data["gl"] != 9                                          # class 9: detections but no ground truth
    for k in ("gp", "gl", "gi", "gd"):
        data[k] = data[k][keep]
    return data, C, I


@pytest.mark.parametrize("kw", [dict(), dict(use_07_metric=False), dict(is_filter_difficult=False), dict(ovthresh=0.7, use_07_metric=False)],
                         ids=["voc07", "area", "hard", "thr07_area"])
def test_many_classes_equal_oracle(many_classes, kw):
    data, C, I = many_classes
    assert 3500 < data["dl"].size < 4500 and 750 < data["gl"].size < 950 and 0.1 < data["gd"].mean() < 0.3
    ref = cpu_reference(data, C, I, **kw)
    assert ref[5]["ndet"] == 0 and ref[5]["npos"] > 0 and ref[9]["npos"] == 0 and ref[9]["ndet"] > 0
    res = run_device(data, C, I, **kw)
    h = host(res)
    assert_equals_reference(h, ref, kw.get("use_07_metric", True), str(kw))
    assert h["valid"][9] == 0 and h["valid"][5] == 1 and h["ap"][5] == 0 and h["num_det_at_f1"][5] == 0
    # the means of val.py:395-399 and the one host read
    (mp, mr, map50, conf), aps = res.summary()
    assert np.array_equal(aps, h["ap"]) and map50 == h["ap"].mean() and mp == h["precision"].mean()
    assert mr == h["recall"].mean() and conf == h["conf"].mean()
    for name, key in (("map50", "ap"), ("mp", "precision"), ("mr", "recall"), ("mf1", "f1"), ("mconf", "conf")):
        v = getattr(res, name)
        assert v.is_cuda and v.dim() == 0 and abs(float(v) - h[key].mean()) <= 1e-15


# ------------------------------------------------------------------------------------------------ 3. the claim under contention
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 4097])
def test_claim_under_contention(n):
    """one ground truth, n near-duplicate detections of it: exactly one TP, at the top rank, wherever the highest score
    sits in the input; a filtered difficult ground truth counts nothing, an unfiltered one counts one TP"""
    from s2anet_amd.evaluate import mark_tp_fp
    rng = np.random.default_rng(n)
    gt = np.round(oracle.rboxes_to_polys(rand_rboxes(rng, 1, span=300.0, lo=40.0)), 1)
    dp = np.round(gt + rng.normal(0, 0.5, (n, 8)), 2)
    for top in sorted({0, n - 1, min(64, n - 1)}):                   # first, last, at a wave boundary
        ds = (rng.permutation(n) + 1.0) / (n + 2.0)
        ds[top] = 1.0
        for difficult, filt in ((0, True), (1, True), (1, False)):
            data = dict(dp=dp, ds=ds, dl=np.zeros(n, np.int32), di=np.zeros(n, np.int32), gp=gt, gl=np.zeros(1, np.int32),
                        gi=np.zeros(1, np.int32), gd=np.full(1, difficult, np.uint8))
            h = host(run_device(data, 1, 1, is_filter_difficult=filt))
            tag = (n, top, difficult, filt)
            assert h["order"][0] == top and (h["ovmax"] > 0.5).all() and (h["argmax"] == 0).all(), tag
            tp, fp = mark_tp_fp(h["ovmax"], h["argmax"], data["gd"], 0.5, filt)
            assert np.array_equal(h["tp_cum"], np.cumsum(tp).astype(np.int64)), tag
            assert np.array_equal(h["fp_cum"], np.cumsum(fp).astype(np.int64)), tag
            if difficult and filt:
                assert h["tp_cum"][-1] == 0 and h["fp_cum"][-1] == 0 and h["valid"][0] == 0 and h["npos"][0] == 0, tag
            else:
                assert h["tp_cum"][0] == 1 and h["tp_cum"][-1] == 1 and h["fp_cum"][-1] == n - 1 and h["npos"][0] == 1, tag
                assert h["num_det_at_f1"][0] == 1 and h["precision"][0] == 1.0 and h["recall"][0] == 1.0 and h["conf"][0] == 1.0, tag


# ------------------------------------------------------------------------------------------------ 4. segment and tile edges
def test_segment_and_tile_edges():
    """class sizes 0, 1 and every tile size minus one, exact, plus one (SCAN_TILE, CLASS_TILE, MATCH_BLOCK), and two
    CLASS_TILE + 1 for the carries across steps; classes 1 and 2 (1 + 1023 rows) meet inside the first scan tile, and so do
    most neighbours behind them; ground-truth groups of GT_CHUNK - 1, GT_CHUNK, GT_CHUNK + 1 and 2 * GT_CHUNK + 1"""
    sizes = [0, 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, MATCH_BLOCK - 1, MATCH_BLOCK, MATCH_BLOCK + 1, CLASS_TILE - 1, CLASS_TILE,
             CLASS_TILE + 1, 2 * CLASS_TILE + 1, 0, 3]
    C, I = len(sizes), 6
    groups = [(2, 0, GT_CHUNK - 1), (3, 1, GT_CHUNK), (4, 2, GT_CHUNK + 1), (8, 3, 2 * GT_CHUNK + 1), (6, 4, GT_CHUNK), (11, 5, GT_CHUNK + 1)]
    rng = np.random.default_rng(4)
    data = make_data(rng, C, I, n_gt=700, n_fa=1500, dup=(1, 4), span=420.0, det_sizes=dict(enumerate(sizes)), gt_groups=groups)
    for c, n in enumerate(sizes):
        assert (data["dl"] == c).sum() == n
    for c, im, n in groups:
        assert ((data["gl"] == c) & (data["gi"] == im)).sum() == n
    for kw in (dict(), dict(use_07_metric=False, is_filter_difficult=False)):
        assert_equals_reference(host(run_device(data, C, I, **kw)), cpu_reference(data, C, I, **kw), kw.get("use_07_metric", True), str(kw))


def test_tile_scan_carry_past_its_step():
    """more than TILE_SCAN_STEP * SCAN_TILE = 2^20 rows, so that k_eval_tile_scan carries from one step of tile totals to the
    next: no polygon overlaps any ground truth (every detection is a false alarm), the counts are known in closed form"""
    D = TILE_SCAN_STEP * SCAN_TILE + SCAN_TILE + 1
    n0 = TILE_SCAN_STEP * SCAN_TILE - 3                              # class 0 ends three rows in front of the step's edge
    from s2anet_amd.evaluate import evaluate_task1
    g = torch.Generator(device=dev()).manual_seed(3)
    xy = torch.rand((D, 2), generator=g, device=dev(), dtype=torch.float64) * 400
    dp = torch.cat([xy, xy + torch.tensor([9.0, 0.0], device=dev()), xy + 9.0, xy + torch.tensor([0.0, 9.0], device=dev())], 1)
    ds = torch.rand(D, generator=g, device=dev(), dtype=torch.float64)
    dl = (torch.arange(D, device=dev()) >= n0).to(torch.int32)
    dl = dl[torch.randperm(D, generator=g, device=dev())]
    di = torch.zeros(D, dtype=torch.int32, device=dev())
    gp = torch.tensor([[5000.0, 5000, 5010, 5000, 5010, 5010, 5000, 5010]] * 2, dtype=torch.float64, device=dev())
    res = evaluate_task1(dp, ds, dl, di, gp, torch.tensor([0, 1], dtype=torch.int32, device=dev()),
                         torch.zeros(2, dtype=torch.int32, device=dev()), torch.zeros(2, dtype=torch.uint8, device=dev()), 2, 1, curves=True)
    seg = res.curves["seg_start"].tolist()
    assert seg == [0, n0, D]
    want = torch.cat([torch.arange(1, n0 + 1, device=dev()), torch.arange(1, D - n0 + 1, device=dev())])
    assert torch.equal(res.curves["fp_cum"], want) and int(res.curves["tp_cum"].max()) == 0
    assert res.ndet.tolist() == [n0, D - n0] and res.ap.tolist() == [0.0, 0.0] and res.valid.tolist() == [1, 1]
    order = res.curves["order"]
    for c, (s, e) in enumerate(((0, n0), (n0, D))):
        assert bool((dl[order[s:e]] == c).all()) and bool((ds[order[s:e]][1:] <= ds[order[s:e]][:-1]).all())


# ------------------------------------------------------------------------------------------------ 5. ties
def test_score_ties_follow_stable_argsort(rng):
    """blocks of equal scores: the order is np.argsort(-s, kind="stable") per class (ties by ascending input row);
    -0.0 and +0.0 are equal"""
    C, I = 4, 5
    data = make_data(rng, C, I, n_gt=150, n_fa=500, dup=(1, 4), span=300.0)
    D = data["ds"].size
    data["ds"] = rng.choice(np.array([0.9, 0.5, 0.25, 0.0, -0.0, -0.5]), D)
    assert (np.signbit(data["ds"]) & (data["ds"] == 0)).sum() > 20 and (~np.signbit(data["ds"]) & (data["ds"] == 0)).sum() > 20
    for kw in (dict(), dict(use_07_metric=False)):
        assert_equals_reference(host(run_device(data, C, I, **kw)), cpu_reference(data, C, I, **kw), kw.get("use_07_metric", True), str(kw))


# ------------------------------------------------------------------------------------------------ 6. padding
def guarded_alloc(store):
    sentinel = {torch.float64: 12345.678, torch.int64: -777, torch.uint8: 0xA5}

    def alloc(name, n, dtype):
        buf = torch.full((n + 32,), sentinel[dtype], dtype=dtype, device=dev())
        store[name] = (buf, sentinel[dtype], n)
        return buf[16:16 + n]
    return alloc


def test_padding_rows_are_ignored(rng):
    """the same rows interleaved with padding (label -1, label == num_classes, image -1, image == num_images; NaN polygons
    and scores) on both sides: every output bit-equal to the compacted input's, indices mapped; guard words around every
    output untouched; two runs bit-equal"""
    from s2anet_amd.evaluate import evaluate_task1
    C, I = 6, 7
    data = make_data(rng, C, I, n_gt=300, n_fa=900, dup=(0, 3), span=350.0)
    D, G = data["ds"].size, data["gl"].size
    n_pd, n_pg = 700, 260
    dpos, gpos = interleave(rng, [D, n_pd]), interleave(rng, [G, n_pg])
    pad = dict(dp=np.full((D + n_pd, 8), np.nan), ds=np.full(D + n_pd, np.nan), dl=np.zeros(D + n_pd, np.int32), di=np.zeros(D + n_pd, np.int32),
               gp=np.full((G + n_pg, 8), np.nan), gl=np.zeros(G + n_pg, np.int32), gi=np.zeros(G + n_pg, np.int32),
               gd=rng.integers(0, 2, G + n_pg).astype(np.uint8))
    for side, pos, n_p in (("d", dpos, n_pd), ("g", gpos, n_pg)):
        kind = np.arange(n_p) % 4                                   # four ways of being padding
        lab = np.select([kind == 0, kind == 1], [-1, C], rng.integers(0, C, n_p))
        img = np.select([kind == 2, kind == 3], [-1, I], rng.integers(0, I, n_p))
        pad[side + "l"][pos[1]], pad[side + "i"][pos[1]] = lab, img
        for k in ("p", "s", "l", "i") if side == "d" else ("p", "l", "i", "d"):
            pad[side + k][pos[0]] = data[side + k]
    want = host(run_device(data, C, I))
    store = {}
    runs = []
    for _ in range(2):
        res = evaluate_task1(*(cu(pad[k]) for k in KEYS), C, I, curves=True, alloc=guarded_alloc(store))
        torch.cuda.synchronize()
        assert len(store) == 9 + 8
        for name, (buf, s, n) in store.items():
            assert bool((buf[:16] == s).all()) and bool((buf[16 + n:] == s).all()), name
        runs.append(host(res))
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    got = runs[0]
    for k in ("ap", "precision", "recall", "f1", "conf", "num_det_at_f1", "npos", "ndet", "valid", "seg_start"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("ovmax", "tp_cum", "fp_cum", "rec", "prec"):
        assert np.array_equal(got[k][:D], want[k]) and (got[k][D:] == 0).all(), k
    assert np.array_equal(got["order"][:D], dpos[0][want["order"]]) and (got["order"][D:] == -1).all()
    assert np.array_equal(got["argmax"][:D], np.where(want["argmax"] >= 0, gpos[0][np.maximum(want["argmax"], 0)], -1))
    assert (got["argmax"][D:] == -1).all()


# ------------------------------------------------------------------------------------------------ 7. graph
def fill(ev, data):
    ev.reset()
    ev.add_ground_truth(cu(data["gp"]), cu(data["gl"]), cu(data["gi"]), cu(data["gd"]))
    half = data["ds"].size // 2                                      # two blocks: the second lands behind the first
    for a, b in ((0, half), (half, data["ds"].size)):
        ev.add_polygons(cu(data["dp"][a:b]), cu(data["ds"][a:b]), cu(data["dl"][a:b]), cu(data["di"][a:b]))


def flat(res):
    return [getattr(res, k) for k in ("ap", "precision", "recall", "f1", "conf", "num_det_at_f1", "npos", "ndet", "valid")] + \
        [res.curves[k] for k in sorted(res.curves)]


def test_compute_hip_graph_replay_equals_eager():
    """Task1Evaluator.compute captured once on a side stream (warm-up outside the capture) and replayed on three further
    table contents -- one of them with class 2 emptied -- is bit-equal to an eager call on the same contents"""
    from s2anet_amd.evaluate import Task1Evaluator
    C, I = 6, 9
    contents = [make_data(np.random.default_rng(70 + k), C, I, n_gt=200 + 40 * k, n_fa=500 + 90 * k, span=350.0) for k in range(4)]
    keep = contents[2]["dl"] != 2
    contents[2] = dict(contents[2], dp=contents[2]["dp"][keep], ds=contents[2]["ds"][keep], dl=contents[2]["dl"][keep], di=contents[2]["di"][keep])
    assert (contents[1]["dl"] == 2).any() and not (contents[2]["dl"] == 2).any()
    ev, ev_eager = (Task1Evaluator(C, 1500, 500, I, dev()) for _ in range(2))
    eager = []
    for d in contents:
        fill(ev_eager, d)
        eager.append([t.clone() for t in flat(ev_eager.compute(curves=True))])
    fill(ev, contents[0])
    side = torch.cuda.Stream(device=dev())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.compute(curves=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_out = flat(ev.compute(curves=True))
    for k in (1, 2, 3):
        fill(ev, contents[k])
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(static_out, eager[k]):
            assert torch.equal(got, ref), k
    assert int(eager[1][7][2]) > 0 and int(eager[2][7][2]) == 0 and float(eager[2][0][2]) == 0.0     # ndet / ap of class 2
    assert not torch.equal(eager[1][0], eager[3][0])


# ------------------------------------------------------------------------------------------------ 8. from the detector
def host_route(polys, scores, labels, image, gp, gl, gi, gd, C, I):
    """rbox_to_poly polygons -> voc_eval_arrays per class (the existing route): VOC07 ap and curve length per class.
    The synthetic detector's float32 scores tie heavily (measured: 999 rows of one class with 25 distinct values) and
    voc_eval_arrays orders by np.argsort(-s), which is not stable: among equal scores its order, and with it its AP, is
    arbitrary (measured: 0.3653 against 0.3670 for the stable order).  So the route is given the ranks of the stable
    order as confidences -- AP depends on the order only -- which is the tie rule the device documents."""
    from s2anet_amd.evaluate import voc_eval_arrays
    aps, lens = np.zeros(C), np.zeros(C, np.int64)
    for c in range(C):
        d, g = np.nonzero(labels == c)[0], gl == c
        if d.size and (g & (gd == 0)).any():
            conf = np.empty(d.size)
            conf[np.argsort(-scores[d], kind="stable")] = np.arange(d.size, 0, -1)
            rec, _, ap, _ = voc_eval_arrays(polys[d], conf, image[d], gp[g], gi[g], gd[g], I, use_07_metric=True, device=dev())
            aps[c], lens[c] = ap, rec.size
        else:
            lens[c] = d.size
    return aps, lens


def test_from_the_detector():
    """detect() on two chips of the small synthetic network -> add_detections -> compute, against the host route on the same
    rows; then the two chips merged as one scene -> add_merged -> compute, against the host route on the merged rows"""
    from s2anet_amd.detector import build_synthetic_detector
    from s2anet_amd.evaluate import Task1Evaluator
    from s2anet_amd.formats import rbox_to_poly
    from s2anet_amd.scene import merge_detections
    m = build_synthetic_detector(device=dev())
    m.head.odm_cls_head.bias.data.fill_(-2.0)
    m.head.odm_cls_head.weight.data.mul_(20.0)
    g = torch.Generator().manual_seed(8)
    imgs = torch.randint(0, 256, (2, 3, 256, 256), dtype=torch.uint8, generator=g).to(dev())
    dets, labels, counts = m.detect(imgs)[:3]
    B, K = labels.shape
    C = m.head.num_classes
    rng = np.random.default_rng(8)
    polys = rbox_to_poly(dets.reshape(-1, 6).contiguous()).cpu().numpy().astype(np.float64)
    scores = dets[..., 5].reshape(-1).cpu().numpy().astype(np.float64)
    lab = labels.reshape(-1).cpu().numpy()
    image = np.repeat(np.arange(B), K)
    valid = (np.arange(K)[None, :] < counts.cpu().numpy()[:, None]).reshape(-1) & (lab >= 0)
    assert valid.sum() > 50
    pick = np.nonzero(valid)[0][::3]                                # ground truth: a jittered subset of its own detections
    gp = polys[pick] + rng.normal(0, 1.0, (pick.size, 8))
    gl, gi, gd = lab[pick].astype(np.int32), image[pick].astype(np.int32), (rng.random(pick.size) < 0.2).astype(np.uint8)
    ev = Task1Evaluator(C, 2 * B * K, 2 * pick.size, 4, dev())
    ev.add_ground_truth(gp, gl, gi, gd)
    assert ev.add_detections(dets, labels, counts, [0, 1]) == 0 and ev.num_dets == B * K
    res = ev.compute()
    aps, lens = host_route(polys[valid], scores[valid], lab[valid], image[valid], gp, gl, gi, gd, C, 4)
    print("detector: ap", res.ap.tolist())
    assert np.array_equal(res.ap.cpu().numpy(), aps) and np.array_equal(res.ndet.cpu().numpy(), lens)
    assert aps.max() > 0
    # the same two chips as one scene (the second 200 px to the right), merged per class
    origins = np.asarray([[0, 0], [200, 0]], np.int32)
    merged = merge_detections(dets, labels, counts, origins, num_classes=C)
    gp2 = gp.copy()
    gp2[:, 0::2] += origins[gi, 0][:, None]
    ev.reset()
    ev.add_ground_truth(cu(gp2), cu(gl), 0, cu(gd))
    assert ev.add_merged(merged, 0) == 0 and ev.num_dets == merged.scores.shape[0]
    res2 = ev.compute()
    mp, ms, ml = merged.polys.cpu().numpy(), merged.scores.cpu().numpy(), merged.labels.cpu().numpy()
    aps2, lens2 = host_route(mp, ms, ml, np.zeros(ml.size, np.int64), gp2, gl, np.zeros(gl.size, np.int32), gd, C, 4)
    assert np.array_equal(res2.ap.cpu().numpy(), aps2) and np.array_equal(res2.ndet.cpu().numpy(), lens2)
