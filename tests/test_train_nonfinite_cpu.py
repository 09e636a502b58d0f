"""Side conditions of the fixtures of tests/nonfinite_cases.py (no GPU): a later edit of a seed or a plant must not make
tests/test_gpu_train_nonfinite.py vacuous.  For every case: the float64 reference contains each class the case is meant
to contain; no finite reference entry exceeds 1024 in magnitude (rounding to f16 creates no infinity by itself);
independent, dependent-finite and non-finite entries partition each tensor, and the parts a case relies on are not
empty; the chain case's sign condition holds; the references' own NaN rules are the ones the tests name."""
import numpy as np
import pytest
import torch

import nonfinite_cases as N
from conftest import golden


def _both(case, where):
    fx = N.conv_fixture(case, where)
    k, relu = fx["geom"]
    return fx, N.conv_reference(fx["planted"], k, relu)[0], N.conv_reference(fx["sanitised"], k, relu)[0]


def _partition_ok(name, ref_p, ref_s):
    ind, dep, non = N.partition(ref_p, ref_s)
    assert bool((ind.int() + dep.int() + non.int() == 1).all()), name
    assert not bool(torch.isfinite(ref_s).logical_not().any()), name + ": the sanitised reference is not finite"
    fin = ref_p[torch.isfinite(ref_p)]
    assert fin.numel() == 0 or float(fin.abs().max()) <= N.LIMIT, (name, float(fin.abs().max()))
    assert float(ref_s.abs().max()) <= N.LIMIT, name
    # rule 3's bound is never infinite: over a set on which the sanitised reference vanishes e_stock counts as 0
    stock = ref_s + 1.0
    assert N._l2_stock(stock, ref_s, dep) < N.INF and N._l2_stock(stock, ref_s, ind) < N.INF, name
    return int(ind.sum()), int(dep.sum()), int(non.sum())


@pytest.mark.parametrize("case,where", N.FORWARD_PLANTS, ids=["%s-%s" % cw for cw in N.FORWARD_PLANTS])
def test_forward_plants(case, where):
    fx, ref_p, ref_s = _both(case, where)
    for n in ("x", "w", "b", "r"):                                  # the plants are where they were put, and only there
        t = fx["planted"][n]
        assert t is None or (N.counts(t)[0] < t.numel()) == (n == where), n
    have = {k for k in range(4) if N.counts(ref_p["out"])[k]}
    assert have == N.FORWARD_EXPECT[(case, where)], (have, N.counts(ref_p["out"]))
    sizes = {}
    for name, t in ref_p.items():
        if t is not None:
            sizes[name] = _partition_ok("%s/%s/%s" % (case, where, name), t, ref_s[name])
            print(case, where, name, N.counts(t), sizes[name])
    assert sizes["out"][0] > 0 and sizes["out"][2] > 0                # locality and the class map both have entries to check
    if where == "x":
        # torch's semantics: the input and bias gradients depend on the cotangent and the filter only
        assert N.counts(ref_p["x"])[0] == ref_p["x"].numel() and N.counts(ref_p["bias"])[0] == ref_p["bias"].numel()
        assert min(N.counts(ref_p["weight"])[1:]) > 0                 # +inf, -inf and NaN rows in the weight gradient
        if fx["geom"][1]:
            # the mask passes the cotangent at a NaN output: some finite gradient entries move with the plants
            assert sizes["weight"][1] > 0 and sizes["bias"][1] > 0


def test_backward_plants():
    fx, ref_p, ref_s = _both(N.FIRST, "cot")
    assert N.counts(fx["planted"]["cot"])[1:] == [1, 1, 1]
    assert all(N.counts(fx["planted"][n])[0] == fx["planted"][n].numel() for n in ("x", "w", "b", "r"))
    x = fx["planted"]["x"]
    assert float(x.min()) == 0 and int((x == 0).sum()) > x.numel() // 3   # x >= 0 with many exact zeros
    assert N.same(ref_p["out"], ref_s["out"]) and N.counts(ref_p["out"])[0] == ref_p["out"].numel()
    # every plant sits where the ReLU passes it
    cot = fx["planted"]["cot"]
    assert bool((ref_p["out"][~torch.isfinite(cot)] > 0).all())
    for name in ("x", "weight", "bias", "residual"):
        ind, dep, non = _partition_ok("cot/" + name, ref_p[name], ref_s[name])
        assert ind > 0 and non > 0, name
    assert N.counts(ref_p["weight"])[3] > 0                            # inf * 0 in the weight gradient
    assert N.counts(ref_p["bias"])[1:] == [1, 1, 1] and N.counts(ref_p["residual"])[1:] == [1, 1, 1]
    # unaffected filter rows: 61 of 64 out channels
    rows = torch.isfinite(ref_p["weight"]).flatten(1).all(1)
    assert int(rows.sum()) == 61


def test_chain_overflows_in_layer_one_and_turns_nan_in_layer_two():
    f = N.chain_fixture(True)
    pre1, out1, out2 = N.chain_reference(f)
    bi, y, x = N.CHAIN_PIXEL
    hood = pre1[bi, :, y - 1:y + 2, x - 1:x + 2]
    assert float(hood.min()) >= 1.2e5 - 1e3                            # 1.8 x f16's overflow threshold
    assert N.counts(out1) == [out1.numel() - 64 * 9, 64 * 9, 0, 0]
    w2 = f["w2"].flatten(1)
    assert bool(((w2 > 0).any(1) & (w2 < 0).any(1)).all())             # every layer-2 filter row has both signs
    assert N.counts(out2) == [out2.numel() - 64 * 9, 0, 0, 64 * 9]
    assert bool(torch.isnan(out2[bi, :, y - 1:y + 2, x - 1:x + 2]).all())
    g = N.chain_fixture(False)
    assert all(N.counts(t)[0] == t.numel() for t in N.chain_reference(g))
    assert float(N.chain_reference(g)[1].max()) < 256
    for n in f:
        assert n == "x" or torch.equal(f[n], g[n])


def test_pool_reference_rules():
    x, go = N.pool_fixture()
    v, g, i = N.pool_reference(x, go)
    assert N.counts(x)[1] > 0 and N.counts(x)[2] > 0 and N.counts(x)[3] >= 7
    assert i[0, 0, 0, 0] == 0 and i[0, 1, 1, 2] == 3 and i[1, 2, 4, 6] == 7      # the NaN's own orientation
    assert i[1, 3, 2, 3] == 2 and torch.isnan(v[1, 3, 2, 3])                     # not the larger finite value
    assert i[0, 2, 3, 3] == 4                                                    # the first NaN
    assert i[0, 1, 4, 0] == 6 and v[0, 1, 4, 0] == N.INF
    assert i[1, 1, 3, 1] == 0 and v[1, 1, 3, 1] == -N.INF
    assert i[0, 3, 2, 2] == 1 and i[1, 0, 4, 4] == 6
    assert N.counts(g)[0] == g.numel() and int((g != 0).sum()) == go.numel() - int((go == 0).sum())
    assert N.counts(v)[3] == 6


@pytest.mark.parametrize("name", list(N.LOSS_SCENARIOS))
def test_loss_scenarios(name):
    g, n = golden("s2anet_loss.npz"), golden("net_forward.npz")
    names = ("fam_cls", "fam_bbox", "odm_cls", "odm_bbox")
    maps = [[torch.from_numpy(n["%s_%d" % (k, l)]).clone() for l in range(5)] for k in names]
    anchors = [[torch.from_numpy(n["%s_anchors_%d" % (k, l)]) for l in range(5)] for k in ("init", "refine")]
    targets = torch.from_numpy(g["targets"])
    B = maps[0][0].shape[0]
    ts = targets[torch.argsort(targets[:, 0], stable=True)]
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(ts[:, 0].long(), minlength=B), 0)
    ids = torch.from_numpy(np.asarray(g["assign_ids"])).long()
    shapes = [tuple(m.shape[2:]) for m in maps[0]]
    plants, ids = N.loss_plants(name, ids, ts, off, shapes)
    clean_loss, clean_items = N.loss_reference(maps + anchors, ids, ts, off)
    assert bool(torch.isfinite(clean_items).all())
    for k, lvl, at, v in plants:
        maps[k][lvl][at] = v
    for lst in maps:
        for t in lst:
            t.requires_grad_(True)
    loss, items = N.loss_reference(maps + anchors, ids, ts, off)
    loss.sum().backward()
    want = N.LOSS_SCENARIOS[name][4]
    assert [k for k in range(4) if not bool(torch.isfinite(items[k]))] == list(want), items
    planted = {(k, lvl, at) for k, lvl, at, _ in plants}
    for k, lst in enumerate(maps):
        for lvl, t in enumerate(lst):
            bad = (~torch.isfinite(t.grad)).nonzero().tolist()
            assert all((k, lvl, tuple(at)) in planted for at in bad), (k, lvl, bad)     # a non-finite gradient only at a plant
    for k, lvl, at, v in plants:
        gv = maps[k][lvl].grad[at]
        if want:
            assert not bool(torch.isfinite(gv)), (k, lvl, at)
        else:
            assert float(gv) == 0.0, (k, lvl, at)                                      # what does not enter gets an exact zero
    if not want:
        assert torch.equal(items, clean_items)


@pytest.mark.parametrize("plant", list(N.ALIGN_PLANTS))
@pytest.mark.parametrize("case", list(N.ALIGN_CASES))
def test_align_conv_plants(case, plant):
    fx = N.align_fixture(case, plant)
    H, W = N.ALIGN_HW
    h, w = N.align_points(fx["anchors"])
    assert float(torch.minimum((h - h.round()).abs().min(), (w - w.round()).abs().min())) > 1e-3    # no zero bilinear weight
    # some sampling points of the planted corner's own position, and of its neighbours, fall outside the image
    assert bool(((h[0, :, :2, :2] < 0) | (w[0, :, :2, :2] < 0)).any()) and bool(((h <= -1) | (w <= -1) | (h >= H) | (w >= W)).any())
    # ... and some corners next to it are dropped while the planted pixel is the clamped neighbour (row or column -1)
    edge = ((h[0] > -1) & (h[0] < 0) & (w[0] > -1) & (w[0] < 1)) | ((w[0] > -1) & (w[0] < 0) & (h[0] > -1) & (h[0] < 1))
    assert bool(edge.any())
    ref_p, pre = N.align_reference(fx["planted"], fx["anchors"])
    ref_s, _ = N.align_reference(fx["sanitised"], fx["anchors"])
    sizes = {n: _partition_ok("%s/%s/%s" % (case, plant, n), ref_p[n], ref_s[n]) for n in ref_p}
    c = N.counts(ref_p["out"])
    assert c[0] > 0 and c[3] > 0 and c[2] == 0 and (c[1] > 0) == (plant != "nan_filter")
    assert sizes["out"][0] > 0 and sizes["out"][2] > 0
    if plant == "nan_filter":
        assert sizes["weight"][0] > 0 and N.counts(ref_p["x"])[3] > 0
    else:
        assert N.counts(ref_p["x"])[0] == ref_p["x"].numel() and sizes["x"][0] > 0 and min(N.counts(ref_p["weight"])[1:]) > 0
        assert bool(torch.isinf(pre).any()) and bool((pre == -N.INF).any())           # what the x3 pin is about
    pin, _ = N.align_reference(fx["planted"], fx["anchors"], inf_is_nan=True)
    assert N.counts(pin["out"])[1:3] == [0, 0] and N.counts(pin["out"])[3] == int((~torch.isfinite(pre)).sum())
