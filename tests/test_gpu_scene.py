"""GPU: whole-scene detection -- chip gather (bit equality with torch slicing), the class-segmented polygon merge
against the CPU oracle's py_cpu_nms_poly_fast restatement (oracle.nms_poly) per class, the text route
(formats-style lines -> merge.merge_lines), overflow reporting, large inputs, HIP-graph capture, and
S2ANet.detect_scene end to end.

Rows of the merge tests come from ONE generator (make_rows): objects of a random class, centre, size in [8, 120] px
and angle; every chip that contains an object's centre emits it once or twice, jittered by ~1.5 px and 3 % in size,
coordinates rounded to 1/16 px, scores k / 10000 with distinct k inside a class, rows shuffled inside a chip, ragged
counts, -1 label padding and garbage behind the counts.  The expectation is built in numpy: the float32 polygons of
the existing rbox_to_poly op (tested on its own in test_gpu_ops.py) widened to float64, (coordinate + origin) / rate in
float64, the float32 scores widened -- then oracle.nms_poly per class on the rows in chip-major order.
"""
import time

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

SUB = 1024


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ------------------------------------------------------------------------------------------------ generator
def make_rows(seed, height, width, n_obj, num_classes=15, K=None, rates=(1.0,), gap=200, classes=None, angle0=False):
    """-> dict(dets [n,K,6] f32, labels [n,K] i32, counts [n] i32, origins [n,2] i32, rates [n] f64).
    rates: the objects live in a height x width scene; for every rate r the scene resized by r is tiled and every
    chip reports its objects in ITS pixels (coordinates * r - origin).  K: slots per chip (None: the largest chip;
    a chip with more emissions than K keeps K of them).  classes: the class ids objects draw from.
    angle0: every box axis aligned with sizes in 1/8 px (its polygon is then exact in 1/16 px)."""
    from s2anet_amd.scene import tile_grid
    rng = np.random.default_rng(seed)
    pool = np.arange(num_classes) if classes is None else np.asarray(classes)
    cls = pool[rng.integers(0, len(pool), n_obj)]
    cx, cy = rng.uniform(0, width, n_obj), rng.uniform(0, height, n_obj)
    w, h = rng.uniform(8, 120, n_obj), rng.uniform(8, 120, n_obj)
    ang = np.zeros(n_obj) if angle0 else rng.uniform(-np.pi / 4, 3 * np.pi / 4, n_obj)
    per_chip, origins, chip_rate = [], [], []
    for r in rates:
        for left, up in tile_grid(int(round(height * r)), int(round(width * r)), SUB, gap):
            x, y = cx * r - left, cy * r - up
            inside = np.nonzero((x >= 0) & (x < SUB) & (y >= 0) & (y < SUB))[0]
            idx = np.repeat(inside, rng.integers(1, 3, inside.size))
            m = idx.size
            q = 8.0 if angle0 else 16.0
            row = np.empty((m, 5))
            row[:, 0] = np.round((x[idx] + rng.normal(0, 1.5, m)) * 16) / 16
            row[:, 1] = np.round((y[idx] + rng.normal(0, 1.5, m)) * 16) / 16
            row[:, 2] = np.maximum(np.round(w[idx] * r * (1 + rng.normal(0, 0.03, m)) * q) / q, 1.0)
            row[:, 3] = np.maximum(np.round(h[idx] * r * (1 + rng.normal(0, 0.03, m)) * q) / q, 1.0)
            row[:, 4] = ang[idx] if angle0 else ang[idx] + rng.normal(0, 0.02, m)
            per_chip.append((row, cls[idx]))
            origins.append((left, up))
            chip_rate.append(r)
    n = len(per_chip)
    if K is None:
        K = max(1, max(len(c[1]) for c in per_chip))
    dets = rng.uniform(0, 900, (n, K, 6)).astype(np.float32)             # garbage behind the counts (never read as rows)
    dets[..., 2:4] = rng.uniform(8, 120, (n, K, 2))
    dets[..., 4] = 0.3
    dets[..., 5] = rng.uniform(0.06, 1, (n, K))
    labels = np.full((n, K), -1, np.int32)
    labels[:, K // 2:] = rng.integers(0, num_classes, (n, K - K // 2))    # ... with real-looking labels on half of it
    counts = np.zeros(n, np.int32)
    for i, (row, c) in enumerate(per_chip):
        sel = rng.permutation(len(c))[:K]
        counts[i] = sel.size
        dets[i, :sel.size, :5] = row[sel]
        labels[i, :sel.size] = c[sel]
    valid = np.arange(K)[None, :] < counts[:, None]
    # distinct scores inside a class: k / 10000 (a finer grid when a class holds more rows than that grid has values)
    for c in range(num_classes):
        at = np.nonzero(valid & (labels == c))
        denom = 10000
        while at[0].size > denom * 9 // 10:
            denom *= 10
        ks = rng.permutation(np.arange(denom // 20, denom))[:at[0].size]
        dets[at[0], at[1], 5] = (ks / denom).astype(np.float32)
    return dict(dets=dets, labels=labels, counts=counts, origins=np.asarray(origins, np.int32).reshape(-1, 2),
                rates=np.asarray(chip_rate, np.float64))


def scene_rows(dets, labels, counts, origins, rates, num_classes):
    """numpy float64 rows of the merge: polys [n*K,8] in scene coordinates, scores, valid mask"""
    from s2anet_amd.formats import rbox_to_poly
    n, K = labels.shape
    d = np.ascontiguousarray(dets, np.float32).reshape(-1, 6)
    p = rbox_to_poly(cu(d)).cpu().numpy().astype(np.float64) if d.shape[0] else np.zeros((0, 8))
    ox = np.repeat(origins[:, 0].astype(np.float64), K)[:, None]
    oy = np.repeat(origins[:, 1].astype(np.float64), K)[:, None]
    rt = np.repeat(np.asarray(rates, np.float64), K)[:, None]
    p[:, 0::2] = (p[:, 0::2] + ox) / rt
    p[:, 1::2] = (p[:, 1::2] + oy) / rt
    sc = d[:, 5].astype(np.float64)
    lb = labels.reshape(-1)
    valid = ((np.arange(K)[None, :] < counts[:, None]).reshape(-1)) & (lb >= 0) & (lb < num_classes)
    return p, sc, lb, valid


def oracle_merge(rows, thresh=0.5, num_classes=15):
    """-> (src, polys, scores, labels, class_counts, share) with share[c] = kept share of class c's rows"""
    p, sc, lb, valid = scene_rows(rows["dets"], rows["labels"], rows["counts"], rows["origins"], rows["rates"], num_classes)
    src, counts, share = [], [], {}
    for c in range(num_classes):
        at = np.nonzero(valid & (lb == c))[0]
        keep = oracle.nms_poly(np.concatenate([p[at], sc[at, None]], 1), thresh) if at.size else np.zeros(0, np.int64)
        src.append(at[keep])
        counts.append(keep.size)
        if at.size:
            share[c] = keep.size / at.size
    src = np.concatenate(src) if src else np.zeros(0, np.int64)
    return src, p[src], sc[src], lb[src].astype(np.int64), np.asarray(counts, np.int64), share


def hbb_pairs(rows, num_classes=15):
    """pairs py_cpu_nms_poly_fast hands to iou_poly: same class, axis-aligned boxes with a positive intersection"""
    p, sc, lb, valid = scene_rows(rows["dets"], rows["labels"], rows["counts"], rows["origins"], rows["rates"], num_classes)
    total = 0
    for c in range(num_classes):
        q = p[valid & (lb == c)]
        x1, x2, y1, y2 = q[:, 0::2].min(1), q[:, 0::2].max(1), q[:, 1::2].min(1), q[:, 1::2].max(1)
        for i in range(0, q.shape[0], 2048):
            w = np.maximum(0.0, np.minimum(x2[i:i + 2048, None], x2[None]) - np.maximum(x1[i:i + 2048, None], x1[None]))
            hh = np.maximum(0.0, np.minimum(y2[i:i + 2048, None], y2[None]) - np.maximum(y1[i:i + 2048, None], y1[None]))
            total += int((w * hh > 0).sum())
        total -= q.shape[0]                                               # (a row with itself)
    return total // 2


def run_merge(rows, thresh=0.5, num_classes=15, **kw):
    from s2anet_amd.scene import merge_detections
    return merge_detections(cu(rows["dets"]), cu(rows["labels"]), cu(rows["counts"]), rows["origins"], rows["rates"],
                            num_classes=num_classes, thresh=thresh, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_equals_oracle(res, want, what=""):
    src, polys, scores, labels, class_counts, _ = want
    assert int(res.status[0]) == 0, what
    got_counts = res.class_counts.cpu().numpy()
    print(what, "rows kept", int(got_counts.sum()), "oracle", int(class_counts.sum()), "status", res.status.tolist())
    assert (got_counts == class_counts).all(), (what, got_counts, class_counts)
    m = int(class_counts.sum())
    assert res.src[:m].cpu().numpy().tolist() == src.tolist(), what
    assert (res.labels[:m].cpu().numpy() == labels).all(), what
    assert (bits(res.polys[:m].cpu().numpy()) == bits(polys)).all(), what
    assert (bits(res.scores[:m].cpu().numpy()) == bits(scores)).all(), what


def assert_not_trivial(rows, want, num_classes=15):
    valid = np.arange(rows["labels"].shape[1])[None, :] < rows["counts"][:, None]
    share = want[5]
    print("rows", int(valid.sum()), "kept", int(want[4].sum()), "kept share per class %.2f .. %.2f" % (min(share.values()), max(share.values())))
    assert len(share) == num_classes
    for c, s in share.items():
        assert 0.25 <= s <= 0.75, (c, s)                                 # kept and suppressed both >= 25 % of the class


# ------------------------------------------------------------------------------------------------ 1. gather
def _expected_chips(scene, origins):
    H, W = scene.shape[:2]
    padded = torch.zeros((H + 2 * SUB, W + 2 * SUB, 3), dtype=torch.uint8, device=scene.device)
    padded[SUB:SUB + H, SUB:SUB + W] = scene
    return torch.stack([padded[up + SUB:up + 2 * SUB, left + SUB:left + 2 * SUB] for left, up in origins.tolist()])


@pytest.mark.parametrize("hw", [(600, 900), (1025, 1849), (2500, 1800), (4096, 4096)])
def test_gather_equals_torch_slicing(hw):
    from s2anet_amd.scene import gather_chips, tile_grid
    H, W = hw
    g = torch.Generator().manual_seed(H * 7 + W)
    scene = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev())
    grid = tile_grid(H, W)
    shuffled = grid[np.random.default_rng(3).permutation(len(grid))]
    # out of grid order, and origins that reach past every border of the scene (negative, partly and wholly outside)
    odd = np.concatenate([shuffled[::-1], np.asarray([[-5, -7], [W - 10, H - 3], [W, H], [-SUB + 1, 3], [3, -SUB + 1], [1, 2]], np.int32)])
    for origins in (grid, shuffled, odd):
        out = torch.full((len(origins), SUB, SUB, 3), 0xFF, dtype=torch.uint8, device=dev())
        chips = gather_chips(scene, origins, SUB, out=out)
        assert chips.shape == (len(origins), 3, SUB, SUB) and chips.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(chips.permute(0, 2, 3, 1), _expected_chips(scene, origins))
    again = gather_chips(scene, cu(grid), SUB)                            # origins already on the device, own output buffer
    assert torch.equal(again.permute(0, 2, 3, 1), _expected_chips(scene, grid))
    view = scene[1:]                                                      # a view that starts W * 3 bytes into the buffer (odd for odd W)
    assert torch.equal(gather_chips(view, grid, SUB).permute(0, 2, 3, 1), _expected_chips(view, grid))


# ------------------------------------------------------------------------------------------------ 2. merge vs the oracle
@pytest.mark.parametrize("case", [(2500, 1800, 1500, 0.5), (2500, 1800, 1500, 0.3), (2500, 1800, 1500, 0.7), (4096, 4096, 6000, 0.5)])
def test_merge_equals_oracle_per_class(case):
    H, W, n_obj, thresh = case
    rows = make_rows(7, H, W, n_obj)
    want = oracle_merge(rows, thresh)
    if thresh == 0.5:
        assert_not_trivial(rows, want)
    res = run_merge(rows, thresh)
    assert res.polys.shape[0] == int(want[4].sum())                       # check=True trims
    assert_equals_oracle(res, want, str(case))
    raw = run_merge(rows, thresh, check=False)                            # untrimmed: the tail behind the kept rows is cleared
    m = int(want[4].sum())
    assert raw.polys.shape[0] == rows["labels"].size
    assert_equals_oracle(raw, want, str(case) + " check=False")
    assert int(raw.src[m:].max()) == -1 and int(raw.labels[m:].max()) == -1 and float(raw.polys[m:].abs().max()) == 0.0
    assert int(raw.status[3]) == int((np.arange(rows["labels"].shape[1])[None, :] < rows["counts"][:, None]).sum())
    assert int(raw.status[1]) == hbb_pairs(rows)


def test_merge_special_inputs():
    from s2anet_amd.scene import merge_detections
    # empty input: no chip at all, and chips without slots
    for shape in ((0, 7), (3, 0)):
        r = merge_detections(torch.zeros(shape + (6,), device=dev()), torch.zeros(shape, dtype=torch.int32, device=dev()),
                             torch.zeros(shape[0], dtype=torch.int32, device=dev()), np.zeros((shape[0], 2), np.int32))
        assert r.polys.shape == (0, 8) and r.src.numel() == 0 and int(r.class_counts.sum()) == 0 and int(r.status[0]) == 0
    # all counts 0 (the rows look real, none is one)
    rows = make_rows(11, 2500, 1800, 400)
    rows0 = dict(rows, counts=np.zeros_like(rows["counts"]))
    r = run_merge(rows0)
    assert r.src.numel() == 0 and int(r.class_counts.sum()) == 0 and r.status.tolist() == [0, 0, 0, 0]
    # one class only: 15 classes of which one occurs, and num_classes = 1
    one = make_rows(12, 2500, 1800, 300, classes=[3])
    want = oracle_merge(one)
    assert want[4][3] == want[4].sum() > 0
    assert_equals_oracle(run_merge(one), want, "class 3 only")
    solo = make_rows(13, 2500, 1800, 300, num_classes=1)
    assert_equals_oracle(run_merge(solo, num_classes=1), oracle_merge(solo, num_classes=1), "num_classes=1")
    # a class with a single row (class 14: its one row is kept whatever lies under it)
    single = make_rows(14, 2500, 1800, 500, classes=list(range(14)))
    single["labels"][0, 0] = 14
    want = oracle_merge(single)
    assert want[4][14] == 1 and want[0][-1] == 0
    assert_equals_oracle(run_merge(single), want, "single-row class")


def test_merge_mixed_rates():
    rows = make_rows(15, 1800, 1500, 900, rates=(1.0, 0.5, 1.5))
    assert sorted(set(rows["rates"].tolist())) == [0.5, 1.0, 1.5]
    want = oracle_merge(rows)
    src_chip = want[0] // rows["labels"].shape[1]
    assert len(set(rows["rates"][src_chip].tolist())) == 3                # survivors from every rate
    # (three rates: an object is reported by the chips of three tilings, about 6.5 rows per object, so about 15 % of a
    # class's rows survive -- the 25 % bound of the one-rate cases does not apply; both sides still hold >= 10 %)
    print("kept share per class %.2f .. %.2f" % (min(want[5].values()), max(want[5].values())))
    assert len(want[5]) == 15 and all(0.10 <= s <= 0.90 for s in want[5].values())
    assert_equals_oracle(run_merge(rows), want, "rates")


def test_merge_score_tie_across_two_chips():
    """the same object reported by two overlapping chips with EQUAL scores: the row of the earlier chip is kept
    (ascending row index, the tie rule of s2a_nms_poly) and the oracle agrees"""
    K, n_tie = 16, 6
    origins = np.asarray([[0, 0], [824, 0]], np.int32)
    dets = np.zeros((2, K, 6), np.float32)
    labels = np.full((2, K), -1, np.int32)
    for k in range(n_tie):
        x, y = 850.0 + 25 * k, 100.0 + 140 * k
        dets[0, k] = [x, y, 40, 20, 0.3, 0.5]
        dets[1, n_tie - 1 - k] = [x - 824 + 0.5, y, 40, 20, 0.3, 0.5]    # the tied twin, listed in another order
        labels[0, k] = labels[1, n_tie - 1 - k] = k % 3
    rows = dict(dets=dets, labels=labels, counts=np.asarray([n_tie, n_tie], np.int32), origins=origins, rates=np.ones(2))
    want = oracle_merge(rows)
    assert sorted(want[0].tolist()) == list(range(n_tie))                 # chip 0's rows win every tie
    assert_equals_oracle(run_merge(rows), want, "ties")


# ------------------------------------------------------------------------------------------------ 3. the text route
def test_merge_equals_text_route():
    """formats.task1_lines-style lines -> merge.merge_lines (the existing path, pinned to the reference script) against
    merged_task1_lines(merge_detections(...)): the same lines per class, in the same order.

    The lines are written as task1_lines writes them (val.py:40-52: chip name, score, the 8 coordinates of
    rbox_to_poly) EXCEPT for the number format: '%.4f' is not exact for these rows -- float32(k / 10000) is not a
    4-decimal number (0.1234 -> 0.12340000271797180), and the corners of a rotated box come out of float32
    trigonometry -- and the merged files print str(confidence), so the two routes could not agree on a single line.
    repr() of the widened float32 is exact, which leaves the merge itself as the only thing compared.  A second pass
    runs formats.task1_lines ITSELF ('%.4f') on axis-aligned boxes with dyadic scores, where its text is exact."""
    from s2anet_amd.formats import merged_task1_lines, rbox_to_poly, task1_lines
    from s2anet_amd.merge import merge_lines
    from s2anet_amd.scene import chip_names
    names = ["c%02d" % c for c in range(15)]
    for exact_fmt in (True, False):
        rows = make_rows(21, 2500, 1800, 1200, angle0=not exact_fmt)
        if not exact_fmt:                                                 # scores on a 1/16 grid: exact with 4 decimals (many ties)
            n, K = rows["labels"].shape
            rows["dets"][..., 5] = ((np.arange(n * K).reshape(n, K) * 7 % 15 + 1) / 16.0).astype(np.float32)
        chips = chip_names("P0007", rows["origins"], 1)
        per_class = {}
        for i, chip in enumerate(chips):
            k = int(rows["counts"][i])
            d, lb = cu(rows["dets"][i, :k]), cu(rows["labels"][i, :k])
            if exact_fmt:
                polys = rbox_to_poly(d[:, :5]).cpu().numpy().astype(np.float64)
                for p, sc, c in zip(polys.tolist(), rows["dets"][i, :k, 5].astype(np.float64).tolist(), rows["labels"][i, :k].tolist()):
                    per_class.setdefault(names[c], []).append(chip + " " + repr(sc) + " " + " ".join(map(repr, p)))
            else:
                for cname, lines in task1_lines(chip, d, lb, names).items():
                    per_class.setdefault(cname, []).extend(lines)
        res = run_merge(rows)
        got = merged_task1_lines("P0007", res, names)
        assert set(got) == set(per_class)
        total = 0
        for cname, lines in per_class.items():
            want = merge_lines(lines, 0.5)
            total += len(want)
            # same lines, same order (tied scores of the second pass: both routes list a class's rows chip-major, in
            # detection order, and break ties by that order)
            assert got[cname] == want, cname
        print("exact format" if exact_fmt else "task1_lines", "rows", int(rows["counts"].sum()), "merged lines", total)
        assert total == int(res.class_counts.sum()) and 0.25 * rows["counts"].sum() < total < 0.75 * rows["counts"].sum()


# ------------------------------------------------------------------------------------------------ 4. overflow
def test_pair_list_overflow_is_reported_and_settled():
    rows = make_rows(7, 2500, 1800, 1500)
    pairs = hbb_pairs(rows)
    cap = max(pairs // 10, 1)
    raw = run_merge(rows, pair_capacity=cap, check=False)
    st = raw.status.tolist()
    print("pairs", pairs, "capacity", cap, "status", st)
    assert st[0] != 0 and st[1] >= pairs
    res = run_merge(rows, pair_capacity=cap, check=True)
    assert_equals_oracle(res, oracle_merge(rows), "overflow, check=True")
    exact = run_merge(rows, pair_capacity=pairs, check=False)             # a list of exactly the pairs found is enough
    assert int(exact.status[0]) == 0


# ------------------------------------------------------------------------------------------------ 5. large
def test_merge_25_full_chips_and_workspace_bound():
    """25 chips x 2 000 rows, every slot full (a 4096 x 4096 scene, 30 000 objects): equal to the oracle.  Measured:
    202 937 candidate pairs against a default capacity of 1.6 M, so the default does not overflow here; had it, check=True's
    second run would settle it (test_pair_list_overflow_is_reported_and_settled covers that route).
    The workspace at the default capacity is below n_rows * 2 KiB: no quadratic mask."""
    from s2anet_amd.scene import merge_workspace_bytes
    rows = make_rows(5, 4096, 4096, 30000, K=2000)
    assert rows["labels"].shape == (25, 2000) and (rows["counts"] == 2000).all()
    n_rows = 25 * 2000
    ws = merge_workspace_bytes(n_rows)
    print("workspace", ws, "bytes =", ws / n_rows, "per row")
    assert ws < n_rows * 2048
    raw = run_merge(rows, check=False)
    print("default capacity: status", raw.status.tolist())
    assert_equals_oracle(run_merge(rows), oracle_merge(rows), "25 x 2000")


def test_merge_625_chips():
    """a 20 000 x 20 000 scene: 625 chips x 2 000 slots = 1.25 M rows of capacity, ragged counts, about 200 000 real
    rows (85 000 objects: 209 134 rows).  The CPU oracle takes about 6 s for it (15 classes of ~14 000 rows each)."""
    rows = make_rows(9, 20000, 20000, 85000, K=2000)
    assert rows["labels"].shape == (625, 2000)
    total = int(rows["counts"].sum())
    t0 = time.time()
    want = oracle_merge(rows)
    print("real rows", total, "oracle seconds %.1f" % (time.time() - t0), "kept", int(want[4].sum()))
    assert 150000 <= total <= 260000 and rows["counts"].min() < rows["counts"].max()
    assert_equals_oracle(run_merge(rows), want, "625 chips")


# ------------------------------------------------------------------------------------------------ 6. no host synchronisation
def test_merge_hip_graph_replay_equals_eager():
    """merge_detections(check=False) captured once on a side stream (after a warm-up call there) and replayed on two
    further inputs written into the captured buffers: bit-equal to eager execution"""
    from s2anet_amd.scene import merge_detections
    inputs = [make_rows(s, 2500, 1800, 1200, K=700) for s in (31, 32, 33)]
    org = cu(inputs[0]["origins"])

    def run(d, l, c):
        r = merge_detections(d, l, c, org, None, check=False)
        return r.polys, r.scores, r.labels, r.src, r.class_counts, r.status
    eager = [tuple(t.clone() for t in run(cu(i["dets"]), cu(i["labels"]), cu(i["counts"]))) for i in inputs]
    for e, i in zip(eager, inputs):
        assert int(e[5][0]) == 0 and int(e[4].sum()) == int(oracle_merge(i)[4].sum())
    sd, sl, sc = cu(inputs[0]["dets"]), cu(inputs[0]["labels"]), cu(inputs[0]["counts"])
    side = torch.cuda.Stream(device=dev())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                         # warm the side stream's workspace before capturing on it
        run(sd, sl, sc)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_out = run(sd, sl, sc)
    for k in (1, 2, 0, 2):
        sd.copy_(cu(inputs[k]["dets"]))
        sl.copy_(cu(inputs[k]["labels"]))
        sc.copy_(cu(inputs[k]["counts"]))
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(static_out, eager[k]):
            assert torch.equal(got, ref), k
    assert not torch.equal(eager[0][3], eager[1][3])


# ------------------------------------------------------------------------------------------------ 7. detect_scene
def _detector():
    from s2anet_amd.detector import build_synthetic_detector
    m = build_synthetic_detector(device=dev())
    m.head.odm_cls_head.bias.data.fill_(-2.0)                            # as test_detect_hip_graph_replay_equals_eager:
    m.head.odm_cls_head.weight.data.mul_(20.0)                           # a few thousand candidates per chip
    return m


def _per_chip_rows(res):
    d, l, c, origins, rates = res.per_chip
    return dict(dets=d.cpu().numpy(), labels=l.cpu().numpy(), counts=c.cpu().numpy(), origins=origins, rates=rates)


def test_detect_scene_end_to_end():
    """S2ANet.detect_scene on a 2500 x 1800 scene (6 chips, one padded batch of 8), a scene smaller than a chip and a
    two-rate list; (e) suppression ACROSS chips is observed on the detector's own output."""
    from s2anet_amd.scene import tile_grid
    m = _detector()
    g = torch.Generator().manual_seed(5)
    H, W = 2500, 1800
    scene = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev())
    res = m.detect_scene(scene, batch=8, return_chips=True)
    grid = tile_grid(H, W)
    assert len(grid) == 6 and res.chips.shape == (8, 3, SUB, SUB)
    # (a) the chips are the scene's pixels, the padded ones blank
    assert torch.equal(res.chips[:6].permute(0, 2, 3, 1), _expected_chips(scene, grid))
    assert int(res.chips[6:].max()) == 0
    rows = _per_chip_rows(res)
    K = rows["labels"].shape[1]
    print("counts", rows["counts"].tolist(), "merged", int(res.class_counts.sum()))
    # (b) the padded chips contribute nothing
    assert rows["counts"][:6].min() > 100 and (rows["counts"][6:] == 0).all()
    assert int(res.src.max()) < 6 * K
    # (c) the merge of the detections that were returned
    want = oracle_merge(rows)
    assert_equals_oracle(res, want, "detect_scene")
    # (e) a suppressed row in an overlap strip whose suppressor is a kept row of ANOTHER chip
    p, sc, lb, valid = scene_rows(rows["dets"], rows["labels"], rows["counts"], rows["origins"], rows["rates"], 15)
    kept = np.zeros(p.shape[0], bool)
    kept[want[0]] = True
    cx, cy = p[:, 0::2].mean(1), p[:, 1::2].mean(1)
    chip = np.arange(p.shape[0]) // K
    cover = sum(((cx >= l) & (cx < l + SUB) & (cy >= u) & (cy < u + SUB)).astype(int) for l, u in grid.tolist())
    sup = np.nonzero(valid & ~kept & (cover >= 2))[0]
    x1, x2, y1, y2 = p[:, 0::2].min(1), p[:, 0::2].max(1), p[:, 1::2].min(1), p[:, 1::2].max(1)
    found = 0
    for j in sup[:4000]:
        cand = np.nonzero(kept & (lb == lb[j]) & (chip != chip[j]) & ((sc > sc[j]) | ((sc == sc[j]) & (np.arange(p.shape[0]) < j))) &
                          (np.minimum(x2, x2[j]) > np.maximum(x1, x1[j])) & (np.minimum(y2, y2[j]) > np.maximum(y1, y1[j])))[0]
        if cand.size and (oracle.polyiou(p[cand], np.repeat(p[j:j + 1], cand.size, 0)) > 0.5).any():
            found += 1
    print("suppressed rows in overlap strips", sup.size, "of them suppressed by a kept row of another chip", found)
    assert found >= 1
    # (f) a scene smaller than a chip: one zero-padded chip (+ one blank chip of the batch of 2)
    small = scene[:600, :900].contiguous()
    r2 = m.detect_scene(small, batch=2, return_chips=True)
    assert r2.chips.shape[0] == 2 and torch.equal(r2.chips[:1].permute(0, 2, 3, 1), _expected_chips(small, tile_grid(600, 900)))
    assert int(r2.per_chip[2][1]) == 0 and int(r2.per_chip[2][0]) > 0
    assert_equals_oracle(r2, oracle_merge(_per_chip_rows(r2)), "small scene")
    # (g) two rates of one image merge into one result (the caller resized: every second pixel here)
    half = small[::2, ::2].contiguous()
    r3 = m.detect_scene([(small, 1.0), (half, 0.5)], batch=2, return_chips=True)
    rows3 = _per_chip_rows(r3)
    assert rows3["rates"].tolist() == [1.0, 1.0, 0.5, 0.5] and rows3["counts"][1] == 0 and rows3["counts"][3] == 0
    want3 = oracle_merge(rows3)
    assert_equals_oracle(r3, want3, "two rates")
    assert set((want3[0] // rows3["labels"].shape[1]).tolist()) == {0, 2}  # survivors from both rates in ONE result


def test_detect_scene_chips_equal_plain_detect(monkeypatch):
    """(d) with S2A_OWN_CONV_ALWAYS=1 (every convolution on the project's own bit-reproducible kernel) the per-chip
    detections detect_scene merged are those of a plain detect() on the same batch, bit for bit"""
    monkeypatch.setenv("S2A_OWN_CONV_ALWAYS", "1")
    m = _detector()
    g = torch.Generator().manual_seed(6)
    scene = torch.randint(0, 256, (2500, 1800, 3), dtype=torch.uint8, generator=g).to(dev())
    res = m.detect_scene(scene, batch=8, return_chips=True)
    d, l, c = m.detect(res.chips.contiguous(memory_format=torch.channels_last))[:3]
    pd, pl, pc = res.per_chip[:3]
    assert torch.equal(pd, d) and torch.equal(pl, l) and torch.equal(pc[:6], c[:6]) and int(pc[6:].sum()) == 0
    assert int(c[:6].min()) > 100
