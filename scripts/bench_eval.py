#!/usr/bin/env python3
"""Time the all-class Task-1 evaluation on one seeded synthetic validation set of the size a user runs:
15 classes, 4 096 images, 1 048 576 detection rows (256 per image, ~10 % of them padding), 131 072 ground truths with a
DOTA-like skew (class 0 holds ~60 % of the boxes, classes 13 and 14 are nearly empty).  Detections are jittered ground
truths plus false alarms, as gen_voc_eval of tests/golden/make_golden.py builds them.

  compute        Task1Evaluator.compute() -- device events, after warm-up, repetitions for about a second
  graph_replay   the same call replayed from a captured graph
  per_class      the existing route: voc_eval_arrays once per class (host argsort, one polyiou_match launch, mark_tp_fp in
                 Python, cumulative sums and AP on the host) -- wall time of ONE pass
Before anything is timed both routes must give equal VOC07 ap per class.

  python scripts/bench_eval.py [--out profiles/eval_bench.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/bench_eval.py --only-compute 5
  python scripts/bench_eval.py --merge-stats DIR/.../run_kernel_stats.csv --out profiles/eval_bench.json
The second command is the separate profiler run of the per-kernel breakdown; the third puts its k_eval_* and sort rows
into the JSON the first one wrote.
"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

C, I, PER_IMAGE, GT_PER_IMAGE = 15, 4096, 256, 32
DUP, PAD = 2, 26                       # detections per ground truth; padded slots per image (26 / 256 = 10.2 %)


def class_weights():
    w = np.full(C, 0.4 / (C - 3))
    w[0], w[13], w[14] = 0.6, 1e-4, 1e-4
    return w / w.sum()


def build(dev, seed=2024):
    """-> dict of device tensors (dp f64 [D,8], ds f64, dl i32, di i32, gp f64 [G,8], gl, gi i32, gd u8)"""
    from s2anet_amd.formats import rbox_to_poly
    rng = np.random.default_rng(seed)
    G, D = I * GT_PER_IMAGE, I * PER_IMAGE

    def rboxes(n):
        b = np.empty((n, 5), np.float32)
        b[:, :2] = rng.uniform(0, 1024, (n, 2))
        b[:, 2:4] = rng.uniform(8, 100, (n, 2))
        b[:, 4] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, n)
        return b

    def polys(b):
        return np.round(rbox_to_poly(torch.from_numpy(b).to(dev)).cpu().numpy().astype(np.float64), 1)
    gp = polys(rboxes(G))
    gl = rng.choice(C, G, p=class_weights()).astype(np.int32)
    gi = np.repeat(np.arange(I, dtype=np.int32), GT_PER_IMAGE)
    gd = (rng.random(G) < 0.2).astype(np.uint8)
    n_fa = PER_IMAGE - PAD - DUP * GT_PER_IMAGE
    dp = np.zeros((I, PER_IMAGE, 8))
    ds = np.zeros((I, PER_IMAGE))
    dl = np.full((I, PER_IMAGE), -1, np.int32)
    n_hit = DUP * GT_PER_IMAGE
    src = np.repeat(np.arange(G).reshape(I, GT_PER_IMAGE), DUP, axis=1)
    dp[:, :n_hit] = np.round(gp[src] + rng.normal(0, 2.5, (I, n_hit, 8)), 1)
    dl[:, :n_hit] = gl[src]
    ds[:, :n_hit] = rng.random((I, n_hit))
    dp[:, n_hit:n_hit + n_fa] = polys(rboxes(I * n_fa)).reshape(I, n_fa, 8)
    dl[:, n_hit:n_hit + n_fa] = rng.choice(C, (I, n_fa), p=class_weights())
    ds[:, n_hit:n_hit + n_fa] = rng.random((I, n_fa)) * 0.8
    dp[:, n_hit + n_fa:] = np.nan                                   # padding is never interpreted
    ds[:, n_hit + n_fa:] = np.nan
    di = np.repeat(np.arange(I, dtype=np.int32), PER_IMAGE)
    host = dict(dp=dp.reshape(D, 8), ds=ds.reshape(D), dl=dl.reshape(D), di=di, gp=gp, gl=gl, gi=gi, gd=gd)
    return host, {k: torch.from_numpy(v).to(dev) for k, v in host.items()}


def evaluator(dev, t):
    from s2anet_amd.evaluate import Task1Evaluator
    ev = Task1Evaluator(C, I * PER_IMAGE, I * GT_PER_IMAGE, I, dev)
    ev.add_ground_truth(t["gp"], t["gl"], t["gi"], t["gd"])
    ev.add_polygons(t["dp"], t["ds"], t["dl"], t["di"])
    return ev


def per_class_route(h, dev):
    from s2anet_amd.evaluate import voc_eval_arrays
    aps = np.zeros(C)
    for c in range(C):
        d, g = h["dl"] == c, h["gl"] == c
        if d.any() and (g & (h["gd"] == 0)).any():
            aps[c] = voc_eval_arrays(h["dp"][d], h["ds"][d], h["di"][d], h["gp"][g], h["gi"][g], h["gd"][g], I,
                                     use_07_metric=True, device=dev)[2]
    return aps


def timed(fn, budget_s=1.0, warmup=3, lo=5, hi=500):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = int(min(hi, max(lo, budget_s / max(time.perf_counter() - t0, 1e-6))))
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return {"median_us": round(times[len(times) // 2], 1), "min_us": round(times[0], 1), "max_us": round(times[-1], 1), "repetitions": reps}


def merge_stats(path, out):
    def short(name):
        m = re.search(r"k_eval_\w+|k_rbox\w*", name)
        if m:
            return m.group(0)
        m = re.search(r"wrapped_(\w+?)_config", name)
        return "rocprim " + (m.group(1) if m else name[:60])
    rows = {}
    for r in csv.DictReader(open(path)):
        if "k_eval_" in r["Name"] or "rocprim" in r["Name"] or "k_rbox" in r["Name"]:
            acc = rows.setdefault(short(r["Name"]), [0, 0.0])
            acc[0] += int(r["Calls"])
            acc[1] += float(r["TotalDurationNs"])
    total = sum(v[1] for v in rows.values())
    res = json.load(open(out))
    res["kernels"] = {"source": "rocprofv3 --kernel-trace --stats on `bench_eval.py --only-compute N` (a run of its own; k_rbox_to_poly "
                                "belongs to building the input)",
                      "rows": [{"name": k, "calls": v[0], "avg_us": round(v[1] / v[0] / 1e3, 1), "share": round(v[1] / total, 4)}
                               for k, v in sorted(rows.items(), key=lambda kv: -kv[1][1])]}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["kernels"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-compute", type=int, default=0, help="just run compute() N times (the program of the profiler run)")
    ap.add_argument("--merge-stats", default=None, help="kernel_stats.csv of the profiler run -> 'kernels' of --out")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out)
    dev = torch.device("cuda:0")
    host, t = build(dev)
    ev = evaluator(dev, t)
    if args.only_compute:
        for _ in range(args.only_compute):
            ev.compute()
        torch.cuda.synchronize()
        return
    res_dev = ev.compute()
    ap_dev = res_dev.ap.cpu().numpy()
    t0 = time.perf_counter()
    ap_host = per_class_route(host, dev)
    torch.cuda.synchronize()
    per_class_s = time.perf_counter() - t0
    equal = bool(np.array_equal(ap_dev, ap_host))
    if not equal:
        raise SystemExit(f"the routes disagree: device {ap_dev.tolist()} per-class {ap_host.tolist()}")
    compute = timed(ev.compute)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.compute()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = ev.compute()
    replay = timed(graph.replay)
    torch.cuda.synchronize()
    res = {"workload": "Task-1 evaluation, all classes: 15 classes, 4096 images, 1048576 detection rows, 131072 ground truths",
           "sizes": {"classes": C, "images": I, "detection_rows": I * PER_IMAGE, "padding_rows": int((host["dl"] < 0).sum()),
                     "ground_truths": I * GT_PER_IMAGE, "detections_per_class": np.bincount(host["dl"][host["dl"] >= 0], minlength=C).tolist(),
                     "ground_truths_per_class": np.bincount(host["gl"], minlength=C).tolist(),
                     "workspace_bytes": int(ev._tables()["ws"].numel())},
           "ap_voc07_equal_between_routes": equal, "map50": float(ap_dev.mean()), "ap_voc07": ap_dev.tolist(),
           "graph_replay_equals_eager": bool(torch.equal(static.ap, res_dev.ap) and torch.equal(static.f1, res_dev.f1)),
           "compute": compute, "graph_replay": replay,
           "per_class_route": {"wall_s": round(per_class_s, 3), "repetitions": 1},
           "speedup_compute_over_per_class": round(per_class_s * 1e6 / compute["median_us"], 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
