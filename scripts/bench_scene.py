#!/usr/bin/env python3
"""Whole-scene detection on one MI355X: S2ANet.detect_scene on a 4096 x 4096 uint8 scene (25 chips of 1024 x 1024 with
200 px overlap, four fixed batches of 8) with the benchmark detector and the benchmark's candidate calibration.

Reports scenes/s and chips/s of detect_scene(check=False) (no host synchronisation inside the timed region), the stages
on runs of their own (gather, the detect() batches, merge; HIP events), the gather's GB/s next to the measured copy
bound of the part, and -- timed in the same process -- the only route there was before: torch-slicing tile loop ->
detect() -> formats.task1_lines -> merge.merge_lines (text on the host, one synchronous polygon NMS per class).

Every figure is the median of --repeats measurements, each `iters` back-to-back runs after a quarter second of the same
work (clock ramp), with min and max next to it.  Writes profiles/scene_bench.json.

    python scripts/bench_scene.py [--size 4096] [--batch 8] [--repeats 5] [--out profiles/scene_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BOUND_GBPS = 6290.0        # float4 copy measured on the part (79 % of the 8 TB/s HBM3E peak)
WARM_SECONDS = 0.25


def measure(fn, repeats, iters):
    """-> seconds per call: median / min / max over `repeats` event-timed groups of `iters` calls"""
    t0, n = time.perf_counter(), 0
    while n < 2 or time.perf_counter() - t0 < WARM_SECONDS:
        fn()
        n += 1
        torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / 1e3 / iters)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out), "repeats": repeats, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--candidates", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
    args = ap.parse_args()
    import bench
    from s2anet_amd import scene as SC
    from s2anet_amd.detector import build_synthetic_detector
    from s2anet_amd.formats import merged_task1_lines, task1_lines
    from s2anet_amd.merge import merge_lines
    dev = torch.device("cuda:0")
    S, B = 1024, args.batch
    g = torch.Generator().manual_seed(1234)
    scene = torch.randint(0, 256, (args.size, args.size, 3), dtype=torch.uint8, generator=g).to(dev)
    grid = SC.tile_grid(args.size, args.size)
    n = len(grid)
    pad = (-n) % B
    model = build_synthetic_detector(device=dev)
    calib = SC.gather_chips(scene, grid[:B], S)
    got = bench.calibrate_cls_bias(model, calib, args.candidates)
    max_cand = int(min(B * 5344 * 15, max(4 * args.candidates * B, 65536)))
    kw = dict(max_candidates=max_cand)
    names = ["c%02d" % c for c in range(15)]

    res = model.detect_scene(scene, batch=B, return_chips=True, **kw)          # checked run: what the scene yields
    dets, labels, counts, origins, rates = res.per_chip
    merged = int(res.class_counts.sum())
    org_dev = SC._origins_dev(np.concatenate([grid, np.tile(np.asarray([[args.size, args.size]], np.int32), (pad, 1))]), dev)
    chips = [res.chips[i:i + B].contiguous(memory_format=torch.channels_last) for i in range(0, n + pad, B)]

    full = measure(lambda: model.detect_scene(scene, batch=B, check=False, **kw), args.repeats, 3)
    gather = measure(lambda: [SC.gather_chips(scene, org_dev[i:i + B], S) for i in range(0, n + pad, B)], args.repeats, 20)
    detect = measure(lambda: [model.detect(c, **kw) for c in chips], args.repeats, 3)
    merge = measure(lambda: SC.merge_detections(dets, labels, counts, origins, rates, check=False), args.repeats, 10)
    moved = (n + pad) * S * S * 3 + int(sum(min(S, args.size - l) * min(S, args.size - u) * 3 for l, u in grid.tolist()))

    def text_route():
        """the parent's route: slicing tile loop -> detect() -> task1_lines (host text) -> merge_lines per class"""
        per_class = {}
        chip_names = SC.chip_names("scene", grid, 1)
        for b0 in range(0, n, B):
            tiles = torch.zeros((B, S, S, 3), dtype=torch.uint8, device=dev)
            for k, (left, up) in enumerate(grid[b0:b0 + B].tolist()):
                sub = scene[up:up + S, left:left + S]
                tiles[k, :sub.shape[0], :sub.shape[1]] = sub
            d, l, c = model.detect(tiles.permute(0, 3, 1, 2), **kw)[:3]
            for k in range(min(B, n - b0)):
                m = int(c[k])
                for cname, lines in task1_lines(chip_names[b0 + k], d[k, :m], l[k, :m], names).items():
                    per_class.setdefault(cname, []).extend(lines)
        return {cname: merge_lines(lines, 0.5) for cname, lines in per_class.items()}

    text_route()
    torch.cuda.synchronize()
    text = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = text_route()
        torch.cuda.synchronize()
        text.append(time.perf_counter() - t0)
    text_lines = sum(len(v) for v in out.values())

    stage_sum = gather["median_s"] + detect["median_s"] + merge["median_s"]
    result = {
        "what": "S2ANet.detect_scene, %d x %d uint8 scene, %d chips of 1024 (gap 200) in %d batches of %d (%d blank)" % (
            args.size, args.size, n, (n + pad) // B, B, pad),
        "device": torch.cuda.get_device_name(0),
        "calibration": {"nms_candidates_per_chip": round(got, 1), "max_candidates": max_cand,
                        "detections_per_chip": round(float(counts[:n].float().mean()), 1), "merged_detections": merged,
                        "merge_status": res.status.tolist()},
        "detect_scene": dict(full, scenes_per_s=1.0 / full["median_s"], chips_per_s=n / full["median_s"]),
        "stages": {
            "gather": dict(gather, bytes_moved=moved, gb_per_s=moved / gather["median_s"] / 1e9, copy_bound_gb_per_s=COPY_BOUND_GBPS),
            "detect_batches": detect, "merge": merge,
            "gather_plus_merge_share_of_stage_sum": (gather["median_s"] + merge["median_s"]) / stage_sum},
        "text_route": {"what": "torch-slicing tile loop -> detect() -> task1_lines -> merge_lines (wall clock, host text)",
                       "median_s": statistics.median(text), "min_s": min(text), "max_s": max(text), "repeats": 3,
                       "merged_lines": text_lines, "scenes_per_s": 1.0 / statistics.median(text)},
    }
    lines_dev = sum(len(v) for v in merged_task1_lines("scene", res, names).values())
    result["calibration"]["merged_lines_device_route"] = lines_dev
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
