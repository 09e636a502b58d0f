#!/usr/bin/env python3
"""Time the training augmentation (s2anet_amd.TrainAugment) at the training batch, uint8 [8,1024,1024,3]:
  * the image launch for each of the 8 group elements (rot 0..3, without and with the left-right flip; the whole batch
    takes one element), and for the recipe's mixed draw;
  * beside them, interleaved in the same process: a plain out.copy_(imgs) of the batch, and the stock route of the same
    element (torch.rot90 + flip + .contiguous(); it leaves no border line, so it only stands for the bytes moved);
  * the draw launch, and the label launch at G = 240 and G = 4096.
Every route's `--inner` launches are captured into one graph; device events around a replay, `--rounds` rounds, every round
walks all routes in turn; the median of the rounds' per-launch times, their minimum and maximum.  The image times come with the ratio to the copy of the same round
order and with the achieved bytes per second (one read and one write of the batch).
Writes one JSON document (default: profiles/augment.json).  --label-report PATH takes in what tests/test_gpu_augment.py wrote
under S2A_AUGMENT_REPORT (`label_tests`, and `worst_label_ratio` = the largest error over tolerance in it).
--add-kernel-stats CSV does not time anything: it adds the k_augment_* rows of a `rocprofv3 --kernel-trace --stats` run of
this script (a run of its own, e.g. `--rounds 2 --inner 10 --out /dev/null`) to the document at --out as `kernel_trace`.

The buffers of every route are the same 25 MB + 25 MB in every launch, so they stay in the Infinity Cache (256 MiB): these
are warm-cache times, for the copy as for the own kernel.  The label rows come from the test tree's generator
(tests/augment_cases.py), the one place that makes such rows."""
import argparse
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def captured(fn, inner):
    """`inner` launches of fn in one graph: replayed, they run back to back on the device, so the host's time to issue a
    launch (about 10 us through ctypes, as long as these kernels run) is not in the figure"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    return graph


def per_launch_us(graph, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / inner


def summary(times):
    return {"median_us": round(statistics.median(times), 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2)}


def worst_ratio(report):
    """the largest error / tolerance among the label tests' figures (counts of rows are not ratios)"""
    worst = 0.0
    for value in report.values():
        ratios = [v for k, v in value.items() if k not in ("compared", "left_out", "rows")] if isinstance(value, dict) else [value]
        worst = max([worst] + [float(v) for v in ratios])
    return worst


def kernel_trace(stats_csv):
    rows = {}
    for r in csv.DictReader(open(stats_csv)):
        m = re.search(r"k_augment_\w+", r["Name"])
        if m:
            rows[m.group(0)] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                                "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    return {"what": "rocprofv3 --kernel-trace --stats over a run of this script of its own; k_augment_images over all elements",
            "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    ap.add_argument("--label-report", default=None)
    ap.add_argument("--add-kernel-stats", default=None)
    args = ap.parse_args()
    if args.add_kernel_stats:
        result = json.load(open(args.out))
        result["kernel_trace"] = kernel_trace(args.add_kernel_stats)
        json.dump(result, open(args.out, "w"), indent=1)
        print(json.dumps(result["kernel_trace"]))
        return
    import augment_cases as AC
    from s2anet_amd import TrainAugment, _lib as L
    dev = "cuda"
    B, S = args.batch, args.size
    torch.manual_seed(0)
    imgs = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev)
    out = torch.empty_like(imgs)
    aug = TrainAugment(degrees=180.0, flipud=0.0, fliplr=0.5, seed=0)
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    elements = [(r, 0, l) for r in range(4) for l in (0, 1)]
    tables = {e: torch.tensor([list(e) + [0]] * B, dtype=torch.int32, device=dev) for e in elements}
    mixed = aug.draw(B)
    lib = L.lib()

    def own(table):                                            # the image launch alone, as TrainAugment.apply issues it
        L.check(lib.s2a_augment_images_u8(L.ptr(imgs), L.ptr(table), B, S, S, L.ptr(out), L.stream_ptr(imgs.device)))

    routes = {"copy": lambda: out.copy_(imgs)}
    for e in elements:
        routes["own rot%d fliplr%d" % (e[0], e[2])] = (lambda t=tables[e]: own(t))
        k = {0: 0, 1: 1, 2: 2, 3: -1}[e[0]]          # rot 1: dst[y'][x'] = src[x'][S - y'], torch.rot90 by one turn over (H, W)

        def stock(k=k, flip=e[2]):
            v = torch.rot90(imgs, k, (1, 2)) if k else imgs
            if flip:
                v = v.flip(2)
            return v.contiguous() if (k or flip) else v.clone()
        routes["stock rot%d fliplr%d" % (e[0], e[2])] = stock
    routes["own mixed draw"] = lambda: own(mixed)
    params = torch.empty((B, 4), dtype=torch.int32, device=dev)
    routes["draw"] = lambda: aug.draw(B, out=params)
    for G in (240, 4096):
        lab = AC.label_cases(11, S, B, n=G)
        lab = torch.from_numpy(lab[:G]).to(dev)
        tgt = torch.empty((lab.shape[0], 7), device=dev)

        def labels(lab=lab, tgt=tgt):
            L.check(lib.s2a_augment_labels(L.ptr(lab), lab.shape[0], L.ptr(mixed), B, S, S, 0, L.ptr(tgt), L.ptr(status),
                                           L.stream_ptr(lab.device)))
        routes["labels G=%d" % lab.shape[0]] = labels

    times = {name: [] for name in routes}
    step0 = aug.step.clone()
    graphs = {name: captured(fn, args.inner) for name, fn in routes.items()}
    for g in graphs.values():                                  # warm-up
        g.replay()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, g in graphs.items():
            times[name].append(per_launch_us(g, args.inner))
    aug.step.copy_(step0)
    copy_us = statistics.median(times["copy"])
    nbytes = 2 * imgs.numel()
    result = {"shape": [B, S, S, 3], "rounds": args.rounds, "inner": args.inner, "bytes_moved": nbytes,
              "device": torch.cuda.get_device_name(0), "mixed_table": mixed[:, :3].tolist(), "routes": {}}
    for name, ts in times.items():
        row = summary(ts)
        if name == "copy" or name.startswith(("own", "stock")):
            row["over_copy"] = round(row["median_us"] / copy_us, 3)
            row["GB_per_s"] = round(nbytes / row["median_us"] / 1e3, 1)
        result["routes"][name] = row
    if args.label_report and os.path.exists(args.label_report):
        result["label_tests"] = json.load(open(args.label_report))
        result["worst_label_ratio"] = worst_ratio(result["label_tests"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
