#!/usr/bin/env python3
"""Time the entry of the training step with the third switch (train_kernels(..., entry=True)) on and off, protocol of
scripts/bench_train_conv.py: both routes in one process, interleaved, three repetitions of --steps steps each, median of the
repetitions' medians and their range, CUDA events after warm-up; per route also the device time of every kernel of one
iteration (torch.profiler).  f32 masters, f16 channels-last activations, every parameter gradient wanted.

  stem      forward + backward at 8 x 3 x 1024^2.  own: StemU8Function on the uint8 batch.  stock: img.half() / 255, F.conv2d
            under torch.autocast, ReLU, F.max_pool2d.  Also torch.cuda.max_memory_allocated of one step of each route above
            what was allocated before it (the batch, the parameters, the cotangent).
  top-down  FPN's top-down steps at the benchmark pyramid (batch 8, 1024^2: C3 512 x 128^2, C4 1024 x 64^2 -> 256 maps over a
            coarser level of half the size; a three-input FPN has these two).  own: FusedConvUp2Function.  stock: every switch
            off, the library 1x1 under torch.autocast + F.interpolate.  Input, weight, bias and coarse gradients.

Prints one JSON line (publish it as profiles/train_entry.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scripts.bench_train_conv import kernels, timed  # noqa: E402

TOP_DOWN = [("topdown_c4_1024_256_64", 1024, 256, 8, 64, 64), ("topdown_c3_512_256_128", 512, 256, 8, 128, 128)]


def measure(routes, steps, warmup):
    got = {r: [] for r in routes}
    for _ in range(3):
        for r, fn in routes.items():
            got[r].append(timed(fn, steps, warmup))
    row = {}
    for r, v in got.items():
        row[r] = {"median": round(sorted(v)[1], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
        try:
            row[r]["kernels"] = kernels(routes[r])
        except Exception as e:                              # the profiler is a convenience here, not the measurement
            row[r]["kernels"] = f"not measured: {type(e).__name__}: {e}"
    row["stock_over_own"] = round(row["stock"]["median"] / row["own"]["median"], 3)
    row["verdict"] = "own kernels faster" if row["stock_over_own"] > 1 else "own kernels LOSE to the library here"
    return row


def peak(fn):
    """bytes one call of fn allocates at its peak above what was allocated before it"""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d
    dev = torch.device("cuda:0")
    res = {"workload": "forward + backward, f32 masters, f16 NHWC activations, all gradients; entry switch on (own) and off (stock)",
           "unit": "us (median)", "layers": {}}

    # ---- the stem
    torch.manual_seed(0)
    B, H = args.batch, args.size
    conv = FusedConv2d(3, 64, 7, 2, 3, relu=True).to(dev)
    img = torch.randint(0, 256, (B, H, H, 3), device=dev, dtype=torch.uint8).permute(0, 3, 1, 2)
    Hp = ((H - 1) // 2 + 1 - 1) // 2 + 1
    cot = torch.randn((B, 64, Hp, Hp), device=dev).half().contiguous(memory_format=torch.channels_last)

    def stem_own():
        conv.zero_grad(set_to_none=True)
        S.StemU8Function.apply(img, conv.weight, conv.bias, 255.0).backward(cot)

    def stem_stock():
        conv.zero_grad(set_to_none=True)
        x = img.half() / 255
        with torch.autocast("cuda", torch.float16):
            y = F.max_pool2d(F.relu(F.conv2d(x, conv.weight, conv.bias, 2, 3)), 3, 2, 1)
        y.backward(cot)

    row = measure({"own": stem_own, "stock": stem_stock}, args.steps, args.warmup)
    row["peak_bytes"] = {"own": peak(stem_own), "stock": peak(stem_stock)}
    res["layers"]["stem_%dx3x%d" % (B, H)] = row

    # ---- the top-down steps
    for name, cin, cout, Bn, Hn, Wn in TOP_DOWN:
        torch.manual_seed(0)
        m = FusedConv2d(cin, cout, 1).to(dev)
        x = torch.randn((Bn, cin, Hn, Wn), device=dev).half().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        coarse = torch.randn((Bn, cout, Hn // 2, Wn // 2), device=dev).half().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        cot = torch.randn((Bn, cout, Hn, Wn), device=dev).half().contiguous(memory_format=torch.channels_last)
        assert S.train_up2_ok(x, m, coarse)

        def step(own, m=m, x=x, coarse=coarse, cot=cot):
            S.train_kernels(m, own, entry=True)
            x.grad = coarse.grad = None
            m.zero_grad(set_to_none=True)
            if own:
                y = S.FusedConvUp2Function.apply(x, m.weight, m.bias, coarse)
            else:
                with torch.autocast("cuda", torch.float16):
                    lat = m(x)
                y = lat + F.interpolate(coarse, scale_factor=2, mode="nearest")
            y.backward(cot)

        res["layers"][name] = measure({"own": lambda: step(True), "stock": lambda: step(False)}, args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
