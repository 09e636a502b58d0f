#!/usr/bin/env python3
"""Time the forward + backward of ONE FusedConv2d layer (f32 masters, f16 channels-last activations, every gradient
wanted) with own_grad on (FusedConvFunction: the project's kernels) and off (the unchanged route: library convolution +
stock epilogue ops under torch.autocast), in the same process, interleaved, three repetitions each: median of the
repetitions' medians and their range, CUDA events after warm-up.
Layers: the head tower (3x3, 256 -> 256, ReLU) on each pyramid level at batch 8 (128^2 ... 8^2), and the trunk's 1x1
layers at their benchmark sizes (64 -> 256 at 256^2, 512 -> 128 at 128^2, 1024 -> 256 at 64^2; bias + ReLU).
The eight stride-2 layers of the R-50-FPN detector at the benchmark's shapes (batch 8, 1024^2 input): conv2 (3x3 / s2) and
downsample (1x1 / s2) of layer{2,3,4}[0], and the neck's two extra levels (3x3 / s2); for them "own" is
train_kernels(m, True, strided=True) (FusedConvS2Function) and "stock" is both switches off.
Per layer also the device time of every kernel of one iteration of each route (torch.profiler).
Prints one JSON line (publish it as profiles/train_conv.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# (name, k, cin, cout, B, H, W of the INPUT, stride)
LAYERS = [("tower3x3_256_256_%d" % s, 3, 256, 256, 8, s, s, 1) for s in (128, 64, 32, 16, 8)] + \
         [("trunk1x1_64_256_256", 1, 64, 256, 8, 256, 256, 1), ("trunk1x1_512_128_128", 1, 512, 128, 8, 128, 128, 1),
          ("trunk1x1_1024_256_64", 1, 1024, 256, 8, 64, 64, 1)] + \
         [("s2_layer2_conv2_3x3_128_128_256", 3, 128, 128, 8, 256, 256, 2), ("s2_layer3_conv2_3x3_256_256_128", 3, 256, 256, 8, 128, 128, 2),
          ("s2_layer4_conv2_3x3_512_512_64", 3, 512, 512, 8, 64, 64, 2), ("s2_layer2_down_1x1_256_512_256", 1, 256, 512, 8, 256, 256, 2),
          ("s2_layer3_down_1x1_512_1024_128", 1, 512, 1024, 8, 128, 128, 2), ("s2_layer4_down_1x1_1024_2048_64", 1, 1024, 2048, 8, 64, 64, 2),
          ("s2_fpn3_3x3_2048_256_32", 3, 2048, 256, 8, 32, 32, 2), ("s2_fpn4_3x3_256_256_16", 3, 256, 256, 8, 16, 16, 2)]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return times[len(times) // 2]


def kernels(fn):
    """{kernel name: device us} of one iteration"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            out[e.name[:96]] = round(out.get(e.name[:96], 0.0) + e.device_time, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import s2anet_amd as S
    from s2anet_amd.fused import FusedConv2d
    dev = torch.device("cuda:0")
    res = {"workload": "forward + backward of one FusedConv2d, f32 masters, f16 NHWC activations, all gradients",
           "unit": "us (median)", "layers": {}}
    for name, k, cin, cout, B, H, W, stride in LAYERS:
        if args.only and args.only not in name:
            continue
        torch.manual_seed(0)
        m = FusedConv2d(cin, cout, k, stride, k // 2, relu=True).to(dev)
        x = torch.randn((B, cin, H, W), device=dev).half().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        cot = torch.randn((B, cout, Ho, Wo), device=dev).half().contiguous(memory_format=torch.channels_last)
        assert S.train_conv_ok(x, m, None) if stride == 1 else S.train_conv_strided_ok(x, m, None)

        def step(own, m=m, x=x, cot=cot, stride=stride):
            S.train_kernels(m, own, strided=stride == 2)
            x.grad = None
            m.zero_grad(set_to_none=True)
            with torch.autocast("cuda", torch.float16, enabled=not own):
                y = m(x)
            y.backward(cot)

        routes = {"own": lambda: step(True), "stock": lambda: step(False)}
        got = {r: [] for r in routes}
        for _ in range(3):
            for r, fn in routes.items():
                got[r].append(timed(fn, args.steps, args.warmup))
        row = {}
        for r, v in got.items():
            row[r] = {"median": round(sorted(v)[1], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            try:
                row[r]["kernels"] = kernels(routes[r])
            except Exception as e:                          # the profiler is a convenience here, not the measurement
                row[r]["kernels"] = f"not measured: {type(e).__name__}: {e}"
        row["stock_over_own"] = round(row["stock"]["median"] / row["own"]["median"], 3)
        row["verdict"] = "own kernels faster" if row["stock_over_own"] > 1 else "own kernels LOSE to the library here"
        res["layers"][name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
