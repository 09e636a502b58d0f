#!/usr/bin/env python3
"""Time the own training-mode BatchNorm (s2anet_amd.batch_norm_train, csrc/bn_ops.hip) against the stock route -- the same
nn.BatchNorm2d with the stock add and ReLU on the same f16 channels-last tensors -- in one process, the two routes
alternating, three repetitions each: median of the repetitions' medians and their range, CUDA events after warm-up (the
protocol of scripts/bench_train_conv.py).  f32 masters, every gradient wanted.

  * forward + backward of BN + residual + ReLU (and of BN + ReLU) at the trunk's batch-8 shapes of the 1024^2 step:
    64 @ 256^2, 256 @ 256^2, 128 @ 128^2, 512 @ 128^2, 1024 @ 64^2, 2048 @ 32^2;
  * forward + backward of one whole unfolded layer2[0] (256 -> 128 -> 512, stride 2, downsample) at batch 8, 256^2 input:
    own = train_batchnorm(block) (own convolutions and own norms), stock = the block as it runs without the flag, under
    torch.autocast;
  * per case the device time of every kernel of one iteration of each route (torch.profiler), the four passes' algorithmic
    bytes and those bytes over the HBM peak, and torch.cuda.max_memory_allocated of one step of each route.

No speed is promised: the comparison is the stock route on the same box in the same process.  Prints one JSON line
(publish it as profiles/train_bn.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_train_conv import kernels, timed  # noqa: E402

HBM_PEAK_GBPS = 8000.0          # MI355X: 8 TB/s HBM3E peak
SHAPES = [(64, 256), (256, 256), (128, 128), (512, 128), (1024, 64), (2048, 32)]    # (channels, side) at batch 8
CL = torch.channels_last


def pass_bytes(P, C, relu, res):
    """algorithmic HBM bytes of each pass on [P, C] f16 (vectors and partials left out: they are C-sized)"""
    t = P * C * 2
    return {"stats": t,                                               # read x
            "apply": t * (2 + int(res)),                              # read x (+ residual), write out
            "backward_reduce": t * (2 + int(relu) + int(relu and res)),   # read grad_out, x (+ out), write g when the residual wants it
            "backward_input": t * 3}                                  # read g, x, write dx (the mask is in g when g was written)


def peak_memory(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return {"max_memory_allocated": torch.cuda.max_memory_allocated(), "allocated_before": base}


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
        row[r]["memory"] = peak_memory(routes[r])
    row["stock_over_own"] = round(row["stock"]["median"] / row["own"]["median"], 3)
    row["verdict"] = "own kernels faster" if row["stock_over_own"] > 1 else "own kernels LOSE to the stock route here"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import s2anet_amd as S
    from s2anet_amd.detector import BottleNeck
    dev = torch.device("cuda:0")
    res = {"workload": "forward + backward of training-mode BatchNorm2d, f32 masters, f16 NHWC activations, all gradients",
           "unit": "us (median)", "hbm_peak_GBps": HBM_PEAK_GBPS, "layers": {}}
    B = 8
    for C, side in SHAPES:
        for relu, with_res in ((True, True), (True, False)):
            name = "bn%s_relu_%d_%d" % ("_res" if with_res else "", C, side)
            if args.only and args.only not in name:
                continue
            torch.manual_seed(0)
            bn = nn.BatchNorm2d(C).to(dev).train()
            x = torch.randn((B, C, side, side), device=dev).half().contiguous(memory_format=CL).requires_grad_(True)
            r = torch.randn((B, C, side, side), device=dev).half().contiguous(memory_format=CL).requires_grad_(True) if with_res else None
            cot = torch.randn((B, C, side, side), device=dev).half().contiguous(memory_format=CL)
            assert S.train_bn_ok(x, bn, r)

            def step(own, bn=bn, x=x, r=r, cot=cot, relu=relu):
                x.grad = None
                if r is not None:
                    r.grad = None
                bn.zero_grad(set_to_none=True)
                if own:
                    y = S.batch_norm_train(x, bn, r, relu)
                else:
                    y = bn(x)
                    if r is not None:
                        y = y + r
                    y = F.relu(y) if relu else y
                y.backward(cot)

            row = measure({"own": lambda: step(True), "stock": lambda: step(False)}, args.steps, args.warmup)
            P = B * side * side
            by = pass_bytes(P, C, relu, with_res)
            row["algorithmic_bytes"] = by
            row["bytes_over_hbm_peak_us"] = {k: round(v / (HBM_PEAK_GBPS * 1e3), 1) for k, v in by.items()}
            row["slices"] = S._lib.lib().s2a_bn_slices(P, C)
            res["layers"][name] = row
            del bn, x, r, cot
    if not args.only or args.only in "layer2_0":
        torch.manual_seed(0)
        down = nn.Sequential(nn.Conv2d(256, 512, 1, 2, bias=False), nn.BatchNorm2d(512))
        blk = BottleNeck(256, 128, 2, down).to(dev).train()
        for m in blk.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data = m.weight.data.contiguous(memory_format=CL)
        x = torch.randn((B, 256, 256, 256), device=dev).half().contiguous(memory_format=CL).requires_grad_(True)
        cot = torch.randn((B, 512, 128, 128), device=dev).half().contiguous(memory_format=CL)

        def block_step(own):
            S.train_batchnorm(blk, own)
            x.grad = None
            blk.zero_grad(set_to_none=True)
            with torch.autocast("cuda", torch.float16, enabled=not own):
                assert blk._own_norm_ok(x) == own
                y = blk(x)
            y.backward(cot)

        res["layers"]["layer2_0_block_256_128_512_s2"] = measure({"own": lambda: block_step(True), "stock": lambda: block_step(False)},
                                                               args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
