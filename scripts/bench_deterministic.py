#!/usr/bin/env python3
"""The price of deterministic mode (s2anet_amd.deterministic), measured in one process with the two modes alternating:
medians of three repetitions' medians after warm-up (CUDA events), and the device time of every kernel of one iteration
of each mode (torch.profiler).
  (a) the f16 one-call deformable backward (s2a_deform_conv_backward_typed) at the benchmarked call: B 8, 256 -> 256, 128^2;
  (b) the head's forward + compute_loss_device + backward on the benchmark pyramid (128^2 ... 8^2) at batch 8, f16
      parameters, train_kernels on: mode off (the narrow layers and ORConv2d on the library, f32 atomics in AlignConv's
      input gradient) against mode on (every layer on the own kernels, fixed-point accumulation).
--dcn-report: the JSON tests/test_gpu_deterministic_dcn.py writes (S2A_DETERMINISTIC_REPORT), embedded as "dcn_tests".
Prints one JSON line (publish it as profiles/deterministic.json)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from scripts.bench_train_conv import kernels, timed  # noqa: E402


def alternate(step, steps, warmup, reps=3):
    """-> {"off": {...}, "on": {...}, "on_over_off": ratio}; step(mode) runs one iteration in that mode"""
    got = {"off": [], "on": []}
    for _ in range(reps):
        for name, mode in (("off", False), ("on", True)):
            got[name].append(timed(lambda: step(mode), steps, warmup))
    row = {}
    for name, v in got.items():
        v = sorted(v)
        row[name] = {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
        try:
            row[name]["kernels"] = kernels(lambda: step(name == "on"))
        except Exception as e:                              # the profiler is a convenience here, not the measurement
            row[name]["kernels"] = f"not measured: {type(e).__name__}: {e}"
    row["on_over_off"] = round(row["on"]["median"] / row["off"]["median"], 3)
    return row


def dcn_case(dev):
    import s2anet_amd as S
    from s2anet_amd.alignconv import align_offsets
    from s2anet_amd.dcn import _fused_backward
    from s2anet_amd.loss import grid_anchors
    B, C, O, H, W, stride = 8, 256, 256, 128, 128, 8
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn((B, C, H, W), device=dev, generator=g).half()
    w = (torch.randn((O, C, 3, 3), device=dev, generator=g) / math.sqrt(9 * C)).half()
    a = grid_anchors((H, W), stride, 4.0, dev).view(1, H, W, 5).repeat(B, 1, 1, 1)
    a[..., :2] += torch.randn((B, H, W, 2), device=dev, generator=g) * 3
    a[..., 2:4] *= torch.exp(torch.randn((B, H, W, 2), device=dev, generator=g) * 0.3)
    a[..., 4] = torch.rand((B, H, W), device=dev, generator=g) * 3.0 - 0.7
    off = align_offsets(a.view(B, H * W, 5), (H, W), stride).half()
    go = torch.randn((B, O, H, W), device=dev, generator=g).half()

    def step(mode):
        with S.deterministic(mode):
            _fused_backward(x, off, w, go)
    return step


def head_case(dev):
    import s2anet_amd as S
    from s2anet_amd.detector import fuse_epilogues
    from s2anet_amd.head import S2ANetHead
    B, sizes = 8, (128, 64, 32, 16, 8)
    torch.manual_seed(0)
    head = S2ANetHead(15).train()
    fuse_epilogues(head)
    head = head.to(dev, torch.float16)
    head.or_conv.channels_last = True
    head.imgs_size = (1024, 1024)
    S.train_kernels(head)
    g = torch.Generator(device=dev).manual_seed(1)
    feats = [torch.randn((B, 256, s, s), device=dev, generator=g).half().contiguous(memory_format=torch.channels_last)
             .requires_grad_(True) for s in sizes]
    n = B * 30
    t = torch.empty((n, 7), device=dev)
    t[:, 0] = torch.arange(B, device=dev).repeat_interleave(30).float()
    t[:, 1] = torch.randint(0, 15, (n,), device=dev, generator=g).float()
    t[:, 2:4] = torch.rand((n, 2), device=dev, generator=g) * 1024
    t[:, 4:6] = 8 + torch.rand((n, 2), device=dev, generator=g) * 200
    t[:, 6] = (torch.rand((n,), device=dev, generator=g) - 0.25) * math.pi

    def step(mode):
        for f in feats:
            f.grad = None
        head.zero_grad(set_to_none=True)
        with S.deterministic(mode):
            loss, _, _ = head.compute_loss_device(head(feats)["pred"], t)
            (loss * 1024.0).backward()                       # (a loss scale, as f16 training has: unscaled, many gradients underflow to 0)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="dcn / head")
    ap.add_argument("--dcn-report", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"what": "deterministic mode on against off, the same process, modes alternating", "unit": "us (median)"}
    if args.only in ("", "dcn"):
        res["dcn_backward_f16_8x256x256_128x128"] = alternate(dcn_case(dev), args.steps, args.warmup)
    if args.only in ("", "head"):
        res["head_step_batch8_pyramid1024"] = alternate(head_case(dev), max(3, args.steps // 2), args.warmup)
    if args.dcn_report and os.path.exists(args.dcn_report):
        with open(args.dcn_report) as f:
            res["dcn_tests"] = json.load(f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
