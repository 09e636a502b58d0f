#!/usr/bin/env python3
"""Time the training update on the parameter set of the full unfused f32 S2ANet(15), synthetic gradients:
  (a) the stock sequence as the reference writes it (train.py:358-373): GradScaler.unscale_, clip_grad_norm_(35),
      scaler.step(SGD, three groups, Nesterov), scaler.update, zero_grad, ModelEMA.update restated
  (b) TrainUpdate.step() eager
  (c) TrainUpdate.step() replayed from a captured graph
The routes are interleaved in one process, three repetitions each: median of the repetitions' medians and their range,
CUDA events after warm-up.  Every timed iteration starts from the same gradients; refilling them (what a backward does)
is outside the timed window for all three routes.
Also: tensor / element counts, the algorithmic bytes (one read of the gradients for the norm, one pass over p, g, buf,
ema: 36 B per trained element, 12 B per ema-only element), the achieved fraction of the 6.3 TB/s copy bound,
kernel launches per iteration (torch.profiler), and the worst error / bound of tests/test_gpu_optim.py's parity run.
Prints one JSON line."""
import argparse
import copy
import io
import json
import math
import os
import sys
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

COPY_BOUND = 6.3e12   # B/s, DESIGN.md 5a


def timed(prepare, fn, steps, warmup):
    for _ in range(warmup):
        prepare()
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return times[len(times) // 2]


def launches(prepare, fn):
    """device kernels of one iteration, counted by torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    prepare()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from s2anet_amd import TrainUpdate, reference_param_groups
    from s2anet_amd.detector import S2ANet
    dev = "cuda"

    def make():
        torch.manual_seed(0)
        model = S2ANet(15).to(dev).train()
        return model, copy.deepcopy(model).eval()

    gen = torch.Generator().manual_seed(1)
    scale = 65536.0

    # ---- (a) stock
    model_a, ema_a = make()
    for p in ema_a.parameters():
        p.requires_grad_(False)
    params_a = [p for p in model_a.parameters() if p.requires_grad]
    src = [(torch.randn(p.shape, generator=gen) * 1e-3 * scale).to(dev) for p in params_a]      # norm << 35 x scale
    hold_a = [torch.empty_like(p) for p in params_a]
    groups = reference_param_groups(model_a, 0.01, 5e-4)
    sgd = torch.optim.SGD(groups[0]["params"], lr=0.01, momentum=0.937, nesterov=True)
    sgd.add_param_group({"params": groups[1]["params"], "weight_decay": 5e-4})
    sgd.add_param_group({"params": groups[2]["params"]})
    scaler = torch.amp.GradScaler("cuda")
    scaler.scale(torch.zeros(1, device=dev))
    ema_state = {"updates": 0}

    def prepare_a():
        torch._foreach_copy_(hold_a, src)
        for p, g in zip(params_a, hold_a):
            p.grad = g

    def stock():
        scaler.unscale_(sgd)
        torch.nn.utils.clip_grad_norm_(filter(lambda p: p.requires_grad, model_a.parameters()), max_norm=35, norm_type=2)
        scaler.step(sgd)
        scaler.update()
        sgd.zero_grad()
        with torch.no_grad():
            ema_state["updates"] += 1
            d = 0.9999 * (1 - math.exp(-ema_state["updates"] / 2000))
            msd = model_a.state_dict()
            for k, v in ema_a.state_dict().items():
                if v.dtype.is_floating_point:
                    v *= d
                    v += (1 - d) * msd[k].detach()

    # ---- (b) eager, (c) replayed
    def ours():
        model, ema = make()
        upd = TrainUpdate(reference_param_groups(model, 0.01, 5e-4), model, ema, momentum=0.937)
        grads = [p.grad for p in model.parameters() if p.requires_grad]
        return model, upd, (lambda: torch._foreach_copy_(grads, src))

    model_b, upd_b, prepare_b = ours()
    model_c, upd_c, prepare_c = ours()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            prepare_c()
            upd_c.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        upd_c.step()

    routes = {"stock": (prepare_a, stock), "train_update_eager": (prepare_b, upd_b.step), "train_update_graph": (prepare_c, graph.replay)}
    got = {k: [] for k in routes}
    for _ in range(3):
        for k, (prep, fn) in routes.items():
            got[k].append(timed(prep, fn, args.steps, args.warmup))
    res = {"workload": "training update, S2ANet(15) f32 unfused parameter set, synthetic gradients", "unit": "us (median)"}
    for k, v in got.items():
        res[k] = {"median": round(sorted(v)[1], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    trained = sum(upd_b.params[i].numel() for i in upd_b.trained)
    res["tensors"] = {"trained": len(upd_b.trained), "ema_only": upd_b.n_tensors - len(upd_b.trained), "chunks": upd_b.n_chunks}
    res["elements"] = {"trained": trained, "ema_only": upd_b.n_elements - trained}
    res["algorithmic_bytes"] = 36 * trained + 12 * (upd_b.n_elements - trained)
    for k in ("train_update_eager", "train_update_graph"):
        res[k]["fraction_of_copy_bound"] = round(res["algorithmic_bytes"] / COPY_BOUND / (res[k]["median"] * 1e-6), 3)
        res[k]["speedup_over_stock"] = round(res["stock"]["median"] / res[k]["median"], 2)
    res["launches"] = {}
    for k, (prep, fn) in routes.items():
        try:
            res["launches"][k] = launches(prep, fn)
        except Exception as e:                                       # the profiler is a convenience here, not the measurement
            res["launches"][k] = f"not measured: {type(e).__name__}: {e}"
    res["launches"]["train_update_by_construction"] = 3
    torch.cuda.synchronize()
    res["stats_last_step"] = dict(zip(("grad_norm", "clip", "found_inf", "skip_update", "scale", "ema_decay", "updates",
                                       "growth_tracker"), [float(v) for v in upd_b.stats.tolist()]))
    from test_gpu_optim import check_against_twin, shared
    specs, gpu, f64, f32 = shared()
    worst = [0.0]
    with redirect_stdout(io.StringIO()):
        for step, (g, w, s) in enumerate(zip(gpu, f64, f32)):
            check_against_twin(specs, g, w, s, f"step {step}", worst)
    res["parity_worst_error_over_bound"] = round(worst[0], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
