#!/usr/bin/env python3
"""Time the S2ANet training loss at B = 8, 1024^2, 30 gts per image, f16 maps (tests/test_gpu_loss.py builds the
same batch):
  (a) the core: s2anet_loss forward + backward (3 launches, no host sync)
  (b) the whole S2ANetHead.compute_loss forward + backward, assignment (2*B assign_labels calls) included
  (d) the assignment alone, per-image route (S2ANetHead.assign_labels_fam_odm) and batched route (assign_labels_batched);
      compute_loss forward + backward with S2A_ASSIGN_BATCHED=0 and with the batched route; compute_loss_device +
      backward replayed from a captured graph.  The routes are interleaved in one process, three repetitions each:
      median of the repetitions' medians and their range
  (c) the reference's algorithm (models/head.py:353-646) restated with torch ops on the same GPU tensors: per level
      boolean-mask indexing, .item() counts, FocalLoss / SmoothL1Loss, autograd backward
Prints one JSON line; median wall time per iteration in microseconds (CUDA events, after warm-up)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def reference_form(head, p6, ts, ids):
    """compute_loss_single_level per level and module, as the reference writes it (masks, .item(), focal wrappers)"""
    B, C = p6[0][0].shape[0], head.num_classes
    off = [0]
    counts = torch.bincount(ts[:, 0].long(), minlength=B).tolist()
    for c in counts:
        off.append(off[-1] + c)
    levels = [a.shape[0] if a.dim() == 2 else a.shape[1] * a.shape[2] for a in p6[4]]
    totals = [max(int((ids[m] >= 0).sum().item()), B) for m in range(2)]
    losses = []
    for m in range(2):
        cls_tot = torch.zeros(1, device=ts.device)
        reg_tot = torch.zeros(1, device=ts.device)
        start = 0
        for l, n in enumerate(levels):
            idl = ids[m][:, start:start + n].reshape(-1)
            start += n
            cls = p6[2 * m][l].permute(0, 2, 3, 1).reshape(-1, C).float()
            box = p6[2 * m + 1][l].permute(0, 2, 3, 1).reshape(-1, 5).float()
            anc = p6[4 + m][l].reshape(-1, 5)
            if m == 0:
                anc = anc.repeat(B, 1)
            pos = idl >= 0
            img = torch.arange(B, device=ts.device).repeat_interleave(n)
            if pos.sum().item() > 0:
                rows = torch.tensor(off[:B], device=ts.device)[img[pos]] + idl[pos]
                gt = ts[rows]
                pa = anc[pos]
                ox, oy = gt[:, 2] - pa[:, 0], gt[:, 3] - pa[:, 1]
                ca, sa = torch.cos(pa[:, 4]), torch.sin(pa[:, 4])
                da = torch.remainder(gt[:, 6] - pa[:, 4] + math.pi / 4, math.pi) - math.pi / 4
                tgt = torch.stack([(ca * ox + sa * oy) / pa[:, 2], (-sa * ox + ca * oy) / pa[:, 3],
                                   torch.log(gt[:, 4] / pa[:, 2]), torch.log(gt[:, 5] / pa[:, 3]), da / math.pi], -1)
                d = (box[pos] - tgt).abs()
                reg_tot = reg_tot + head.FPN_balance[l] * torch.where(d < head.smoothL1_beta, 0.5 * d * d / head.smoothL1_beta,
                                                                      d - 0.5 * head.smoothL1_beta).sum()
                t = torch.zeros_like(cls[pos])
                t[range(int(pos.sum().item())), gt[:, 1].long()] = 1
                cls_tot = cls_tot + head.FPN_balance[l] * focal(cls[pos], t, head)
            neg = idl == -1
            if neg.sum().item() > 0:
                cls_tot = cls_tot + head.FPN_balance[l] * focal(cls[neg], torch.zeros_like(cls[neg]), head)
        bal = head.odm_balance if m else 1.0
        losses += [cls_tot / totals[m] * bal, reg_tot / totals[m] * head.reg_balance * bal]
    loss = losses[0] + losses[1] + losses[2] + losses[3]
    return loss, torch.cat(losses).detach().cpu().numpy()


def focal(x, t, head):
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    p = torch.sigmoid(x)
    p_t = t * p + (1 - t) * (1 - p)
    return (bce * (t * head.fl_alpha + (1 - t) * (1 - head.fl_alpha)) * (1.0 - p_t) ** head.fl_gamma).sum()


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


def interleaved(rows, steps, warmup, reps=3):
    """rows: name -> fn.  Every repetition times every row (A, B, ..., A, B, ...): -> name -> {median, min, max} over the
    repetitions' medians"""
    got = {k: [] for k in rows}
    for _ in range(reps):
        for k, fn in rows.items():
            got[k].append(timed(fn, steps, warmup))
    return {k: {"median": round(sorted(v)[len(v) // 2], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from test_gpu_loss import full_size_batch
    from s2anet_amd import s2anet_loss
    from s2anet_amd.head import S2ANetHead
    head = S2ANetHead(15)
    p, t = full_size_batch(seed=0, B=8, size=1024, n_gt=30, dtype=torch.float16)
    maps = [x for lst in p[:4] for x in lst]
    ids, ts, off = head.assign_labels_fam_odm(p, t)

    def core():
        loss, _ = s2anet_loss(*p, ids, ts, off)
        torch.autograd.grad(loss, maps)

    def whole():
        loss, _ = head.compute_loss(p, t)
        torch.autograd.grad(loss, maps)

    def reference():
        loss, _ = reference_form(head, p, ts, ids)
        torch.autograd.grad(loss, maps, allow_unused=True)

    res = {"workload": "s2anet_loss B=8 1024^2 30 gts/img f16 maps", "unit": "us (median)",
           "core_fwd_bwd": round(timed(core, args.steps, args.warmup), 1),
           "compute_loss_fwd_bwd": round(timed(whole, args.steps, args.warmup), 1),
           "reference_form_fwd_bwd": round(timed(reference, max(args.steps // 5, 3), 2), 1)}
    # (d) the two assignment routes, A/B in one process
    from s2anet_amd import assign_labels_batched
    from s2anet_amd.rotated import ASSIGN_PAIR_CAPACITY
    B = p[1][0].shape[0]

    def assign_batched():
        init_all = torch.cat([a.reshape(-1, 5) for a in p[4]], 0)
        refine_all = torch.cat([a.reshape(B, -1, 5) for a in p[5]], 1)
        return assign_labels_batched((init_all, refine_all), t, B, imgs_size=head.imgs_size)

    def route(value):
        def fn():
            os.environ["S2A_ASSIGN_BATCHED"] = value
            loss, _ = head.compute_loss(p, t)
            torch.autograd.grad(loss, maps)
        return fn

    def device_step():
        loss, items, status = head.compute_loss_device(p, t)
        return (loss, items, status, *torch.autograd.grad(loss, maps))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            device_step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = device_step()
    prior = os.environ.get("S2A_ASSIGN_BATCHED")
    ab = interleaved({"assign_per_image": lambda: head.assign_labels_fam_odm(p, t), "assign_batched": assign_batched,
                      "compute_loss_per_image_fwd_bwd": route("0"), "compute_loss_batched_fwd_bwd": route("1"),
                      "compute_loss_device_graph_replay": graph.replay}, args.steps, args.warmup)
    if prior is None:
        os.environ.pop("S2A_ASSIGN_BATCHED", None)
    else:
        os.environ["S2A_ASSIGN_BATCHED"] = prior
    res.update(ab)
    ids_b, _, _, status = assign_batched()
    graph.replay()
    torch.cuda.synchronize()
    res["assign_pairs_found"] = int(status[1])
    res["assign_pair_capacity_default"] = min(2 * ids.shape[2] * t.shape[0], ASSIGN_PAIR_CAPACITY)
    res["assign_routes_equal"] = bool(torch.equal(ids_b, ids)) and int(status[0]) == 0
    res["graph_replay_equals_eager"] = all(bool(torch.equal(a, b)) for a, b in zip(static, device_step()))
    l1, it1 = head.compute_loss(p, t)
    _, it2 = reference_form(head, p, ts, ids)
    res["items_core"] = [float(v) for v in it1]
    res["items_reference_form"] = [float(v) for v in it2]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
