"""Same-session measurement of the opt-in e4m3 tower route (csrc/conv_fp8_ops.hip) against the f16 route it replaces
-> profiles/conv_fp8.json (or the path given with --out).

  launches   the pyramid-packed 3x3 256 -> 256 launch on the benchmark pyramid (batch 8, 1024^2 chips: 128^2 ... 8^2):
             f16 (k_conv_f16<9,4,2>), fp8 with f16 out, fp8 with e4m3 out, and the quantise launch, alternating in one
             process, best of ROUNDS x 200, on zeros / ReLU-sparse / dense data (the clock the chip holds depends on the
             data); all rounds are kept, so the repeat spread of the f16 launch is in the file
  head       S2ANetHead.forward_pyramid and S2ANet.detect (one stream) with the mode off and on, alternating
  accuracy   largest err / bound of the fp8 launch against float64 (the bounds of tests/test_gpu_conv_fp8.py, small ragged
             pyramid), and the deviation of odm_cls / odm_bbox on the tests/golden/net_forward fixture (fixture anchors
             injected, S2A_OWN_CONV_ALWAYS=1 as tests/test_net_forward.py) with the mode on from the f16 path and from
             the f32 fixture.  Recorded, not asserted."""
import argparse
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import s2anet_amd as S  # noqa: E402
from s2anet_amd import pyramid as P  # noqa: E402
from s2anet_amd.fused import conv_pack_weight, conv_pack_weight_fp8  # noqa: E402
from s2anet_amd.pyramid import PyramidLayout  # noqa: E402

dev = torch.device("cuda:0")
F8 = torch.float8_e4m3fn


def timeit(f, n=200, warm=30):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        f()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n * 1e3


def summary(v):
    return {"us": round(min(v), 1), "all_us": [round(t, 1) for t in v], "spread_us": round(max(v) - min(v), 1)}


def bench_launches(rounds):
    layout = PyramidLayout(8, [(128, 128), (64, 64), (32, 32), (16, 16), (8, 8)], (8, 16, 32, 64, 128))
    g = torch.Generator().manual_seed(0)
    xr = torch.randn(layout.pixels, 256, generator=g).to(dev).half()
    w = (torch.randn(256, 256, 3, 3, generator=g) * 0.02).to(dev).half()
    b = torch.randn(256, generator=g).to(dev).half()
    out16, out8, q = layout.new(256, dev), layout.new(256, dev, torch.uint8), layout.new(256, dev, torch.uint8)
    res = {}
    for name, x, ww in (("zeros", torch.zeros_like(xr), torch.zeros_like(w)), ("relu-sparse", torch.relu(xr), w), ("dense", xr, w)):
        s_x = max(float(x.float().abs().max()), 1e-30) / 448 if name != "zeros" else 1.0
        wd = conv_pack_weight(ww)
        w8, sc = conv_pack_weight_fp8(ww, s_x)
        b32 = b.float()
        xq = P.quantize_e4m3(x, 1.0 / s_x)
        t = collections.defaultdict(list)
        for _ in range(rounds):
            t["f16"].append(timeit(lambda: P.conv3x3(layout, x, wd, b, 256, relu=True, out=out16)))
            t["fp8_f16_out"].append(timeit(lambda: P.conv3x3_fp8(layout, xq, w8, sc, b32, 256, True, out=out16)))
            t["fp8_e4m3_out"].append(timeit(lambda: P.conv3x3_fp8(layout, xq, w8, sc, b32, 256, True, True, 16.0, out=out8)))
            t["quantize"].append(timeit(lambda: P.quantize_e4m3(x, 1.0 / s_x, out=q)))
        res[name] = {k: summary(v) for k, v in t.items()}
        print(json.dumps({"data": name, **{k: v["us"] for k, v in res[name].items()}}), flush=True)
    return res


def bench_head(rounds):
    from s2anet_amd.detector import build_synthetic_detector
    model = build_synthetic_detector(device=dev)
    model.head.odm_cls_head.bias.data.fill_(-2.0)
    model.head.odm_cls_head.weight.data.mul_(20.0)
    imgs = torch.randint(0, 256, (8, 3, 1024, 1024), dtype=torch.uint8, device=dev,
                         generator=torch.Generator(dev).manual_seed(1)).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        scales = S.calibrate_fp8(model, [imgs])
        tr = {}
        model.features_to_pred(imgs, model.backbone.forward_u8(imgs, 255.0), trace=tr)
        layout, x = tr["layout"], tr["x"]
        t = collections.defaultdict(list)
        for _ in range(rounds):
            for mode in (False, True):
                S.fp8_towers(model, mode)
                k = "fp8" if mode else "f16"
                t["forward_pyramid_" + k].append(timeit(lambda: model.head.forward_pyramid(layout, x), 50, 10))
                t["detect_" + k].append(timeit(lambda: model.detect(imgs), 20, 5))
        S.fp8_towers(model, False)
    res = {k: summary(v) for k, v in t.items()}
    res["scales"] = scales
    print(json.dumps({k: v["us"] for k, v in res.items() if k != "scales"}), flush=True)
    return res


def accuracy_launch():
    from oracle.conv64 import conv64
    layout = PyramidLayout(2, [(20, 28), (10, 14), (5, 7), (3, 3)], (8, 16, 32, 64))
    g = torch.Generator().manual_seed(1)
    xq = torch.randn(layout.pixels, 256, generator=g).clamp(-448, 448).to(F8)
    wq = (torch.randn(256, 256, 3, 3, generator=g) / 48).to(F8)
    scale, bias = torch.rand(256, generator=g) * 1.5 + 0.5, torch.randn(256, generator=g) * 0.5
    packed = torch.empty(wq.numel(), dtype=torch.uint8, device=dev)
    wdev = wq.view(torch.uint8).to(dev)
    S._lib.check(S._lib.lib().s2a_conv_pack_weight_fp8(S._lib.ptr(wdev), 256, 256, S._lib.ptr(packed), S._lib.stream_ptr(dev)))
    got = P.conv3x3_fp8(layout, xq.view(torch.uint8).to(dev), packed, scale.to(dev), bias.to(dev), 256, relu=False)
    w64 = wq.float().double() * scale.double().view(-1, 1, 1, 1)
    worst = 0.0
    for l in range(len(layout.sizes)):
        y, Sa = conv64(layout.level(xq.float().double(), l), w64, bias.double(), 1, 3)
        err = (layout.level(got, l).cpu().double() - y).abs()
        worst = max(worst, (err / ((2.0 ** -11 + 2 * (2304 + 3) * 2.0 ** -24) * Sa + 2.0 ** -25)).max().item())
    return {"f16_out_max_err_over_bound": round(worst, 4), "bound": "(2^-11 + 2 (K + 3) 2^-24) S + 2^-25, K = 2304"}


def accuracy_fixture():
    import synth_net
    from conftest import golden
    from s2anet_amd.detector import S2ANet, fold_batchnorm, fuse_epilogues, load_reference_checkpoint
    os.environ["S2A_OWN_CONV_ALWAYS"] = "1"
    g = golden("net_forward.npz")
    names = [str(n) for n in g["names"]]
    shapes = [tuple(int(v) for v in str(s).split(",") if v) for s in g["shapes"]]
    fixed = {str(n): g["fixed:" + str(n)] for n in g["fixed_names"]}
    scales = {str(n): float(v) for n, v in zip(g["scale_names"], g["scale_values"])}
    state = synth_net.synth_state(names, shapes, [str(d) for d in g["dtypes"]], fixed, scales, seed=int(g["seed"]))
    imgs = synth_net.synth_images(int(g["batch"]), int(g["size"]), int(g["size"]), seed=int(g["seed"]))
    torch.manual_seed(0)
    m = S2ANet(15)
    load_reference_checkpoint(m, {"state_dict": collections.OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in state.items())})
    m = fuse_epilogues(fold_batchnorm(m.eval())).to(dev, torch.float16)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d) and mod.weight.dim() == 4 and mod.weight.shape[1] >= 8:
            mod.weight.data = mod.weight.data.contiguous(memory_format=torch.channels_last)
    m.head.or_conv.channels_last = True
    imgs = torch.from_numpy(imgs).to(dev).contiguous(memory_format=torch.channels_last)
    anc = torch.cat([torch.from_numpy(g[f"refine_anchors_{l}"]).reshape(-1, 5) for l in range(5)], 0).float().to(dev).contiguous()
    out = {}
    with torch.no_grad():
        cal = S.calibrate_fp8(m, [imgs])
        preds = {}
        for mode in (False, True):
            S.fp8_towers(m, mode)
            preds[mode] = m.features_to_pred(imgs, m.backbone.forward_u8(imgs, 255.0), anchors=anc)
        S.fp8_towers(m, False)
    for i, key in ((2, "odm_cls"), (3, "odm_bbox")):
        d_on_off = d_off_fx = d_on_fx = 0.0
        for l in range(5):
            ref = torch.from_numpy(g[f"{key}_{l}"]).double()
            off, on = preds[False][i][l].cpu().double(), preds[True][i][l].cpu().double()
            d_on_off = max(d_on_off, (on - off).abs().max().item())
            d_off_fx = max(d_off_fx, (off - ref).abs().max().item())
            d_on_fx = max(d_on_fx, (on - ref).abs().max().item())
        out[key] = {"fp8_vs_f16_max": round(d_on_off, 5), "f16_vs_f32_fixture_max": round(d_off_fx, 5),
                    "fp8_vs_f32_fixture_max": round(d_on_fx, 5)}
    out["scales"] = cal
    out["note"] = "fixture anchors injected; maximum over all positions and levels; synthetic weights, no mAP"
    os.environ.pop("S2A_OWN_CONV_ALWAYS")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_fp8.json"))
    ap.add_argument("--skip", default="", help="comma list of: launches, head, accuracy")
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds}
    if "accuracy" not in skip:
        res["accuracy_launch"] = accuracy_launch()
        res["accuracy_fixture"] = accuracy_fixture()
        print(json.dumps({"accuracy_launch": res["accuracy_launch"], "accuracy_fixture": res["accuracy_fixture"]}), flush=True)
    if "launches" not in skip:
        res["launches"] = bench_launches(a.rounds)
    if "head" not in skip:
        res["head"] = bench_head(a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
