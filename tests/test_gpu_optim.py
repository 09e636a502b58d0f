"""GPU: TrainUpdate (csrc/optim_ops.hip) against the float64 twin of tests/optim_twin.py.

Tolerance of the parity tests, per tensor: max abs error against the twin <= 4 x the error of the stock float32 torch
route (the same twin class in float32, on the CPU) against the same twin + one float32 ulp of the tensor's largest
magnitude.  The factor covers FMA contraction and the other summation order of the norm.
Gradient norm: a chunk's sum of squares is 16 sequential additions per thread and 8 tree levels of non-negative terms,
the unscale and the square add 2 roundings: relative error <= 26 x 2^-24 on the sum, half of it after the root, one more
rounding for the stored float32 -> asserted at 16 x 2^-24 relative.
"""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from optim_twin import Spec, Twin, max_err, ulp32

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 4096
STEPS, INF_STEP, NAN_STEP = 12, 5, 8
GROUPS = [dict(lr=0.0, weight_decay=0.0, momentum=0.9, nesterov=True),
          dict(lr=0.01, weight_decay=1e-4, momentum=0.9, nesterov=True),
          dict(lr=0.01, weight_decay=0.0, momentum=0.8, nesterov=False)]
# (size, group): 1, 3, 4, 5, 63, 64, 65, 1023, chunk - 1, chunk, chunk + 1, 3 chunks + 7; "view" sits at an odd element offset
SIZES = [(1, 0), (4, 0), (63, 0), (1023, 0), (3, 1), (64, 1), (CHUNK - 1, 1), (CHUNK, 1), (5, 2), (65, 2), (CHUNK + 1, 2)]
VIEW, LAST = "view", "last"
KW = dict(growth_interval=3, ema_tau=20.0)


def make_specs():
    g = torch.Generator().manual_seed(11)
    specs = [Spec(f"t{n}", torch.randn(n, generator=g), "param", grp) for n, grp in SIZES]
    specs.insert(7, Spec(VIEW, torch.randn(2 * CHUNK + 5, generator=g), "param", 1))
    specs.append(Spec(LAST, torch.randn(3 * CHUNK + 7, generator=g), "param", 2))
    specs += [Spec("frozen", torch.randn(37, generator=g), "frozen"), Spec("stat", torch.randn(19, generator=g), "buffer"),
              Spec("count", torch.tensor(3, dtype=torch.int64), "int")]
    return specs


class Holder(nn.Module):
    """the specs as a module: parameters (one a view at element offset 1 of a flat buffer), a frozen parameter, a
    floating and an int64 buffer"""

    def __init__(self, specs):
        super().__init__()
        for s in specs:
            v = s.init.to(DEV)
            if s.kind in ("buffer", "int"):
                self.register_buffer(s.name, v.clone())
            elif s.name == VIEW:
                flat = torch.zeros(v.numel() + 3, device=DEV)
                flat[1:1 + v.numel()] = v
                self.register_parameter(s.name, nn.Parameter(flat[1:1 + v.numel()]))
            else:
                self.register_parameter(s.name, nn.Parameter(v.clone(), requires_grad=s.kind == "param"))


def build(specs, ema=True, **kw):
    from s2anet_amd import TrainUpdate
    model = Holder(specs)
    view = getattr(model, VIEW)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    view.grad = torch.zeros(view.numel() + 3, device=DEV)[1:1 + view.numel()]        # an unaligned gradient too
    avg = copy.deepcopy(model).eval() if ema else None
    groups = [{"params": [getattr(model, s.name) for s in specs if s.kind == "param" and s.group == gi], **g}
              for gi, g in enumerate(GROUPS)]
    upd = TrainUpdate(groups, model if ema else None, avg, **{**KW, **kw})
    return model, avg, upd


def step_inputs(specs, step, scale, gen, inf=True):
    """gradients as a backward would leave them (x scale), lrs of the warm-up ramp, the new BN statistic"""
    from s2anet_amd import reference_lr
    sigma = 3.0 if step % 2 else 0.01                          # norm = 184 sigma: >> 35 and << 35 alternate
    grads = {s.name: torch.randn(s.init.shape, generator=gen) * sigma * scale for s in specs if s.kind == "param"}
    if inf and step == INF_STEP:
        grads[LAST][-1] = float("inf")
    if inf and step == NAN_STEP:
        grads[VIEW][2 * CHUNK + 1] = float("nan")
    lr = reference_lr(step, STEPS, 0.01, 1.0)
    return grads, [0.0, lr, lr], torch.randn(19, generator=gen)


def gpu_step(model, upd, grads, lrs, stat, skip=None):
    for n, g in grads.items():
        getattr(model, n).grad.copy_(g)
    model.stat.copy_(stat)
    upd.set_lr(lrs)
    upd.step(skip)


def snapshot(specs, model, avg, upd):
    snap = {"stats": upd.stats.cpu().numpy().copy(), "scale": float(upd.scale.item()), "counters": upd.counters.tolist()}
    for s in specs:
        p = getattr(model, s.name)
        snap["p/" + s.name] = p.detach().cpu().clone()
        if avg is not None:
            snap["ema/" + s.name] = getattr(avg, s.name).detach().cpu().clone()
        if s.kind == "param":
            snap["buf/" + s.name] = upd.momentum_buffer(p).cpu().clone()
            snap["grad/" + s.name] = p.grad.cpu().clone()
    return snap


def run_gpu(specs, inf=True, **kw):
    model, avg, upd = build(specs, **kw)
    gen = torch.Generator().manual_seed(5)
    snaps, scale = [], 65536.0 if upd.scaling else 1.0
    for step in range(STEPS):
        grads, lrs, stat = step_inputs(specs, step, scale, gen, inf)
        gpu_step(model, upd, grads, lrs, stat)
        snaps.append(snapshot(specs, model, avg, upd))
        scale = snaps[-1]["scale"]
    return snaps


def run_twin(specs, dtype, inf=True, **kw):
    """-> per step (twin state copies, info); the scale fed to the gradients is the twin's own"""
    twin = Twin(specs, GROUPS, dtype=dtype, **{**KW, **kw})
    gen = torch.Generator().manual_seed(5)
    out = []
    for step in range(STEPS):
        grads, lrs, stat = step_inputs(specs, step, twin.scale, gen, inf)
        info = twin.step(grads, lrs, buffers={"stat": stat})
        state = {"scale": twin.scale, "growth_tracker": twin.growth_tracker, "updates": twin.updates, **info}
        for s in specs:
            state["p/" + s.name] = twin.value[s.name].detach().clone()
            if twin.ema is not None:
                state["ema/" + s.name] = twin.ema[s.name].clone()
            if s.kind == "param":
                state["buf/" + s.name] = twin.buf(s.name).detach().clone()
        out.append(state)
    return out


_cache = {}


def shared():
    """the twelve-step sequence on the GPU, in the float64 twin and in stock float32 on the CPU: computed once"""
    if not _cache:
        specs = make_specs()
        _cache.update(specs=specs, gpu=run_gpu(specs), f64=run_twin(specs, torch.float64), f32=run_twin(specs, torch.float32))
    return _cache["specs"], _cache["gpu"], _cache["f64"], _cache["f32"]


def check_against_twin(specs, got, want, stock, what, worst):
    """the tolerance of the module docstring for every p / buf / ema tensor of one step; worst: running max of
    error / bound, kept for the record"""
    for key in want:
        if "/" not in key:
            continue
        if got[key].dtype == torch.int64:
            assert torch.equal(got[key], want[key]), f"{what}: {key} changed"
            continue
        ref = want[key].double()
        err, err_stock = max_err(got[key], ref), max_err(stock[key], ref)
        fin = torch.isfinite(ref)
        bound = 4 * err_stock + ulp32(ref[fin].abs().max() if bool(fin.any()) else 0.0)
        worst[0] = max(worst[0], err / bound)
        print(f"{what} {key}: err {err:.3e} stock {err_stock:.3e} bound {bound:.3e}")
        assert err <= bound, f"{what}: {key} off by {err:.3e}, stock float32 by {err_stock:.3e}, bound {bound:.3e}"


# ------------------------------------------------------------------------------------------------- 1. parity
def test_twelve_steps_match_the_float64_twin():
    specs, gpu, f64, f32 = shared()
    worst = [0.0]
    for step, (g, w, s) in enumerate(zip(gpu, f64, f32)):
        st = g["stats"]
        assert g["scale"] == w["scale"] == s["scale"] == st[4], (step, g["scale"], w["scale"])
        assert g["counters"] == [w["growth_tracker"], w["updates"]] and st[6] == w["updates"] and st[7] == w["growth_tracker"]
        assert bool(st[2]) == w["found_inf"] == (step in (INF_STEP, NAN_STEP)) and bool(st[3]) == w["skipped"]
        if w["found_inf"]:
            assert not np.isfinite(st[0])
        else:
            assert (st[1] < 1.0) == (w["clip"] < 1.0) == bool(step % 2), (step, st[1], w["clip"])
            print(f"step {step}: norm {st[0]!r} twin {w['norm']!r} clip {st[1]!r} twin {w['clip']!r}")
            assert abs(float(st[0]) - w["norm"]) <= 16 * 2.0 ** -24 * w["norm"], (step, st[0], w["norm"])
        d = 0.9999 * (1 - np.exp(-w["updates"] / 20.0))
        assert abs(float(st[5]) - d) <= ulp32(d)
        check_against_twin(specs, g, w, s, f"step {step}", worst)
    print(f"worst error / bound over the sequence: {worst[0]:.3f}")
    assert f64[-1]["scale"] == 65536.0 * 2 * 0.5 * 0.5 * 2 and f64[-1]["updates"] == STEPS


# ------------------------------------------------------------------------------------------------- 2. skipped steps
def assert_skipped(specs, before, after, halved):
    for s in specs:
        if s.kind == "param":
            assert torch.equal(after["p/" + s.name], before["p/" + s.name]), s.name
            assert torch.equal(after["buf/" + s.name], before["buf/" + s.name]), s.name
            assert not bool(after["grad/" + s.name].any()), f"gradient of {s.name} is not zero"
        if (s.kind == "param" and s.group != 0) or s.kind == "buffer":
            # the average of a tensor that has moved; group 0 has lr 0 and the frozen one never moves: their average is the
            # average of a constant, which the parity test covers
            assert not torch.equal(after["ema/" + s.name], before["ema/" + s.name]), f"the EMA of {s.name} did not move"
    assert after["stats"][3] == 1.0
    if halved:
        assert after["scale"] == before["scale"] / 2 and after["counters"][0] == 0 and after["stats"][2] == 1.0
    assert after["counters"][1] == before["counters"][1] + 1


def test_inf_and_nan_steps_leave_parameters_alone():
    specs, gpu, _, _ = shared()
    for step in (INF_STEP, NAN_STEP):
        assert_skipped(specs, gpu[step - 1], gpu[step], halved=True)
    for step in range(STEPS):                                       # every step zeroes the gradients
        assert not any(bool(gpu[step]["grad/" + s.name].any()) for s in specs if s.kind == "param")


def test_skip_flag_with_finite_gradients():
    specs = make_specs()
    model, avg, upd = build(specs)
    gen = torch.Generator().manual_seed(5)
    for step, skip in enumerate((None, torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int64, device=DEV),
                                 torch.full((4,), 2, dtype=torch.int32, device=DEV))):
        before = snapshot(specs, model, avg, upd)
        grads, lrs, stat = step_inputs(specs, step, before["scale"], gen, inf=False)
        gpu_step(model, upd, grads, lrs, stat, skip)
        after = snapshot(specs, model, avg, upd)
        if step < 2:
            assert after["stats"][3] == 0.0 and not torch.equal(after["p/" + LAST], before["p/" + LAST])
        else:
            assert_skipped(specs, before, after, halved=False)
        assert after["stats"][2] == 0.0                              # the flag is no inf: the scale follows the no-inf rule
    assert after["scale"] == 2 * 65536.0 and after["counters"] == [1, 4]      # grown after three clean steps, then one more
    with pytest.raises(TypeError):
        upd.step(torch.ones(1, device=DEV))
    with pytest.raises(NotImplementedError):
        upd.step(torch.ones(1, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------- 3. switches
def test_switches_no_clip_no_scaling_no_ema():
    specs = make_specs()
    worst = [0.0]
    # max_norm=None: clip 1 on the steps whose norm is >> 35
    kw = dict(max_norm=None)
    gpu, f64, f32 = run_gpu(specs, **kw), run_twin(specs, torch.float64, **kw), run_twin(specs, torch.float32, **kw)
    for step in (0, 1, 2, 3):
        assert gpu[step]["stats"][1] == 1.0 and f64[step]["clip"] == 1.0
        assert abs(float(gpu[step]["stats"][0]) - f64[step]["norm"]) <= 16 * 2.0 ** -24 * f64[step]["norm"]
        check_against_twin(specs, gpu[step], f64[step], f32[step], f"max_norm=None step {step}", worst)
    # loss_scale=None: no skip on inf / nan, parameters non-finite exactly where torch's are (max_err compares the masks)
    kw = dict(loss_scale=None)
    gpu, f64, f32 = run_gpu(specs, **kw), run_twin(specs, torch.float64, **kw), run_twin(specs, torch.float32, **kw)
    for step in range(NAN_STEP + 1):
        assert gpu[step]["stats"][3] == 0.0 and gpu[step]["scale"] == 1.0 and gpu[step]["stats"][2] == (step in (INF_STEP, NAN_STEP))
        check_against_twin(specs, gpu[step], f64[step], f32[step], f"loss_scale=None step {step}", worst)
    bad = gpu[INF_STEP]["p/" + LAST]
    assert not bool(torch.isfinite(bad[-1])) and bool(torch.isfinite(bad[:-1]).all())       # clip 0 x inf = nan, there alone
    assert not any(bool(torch.isfinite(gpu[NAN_STEP]["p/" + s.name]).any()) for s in specs if s.kind == "param" and s.group != 0)
    # neither: launch 1 is skipped, the norm is reported as 0
    kw = dict(max_norm=None, loss_scale=None)
    gpu, f64, f32 = run_gpu(specs, False, **kw), run_twin(specs, torch.float64, False, **kw), run_twin(specs, torch.float32, False, **kw)
    for step in (0, 1, 2):
        assert gpu[step]["stats"][0] == 0.0 and gpu[step]["stats"][1] == 1.0 and gpu[step]["counters"] == [0, step + 1]
        check_against_twin(specs, gpu[step], f64[step], f32[step], f"no clip, no scaling, step {step}", worst)
    # no ema; a gradient set to None outside a capture gets a new static buffer
    kw = dict(ema=False)
    model, avg, upd = build(specs, **kw)
    assert avg is None
    f64, f32 = run_twin(specs, torch.float64, **kw), run_twin(specs, torch.float32, **kw)
    gen = torch.Generator().manual_seed(5)
    scale = 65536.0
    for step in (0, 1, 2):
        if step == 2:
            model.t64.grad = None
            model.t64.grad = torch.zeros(64, device=DEV)
        grads, lrs, stat = step_inputs(specs, step, scale, gen)
        gpu_step(model, upd, grads, lrs, stat)
        snap = snapshot(specs, model, None, upd)
        scale = snap["scale"]
        check_against_twin(specs, snap, f64[step], f32[step], f"no ema, step {step}", worst)
    model.t64.grad = None
    upd.step()
    assert model.t64.grad is not None and not bool(model.t64.grad.any())


def test_non_f32_and_non_contiguous_tensors_are_refused():
    from s2anet_amd import TrainUpdate
    with pytest.raises(TypeError):
        TrainUpdate([nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))])
    with pytest.raises(ValueError):
        TrainUpdate([nn.Parameter(torch.zeros(4, 6, device=DEV).t())])
    model = nn.BatchNorm2d(4).to(DEV).half()                          # a float16 buffer that the EMA would have to average
    with pytest.raises(TypeError):
        TrainUpdate([nn.Parameter(torch.zeros(4, device=DEV))], model, copy.deepcopy(model))


# ------------------------------------------------------------------------------------------------- 4. determinism
def test_two_fresh_runs_are_bit_equal():
    specs, first, _, _ = shared()
    second = run_gpu(specs)
    for a, b in zip(first, second):
        assert a["scale"] == b["scale"] and a["counters"] == b["counters"]
        assert np.array_equal(a["stats"], b["stats"], equal_nan=True)
        for k in a:
            if "/" in k:
                assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                   b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


# ------------------------------------------------------------------------------------------------- 5. capture
def test_backward_and_step_captured_and_replayed():
    """scale_loss(loss).backward() + step() as ONE graph, replayed six times with new inputs and set_lr between the
    replays: bit-equal to the eager TrainUpdate route on the same sequence"""
    from s2anet_amd import TrainUpdate, reference_lr, reference_param_groups

    def make():
        torch.manual_seed(0)
        model = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(), nn.Conv2d(8, 4, 3, padding=1)).to(DEV).train()
        avg = copy.deepcopy(model).eval()
        return model, avg, TrainUpdate(reference_param_groups(model, 0.01, 1e-4), model, avg, **KW)

    def state(model, avg, upd):
        out = {"scale": upd.scale.clone(), "counters": upd.counters.clone()}
        out.update({"p/" + k: v.detach().clone() for k, v in model.state_dict().items()})
        out.update({"ema/" + k: v.detach().clone() for k, v in avg.state_dict().items()})
        out.update({f"buf/{i}": b.clone() for i, b in upd.bufs.items()})
        return out

    g = torch.Generator().manual_seed(2)
    xs = [torch.randn((2, 3, 16, 16), generator=g).to(DEV) for _ in range(8)]
    lrs = [[reference_lr(i, 8, 0.01, 1.0)] * 3 for i in range(8)]
    det0, bench0 = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        model, avg, upd = make()                                    # eager
        for x, lr in zip(xs, lrs):
            upd.set_lr(lr)
            upd.scale_loss(model(x).square().mean()).backward()
            upd.step()
        want = state(model, avg, upd)

        model, avg, upd = make()                                    # two eager warm-up steps on a side stream, then replays
        static_x = torch.empty_like(xs[0])

        def iteration():
            upd.scale_loss(model(static_x).square().mean()).backward()
            upd.step()

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for x, lr in zip(xs[:2], lrs[:2]):
                static_x.copy_(x)
                upd.set_lr(lr)
                iteration()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            iteration()
        versions = [p._version for p in model.parameters()]
        for x, lr in zip(xs[2:], lrs[2:]):
            static_x.copy_(x)
            upd.set_lr(lr)
            graph.replay()
        torch.cuda.synchronize()
        assert [p._version for p in model.parameters()] == versions      # a replay runs no Python ...
        upd.mark_updated()
        assert all(p._version > v for p, v in zip(model.parameters(), versions))   # ... so the caller says so
        got = state(model, avg, upd)
        assert int(got["counters"][1]) == 8 and float(got["scale"]) == 65536.0 * 4
        assert not torch.equal(got["p/0.weight"], make()[0][0].weight)
        for k in want:
            assert torch.equal(got[k], want[k]), f"{k}: the replayed route differs from the eager one"
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det0, bench0


# ------------------------------------------------------------------------------------------------- 6. weight caches
def first_difference(got, want):
    assert list(got) == list(want)
    for k in got:
        if got[k].shape != want[k].shape or not torch.equal(got[k], want[k]):
            return k
    return None


def test_weight_caches_follow_step_and_mark_updated(monkeypatch):
    """the packed-weight caches are keyed on (_version, data_ptr): an eager step() bumps the versions itself; the bare
    launch (what a graph replay amounts to) leaves the cached forward stale until mark_updated()"""
    from s2anet_amd import TrainUpdate
    from s2anet_amd.head import S2ANetHead
    monkeypatch.setenv("S2A_OWN_CONV_ALWAYS", "1")

    def build_head():
        torch.manual_seed(3)
        h = S2ANetHead(15, in_channels=64, feat_channels=64).to(DEV).train()
        with torch.no_grad():
            for m in h.modules():
                if isinstance(m, nn.Conv2d) and m.weight.shape[-1] == 3:
                    m.weight.normal_(0, 0.05)
            h.align_conv.deform_conv.weight.normal_(0, 0.05)
        return h

    def validate(h):
        with torch.no_grad():
            p = h([f.detach() for f in feats])["pred"]
        names = ("fam_cls", "fam_bbox", "odm_cls", "odm_bbox", "refine_anchor")
        return {f"{n}[{l}]": t for n, per_level in zip(names, p) for l, t in enumerate(per_level)}

    def twin(h):
        t = build_head()
        t.load_state_dict(h.state_dict(), strict=True)
        return t.train(h.training)

    det0, bench0 = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        head = build_head()
        B, size = 2, 256
        g = torch.Generator().manual_seed(4)
        feats = [torch.randn((B, 64, size // s, size // s), generator=g).to(DEV) for s in head.featmap_strides]
        t = torch.tensor([[0, 3, 0.30, 0.40, 0.20, 0.10, 0.3], [0, 14, 0.70, 0.60, 0.12, 0.25, 1.2],
                          [0, 0, 0.50, 0.20, 0.40, 0.30, -0.5], [1, 7, 0.25, 0.75, 0.15, 0.15, 0.0],
                          [1, 9, 0.55, 0.50, 0.50, 0.22, 2.0]], device=DEV)
        assert first_difference(validate(twin(head)), validate(twin(head))) is None, "precondition: two twins disagree"
        before = validate(head)                                             # warms the caches
        upd = TrainUpdate([{"params": list(head.parameters()), "lr": 1e-3}], model=head, ema=twin(head).eval())
        for step in range(2):
            loss = head(feats, t.clone(), (size, size))["loss"]
            upd.scale_loss(loss).backward()
            upd.step()
        assert upd.stats[3].item() == 0.0 and upd.counters.tolist() == [2, 2]
        got = validate(head)
        for k, v in got.items():
            assert bool(torch.isfinite(v).all()), k
        assert first_difference(got, validate(twin(head))) is None, "stale cache after two eager steps"
        for k in ("fam_bbox[0]", "odm_cls[0]", "odm_bbox[0]"):
            assert not torch.equal(got[k], before[k]), f"precondition: {k} did not change with training"
        # the kernel alone, as a replay would run it: parameters move, versions do not
        versions = [p._version for p in head.parameters()]
        for p in head.parameters():
            p.grad.normal_(0, 0.1 * 65536.0)
        upd.launch()
        assert [p._version for p in head.parameters()] == versions
        stale = validate(head)
        assert first_difference(stale, validate(twin(head))) is not None, \
            "precondition: the cached forward followed an update it cannot have seen"
        upd.mark_updated()
        assert first_difference(validate(head), validate(twin(head))) is None, "stale cache after mark_updated()"
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det0, bench0


# ------------------------------------------------------------------------------------------------- 7. state dict
def test_state_loaded_from_torch_sgd_continues_like_the_twin():
    """two steps of torch.optim.SGD on a GPU copy -> load_state_dict -> one TrainUpdate step == the twin continued from the
    same state (the tolerance of test 1); and state_dict() goes back into torch.optim.SGD"""
    specs = make_specs()
    model, avg, upd = build(specs)
    trained = [s for s in specs if s.kind == "param"]
    groups = lambda get: [{"params": [get(s) for s in trained if s.group == gi], **g} for gi, g in enumerate(GROUPS)]  # noqa: E731
    sgd = torch.optim.SGD(groups(lambda s: getattr(model, s.name)), lr=1e-3)
    twins = {dt: Twin(specs, GROUPS, dtype=dt, **KW) for dt in (torch.float64, torch.float32)}
    gen = torch.Generator().manual_seed(9)
    for step in range(2):                                           # plain SGD steps: no scaling, no clipping, no EMA
        for s in trained:
            gr = torch.randn(s.init.shape, generator=gen) * 0.1
            getattr(model, s.name).grad.copy_(gr)
            for tw in twins.values():
                tw.value[s.name].grad = gr.to(tw.dtype)
        sgd.step()
        sgd.zero_grad(set_to_none=False)
        for tw in twins.values():
            tw.sgd.step()
            tw.sgd.zero_grad()
    sd = sgd.state_dict()
    sd["updates"] = 40
    sd["scaler"] = {"scale": 1024.0, "growth_tracker": 2}
    upd.load_state_dict(sd)
    for tw in twins.values():
        tw.updates, tw.scale, tw.growth_tracker = 40, 1024.0, 2
        for n in tw.ema:
            tw.ema[n] = tw.value[n].detach().clone()
    with torch.no_grad():
        for s in specs:                                             # the EMA starts from the two-step weights on both sides
            getattr(avg, s.name).copy_(getattr(model, s.name))
    grads, lrs, stat = step_inputs(specs, 1, 1024.0, gen, inf=False)
    lrs = [0.0, 0.004, 0.006]
    gpu_step(model, upd, grads, lrs, stat)
    infos = {dt: tw.step(grads, lrs, buffers={"stat": stat}) for dt, tw in twins.items()}
    assert infos[torch.float64]["clip"] < 1.0 and upd.stats[1].item() < 1.0
    assert upd.scale.item() == 2048.0 == twins[torch.float64].scale and upd.counters.tolist() == [0, 41]

    def state(tw):
        out = {}
        for s in specs:
            out["p/" + s.name], out["ema/" + s.name] = tw.value[s.name].detach(), tw.ema[s.name]
            if s.kind == "param":
                out["buf/" + s.name] = tw.buf(s.name).detach()
        return out
    check_against_twin(specs, snapshot(specs, model, avg, upd), state(twins[torch.float64]), state(twins[torch.float32]),
                       "after load_state_dict", [0.0])
    # and back: torch.optim.SGD accepts state_dict()
    out = upd.state_dict()
    assert out["updates"] == 41 and out["scaler"] == {"scale": 2048.0, "growth_tracker": 0}
    assert [g["lr"] for g in out["param_groups"]] == pytest.approx(lrs)
    back = torch.optim.SGD(groups(lambda s: getattr(model, s.name)), lr=1e-3)
    back.load_state_dict(out)
    for s in trained:
        p = getattr(model, s.name)
        assert torch.equal(back.state[p]["momentum_buffer"], upd.momentum_buffer(p))
