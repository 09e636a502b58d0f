"""CPU: the float64 twin of the training update against torch's own SGD + GradScaler, and the host helpers of
s2anet_amd.optim (parameter split, warm-up, state-dict conversion, refusal of CPU tensors)."""
import copy
import math

import pytest
import torch
from torch import nn

from optim_twin import Spec, Twin

GROUPS = [dict(lr=0.01, weight_decay=0.0, momentum=0.9, nesterov=True),
          dict(lr=0.01, weight_decay=1e-4, momentum=0.9, nesterov=True),
          dict(lr=0.02, weight_decay=0.0, momentum=0.8, nesterov=False)]


def small_specs(gen):
    def r(*shape):
        return torch.randn(*shape, generator=gen)
    return [Spec("bn.weight", r(6), "param", 0), Spec("conv.weight", r(6, 3, 3, 3), "param", 1), Spec("conv.bias", r(6), "param", 2),
            Spec("frozen", r(5), "frozen"), Spec("bn.running_mean", r(6), "buffer"),
            Spec("bn.num_batches_tracked", torch.zeros((), dtype=torch.int64), "int")]


def test_twin_equals_torch_sgd_and_gradscaler_bit_for_bit():
    """twelve float64 steps (clipping on alternate steps, one inf step, one nan step, a warm-up ramp, growth_interval 3):
    the twin's hand-written scaler rule, inf check and EMA against torch.amp.GradScaler + torch.optim.SGD + the
    reference's ModelEMA.update, restated"""
    gen = torch.Generator().manual_seed(0)
    specs = small_specs(gen)
    twin = Twin(specs, GROUPS, dtype=torch.float64, growth_interval=3, ema_tau=20.0)
    trained = [s for s in specs if s.kind == "param"]
    ps = {s.name: s.init.double().clone().requires_grad_(True) for s in trained}
    other = {s.name: (s.init.clone() if s.kind == "int" else s.init.double().clone()) for s in specs if s.kind != "param"}
    sgd = torch.optim.SGD([{"params": [ps[s.name] for s in trained if s.group == gi], **g} for gi, g in enumerate(GROUPS)], lr=1e-3)
    scaler = torch.amp.GradScaler("cpu", init_scale=65536.0, growth_interval=3)
    scaler.scale(torch.zeros(1))                                            # creates the scale tensor, as scale(loss) does
    ema = {**{k: v.detach().clone() for k, v in ps.items()}, **{k: v.clone() for k, v in other.items()}}
    updates = 0
    for step in range(12):
        lrs = [g["lr"] * (1 + step) / 12 for g in GROUPS]
        scale = float(scaler.get_scale())
        assert scale == twin.scale
        grads = {s.name: torch.randn(s.init.shape, generator=gen) * (30.0 if step % 2 else 0.1) * scale for s in trained}
        if step == 4:
            grads["conv.bias"][-1] = float("inf")
        if step == 7:
            grads["conv.weight"].view(-1)[5] = float("nan")
        new_mean = torch.randn(6, generator=gen)
        info = twin.step(grads, lrs, buffers={"bn.running_mean": new_mean})
        # torch's route
        for g, lr in zip(sgd.param_groups, lrs):
            g["lr"] = lr
        other["bn.running_mean"] = new_mean.double()
        for n, p in ps.items():
            p.grad = grads[n].double()
        scaler.unscale_(sgd)
        norm = torch.nn.utils.clip_grad_norm_(list(ps.values()), max_norm=35, norm_type=2)
        scaler.step(sgd)
        scaler.update()
        sgd.zero_grad()
        updates += 1
        d = 0.9999 * (1 - math.exp(-updates / 20.0))
        with torch.no_grad():
            for k, v in ema.items():
                if v.dtype.is_floating_point:
                    v *= d
                    v += (1 - d) * (ps[k] if k in ps else other[k]).detach()
        assert info["found_inf"] == (step in (4, 7)) and info["skipped"] == info["found_inf"]
        if not info["found_inf"]:
            assert float(norm) == info["norm"] and (info["clip"] < 1.0) == bool(step % 2)
        assert float(scaler.get_scale()) == twin.scale and scaler._growth_tracker.item() == twin.growth_tracker
        for n, p in ps.items():
            assert torch.equal(p.detach(), twin.value[n].detach()), (step, n)
            b = sgd.state[p].get("momentum_buffer")
            assert torch.equal(b if b is not None else torch.zeros_like(p), twin.buf(n)), (step, n)
        for k, v in ema.items():
            assert torch.equal(v, twin.ema[k]), (step, k)
    assert twin.scale == 65536.0 * 2 * 0.5 * 0.5 * 2 and twin.updates == 12   # grown after steps 2 and 10, halved at 4 and 7


def test_reference_param_groups_on_the_detector():
    from s2anet_amd import reference_param_groups
    from s2anet_amd.detector import S2ANet
    model = S2ANet(15)
    groups = reference_param_groups(model, 0.01, 5e-4)
    assert [g["weight_decay"] for g in groups] == [0.0, 5e-4, 0.0] and all(g["lr"] == 0.01 for g in groups)
    where = {}
    for gi, g in enumerate(groups):
        for p in g["params"]:
            assert id(p) not in where, "a tensor in two groups"
            where[id(p)] = gi
    bn = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    assert bn and all(where[id(m.weight)] == 0 and where[id(m.bias)] == 2 for m in bn)
    assert len(groups[0]["params"]) == len(bn)
    names = dict(model.named_parameters())
    for n, p in names.items():
        if p.requires_grad:
            assert id(p) in where, f"{n} is in no group"
            if n.endswith(".bias"):
                assert where[id(p)] == 2, n
            elif n.endswith(".weight") and where[id(p)] != 0:
                assert where[id(p)] == 1, n
    assert len(where) == sum(p.requires_grad for p in names.values())
    torch.optim.SGD(groups, lr=0.01, momentum=0.9, nesterov=True)          # torch accepts the format


def test_reference_lr_warm_up_ends():
    from s2anet_amd import reference_lr
    lr0, lf, nw = 0.01, 0.8, 500
    assert reference_lr(0, nw, lr0, lf) == pytest.approx(lr0 * lf / 3, rel=1e-14)
    assert reference_lr(nw, nw, lr0, lf) == lr0 * lf
    assert reference_lr(nw + 1, nw, lr0, lf) == lr0 * lf
    mid = reference_lr(nw // 2, nw, lr0, lf)
    assert mid == pytest.approx(lr0 * lf * 2 / 3, rel=1e-14)
    assert all(reference_lr(i, nw, lr0, lf) < reference_lr(i + 1, nw, lr0, lf) for i in range(nw))


def test_state_dict_round_trips_through_torch_sgd():
    """torch.optim.SGD -> unpack -> pack -> a fresh torch.optim.SGD that then steps exactly like the first"""
    from s2anet_amd.optim import pack_state_dict, unpack_state_dict

    def make():
        torch.manual_seed(1)
        ps = [nn.Parameter(torch.randn(n)) for n in (3, 5, 2, 7)]
        opt = torch.optim.SGD([{"params": ps[:1], "lr": 0.0}, {"params": ps[1:3], "weight_decay": 1e-4},
                               {"params": ps[3:], "nesterov": False, "momentum": 0.8}], lr=0.01, momentum=0.9, nesterov=True)
        return ps, opt

    def run(ps, opt, seed):
        g = torch.Generator().manual_seed(seed)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()

    ps, opt = make()
    run(ps, opt, 2)
    sd = opt.state_dict()
    sizes = [1, 2, 1]
    hypers, bufs, scaler, updates = unpack_state_dict(sd, sizes)
    assert scaler is None and updates is None and len(bufs) == 4
    assert [h["lr"] for h in hypers] == [0.0, 0.01, 0.01] and [h["nesterov"] for h in hypers] == [True, True, False]
    assert hypers[1]["weight_decay"] == 1e-4 and hypers[2]["momentum"] == 0.8
    assert all(torch.equal(b, sd["state"][i]["momentum_buffer"]) for i, b in enumerate(bufs))
    packed = pack_state_dict(hypers, sizes, bufs, {"scale": 1024.0, "growth_tracker": 2}, 17)
    assert packed["param_groups"] == sd["param_groups"] and packed["scaler"] == {"scale": 1024.0, "growth_tracker": 2}
    assert unpack_state_dict(packed, sizes)[2:] == ({"scale": 1024.0, "growth_tracker": 2}, 17)
    ps2, opt2 = make()
    with torch.no_grad():
        for a, b in zip(ps2, ps):
            a.copy_(b)
    opt2.load_state_dict(copy.deepcopy(packed))
    run(ps, opt, 3)
    run(ps2, opt2, 3)
    assert all(torch.equal(a, b) for a, b in zip(ps, ps2))
    with pytest.raises(ValueError):
        unpack_state_dict(sd, [2, 1, 1])
    # a parameter that never stepped has no buffer
    _, fresh = make()
    assert unpack_state_dict(fresh.state_dict(), sizes)[1] == [None] * 4


def test_train_update_refuses_cpu_tensors_and_bad_arguments():
    from s2anet_amd import TrainUpdate
    with pytest.raises(NotImplementedError):
        TrainUpdate([nn.Parameter(torch.zeros(4))])
    with pytest.raises(NotImplementedError):
        TrainUpdate([{"params": [nn.Parameter(torch.zeros(4))], "lr": 0.1}], max_norm=None, loss_scale=None)
    p = nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError):
        TrainUpdate([{"params": [p]}, {"params": [p]}])
    with pytest.raises(ValueError):
        TrainUpdate([{"params": [p], "dampening": 0.1}])
    with pytest.raises(ValueError):
        TrainUpdate([])
