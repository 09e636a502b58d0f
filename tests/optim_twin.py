"""The reference's training update (train.py:358-373, utils/torch_utils.py:276-307) in plain torch on the CPU, in a
dtype of the caller's choice: float64 is the twin the kernel is pinned to, float32 is the stock route whose own error
against that twin sets the kernel's tolerance.  A helper, not a test.

    unscale (GradScaler.unscale_) -> per-element inf check -> clip_grad_norm_ -> torch.optim.SGD.step unless skipped ->
    the scaler rule (_amp_update_scale_) -> zero_grad -> ModelEMA.update

The scaler rule, the inf check and the EMA are restated by hand (tests/test_optim_cpu.py holds them against
torch.amp.GradScaler); the clipping and the SGD step are torch's own.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch


@dataclass
class Spec:
    name: str
    init: torch.Tensor          # float32 (int64 for kind "int"), CPU
    kind: str = "param"         # "param" (trained) | "frozen" | "buffer" (floating) | "int"
    group: int = 0              # parameter group of a trained tensor


class Twin:
    def __init__(self, specs, groups, dtype=torch.float64, max_norm=35.0, loss_scale=65536.0, growth_factor=2.0,
                 backoff_factor=0.5, growth_interval=2000, ema=True, ema_decay=0.9999, ema_tau=2000.0):
        """groups: per group dict(lr, weight_decay, momentum, nesterov)"""
        self.dtype, self.specs = dtype, specs
        self.value = {s.name: (s.init.clone() if s.kind == "int" else s.init.to(dtype).clone()) for s in specs}
        self.trained = [s.name for g in range(len(groups)) for s in specs if s.kind == "param" and s.group == g]
        for n in self.trained:
            self.value[n].requires_grad_(True)
        self.sgd = torch.optim.SGD([{"params": [self.value[s.name] for s in specs if s.kind == "param" and s.group == gi],
                                     "lr": g["lr"], "weight_decay": g["weight_decay"], "momentum": g["momentum"],
                                     "nesterov": g["nesterov"]} for gi, g in enumerate(groups)], lr=1e-3)
        self.max_norm, self.scaling = max_norm, loss_scale is not None
        self.scale = float(loss_scale) if self.scaling else 1.0
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval
        self.growth_tracker, self.updates = 0, 0
        self.ema_decay, self.ema_tau = ema_decay, ema_tau
        self.ema = {s.name: self.value[s.name].detach().clone() for s in specs} if ema else None

    def buf(self, name):
        b = self.sgd.state.get(self.value[name], {}).get("momentum_buffer")
        return torch.zeros_like(self.value[name]) if b is None else b

    def step(self, grads, lrs, skip=False, buffers=None):
        """grads: name -> float32 gradient as backward leaves it (times the scale); lrs: per group; buffers: name -> the
        new float32 value of a floating buffer (what a forward in train mode does to BN statistics)
        -> dict(norm, clip, found_inf, skipped)"""
        for g, lr in zip(self.sgd.param_groups, lrs):
            g["lr"] = lr
        for n, v in (buffers or {}).items():
            self.value[n] = v.to(self.dtype).clone()
        # GradScaler.unscale_: found_inf from the gradient as it is, then grad *= 1 / scale
        inv = 1.0 / self.scale if self.scaling else 1.0
        found_inf = any(not bool(torch.isfinite(grads[n]).all()) for n in self.trained)
        params = [self.value[n] for n in self.trained]
        for n, p in zip(self.trained, params):
            p.grad = grads[n].to(self.dtype) * inv
        if self.max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(params, max_norm=self.max_norm, norm_type=2)
            clip = float(torch.clamp(self.max_norm / (norm + 1e-6), max=1.0))
        else:
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))
            clip = 1.0
        skipped = (self.scaling and found_inf) or skip
        if not skipped:
            self.sgd.step()
        if self.scaling:                                    # _amp_update_scale_
            if found_inf:
                self.scale *= self.backoff_factor
                self.growth_tracker = 0
            else:
                self.growth_tracker += 1
                if self.growth_tracker == self.growth_interval:
                    if math.isfinite(float(np.float32(self.scale * self.growth_factor))):
                        self.scale *= self.growth_factor
                    self.growth_tracker = 0
        self.sgd.zero_grad()
        self.updates += 1
        if self.ema is not None:                            # ModelEMA.update
            d = self.ema_decay * (1 - math.exp(-self.updates / self.ema_tau))
            with torch.no_grad():
                for s in self.specs:
                    v = self.ema[s.name]
                    if v.dtype.is_floating_point:
                        v *= d
                        v += (1 - d) * self.value[s.name].detach()
        return {"norm": float(norm), "clip": clip, "found_inf": found_inf, "skipped": bool(skipped)}


def ulp32(x):
    """one float32 ulp at magnitude x"""
    return float(np.spacing(np.float32(abs(float(x)))))


def max_err(a, ref):
    """max abs error of a against the float64 ref over the elements where ref is finite; non-finite masks must agree"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(a), fin), "finite masks differ"
    return float((a[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0
