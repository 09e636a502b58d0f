"""The end of the reference's training iteration as one capturable launch sequence (csrc/optim_ops.hip).

The reference finishes every iteration with (train.py:358-373, utils/torch_utils.py:276-307)

    scaler.unscale_(optimizer); clip_grad_norm_(params, max_norm=35); scaler.step(optimizer); scaler.update()
    optimizer.zero_grad(); ema.update(model)

with SGD(momentum, nesterov=True) over three parameter groups.  `TrainUpdate.step()` is that sequence in three launches
over a device tensor table: no host read (torch's GradScaler.step reads found_inf back, so it cannot be captured), no
allocation, bit-reproducible.  `reference_param_groups` / `reference_lr` restate the reference's parameter split and
warm-up on the host.
"""
import ctypes

import torch
from torch import nn

from . import _lib
from ._lib import OPTIM_CHUNK, OPTIM_EMA_ONLY, OPTIM_STATS, OPTIM_TRAINED

STAT_NAMES = ("grad_norm", "clip", "found_inf", "skip_update", "scale", "ema_decay", "updates", "growth_tracker")


# ----------------------------------------------------------------------------------------------------- host helpers
def reference_param_groups(model, lr0, weight_decay):
    """the parameter split of train.py:159-177, same hasattr rules in the same order: group 0 = BatchNorm weights (no
    decay), group 1 = every other `.weight` (decay), group 2 = every `.bias` (no decay); torch.optim.SGD's format"""
    g0, g1, g2 = [], [], []
    for v in model.modules():
        if hasattr(v, "bias") and isinstance(v.bias, nn.Parameter):
            g2.append(v.bias)
        if isinstance(v, nn.BatchNorm2d):
            g0.append(v.weight)
        elif hasattr(v, "weight") and isinstance(v.weight, nn.Parameter):
            g1.append(v.weight)
    return [{"params": g0, "lr": lr0, "initial_lr": lr0, "weight_decay": 0.0},
            {"params": g1, "lr": lr0, "initial_lr": lr0, "weight_decay": weight_decay},
            {"params": g2, "lr": lr0, "initial_lr": lr0, "weight_decay": 0.0}]


def reference_lr(ni, nw, initial_lr, lf_epoch):
    """the warm-up of train.py:326-330 for integrated batch `ni` of `nw` warm-up batches: a linear ramp from a third of
    the scheduled rate (initial_lr * lf(epoch)) to all of it; past the warm-up the scheduled rate itself"""
    if ni > nw:
        return initial_lr * lf_epoch
    k = (1 - ni / nw) * (1 - 1.0 / 3)
    return (1 - k) * initial_lr * lf_epoch


def _normalise_groups(param_groups, momentum, nesterov):
    groups = list(param_groups)
    if not groups:
        raise ValueError("TrainUpdate: empty parameter list")
    if not isinstance(groups[0], dict):
        groups = [{"params": groups}]
    out, seen = [], set()
    for g in groups:
        if not isinstance(g, dict):
            raise TypeError("TrainUpdate: param_groups is a list of tensors or a list of dicts (torch.optim.SGD's format)")
        params = g["params"]
        params = [params] if isinstance(params, torch.Tensor) else list(params)
        for p in params:
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"TrainUpdate: a parameter group holds a {type(p).__name__}, not a tensor")
            if id(p) in seen:
                raise ValueError("TrainUpdate: a parameter appears in more than one parameter group")
            seen.add(id(p))
        if g.get("dampening", 0) != 0 or g.get("maximize", False):
            raise ValueError("TrainUpdate: dampening and maximize are not supported (the reference uses neither)")
        out.append({"params": params, "lr": float(g.get("lr", 1e-3)), "weight_decay": float(g.get("weight_decay", 0.0)),
                    "momentum": float(g.get("momentum", momentum)), "nesterov": bool(g.get("nesterov", nesterov))})
    return out


def pack_state_dict(hypers, group_sizes, bufs, scaler=None, updates=None):
    """a torch.optim.SGD state dict (`momentum_buffer` per parameter, parameters numbered in group order) plus the
    scaler's `scale` / `growth_tracker` and the EMA's `updates`.  hypers: per group dict(lr, momentum, weight_decay,
    nesterov); bufs: per parameter a tensor or None (never stepped); torch.optim.SGD.load_state_dict accepts the result"""
    if sum(group_sizes) != len(bufs) or len(hypers) != len(group_sizes):
        raise ValueError("pack_state_dict: group sizes do not add up to the parameters")
    groups, first = [], 0
    for h, n in zip(hypers, group_sizes):
        groups.append({"lr": float(h["lr"]), "momentum": float(h["momentum"]), "dampening": 0,
                       "weight_decay": float(h["weight_decay"]), "nesterov": bool(h["nesterov"]), "maximize": False,
                       "foreach": None, "differentiable": False, "fused": None, "params": list(range(first, first + n))})
        first += n
    sd = {"state": {i: {"momentum_buffer": b} for i, b in enumerate(bufs) if b is not None}, "param_groups": groups}
    if scaler is not None:
        sd["scaler"] = {"scale": float(scaler["scale"]), "growth_tracker": int(scaler["growth_tracker"])}
    if updates is not None:
        sd["updates"] = int(updates)
    return sd


def unpack_state_dict(sd, group_sizes):
    """inverse of pack_state_dict; also reads a plain torch.optim.SGD state dict (then scaler and updates are None)
    -> (hypers, bufs, scaler, updates)"""
    groups = sd["param_groups"]
    if [len(g["params"]) for g in groups] != list(group_sizes):
        raise ValueError(f"state dict has parameter groups of {[len(g['params']) for g in groups]} parameters, "
                         f"this update has {list(group_sizes)}")
    hypers, bufs = [], []
    for g in groups:
        if g.get("dampening", 0) != 0 or g.get("maximize", False):
            raise ValueError("state dict uses dampening / maximize: not supported")
        hypers.append({"lr": float(g["lr"]), "momentum": float(g.get("momentum", 0.0)),
                       "weight_decay": float(g.get("weight_decay", 0.0)), "nesterov": bool(g.get("nesterov", False))})
        for i in g["params"]:
            bufs.append(sd["state"].get(i, {}).get("momentum_buffer"))
    scaler = sd.get("scaler")
    if scaler is not None:
        scaler = {"scale": float(scaler["scale"]), "growth_tracker": int(scaler.get("growth_tracker", scaler.get("_growth_tracker", 0)))}
    updates = sd.get("updates")
    return hypers, bufs, scaler, None if updates is None else int(updates)


def _check_f32(t, what):
    if t.dtype != torch.float32:
        raise TypeError(f"TrainUpdate: {what} is {t.dtype}; contiguous float32 only")
    if not t.is_contiguous():
        raise ValueError(f"TrainUpdate: {what} is not contiguous")


# ----------------------------------------------------------------------------------------------------- the update
class TrainUpdate:
    """unscale + clip_grad_norm_ + SGD (momentum / Nesterov, parameter groups) + GradScaler update + zero_grad + EMA.

    param_groups   torch.optim.SGD's format (per-group lr, weight_decay, optional momentum / nesterov), or a list of tensors
    model, ema     with `ema` (a module whose state_dict mirrors `model`'s, typically copy.deepcopy(model).eval()) every
                   floating state_dict entry is averaged as ModelEMA.update does; integer entries are left alone;
                   parameters with requires_grad=False and floating buffers only feed the average
    max_norm       None: no clipping;  loss_scale None: GradScaler(enabled=False), no scaling and no inf-skip

    Gradients are STATIC buffers: every trained parameter gets p.grad = zeros_like(p) when it has none, the addresses go
    into a device table and the kernel zeroes them after use.  Never call zero_grad(set_to_none=True) on them.  Outside a
    capture step() notices a changed p.grad address and rebuilds the table (a host-to-device copy); inside a capture it
    raises.  One consequence: a parameter that took no part in a backward has a ZERO gradient, not None, so it still sees
    weight decay and momentum -- torch's zero_grad(set_to_none=False) behaviour.

    .lr            device f32 [n_groups];  set_lr(values): asynchronous copy on the current stream, also between replays
    .stats         device f32 [8]: STAT_NAMES, written by every step
    .step(skip)    skip: optional device int32 / int64 tensor, non-zero = leave p and the momentum buffers alone
                   (status[:1] of S2ANetHead.compute_loss_device); it does not enter the scale update.  The EMA moves
                   and the gradients are zeroed on skipped steps too, as in the reference's loop.
    .mark_updated()  bumps `_version` of everything the kernel wrote so that the packed-weight caches follow.  An eager
                   step() calls it itself.  A graph replay runs no Python: AFTER REPLAYING captured steps the caller
                   must call mark_updated() before the next forward that is not part of the graph."""

    def __init__(self, param_groups, model=None, ema=None, momentum=0.9, nesterov=True, max_norm=35.0, loss_scale=65536.0,
                 growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, ema_decay=0.9999, ema_tau=2000.0):
        self.groups = _normalise_groups(param_groups, momentum, nesterov)
        self.params = [p for g in self.groups for p in g["params"]]
        _lib.require_cuda(*self.params)
        if ema is not None:
            if model is None:
                raise ValueError("TrainUpdate: `ema` needs `model`, the module it averages")
            _lib.require_cuda(*model.state_dict().values(), *ema.state_dict().values())
        self.device = self.params[0].device
        for i, p in enumerate(self.params):
            _check_f32(p, f"parameter {i}")
            if p.device != self.device:
                raise ValueError("TrainUpdate: parameters on more than one device")
        if max_norm is not None and not max_norm > 0:
            raise ValueError("TrainUpdate: max_norm must be positive (None disables clipping)")
        if loss_scale is not None and (not loss_scale > 0 or growth_interval < 1):
            raise ValueError("TrainUpdate: loss_scale must be positive and growth_interval >= 1")
        if not ema_tau > 0:
            raise ValueError("TrainUpdate: ema_tau must be positive")
        self.max_norm, self.scaling = max_norm, loss_scale is not None
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, int(growth_interval)
        self.ema_decay, self.ema_tau = float(ema_decay), float(ema_tau)
        dev = self.device
        self.trained = [i for i, p in enumerate(self.params) if p.requires_grad and p.numel() > 0]
        self.bufs = {i: torch.zeros_like(self.params[i], memory_format=torch.contiguous_format) for i in self.trained}
        # EMA pairs: (source, destination); a trained parameter's destination rides on its own row
        self._ema_of, self._ema_only = {}, []
        if ema is not None:
            msd, esd = model.state_dict(keep_vars=True), ema.state_dict(keep_vars=True)
            if list(msd) != list(esd):
                raise ValueError("TrainUpdate: ema.state_dict() does not mirror model.state_dict()")
            index = {id(self.params[i]): i for i in self.trained}
            seen = set()
            for k, ev in esd.items():
                mv = msd[k]
                if not ev.dtype.is_floating_point or id(ev) in seen or ev.numel() == 0:
                    continue
                seen.add(id(ev))
                _check_f32(ev, f"ema entry {k}")
                _check_f32(mv, f"model entry {k}")
                if ev.shape != mv.shape or ev.device != dev or mv.device != dev:
                    raise ValueError(f"TrainUpdate: ema entry {k} does not match the model's ({tuple(ev.shape)} on {ev.device} "
                                     f"against {tuple(mv.shape)} on {mv.device})")
                if ev.data_ptr() == mv.data_ptr():
                    raise ValueError(f"TrainUpdate: ema entry {k} shares its memory with the model's")
                if id(mv) in index:
                    self._ema_of[index[id(mv)]] = ev
                else:
                    self._ema_only.append((mv, ev))
        self.lr = torch.tensor([g["lr"] for g in self.groups], dtype=torch.float32, device=dev)
        self._lr_stage = torch.empty(len(self.groups), dtype=torch.float32).pin_memory()
        self._lr_event = None
        self._hyper = torch.empty((len(self.groups), 4), dtype=torch.float32, device=dev)
        self._write_hyper()
        self.scale = torch.full((1,), float(loss_scale if self.scaling else 1.0), dtype=torch.float32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)              # growth_tracker, updates
        self.stats = torch.zeros(OPTIM_STATS, dtype=torch.float32, device=dev)
        self._skip = None
        self._grad_ptrs = None
        self._build_tables()

    # ------------------------------------------------------------------------------------------------- tables
    def _write_hyper(self):
        self._hyper.copy_(torch.tensor([[g["momentum"], g["weight_decay"], float(g["nesterov"]), 0.0] for g in self.groups],
                                       dtype=torch.float32))

    def _build_tables(self):
        """static gradient buffers, the device tensor table and the chunk map"""
        group_of = {}
        for gi, g in enumerate(self.groups):
            for p in g["params"]:
                group_of[id(p)] = gi
        rows, chunks = [], []
        for i in self.trained:
            p = self.params[i]
            if p.grad is None:
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            _check_f32(p.grad, f"the gradient of parameter {i}")
            if p.grad.shape != p.shape or p.grad.device != p.device:
                raise ValueError(f"TrainUpdate: the gradient of parameter {i} does not match it")
            e = self._ema_of.get(i)
            rows.append((p.data_ptr(), p.grad.data_ptr(), self.bufs[i].data_ptr(), e.data_ptr() if e is not None else 0,
                         p.numel(), group_of[id(p)], OPTIM_TRAINED))
        for r, row in enumerate(rows):
            chunks += [(r, s) for s in range(0, row[4], OPTIM_CHUNK)]
        self.n_trained_chunks = len(chunks)
        for mv, ev in self._ema_only:
            chunks += [(len(rows), s) for s in range(0, mv.numel(), OPTIM_CHUNK)]
            rows.append((mv.data_ptr(), 0, 0, ev.data_ptr(), mv.numel(), 0, OPTIM_EMA_ONLY))
        table = (_lib.OptimTensor * max(len(rows), 1))()
        for r, row in enumerate(rows):
            table[r] = _lib.OptimTensor(*row)
        dev = self.device
        host = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8)
        self._table = host.to(dev)
        self._chunks = torch.tensor(chunks, dtype=torch.int64).reshape(-1, 2).to(dev)
        self.n_tensors, self.n_chunks = len(rows), len(chunks)
        self.n_elements = sum(r[4] for r in rows)
        self._grad_ptrs = [self.params[i].grad.data_ptr() for i in self.trained]
        nbytes = _lib.lib().s2a_train_update_workspace_bytes(self.n_trained_chunks)
        self._ws = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)   # owned: a captured graph keeps its address
        a = _lib.TrainUpdateArgs()
        a.tensors, a.chunks = self._table.data_ptr(), self._chunks.data_ptr()
        a.n_tensors, a.n_chunks, a.n_trained_chunks = self.n_tensors, self.n_chunks, self.n_trained_chunks
        a.lr, a.hyper, a.n_groups = self.lr.data_ptr(), self._hyper.data_ptr(), len(self.groups)
        a.scaling_enabled = int(self.scaling)
        a.scale, a.counters, a.stats = self.scale.data_ptr(), self.counters.data_ptr(), self.stats.data_ptr()
        a.growth_interval = self.growth_interval
        a.max_norm = float(self.max_norm) if self.max_norm is not None else 0.0
        a.growth_factor, a.backoff_factor = self.growth_factor, self.backoff_factor
        a.ema_decay, a.ema_tau = self.ema_decay, self.ema_tau
        self._args = a
        self._written = [self.params[i] for i in self.trained] + [self.bufs[i] for i in self.trained] + \
            list(self._ema_of.values()) + [ev for _, ev in self._ema_only]

    def _grads_match(self):
        for i, ptr in zip(self.trained, self._grad_ptrs):
            g = self.params[i].grad
            if g is None or g.data_ptr() != ptr:
                return False
        return True

    # ------------------------------------------------------------------------------------------------- public surface
    def set_lr(self, values):
        """per-group learning rates -> .lr, an asynchronous copy from a pinned staging buffer on the current stream; a
        captured step reads .lr on the device, so this is how the schedule moves between replays"""
        values = [float(v) for v in values] if not isinstance(values, (int, float)) else [float(values)] * len(self.groups)
        if len(values) != len(self.groups):
            raise ValueError(f"set_lr: {len(values)} values for {len(self.groups)} parameter groups")
        if self._lr_event is not None:
            self._lr_event.synchronize()               # the previous copy has read the staging buffer
        self._lr_stage.copy_(torch.tensor(values, dtype=torch.float32))
        self.lr.copy_(self._lr_stage, non_blocking=True)
        self._lr_event = torch.cuda.Event()
        self._lr_event.record(torch.cuda.current_stream(self.device))
        for g, v in zip(self.groups, values):
            g["lr"] = v

    def scale_loss(self, loss):
        """loss * scale with the device scale (GradScaler.scale); the identity when scaling is off"""
        _lib.require_cuda(loss)
        return loss * self.scale.view(()) if self.scaling else loss

    def launch(self, skip=None):
        """the launch sequence alone, through the C ABI: no table check and no mark_updated()"""
        a = self._args
        if skip is not None:
            _lib.require_cuda(skip)
            if skip.dtype not in (torch.int32, torch.int64) or skip.numel() < 1 or not skip.is_contiguous():
                raise TypeError("TrainUpdate.step: skip is a contiguous device int32 / int64 tensor with at least one element")
            a.skip, a.skip_elem_bytes = skip.data_ptr(), skip.element_size()
        else:
            a.skip, a.skip_elem_bytes = None, 0
        self._skip = skip                              # a captured graph reads it at every replay
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().s2a_train_update(ctypes.byref(a), _lib.ptr(self._ws), self._ws.numel(),
                                                   _lib.stream_ptr(self.device)))

    def step(self, skip=None):
        capturing = torch.cuda.is_current_stream_capturing()
        if not self._grads_match():
            if capturing:
                raise RuntimeError("TrainUpdate.step: a p.grad address changed (zero_grad(set_to_none=True)?); the table "
                                   "cannot be rebuilt inside a capture")
            self._build_tables()
        self.launch(skip)
        if not capturing:
            self.mark_updated()

    def momentum_buffer(self, p):
        """the momentum buffer of trained parameter p (torch.optim.SGD's state[p]["momentum_buffer"])"""
        for i in self.trained:
            if self.params[i] is p:
                return self.bufs[i]
        raise KeyError("not a trained parameter of this update")

    def mark_updated(self):
        """bump `_version` of every parameter, momentum buffer and EMA entry the kernel writes, so that the weight caches
        keyed on (_version, data_ptr) repack.  Call it after replaying a graph that holds step()."""
        torch.autograd.graph.increment_version(self._written)

    # ------------------------------------------------------------------------------------------------- state
    def _group_sizes(self):
        return [len(g["params"]) for g in self.groups]

    def state_dict(self):
        """torch.optim.SGD's state dict (loadable by it) + `scaler` {scale, growth_tracker} (None: scaling off) + the
        EMA's `updates`.  Reads the device state: one host synchronisation."""
        counters = self.counters.tolist()
        bufs = [self.bufs[i].clone() if i in self.bufs else None for i in range(len(self.params))]
        scaler = {"scale": float(self.scale.item()), "growth_tracker": counters[0]} if self.scaling else None
        return pack_state_dict(self.groups, self._group_sizes(), bufs, scaler, counters[1])

    def load_state_dict(self, sd):
        """a state_dict() of this class or of torch.optim.SGD (a reference checkpoint's `optimizer` entry; pass its
        `updates` as sd["updates"]).  Buffers are copied in place: captured graphs stay valid."""
        hypers, bufs, scaler, updates = unpack_state_dict(sd, self._group_sizes())
        for i, b in enumerate(bufs):
            if i not in self.bufs:
                continue
            if b is None:
                self.bufs[i].zero_()
            else:
                if b.shape != self.bufs[i].shape:
                    raise ValueError(f"momentum buffer {i}: {tuple(b.shape)} against {tuple(self.bufs[i].shape)}")
                self.bufs[i].copy_(b)
        for g, h in zip(self.groups, hypers):
            g.update(h)
        self._write_hyper()
        self.set_lr([g["lr"] for g in self.groups])
        if scaler is not None and self.scaling:
            self.scale.fill_(scaler["scale"])
            self.counters[0] = scaler["growth_tracker"]
        if updates is not None:
            self.counters[1] = updates
