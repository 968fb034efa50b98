"""torch.optim.Adam whose step is ONE HIP launch per 80 parameter tensors (include/advhip.h: advhip_adam_multi_f32).

The reference trains with `torch.optim.Adam(params, lr, weight_decay)` (/root/reference/src/runner.py:53-59).  torch's fused,
capturable form of it costs seven launches per step on the scorer's 130 parameters (0.28 ms of a 15.7-ms step); here the update
of all of them is two launches plus one add on the step counters.  Same update rule, same state layout -- `state[p]` holds
`step` (a device-side fp32 scalar, as torch's capturable Adam keeps it), `exp_avg`, `exp_avg_sq` -- so `state_dict()` /
`load_state_dict()` interchange with torch.optim.Adam, checkpoints of the reference included.  CUDA fp32 parameters only;
amsgrad / maximize / differentiable are not offered (the reference uses none of them).

Two opt-in extensions keep a captured training step (train_graph.GraphedTrainStep) valid where the by-value launch cannot:
`device_lr=True` keeps the learning rate in device memory, so a per-step schedule does not stale the graph, and
`max_grad_norm=x` clips the global gradient norm with one reduction (advhip_grad_norm_multi_f32) whose factor the Adam launch
applies on read (advhip_adam_multi_dev_f32).  `lr_at` is the schedule rule the trainer's `runner.optimizer.schedule` key evaluates.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional

import torch

from . import _lib
from ._lib import check

SCHEDULES = ("constant", "linear", "cosine", "multistep")
SCHEDULE_DEFAULTS = {"name": None, "warmup_steps": 0, "total_steps": None, "min_lr_ratio": 0.0, "milestones": [], "gamma": 0.1}


def check_schedule(spec) -> Optional[Dict[str, Any]]:
    """`runner.optimizer.schedule` with its defaults filled in (None stays None); ValueError for anything `lr_at` could not evaluate."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError(f"runner.optimizer.schedule={spec!r} is not a mapping ({{name: constant|linear|cosine|multistep, ...}}) or null")
    unknown = sorted(set(spec) - set(SCHEDULE_DEFAULTS))
    if unknown:
        raise ValueError(f"runner.optimizer.schedule: unknown key(s) {unknown}; the keys are {sorted(SCHEDULE_DEFAULTS)}")
    out = {**SCHEDULE_DEFAULTS, **spec}
    if out["name"] not in SCHEDULES:
        raise ValueError(f"runner.optimizer.schedule.name={out['name']!r}: not one of {list(SCHEDULES)}")
    is_count = lambda v: isinstance(v, int) and not isinstance(v, bool) and v >= 0
    if not is_count(out["warmup_steps"]):
        raise ValueError(f"runner.optimizer.schedule.warmup_steps={out['warmup_steps']!r} must be an integer >= 0")
    if out["total_steps"] is not None and not is_count(out["total_steps"]):
        raise ValueError(f"runner.optimizer.schedule.total_steps={out['total_steps']!r} must be an integer >= 0 or null")
    r = out["min_lr_ratio"]
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not 0.0 <= r <= 1.0:
        raise ValueError(f"runner.optimizer.schedule.min_lr_ratio={r!r} is outside [0, 1]")
    ms = out["milestones"]
    if not isinstance(ms, (list, tuple)) or not all(is_count(m) for m in ms):
        raise ValueError(f"runner.optimizer.schedule.milestones={ms!r} must be a list of integers >= 0")
    g = out["gamma"]
    if isinstance(g, bool) or not isinstance(g, (int, float)) or not math.isfinite(g) or g <= 0:
        raise ValueError(f"runner.optimizer.schedule.gamma={g!r} must be a finite number > 0")
    out["min_lr_ratio"], out["gamma"], out["milestones"] = float(r), float(g), [int(m) for m in ms]
    return out


def lr_at(spec, base_lr: float, step: int, total_steps: Optional[int] = None) -> float:
    """The learning rate of training step `step` (0-based: trainer.global_step of the step about to be taken) under
    `runner.optimizer.schedule`.  A pure function of Python floats -- nothing to checkpoint, a resumed run continues from its
    global_step alone (the philosophy of dataset.epoch_order).  With W = warmup_steps, N = total_steps, r = min_lr_ratio:
        step < W           base * (step + 1) / W
        q                = min(1, (step - W) / max(1, N - W))
        constant           base
        linear             base * (r + (1 - r) * (1 - q))
        cosine             base * (r + (1 - r) * 0.5 * (1 + cos(pi q)))
        multistep          base * gamma ** (number of milestones <= step)
    `total_steps` (argument): N where the spec leaves it null -- the trainer passes max_steps, or max_epochs x steps per epoch."""
    spec = check_schedule(spec)
    base, s = float(base_lr), int(step)
    if spec is None:
        return base
    if s < 0:
        raise ValueError(f"lr_at: step {step} is negative")
    W, name = spec["warmup_steps"], spec["name"]
    if s < W:
        return base * (s + 1) / W
    if name == "constant":
        return base
    if name == "multistep":
        return base * spec["gamma"] ** sum(1 for m in spec["milestones"] if m <= s)
    N = spec["total_steps"] if spec["total_steps"] is not None else total_steps
    if N is None:
        raise ValueError(f"runner.optimizer.schedule: a {name} schedule needs total_steps (or a trainer with max_steps / max_epochs)")
    q = min(1.0, (s - W) / max(1, int(N) - W))
    r = spec["min_lr_ratio"]
    if name == "linear":
        return base * (r + (1.0 - r) * (1.0 - q))
    return base * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * q)))


def check_max_grad_norm(value) -> Optional[float]:
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
        raise ValueError(f"max_grad_norm={value!r} must be a finite number > 0 (or None: no clipping)")
    return float(value)


class HipAdam(torch.optim.Adam):
    """`device_lr=True`: one float64 device scalar per param group holds the group's lr and the Adam launch reads it there.
    `group["lr"]` stays the Python float everything else works with (torch's lr_scheduler classes, LearningRateMonitor); `sync_lr()`
    uploads it when it changed -- one asynchronous `fill_` on the current stream, the value travelling as a kernel argument -- and
    `step()` calls it.  Inside a graph capture nothing is written (a captured fill would reset the lr on every replay): whoever
    replays the graph calls `sync_lr()` first, as GraphedTrainStep does.

    `max_grad_norm=x`: torch.nn.utils.clip_grad_norm_(params, x) folded into the step.  The global L2 norm of the live gradients
    is reduced on the device (double accumulation in a fixed order: bit-reproducible), `grad_norm` is the 0-dim fp32 device tensor
    with the last pre-clip norm, and the Adam launch multiplies every gradient element by min(1, x / (norm + 1e-6)) as it reads it.
    Unlike torch, `p.grad` is NOT rewritten: after `step()` it still holds the unclipped gradient.  (The lr is read from the device
    scalar here too, `sync_lr()` included; without `device_lr` a graph is still re-captured when it changes.)"""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 device_lr: bool = False, max_grad_norm: Optional[float] = None):
        if torch.is_tensor(lr) or any(torch.is_tensor(b) for b in betas):
            raise ValueError("HipAdam takes lr / betas as Python numbers (a tensor would be read back on the host every step: a sync inside a graph capture)")
        if torch.is_tensor(max_grad_norm):
            raise ValueError("HipAdam takes max_grad_norm as a Python number")
        self.device_lr, self.max_grad_norm = bool(device_lr), check_max_grad_norm(max_grad_norm)
        # capturable=True: the step counters live on the device, which is what lets a whole training step be one HIP graph
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=False, capturable=True)
        self._steps = None  # one flat fp32 tensor; state[p]["step"] is a 0-dim view of it
        self._lr_dev = None  # device_lr / max_grad_norm: one float64 slot per param group ...
        self._lr_sent: list = []  # ... and the Python float last written to it
        self._norm_partials = None  # max_grad_norm: float64 block sums, and (norm, scale) as two fp32
        self._norm_out = None
        self.grad_norm: Optional[torch.Tensor] = None

    @property
    def reads_device_scalars(self) -> bool:
        return self.device_lr or self.max_grad_norm is not None

    def sync_lr(self) -> None:
        """Upload every group's lr that changed since the last upload (nothing otherwise, and nothing at all for a default HipAdam)."""
        if not self.reads_device_scalars:
            return
        if torch.cuda.is_current_stream_capturing():
            raise _lib.HipExtensionError("HipAdam.sync_lr inside a graph capture: the fill would be replayed, resetting the lr to the captured "
                                         "value every step; call it before graph.replay() instead")
        groups = self.param_groups
        if self._lr_dev is None or self._lr_dev.numel() != len(groups):
            dev = next(p.device for g in groups for p in g["params"])
            self._lr_dev = torch.empty(len(groups), device=dev, dtype=torch.float64)
            self._lr_slots = list(self._lr_dev.unbind(0))
            self._lr_sent = [None] * len(groups)
        for i, g in enumerate(groups):
            lr = g["lr"]
            if torch.is_tensor(lr):
                raise _lib.HipExtensionError("HipAdam: a tensor learning rate is not offered (float(lr) would synchronise, and cannot be captured)")
            lr = float(lr)
            if lr != self._lr_sent[i]:
                self._lr_slots[i].fill_(lr)
                self._lr_sent[i] = lr

    def graph_stamp(self):
        """What a captured step holds of this optimizer beyond torch's param_groups: the clip value and the device buffers' addresses."""
        return (self.device_lr, self.max_grad_norm) + tuple(None if t is None else t.data_ptr() for t in (self._lr_dev, self._norm_partials, self._norm_out))

    def _launch_grad_norm(self, lib, grads, capturing: bool) -> None:
        need = sum((g.numel() + 4095) // 4096 for g in grads)
        if self._norm_partials is None or self._norm_partials.numel() < need:
            if capturing:
                raise _lib.HipExtensionError("HipAdam(max_grad_norm=): a graph capture needs one eager step first (it allocates the norm buffers)")
            self._norm_partials = torch.empty(need, device=grads[0].device, dtype=torch.float64)
        if self._norm_out is None:
            if capturing:
                raise _lib.HipExtensionError("HipAdam(max_grad_norm=): a graph capture needs one eager step first (it allocates the norm buffers)")
            self._norm_out = torch.zeros(2, device=grads[0].device, dtype=torch.float32)
            self.grad_norm = self._norm_out[0]
        arr = (_lib.NormItem * len(grads))()
        for it, g in zip(arr, grads):
            it.grad, it.n = g.data_ptr(), g.numel()
        check(lib.advhip_grad_norm_multi_f32(arr, len(grads), self.max_grad_norm, self._norm_partials.data_ptr(), self._norm_partials.numel(),
                                             self._norm_out.data_ptr(), self._norm_out.data_ptr() + 4, _lib.stream(grads[0])), "grad_norm_multi")

    def _bind_steps(self, params, live):
        """Every parameter's `step` as a view of ONE flat tensor (slot i = parameter i), so that `+= 1` for all of them is one
        launch; re-bound whenever the state was replaced from outside (load_state_dict hands every parameter a tensor of its own).
        State is created lazily, for the parameters in `live` (those with a gradient) only -- as torch.optim.Adam does, so that the
        state_dict of a model with frozen parameters has the same entries."""
        flat = self._steps
        ok = flat is not None and flat.numel() == len(params)
        if ok:
            base = flat.data_ptr()
            live_ids = {id(p) for p in live}
            for i, p in enumerate(params):
                st = self.state.get(p)
                if st:
                    ok = ok and "step" in st and torch.is_tensor(st["step"]) and st["step"].data_ptr() == base + 4 * i
                elif id(p) in live_ids:
                    ok = False
        if ok:
            return flat
        dev = params[0].device
        vals = [float(self.state[p]["step"]) if p in self.state and "step" in self.state[p] else 0.0 for p in params]
        flat = torch.tensor(vals, device=dev, dtype=torch.float32)
        live_ids = {id(p) for p in live}
        for i, p in enumerate(params):
            if p not in self.state and id(p) not in live_ids:
                continue
            st = self.state[p]
            st["step"] = flat[i]
            if "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        self._steps = flat
        return flat

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        every = [p for g in self.param_groups for p in g["params"]]
        if not every:
            return loss
        for p in every:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise _lib.HipExtensionError("HipAdam updates contiguous fp32 parameters on the GPU (use torch.optim.Adam for anything else)")
        # (the counters of ALL parameters: a parameter without a gradient this step keeps its count, as in torch)
        capturing = torch.cuda.is_current_stream_capturing()
        with_grad = [p for p in every if p.grad is not None]
        if not capturing:
            self._bind_steps(every, with_grad)
        elif self._steps is None or any(p not in self.state for p in with_grad):
            raise _lib.HipExtensionError("HipAdam: a graph capture needs one eager step first (the step counters and moments are created with host -> device "
                                         "copies; train_graph.GraphedTrainStep runs that step)")
        dev_scalars = self.reads_device_scalars
        if dev_scalars:
            if not capturing:
                self.sync_lr()
            elif self._lr_dev is None or self._lr_dev.numel() != len(self.param_groups):
                raise _lib.HipExtensionError("HipAdam(device_lr / max_grad_norm): a graph capture needs one eager step first (it creates the "
                                             "device-side lr scalars)")
        keep = []  # fp32 contiguous copies of gradients that are neither, alive until the launches are issued

        def plain(p):
            g = p.grad
            if g.is_sparse:
                raise _lib.HipExtensionError("HipAdam does not take sparse gradients")
            if not g.is_contiguous() or g.dtype != torch.float32:
                g = g.contiguous().float()
                keep.append(g)
            return g

        grad_of = {}
        if self.max_grad_norm is not None and with_grad:
            # ONE norm over every group's live gradients, as clip_grad_norm_(model.parameters()) takes it
            grad_of = {id(p): plain(p) for p in with_grad}
            self._launch_grad_norm(lib, [grad_of[id(p)] for p in with_grad], capturing)
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("differentiable"):
                raise _lib.HipExtensionError("HipAdam: amsgrad / maximize / differentiable are not offered")
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            if len(live) == len(every):  # (every slot of the flat tensor is some parameter's live counter)
                self._steps.add_(1.0)
            else:
                torch._foreach_add_([self.state[p]["step"] for p in live], 1.0)
            arr = (_lib.AdamItem * len(live))()
            for it, p in zip(arr, live):
                g = grad_of[id(p)] if id(p) in grad_of else plain(p)
                st = self.state[p]
                it.param, it.grad, it.exp_avg, it.exp_avg_sq, it.step, it.n = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                                                                  st["step"].data_ptr(), p.numel())
            lr = group["lr"]
            if torch.is_tensor(lr):
                raise _lib.HipExtensionError("HipAdam: a tensor learning rate is not offered (float(lr) would synchronise, and cannot be captured)")
            b1, b2 = group["betas"]
            if dev_scalars:
                scale = self._norm_out.data_ptr() + 4 if self.max_grad_norm is not None else None
                check(lib.advhip_adam_multi_dev_f32(arr, len(live), self._lr_dev.data_ptr() + 8 * gi, scale, float(b1), float(b2), float(group["eps"]),
                                                    float(group["weight_decay"]), _lib.stream(live[0])), "adam_multi_dev")
                continue
            check(lib.advhip_adam_multi_f32(arr, len(live), float(lr), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                                            _lib.stream(live[0])), "adam_multi")
        return loss
