"""Fused dense Adam on the embedding tables (the optimiser step on the other side of the hot path):
`torch.optim.Adam(model.parameters(), lr=...)` of ncl.py:305, lightgcn.py:84, gcl.py:201 (with weight_decay) as ONE
streaming HIP kernel per parameter (gcr_adam_step_f32): reads p, g, m, v and writes p, m, v once (28 B per element).
Same update rule and defaults as torch.optim.Adam (no amsgrad, L2 weight_decay folded into the gradient).
`FusedSGD` is directau.py:214's `torch.optim.SGD(lr, momentum=0.9)` the same way (gcr_sgd_momentum_step_f32)."""
from __future__ import annotations

import torch

from . import _lib


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False):
        """capturable: keep the step count in device memory (gcr_adam_step_dev_f32), so that a step captured in a
        hipGraph replays with the current bias corrections (torch.optim.Adam's flag of the same name).  A checkpoint
        (`state_dict()` / `load_state_dict()`) resumes with either setting: the host count is synchronised on save and
        the int64 device count rebuilt from it on load."""
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=bool(capturable)))

    @torch.no_grad()
    def step(self, closure=None, extra_grads=None):
        """extra_grads: optional {param: [tensor, ...]} of up to two further gradient pieces per parameter that were
        NOT accumulated into p.grad; they are summed inside the kernel."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                _lib.require_cuda(p, p.grad)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("FusedAdam needs contiguous float32 parameters")
                st = self.state[p]
                if not st:
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("FusedAdam: the first step() must run eagerly (it allocates the state; inside a "
                                           "stream capture the allocation and the zero count would be replayed every time)")
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                    if group.get("capturable"):            # device-side step count, allocated with the rest of the state
                        st["step_dev"] = torch.zeros(1, dtype=torch.int64, device=p.device)
                st["step"] += 1
                extra = list((extra_grads or {}).get(p, []))
                if len(extra) > 2:
                    raise ValueError("at most two extra gradient pieces")
                g = p.grad.contiguous()
                ex = [e.contiguous() for e in extra] + [None, None]
                # the group's values and `step` are user and state_dict data (torch.optim.Adam allows a tensor lr and keeps
                # `step` as a tensor): these float() / int() convert, they are not wrappers around call-site numbers
                lr, eps, wd = float(group["lr"]), float(group["eps"]), float(group["weight_decay"])
                if group.get("capturable"):
                    if "step_dev" not in st:               # state loaded from a non-capturable run
                        if torch.cuda.is_current_stream_capturing():
                            raise RuntimeError("FusedAdam: no device step count yet; run one eager step() before capturing")
                        st["step_dev"] = torch.full((1,), st["step"] - 1, dtype=torch.int64, device=p.device)
                    st["step_dev"].add_(1)
                    _lib.call("gcr_adam_step_dev_f32", p, g, ex[0], ex[1], st["exp_avg"], st["exp_avg_sq"], p.numel(), lr,
                              float(b1), float(b2), eps, wd, st["step_dev"], 1.0, on=p)
                    continue
                _lib.call("gcr_adam_step_f32", p, g, ex[0], ex[1], st["exp_avg"], st["exp_avg_sq"], p.numel(), lr,
                          float(b1), float(b2), eps, wd, int(st["step"]), 1.0, on=p)
        return loss

    def sync_step_counts(self):
        """Host step counts <- device step counts (one read-back per capturable parameter): graph replays advance only the
        device counter.  `state_dict()` calls it, so that a checkpoint resumed on either path gets the right bias corrections."""
        for st in self.state.values():
            if "step_dev" in st:
                st["step"] = int(st["step_dev"].item())

    def state_dict(self):
        self.sync_step_counts()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict, with the device step count rebuilt.  The base class casts every state
        tensor but `step` to the parameter's dtype, which would turn a saved int64 `step_dev` into float32 (the kernel
        reads 8 bytes of it).  So a capturable group gets a fresh int64 `step_dev` equal to the host `step` (which
        `state_dict()` synchronised), on the parameter's device; a non-capturable group drops it, because a stale device
        count would overwrite the host one at the next `state_dict()`.  Each group also keeps its own `capturable`
        flag rather than the checkpoint's: the flag says how this optimiser runs (graph replay or not), not what it
        computes, so a checkpoint resumes on either path."""
        modes = [bool(g.get("capturable")) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, capturable in zip(self.param_groups, modes):
            group["capturable"] = capturable
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                st.pop("step_dev", None)
                if capturable:
                    st["step_dev"] = torch.full((1,), int(st["step"]), dtype=torch.int64, device=p.device)


class FusedSGD(torch.optim.Optimizer):
    """`torch.optim.SGD(params, lr, momentum=0.9)` of directau.py:214 (dampening 0, no nesterov, L2 weight_decay folded
    into the gradient) as ONE streaming HIP kernel per parameter (gcr_sgd_momentum_step_f32): buf = g on the first step,
    buf = momentum * buf + g after it, p -= lr * buf.  The group keys and the state key (`momentum_buffer`) are
    torch.optim.SGD's, so `state_dict()` / `load_state_dict()` pass between the two."""

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=0.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameters")
        # torch.optim.SGD's own defaults for this torch version, so that the param_groups of the two carry the same keys
        defaults = dict(torch.optim.SGD([torch.zeros(1)], lr=lr, momentum=momentum, weight_decay=weight_decay).defaults)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            mu = float(group["momentum"])
            # a torch.optim.SGD state_dict can load these into the group: the kernel implements one setting of them
            if group.get("nesterov") or group.get("dampening", 0) != 0 or group.get("maximize"):
                raise ValueError("FusedSGD implements dampening = 0, nesterov = False, maximize = False only")
            for p in group["params"]:
                if p.grad is None:
                    continue
                _lib.require_cuda(p, p.grad)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("FusedSGD needs contiguous float32 parameters")
                st = self.state[p]
                buf, first = None, False
                if mu != 0.0:
                    buf = st.get("momentum_buffer")
                    first = buf is None
                    if first:
                        buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                g = p.grad.contiguous()
                _lib.call("gcr_sgd_momentum_step_f32", p, g, buf, p.numel(), float(group["lr"]), mu, float(group["weight_decay"]),
                          first, on=p)
        return loss
