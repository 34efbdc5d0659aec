"""FusedAdamW: gradient clipping, the AdamW update and a weight EMA as one optimiser step on HIP kernels (ops.adamw_step).

It replaces the reference drivers' three-part step (experiments/imagenet_ab_param_budgets.py:699-716)

    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
    optimizer.step()
    for e, p in zip(ema_params, model.parameters()): e.mul_(d).add_(p, alpha=1 - d)

with `FusedAdamW(model.parameters(), ..., max_grad_norm=max_norm, ema_decay=d).step()`.  A step makes no host synchronisation and
no host-to-device copy; with stable gradient pointers it can be captured in a HIP graph.  Steps that the kernels do not take (CPU
tensors, other dtypes, non-contiguous parameters) run the same arithmetic in torch ops (ops.adamw_step_torch).
"""
from __future__ import annotations

import contextlib
from typing import List, Optional

import torch

from . import ops

__all__ = ["FusedAdamW"]


def _like_param(p: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """zeros of p's shape and of `dtype` that sit as p does relative to a 16-byte boundary, so the kernels read p, its moments and
    its EMA in vectors from the same element on (a parameter may be a view that starts at any element of its storage)"""
    if not p.is_contiguous():
        return torch.zeros_like(p, dtype=dtype, memory_format=torch.preserve_format)
    phase = (p.data_ptr() % 16) // p.element_size()
    buf = torch.zeros(phase + p.numel(), dtype=dtype, device=p.device)
    return buf[phase:].view(p.shape)


class FusedAdamW(torch.optim.Optimizer):
    """AdamW with decoupled weight decay (torch.optim.AdamW's arithmetic), optional global gradient-norm clipping, an optional EMA
    of the weights and an optional skip of steps whose gradient norm is not finite.

    State per parameter, under torch's keys: `step` (an fp32 scalar on the parameter's device), `exp_avg`, `exp_avg_sq` (always
    fp32, also for bf16 parameters: a bf16 second moment underflows) and, with ema_decay, `ema` (the parameter's dtype, initialised
    to the parameter).  `state_dict()` loads into torch.optim.AdamW and the reverse; moments that arrive in another dtype become fp32.
    `lr` is a float (schedulers write it) or a one-element fp32 device tensor (captured steps read it on replay).
    A parameter without a gradient is skipped and its step does not advance.  All parameters live on one device.
    `p.grad` is never modified: the clip coefficient multiplies the gradient inside the update."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm: Optional[float] = None,
                 ema_decay: Optional[float] = None, skip_nonfinite: bool = False, amsgrad: bool = False, maximize: bool = False):
        if amsgrad or maximize:
            raise ValueError("FusedAdamW does not support amsgrad or maximize")
        if not isinstance(lr, torch.Tensor) and not lr >= 0.0:
            raise ValueError(f"invalid learning rate: {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas: {betas}")
        if not eps >= 0.0 or not weight_decay >= 0.0:
            raise ValueError(f"invalid eps / weight_decay: {eps}, {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"invalid max_grad_norm: {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= ema_decay <= 1.0:
            raise ValueError(f"invalid ema_decay: {ema_decay}")
        self.max_grad_norm, self.ema_decay, self.skip_nonfinite = max_grad_norm, ema_decay, bool(skip_nonfinite)
        self._stats = None          # int32 (4,): MopkAdamWStats
        self._cache = {}
        # torch.optim.AdamW's own group keys travel with a checkpoint, so that it loads ours as what it is (a group without
        # decoupled_weight_decay would be read as Adam with L2 decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                                      capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True))
        for group in self.param_groups:
            for p in group["params"]:
                if p.is_complex():
                    raise ValueError("FusedAdamW does not support complex parameters")

    # ---- state ----
    def _stats_on(self, device) -> torch.Tensor:
        if self._stats is None or self._stats.device != device:
            skipped = 0 if self._stats is None else self._stats[3].to(device)
            self._stats = torch.zeros(4, dtype=torch.int32, device=device)
            self._stats.view(torch.float32)[0] = float("nan")       # no norm taken yet
            self._stats.view(torch.float32)[1] = 1.0
            self._stats[3] = skipped
        return self._stats

    def _device(self):
        for group in self.param_groups:
            for p in group["params"]:
                return p.device
        return torch.device("cpu")

    @property
    def grad_norm(self) -> torch.Tensor:
        """total gradient norm of the last step before clipping, what clip_grad_norm_ returns: an fp32 scalar on the parameters'
        device (NaN until a step with max_grad_norm or skip_nonfinite has run)"""
        return self._stats_on(self._device()).view(torch.float32)[0]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """number of steps skipped for a non-finite gradient norm: an int32 scalar on the parameters' device"""
        return self._stats_on(self._device())[3]

    def _init_state(self, p: torch.Tensor) -> dict:
        st = self.state[p]
        if "step" not in st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = _like_param(p, torch.float32)
            st["exp_avg_sq"] = _like_param(p, torch.float32)
        if self.ema_decay is not None and "ema" not in st:
            st["ema"] = _like_param(p, p.dtype)
            st["ema"].copy_(p.detach())
        return st

    def load_state_dict(self, state_dict) -> None:
        """torch's loader, then the state as the kernels keep it: `step` an fp32 scalar on the parameter's device; `exp_avg` and
        `exp_avg_sq` fp32 whatever dtype arrives, taken from the incoming values (torch's loader casts them to the parameter's
        dtype, which would round fp32 moments of a bf16 parameter); every state tensor laid out like its parameter"""
        super().load_state_dict(state_dict)
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, params):
            st, src = self.state.get(p), state_dict["state"].get(i)
            if not st or src is None:
                continue
            step = st["step"]
            st["step"] = (step.detach().clone() if isinstance(step, torch.Tensor) else torch.tensor(float(step))).to(
                device=p.device, dtype=torch.float32).reshape(())
            for k in ("exp_avg", "exp_avg_sq"):
                t = _like_param(p, torch.float32)
                t.copy_(src[k])
                st[k] = t
            if "ema" in st:
                t = _like_param(p, p.dtype)
                t.copy_(src["ema"])
                st["ema"] = t
        self._cache.clear()

    # ---- EMA access ----
    def ema_parameters(self) -> List[torch.Tensor]:
        """the EMA tensors in parameter order (created on first use, equal to the parameters then)"""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW was built without ema_decay")
        return [self._init_state(p)["ema"] for group in self.param_groups for p in group["params"]]

    @contextlib.contextmanager
    def swap_ema(self):
        """exchange the parameters and their EMA in place (evaluate the averaged weights), and exchange them back on exit"""
        pairs = list(zip([p for group in self.param_groups for p in group["params"]], self.ema_parameters()))

        def swap():
            with torch.no_grad():
                for p, e in pairs:
                    tmp = p.detach().clone()
                    p.copy_(e)
                    e.copy_(tmp)
        swap()
        try:
            yield self
        finally:
            swap()

    # ---- the step ----
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = []
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdamW does not support amsgrad or maximize")
            ps, gs, ms, vs, steps, emas = [], [], [], [], [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError("FusedAdamW does not support sparse gradients")
                st = self._init_state(p)
                ps.append(p)
                gs.append(p.grad)
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
                steps.append(st["step"])
                if self.ema_decay is not None:
                    emas.append(st["ema"])
            b1, b2 = group["betas"]
            groups.append(dict(params=ps, grads=gs, exp_avgs=ms, exp_avg_sqs=vs, steps=steps, emas=emas if self.ema_decay is not None else None,
                               lr=group["lr"], beta1=b1, beta2=b2, eps=group["eps"], weight_decay=group["weight_decay"]))
        ops.adamw_step(groups, max_grad_norm=self.max_grad_norm, ema_decay=self.ema_decay, skip_nonfinite=self.skip_nonfinite,
                       stats=self._stats_on(self._device()), cache=self._cache)
        return loss
