"""The optimizer step of the training loop on the GPU: torch.optim.Adam's update for every parameter of every sub-model
in ONE HIP launch (csrc/optim.hip, sc_adam_step).

The reference keeps one `torch.optim.Adam(l, lr=0.0, eps=1e-15)` with seven groups per sub-model (gaussian_model.py:
293-305) and steps them one after the other (street_gaussian_model.py:467-484): tens of `step()` calls, each about a
dozen multi-tensor launches.  Here

    Adam(params, ...)          a torch.optim.Optimizer with torch.optim.Adam's constructor signature and state layout
                               (state[p]["step"], ["exp_avg"], ["exp_avg_sq"]): state_dict() / load_state_dict() are
                               interchangeable with torch.optim.Adam's, and code that edits `optimizer.state` and
                               `param_groups` by hand (gaussian_model.py:344-408: reset / prune / cat) keeps working
    step_many(optimizers)      steps several of them through one table, i.e. one launch for the whole scene

The formula is torch's (no amsgrad, no weight decay), per element in fp32; see include/street_crafter_amd.h.  A
parameter whose .grad is None is skipped as torch skips it: its step count does not advance, its moments do not decay.
`param_groups` is read afresh on every call (the learning rate changes per iteration, parameters are replaced at
densification).  step_many() does not run the optimizers' step hooks.

fp32 parameters on a HIP device only; there is no CPU path.  Everything is checked before anything is modified.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch

from . import _lib
from . import rendering as _r

__all__ = ["Adam", "step_many"]

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


def _refuse_options(options: dict, what: str):
    if options.get("weight_decay", 0) != 0:
        raise NotImplementedError(f"{what}: weight_decay != 0 is not implemented (the fused kernel has no decay term)")
    for key in _UNSUPPORTED:
        if options.get(key, False):
            raise NotImplementedError(f"{what}: {key}=True is not implemented")


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam through the fused HIP kernel.  `foreach` / `fused` / `decoupled_weight_decay` are accepted for
    signature and state_dict compatibility and have no effect: there is one route."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 foreach: Optional[bool] = None, maximize: bool = False, capturable: bool = False,
                 differentiable: bool = False, fused: Optional[bool] = None, decoupled_weight_decay: bool = False):
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        _refuse_options(defaults, "street_crafter_amd.optim.Adam")
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        _refuse_options(param_group, "street_crafter_amd.optim.Adam.add_param_group")
        super().add_param_group(param_group)

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        step_many([self])
        return loss


def _check_param(p, state):
    """Everything that can be refused about one parameter with a gradient; modifies nothing."""
    what = "street_crafter_amd.optim.Adam.step"
    if not p.is_cuda:
        raise RuntimeError(f"{what}: parameters must live on a HIP device (got {p.device}); "
                           "street_crafter_amd has no CPU path")
    if p.dtype != torch.float32:
        raise ValueError(f"{what}: parameters must be float32, got {p.dtype}")
    if not p.is_contiguous():
        raise ValueError(f"{what}: parameters must be contiguous (shape {tuple(p.shape)}, strides {p.stride()})")
    g = p.grad
    if g.is_sparse:
        raise NotImplementedError(f"{what}: sparse gradients are not implemented")
    if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
        raise ValueError(f"{what}: a gradient must match its parameter (float32 {tuple(p.shape)} on {p.device}), got "
                         f"{g.dtype} {tuple(g.shape)} on {g.device}")
    if state:
        for key in ("exp_avg", "exp_avg_sq"):
            m = state.get(key)
            if not isinstance(m, torch.Tensor) or m.dtype != torch.float32 or m.device != p.device \
                    or m.shape != p.shape or not m.is_contiguous():
                raise ValueError(f"{what}: state[{key!r}] must be a contiguous float32 tensor of the parameter's shape "
                                 f"{tuple(p.shape)} on {p.device}")
        if "step" not in state:
            raise ValueError(f"{what}: state without a step count")


def _advance(state) -> float:
    """step += 1 in torch's representation (a 0-d CPU tensor; a plain number in old checkpoints) -> the new count."""
    step = state["step"]
    if isinstance(step, torch.Tensor):
        step += 1
        return step.item()
    state["step"] = step + 1
    return state["step"]


@torch.no_grad()
def step_many(optimizers: Iterable[Adam]) -> None:
    """One Adam step of every optimizer in `optimizers` (street_crafter_amd.optim.Adam instances) through one table:
    what the loop over sub-models in StreetGaussianModel.update_optimizer does, in one launch per 64 tensors."""
    optimizers = list(optimizers)
    todo = []                                              # (optimizer, group, parameter)
    for opt in optimizers:
        if not isinstance(opt, Adam):
            raise TypeError(f"step_many: expected street_crafter_amd.optim.Adam, got {type(opt).__name__}")
        for group in opt.param_groups:
            _refuse_options(group, "street_crafter_amd.optim.Adam.step")
            for p in group["params"]:
                if p.grad is None:
                    continue
                _check_param(p, opt.state.get(p))
                todo.append((opt, group, p))
    # nothing was refused: from here on state is created and advanced
    calls = {}                                             # (device, beta1, beta2, eps) -> the lists of one launch table
    for opt, group, p in todo:
        state = opt.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float64 if torch.get_default_dtype() == torch.float64
                                         else torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        t = _advance(state)
        beta1, beta2 = group["betas"]
        beta1, beta2, lr, eps = float(beta1), float(beta2), float(group["lr"]), float(group["eps"])
        step_size = lr / (1.0 - beta1 ** t)                # in double, as torch's _single_tensor_adam
        bias2_sqrt = (1.0 - beta2 ** t) ** 0.5
        g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
        lists = calls.setdefault((p.device, beta1, beta2, eps), ([], [], [], [], [], []))
        for lst, item in zip(lists, (p, g, state["exp_avg"], state["exp_avg_sq"], step_size, bias2_sqrt)):
            lst.append(item)
    for (device, beta1, beta2, eps), lists in calls.items():
        _launch(lists, 1.0 - beta1, beta2, 1.0 - beta2, eps)


def _launch(lists, one_minus_beta1: float, beta2: float, one_minus_beta2: float, eps: float):
    params, grads, exp_avg, exp_avg_sq, step_size, bias2_sqrt = lists
    rc = _lib.binding().adam_step(params, grads, exp_avg, exp_avg_sq, step_size, bias2_sqrt, one_minus_beta1, beta2,
                                  one_minus_beta2, eps, _r._stream(params[0]))
    if rc:
        _lib.check(rc, "sc_adam_step")

