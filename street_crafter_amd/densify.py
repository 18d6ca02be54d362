"""Densify and prune on the GPU: clone, split and prune of any number of sub-models in one pass (csrc/densify.hip,
sc_densify_plan + sc_densify_apply).

The reference runs, every 100 iterations (train.py:292-299), StreetGaussianModel.densify_and_prune
(street_gaussian_model.py:535-549): per sub-model densify_and_clone, densify_and_split and prune_points
(gaussian_model.py:363-547, gaussian_model_bkgd.py:100-157, gaussian_model_actor.py:201-272).  That is `cat`, `cat`, then a
mask over all seven parameters and their Adam moments, dozens of boolean-mask indexings (a `nonzero` and a host wait each)
and a `.sum().item()` per counter, per sub-model.  Here

    densify_and_prune_many(jobs)    one DensifyJob per sub-model: ONE host round trip for all of them (the new row
                                    counts must reach the host to allocate) and ONE read and ONE write of every parameter
                                    and moment

The selection rule is DensificationStats.clone_split_masks; the full statement of what is computed is in
include/street_crafter_amd.h.  The function replaces each group's nn.Parameter and moves the optimizer state across as
cat_optimizer / prune_optimizer do (`step` kept, `exp_avg` / `exp_avg_sq` replaced, new rows' moments zero; a group
without state gets only the parameter).  It works on street_crafter_amd.optim.Adam and torch.optim.Adam alike.

Not covered: the sky model (its extent is a top-k statistic recomputed between split and prune, gaussian_model_sky.py:
48-60, 90, 103: a second round trip in the middle; it keeps the reference path, which works with optim.Adam),
`background_mask`, `reset_opacity`; torch.cuda.empty_cache() is not called.

fp32 parameters on a HIP device only; there is no CPU path.  Everything is checked before anything is modified.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _lib
from . import optim as _optim
from . import rendering as _r

__all__ = ["DensifyJob", "DensifyResult", "densify_and_prune_many", "scan_block", "COUNTERS"]

COUNTERS = ("points_total", "points_clone", "points_split", "points_below_min_opacity", "points_big_ws", "points_pruned")


def scan_block() -> int:
    """Rows per block of the plan's scan (the sizes at which the kernels change path are its multiples)."""
    return _lib.load().sc_densify_scan_block()


@dataclass
class DensifyJob:
    """One sub-model.  `optimizer` holds one named group per tensor (gaussian_model.py:293-305); `xyz`, `scaling`,
    `rotation`, `opacity` name the groups the decisions read, `passengers` the groups that are only moved.  The three
    statistics tensors are DensificationStats' (xyz_gradient_accum [n,2], denom [n,1], max_radii2D [n]).
    `use_abs`: column 1 of xyz_gradient_accum (the densify_grad_abs_* variants).  `prune_big_points` with
    `sphere=(center, radius)` is the background's rule (gaussian_model_bkgd.py:125-138), with `box=(min_xyz, max_xyz)` the
    actors' (gaussian_model_actor.py:226-251); centre and corners are three numbers each (a device tensor is read back:
    pass numbers).  `split_noise` [2,n,3] and `box_noise` [4,n,2,3] are standard normals indexed by original row and by
    child / slot; absent, they are drawn with torch.randn."""
    optimizer: torch.optim.Optimizer
    xyz_gradient_accum: torch.Tensor
    denom: torch.Tensor
    max_radii2D: torch.Tensor
    max_grad: float
    extent: float
    min_opacity: float
    percent_dense: float = 0.01
    use_abs: bool = False
    prune_big_points: bool = False
    percent_big_ws: float = 0.1
    max_screen_size: Optional[float] = None
    sphere: Optional[Tuple[Sequence[float], float]] = None
    box: Optional[Tuple[Sequence[float], Sequence[float]]] = None
    split_noise: Optional[torch.Tensor] = None
    box_noise: Optional[torch.Tensor] = None
    xyz: str = "xyz"
    scaling: str = "scaling"
    rotation: str = "rotation"
    opacity: str = "opacity"
    passengers: Sequence[str] = ("f_dc", "f_rest", "semantic")


@dataclass
class DensifyResult:
    """`params`: the new nn.Parameters by group name (already installed in the optimizer); the three statistics tensors
    zeroed at the new length (gaussian_model.py:545-547; views of one buffer per call); `scalar_dict`: the reference's
    counters; `src_row` int32 [n'] / `slot` uint8 [n']: where each new row came from (slot 0 the original row, 1 its
    clone, 2 / 3 its split children)."""
    params: Dict[str, nn.Parameter]
    xyz_gradient_accum: torch.Tensor
    denom: torch.Tensor
    max_radii2D: torch.Tensor
    scalar_dict: Dict[str, int]
    src_row: torch.Tensor
    slot: torch.Tensor
    n_out: int = field(default=0)


_WHAT = "densify_and_prune_many"


def _shape_check(where: str, name: str, t, shapes) -> None:
    """Type, dtype, layout and shape of one tensor; modifies nothing.  (The device is checked afterwards, so that a
    malformed tensor is reported as such wherever it lives.)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{_WHAT}: {where}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{_WHAT}: {where}: {name} must be float32, got {t.dtype}")
    if shapes is not None and tuple(t.shape) not in shapes:
        raise ValueError(f"{_WHAT}: {where}: {name} must have shape {' or '.join(str(s) for s in shapes)}, got "
                         f"{tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{_WHAT}: {where}: {name} must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")


def _three(where: str, name: str, v) -> List[float]:
    if isinstance(v, torch.Tensor):
        v = v.detach().reshape(-1).tolist()
    v = [float(x) for x in v]
    if len(v) != 3:
        raise ValueError(f"{_WHAT}: {where}: {name} must be three numbers, got {len(v)}")
    return v


class _Checked:
    """What the checks of one job established: the groups in table order, their parameters and state."""
    __slots__ = ("job", "n", "names", "groups", "params", "states", "fparams", "iparams", "device", "need_box", "tensors")


def _check_job(k: int, job: DensifyJob) -> _Checked:
    where = f"job {k}"
    if not isinstance(job, DensifyJob):
        raise TypeError(f"{_WHAT}: {where}: expected a DensifyJob, got {type(job).__name__}")
    opt = job.optimizer
    if not isinstance(opt, (torch.optim.Adam, _optim.Adam)):
        raise TypeError(f"{_WHAT}: {where}: optimizer must be street_crafter_amd.optim.Adam or torch.optim.Adam, got "
                        f"{type(opt).__name__}")
    # ---- numbers ---------------------------------------------------------------------------------------------------
    max_grad = float(job.max_grad)
    if not max_grad > 0.0:
        raise ValueError(f"{_WHAT}: {where}: max_grad must be > 0 (a clone has gradient 0 and would qualify for "
                         f"splitting), got {job.max_grad}")
    if job.sphere is not None and job.box is not None:
        raise ValueError(f"{_WHAT}: {where}: give a sphere (background) or a box (actor), not both")
    for name in ("extent", "percent_dense", "min_opacity", "percent_big_ws"):
        if not math.isfinite(float(getattr(job, name))):
            raise ValueError(f"{_WHAT}: {where}: {name} must be finite, got {getattr(job, name)}")
    max_screen = 0.0 if not job.max_screen_size else float(job.max_screen_size)       # `if self.max_screen_size:`
    if not max_screen >= 0.0:
        raise ValueError(f"{_WHAT}: {where}: max_screen_size must be None or >= 0, got {job.max_screen_size}")
    region, a, b = 0, [0.0] * 3, [0.0] * 3
    if job.sphere is not None:
        region, a, b = 1, _three(where, "sphere centre", job.sphere[0]), [float(job.sphere[1]), 0.0, 0.0]
    elif job.box is not None:
        region, a, b = 2, _three(where, "box min_xyz", job.box[0]), _three(where, "box max_xyz", job.box[1])
    # ---- groups ----------------------------------------------------------------------------------------------------
    names = [job.xyz, job.scaling, job.rotation, job.opacity, *job.passengers]
    if len(set(names)) != len(names):
        raise ValueError(f"{_WHAT}: {where}: a group is named twice in {names}")
    by_name = {}
    for g in opt.param_groups:
        if g.get("name") in by_name:
            raise ValueError(f"{_WHAT}: {where}: the optimizer has two groups named {g.get('name')!r}")
        by_name[g.get("name")] = g
    groups = []
    for name in names:
        if name not in by_name:
            raise ValueError(f"{_WHAT}: {where}: the optimizer has no group named {name!r}")
        if len(by_name[name]["params"]) != 1:
            raise ValueError(f"{_WHAT}: {where}: group {name!r} must hold exactly one parameter")
        groups.append(by_name[name])
    params = [g["params"][0] for g in groups]
    if params[0].dim() < 1:
        raise ValueError(f"{_WHAT}: {where}: {job.xyz} must be [n,3]")
    n = params[0].shape[0]
    fixed = {job.xyz: ((n, 3),), job.scaling: ((n, 3),), job.rotation: ((n, 4),), job.opacity: ((n, 1), (n,))}
    states = []
    for name, p in zip(names, params):
        _shape_check(where, name, p, fixed.get(name))
        if p.dim() < 1 or p.shape[0] != n:
            raise ValueError(f"{_WHAT}: {where}: {name} must have {n} rows, got shape {tuple(p.shape)}")
        state = opt.state.get(p)
        if state:
            for key in ("exp_avg", "exp_avg_sq"):
                _shape_check(where, f"{name} state[{key!r}]", state.get(key), (tuple(p.shape),))
            if "step" not in state:
                raise ValueError(f"{_WHAT}: {where}: {name}: state without a step count")
        states.append(state if state else None)
    _shape_check(where, "xyz_gradient_accum", job.xyz_gradient_accum, ((n, 2),))
    _shape_check(where, "denom", job.denom, ((n, 1), (n,)))
    _shape_check(where, "max_radii2D", job.max_radii2D, ((n,),))
    need_box = bool(job.prune_big_points) and region == 2
    if job.split_noise is not None:
        _shape_check(where, "split_noise", job.split_noise, ((2, n, 3),))
    if job.box_noise is not None:
        _shape_check(where, "box_noise", job.box_noise, ((4, n, 2, 3),))
    tensors = [(nm, p) for nm, p in zip(names, params)]
    tensors += [("xyz_gradient_accum", job.xyz_gradient_accum), ("denom", job.denom), ("max_radii2D", job.max_radii2D)]
    tensors += [(f"{nm} state", s[key]) for nm, s in zip(names, states) if s for key in ("exp_avg", "exp_avg_sq")]
    tensors += [(nm, t) for nm, t in (("split_noise", job.split_noise), ("box_noise", job.box_noise)) if t is not None]
    c = _Checked()
    c.job, c.n, c.names, c.groups, c.params, c.states, c.need_box = job, n, names, groups, params, states, need_box
    c.device, c.tensors = params[0].device, tensors
    c.fparams = [max_grad, float(job.percent_dense) * float(job.extent), float(job.min_opacity),
                 float(job.extent) * float(job.percent_big_ws), max_screen, *a, *b]
    c.iparams = [1 if job.use_abs else 0, 1 if job.prune_big_points else 0, region]
    return c


@torch.no_grad()
def densify_and_prune_many(jobs: Sequence[DensifyJob], *, generator: Optional[torch.Generator] = None
                           ) -> List[DensifyResult]:
    """densify_and_prune of every sub-model in `jobs` (see DensifyJob): what the loop of
    StreetGaussianModel.densify_and_prune does for the background and the actors, with one host round trip.  Returns one
    DensifyResult per job, in order.  Missing noise is drawn with torch.randn(..., generator=generator)
    (torch.normal(0, std) is randn * std, so the distribution is the reference's)."""
    jobs = list(jobs)
    checked = [_check_job(k, job) for k, job in enumerate(jobs)]
    if not checked:
        return []
    # (devices after every job's shapes, so that a malformed job is reported as such wherever its tensors live)
    device = checked[0].device
    for k, c in enumerate(checked):
        for name, t in c.tensors:
            if not t.is_cuda:
                raise RuntimeError(f"{_WHAT}: job {k}: {name} must live on a HIP device (got {t.device}); "
                                   "street_crafter_amd has no CPU path")
            if t.device != device:
                raise ValueError(f"{_WHAT}: job {k}: {name} lives on {t.device}, job 0 on {device}: one device per call")
    # nothing was refused: from here on tensors are allocated, and the optimizers are modified once both calls returned
    binding = _lib.binding()
    lists = [[] for _ in range(9)]
    fparams, iparams = [], []
    for c in checked:
        job, p = c.job, dict(zip(c.names, c.params))
        split_noise = job.split_noise if job.split_noise is not None else \
            torch.randn((2, c.n, 3), generator=generator, device=device, dtype=torch.float32)
        box_noise = job.box_noise
        if box_noise is None and c.need_box:
            box_noise = torch.randn((4, c.n, 2, 3), generator=generator, device=device, dtype=torch.float32)
        for lst, t in zip(lists, (p[job.xyz].detach(), p[job.scaling].detach(), p[job.rotation].detach(),
                                  p[job.opacity].detach(), job.xyz_gradient_accum, job.denom, job.max_radii2D,
                                  split_noise, box_noise if c.need_box else None)):
            lst.append(t)
        fparams += c.fparams
        iparams += c.iparams
    stream = _r._stream(checked[0].params[0])
    rc, counters, src_row, slot, child_xyz, child_scaling = binding.densify_plan(*lists, fparams, iparams, stream)
    if rc:
        _lib.check(rc, "sc_densify_plan")
    host = counters.cpu().tolist()                          # the one host round trip of the call
    n_outs = [row[6] for row in host]
    cols = [[] for _ in range(9)]                           # src, exp_avg, exp_avg_sq, child, src_row, slot, n, n_out, width
    for k, c in enumerate(checked):
        for name, p, state in zip(c.names, c.params, c.states):
            child = child_xyz[k] if name == c.job.xyz else child_scaling[k] if name == c.job.scaling else None
            width = math.prod(p.shape[1:])
            for col, item in zip(cols, (p.detach(), state["exp_avg"] if state else None,
                                        state["exp_avg_sq"] if state else None, child, src_row[k], slot[k], c.n,
                                        n_outs[k], width)):
                col.append(item)
    rc, new_p, new_m, new_v = binding.densify_apply(*cols, stream)
    if rc:
        _lib.check(rc, "sc_densify_apply")
    zeros = torch.zeros(4 * sum(n_outs), dtype=torch.float32, device=device)      # the statistics of every job: one fill
    results, g, z = [], 0, 0
    for k, c in enumerate(checked):
        opt, n_out, out = c.job.optimizer, n_outs[k], {}
        for name, group, p, state in zip(c.names, c.groups, c.params, c.states):
            fresh = nn.Parameter(new_p[g].view(n_out, *p.shape[1:]).requires_grad_(True))
            if state is not None:                           # gaussian_model.py:369-378 / 393-403: `step` stays
                state["exp_avg"] = new_m[g].view(fresh.shape)
                state["exp_avg_sq"] = new_v[g].view(fresh.shape)
                del opt.state[p]
                opt.state[fresh] = state
            group["params"][0] = fresh
            out[name] = fresh
            g += 1
        results.append(DensifyResult(
            params=out, xyz_gradient_accum=zeros[z:z + 2 * n_out].view(n_out, 2),
            denom=zeros[z + 2 * n_out:z + 3 * n_out].view(n_out, 1), max_radii2D=zeros[z + 3 * n_out:z + 4 * n_out],
            scalar_dict=dict(zip(COUNTERS, host[k][:6])), src_row=src_row[k][:n_out], slot=slot[k][:n_out], n_out=n_out))
        z += 4 * n_out
    return results
