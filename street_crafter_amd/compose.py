"""The head of a frame on the GPU: what StreetGaussianModel.parse_camera and its five get_* properties do
(street_gaussian_model.py:202-407), in ONE HIP launch forward and one backward (csrc/compose.hip, sc_compose_fwd / bwd).

The reference turns the raw parameters of the background, every visible actor and the sky into the flat
`means / quats / scales / opacities / sh` arrays of a frame with a few small torch ops per sub-model and five `torch.cat`s,
and autograd walks all of it back.  Here

    plan_frame(models, actor_rows, include=...)       host only: which sub-models, in which order, at which rows
    compose_frame(models, obj_rots, obj_trans, frame) the arrays and `graph_gaussian_range`, differentiable with respect to
                                                      every raw parameter and the two pose tensors

Opt-in: nothing else in the package calls it; `scene_io.compose_scene` stays the CPU statement used to build scenes.

obj_rots [A,4] / obj_trans [A,3], the pose inputs here, are what street_crafter_amd.actor_pose.actor_poses returns: the
tracklet lookup, the opt_rots / opt_trans deltas and the slerp of validation frames (actor_pose.py:83-144) in one launch
of their own.  What stays on torch: the flip masks' random draw.  Host: visibility and the row
ranges; the IDFT basis of the frame (scene_io.idft, F numbers per actor).  The background mask (always None in the
reference) and semantics are not supported.

fp32 contiguous tensors on a HIP device only; there is no CPU path.  Formulas: include/street_crafter_amd.h.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from . import scene_io

__all__ = ["FrameModel", "FramePlan", "plan_frame", "compose_frame", "STATIC", "ACTOR", "SKY", "MAX_FOURIER",
           "DEFAULT_FLIP_Q"]

STATIC, ACTOR, SKY, MAX_FOURIER = (_lib.CONSTANTS["SC_COMPOSE_" + k] for k in ("STATIC", "ACTOR", "SKY", "MAX_FOURIER"))
# matrix_to_quaternion(diag(-1, 1, -1)): half a turn about y (street_gaussian_model.py:56-58)
DEFAULT_FLIP_Q = (0.0, 0.0, 1.0, 0.0)

_RAW = ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest")


@dataclass
class FrameModel:
    """One sub-model of the scene graph: its six raw (pre-activation) tensors and what its kind needs."""
    name: str
    kind: int                       # STATIC (background), ACTOR or SKY
    xyz: torch.Tensor               # [n,3]
    scaling: torch.Tensor           # [n,3]   log scale
    rotation: torch.Tensor          # [n,4]   wxyz, not normalised
    opacity: torch.Tensor           # [n,1]   logit
    features_dc: torch.Tensor       # [n,F,3] F = fourier_dim for actors
    features_rest: torch.Tensor     # [n,K-1,3]
    # actors: the time axis of the Fourier colour model (gaussian_model_actor.py:68-69)
    start_frame: int = 0
    end_frame: int = 1
    fourier_scale: float = 1.0
    # sky (gaussian_model_sky.py:62-76)
    centre: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    radius: float = 1.0

    @classmethod
    def wrap(cls, m: "scene_io.SubModel", kind: int, **kw) -> "FrameModel":
        """A scene_io.SubModel as a record of this module (the tensors are shared, not copied)."""
        return cls(name=m.name, kind=kind, xyz=m.xyz, scaling=m.scaling, rotation=m.rotation, opacity=m.opacity,
                   features_dc=m.features_dc, features_rest=m.features_rest, start_frame=m.start_frame,
                   end_frame=m.end_frame, fourier_scale=m.fourier_scale, **kw)

    @property
    def n(self) -> int:
        return int(self.xyz.shape[0])


@dataclass
class FramePlan:
    """Row ranges as StreetGaussianModel.graph_gaussian_range has them, and the segment table in frame order."""
    ranges: Dict[str, List[int]] = field(default_factory=dict)       # name -> [start, end]
    segments: List[dict] = field(default_factory=list)               # name, kind, start, end, pose_row (-1: none)
    n: int = 0

    @property
    def order(self) -> List[str]:
        return [s["name"] for s in self.segments]


def plan_frame(models: Sequence[FrameModel], actor_rows: Optional[Dict[str, int]], *,
               include: Optional[Sequence[str]] = None, frame=None) -> FramePlan:
    """Host only.  Order: background, visible actors in list order, sky (street_gaussian_model.py:216-241).
    `actor_rows[name]` is the actor's row of obj_rots / obj_trans; an actor without one is not visible.  With `frame`, an
    actor whose [start_frame, end_frame] does not contain it is left out (:229).  `actor_rows=None`: the included actors
    that pass the frame rule take rows 0, 1, ... in list order (graph_obj_list).  `include` restricts the sub-models, as
    set_visibility does for render_object / render_background (street_gaussian_renderer.py:64-104)."""
    seen = set()
    for m in models:
        if m.kind not in (STATIC, ACTOR, SKY):
            raise ValueError(f"plan_frame: {m.name}: unknown kind {m.kind!r}")
        if m.name in seen:
            raise ValueError(f"plan_frame: two sub-models named {m.name!r}")
        seen.add(m.name)
    live = [m for m in models if include is None or m.name in include]

    in_range = lambda m: frame is None or m.start_frame <= frame <= m.end_frame
    if actor_rows is None:
        actor_rows = {m.name: i for i, m in enumerate(m for m in live if m.kind == ACTOR and in_range(m))}

    def visible(m):
        return m.kind != ACTOR or (m.name in actor_rows and in_range(m))

    picked = [m for m in live if m.kind == STATIC] + [m for m in live if m.kind == ACTOR and visible(m)] + \
             [m for m in live if m.kind == SKY]
    plan, at = FramePlan(), 0
    for m in picked:
        plan.ranges[m.name] = [at, at + m.n]
        plan.segments.append(dict(name=m.name, kind=m.kind, start=at, end=at + m.n,
                                  pose_row=int(actor_rows[m.name]) if m.kind == ACTOR else -1))
        at += m.n
    plan.n = at
    return plan


def _check_models(models: Sequence[FrameModel]) -> int:
    """Everything that can be refused about the raw tensors without a device -> K."""
    what = "street_crafter_amd.compose.compose_frame"
    K = None
    for m in models:
        n = m.n
        for attr, tail in zip(_RAW, ((3,), (3,), (4,), (1,), None, None)):
            t = getattr(m, attr)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise ValueError(f"{what}: {m.name}.{attr} must be a float32 tensor, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)}")
            if not t.is_contiguous():
                raise ValueError(f"{what}: {m.name}.{attr} must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
            if tail is not None and tuple(t.shape) != (n,) + tail:
                raise ValueError(f"{what}: {m.name}.{attr} must be {(n,) + tail}, got {tuple(t.shape)}")
        dc, rest = m.features_dc, m.features_rest
        if dc.dim() != 3 or dc.shape[0] != n or dc.shape[2] != 3 or rest.dim() != 3 or rest.shape[0] != n \
                or rest.shape[2] != 3:
            raise ValueError(f"{what}: {m.name}: features_dc must be [n,F,3] and features_rest [n,K-1,3], got "
                             f"{tuple(dc.shape)} and {tuple(rest.shape)}")
        if not 1 <= dc.shape[1] <= MAX_FOURIER:
            raise ValueError(f"{what}: {m.name}: fourier_dim {dc.shape[1]} outside [1, {MAX_FOURIER}]")
        k = rest.shape[1] + 1
        if K is not None and k != K:
            raise ValueError(f"{what}: sub-models with different K ({K} and {k}: {m.name}); the frame's sh is one [N,K,3]")
        K = k
    return K


@functools.lru_cache(maxsize=4096)
def _basis(t: float, dim: int) -> Tuple[float, ...]:
    """scene_io.idft's row at time t as python floats (the same fp32 values; kept, since a scene asks for the same few
    (time, dim) pairs again and again and each costs several small CPU tensor ops)"""
    return tuple(scene_io.idft(t, dim)[0].tolist())


class _Call:
    """The host side of one compose_frame: everything the two entry calls share."""
    __slots__ = ("lists", "flips", "ranges", "kinds", "pose_rows", "fparams", "N", "K", "A", "flip_q", "n_seg")


def _stream(t):
    from . import rendering as _r
    return _r._stream(t)


class _Compose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call: _Call, obj_rots, obj_trans, *raws):
        lists = [list(raws[k::6]) for k in range(6)]
        rc, means, quats, scales, opac, sh = _lib.binding().compose_fwd(
            *lists, call.flips, call.ranges, call.kinds, call.pose_rows, call.fparams, call.N, call.K, obj_rots,
            obj_trans, call.A, call.flip_q, _stream(raws[0]))
        if rc:
            _lib.check(rc, "sc_compose_fwd")
        ctx.call = call
        ctx.has_pose = obj_rots is not None
        ctx.save_for_backward(*([obj_rots, obj_trans] if ctx.has_pose else []), *raws)
        ctx.set_materialize_grads(False)
        return means, quats, scales, opac, sh

    @staticmethod
    def backward(ctx, g_means, g_quats, g_scales, g_opac, g_sh):
        call = ctx.call
        saved = ctx.saved_tensors
        obj_rots, obj_trans = (saved[0], saved[1]) if ctx.has_pose else (None, None)
        raws = saved[2:] if ctx.has_pose else saved
        lists = [list(raws[k::6]) for k in range(6)]
        ups = [None if g is None else g.contiguous() for g in (g_means, g_quats, g_scales, g_opac, g_sh)]
        want_rots = ctx.has_pose and ctx.needs_input_grad[1]
        want_trans = ctx.has_pose and ctx.needs_input_grad[2]
        out = _lib.binding().compose_bwd(*lists, call.flips, call.ranges, call.kinds, call.pose_rows, call.fparams,
                                         call.N, call.K, obj_rots, obj_trans, call.A, call.flip_q, *ups, want_rots,
                                         want_trans, _stream(raws[0]))
        if out[0]:
            _lib.check(out[0], "sc_compose_bwd")
        grads = [None] * (6 * call.n_seg)
        for k in range(6):
            grads[k::6] = out[1 + k]
        return (None, out[7], out[8], *grads)


def compose_frame(models: Sequence[FrameModel], obj_rots: Optional[torch.Tensor], obj_trans: Optional[torch.Tensor],
                  frame, *, flip: Optional[Dict[str, torch.Tensor]] = None, flip_q: Optional[Sequence[float]] = None,
                  actor_rows: Optional[Dict[str, int]] = None, include: Optional[Sequence[str]] = None):
    """-> (means [N,3], quats [N,4], scales [N,3], opacities [N,1], sh [N,K,3], ranges).

    `obj_rots [A,4]` / `obj_trans [A,3]`: the object-to-world poses of the frame's actors (what
    actor_pose.get_tracking_rotation / get_tracking_translation return, stacked); with requires_grad they receive
    gradients, without (novel-view frames, street_gaussian_model.py:249) the reduction is skipped.  `actor_rows` maps actor
    names to pose rows; by default the actors of `models` whose frame range contains `frame` take rows 0, 1, ... in list
    order (graph_obj_list).  `flip[name]`: bool / uint8 [n] rows mirrored about the local y axis (:263-271, training only);
    `flip_q`: the quaternion of diag(-1,1,-1) (default: DEFAULT_FLIP_Q).  One forward and one backward host call."""
    what = "street_crafter_amd.compose.compose_frame"
    models = list(models)
    plan = plan_frame(models, actor_rows, include=include, frame=frame)
    by_name = {m.name: m for m in models}
    picked = [by_name[s["name"]] for s in plan.segments]
    if not picked:
        raise ValueError(f"{what}: no sub-model to compose")
    K = _check_models(picked)
    A = 0
    if any(m.kind == ACTOR for m in picked):
        for t, w, name in ((obj_rots, 4, "obj_rots"), (obj_trans, 3, "obj_trans")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != w \
                    or not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be a contiguous float32 [A,{w}] tensor")
        A = int(obj_rots.shape[0])
        if obj_trans.shape[0] != A:
            raise ValueError(f"{what}: obj_rots has {A} rows, obj_trans {obj_trans.shape[0]}")
        for s in plan.segments:
            if s["kind"] == ACTOR and not 0 <= s["pose_row"] < A:
                raise ValueError(f"{what}: {s['name']}: pose row {s['pose_row']} outside [0, {A})")
    else:
        obj_rots = obj_trans = None
    dev = picked[0].xyz.device
    tensors = [getattr(m, a) for m in picked for a in _RAW] + ([obj_rots, obj_trans] if A else [])
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{what}: tensors must live on a HIP device (got {t.device}); "
                               "street_crafter_amd has no CPU path")
        if t.device != dev:
            raise ValueError(f"{what}: tensors on different devices ({dev} and {t.device})")
    call = _Call()
    call.N, call.K, call.A, call.n_seg = plan.n, K, A, len(picked)
    call.ranges = [v for s in plan.segments for v in (s["start"], s["end"])]
    call.kinds = [s["kind"] for s in plan.segments]
    call.pose_rows = [max(s["pose_row"], 0) for s in plan.segments]
    call.flips, call.fparams = [], []
    none = torch.empty(0, dtype=torch.uint8, device=dev)
    any_flip = False
    for m in picked:
        f = (flip or {}).get(m.name) if m.kind == ACTOR else None
        if f is not None:
            if f.dtype not in (torch.bool, torch.uint8) or tuple(f.shape) != (m.n,) or not f.is_contiguous() \
                    or f.device != dev:
                raise ValueError(f"{what}: flip[{m.name!r}] must be a contiguous bool / uint8 [{m.n}] tensor on {dev}")
            f = f.view(torch.uint8)
            any_flip = True
        call.flips.append(none if f is None else f)
        basis = [0.0] * 8
        if m.kind == ACTOR and m.features_dc.shape[1] > 1:
            # the reference's time axis (gaussian_model_actor.py:68-71); the basis is scene_io.idft's, bit for bit
            t = m.fourier_scale * (frame - m.start_frame) / (m.end_frame - m.start_frame)
            b = _basis(float(t), m.features_dc.shape[1])
            basis[:len(b)] = b
        else:
            basis[0] = 1.0
        c = [float(v) for v in m.centre] if m.kind == SKY else [0.0, 0.0, 0.0]
        call.fparams += basis + c + [float(m.radius) if m.kind == SKY else 0.0]
    call.flip_q = [float(v) for v in (flip_q if flip_q is not None else DEFAULT_FLIP_Q)] if any_flip else []
    if len(call.flip_q) not in (0, 4):
        raise ValueError(f"{what}: flip_q must have 4 values (wxyz)")
    if plan.n == 0:
        new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        return new(0, 3), new(0, 4), new(0, 3), new(0, 1), new(0, K, 3), plan.ranges
    raws = [getattr(m, a) for m in picked for a in _RAW]
    means, quats, scales, opac, sh = _Compose.apply(call, obj_rots, obj_trans, *raws)
    return means, quats, scales, opac, sh, plan.ranges
