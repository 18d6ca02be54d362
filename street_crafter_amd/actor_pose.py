"""The actor poses of a frame on the GPU: what ActorPose.get_tracking_rotation / get_tracking_translation return for every
visible actor (street_gaussian/models/actor_pose.py:83-144), stacked, in ONE HIP launch forward and one backward
(csrc/actor_pose.hip, sc_actor_poses_fwd / bwd).  They are `obj_rots [A,4]` / `obj_trans [A,3]`, the pose inputs of
compose.compose_frame.

The reference asks per actor: two `assert self.valid_mask[cam, frame_idx, id] == 1` on a device tensor (a host wait each,
more on validation frames), some twenty small launches for the lookup, the opt_trans / opt_rots deltas and the slerp, then
a torch.stack.  Here

    table = TrackTable(camera_tracklets, camera_timestamps)     once: the valid mask and the timestamps stay on the HOST,
                                                                input_trans / input_rots go to the device
    plan  = table.plan(ids, cam, frame_idx, timestamp, is_val=..., is_novel_view=..., opt_track=...)       host only
    obj_rots, obj_trans = actor_poses(table, plan, opt_trans, opt_rots)                                    one launch

and no host wait anywhere, forward or backward: the plan travels by value in the kernel arguments.  `opt_trans
[cams,frames,max_obj,3]` / `opt_rots [cams,frames,max_obj,1]` are the caller's leaf parameters, used in place; their
gradients come back as dense tables (zero outside the frame's rows).  A validation frame between two valid neighbours is
interpolated (translation linearly, rotation by slerp) as the reference does; there is no gradient through such a row
(NotImplementedError: the reference renders validation frames under no_grad only).

Opt-in: nothing else in the package calls it.  fp32 contiguous tensors on a HIP device only; there is no CPU path.
Formulas: include/street_crafter_amd.h.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["TrackTable", "PosePlan", "actor_poses", "DELTA", "INTERP"]

DELTA, INTERP = _lib.CONSTANTS["SC_POSE_DELTA"], _lib.CONSTANTS["SC_POSE_INTERP"]
PoseItem = _lib.STRUCTS["sc_actor_pose_item"]           # one actor of sc_actor_poses_fwd / _bwd's host table


@dataclass
class PosePlan:
    """The host table of one frame: item i is row i of obj_rots / obj_trans."""
    items: "ctypes.Array"           # PoseItem * max(A, 1)
    ids: Tuple[int, ...]
    A: int
    rows: int                       # cams * frames * max_obj of the table it was made from
    delta: bool                     # some item reads opt_trans / opt_rots
    interp: bool                    # some item is interpolated


class TrackTable:
    """The tracklets of a scene as ActorPose.__init__ takes them: `camera_tracklets` numpy [cams, frames, max_obj, 8] =
    x y z qw qx qy qz valid, `camera_timestamps[cam][frame_idx]` indexable.  The valid mask (int, as the reference's
    `.float()[..., -1].int()`) and the timestamps stay on the host; input_trans [cams,frames,max_obj,3] and input_rots
    [cams,frames,max_obj,4] are uploaded once, contiguous fp32."""

    def __init__(self, camera_tracklets, camera_timestamps, device="cuda"):
        t = np.asarray(camera_tracklets)
        if t.ndim != 4 or t.shape[-1] != 8:
            raise ValueError(f"TrackTable: camera_tracklets must be [cams, frames, max_obj, 8], got {t.shape}")
        t = np.ascontiguousarray(t, dtype=np.float32)
        self.cams, self.frames, self.max_obj = (int(v) for v in t.shape[:3])
        self.rows = self.cams * self.frames * self.max_obj
        if self.rows >= 2 ** 31:
            raise ValueError(f"TrackTable: {self.rows} rows do not fit the item table's int32 row index")
        self.valid = t[..., 7].astype(np.int32)
        self.camera_timestamps = camera_timestamps
        self.input_trans = torch.from_numpy(np.ascontiguousarray(t[..., 0:3])).to(device)
        self.input_rots = torch.from_numpy(np.ascontiguousarray(t[..., 3:7])).to(device)

    def row(self, cam: int, frame_idx: int, id: int) -> int:
        return (cam * self.frames + frame_idx) * self.max_obj + id

    def plan(self, ids: Sequence[int], cam: int, frame_idx: int, timestamp: float, *, is_val: bool = False,
             is_novel_view: bool = False, opt_track: bool = True) -> PosePlan:
        """Host only: the rules of actor_pose.py:95-144 for the actors `ids` (indices into max_obj, obj_info[..]['id']) as
        seen by the camera (cam, frame_idx, timestamp).  No device is touched."""
        what = "street_crafter_amd.actor_pose.TrackTable.plan"
        cam, frame_idx = int(cam), int(frame_idx)
        if not (0 <= cam < self.cams and 0 <= frame_idx < self.frames):
            raise ValueError(f"{what}: (cam {cam}, frame {frame_idx}) outside [{self.cams}, {self.frames}]")
        ids = tuple(int(i) for i in ids)
        if len(set(ids)) != len(ids):
            raise ValueError(f"{what}: an actor id is listed twice: {ids}")
        may_interp = bool(opt_track) and bool(is_val) and 0 < frame_idx < self.frames - 1
        flag = DELTA if (opt_track and not is_novel_view) else 0
        items = (PoseItem * max(len(ids), 1))()
        interp = False
        for k, i in enumerate(ids):
            if not 0 <= i < self.max_obj:
                raise ValueError(f"{what}: actor id {i} outside [0, {self.max_obj})")
            if self.valid[cam, frame_idx, i] != 1:
                raise ValueError(f"Invalid object {i} at camera {cam}, frame {frame_idx}")
            it = items[k]
            it.row = it.row_prev = it.row_next = self.row(cam, frame_idx, i)
            it.flags, it.alpha, it.one_minus_alpha = flag, 0.0, 1.0
            if may_interp and self.valid[cam, frame_idx - 1, i] == 1 and self.valid[cam, frame_idx + 1, i] == 1:
                pre = float(self.camera_timestamps[cam][frame_idx - 1])
                nxt = float(self.camera_timestamps[cam][frame_idx + 1])
                if nxt == pre:
                    raise ValueError(f"{what}: frames {frame_idx - 1} and {frame_idx + 1} of camera {cam} carry the same "
                                     f"timestamp {pre}: nothing to interpolate along")
                alpha = (float(timestamp) - pre) / (nxt - pre)
                it.row_prev, it.row_next = self.row(cam, frame_idx - 1, i), self.row(cam, frame_idx + 1, i)
                it.flags = flag | INTERP
                it.alpha, it.one_minus_alpha = alpha, 1.0 - alpha         # (float) of the Python floats
                interp = True
        return PosePlan(items=items, ids=ids, A=len(ids), rows=self.rows, delta=bool(flag) and len(ids) > 0, interp=interp)


def _stream(t):
    from .isect import _stream as raw
    return raw(t)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _forward(table: TrackTable, plan: PosePlan, opt_trans, opt_rots):
    dev = table.input_trans.device
    obj_rots = torch.empty((plan.A, 4), dtype=torch.float32, device=dev)
    obj_trans = torch.empty((plan.A, 3), dtype=torch.float32, device=dev)
    rc = _lib.load().sc_actor_poses_fwd(plan.items, plan.A, plan.rows, table.input_trans.data_ptr(),
                                        table.input_rots.data_ptr(), _p(opt_trans), _p(opt_rots), obj_rots.data_ptr(),
                                        obj_trans.data_ptr(), _stream(obj_rots))
    if rc:
        _lib.check(rc, "sc_actor_poses_fwd")
    return obj_rots, obj_trans


class _ActorPoses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table: TrackTable, plan: PosePlan, opt_trans, opt_rots):
        obj_rots, obj_trans = _forward(table, plan, opt_trans, opt_rots)
        ctx.table, ctx.plan, ctx.trans_shape = table, plan, tuple(opt_trans.shape)
        ctx.save_for_backward(opt_rots)
        ctx.set_materialize_grads(False)
        return obj_rots, obj_trans

    @staticmethod
    def backward(ctx, g_rots, g_trans):
        table, plan = ctx.table, ctx.plan
        opt_rots, = ctx.saved_tensors
        g_rots = None if g_rots is None else g_rots.contiguous()
        g_trans = None if g_trans is None else g_trans.contiguous()
        new = lambda shape: torch.empty(shape, dtype=torch.float32, device=opt_rots.device)
        grad_trans = new(ctx.trans_shape) if ctx.needs_input_grad[2] else None
        grad_rots = new(tuple(opt_rots.shape)) if ctx.needs_input_grad[3] else None
        rc = _lib.load().sc_actor_poses_bwd(plan.items, plan.A, plan.rows, table.input_rots.data_ptr(), opt_rots.data_ptr(),
                                            _p(g_rots), _p(g_trans), _p(grad_trans), _p(grad_rots), _stream(opt_rots))
        if rc:
            _lib.check(rc, "sc_actor_poses_bwd")
        return None, None, grad_trans, grad_rots


def actor_poses(table: TrackTable, plan: PosePlan, opt_trans: Optional[torch.Tensor] = None,
                opt_rots: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (obj_rots [A,4] wxyz, not normalised; obj_trans [A,3]) of the plan's actors, in the plan's order.

    `opt_trans` / `opt_rots`: ActorPose's parameters, required when the plan applies them (opt_track and not a novel view),
    ignored otherwise.  Refused, in this order and before any launch: a plan of another table, a missing / mistyped /
    misshapen / non-contiguous opt_* (ValueError); a gradient asked through an interpolated row (NotImplementedError);
    CPU tensors (RuntimeError).  One forward and one backward host call; nothing waits for the device."""
    what = "street_crafter_amd.actor_pose.actor_poses"
    if plan.rows != table.rows:
        raise ValueError(f"{what}: the plan was made for a table of {plan.rows} rows, this one has {table.rows}")
    shape = (table.cams, table.frames, table.max_obj)
    if plan.delta:
        for t, w, name in ((opt_trans, 3, "opt_trans"), (opt_rots, 1, "opt_rots")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise ValueError(f"{what}: {name} must be a float32 tensor (the plan applies the deltas), got "
                                 f"{getattr(t, 'dtype', type(t).__name__)}")
            if tuple(t.shape) != shape + (w,):
                raise ValueError(f"{what}: {name} must be {shape + (w,)}, got {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous (strides {t.stride()})")
    else:
        opt_trans = opt_rots = None                     # not read: no gradient either
    want_grad = plan.delta and torch.is_grad_enabled() and (opt_trans.requires_grad or opt_rots.requires_grad)
    if want_grad and plan.interp:
        raise NotImplementedError(f"{what}: no gradient through an interpolated (validation) row; call under "
                                  "torch.no_grad(), as the reference renders validation frames")
    dev = table.input_trans.device
    for t in (table.input_trans, table.input_rots, opt_trans, opt_rots):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{what}: tensors must live on a HIP device (got {t.device}); "
                               "street_crafter_amd has no CPU path")
        if t.device != dev:
            raise ValueError(f"{what}: tensors on different devices ({dev} and {t.device})")
    if plan.A == 0:
        return (torch.zeros((0, 4), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.float32, device=dev))
    if want_grad:
        return _ActorPoses.apply(table, plan, opt_trans, opt_rots)
    with torch.no_grad():
        return _forward(table, plan, opt_trans.detach() if opt_trans is not None else None,
                        opt_rots.detach() if opt_rots is not None else None)
