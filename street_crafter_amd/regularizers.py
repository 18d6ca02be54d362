"""Regularizers of the training step on the GPU: the trimmed LiDAR depth loss (train.py:211-218), the sky loss
(train.py:194-196) and the object accumulation loss (train.py:204-208), through the HIP kernels of csrc/regularizers.hip,
with their backward.

    lidar_depth_loss(depth, lidar_depth, mask)   the mean of the 95 % smallest |depth - lidar_depth| over the pixels
                                                 where lidar_depth > 0 and mask
    sky_loss(acc, sky_mask)                      where(sky_mask, -log(1 - a), entropy(a)).mean(), a = clamp(acc)
    obj_acc_loss(acc_obj, obj_bound)             where(obj_bound, entropy(a), -log(1 - a)).mean()

Each returns a 0-d fp32 tensor on the device and never reads anything back to the host: the depth loss selects its k
smallest errors with a radix select on the device instead of the reference's boolean index (a nonzero, which makes the
host wait) and sorted topk.  Inputs are read through their strides: the rasterizer's depth view
`render_colors[..., -1:] / alphas` taken as `[..., 0]`, `render_alphas[..., 0]` and sliced masks need no copy.

Ties.  The value does not depend on which of several equal errors at the threshold t (the k-th smallest error) are taken;
the gradient does.  Here every pixel with error < t is selected, then the first k - count(error < t) pixels with
error == t in row-major pixel order.  torch.topk leaves its own choice unspecified.

fp32 only; no CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib
from . import rendering as _r

__all__ = ["lidar_depth_loss", "sky_loss", "obj_acc_loss", "lidar_depth_forward", "DepthTrimForward"]

MODE_SKY, MODE_OBJ = 0, 1


class DepthTrimForward(NamedTuple):
    """What the depth loss's forward computes, as device tensors: value (0-d fp32; NaN when k == 0), threshold t (0-d
    fp32, the k-th smallest error; NaN when k == 0), n (kept pixels), k (int(keep * n)) and count_below (#error < t)."""
    value: Tensor
    threshold: Tensor
    n: Tensor
    k: Tensor
    count_below: Tensor


def _check_tensor(name: str, t, what: str):
    if not isinstance(t, Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")


def _check_map(name: str, t: Tensor, what: str):
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if t.dim() != 3 or t.shape[0] != 1:
        raise ValueError(f"{what}: {name} must be [1,H,W], got {tuple(t.shape)}")
    if t.shape[1] == 0 or t.shape[2] == 0:
        raise ValueError(f"{what}: empty {name} {tuple(t.shape)}")


def _check_mask(name: str, m: Tensor, H: int, W: int, what: str, one_channel: bool):
    if m.dtype != torch.bool:
        raise ValueError(f"{what}: {name} must be a bool tensor, got {m.dtype}")
    if m.dim() != 3 or tuple(m.shape[1:]) != (H, W) or m.shape[0] < 1 or (one_channel and m.shape[0] != 1):
        want = "[1,H,W]" if one_channel else "[Cm,H,W]"
        raise ValueError(f"{what}: {name} of shape {tuple(m.shape)} does not match H, W = {H}, {W} "
                         f"(expected {want})")


def _check_depth(depth, lidar_depth, mask, keep, what):
    for name, t in (("depth", depth), ("lidar_depth", lidar_depth), ("mask", mask)):
        if t is not None:
            _check_tensor(name, t, what)
    _check_map("depth", depth, what)
    _check_map("lidar_depth", lidar_depth, what)
    H, W = depth.shape[1:]
    if tuple(lidar_depth.shape) != (1, H, W):
        raise ValueError(f"{what}: shape mismatch {tuple(depth.shape)} vs {tuple(lidar_depth.shape)}")
    if mask is not None:
        _check_mask("mask", mask, H, W, what, one_channel=True)
    if lidar_depth.device != depth.device or (mask is not None and mask.device != depth.device):
        raise ValueError(f"{what}: inputs live on different devices")
    if isinstance(keep, bool) or not isinstance(keep, (int, float)) or not (0.0 < float(keep) <= 1.0):
        raise ValueError(f"{what}: keep must be a number in (0, 1], got {keep!r}")
    if H * W >= 1 << 31:
        raise ValueError(f"{what}: {H}x{W} pixels is too many (at most 2^31 - 1)")
    st = [depth.stride(1), depth.stride(2), lidar_depth.stride(1), lidar_depth.stride(2)]
    st += [0, 0] if mask is None else [mask.stride(1), mask.stride(2)]
    return int(H), int(W), [int(v) for v in st]


def _check_acc(acc, mask, what):
    _check_tensor("acc", acc, what)
    _check_tensor("mask", mask, what)
    _check_map("acc", acc, what)
    H, W = acc.shape[1:]
    _check_mask("mask", mask, H, W, what, one_channel=False)
    if mask.device != acc.device:
        raise ValueError(f"{what}: inputs live on different devices")
    if H * W >= 1 << 31:
        raise ValueError(f"{what}: {H}x{W} pixels is too many (at most 2^31 - 1)")
    st = [acc.stride(1), acc.stride(2), mask.stride(0), mask.stride(1), mask.stride(2)]
    return int(mask.shape[0]), int(H), int(W), [int(v) for v in st]


# ---- LiDAR depth loss -------------------------------------------------------------------------------------------
def _depth_fwd(depth, lidar, mask, st, H, W, keep):
    """-> (DepthTrimForward, workspace)."""
    rc, value, thr, counts, ws = _lib.binding().depth_trim_fwd(depth, lidar, mask, st, H, W, float(keep),
                                                               _r._stream(depth))
    if rc:
        _lib.check(rc, "sc_depth_trim_fwd")
    return DepthTrimForward(value, thr, counts[0], counts[1], counts[2]), ws


def _depth_bwd(depth, lidar, mask, st, H, W, g, ws, need_d, need_l):
    rc, gd, gl = _lib.binding().depth_trim_bwd(depth, lidar, mask, st, H, W, g, ws, need_d, need_l, _r._stream(depth))
    if rc:
        _lib.check(rc, "sc_depth_trim_bwd")
    return gd, gl


class _LidarDepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, lidar, mask, meta):
        H, W, st, keep = meta
        fw, ws = _depth_fwd(depth, lidar, mask, st, H, W, keep)
        ctx.set_materialize_grads(False)
        ctx.meta, ctx.mask, ctx.ws = meta, mask, ws         # (the selection state lives in the workspace)
        ctx.save_for_backward(depth, lidar)
        return fw.value

    @staticmethod
    def backward(ctx, g):
        need_d, need_l = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g is None or not (need_d or need_l):
            return None, None, None, None
        depth, lidar = ctx.saved_tensors
        H, W, st, _keep = ctx.meta
        gd, gl = _depth_bwd(depth, lidar, ctx.mask, st, H, W, g.reshape(1).contiguous(), ctx.ws, need_d, need_l)
        return gd, gl, None, None


def lidar_depth_forward(depth: Tensor, lidar_depth: Tensor, mask: Optional[Tensor] = None,
                        keep: float = 0.95) -> DepthTrimForward:
    """The depth loss's forward without autograd: (value, threshold, n, k, count_below), all device tensors."""
    H, W, st = _check_depth(depth, lidar_depth, mask, keep, "lidar_depth_forward")
    return _depth_fwd(depth, lidar_depth, mask, st, H, W, keep)[0]


def lidar_depth_loss(depth: Tensor, lidar_depth: Tensor, mask: Optional[Tensor] = None, keep: float = 0.95) -> Tensor:
    """train.py:213-218: depth_mask = logical_and(lidar_depth > 0, mask); e = |depth - lidar_depth| on it;
    topk(e, int(keep * n), largest=False)[0].mean().  depth, lidar_depth fp32 [1,H,W]; mask bool [1,H,W] (None: all
    True).  NaN when int(keep * n) == 0, as the reference's mean of an empty tensor.  See the module docstring for ties."""
    H, W, st = _check_depth(depth, lidar_depth, mask, keep, "lidar_depth_loss")
    return _LidarDepthLoss.apply(depth, lidar_depth, mask, (H, W, st, float(keep)))


# ---- accumulation losses -----------------------------------------------------------------------------------------
def _acc_fwd(acc, mask, st, Cm, H, W, mode):
    rc, value = _lib.binding().acc_reg_fwd(acc, mask, st, Cm, H, W, mode, _r._stream(acc))
    if rc:
        _lib.check(rc, "sc_acc_reg_fwd")
    return value


def _acc_bwd(acc, mask, st, Cm, H, W, mode, g):
    rc, ga = _lib.binding().acc_reg_bwd(acc, mask, st, Cm, H, W, mode, g, _r._stream(acc))
    if rc:
        _lib.check(rc, "sc_acc_reg_bwd")
    return ga


class _AccReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acc, mask, meta):
        Cm, H, W, st, mode = meta
        value = _acc_fwd(acc, mask, st, Cm, H, W, mode)
        ctx.set_materialize_grads(False)
        ctx.meta, ctx.mask = meta, mask
        ctx.save_for_backward(acc)
        return value

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        (acc,) = ctx.saved_tensors
        Cm, H, W, st, mode = ctx.meta
        return _acc_bwd(acc, ctx.mask, st, Cm, H, W, mode, g.reshape(1).contiguous()), None, None


def _acc_apply(acc, mask, mode, what):
    Cm, H, W, st = _check_acc(acc, mask, what)
    return _AccReg.apply(acc, mask, (Cm, H, W, st, mode))


def sky_loss(acc: Tensor, sky_mask: Tensor) -> Tensor:
    """train.py:194-196: a = clamp(acc, 1e-6, 1 - 1e-6); where(sky_mask, -log(1 - a), -(a log a + (1 - a) log(1 - a)))
    .mean().  acc fp32 [1,H,W]; sky_mask bool [Cm,H,W] (the mean runs over Cm*H*W, as torch.where broadcasts).
    lambda_sky_scale stays a scalar multiply at the call site."""
    return _acc_apply(acc, sky_mask, MODE_SKY, "sky_loss")


def obj_acc_loss(acc_obj: Tensor, obj_bound: Tensor) -> Tensor:
    """train.py:205-206: the same expression as sky_loss with the branches swapped: obj_bound True selects the entropy
    term -(a log a + (1 - a) log(1 - a)), False selects -log(1 - a)."""
    return _acc_apply(acc_obj, obj_bound, MODE_OBJ, "obj_acc_loss")

