"""The pixel-wise tail of a training frame on the GPU: what sits between the rasterizer and the losses
(street_gaussian_renderer.py:282-300, :116-132 and ColorCorrection.forward, color_correction.py:135-138), through the HIP
kernels of csrc/frame_tail.hip, with its backward.

    frame_tail(render_colors, render_alphas, sky=None, affine=None, clamp=False) -> FrameTail(rgb, acc, depth)

        rgb   = A[:3, :3] @ (render_colors[..., :3] + sky * (1 - render_alphas)) + A[:3, 3]      [3,H,W] planes
        depth = render_colors[..., 3] / render_alphas.clamp(min=1e-10)                           [1,H,W], None for D == 3
        acc   = render_alphas[..., 0]                                                            the reference's own view

One launch forward; one launch backward plus a one-block finishing stage for the affine's twelve sums, which are
deterministic (no float atomics; include/street_crafter_amd.h has the formulas, their evaluation order and the order of
the sums).  Nothing is read back to the host.  `sky` is read through its strides: the `[..., :3]` view of the sky pass's
4-channel render, a dense [1,H,W,3] image and SkyCubeMap's [3,H,W] `sky_color` have 16-byte paths, anything else is read
element by element; no copy is made.  `acc` is a torch view: the kernel moves no bytes for it, and autograd adds what
flows into it to the tail's own gradient of render_alphas.  The affine itself (ColorCorrection.get_affine_trans: a table
lookup or an MLP) stays on torch.

`clamp=True` is the `cfg.mode != 'train'` form (foreground and sky clamped to [0,1] before the composite, the result after
the colour correction); it is forward only.

fp32 only; no CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib
from . import rendering as _r

__all__ = ["frame_tail", "FrameTail"]


class FrameTail(NamedTuple):
    """rgb [3,H,W] contiguous planes; acc [1,H,W], the view render_alphas[..., 0]; depth [1,H,W] contiguous, or None
    when render_colors has no depth channel."""
    rgb: Tensor
    acc: Tensor
    depth: Optional[Tensor]


def _check(render_colors, render_alphas, sky, affine, clamp):
    """Shapes and dtypes first, then devices.  -> (H, W, render_colors is stored as planes, sky strides (channel, row,
    column), sky is [3,H,W])"""
    what = "frame_tail"
    for name, t in (("render_colors", render_colors), ("render_alphas", render_alphas), ("sky", sky), ("affine", affine)):
        if t is None and name in ("sky", "affine"):
            continue
        if not isinstance(t, Tensor):
            raise ValueError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if render_colors.dim() != 4 or render_colors.shape[0] != 1:
        raise ValueError(f"{what}: render_colors must be [1,H,W,D], got {tuple(render_colors.shape)} "
                         "(batches of cameras are not supported)")
    _, H, W, D = (int(v) for v in render_colors.shape)
    if D not in (3, 4):
        raise NotImplementedError(f"{what}: render_colors must have 3 or 4 channels, got {D}")
    if H == 0 or W == 0:
        raise ValueError(f"{what}: empty render_colors {tuple(render_colors.shape)}")
    if H * W >= 1 << 31:
        raise ValueError(f"{what}: {H}x{W} pixels is too many (at most 2^31 - 1)")
    if tuple(render_alphas.shape) != (1, H, W, 1):
        raise ValueError(f"{what}: render_alphas must be [1,{H},{W},1], got {tuple(render_alphas.shape)}")
    # the rasterizer's output as it comes: interleaved, or (under no_grad, set_planar_output) the view of [1,D,H,W] planes
    colors_planar = not render_colors.is_contiguous()
    if colors_planar and not render_colors.permute(0, 3, 1, 2).is_contiguous():
        raise ValueError(f"{what}: render_colors must be contiguous or the permuted view of contiguous [1,D,H,W] planes "
                         f"(the rasterizer's output as it comes), got strides {tuple(render_colors.stride())}")
    if not render_alphas.is_contiguous():
        raise ValueError(f"{what}: render_alphas must be contiguous (the rasterizer's output as it comes), got strides "
                         f"{tuple(render_alphas.stride())}")
    sky_st, planar = (0, 0, 0), False
    if sky is not None:
        if tuple(sky.shape) == (1, H, W, 3):
            sky_st = (sky.stride(3), sky.stride(1), sky.stride(2))
        elif tuple(sky.shape) == (3, H, W):
            sky_st, planar = tuple(sky.stride()), True
        else:
            raise ValueError(f"{what}: sky must be [1,{H},{W},3] or [3,{H},{W}], got {tuple(sky.shape)}")
    if affine is not None and tuple(affine.shape) != (3, 4):
        raise ValueError(f"{what}: affine must be [3,4], got {tuple(affine.shape)}")
    if not isinstance(clamp, bool):
        raise ValueError(f"{what}: clamp must be a bool, got {clamp!r}")
    tensors = [t for t in (render_colors, render_alphas, sky, affine) if t is not None]
    if clamp and torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: clamp=True is forward only: call it under torch.no_grad() or on detached "
                                  "tensors")
    for name, t in (("render_colors", render_colors), ("render_alphas", render_alphas), ("sky", sky), ("affine", affine)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{what}: {name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU "
                             "path")
    if any(t.device != render_colors.device for t in tensors):
        raise ValueError(f"{what}: inputs live on different devices")
    return H, W, colors_planar, [int(v) for v in sky_st], planar


def _fwd(colors, colors_planar, alphas, sky, sky_st, affine, H, W, clamp):
    rc, rgb, depth = _lib.binding().frame_tail_fwd(colors, colors_planar, alphas, sky, sky_st, affine, H, W, clamp,
                                                   _r._stream(colors))
    if rc:
        _lib.check(rc, "sc_frame_tail_fwd")
    return rgb, depth


class _FrameTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, alphas, sky, affine, meta):
        H, W, colors_planar, sky_st, _planar = meta
        rgb, depth = _fwd(colors, colors_planar, alphas, sky, sky_st, affine, H, W, False)
        ctx.set_materialize_grads(False)
        ctx.meta = meta
        ctx.save_for_backward(colors, alphas, sky, affine)
        return rgb, depth

    @staticmethod
    def backward(ctx, g, h):
        colors, alphas, sky, affine = ctx.saved_tensors
        H, W, colors_planar, sky_st, planar = ctx.meta
        need_c, need_a, need_s, need_A = ctx.needs_input_grad[:4]
        # what an absent upstream gradient leaves identically zero is not computed: None
        need_s = need_s and g is not None
        need_A = need_A and g is not None
        need_a = need_a and ((g is not None and sky is not None) or h is not None)
        if (g is None and h is None) or not (need_c or need_a or need_s or need_A):
            return None, None, None, None, None
        rc, gc, ga, gs, gA = _lib.binding().frame_tail_bwd(
            colors, colors_planar, alphas, sky, sky_st, affine, H, W, None if g is None else g.contiguous(),
            None if h is None else h.contiguous(), need_c, need_a, need_s, planar, need_A, _r._stream(colors))
        if rc:
            _lib.check(rc, "sc_frame_tail_bwd")
        return gc, ga, gs, gA, None


def frame_tail(render_colors: Tensor, render_alphas: Tensor, sky: Optional[Tensor] = None,
               affine: Optional[Tensor] = None, clamp: bool = False) -> FrameTail:
    """render_colors fp32 [1,H,W,D], D in {3, 4}, and render_alphas fp32 [1,H,W,1]: the rasterizer's outputs as they come.
    sky: None, or fp32 [1,H,W,3] (usually `sky_render_colors[..., :3]`) or [3,H,W] (SkyCubeMap's sky_color), any strides.
    affine: None or fp32 [3,4], ColorCorrection.get_affine_trans(camera).  See the module docstring."""
    H, W, colors_planar, sky_st, planar = _check(render_colors, render_alphas, sky, affine, clamp)
    if affine is not None:
        affine = affine.contiguous()                    # (12 numbers; a table row already is)
    acc = render_alphas[..., 0]
    if clamp:
        rgb, depth = _fwd(render_colors.detach(), colors_planar, render_alphas.detach(),
                          None if sky is None else sky.detach(), sky_st, None if affine is None else affine.detach(), H, W,
                          True)
    else:
        rgb, depth = _FrameTail.apply(render_colors, render_alphas, sky, affine, (H, W, colors_planar, sky_st, planar))
    return FrameTail(rgb, acc, depth)
