"""The composite image and one image per Gaussian group from one rasterizer pass.

`StreetGaussianRenderer.render_all` (street_gaussian/models/street_gaussian_renderer.py:17-45, the body of
`render.py mode trajectory`) runs the whole operator sequence three times per frame: over all non-sky models, over
`['background']` and over `pc.obj_list`.  The background and the object Gaussians partition the full set, so the three
images are three blends over ONE depth-sorted list: `rasterize_to_pixels_grouped` walks it once (csrc/raster_groups.hip)
and returns the composite plus one image per group, each bit-identical to what `rasterize_to_pixels` gives on that
group's own projection and intersection lists.  Forward only.

`rasterize_to_pixels_grouped_train` is the same operator with a backward pass (csrc/raster_groups_bwd.hip): the object
accumulation loss of train.py:202-208, which the reference pays a second whole operator sequence for, comes from the
composite's own walk, forward and backward.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import _lib
from .isect import _stream
from .lazy import LazyTensor as _LazyTensor
from .rendering import _AbsgradTarget

__all__ = ["rasterize_to_pixels_grouped", "rasterize_to_pixels_grouped_train"]

MAX_GROUPS = 2


def _shape_checks(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                  group_ids, n_groups):
    named = (("means2d", means2d, torch.float32), ("conics", conics, torch.float32), ("colors", colors, torch.float32),
             ("opacities", opacities, torch.float32), ("isect_offsets", isect_offsets, torch.int32),
             ("flatten_ids", flatten_ids, torch.int32), ("group_ids", group_ids, torch.uint8))
    for name, t, dtype in named:
        if not isinstance(t, Tensor):
            raise ValueError(f"{name} must be a torch.Tensor, got {type(t)}")
        if t.dtype != dtype:                       # (dtype never settles a deferred flatten_ids: lazy.py)
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if opacities.ndim != 2:
        raise ValueError(f"opacities must be [C,N], got {tuple(opacities.shape)}")
    C, N = opacities.shape
    if colors.ndim != 3:
        raise ValueError(f"colors must be [C,N,D], got {tuple(colors.shape)}")
    D = colors.shape[-1]
    for name, t, want in (("means2d", means2d, (C, N, 2)), ("conics", conics, (C, N, 3)), ("colors", colors, (C, N, D)),
                          ("group_ids", group_ids, (N,))):
        if tuple(t.shape) != want:
            raise ValueError(f"{name} must be {list(want)}, got {list(t.shape)}")
    if isect_offsets.ndim != 3 or isect_offsets.shape[0] != C:
        raise ValueError(f"isect_offsets must be [C,tile_height,tile_width], got {list(isect_offsets.shape)}")
    if flatten_ids.ndim != 1:
        raise ValueError("flatten_ids must be one-dimensional")
    if int(image_width) <= 0 or int(image_height) <= 0 or int(tile_size) <= 0:
        raise ValueError("image_width, image_height and tile_size must be positive")
    th, tw = isect_offsets.shape[1], isect_offsets.shape[2]
    if tw * int(tile_size) < int(image_width) or th * int(tile_size) < int(image_height):
        raise ValueError("the tile grid of isect_offsets does not cover the image")
    if int(n_groups) < 1:
        raise ValueError(f"n_groups must be at least 1, got {n_groups}")
    if int(n_groups) > MAX_GROUPS:
        raise NotImplementedError(f"n_groups > {MAX_GROUPS} is not supported, got {n_groups}")
    if int(tile_size) != 16:
        raise NotImplementedError(f"tile_size must be 16, got {tile_size}")
    if D not in (3, 4):
        raise NotImplementedError(f"colour channels must be 3 or 4, got {D}")


def _device_checks(means2d, conics, colors, opacities, isect_offsets, flatten_ids, group_ids):
    """Every tensor on a HIP device; a deferred `flatten_ids` settled, `isect_offsets` without its dispatch list."""
    for name, t in (("means2d", means2d), ("conics", conics), ("colors", colors), ("opacities", opacities),
                    ("isect_offsets", isect_offsets), ("flatten_ids", flatten_ids), ("group_ids", group_ids)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")
    if type(flatten_ids) is _LazyTensor:      # isect_tiles' deferred list: length and contents are settled here (lazy.py)
        flatten_ids = flatten_ids.plain()
    if type(isect_offsets) is not Tensor:
        isect_offsets = isect_offsets.as_subclass(Tensor)
    return isect_offsets, flatten_ids


def rasterize_to_pixels_grouped(means2d: Tensor, conics: Tensor, colors: Tensor, opacities: Tensor, image_width: int,
                                image_height: int, tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor,
                                group_ids: Tensor, n_groups: int = 2, return_extents: bool = False
                                ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (render_colors [C,H,W,D], render_alphas [C,H,W,1], group_colors [n_groups,C,H,W,D],
    group_alphas [n_groups,C,H,W,1]); with `return_extents` also the kernel's `group_end` int32 [C*tiles, n_groups].

    The first six tensors and the sizes are `rasterize_to_pixels`' (no backgrounds, masks or absgrad).  `group_ids`:
    uint8 [N], shared by all cameras; an id >= n_groups is blended into the composite only.  Group k's images equal, bit
    for bit, `rasterize_to_pixels` on the `group_ids == k` subset through its own projection and intersection.
    Forward only: an input that requires grad (with grad enabled) is refused rather than answered with a detached
    result.  A dispatch list carried by `isect_offsets` is ignored."""
    _shape_checks(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                  group_ids, n_groups)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (means2d, conics, colors, opacities)):
        raise NotImplementedError("rasterize_to_pixels_grouped is forward only: call it under torch.no_grad() or on "
                                  "detached tensors (rasterize_to_pixels_grouped_train has the backward pass)")
    isect_offsets, flatten_ids = _device_checks(means2d, conics, colors, opacities, isect_offsets, flatten_ids, group_ids)
    return _forward_only(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets,
                         flatten_ids, group_ids, n_groups, return_extents)


def _forward_only(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                  group_ids, n_groups, return_extents=False):
    means2d, conics, colors, opacities, isect_offsets, flatten_ids, group_ids = (
        t.detach().contiguous() for t in (means2d, conics, colors, opacities, isect_offsets, flatten_ids, group_ids))
    rc, render_colors, render_alphas, group_colors, group_alphas, group_end = _lib.binding().rasterize_fwd_groups(
        means2d, conics, colors, opacities, group_ids, int(n_groups), int(image_width), int(image_height),
        int(tile_size), isect_offsets, flatten_ids, _stream(means2d))
    if rc:
        _lib.check(rc, "sc_rasterize_fwd_groups")
    if return_extents:
        return render_colors, render_alphas, group_colors, group_alphas, group_end
    return render_colors, render_alphas, group_colors, group_alphas


class _RasterizeGrouped(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2d, conics, colors, opacities, group_ids, n_groups, width, height, tile_size, isect_offsets,
                flatten_ids, absgrad, means2d_obj):
        rc, render_colors, render_alphas, group_colors, group_alphas, last_pos = _lib.binding().rasterize_fwd_groups_ids(
            means2d, conics, colors, opacities, group_ids, n_groups, width, height, tile_size, isect_offsets, flatten_ids,
            _stream(means2d))
        if rc:
            _lib.check(rc, "sc_rasterize_fwd_groups_ids")
        ctx.save_for_backward(means2d, conics, colors, opacities, group_ids, isect_offsets, flatten_ids, render_alphas,
                              group_alphas, last_pos)
        ctx.meta = (n_groups, width, height, tile_size, absgrad)
        ctx.means2d_obj = means2d_obj
        ctx.set_materialize_grads(False)      # an output nobody differentiates: None, and a null pointer in the kernel
        return render_colors, render_alphas, group_colors, group_alphas

    @staticmethod
    def backward(ctx, v_render_colors, v_render_alphas, v_group_colors, v_group_alphas):
        (means2d, conics, colors, opacities, group_ids, isect_offsets, flatten_ids, render_alphas, group_alphas,
         last_pos) = ctx.saved_tensors
        n_groups, width, height, tile_size, absgrad = ctx.meta
        upstream = [None if v is None else v.contiguous()
                    for v in (v_render_colors, v_render_alphas, v_group_colors, v_group_alphas)]
        rc, v_means2d, v_conics, v_colors, v_opacities, v_abs = _lib.binding().rasterize_bwd_groups(
            means2d, conics, colors, opacities, group_ids, n_groups, width, height, tile_size, isect_offsets, flatten_ids,
            render_alphas, group_alphas, last_pos, *upstream, absgrad, _stream(means2d))
        if rc:
            _lib.check(rc, "sc_rasterize_bwd_groups")
        if absgrad:
            # gsplat's contract, as rasterize_to_pixels keeps it: the tensor object the CALLER passed gets `.absgrad`
            # (read at street_gaussian/models/street_gaussian_model.py:505-506).  The composite set's terms only.
            ctx.means2d_obj.tensor.absgrad = v_abs
        need = ctx.needs_input_grad
        return (v_means2d if need[0] else None, v_conics if need[1] else None, v_colors if need[2] else None,
                v_opacities if need[3] else None, None, None, None, None, None, None, None, None, None)


def rasterize_to_pixels_grouped_train(means2d: Tensor, conics: Tensor, colors: Tensor, opacities: Tensor,
                                      image_width: int, image_height: int, tile_size: int, isect_offsets: Tensor,
                                      flatten_ids: Tensor, group_ids: Tensor, n_groups: int = 2, absgrad: bool = False
                                      ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """`rasterize_to_pixels_grouped` with a backward pass: the same four images, bit for bit, differentiable in means2d,
    conics, colors and opacities.  The gradient of a Gaussian is the sum of its gradients through the composite and
    through its own group's image (an id >= n_groups: the composite alone), from one replay of the tile lists.

    absgrad=True attaches `.absgrad` [C,N,2] to the `means2d` object passed in, during backward, as `rasterize_to_pixels`
    does.  It holds the COMPOSITE's terms only -- what `rasterize_to_pixels(..., absgrad=True)` on the full set attaches;
    the group images add nothing to it (the reference's object render has a means2d of its own).  `means2d.grad` carries
    the group images' share as well.  An output that nobody differentiates costs the backward nothing.
    Under torch.no_grad(), or when no input requires grad, this IS the forward-only operator."""
    _shape_checks(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                  group_ids, n_groups)
    isect_offsets, flatten_ids = _device_checks(means2d, conics, colors, opacities, isect_offsets, flatten_ids, group_ids)
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in (means2d, conics, colors, opacities))):
        return _forward_only(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets,
                             flatten_ids, group_ids, n_groups)
    return _RasterizeGrouped.apply(means2d.contiguous(), conics.contiguous(), colors.contiguous(), opacities.contiguous(),
                                   group_ids.contiguous(), int(n_groups), int(image_width), int(image_height),
                                   int(tile_size), isect_offsets.detach().contiguous(), flatten_ids.detach().contiguous(),
                                   bool(absgrad), _AbsgradTarget(means2d))
