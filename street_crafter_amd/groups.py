"""The composite image and one image per Gaussian group from one rasterizer pass.

`StreetGaussianRenderer.render_all` (street_gaussian/models/street_gaussian_renderer.py:17-45, the body of
`render.py mode trajectory`) runs the whole operator sequence three times per frame: over all non-sky models, over
`['background']` and over `pc.obj_list`.  The background and the object Gaussians partition the full set, so the three
images are three blends over ONE depth-sorted list: `rasterize_to_pixels_grouped` walks it once (csrc/raster_groups.hip)
and returns the composite plus one image per group, each bit-identical to what `rasterize_to_pixels` gives on that
group's own projection and intersection lists.  Forward only.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import _lib
from .isect import _stream
from .lazy import LazyTensor as _LazyTensor

__all__ = ["rasterize_to_pixels_grouped"]

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
                                  "detached tensors (the backward pass is not implemented)")
    for name, t in (("means2d", means2d), ("conics", conics), ("colors", colors), ("opacities", opacities),
                    ("isect_offsets", isect_offsets), ("flatten_ids", flatten_ids), ("group_ids", group_ids)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")
    if type(flatten_ids) is _LazyTensor:      # isect_tiles' deferred list: length and contents are settled here (lazy.py)
        flatten_ids = flatten_ids.plain()
    if type(isect_offsets) is not Tensor:
        isect_offsets = isect_offsets.as_subclass(Tensor)
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
