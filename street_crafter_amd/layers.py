"""The novel-view frame's foreground and sky from one rasterizer pass.

`StreetGaussianRenderer.render_novel_view` (street_gaussian/models/street_gaussian_renderer.py:136-163, the body of
`render.py mode novel_view`) runs the whole operator sequence twice per frame when the scene has a sky sub-model: over
every sub-model but the sky, then over the sky Gaussians alone (`render_sky`, :80-93), and composes
`rgb + rgb_sky * (1 - acc)`.  The two passes are two INDEPENDENT blends, so they cannot share one depth-sorted list as
the groups of `groups.py` do -- unless the list keeps them apart.  `isect_tiles` uses `depths` only as its sort key
(order contract: (depth bits, flat id) ascending), so it is handed LAYERED keys: the back rows' depths times 2^64, an exact
power-of-two lift that keeps order and ties inside the back layer and puts every back record behind every front record of
its tile.  Every tile list is then [front records by depth][back records by depth], each part that layer's own list, and
`rasterize_to_pixels_layered` (csrc/raster_layers.hip) blends the two parts into two accumulator sets one after the other,
jumping from wherever the front part terminates to where the back part begins.  Each layer's images are bit-identical to
`rasterize_to_pixels` on that layer's own projection and intersection lists.  Forward only.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .isect import _ISECT_MODE, _isect_tiles_bin, _req, _stream, isect_offset_encode, isect_tiles
from .lazy import LazyTensor as _LazyTensor

__all__ = ["layered_depths", "smallest_lift", "rasterize_to_pixels_layered", "novel_view_frame", "LIFT"]

LIFT = 2.0 ** 64
_F32_MAX = 3.4028234663852886e38
ROUNDING = {"video": 0, "save_image": 1}          # dist.to_uint8_frame's two modes


def _lift_checks(lift: float):
    lift = float(lift)
    m, e = math.frexp(lift)
    if not (lift > 1.0 and m == 0.5 and math.isfinite(lift)):
        raise ValueError(f"lift must be a power of two greater than 1, got {lift!r}")
    return lift


def layered_depths(depths: Tensor, n_front: int, lift: float = LIFT) -> Tensor:
    """The sort key to hand to `isect_tiles` in place of `depths` [C,N]: rows [0, n_front) unchanged, rows
    [n_front, N) (the back layer) multiplied by `lift`, a power of two -- exact, so order and ties inside the back layer
    are kept and `/ lift` gives the input back bit for bit.

    Precondition, for visible Gaussians with depths in [near, far]: `near * lift > far` (every back key is greater than
    every front key) and `far * lift` finite in float32.  With the default 2^64 that is `far < near * 2^64` and
    `far < 2^64`: the reference's Camera planes (0.001 / 1000) and `rasterization()`'s defaults (0.01 / 1e10) both
    qualify.  The `isect_ids` that `isect_tiles` returns for such keys carry the LIFTED depth bits in their low 32 bits.
    Any qualifying lift gives the same lists, but not at the same price: see `smallest_lift`."""
    if not isinstance(depths, Tensor):
        raise ValueError(f"depths must be a torch.Tensor, got {type(depths)}")
    if depths.dtype != torch.float32:
        raise ValueError(f"depths must be {torch.float32}, got {depths.dtype}")
    if depths.ndim != 2:
        raise ValueError(f"depths must be [C,N], got {tuple(depths.shape)}")
    n_front = int(n_front)
    if not 0 <= n_front <= depths.shape[1]:
        raise ValueError(f"n_front must be in [0, {depths.shape[1]}], got {n_front}")
    lift = _lift_checks(lift)
    out = depths.detach().clone()
    out[:, n_front:] *= lift
    return out


def _planes_ok(near_plane: float, far_plane: float, lift: float) -> bool:
    near, far = float(near_plane), float(far_plane)
    return 0.0 < near <= far and near * lift > far and far * lift <= _F32_MAX


def smallest_lift(near_plane: float, far_plane: float) -> float:
    """The smallest power of two `lift` with `near_plane * lift > far_plane`: 2^20 for the reference's Camera planes
    (0.001 / 1000), 2^40 for 0.01 / 1e10.  Any lift that meets `layered_depths`' precondition gives the same lists; a
    smaller one leaves a smaller hole in the key range, which `isect_tiles` cuts into equal-width depth bins when a
    tile bucket is too long for one sort."""
    near, far = float(near_plane), float(far_plane)
    if not 0.0 < near <= far or not math.isfinite(far):
        raise ValueError(f"0 < near_plane <= far_plane < inf is required, got {near_plane!r} / {far_plane!r}")
    lift = 2.0 ** max(1, math.ceil(math.log2(far / near)))
    while near * lift <= far:
        lift *= 2.0
    return lift


def _shape_checks(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                  n_front):
    named = (("means2d", means2d, torch.float32), ("conics", conics, torch.float32), ("colors", colors, torch.float32),
             ("opacities", opacities, torch.float32), ("isect_offsets", isect_offsets, torch.int32),
             ("flatten_ids", flatten_ids, torch.int32))
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
    for name, t, want in (("means2d", means2d, (C, N, 2)), ("conics", conics, (C, N, 3)), ("colors", colors, (C, N, D))):
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
    if not 0 <= int(n_front) <= N:
        raise ValueError(f"n_front must be in [0, {N}], got {n_front}")
    if int(tile_size) != 16:
        raise NotImplementedError(f"tile_size must be 16, got {tile_size}")
    if D not in (3, 4):
        raise NotImplementedError(f"colour channels must be 3 or 4, got {D}")


def _device_checks(means2d, conics, colors, opacities, isect_offsets, flatten_ids):
    """Every tensor on a HIP device; a deferred `flatten_ids` settled, `isect_offsets` without its dispatch list."""
    for name, t in (("means2d", means2d), ("conics", conics), ("colors", colors), ("opacities", opacities),
                    ("isect_offsets", isect_offsets), ("flatten_ids", flatten_ids)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")
    if type(flatten_ids) is _LazyTensor:      # isect_tiles' deferred list: length and contents are settled here (lazy.py)
        flatten_ids = flatten_ids.plain()
    if type(isect_offsets) is not Tensor:
        isect_offsets = isect_offsets.as_subclass(Tensor)
    return isect_offsets, flatten_ids


def rasterize_to_pixels_layered(means2d: Tensor, conics: Tensor, colors: Tensor, opacities: Tensor, image_width: int,
                                image_height: int, tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor,
                                n_front: int, return_layer_begin: bool = False):
    """-> (front_colors [C,H,W,D], front_alphas [C,H,W,1], back_colors [C,H,W,3], back_alphas [C,H,W,1]); with
    `return_layer_begin` also `layer_begin` int32 [C*tiles], the list position each tile took as its back part's start.

    The first six tensors and the sizes are `rasterize_to_pixels`' (no backgrounds, masks or absgrad).  Rows
    [0, n_front) of every camera are the front layer, rows [n_front, N) the back layer; `isect_offsets` / `flatten_ids`
    must come from `isect_tiles` on `layered_depths(depths, n_front)`.  Each layer's images then equal, bit for bit,
    `rasterize_to_pixels` on that layer's own rows through its own projection and intersection (the back layer's first
    three colour channels).  `n_front == N` and `n_front == 0` are valid: the absent layer's images are zero.  On lists
    that are not layered the images are unspecified.
    Forward only: an input that requires grad (with grad enabled) is refused rather than answered with a detached
    result.  A dispatch list carried by `isect_offsets` is ignored."""
    _shape_checks(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                  n_front)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (means2d, conics, colors, opacities)):
        raise NotImplementedError("rasterize_to_pixels_layered is forward only: call it under torch.no_grad() or on "
                                  "detached tensors")
    isect_offsets, flatten_ids = _device_checks(means2d, conics, colors, opacities, isect_offsets, flatten_ids)
    means2d, conics, colors, opacities, isect_offsets, flatten_ids = (
        t.detach().contiguous() for t in (means2d, conics, colors, opacities, isect_offsets, flatten_ids))
    rc, front_colors, front_alphas, back_colors, back_alphas, layer_begin = _lib.binding().rasterize_fwd_layers(
        means2d, conics, colors, opacities, int(n_front), int(image_width), int(image_height), int(tile_size),
        isect_offsets, flatten_ids, 0, 0, bool(return_layer_begin), None, _stream(means2d))
    if rc:
        _lib.check(rc, "sc_rasterize_fwd_layers")
    if return_layer_begin:
        return front_colors, front_alphas, back_colors, back_alphas, layer_begin
    return front_colors, front_alphas, back_colors, back_alphas


def novel_view_frame(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, sh: Tensor, viewmat: Tensor,
                     K: Tensor, width: int, height: int, n_front: int, *, near_plane: float, far_plane: float,
                     sh_degree: int, antialiased: bool = True, output: str = "float", rounding: str = "video",
                     camera_center: Optional[Tensor] = None, out: Optional[Tensor] = None, lift: Optional[float] = None):
    """`render_novel_view`'s frame for one camera from ONE operator sequence over the concatenated scene: rows
    [0, n_front) are every sub-model but the sky, rows [n_front, N) the sky Gaussians (the order of the reference's scene
    graph, street_gaussian_model.py:236-241).  means [N,3], quats [N,4], scales [N,3], opacities [N], sh [N,K,3], viewmat
    [4,4], K [3,3]; `camera_center` [3]: the reference's Camera.camera_center (derived from `viewmat` when None).

    One fused projection + SH kernel, `layered_depths`, one bucketed `isect_tiles`, one layered rasterizer launch whose
    epilogue is the frame's composite `clamp(clamp(rgb) + clamp(rgb_sky) * (1 - acc), 0, 1)`:
      output="float" -> {"rgb": [3,H,W], "acc": [1,H,W], "depth": [1,H,W]}, the values `render_novel_view` returns
      output="u8"    -> uint8 [H,W,3], `dist.to_uint8_frame` of the two-pass frame; `rounding` "video" (truncate) or
                        "save_image" (+0.5); `out`: optional preallocated contiguous uint8 [H,W,3].
    Bit-identical to the two-pass frame.  Raises ValueError unless `near_plane * 2^64 > far_plane` and
    `far_plane * 2^64` is finite in float32 (see `layered_depths`).  `lift`: the power of two the sky's depth keys are
    multiplied by; default `smallest_lift(near_plane, far_plane)`, never more than 2^64.  The frame does not depend on
    it, `isect_tiles`' time on long tile lists does.  Inference only: an input that requires grad (with grad enabled) is
    refused with NotImplementedError."""
    if output not in ("float", "u8"):
        raise ValueError(f"output must be 'float' or 'u8', got {output!r}")
    if rounding not in ROUNDING:
        raise ValueError(f"rounding must be one of {sorted(ROUNDING)}, got {rounding!r}")
    if not _planes_ok(near_plane, far_plane, LIFT):
        raise ValueError(f"near_plane {near_plane!r} / far_plane {far_plane!r} do not keep the layers apart: "
                         "near_plane * 2^64 > far_plane and far_plane * 2^64 finite in float32 are required")
    if out is not None and output != "u8":
        raise ValueError("out goes with output='u8'")
    lift = smallest_lift(near_plane, far_plane) if lift is None else _lift_checks(lift)
    if lift > LIFT or not _planes_ok(near_plane, far_plane, lift):
        raise ValueError(f"lift {lift!r} does not keep the layers apart for near_plane {near_plane!r} / far_plane "
                         f"{far_plane!r}")
    if torch.is_grad_enabled() and any(isinstance(t, Tensor) and t.requires_grad
                                       for t in (means, quats, scales, opacities, sh)):
        raise NotImplementedError("novel_view_frame is forward only: call it under torch.no_grad() or on detached tensors")
    with torch.no_grad():
        means, quats, scales = _req(means, "means"), _req(quats, "quats"), _req(scales, "scales")
        opacities = _req(opacities, "opacities").reshape(-1)
        sh = _req(sh, "sh")
        viewmats = _req(viewmat, "viewmat").reshape(1, 4, 4)
        Ks = _req(K, "K").reshape(1, 3, 3)
        N = means.shape[0]
        width, height, n_front = int(width), int(height), int(n_front)
        if not 0 <= n_front <= N:
            raise ValueError(f"n_front must be in [0, {N}], got {n_front}")
        if opacities.shape[0] != N or sh.ndim != 3 or sh.shape[0] != N:
            raise ValueError(f"opacities must be [N] and sh [N,K,3], got {tuple(opacities.shape)} / {tuple(sh.shape)}")
        if out is not None and (out.shape != (height, width, 3) or out.dtype != torch.uint8 or not out.is_contiguous()
                                or out.device != means.device):
            raise ValueError("out must be a contiguous uint8 [H,W,3] tensor on the scene's device")
        if camera_center is None:
            from .rendering import camera_centers
            centers = camera_centers(viewmats)
        else:
            centers = _req(camera_center, "camera_center").reshape(1, 3)
        st = _stream(means)
        b = _lib.binding()
        rc, radii, means2d, depths, _, conics, opac, cols = b.projection_sh_fwd(
            means, quats, scales, opacities, sh, viewmats, Ks, centers, int(sh_degree), width, height, 0.3,
            float(near_plane), float(far_plane), 0.0, bool(antialiased), False, st)
        if rc:
            _lib.check(rc, "sc_projection_sh_fwd")
        keys = layered_depths(depths, n_front, lift)
        tile_width, tile_height = math.ceil(width / 16.0), math.ceil(height / 16.0)
        res = None
        if _ISECT_MODE["mode"] == "bin":
            res = _isect_tiles_bin(means2d, radii, keys, 1, N, 16, tile_width, tile_height, st, want_ids=False)
        if res is not None:
            _, _, flatten_ids, isect_offsets = res
        else:
            _, isect_ids, flatten_ids = isect_tiles(means2d, radii, keys, 16, tile_width, tile_height, packed=False,
                                                    n_cameras=1)
            isect_offsets = isect_offset_encode(isect_ids, 1, tile_width, tile_height)
        isect_offsets, flatten_ids = _device_checks(means2d, conics, cols, opac, isect_offsets, flatten_ids)
        epilogue = 1 if output == "float" else 2
        rc, o0, o1, o2, _, _ = b.rasterize_fwd_layers(means2d, conics, cols, opac, n_front, width, height, 16,
                                                      isect_offsets, flatten_ids, epilogue, ROUNDING[rounding], False, out,
                                                      st)
        if rc:
            _lib.check(rc, "sc_rasterize_fwd_layers")
        if output == "u8":
            return o0.reshape(height, width, 3)
        return {"rgb": o0[0].permute(2, 0, 1), "acc": o1[..., 0], "depth": o2[..., 0]}
