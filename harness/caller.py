"""The caller's sequence around the hot path, as a standalone harness.

`render_gaussians` restates what `StreetGaussianRenderer.render_kernel_gsplat` does with the six
operators (street_gaussian/models/street_gaussian_renderer.py:186-302): same five operator
calls in the same order with the same keyword arguments, and the same torch glue in between
(opacity * compensation :235-238, dirs/masks :256-258, clamp_min(colors+0.5) :260, depth as 4th
channel :265-266, depth normalisation / clamp / permute :282-300).  It goes through the
`gsplat.rendering` names, i.e. through the drop-in boundary, so benchmarks and parity tests
exercise exactly what the reference would call.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

from street_crafter_amd.scenes import Camera, Scene


def render_gaussians(scene: Scene, camera: Camera, tile_size: int = 16, use_depth: bool = True,
                     absgrad: bool = True, antialiasing: bool = True, mode: str = "eval",
                     return_intermediates: bool = False, stage_events=None) -> Dict[str, torch.Tensor]:
    """`stage_events`: optional dict; when given, a (start, end) pair of torch.cuda.Event (HIP events
    on the current stream, the stream every kernel is launched on) is appended per operator call."""
    from gsplat.rendering import (fully_fused_projection, isect_offset_encode, isect_tiles,
                                  rasterize_to_pixels, spherical_harmonics)

    def timed(name, fn, *a, **k):
        if stage_events is None:
            return fn(*a, **k)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn(*a, **k)
        e.record()
        stage_events.setdefault(name, []).append((s, e))
        return r

    xyz3 = scene.means
    rgb3 = scene.sh
    width, height = camera.width, camera.height
    w2c = camera.viewmat.to(xyz3)[None]
    K = camera.K.to(xyz3)[None]

    radii, means2d, depths, conics, compensations = timed(
        "projection", fully_fused_projection, xyz3, None, scene.quats, scene.scales, w2c, K, width, height, packed=False,
        near_plane=camera.znear, far_plane=camera.zfar, calc_compensations=antialiasing)
    opacities = scene.opacities[None, :, 0]
    if compensations is not None:
        opacities = opacities * compensations

    tile_width = math.ceil(width / float(tile_size))
    tile_height = math.ceil(height / float(tile_size))
    tiles_per_gauss, isect_ids, flatten_ids = timed(
        "isect_tiles", isect_tiles, means2d, radii, depths, tile_size, tile_width, tile_height, packed=False, n_cameras=1)
    isect_offsets = timed("isect_offset_encode", isect_offset_encode, isect_ids, 1, tile_width, tile_height)

    dirs = xyz3[None, :, :] - camera.camera_center.to(xyz3)
    masks = radii > 0
    shs = rgb3.expand(1, -1, -1, -1)
    colors = timed("spherical_harmonics", spherical_harmonics, scene.sh_degree, dirs, shs, masks=masks)
    colors = torch.clamp_min(colors + 0.5, 0.0)

    if mode == "train" and means2d.requires_grad:
        means2d.retain_grad()

    if use_depth:
        colors = torch.cat((colors, depths[..., None]), dim=-1)
    if stage_events is not None and hasattr(flatten_ids, "plain"):
        # (probe frames only: the deferred list is settled -- the host's wait for the frame's counts -- BEFORE the rasterizer's
        #  start event, so that the bracket holds the kernel, not the GPU idling while the host waits; the operator would do
        #  the same settle as its first step)
        flatten_ids = flatten_ids.plain()
    render_colors, render_alphas = timed(
        "rasterize_to_pixels", rasterize_to_pixels, means2d, conics, colors, opacities, width, height, tile_size, isect_offsets, flatten_ids,
        backgrounds=None, packed=False, absgrad=absgrad)

    if use_depth:
        rendered_color = render_colors[..., :-1]
        rendered_depth = render_colors[..., -1:] / render_alphas.clamp(min=1e-10)
    else:
        rendered_color = render_colors
        rendered_depth = render_alphas
    rendered_acc = render_alphas
    if mode != "train":
        rendered_color = torch.clamp(rendered_color, 0.0, 1.0)

    result = {
        "rgb": rendered_color[0].permute(2, 0, 1),
        "acc": rendered_acc[..., 0],
        "depth": rendered_depth[..., 0],
        "viewspace_points": means2d,
        "visibility_filter": radii[0] > 0,
        "radii": radii[0] / float(max(height, width)),
    }
    if return_intermediates:
        result.update(dict(_radii=radii, _means2d=means2d, _depths=depths, _conics=conics,
                           _compensations=compensations, _opacities=opacities,
                           _tiles_per_gauss=tiles_per_gauss, _isect_ids=isect_ids,
                           _flatten_ids=flatten_ids, _isect_offsets=isect_offsets, _colors=colors,
                           _render_colors=render_colors, _render_alphas=render_alphas))
    return result


def scene_subset(scene: Scene, mask: torch.Tensor) -> Scene:
    """The Gaussians of `scene` where `mask` (bool [N]) is set, in their original order: what `pc.set_visibility(names)`
    followed by the getters hands the renderer for a subset of the sub-models."""
    mask = mask.to(device=scene.means.device, dtype=torch.bool)
    return Scene(scene.means[mask], scene.quats[mask], scene.scales[mask], scene.opacities[mask], scene.sh[mask],
                 scene.sh_degree)


def _zero_images(camera: Camera, device) -> Dict[str, torch.Tensor]:
    # render_kernel's answer for a model without Gaussians (len(xyz) == 0, white_background False): zeros
    H, W = camera.height, camera.width
    return {"rgb": torch.zeros(3, H, W, device=device), "acc": torch.zeros(1, H, W, device=device),
            "depth": torch.zeros(1, H, W, device=device)}


def _images_of(render_colors, render_alphas, use_depth: bool) -> Dict[str, torch.Tensor]:
    # the eval-mode glue of render_gaussians behind the rasterizer (renderer.py:282-300)
    if use_depth:
        rendered_color = render_colors[..., :-1]
        rendered_depth = render_colors[..., -1:] / render_alphas.clamp(min=1e-10)
    else:
        rendered_color = render_colors
        rendered_depth = render_alphas
    rendered_color = torch.clamp(rendered_color, 0.0, 1.0)
    return {"rgb": rendered_color[0].permute(2, 0, 1), "acc": render_alphas[..., 0], "depth": rendered_depth[..., 0]}


def render_all(scene: Scene, camera: Camera, group_ids: torch.Tensor, grouped: bool = True, tile_size: int = 16,
               use_depth: bool = True, antialiasing: bool = True) -> Dict[str, torch.Tensor]:
    """StreetGaussianRenderer.render_all (street_gaussian_renderer.py:17-45, the body of `render.py mode trajectory`) for
    one camera: the image of all non-sky models, of the background alone and of the objects alone.  `group_ids`: uint8
    [N], 0 = background, 1 = object (how the reference's `pc.graph_gaussian_range` maps onto it: INTEGRATION.md).

    grouped=False spells it as the reference does: three `render_gaussians` calls, over the full scene and over the two
    subsets.  grouped=True runs the operator sequence ONCE over the full scene and ends in
    `rasterize_to_pixels_grouped`; every output is bit-identical to the other spelling's.
    -> rgb, rgb_background, rgb_object [3,H,W]; acc, depth, acc_background, acc_object [1,H,W] (eval mode)."""
    def named(full, bkgd, obj):
        return {"rgb": full["rgb"], "acc": full["acc"], "depth": full["depth"],
                "rgb_background": bkgd["rgb"], "acc_background": bkgd["acc"],
                "rgb_object": obj["rgb"], "acc_object": obj["acc"]}

    dev = scene.means.device
    if not grouped:
        def one(sc):
            if sc.n == 0:
                return _zero_images(camera, dev)
            return render_gaussians(sc, camera, tile_size=tile_size, use_depth=use_depth, antialiasing=antialiasing)
        return named(one(scene), one(scene_subset(scene, group_ids == 0)), one(scene_subset(scene, group_ids == 1)))

    if scene.n == 0:
        z = _zero_images(camera, dev)
        return named(z, z, z)
    from gsplat.rendering import fully_fused_projection, isect_offset_encode, isect_tiles, spherical_harmonics
    from street_crafter_amd.groups import rasterize_to_pixels_grouped
    with torch.no_grad():
        xyz3 = scene.means
        width, height = camera.width, camera.height
        w2c = camera.viewmat.to(xyz3)[None]
        K = camera.K.to(xyz3)[None]
        radii, means2d, depths, conics, compensations = fully_fused_projection(
            xyz3, None, scene.quats, scene.scales, w2c, K, width, height, packed=False,
            near_plane=camera.znear, far_plane=camera.zfar, calc_compensations=antialiasing)
        opacities = scene.opacities[None, :, 0]
        if compensations is not None:
            opacities = opacities * compensations
        tile_width = math.ceil(width / float(tile_size))
        tile_height = math.ceil(height / float(tile_size))
        _, isect_ids, flatten_ids = isect_tiles(means2d, radii, depths, tile_size, tile_width, tile_height,
                                                packed=False, n_cameras=1)
        isect_offsets = isect_offset_encode(isect_ids, 1, tile_width, tile_height)
        dirs = xyz3[None, :, :] - camera.camera_center.to(xyz3)
        shs = scene.sh.expand(1, -1, -1, -1)
        colors = spherical_harmonics(scene.sh_degree, dirs, shs, masks=radii > 0)
        colors = torch.clamp_min(colors + 0.5, 0.0)
        if use_depth:
            colors = torch.cat((colors, depths[..., None]), dim=-1)
        render_colors, render_alphas, group_colors, group_alphas = rasterize_to_pixels_grouped(
            means2d, conics, colors, opacities, width, height, tile_size, isect_offsets, flatten_ids,
            group_ids.to(device=dev, dtype=torch.uint8), n_groups=2)
        return named(_images_of(render_colors, render_alphas, use_depth),
                     _images_of(group_colors[0], group_alphas[0], use_depth),
                     _images_of(group_colors[1], group_alphas[1], use_depth))


def render_train_objects(scene: Scene, camera: Camera, object_mask: torch.Tensor, grouped: bool = True,
                         tile_size: int = 16, use_depth: bool = True, antialiasing: bool = True,
                         absgrad: bool = True) -> Dict[str, torch.Tensor]:
    """What one training iteration with the object accumulation loss renders (train.py:154 and :202-208): the composite
    of all non-sky models in train mode, and `acc_object`, the accumulation of the object Gaussians alone, both under
    grad.  `object_mask`: bool [N].

    grouped=False spells it as the reference does: `render` over the full scene, then `render_object` -- the whole
    operator sequence again over the object subset.  grouped=True runs the sequence ONCE and ends in
    `rasterize_to_pixels_grouped_train` with the objects as group 0 and everything else as id 255 (`n_groups=1`); the
    images are bit-identical to the other spelling's, and `viewspace_points.absgrad` is the composite's in both.
    -> rgb [3,H,W], acc, depth, acc_object [1,H,W], viewspace_points, visibility_filter, radii."""
    dev = scene.means.device
    object_mask = object_mask.to(device=dev, dtype=torch.bool)
    if not grouped:
        out = render_gaussians(scene, camera, tile_size=tile_size, use_depth=use_depth, absgrad=absgrad,
                               antialiasing=antialiasing, mode="train")
        obj = scene_subset(scene, object_mask)
        if obj.n == 0:
            out["acc_object"] = _zero_images(camera, dev)["acc"]
        else:
            out["acc_object"] = render_gaussians(obj, camera, tile_size=tile_size, use_depth=use_depth, absgrad=absgrad,
                                                 antialiasing=antialiasing, mode="train")["acc"]
        return out

    from gsplat.rendering import fully_fused_projection, isect_offset_encode, isect_tiles, spherical_harmonics
    from street_crafter_amd.groups import rasterize_to_pixels_grouped_train
    xyz3 = scene.means
    width, height = camera.width, camera.height
    w2c = camera.viewmat.to(xyz3)[None]
    K = camera.K.to(xyz3)[None]
    radii, means2d, depths, conics, compensations = fully_fused_projection(
        xyz3, None, scene.quats, scene.scales, w2c, K, width, height, packed=False,
        near_plane=camera.znear, far_plane=camera.zfar, calc_compensations=antialiasing)
    opacities = scene.opacities[None, :, 0]
    if compensations is not None:
        opacities = opacities * compensations
    tile_width = math.ceil(width / float(tile_size))
    tile_height = math.ceil(height / float(tile_size))
    _, isect_ids, flatten_ids = isect_tiles(means2d, radii, depths, tile_size, tile_width, tile_height,
                                            packed=False, n_cameras=1)
    isect_offsets = isect_offset_encode(isect_ids, 1, tile_width, tile_height)
    dirs = xyz3[None, :, :] - camera.camera_center.to(xyz3)
    shs = scene.sh.expand(1, -1, -1, -1)
    colors = spherical_harmonics(scene.sh_degree, dirs, shs, masks=radii > 0)
    colors = torch.clamp_min(colors + 0.5, 0.0)
    if means2d.requires_grad:
        means2d.retain_grad()
    if use_depth:
        colors = torch.cat((colors, depths[..., None]), dim=-1)
    group_ids = torch.where(object_mask, 0, 255).to(torch.uint8)
    render_colors, render_alphas, _, group_alphas = rasterize_to_pixels_grouped_train(
        means2d, conics, colors, opacities, width, height, tile_size, isect_offsets, flatten_ids, group_ids, n_groups=1,
        absgrad=absgrad)
    if use_depth:
        rendered_color = render_colors[..., :-1]
        rendered_depth = render_colors[..., -1:] / render_alphas.clamp(min=1e-10)
    else:
        rendered_color = render_colors
        rendered_depth = render_alphas
    return {"rgb": rendered_color[0].permute(2, 0, 1), "acc": render_alphas[..., 0], "depth": rendered_depth[..., 0],
            "acc_object": group_alphas[0][..., 0], "viewspace_points": means2d, "visibility_filter": radii[0] > 0,
            "radii": radii[0] / float(max(height, width))}


def algorithmic_bytes(n_gauss: int, n_isects: int, width: int, height: int, tile_size: int = 16,
                      sh_bases: int = 4) -> int:
    """compulsory HBM bytes per forward frame at the operator boundaries,
    B_alg = (72 + 25 + 12*K + 52) N + 88 I + 24 P + 4 T   (= 197 N + ... for K = 4)."""
    tiles = math.ceil(width / tile_size) * math.ceil(height / tile_size)
    per_gauss = 72 + (12 + 12 * sh_bases + 1 + 12) + 52
    return per_gauss * n_gauss + 88 * n_isects + 24 * width * height + 4 * tiles


def render_novel_view(fg_scene: Scene, sky_scene, camera: Camera, **kw) -> Dict[str, torch.Tensor]:
    """StreetGaussianRenderer.render_novel_view (street_gaussian_renderer.py:136-163) as the reference
    spells it: the foreground pass over every sub-model but the sky (`render_kernel`, :148), then -- when
    the scene has a sky sub-model (`pc.include_sky`, 5 of the 7 shipped configs) -- a second pass over the
    sky Gaussians alone (`render_sky`, :80-93) and `rgb = rgb + rgb_sky * (1 - acc)` (:152), clamp (:159).
    Both passes go through the drop-in operators exactly like `render_gaussians`; the composite is the
    reference's torch expression.  `sky_scene=None`: single pass (include_sky False)."""
    result = render_gaussians(fg_scene, camera, **kw)
    if sky_scene is not None:
        result_sky = render_gaussians(sky_scene, camera, **kw)
        result["rgb"] = result["rgb"] + result_sky["rgb"] * (1 - result["acc"])
        result["_sky"] = result_sky
    result["rgb"] = torch.clamp(result["rgb"], 0.0, 1.0)
    return result


@torch.no_grad()
def render_novel_view_u8(fg_scene: Scene, sky_scene, camera: Camera, rounding: str = "video", out=None,
                         fused: bool = True) -> torch.Tensor:
    """The same frame as `to_uint8_frame(render_novel_view(...)["rgb"])`, bit for bit, as the sharded
    novel-view loop produces it: each pass is ONE call of gsplat's `rasterization()` (fused forward,
    SURVEY 8f-2) and composite + clamp + uint8 conversion are ONE kernel (sc_frame_composite_u8) instead
    of seven torch elementwise passes over the frame.  -> uint8 [H,W,3]."""
    from gsplat.rendering import rasterization
    from street_crafter_amd.dist import to_uint8_frame

    def one_pass(sc):
        if not fused:
            o = render_gaussians(sc, camera, return_intermediates=True)
            return o["_render_colors"], o["_render_alphas"]
        rc, ra, _ = rasterization(sc.means, sc.quats, sc.scales, sc.opacities.reshape(-1), sc.sh,
                                  camera.viewmat[None], camera.K[None], camera.width, camera.height,
                                  near_plane=camera.znear, far_plane=camera.zfar, sh_degree=sc.sh_degree,
                                  render_mode="RGB+ED", rasterize_mode="antialiased",
                                  camera_centers_=camera.camera_center[None])
        return rc, ra

    rc, ra = one_pass(fg_scene)
    rgb = rc[0, ..., :3].permute(2, 0, 1)
    if sky_scene is None:
        return to_uint8_frame(rgb, rounding=rounding, out=out)
    rc_s, _ = one_pass(sky_scene)
    return to_uint8_frame(rgb, acc=ra[0, ..., 0], sky_rgb_chw=rc_s[0, ..., :3].permute(2, 0, 1),
                          rounding=rounding, out=out)
