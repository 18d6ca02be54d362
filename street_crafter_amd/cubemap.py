"""The sky cube map on the GPU: seamless bilinear sampling of a cube texture through the HIP kernel of csrc/cubemap.hip,
with its backward.  What the reference asks of `nvdiffrast.torch.texture(..., boundary_mode='cube')`
(street_gaussian/models/sky_cubemap.py:102,120,205) and the body of `SkyCubeMap.forward` (sky_cubemap.py:92-127).

    texture_cube(tex, dirs, activation=None)     tex [6,R,R,C] or [1,6,R,R,C], dirs [...,3]  ->  [...,C]
    sky_color(cube_map, K, R, T, H, W, ...)      SkyCubeMap.forward:92-127 in one launch       ->  [3,H,W]

Sampling rule (normative here; parity with nvdiffrast itself is unpinned).  Faces +x -x +y -y +z -z.  The
major axis is z if |z| > max(|x|,|y|), else y if |y| > |x|, else x; face coordinates follow the OpenGL table, the mapping of
the reference's `cube_to_dir` (sky_cubemap.py:166-173).  The texel position is ((s+1)/2 R - 0.5, (t+1)/2 R - 0.5) with s along
the last spatial axis, the taps are floor and floor + 1.  A tap that leaves the face in one axis is the geometrically adjacent
edge texel of the neighbouring face; a tap that leaves it in both (a cube corner) is dropped and the other three weights
are renormalised.  A direction that is all zero or not finite gives zeros and no gradient; directions need not be
normalised.  Gradients flow into the texture only, by fp32 atomic adds: their sum order, hence their last bits, may differ
from run to run.

fp32 only; no CPU path: tensors must live on a HIP device.  Nothing here waits for the device.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .isect import _stream

__all__ = ["texture_cube", "sky_color", "ray_matrix"]

FLAG_SIGMOID, FLAG_CLAMP, FLAG_PLANAR = (_lib.CONSTANTS["SC_CUBE_" + k] for k in ("SIGMOID", "CLAMP", "PLANAR"))
MAX_RESOLUTION = 16384


def _check_tensor(name: str, t, what: str, dtype=torch.float32):
    if not isinstance(t, Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be {dtype}, got {t.dtype}")


def _check_tex(tex, what: str) -> Tensor:
    """-> the [6,R,R,C] view of a [6,R,R,C] or [1,6,R,R,C] texture."""
    _check_tensor("tex", tex, what)
    if tex.dim() == 5 and tex.shape[0] == 1:
        tex = tex[0]
    if tex.dim() != 4 or tex.shape[0] != 6:
        raise ValueError(f"{what}: tex must be [6,R,R,C] or [1,6,R,R,C], got {tuple(tex.shape)}")
    if tex.shape[1] != tex.shape[2]:
        raise ValueError(f"{what}: cube faces must be square, got {tuple(tex.shape)}")
    if not 2 <= tex.shape[1] <= MAX_RESOLUTION:
        raise ValueError(f"{what}: the face resolution must be in [2, {MAX_RESOLUTION}], got {tex.shape[1]}")
    if not 1 <= tex.shape[3] <= 4:
        raise ValueError(f"{what}: 1 to 4 channels, got {tex.shape[3]}")
    return tex


class _CubeSample(torch.autograd.Function):
    """meta = (dirs, ray_m, perturb, mask, acc, n, width, flags, fill): everything but the texture carries no gradient."""

    @staticmethod
    def forward(ctx, tex, meta):
        dirs, ray_m, perturb, mask, acc, n, width, flags, fill = meta
        R, C = int(tex.shape[1]), int(tex.shape[3])
        rc, out = _lib.binding().cubemap_fwd(tex, dirs, ray_m, perturb, mask, acc, R, C, n, width, flags, fill, _stream(tex))
        if rc:
            _lib.check(rc, "sc_cubemap_fwd")
        ctx.meta = meta
        ctx.save_for_backward(tex)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        (tex,) = ctx.saved_tensors
        dirs, ray_m, perturb, mask, acc, n, width, flags, fill = ctx.meta
        R, C = int(tex.shape[1]), int(tex.shape[3])
        rc, gt = _lib.binding().cubemap_bwd(tex, dirs, ray_m, perturb, mask, acc, R, C, n, width, flags, fill,
                                            g.contiguous(), _stream(tex))
        if rc:
            _lib.check(rc, "sc_cubemap_bwd")
        return gt, None


def texture_cube(tex: Tensor, dirs: Tensor, activation: Optional[str] = None) -> Tensor:
    """Samples tex ([6,R,R,C] or [1,6,R,R,C], fp32) along dirs ([...,3], fp32) -> [...,C].  activation None or "sigmoid":
    the sigmoid is applied to each tap inside the kernel (and its derivative in the backward), so a map of logits is never
    materialised in activated form.  Differentiable in tex only."""
    what = "texture_cube"
    tex4 = _check_tex(tex, what)
    _check_tensor("dirs", dirs, what)
    if dirs.dim() < 1 or dirs.shape[-1] != 3:
        raise ValueError(f"{what}: dirs must be [...,3], got {tuple(dirs.shape)}")
    if dirs.device != tex.device:
        raise ValueError(f"{what}: inputs live on different devices")
    if activation not in (None, "sigmoid"):
        raise ValueError(f"{what}: activation must be None or 'sigmoid', got {activation!r}")
    if dirs.requires_grad:
        raise NotImplementedError(f"{what}: gradients with respect to dirs are not implemented (the reference's rays carry "
                                  "none, sky_cubemap.py:97-99); detach dirs")
    flat = dirs.reshape(-1, 3).contiguous()
    flags = FLAG_SIGMOID if activation == "sigmoid" else 0
    out = _CubeSample.apply(tex4.contiguous(), (flat, None, None, None, None, int(flat.shape[0]), 0, flags, 0.0))
    return out.reshape(*dirs.shape[:-1], tex4.shape[3])


def _host_f64(name: str, v, shape, what: str) -> np.ndarray:
    if isinstance(v, Tensor):
        v = v.detach().cpu()          # (a device tensor makes the host wait here: hand K and R over as host arrays)
    a = np.asarray(v, dtype=np.float64)
    if a.size != int(np.prod(shape)):
        raise ValueError(f"{what}: {name} must be {list(shape)}, got {list(a.shape)}")
    return a.reshape(shape)


def ray_matrix(K, R) -> np.ndarray:
    """M = R^T K^-1 in float64 (K [3,3] intrinsics, R [3,3] world-to-camera rotation): the world direction of pixel
    position (u, v) is M (u, v, 1).  This is get_rays_torch (street_gaussian/utils/graphics_utils.py:200-221) with the
    camera origin, which the reference adds and subtracts again in fp32, cancelled: R^T (K^-1 p - T) + R^T T."""
    K = _host_f64("K", K, (3, 3), "ray_matrix")
    R = _host_f64("R", R, (3, 3), "ray_matrix")
    return R.T @ np.linalg.inv(K)


def sky_color(cube_map: Tensor, K, R, T, H: int, W: int, *, sky_mask: Optional[Tensor] = None,
              acc: Optional[Tensor] = None, perturb: Optional[Tensor] = None, white_background: bool) -> Tensor:
    """SkyCubeMap.forward (sky_cubemap.py:92-127) in one launch -> [3,H,W] fp32, clamped to [0,1].

    cube_map: the stored logits [6,R,R,3]; the sigmoid is applied per tap.  K [3,3], R [3,3] and T [3] are the camera's
    intrinsics and world-to-camera pose, best as host arrays (a device tensor is copied to the host, which waits); T does not
    enter the direction (see ray_matrix) and is accepted for the call site's sake.  The pixel mask is sky_mask (bool [H,W])
    if given, else acc (fp32 [1,H,W], tested as (1 - acc) > 1e-3 in fp32, sky_cubemap.py:88), else every pixel; pixels
    outside it get 1 (white_background) or 0.  perturb: fp32 [H,W,2] sub-pixel offsets (torch.rand, the reference's
    perturb=True) or None for pixel centres.  The gradient flows to cube_map only, and only from pixels inside the mask."""
    what = "sky_color"
    tex = _check_tex(cube_map, what)
    if tex.shape[3] != 3:
        raise ValueError(f"{what}: cube_map must have 3 channels, got {tex.shape[3]}")
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"{what}: empty image {H}x{W}")
    dev = tex.device
    mask = accf = None
    if sky_mask is not None:
        _check_tensor("sky_mask", sky_mask, what, torch.bool)
        if tuple(sky_mask.shape) != (H, W):
            raise ValueError(f"{what}: sky_mask must be [H,W] = [{H},{W}], got {tuple(sky_mask.shape)}")
        mask = sky_mask.contiguous()
    elif acc is not None:
        _check_tensor("acc", acc, what)
        if tuple(acc.shape) != (1, H, W):
            raise ValueError(f"{what}: acc must be [1,H,W] = [1,{H},{W}], got {tuple(acc.shape)}")
        accf = acc.detach().contiguous()
    if perturb is not None:
        _check_tensor("perturb", perturb, what)
        if tuple(perturb.shape) != (H, W, 2):
            raise ValueError(f"{what}: perturb must be [H,W,2] = [{H},{W},2], got {tuple(perturb.shape)}")
        perturb = perturb.detach().contiguous()
    for t in (mask, accf, perturb):
        if t is not None and t.device != dev:
            raise ValueError(f"{what}: inputs live on different devices")
    _host_f64("T", T, (3,), what)
    m = [float(v) for v in ray_matrix(K, R).reshape(9)]
    flags = FLAG_SIGMOID | FLAG_CLAMP | FLAG_PLANAR
    out = _CubeSample.apply(tex.contiguous(), (None, m, perturb, mask, accf, H * W, W, flags, 1.0 if white_background else 0.0))
    return out.view(3, H, W)
