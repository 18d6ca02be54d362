"""Drop-in `diff_point_rasterization` package: `from diff_point_rasterization import PointRasterizationSettings,
PointRasterizer` (data_processor/utils/render_utils.py:129) resolves to the HIP point render of
street_crafter_amd/point_render.py (kernels: csrc/point_raster.hip).

Forward only: the reference renders its LiDAR condition under torch.no_grad and never reads the gradient of the
`means2D` placeholder (render_utils.py:167), so the outputs carry no autograd graph and `means2D` is accepted unused.
Conventions (3DGS row-vector form): p_view = [p, 1] @ viewmatrix, z = p_view.z;
p_clip = [p, 1] @ projmatrix, ndc = xyz / w; pixel = ((ndc + 1) * W - 1) / 2 + 0.5 (3DGS ndc2Pix moved to pixel
centres at +0.5); pixel radius = radius * scale_modifier * fx / z with fx = W / (2 tanfovx); alpha = opacities, each in
(0, 1].  A point is drawn iff znear < z < zfar, the planes read back from projmatrix's depth row.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
from torch import nn

__all__ = ["PointRasterizationSettings", "PointRasterizer"]


class PointRasterizationSettings(NamedTuple):
    """The 13 fields render_utils.py:150-164 fills."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    max_hit: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _host64(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu()
    return np.asarray(x, dtype=np.float64)


def _cuda(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")
    return t


def camera_from_settings(s: PointRasterizationSettings):
    """-> (w2c [4,4], fx, fy, cx, cy, znear, zfar, focal_r) in float64 out of the settings' row-vector matrices.
    projmatrix = viewmatrix @ P with P the perspective of 3DGS getProjectionMatrix (column form: w = z, x and y
    rows (P00, 0, P02, 0) / (0, P11, P12, 0), depth row (0, 0, P22, P23)); anything else is refused."""
    H, W = int(s.image_height), int(s.image_width)
    V = _host64(s.viewmatrix)
    F = _host64(s.projmatrix)
    if V.shape != (4, 4) or F.shape != (4, 4):
        raise ValueError(f"viewmatrix / projmatrix must be [4,4], got {V.shape} / {F.shape}")
    P = (np.linalg.inv(V) @ F).T                          # column form of the projection alone
    tol = 1e-5 * max(1.0, float(np.abs(P).max()))
    off = [P[0, 1], P[0, 3], P[1, 0], P[1, 3], P[2, 0], P[2, 1], P[3, 0], P[3, 1], P[3, 3], P[3, 2] - 1.0]
    if max(abs(v) for v in off) > tol:
        raise NotImplementedError("projmatrix must be viewmatrix @ a pinhole perspective with w = z "
                                  "(3DGS getProjectionMatrix)")
    fx, cx = 0.5 * W * P[0, 0], 0.5 * W * (1.0 + P[0, 2])
    fy, cy = 0.5 * H * P[1, 1], 0.5 * H * (1.0 + P[1, 2])
    znear, zfar = -P[2, 3] / P[2, 2], -P[2, 3] / (P[2, 2] - 1.0)
    focal_r = W / (2.0 * float(s.tanfovx))
    return V.T.copy(), fx, fy, cx, cy, znear, zfar, focal_r


class PointRasterizer(nn.Module):
    def __init__(self, raster_settings: PointRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    @torch.no_grad()
    def forward(self, means3D, means2D=None, colors_precomp=None, opacities=None, radius=None, shs=None):
        """-> (image [3,H,W], depth [1,H,W] = sum of T * alpha * z, alpha [1,H,W], radii i32[N] = ceil(pixel radius), at
        least 1 for a drawn point (a radius of 0 still covers the pixel whose centre the point sits on), 0 for culled
        points)."""
        from street_crafter_amd import point_render as pr
        s = self.raster_settings
        if int(s.sh_degree) != 0 or shs is not None:
            raise NotImplementedError("sh_degree != 0 / shs are not supported: the reference passes colors_precomp")
        if colors_precomp is None:
            raise NotImplementedError("colors_precomp is required (the reference's only form)")
        if opacities is None or radius is None:
            raise ValueError("opacities and radius are required")
        means3D = _cuda(means3D, "means3D")
        dev = means3D.device
        colors = _cuda(colors_precomp, "colors_precomp")
        op = _cuda(opacities, "opacities")
        rad = _cuda(radius, "radius")
        bg = _cuda(s.bg, "bg").detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous() \
            if s.bg is not None else None
        N = means3D.shape[0]
        pts = means3D.detach().to(torch.float32).reshape(N, 3).contiguous()
        colors = colors.detach().to(torch.float32).reshape(N, 3).contiguous()
        op = op.detach().to(torch.float32).reshape(N).contiguous()
        rad = rad.detach().to(torch.float32).reshape(N).contiguous()
        if N and not bool(((op > 0) & (op <= 1)).all()):
            raise ValueError("opacities must lie in (0, 1]")
        if int(s.max_hit) < 1:
            raise ValueError(f"max_hit must be >= 1, got {s.max_hit}")
        if bg is not None and bg.numel() != 3:
            raise ValueError(f"bg must have 3 entries, got {bg.numel()}")
        w2c, fx, fy, cx, cy, znear, zfar, focal_r = camera_from_settings(s)
        H, W = int(s.image_height), int(s.image_width)
        img, alpha, depth, radii = pr._render(pts, colors, op, 1.0, rad, w2c, fx, fy, cx, cy, focal_r, H, W, znear, zfar,
                                              pr.RADIUS_ARRAY, float(s.scale_modifier), 1.0, int(s.max_hit), bg,
                                              planar=True, want_depth=True)
        return img, depth, alpha, radii
