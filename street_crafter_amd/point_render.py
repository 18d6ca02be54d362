"""LiDAR condition render on the GPU: `diff_point_rasterization.PointRasterizer`'s forward, as called by
data_processor/utils/render_utils.py:83-183, through the HIP kernels of csrc/point_raster.hip.

The contract is `lidar_condition.render_points` (CPU / numpy): `render_points_hip` takes the same arguments and returns
the same [1, H, W, 4] image, on the device.  Data flow, all on the device's current stream:
    sc_point_project  (means2d / depths / radii = max(ceil(r), 1), and one 32-B record per point)
    -> count -> emit -> radix sort (isect._isect_tiles_radix) -> isect_offset_encode
    -> sc_point_rasterize_fwd  (one wave per 16 x 16 tile, front to back, at most max_hit hits per pixel)
The tile binning takes the count / emit / radix-sort route on purpose, never the tile-bucketed one, whatever
rendering.set_isect_mode says: aggregated LiDAR gives dense, depth-clustered super-tiles, the shape the bucketed route's
range tables are not sized for.  No CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import lidar_condition as _lc
from . import rendering as _r

__all__ = ["render_points_hip", "render_condition_frame_hip", "LidarSequence", "render_condition_frame_resident"]
_RESIDENT = ("LidarSequence", "FramePlan", "render_condition_frame_resident")


def __getattr__(name):
    # the resident-sweep route (lidar_sequence.py, which builds on this module) is re-exported from here on first use
    if name in _RESIDENT:
        from . import lidar_sequence
        return getattr(lidar_sequence, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

TILE = 16
# radius modes of sc_point_project (include/street_crafter_amd.h)
RADIUS_CONST, RADIUS_NDC, RADIUS_KNN, RADIUS_ARRAY = 0, 1, 2, 3


def _device(device, *tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor):
            if not t.is_cuda:
                raise RuntimeError(f"inputs must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")
            return t.device
    if device is not None:
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"inputs must live on a HIP device (got {device}); street_crafter_amd has no CPU path")
        return device
    if not torch.cuda.is_available():
        raise RuntimeError("the point render needs a HIP device; street_crafter_amd has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _on(x, dev, name, dtype=torch.float32) -> torch.Tensor:
    """numpy -> device tensor; a torch tensor must already live on a HIP device."""
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError(f"{name} must live on a HIP device (got {x.device}); street_crafter_amd has no CPU path")
        return x.detach().to(device=dev, dtype=dtype)
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(dev)


def _host64(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu()
    return np.asarray(x, dtype=np.float64)


def _bin_and_blend(project, N: int, dev, st, H: int, W: int, max_hit: int, bg: Optional[torch.Tensor], planar: bool,
                   want_depth: bool):
    """Everything behind the projection, for one camera: `project(radii, means2d, depths, records)` launches the
    kernel that fills the four per-point arrays (only called when N > 0), then count -> emit -> radix sort ->
    offsets -> blend.  -> (rgb, alpha, depth | None, radii i32[N]), as _render."""
    lib = _lib.load()
    if N > 0x7fffffff:
        raise ValueError(f"{N} points exceed the int32 point index of the tile lists")
    if planar:
        img = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        alpha = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        strides, a_stride = (1, H * W), 1
    else:
        img = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
        alpha = img[..., 3]
        strides, a_stride = (4, 1), 4
    depth = torch.empty((1, H, W), dtype=torch.float32, device=dev) if want_depth else None
    radii = torch.empty((1, N), dtype=torch.int32, device=dev)
    tw, th = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    n_isects = 0
    if N:
        means2d = torch.empty((1, N, 2), dtype=torch.float32, device=dev)
        depths = torch.empty((1, N), dtype=torch.float32, device=dev)
        records = torch.empty((N, 8), dtype=torch.float32, device=dev)
        project(radii, means2d, depths, records)
        # (count -> emit -> radix sort directly: see the module docstring)
        _, isect_ids, flatten_ids = _r._isect_tiles_radix(means2d, radii, depths, 1, N, TILE, tw, th, True, st)
        n_isects = int(flatten_ids.numel())
    if n_isects == 0:
        # nothing covers a pixel: the background, without a launch of the blend kernel
        if planar:
            img.copy_(bg.view(3, 1, 1).expand(3, H, W)) if bg is not None else img.zero_()
        else:
            img[..., :3] = bg if bg is not None else 0.0
        alpha.zero_()
        if depth is not None:
            depth.zero_()
        return img, alpha, depth, radii[0]
    offsets = _r.isect_offset_encode(isect_ids, 1, tw, th)
    _lib.check(lib.sc_point_rasterize_fwd(_r._p(records), N, int(W), int(H), tw, th, _r._p(offsets), _r._p(flatten_ids),
                                          n_isects, int(max_hit), _r._p(bg), _r._p(img), strides[0], strides[1],
                                          _r._p(alpha), a_stride, _r._p(depth), st), "sc_point_rasterize_fwd")
    return img, alpha, depth, radii[0]


def _render(pts: torch.Tensor, colors: torch.Tensor, opacities: Optional[torch.Tensor], occ: float,
            radius_in: Optional[torch.Tensor], w2c: np.ndarray, fx: float, fy: float, cx: float, cy: float,
            focal_r: float, H: int, W: int, near: float, far: float, radius_mode: int, scale: float,
            knn_scale_down: float, max_hit: int, bg: Optional[torch.Tensor], planar: bool, want_depth: bool):
    """The device pipeline for one camera.  pts [N,3], colors [N,3] (float32, contiguous, on one device).
    -> (rgb, alpha, depth | None, radii i32[N]): interleaved form rgb = [1,H,W,4] (alpha is its channel 3), or planes
    rgb [3,H,W] + alpha [1,H,W]; depth [1,H,W]."""
    lib = _lib.load()
    dev = pts.device
    st = _r._stream(pts)
    N = int(pts.shape[0])

    def project(radii, means2d, depths, records):
        vm = torch.as_tensor(np.ascontiguousarray(w2c, dtype=np.float64)).to(dev)
        _lib.check(lib.sc_point_project(_r._p(pts), _r._p(colors), _r._p(opacities), float(occ), _r._p(radius_in), N,
                                        _r._p(vm), float(fx), float(fy), float(cx), float(cy), float(focal_r), int(W),
                                        int(H), float(near), float(far), int(radius_mode), float(scale),
                                        float(knn_scale_down), _r._p(radii), _r._p(means2d), _r._p(depths),
                                        _r._p(records), st), "sc_point_project")
    return _bin_and_blend(project, N, dev, st, H, W, max_hit, bg, planar, want_depth)


@torch.no_grad()
def render_points_hip(c2w, ixt, points, features, H: int, W: int, occ: float = 1.0, scale: float = 0.035,
                      use_ndc_scale: bool = False, max_hit: int = 10, near: float = 1.0, far: float = 100.0,
                      use_knn_scale: bool = False, knn_scale_down: float = 1.0, knn_dist2=None, bg=None,
                      return_depth: bool = False, device=None):
    """`lidar_condition.render_points` on the GPU: same arguments and meaning; numpy arrays or torch tensors (tensors
    must live on a HIP device; numpy inputs go to `device`, default the current one).
    -> float32 [1, H, W, 4] (rgb over `bg`, default black, + alpha) on the device; with return_depth also the depth
    [1, H, W] = sum over the blended points of T * alpha * z (unnormalised).
    `use_knn_scale` (without `use_ndc_scale`): the world radius comes from simple_knn's distCUDA2 of ALL points,
    computed on the device, or from `knn_dist2` when given."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"image size must be positive, got {H}x{W}")
    if not 0.0 < float(occ) <= 1.0:
        raise ValueError(f"occ must lie in (0, 1], got {occ}")
    if int(max_hit) < 1:
        raise ValueError(f"max_hit must be >= 1, got {max_hit}")
    dev = _device(device, points, features)
    K = _host64(ixt)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    c2w = _host64(c2w)
    w2c = np.linalg.inv(c2w)
    pts_world = None
    if isinstance(points, torch.Tensor):
        pts = _on(points, dev, "points").reshape(-1, 3).contiguous()
    else:
        # host points (float64 in the offline script): moved to the camera centre in float64 before the float32 upload,
        # so that their rounding is relative to the distance from the camera, not from the world origin (tens of metres
        # away); the camera transform follows: w2c @ translate(origin)
        p64 = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        origin = c2w[:3, 3].copy()
        pts = torch.from_numpy((p64 - origin).astype(np.float32)).to(dev)
        w2c = w2c.copy()
        w2c[:3, 3] += w2c[:3, :3] @ origin
        if use_knn_scale and not use_ndc_scale and knn_dist2 is None:
            pts_world = torch.from_numpy(p64.astype(np.float32)).to(dev)   # distCUDA2 of the points as handed in
    feat = _on(features, dev, "features")
    if feat.shape[0] != pts.shape[0] or feat.dim() != 2 or feat.shape[1] < 3:
        raise ValueError(f"features must be [N, >=3] for {pts.shape[0]} points, got {tuple(feat.shape)}")
    colors = feat[:, :3].contiguous()
    bg_t = None
    if bg is not None:
        bg_t = _on(bg, dev, "bg").reshape(-1).contiguous()
        if bg_t.numel() != 3:
            raise ValueError(f"bg must have 3 entries, got {bg_t.numel()}")
    mode, radius_in = RADIUS_CONST, None
    if use_ndc_scale:
        mode = RADIUS_NDC
    elif use_knn_scale and pts.shape[0]:
        mode = RADIUS_KNN
        if knn_dist2 is None:
            from .knn import distCUDA2
            radius_in = distCUDA2(pts if pts_world is None else pts_world)
        else:
            radius_in = _on(knn_dist2, dev, "knn_dist2").reshape(-1).contiguous()
            if radius_in.numel() != pts.shape[0]:
                raise ValueError(f"knn_dist2 has {radius_in.numel()} entries for {pts.shape[0]} points")
    img, _, depth, _ = _render(pts, colors, None, float(occ), radius_in, w2c, fx, fy, cx, cy, fx, H, W, near, far, mode,
                               scale, knn_scale_down, int(max_hit), bg_t, planar=False, want_depth=return_depth)
    return (img, depth) if return_depth else img


def render_condition_frame_hip(ply_dict, track_info_frame, ego_frame_poses, ego_cam_pose: np.ndarray, frame: int,
                               extrinsic: np.ndarray, ixt: np.ndarray, h: int, w: int, delta_frames: int = 10,
                               shift: float = 0.0, lane_shift_sign: float = 1.0, device=None
                               ) -> Tuple[np.ndarray, np.ndarray]:
    """`lidar_condition.render_condition_frame` with the render on the GPU: the frame assembly and the visibility
    filter stay numpy (host plumbing; `render_condition_frame_resident` of lidar_sequence.py does both on the device from
    sweeps uploaded once).  -> (uint8 rgb [h,w,3], uint8 mask [h,w]), `(x * 255).astype(np.uint8)`."""
    cloud = _lc.assemble_frame(ply_dict, track_info_frame, ego_cam_pose, frame, len(ego_frame_poses), delta_frames,
                               shift)
    c2w = _lc.shifted_camera(ego_cam_pose, ego_frame_poses, frame, extrinsic, shift, lane_shift_sign)
    xyz, feat = _lc.filter_visible(cloud[:, :3], cloud[:, 3:], c2w, ixt, h, w)
    r = render_points_hip(c2w, ixt, xyz, feat, h, w, use_ndc_scale=True, scale=0.01, device=device)
    r = r.cpu().numpy()
    return (r[0, ..., :3] * 255).astype(np.uint8), (r[0, ..., 3] * 255).astype(np.uint8)
