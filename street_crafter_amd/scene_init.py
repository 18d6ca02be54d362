"""Scene initialisation on the GPU: from the LiDAR sweeps to the first trainable Gaussians, without open3d.

What the reference does once per sequence on the host (street_gaussian/pointcloud_processor/base_processor.py:65-131,
`initailize_ply`, then `create_from_pcd` of models/gaussian_model.py:56-80 and models/gaussian_model_actor.py:79-157):

  voxel_down_sample        open3d `voxel_down_sample(voxel_size=0.1)`                          base_processor.py:85
  radius_outlier_mask      open3d `remove_radius_outlier(nb_points=10, radius=0.5)`            base_processor.py:86
  sphere_norm              `get_Sphere_Norm`                                datasets/base_readers.py:79-91, called :92
  lidar_background_cloud   base_processor.py:80-117 as one call
  gaussians_from_points    `create_from_pcd`: RGB2SH, distCUDA2 scales, identity rotations, inverse_sigmoid(0.1)
  actor_cloud              the point selection of GaussianModelActor.create_from_pcd      gaussian_model_actor.py:84-126

The two open3d calls are RESTATED (csrc/point_cloud.hip): open3d's source is not part of the
reference, so parity with open3d itself is unpinned.  The restatement is normative and tests/scene_init_ref.py holds it
in numpy: voxel index floor((p - (min - v/2)) / v) in float64, means summed sequentially in input order; a point is kept
when more than nb_points points (itself included) lie at d^2 < r^2, strictly.  Output order of the down-sampler:
ascending (ix, iy, iz), lexicographic (open3d's is its hash map's).

Kernels are launched through the C ABI (include/street_crafter_amd.h); there is no CPU path for them.  The down-sampler
and the filter each read the cloud's bounds (and the down-sampler the voxel count) back to the host: they wait for the
stream, which is acceptable once per sequence.  Out of scope: the sky point cloud (waymo_processor.py:126-176), parsing
the sweeps' ply files, the per-camera visibility mask.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .scene_io import SubModel


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _device_points(t, what, dtypes, cols=3):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor")
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{what} must be [N,{cols}], got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise ValueError(f"{what} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")
    return t.detach().contiguous()


def _refused(code, what, why):
    if code == _lib.CONSTANTS["SC_EINVAL"]:
        raise ValueError(f"{what}: refused: {why}")
    _lib.check(code, what)


@torch.no_grad()
def voxel_down_sample(xyz: torch.Tensor, colors: torch.Tensor, voxel_size: float, return_info: bool = False):
    """(xyz f64[M,3], colors f64[M,3], counts i32[M]): one row per occupied voxel in ascending (ix, iy, iz) order, the
    float64 mean of its points and colours summed in input order.  xyz, colors: float64 [N,3] on the device.
    return_info: also {"key_bits": (bx, by, bz), "sort_passes", "longest_segment"}."""
    xyz = _device_points(xyz, "xyz", (torch.float64,))
    colors = _device_points(colors, "colors", (torch.float64,))
    if colors.shape[0] != xyz.shape[0] or colors.device != xyz.device:
        raise ValueError(f"colors must match xyz: {tuple(colors.shape)} on {colors.device} vs {tuple(xyz.shape)} on {xyz.device}")
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and np.isfinite(voxel_size)):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    n, dev = int(xyz.shape[0]), xyz.device
    if n >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 points, got {n}")
    lib = _lib.load()
    info = {"key_bits": (0, 0, 0), "sort_passes": 0, "longest_segment": 0}
    if n == 0:
        out = (torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.float64, device=dev),
               torch.empty((0,), dtype=torch.int32, device=dev))
        return out + (info,) if return_info else out
    with torch.cuda.device(dev):
        ws = torch.empty((lib.sc_voxel_downsample_workspace_bytes(n),), dtype=torch.uint8, device=dev)
        m_host, info_host = ctypes.c_int64(0), (ctypes.c_int32 * 4)()
        _refused(lib.sc_voxel_downsample_plan(xyz.data_ptr(), n, voxel_size, ws.data_ptr(), ws.numel(), ctypes.byref(m_host),
                                              info_host, _stream(xyz)),
                 "sc_voxel_downsample_plan", "a coordinate is NaN or infinite, or the voxel key needs more than 63 bits "
                 "(extent / voxel_size too large)")
        m = int(m_host.value)
        points = torch.empty((m, 3), dtype=torch.float64, device=dev)
        cols = torch.empty((m, 3), dtype=torch.float64, device=dev)
        counts = torch.empty((m,), dtype=torch.int32, device=dev)
        _lib.check(lib.sc_voxel_downsample_reduce(xyz.data_ptr(), colors.data_ptr(), n, m, ws.data_ptr(), ws.numel(),
                                                  points.data_ptr(), cols.data_ptr(), counts.data_ptr(), _stream(xyz)),
                   "sc_voxel_downsample_reduce")
    if return_info:
        bits = tuple(int(b) for b in info_host[:3])
        info = {"key_bits": bits, "sort_passes": (sum(bits) + 7) // 8, "longest_segment": int(info_host[3])}
        return points, cols, counts, info
    return points, cols, counts


@torch.no_grad()
def radius_outlier_mask(xyz: torch.Tensor, nb_points: int, radius: float) -> torch.Tensor:
    """bool[M]: True where more than nb_points points of xyz (float64 [M,3], the point itself included) lie at
    d^2 < radius^2.  `xyz[mask]` is what open3d's remove_radius_outlier returns."""
    xyz = _device_points(xyz, "xyz", (torch.float64,))
    nb_points, radius = int(nb_points), float(radius)
    if nb_points < 0:
        raise ValueError(f"nb_points must be >= 0, got {nb_points}")
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    m, dev = int(xyz.shape[0]), xyz.device
    if m >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 points, got {m}")
    keep = torch.empty((m,), dtype=torch.uint8, device=dev)
    if m == 0:
        return keep.to(torch.bool)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = torch.empty((lib.sc_radius_outlier_workspace_bytes(m),), dtype=torch.uint8, device=dev)
        _refused(lib.sc_radius_outlier_mask(xyz.data_ptr(), m, nb_points, radius, keep.data_ptr(), ws.data_ptr(), ws.numel(),
                                            None, _stream(xyz)),
                 "sc_radius_outlier_mask", "a coordinate is NaN or infinite, or extent / radius needs more than 26 bits on "
                 "an axis")
    return keep.view(torch.bool)


def _sphere_from_bounds(lo: np.ndarray, hi: np.ndarray, scale: float):
    """get_Sphere_Norm (datasets/base_readers.py:83-86) on the float32 extremes: the box's midpoint, half its diagonal."""
    half_diagonal = np.linalg.norm(hi - lo) / 2.0
    return (hi + lo) / 2, half_diagonal * scale


@torch.no_grad()
def sphere_norm(xyz_f32: torch.Tensor, scale: float = 1.0) -> Tuple[np.ndarray, float]:
    """(center float32[3], radius): the bounding sphere of get_Sphere_Norm.  Minimum and maximum on the GPU (exact), the
    reference's numpy float32 expressions on the six downloaded values: identical to the reference's result."""
    xyz = _device_points(xyz_f32, "xyz", (torch.float32,))
    n, dev = int(xyz.shape[0]), xyz.device
    if n == 0:
        raise ValueError("sphere_norm of an empty cloud")
    lib = _lib.load()
    bounds = (ctypes.c_float * 6)()
    with torch.cuda.device(dev):
        ws = torch.empty((lib.sc_point_bounds_workspace_bytes(),), dtype=torch.uint8, device=dev)
        _refused(lib.sc_point_bounds_f32(xyz.data_ptr(), n, bounds, ws.data_ptr(), ws.numel(), _stream(xyz)),
                 "sc_point_bounds_f32", "a coordinate is NaN or infinite")
    b = np.array(list(bounds), dtype=np.float32)
    return _sphere_from_bounds(b[:3], b[3:], scale)


@dataclass
class BackgroundCloud:
    """What initailize_ply leaves for the background: points3D_bkgd.ply (xyz, rgb), the sphere, and with COLMAP points
    points3D_bkgd_vis.ply (xyz_vis, rgb_vis: the LiDAR points and the COLMAP points nearer than 2 radius)."""
    xyz: torch.Tensor            # f32 [P,3]
    rgb: torch.Tensor            # f32 [P,3]
    center: np.ndarray           # float32 [3]
    radius: float
    n_voxels: int
    n_kept: int
    xyz_vis: Optional[torch.Tensor] = None
    rgb_vis: Optional[torch.Tensor] = None


@torch.no_grad()
def lidar_background_cloud(xyz: torch.Tensor, colors: torch.Tensor, voxel_size: float = 0.1, nb_points: int = 10,
                           radius: float = 0.5, extra_xyz: Optional[torch.Tensor] = None,
                           extra_rgb: Optional[torch.Tensor] = None, sphere_scale: float = 1.0) -> BackgroundCloud:
    """base_processor.py:80-117: down-sample the concatenated sweeps (float64 xyz / colours on the device), drop the
    stragglers, cast to float32, take the sphere of the LiDAR points, append the optional COLMAP points (`extra_*`,
    colours already in [0, 1]; they are cast to float32, which create_from_pcd does to every point anyway)."""
    if (extra_xyz is None) != (extra_rgb is None):
        raise ValueError("extra_xyz and extra_rgb come together")
    vx, vc, _ = voxel_down_sample(xyz, colors, voxel_size)
    keep = radius_outlier_mask(vx, nb_points, radius)
    pts = vx[keep].to(torch.float32)
    rgb = vc[keep].to(torch.float32)
    if pts.shape[0] == 0:
        raise ValueError("the outlier filter left no point")
    center, rad = sphere_norm(pts, sphere_scale)
    out = BackgroundCloud(pts, rgb, center, rad, int(vx.shape[0]), int(pts.shape[0]))
    if extra_xyz is not None:
        ex = _device_points(extra_xyz, "extra_xyz", (torch.float32, torch.float64))
        er = _device_points(extra_rgb, "extra_rgb", (torch.float32, torch.float64))
        if er.shape[0] != ex.shape[0]:
            raise ValueError("extra_rgb must match extra_xyz")
        c = torch.as_tensor(np.asarray(center), dtype=ex.dtype, device=ex.device)
        near = torch.linalg.norm(ex - c, dim=-1) < 2 * float(rad)
        ex32, er32 = ex.to(torch.float32), er.to(torch.float32)
        out.xyz = torch.cat([pts, ex32.to(pts.device)])
        out.rgb = torch.cat([rgb, er32.to(pts.device)])
        out.xyz_vis = torch.cat([pts, ex32[near].to(pts.device)])
        out.rgb_vis = torch.cat([rgb, er32[near].to(pts.device)])
    return out


def initial_opacity() -> float:
    """inverse_sigmoid(0.1) as the reference computes it, in torch CPU float32 (general_utils.inverse_sigmoid)."""
    x = 0.1 * torch.ones((1, 1), dtype=torch.float)
    return float(torch.log(x / (1 - x))[0, 0])


@torch.no_grad()
def gaussians_from_points(xyz: torch.Tensor, rgb: torch.Tensor, max_sh_degree: int, fourier_dim: int = 1,
                          num_classes: int = 0, name: str = "background", return_max_radii2D: bool = False):
    """create_from_pcd as a scene_io.SubModel on the points' device: xyz float32, features_dc [M, fourier_dim, 3] with
    RGB2SH(rgb) in row 0, features_rest [M, (deg + 1)^2 - 1, 3] zeros, scaling log(sqrt(clamp_min(distCUDA2, 1e-7))) three
    times, rotation (1, 0, 0, 0), opacity inverse_sigmoid(0.1), semantic [M, num_classes] zeros."""
    from .knn import distCUDA2
    xyz = _device_points(xyz, "xyz", (torch.float32, torch.float64)).to(torch.float32)
    rgb = _device_points(rgb, "rgb", (torch.float32, torch.float64)).to(torch.float32)
    if rgb.shape[0] != xyz.shape[0] or rgb.device != xyz.device:
        raise ValueError(f"rgb must match xyz: {tuple(rgb.shape)} on {rgb.device} vs {tuple(xyz.shape)} on {xyz.device}")
    max_sh_degree, fourier_dim, num_classes = int(max_sh_degree), int(fourier_dim), int(num_classes)
    if max_sh_degree < 0 or fourier_dim < 1 or num_classes < 0:
        raise ValueError(f"max_sh_degree >= 0, fourier_dim >= 1, num_classes >= 0; got {max_sh_degree}, {fourier_dim}, {num_classes}")
    m, dev = int(xyz.shape[0]), xyz.device
    n_rest = (max_sh_degree + 1) ** 2 - 1
    lib = _lib.load()
    with torch.cuda.device(dev):
        dist2 = distCUDA2(xyz)
        f32 = dict(dtype=torch.float32, device=dev)
        dc = torch.empty((m, fourier_dim, 3), **f32)
        rest = torch.empty((m, n_rest, 3), **f32)
        scaling = torch.empty((m, 3), **f32)
        rotation = torch.empty((m, 4), **f32)
        opacity = torch.empty((m, 1), **f32)
        semantic = torch.empty((m, num_classes), **f32)
        max_radii = torch.empty((m,), **f32)
        _lib.check(lib.sc_gaussian_init(rgb.data_ptr(), dist2.data_ptr(), m, fourier_dim, n_rest, num_classes,
                                        initial_opacity(), dc.data_ptr(), rest.data_ptr() if n_rest else None,
                                        scaling.data_ptr(), rotation.data_ptr(), opacity.data_ptr(),
                                        semantic.data_ptr() if num_classes else None, max_radii.data_ptr(), _stream(xyz)),
                   "sc_gaussian_init")
    model = SubModel(name=name, xyz=xyz, features_dc=dc, features_rest=rest,
                     scaling=scaling, rotation=rotation, opacity=opacity, semantic=semantic)
    return (model, max_radii) if return_max_radii2D else model


def actor_cloud(xyz: Optional[torch.Tensor], rgb: Optional[torch.Tensor], bbox, flip_axis: int = 1,
                deformable: bool = False, flip_prob: float = 0., generator: Optional[torch.Generator] = None):
    """(xyz f32[P,3], rgb f32[P,3], random_initialization): the points GaussianModelActor.create_from_pcd starts from
    (gaussian_model_actor.py:84-126).  Fewer than 2000 points, or none (xyz None): the 20^3 grid over the box `bbox`
    (its three edge lengths), coloured from `generator`.  A rigid actor (not deformable) with flip_prob > 0: the points
    plus the mirror image, across flip_axis, of the side that holds more of them (a tie: the positive side).  Plain
    torch indexing on the tensors' device, CPU included; no kernel."""
    if xyz is not None:
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError("xyz must be a [N,3] tensor or None")
        if not isinstance(rgb, torch.Tensor) or rgb.shape != xyz.shape:
            raise ValueError("rgb must be a tensor of xyz's shape")
    if flip_axis not in (0, 1, 2):
        raise ValueError(f"flip_axis must be 0, 1 or 2, got {flip_axis}")
    random_initialization = xyz is None or xyz.shape[0] < 2000
    if random_initialization:
        dev = xyz.device if xyz is not None else (bbox.device if isinstance(bbox, torch.Tensor) else torch.device("cpu"))
        box = torch.as_tensor(bbox, dtype=torch.float64).reshape(3).cpu()
        dim = 20
        lin = torch.arange(dim, dtype=torch.float64) * (2.0 / (dim - 1)) + (-1.0)        # np.linspace(-1., 1., 20)
        lin[-1] = 1.0
        gx, gy, gz = torch.meshgrid(lin, lin, lin, indexing="xy")                         # np.meshgrid's default
        pts = torch.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], dim=-1) * (box / 2.)
        gen_dev = generator.device if generator is not None else torch.device("cpu")
        colours = torch.rand(pts.shape, generator=generator, dtype=torch.float32, device=gen_dev)
        return pts.to(torch.float32).to(dev), colours.to(dev), True
    xyz, rgb = xyz.detach(), rgb.detach()
    if not deformable and flip_prob > 0.:
        pos, neg = xyz[:, flip_axis] > 0, xyz[:, flip_axis] < 0
        side = pos if int(pos.sum()) >= int(neg.sum()) else neg
        flipped = xyz[side].clone()
        flipped[:, flip_axis] *= -1
        xyz = torch.cat([xyz, flipped], dim=0)
        rgb = torch.cat([rgb, rgb[side].clone()], dim=0)
    return xyz.to(torch.float32), rgb.to(torch.float32), False
