"""Scene initialisation on the GPU (street_crafter_amd/scene_init.py, csrc/point_cloud.hip) against the restatements of
tests/scene_init_ref.py, which test_scene_init_cpu.py pins on the CPU.

Voxel down-sample: points, colours, counts and order bit-equal to the restatement (the sums are sequential in input
order, so there is one right answer).  Radius filter: the mask equal to brute force with the unfused d^2, strict `<`.
First Gaussians: bit-equal to the reference's torch-CPU float32 expressions, the log-scale within
2^-22 (1 + |s|) of float64 (twice what a 1-ulp sqrt and a 1-ulp log can add: 2^-23 and 2^-23 |s|).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_init_ref as ref  # noqa: E402
from guard_arena import GuardedAlloc, TorchProxy  # noqa: E402

from street_crafter_amd import scene_init  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.asarray(want).dtype and got.shape == np.asarray(want).shape, (got.dtype, got.shape)
    np.testing.assert_array_equal(_bits(got), _bits(np.asarray(want)))


def _check_voxels(xyz, col, v):
    want = ref.voxel_down_sample(xyz, col, v)
    got = scene_init.voxel_down_sample(_dev(xyz), _dev(col), v)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.float64 and got[2].dtype == torch.int32
    np.testing.assert_array_equal(got[2].cpu().numpy(), want[2])
    _same_bits(got[0], want[0])
    _same_bits(got[1], want[1])
    return got, want


# ---- voxel down-sample -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_voxel_means_bit_equal(n):
    _, want = _check_voxels(*ref.voxel_cloud("random", n))
    if n == 4097:
        assert want[2].max() > 8 and len(want[0]) > 256          # shared voxels, more than one block of voxels


def test_voxel_one_crowded_voxel():
    xyz, col, v = ref.voxel_cloud("crowded")
    _, want = _check_voxels(xyz, col, v)
    assert want[2].max() == 5000
    info = scene_init.voxel_down_sample(_dev(xyz), _dev(col), v, return_info=True)[3]
    assert info["longest_segment"] == 5000 and info["sort_passes"] == (sum(info["key_bits"]) + 7) // 8


def test_voxel_every_point_alone():
    got, want = _check_voxels(*ref.voxel_cloud("alone"))
    assert (want[2] == 1).all() and got[0].shape[0] == 605


def test_voxel_dyadic_every_floor_on_its_boundary():
    _check_voxels(*ref.voxel_cloud("dyadic"))


def test_voxel_world_offset_needs_float64():
    xyz, col, v = ref.voxel_cloud("offset")
    moved = (ref.voxel_index(xyz, v) != ref.voxel_index_f32(xyz, v)).any(axis=1)
    assert moved.any()                                            # a float32 kernel puts these points elsewhere
    _check_voxels(xyz, col, v)


def test_voxel_refusals():
    xyz = np.random.default_rng(0).uniform(size=(100, 3))
    col = _dev(xyz)
    wide = xyz * 1e9                                              # 1e9 / 1e-3 = 2^40 per axis: 120 key bits
    with pytest.raises(ValueError, match="63 bits"):
        scene_init.voxel_down_sample(_dev(wide), col, 1e-3)
    for v in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="voxel_size"):
            scene_init.voxel_down_sample(_dev(xyz), col, v)
    bad = xyz.copy()
    bad[37, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        scene_init.voxel_down_sample(_dev(bad), col, 0.1)
    bad[37, 1] = np.inf
    with pytest.raises(ValueError):
        scene_init.voxel_down_sample(_dev(bad), col, 0.1)
    with pytest.raises(ValueError):
        scene_init.radius_outlier_mask(_dev(bad), 10, 0.5)
    with pytest.raises(ValueError, match="26 bits"):
        scene_init.radius_outlier_mask(_dev(wide), 10, 0.5)
    # 21 bits an axis is accepted: the key has exactly 63
    corner = np.array([[0.0, 0.0, 0.0], [2.0 ** 21 - 2.0, 2.0 ** 21 - 2.0, 2.0 ** 21 - 2.0], [5.25, 7.5, 1.0]])
    got, _ = _check_voxels(corner, corner / 2.0 ** 21, 1.0)
    assert got[0].shape[0] == 3
    assert scene_init.voxel_down_sample(_dev(corner), _dev(corner), 1.0, return_info=True)[3]["key_bits"] == (21, 21, 21)


# ---- radius filter -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _radius_case():
    xyz, tags = ref.radius_cloud()
    return xyz, tags, ref.radius_counts(xyz, ref.RADIUS)


def test_radius_mask_equals_brute_force():
    xyz, tags, cnt = _radius_case()
    want = cnt > ref.NB_POINTS
    got = scene_init.radius_outlier_mask(_dev(xyz), ref.NB_POINTS, ref.RADIUS)
    assert got.dtype == torch.bool and got.shape == (len(xyz),)
    got = got.cpu().numpy()
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, {k: int(np.isin(v, wrong).sum()) for k, v in tags.items() if np.isin(v, wrong).any()}
    # the structures decide what they were built to decide
    assert not got[tags["ten"]].any() and got[tags["eleven"]].all()              # exactly 10 / 11 inside, self included
    assert not got[tags["dup10"]].any() and got[tags["dup12"]].all()             # d = 0 counts
    assert not got[tags["star_centre"]].any()                                    # six neighbours at exactly d = r do not
    assert got[tags["dense"]].all() and got[tags["lattice"]].all() and not got[tags["stragglers"]].any()
    assert got[tags["blob"]].any() and not got[tags["blob"]].all()


def test_radius_exact_rim_never_counts():
    sheet, most = ref.lattice_sheet()
    assert not scene_init.radius_outlier_mask(_dev(sheet), most, ref.RADIUS).any()
    assert scene_init.radius_outlier_mask(_dev(sheet), most - 1, ref.RADIUS).any()


def test_radius_single_point_and_small_thresholds():
    one = _dev(np.array([[3.5, -2.0, 7.25]]))
    assert scene_init.radius_outlier_mask(one, 0, 0.5).tolist() == [True]       # the point itself: 1 > 0
    assert scene_init.radius_outlier_mask(one, 1, 0.5).tolist() == [False]


def test_radius_adversarial_pairs_need_the_unfused_distance():
    """Ten copies of the origin and one partner whose unfused d^2 and both fused evaluations fall on different sides of
    r^2 (found and asserted on the CPU): with nb_points = 10 every point is kept exactly when the partner is inside."""
    pairs = ref.adversarial_pairs(ref.RADIUS, want=8)
    assert len(pairs) >= 8
    r2 = ref.RADIUS * ref.RADIUS
    seen = set()
    for dx, dy, dz, inside in pairs:
        assert ((dx * dx + dy * dy) + dz * dz < r2) == inside
        assert all((f < r2) != inside for f in ref.d2_fused_variants(dx, dy, dz))
        xyz = np.concatenate([np.zeros((10, 3)), [[dx, dy, dz]]])
        want = ref.radius_outlier_mask(xyz, 10, ref.RADIUS)
        assert want[:10].all() == inside and want[:10].any() == inside and want[10] == inside
        got = scene_init.radius_outlier_mask(_dev(xyz), 10, ref.RADIUS).cpu().numpy()
        np.testing.assert_array_equal(got, want)
        seen.add(inside)
    print("adversarial pairs: inside / outside by the unfused rule:", sorted(seen))


# ---- first Gaussians ---------------------------------------------------------------------------------------------------------
def _reference_init(xyz32, rgb32, deg, fourier_dim, num_classes, dist2):
    """create_from_pcd's expressions in torch CPU float32 (gaussian_model.py:59-80, gaussian_model_actor.py:128-157)."""
    m = xyz32.shape[0]
    rgb = torch.from_numpy(rgb32)
    dc = torch.zeros(m, 3, fourier_dim)
    dc[:, :3, 0] = (rgb - 0.5) / ref.C0
    x = 0.1 * torch.ones((m, 1), dtype=torch.float)
    rot = torch.zeros(m, 4)
    rot[:, 0] = 1
    d = torch.clamp_min(torch.from_numpy(dist2), 0.0000001)
    return dict(features_dc=dc.transpose(1, 2).contiguous(), features_rest=torch.zeros(m, (deg + 1) ** 2 - 1, 3),
                rotation=rot, opacity=torch.log(x / (1 - x)), semantic=torch.zeros(m, num_classes),
                scaling=torch.log(torch.sqrt(d))[..., None].repeat(1, 3))


def _check_init(model, xyz32, rgb32, deg, fourier_dim, num_classes):
    from simple_knn._C import distCUDA2
    dist2 = distCUDA2(_dev(xyz32, torch.float32)).cpu().numpy()
    want = _reference_init(xyz32, rgb32, deg, fourier_dim, num_classes, dist2)
    _same_bits(model.xyz, xyz32)
    for k in ("features_dc", "features_rest", "rotation", "opacity", "semantic"):
        got = getattr(model, k)
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous(), k
        _same_bits(got, want[k].numpy())
    s64 = ref.init_scaling_f64(dist2)
    got = model.scaling.cpu().numpy()
    assert got.shape == (len(xyz32), 3) and (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    err = np.abs(got[:, 0].astype(np.float64) - s64)
    bar = 2.0 ** -22 * (1.0 + np.abs(s64))
    print("scaling: worst error / bar =", float((err / bar).max()), "worst error", float(err.max()))
    assert (err <= bar).all()
    return dist2, got


@pytest.mark.parametrize("fourier_dim,deg,num_classes", [(1, 3, 0), (5, 1, 3), (1, 0, 0)])
def test_gaussians_from_points(fourier_dim, deg, num_classes):
    rng = np.random.default_rng(fourier_dim)
    xyz = (rng.normal(size=(3001, 3)) * [6.0, 2.0, 0.5]).astype(np.float32)
    xyz[100:104] = xyz[100]                     # four coincident points: dist2 = 0 clamps to log(sqrt(1e-7))
    rgb = rng.uniform(size=(3001, 3)).astype(np.float32)
    rgb[:3] = [[0.0, 0.5, 1.0], [1.0, 0.0, 0.5], [0.25, 0.75, 0.1]]
    model, max_radii = scene_init.gaussians_from_points(_dev(xyz, torch.float32), _dev(rgb, torch.float32), deg, fourier_dim,
                                                        num_classes, name="obj_007", return_max_radii2D=True)
    assert model.name == "obj_007" and model.features_dc.shape == (3001, fourier_dim, 3)
    assert model.features_rest.shape == (3001, (deg + 1) ** 2 - 1, 3) and model.semantic.shape == (3001, num_classes)
    assert max_radii.shape == (3001,) and not max_radii.any()
    dist2, scaling = _check_init(model, xyz, rgb, deg, fourier_dim, num_classes)
    assert (dist2[100:104] == 0).all()
    floor = np.log(np.sqrt(np.float64(np.float32(1e-7))))
    assert (scaling[100:104] == scaling[100, 0]).all() and abs(float(scaling[100, 0]) - floor) <= 2.0 ** -22 * (1 + abs(floor))
    assert float(model.opacity[0, 0]) == scene_init.initial_opacity()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_sweeps_to_a_rendered_frame():
    from gsplat.rendering import rasterization
    from street_crafter_amd import compose
    from street_crafter_amd.scenes import make_camera
    xyz, col = ref.street_cloud()
    want_p, want_c, want_n = ref.voxel_down_sample(xyz, col, 0.1)
    assert 59_000 <= len(xyz) <= 61_000 and len(want_p) <= 20_000
    keep = ref.radius_outlier_mask(want_p, 10, 0.5)
    assert 200 <= (~keep).sum() < len(keep) // 4                  # the stragglers go, the surfaces stay
    want_xyz, want_rgb = want_p[keep].astype(np.float32), want_c[keep].astype(np.float32)
    want_centre, want_radius = ref.sphere_norm(want_xyz, 1.0)

    cloud = scene_init.lidar_background_cloud(_dev(xyz), _dev(col))
    assert cloud.n_voxels == len(want_p) and cloud.n_kept == int(keep.sum())
    _same_bits(cloud.xyz, want_xyz)
    _same_bits(cloud.rgb, want_rgb)
    _same_bits(np.asarray(cloud.center), want_centre)
    assert cloud.radius == want_radius and type(cloud.radius) is type(want_radius)
    # with COLMAP-like extras: all of them in the cloud, the near ones in the visible cloud
    rng = np.random.default_rng(9)
    ex = want_centre.astype(np.float64) + rng.normal(size=(500, 3)) * 2.0 * float(want_radius)
    er = rng.uniform(size=(500, 3))
    near = np.linalg.norm(ex - want_centre, axis=-1) < 2 * want_radius
    assert near.any() and not near.all()
    both = scene_init.lidar_background_cloud(_dev(xyz), _dev(col), extra_xyz=_dev(ex), extra_rgb=_dev(er))
    _same_bits(both.xyz, np.concatenate([want_xyz, ex.astype(np.float32)]))
    _same_bits(both.xyz_vis, np.concatenate([want_xyz, ex[near].astype(np.float32)]))
    _same_bits(both.rgb_vis, np.concatenate([want_rgb, er[near].astype(np.float32)]))

    model = scene_init.gaussians_from_points(cloud.xyz, cloud.rgb, 3)
    _check_init(model, want_xyz, want_rgb, 3, 1, 0)
    means, quats, scales, opacities, sh, _ = compose.compose_frame([compose.FrameModel.wrap(model, compose.STATIC)],
                                                                   None, None, 0)
    # a camera 1.5 m above the ground looking down the street (+x): world x -> camera z, world z -> camera -y
    R = torch.tensor([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    eye = torch.tensor([1195.0, -350.0, 13.5])
    view = torch.eye(4)
    view[:3, :3] = R
    view[:3, 3] = -R @ eye
    cam = make_camera(160, 96, 120.0, 120.0)
    colors, alphas, _ = rasterization(means, quats, scales, opacities[:, 0], sh, view[None].to(DEV), cam.K[None].to(DEV),
                                      160, 96, sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased")
    torch.cuda.synchronize()
    assert colors.shape == (1, 96, 160, 4) and torch.isfinite(colors).all() and float(alphas.max()) > 0.05


# ---- hygiene ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_in_a_row_are_bit_identical():
    xyz, col, v = ref.voxel_cloud("crowded")
    a = scene_init.voxel_down_sample(_dev(xyz), _dev(col), v)
    b = scene_init.voxel_down_sample(_dev(xyz), _dev(col), v)
    for x, y in zip(a, b):
        _same_bits(x, y.cpu().numpy())
    pts, _, _ = _radius_case()
    m1 = scene_init.radius_outlier_mask(_dev(pts), ref.NB_POINTS, ref.RADIUS)
    m2 = scene_init.radius_outlier_mask(_dev(pts), ref.NB_POINTS, ref.RADIUS)
    assert torch.equal(m1, m2)


def test_outputs_and_workspaces_stay_inside_their_buffers(monkeypatch):
    """Every tensor scene_init allocates for one down-sample and one filter call -- outputs and workspaces -- comes from
    tests/guard_arena.py's GuardedAlloc: no byte next to any of them changes, and the results are the plain ones."""
    xyz, col, v = ref.voxel_cloud("random", 4097)
    pts, _, cnt = _radius_case()
    d_xyz, d_col, d_pts = _dev(xyz), _dev(col), _dev(pts)
    alloc = GuardedAlloc()
    monkeypatch.setattr(scene_init, "torch", TorchProxy(alloc))
    got = scene_init.voxel_down_sample(d_xyz, d_col, v)
    mask = scene_init.radius_outlier_mask(d_pts, ref.NB_POINTS, ref.RADIUS)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(alloc.records) == 4 + 2                            # workspace + three outputs; mask + workspace
    assert alloc.broken_guards() == []
    want = ref.voxel_down_sample(xyz, col, v)
    _same_bits(got[0], want[0])
    _same_bits(got[1], want[1])
    np.testing.assert_array_equal(got[2].cpu().numpy(), want[2])
    np.testing.assert_array_equal(mask.cpu().numpy(), cnt > ref.NB_POINTS)
