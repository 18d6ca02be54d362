"""Scene initialisation without a GPU: the restatements of tests/scene_init_ref.py are pinned against independent
formulations (a literal dict loop for open3d's VoxelDownSample, scipy's cKDTree for the radius count), the shared test
clouds are shown to hold what test_scene_init_gpu.py relies on, actor_cloud runs on CPU tensors, and the entry points
refuse bad arguments before they touch a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_init_ref as ref  # noqa: E402

from street_crafter_amd import scene_init  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the restatements ------------------------------------------------------------------------------------------------------
def test_voxel_restatement_is_the_dict_accumulate_loop():
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-1.0, 1.0, size=(2000, 3)) * np.array([1.0, 0.6, 0.3]) + np.array([105.0, -40.0, 3.0])
    col = rng.uniform(size=(2000, 3))
    got, want = ref.voxel_down_sample(xyz, col, 0.1), ref.voxel_down_sample_dict(xyz, col, 0.1)
    assert 300 < len(want[0]) < 2000 and want[2].max() >= 4          # voxels are shared: the order of the sums matters
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
    np.testing.assert_array_equal(got[2], want[2])
    assert got[2].dtype == np.int32 and int(got[2].sum()) == 2000
    # the order is lexicographic in (ix, iy, iz): row s is the voxel of the s-th smallest index triple
    keys = np.unique(ref.voxel_index(xyz, 0.1), axis=0)
    assert len(keys) == len(got[0]) and all(tuple(keys[i]) < tuple(keys[i + 1]) for i in range(len(keys) - 1))
    for s in (0, len(keys) // 2, len(keys) - 1):
        members = (ref.voxel_index(xyz, 0.1) == keys[s]).all(axis=1)
        assert got[2][s] == members.sum() and np.allclose(got[0][s], xyz[members].mean(axis=0), rtol=0, atol=1e-12)


def test_voxel_cases_hold_what_the_gpu_test_relies_on():
    xyz, col, v = ref.voxel_cloud("crowded")
    assert ref.voxel_down_sample(xyz, col, v)[2].max() == 5000
    xyz, col, v = ref.voxel_cloud("alone")
    assert (ref.voxel_down_sample(xyz, col, v)[2] == 1).all()
    xyz, col, v = ref.voxel_cloud("dyadic")
    q = (xyz - (xyz.min(axis=0) - 0.5 * v)) / v
    on_boundary = (q == np.floor(q)).all(axis=1)
    assert v == 0.125 and on_boundary.sum() == len(xyz) - 1 and (xyz < 0).all()      # all but the min-bound corner
    assert (xyz == xyz.max(axis=0)).any(axis=1).sum() > 50                            # points on the max faces
    assert ref.voxel_down_sample(xyz, col, v)[2].max() >= 3
    xyz, col, v = ref.voxel_cloud("offset")
    assert (ref.voxel_index(xyz, v) != ref.voxel_index_f32(xyz, v)).any()


def test_radius_restatement_counts_like_ckdtree():
    from scipy.spatial import cKDTree
    xyz = np.random.default_rng(4).uniform(-9.0, -3.0, size=(3000, 3))
    gap = ref.min_relative_gap_to_r2(xyz, ref.RADIUS)
    assert gap > 2.0 ** -30, gap           # no pair near the boundary: `<` and `<=`, fused and unfused all agree here
    want = cKDTree(xyz).query_ball_point(xyz, ref.RADIUS, return_length=True)
    got = ref.radius_counts(xyz, ref.RADIUS)
    np.testing.assert_array_equal(got, want)
    assert (got > ref.NB_POINTS).any() and (got <= ref.NB_POINTS).any() and got.min() >= 1
    np.testing.assert_array_equal(ref.radius_outlier_mask(xyz, ref.NB_POINTS, ref.RADIUS), want > ref.NB_POINTS)


def test_radius_cloud_holds_what_the_gpu_test_relies_on():
    xyz, tags = ref.radius_cloud()
    assert 7500 <= len(xyz) <= 8500
    cnt = ref.radius_counts(xyz, ref.RADIUS)
    assert (cnt[tags["ten"]] == 10).all() and (cnt[tags["eleven"]] == 11).all()
    assert (cnt[tags["dup10"]] == 10).all() and (cnt[tags["dup12"]] == 12).all()
    assert (cnt[tags["star_centre"]] == 10).all()                    # 16 if d = r counted
    assert (cnt[tags["dense"]] == 400).all()
    blob = cnt[tags["blob"]] > ref.NB_POINTS
    assert 0.2 < blob.mean() < 0.8 and (xyz[tags["blob"]] < 0).all()
    assert (cnt[tags["stragglers"]] <= 2).all()
    # d = r exactly occurs in the lattice
    lat = xyz[tags["lattice"]]
    assert (ref.d2_unfused(lat[:1], lat) == ref.RADIUS ** 2).sum() >= 3
    sheet, most = ref.lattice_sheet()
    d2 = ref.d2_unfused(sheet[:, None, :], sheet[None, :, :])
    assert ((d2 <= ref.RADIUS ** 2).sum(axis=1) > most).any() and not ((d2 < ref.RADIUS ** 2).sum(axis=1) > most).any()


def test_adversarial_pairs_separate_fused_from_unfused():
    pairs = ref.adversarial_pairs(ref.RADIUS, want=8)
    assert len(pairs) >= 8
    r2 = ref.RADIUS * ref.RADIUS
    for dx, dy, dz, inside in pairs:
        unfused = (dx * dx + dy * dy) + dz * dz
        assert (unfused < r2) == inside
        assert all((f < r2) != inside for f in ref.d2_fused_variants(dx, dy, dz))


def test_sphere_restatement_and_the_products_expression_agree():
    pts = (np.random.default_rng(1).normal(size=(500, 3)) * [30.0, 8.0, 2.0] + [1200.0, -350.0, 12.0]).astype(np.float32)
    c, r = ref.sphere_norm(pts, 1.25)
    c2, r2 = scene_init._sphere_from_bounds(pts.min(axis=0), pts.max(axis=0), 1.25)
    assert c.dtype == np.float32 and np.array_equal(c, c2) and r == r2
    assert abs(float(r) - 1.25 * 0.5 * float(np.linalg.norm(pts.max(0).astype(np.float64) - pts.min(0)))) < 1e-3


# ---- actor_cloud on CPU tensors ----------------------------------------------------------------------------------------------
def _actor_points(n_pos, n_neg, n_zero=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n_pos + n_neg + n_zero, 3, generator=g, dtype=torch.float64) + 0.1
    xyz[n_pos:n_pos + n_neg, 1] *= -1
    xyz[n_pos + n_neg:, 1] = 0.0
    perm = torch.randperm(len(xyz), generator=g)
    return xyz[perm], torch.rand(len(xyz), 3, generator=g, dtype=torch.float64)[perm]


def test_actor_cloud_mirrors_the_majority_side():
    xyz, rgb = _actor_points(1500, 900, 7)
    out_xyz, out_rgb, random_init = scene_init.actor_cloud(xyz, rgb, torch.tensor([4.0, 2.0, 1.5]), flip_axis=1, flip_prob=0.5)
    side = xyz[:, 1] > 0
    assert not random_init and out_xyz.dtype == torch.float32 and out_xyz.shape == (2407 + 1500, 3)
    want = xyz[side].clone()
    want[:, 1] *= -1
    assert torch.equal(out_xyz[:2407], xyz.float()) and torch.equal(out_xyz[2407:], want.float())
    assert torch.equal(out_rgb[2407:], rgb[side].float())
    # the minority side is never mirrored; the negative side is when it holds more
    xyz, rgb = _actor_points(900, 1500)
    out_xyz, _, _ = scene_init.actor_cloud(xyz, rgb, torch.ones(3), flip_axis=1, flip_prob=0.5)
    assert out_xyz.shape[0] == 2400 + 1500 and (out_xyz[2400:, 1] > 0).all()
    # deformable, or flip_prob == 0: the points as they are
    for kw in (dict(deformable=True, flip_prob=0.5), dict(flip_prob=0.0)):
        o, c, _ = scene_init.actor_cloud(xyz, rgb, torch.ones(3), **kw)
        assert torch.equal(o, xyz.float()) and torch.equal(c, rgb.float())


def test_actor_cloud_tie_goes_to_the_positive_side():
    xyz, rgb = _actor_points(1200, 1200, 3)
    out_xyz, _, _ = scene_init.actor_cloud(xyz, rgb, torch.ones(3), flip_axis=1, flip_prob=1.0)
    assert out_xyz.shape[0] == 2403 + 1200 and (out_xyz[2403:, 1] < 0).all()        # mirrored positives


def test_actor_cloud_grid_below_2000_points():
    bbox = torch.tensor([4.5, 2.0, 1.6])
    xyz, rgb = _actor_points(1000, 999)                    # 1999 points: the grid
    g_xyz, g_rgb, random_init = scene_init.actor_cloud(xyz, rgb, bbox, generator=torch.Generator().manual_seed(3))
    assert random_init and g_xyz.shape == g_rgb.shape == (8000, 3) and g_xyz.dtype == g_rgb.dtype == torch.float32
    lx, ly, lz = np.meshgrid(np.linspace(-1., 1., 20), np.linspace(-1., 1., 20), np.linspace(-1., 1., 20))
    want = np.stack([lx.reshape(-1), ly.reshape(-1), lz.reshape(-1)], axis=-1) * (bbox.numpy().astype(np.float64) / 2.)
    np.testing.assert_array_equal(g_xyz.numpy(), want.astype(np.float32))
    assert torch.equal(g_rgb, torch.rand(8000, 3, generator=torch.Generator().manual_seed(3)))
    assert float(g_rgb.min()) >= 0.0 and float(g_rgb.max()) < 1.0
    none_xyz, _, random_init = scene_init.actor_cloud(None, None, bbox, generator=torch.Generator().manual_seed(3))
    assert random_init and torch.equal(none_xyz, g_xyz)
    xyz, rgb = _actor_points(1000, 1000)                   # 2000 points: the points
    o, _, random_init = scene_init.actor_cloud(xyz, rgb, bbox)
    assert not random_init and torch.equal(o, xyz.float())


# ---- refusals that need no device ----------------------------------------------------------------------------------------------
def test_python_entries_refuse_before_any_launch():
    x64, x32 = torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        scene_init.voxel_down_sample(x64, x64, 0.1)
    with pytest.raises(RuntimeError, match="HIP device"):
        scene_init.radius_outlier_mask(x64, 10, 0.5)
    with pytest.raises(RuntimeError, match="HIP device"):
        scene_init.sphere_norm(x32)
    with pytest.raises(RuntimeError, match="HIP device"):
        scene_init.gaussians_from_points(x32, x32, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        scene_init.lidar_background_cloud(x64, x64)
    with pytest.raises(ValueError, match="float64"):
        scene_init.voxel_down_sample(x32, x32, 0.1)
    with pytest.raises(ValueError, match="float64"):
        scene_init.radius_outlier_mask(x32, 10, 0.5)
    with pytest.raises(ValueError, match="float32"):
        scene_init.sphere_norm(x64)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        scene_init.voxel_down_sample(torch.zeros(8, 4, dtype=torch.float64), x64, 0.1)
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        scene_init.radius_outlier_mask(torch.zeros(24, dtype=torch.float64), 10, 0.5)
    with pytest.raises(TypeError):
        scene_init.voxel_down_sample(np.zeros((8, 3)), x64, 0.1)
    with pytest.raises(ValueError, match="flip_axis"):
        scene_init.actor_cloud(None, None, torch.ones(3), flip_axis=3)
    with pytest.raises(ValueError, match="come together"):
        scene_init.lidar_background_cloud(x64, x64, extra_xyz=x64)
    assert scene_init.initial_opacity() == float(torch.log(torch.tensor(0.1) / (1 - torch.tensor(0.1))))


def test_c_entries_refuse_before_any_launch():
    from street_crafter_amd import build, _lib
    build.build()
    lib = _lib.load()
    m, info = ctypes.c_int64(-7), (ctypes.c_int32 * 4)()
    fake = 4096                              # never dereferenced: every call below is refused on its scalars first
    big = 1 << 31
    assert lib.sc_voxel_downsample_plan(fake, 10, 0.0, fake, 1 << 40, ctypes.byref(m), info, None) == -1      # v <= 0
    assert lib.sc_voxel_downsample_plan(fake, 10, -0.1, fake, 1 << 40, ctypes.byref(m), info, None) == -1
    assert lib.sc_voxel_downsample_plan(fake, 10, float("nan"), fake, 1 << 40, ctypes.byref(m), info, None) == -1
    assert lib.sc_voxel_downsample_plan(fake, 10, float("inf"), fake, 1 << 40, ctypes.byref(m), info, None) == -1
    assert lib.sc_voxel_downsample_plan(fake, big, 0.1, fake, 1 << 40, ctypes.byref(m), info, None) == -1     # N >= 2^31
    assert lib.sc_voxel_downsample_plan(fake, 0, 0.1, fake, 1 << 40, ctypes.byref(m), info, None) == -1
    assert lib.sc_voxel_downsample_plan(None, 10, 0.1, fake, 1 << 40, ctypes.byref(m), info, None) == -1
    assert lib.sc_voxel_downsample_plan(fake, 10, 0.1, fake, 1 << 40, None, info, None) == -1
    assert lib.sc_voxel_downsample_plan(fake, 10, 0.1, fake, 16, ctypes.byref(m), info, None) == -2           # workspace
    assert m.value == -7
    assert lib.sc_voxel_downsample_reduce(fake, fake, 10, 11, fake, 1 << 40, fake, fake, fake, None) == -1    # m > n
    assert lib.sc_voxel_downsample_reduce(fake, fake, 10, 0, fake, 1 << 40, fake, fake, fake, None) == 0
    assert lib.sc_voxel_downsample_reduce(fake, fake, 10, 5, fake, 1 << 40, fake, None, fake, None) == -1
    assert lib.sc_voxel_downsample_reduce(fake, fake, 10, 5, fake, 16, fake, fake, fake, None) == -2
    assert lib.sc_radius_outlier_mask(fake, 10, 10, 0.0, fake, fake, 1 << 40, None, None) == -1
    assert lib.sc_radius_outlier_mask(fake, 10, -1, 0.5, fake, fake, 1 << 40, None, None) == -1
    assert lib.sc_radius_outlier_mask(fake, big, 10, 0.5, fake, fake, 1 << 40, None, None) == -1
    assert lib.sc_radius_outlier_mask(fake, 10, 10, 1e200, fake, fake, 1 << 40, None, None) == -1             # r^2 overflows
    assert lib.sc_radius_outlier_mask(fake, 0, 10, 0.5, None, None, 0, None, None) == 0
    assert lib.sc_radius_outlier_mask(fake, 10, 10, 0.5, fake, fake, 16, None, None) == -2
    assert lib.sc_point_bounds_f32(fake, 0, (ctypes.c_float * 6)(), fake, 1 << 20, None) == -1
    assert lib.sc_point_bounds_f64(fake, 10, (ctypes.c_double * 6)(), fake, 16, None) == -2
    assert lib.sc_gaussian_init(fake, fake, 10, 0, 15, 0, 0.0, fake, fake, fake, fake, fake, None, fake, None) == -1    # F < 1
    assert lib.sc_gaussian_init(fake, fake, 10, 1, 15, 0, 0.0, fake, None, fake, fake, fake, None, fake, None) == -1    # rest null
    assert lib.sc_gaussian_init(fake, fake, 0, 1, 15, 0, 0.0, fake, fake, fake, fake, fake, None, fake, None) == 0
    # the workspace sizes: room for the sort's pairs twice over, and for the filter's cell table and sorted copy as well
    n = 100_000
    assert lib.sc_voxel_downsample_workspace_bytes(n) >= n * 24 + lib.sc_radix_sort_workspace_bytes(n)
    assert lib.sc_radius_outlier_workspace_bytes(n) >= lib.sc_voxel_downsample_workspace_bytes(n) + n * 32
    assert lib.sc_point_bounds_workspace_bytes() > 0 and lib.sc_voxel_downsample_workspace_bytes(0) == 256
