"""GPU checks of the LiDAR point render (csrc/point_raster.hip through street_crafter_amd/point_render.py and the
drop-in diff_point_rasterization) against the contract, `lidar_condition.render_points` (float64 numpy).

Verdict ("decidable pixels"): a pixel is UNDECIDABLE when, for some point in the depth window, |d^2 - r^2| <=
1e-4 max(r^2, 1) there (the disc edge passes through the pixel centre), or two of its covering points among the first
max_hit differ in depth by less than 1e-6 z without being equal (fp32 depth keys may order them either way).  The
GPU image must equal the contract on every decidable pixel, and undecidable pixels must be at most 1e-3 of the frame.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from street_crafter_amd import lidar_condition as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _geometry(c2w, ixt, points, H, W, scale, use_ndc_scale, near, far, knn_r=None):
    """The contract's f64 projection (render_points, step by step) -> kept u, v, z, pixel radius, index."""
    w2c = np.linalg.inv(np.asarray(c2w, np.float64))
    cam = np.asarray(points, np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    z = cam[:, 2]
    keep = (z > near) & (z < far)
    idx = np.nonzero(keep)[0]
    cam, z = cam[keep], z[keep]
    fx, fy, cx, cy = ixt[0, 0], ixt[1, 1], ixt[0, 2], ixt[1, 2]
    u, v = fx * cam[:, 0] / z + cx, fy * cam[:, 1] / z + cy
    if use_ndc_scale:
        wr = scale * z / fx * (0.5 * H if H <= W else 0.5 * W)
    elif knn_r is not None:
        wr = knn_r[keep]
    else:
        wr = np.full_like(z, scale)
    return u, v, z, wr * fx / z, idx


def _undecidable(u, v, z, rad, H, W, max_hit):
    bad = np.zeros((H, W), bool)
    cnt = np.zeros((H, W), np.int32)
    last = np.full((H, W), np.nan)
    for i in np.argsort(z, kind="stable"):
        R = int(np.ceil(rad[i])) + 1
        x0, x1 = max(int(np.floor(u[i])) - R, 0), min(int(np.floor(u[i])) + R, W - 1)
        y0, y1 = max(int(np.floor(v[i])) - R, 0), min(int(np.floor(v[i])) + R, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        xs, ys = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
        d2 = (xs - u[i]) ** 2 + (ys - v[i]) ** 2
        r2 = rad[i] ** 2
        win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        bad[win] |= np.abs(d2 - r2) <= 1e-4 * max(r2, 1.0)
        cov = (d2 <= r2) & (cnt[win] < max_hit)
        dz = np.abs(last[win] - z[i])
        bad[win] |= cov & (dz > 0) & (dz < 1e-6 * z[i])
        last[win] = np.where(cov, z[i], last[win])
        cnt[win] += cov
    return bad


def _verdict(got, want, bad, atol):
    """got / want [H,W,C]; bad [H,W]."""
    assert got.shape == want.shape, (got.shape, want.shape)
    ok = ~bad
    assert bad.mean() <= 1e-3, f"undecidable pixels {bad.mean():.2e} of the frame"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=-1)
    worst = err[ok].max() if ok.any() else 0.0
    assert worst <= atol, f"max error {worst} on decidable pixels ({(err[ok] > atol).sum()} pixels over {atol})"


def _check(c2w, ixt, pts, feat, H, W, atol=None, knn_dist2=None, **kw):
    from street_crafter_amd.point_render import render_points_hip
    occ, max_hit = kw.get("occ", 1.0), kw.get("max_hit", 10)
    want = lc.render_points(c2w, ixt, pts, feat, H, W, knn_dist2=knn_dist2, **kw)
    got = render_points_hip(c2w, ixt, pts, feat, H, W, knn_dist2=knn_dist2, **kw)
    assert got.shape == (1, H, W, 4) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    knn_r = None
    if kw.get("use_knn_scale") and not kw.get("use_ndc_scale"):
        knn_r = lc.knn_point_radii(pts, kw.get("scale", 0.035), kw.get("knn_scale_down", 1.0), knn_dist2)
    u, v, z, rad, _ = _geometry(c2w, ixt, pts, H, W, kw.get("scale", 0.035), kw.get("use_ndc_scale", False),
                                kw.get("near", 1.0), kw.get("far", 100.0), knn_r)
    bad = _undecidable(u, v, z, rad, H, W, max_hit)
    _verdict(got[0], want[0], bad, (0.0 if occ >= 1.0 else 1e-5) if atol is None else atol)
    return got, want, bad


def _cloud(n, seed, H, W, fx, zr=(2.0, 60.0)):
    rng = np.random.default_rng(seed)
    z = rng.uniform(*zr, n)
    u, v = rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)
    pts = np.stack([(u - W / 2) * z / fx, (v - H / 2) * z / fx, z], 1).astype(np.float32)
    feat = np.concatenate([rng.uniform(0, 1, (n, 3)), z[:, None], np.ones((n, 1))], 1).astype(np.float32)
    return pts, feat


def _K(fx, W, H):
    return np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1.0]])


def test_opaque_ndc_scale_40k_points():
    H, W, fx = 320, 480, 400.0
    pts, feat = _cloud(40_000, 1, H, W, fx)
    got, want, _ = _check(np.eye(4), _K(fx, W, H), pts, feat, H, W, use_ndc_scale=True, scale=0.01)
    assert 0.2 < (got[0, ..., 3] > 0).mean() < 1.0
    assert set(np.unique(got[0, ..., 3])) <= {0.0, 1.0}


def test_translucent_max_hit_is_exercised():
    H, W, fx = 120, 160, 150.0
    rng = np.random.default_rng(2)
    pts, feat = _cloud(2_000, 3, H, W, fx, zr=(3.0, 30.0))
    # a stack of 40 points along one ray at distinct depths: > max_hit covering points on the same pixels
    zs = np.linspace(4.0, 20.0, 40)
    stack = np.stack([np.full(40, 0.2) * zs / fx, np.full(40, -0.3) * zs / fx, zs], 1)
    stack_f = np.concatenate([rng.uniform(0, 1, (40, 3)), zs[:, None], np.ones((40, 1))], 1)
    pts = np.concatenate([pts, stack.astype(np.float32)])
    feat = np.concatenate([feat, stack_f.astype(np.float32)])
    got, want, _ = _check(np.eye(4), _K(fx, W, H), pts, feat, H, W, occ=0.4, max_hit=10, scale=0.05)
    a = got[0, ..., 3]
    assert abs(a.max() - (1 - 0.6 ** 10)) < 1e-5          # the cap binds: 10 hits, not 40
    more = lc.render_points(np.eye(4), _K(fx, W, H), pts, feat, H, W, occ=0.4, max_hit=40, scale=0.05)
    assert more[0, ..., 3].max() > a.max() + 1e-3


def test_knn_scale_uses_hip_distcuda2():
    from scipy.spatial import cKDTree
    from street_crafter_amd.point_render import render_points_hip
    H, W, fx = 120, 160, 300.0
    rng = np.random.default_rng(4)
    dense = rng.normal(scale=0.02, size=(400, 3)) + np.array([0.0, 0.0, 10.0])
    sparse = rng.uniform(-3, 3, size=(60, 3)) + np.array([0.0, 0.0, 12.0])
    pts = np.concatenate([dense, sparse]).astype(np.float32)
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4)
    d2 = (d[:, 1:] ** 2).mean(1).astype(np.float32)
    feat = np.concatenate([rng.uniform(0, 1, (pts.shape[0], 3)), np.ones((pts.shape[0], 2))], 1).astype(np.float32)
    K = _K(fx, W, H)
    # the GPU radii come from the HIP distCUDA2 (knn_dist2 not given); the oracle is given the scipy distances
    want = lc.render_points(np.eye(4), K, pts, feat, H, W, scale=0.05, use_knn_scale=True, knn_dist2=d2)
    got = render_points_hip(np.eye(4), K, pts, feat, H, W, scale=0.05, use_knn_scale=True).cpu().numpy()
    knn_r = lc.knn_point_radii(pts, 0.05, 1.0, d2)
    u, v, z, rad, _ = _geometry(np.eye(4), K, pts, H, W, 0.05, False, 1.0, 100.0, knn_r)
    _verdict(got[0], want[0], _undecidable(u, v, z, rad, H, W, 10), 0.0)
    const = lc.render_points(np.eye(4), K, pts, feat, H, W, scale=0.05)
    assert 0 < (got[0, ..., 3] > 0).sum() < (const[0, ..., 3] > 0).sum()


def test_depth_plane_and_background():
    from street_crafter_amd.point_render import render_points_hip
    H, W, fx = 96, 128, 110.0
    pts, feat = _cloud(3_000, 5, H, W, fx, zr=(2.0, 40.0))
    K = _K(fx, W, H)
    kw = dict(occ=0.4, max_hit=10, scale=0.04)
    img, depth = render_points_hip(np.eye(4), K, pts, feat, H, W, return_depth=True, **kw)
    assert depth.shape == (1, H, W)
    zfeat = feat.copy()
    zfeat[:, :3] = feat[:, 3:4]                             # features = z: the same weights give the depth sum
    want_d = lc.render_points(np.eye(4), K, pts, zfeat, H, W, **kw)[0, ..., :1]
    u, v, z, rad, _ = _geometry(np.eye(4), K, pts, H, W, 0.04, False, 1.0, 100.0)
    bad = _undecidable(u, v, z, rad, H, W, 10)
    _verdict(depth.cpu().numpy()[0][..., None], want_d, bad, 1e-5 * 40)
    bg = np.array([0.2, 0.5, 0.9], np.float32)
    got = render_points_hip(np.eye(4), K, pts, feat, H, W, bg=bg, **kw).cpu().numpy()[0]
    want = lc.render_points(np.eye(4), K, pts, feat, H, W, **kw)[0]
    want_bg = want.copy()
    want_bg[..., :3] += (1 - want[..., 3:4]) * bg
    _verdict(got, want_bg, bad, 1e-5)
    np.testing.assert_array_equal(got[..., 3], img.cpu().numpy()[0, ..., 3])


def test_ties_lower_index_wins_bit_exact():
    from street_crafter_amd.point_render import render_points_hip
    H, W, fx = 64, 64, 80.0
    base, _ = _cloud(300, 6, H, W, fx, zr=(3.0, 20.0))
    pts = np.concatenate([base, base, base])                 # three copies at identical depths
    n = base.shape[0]
    feat = np.zeros((3 * n, 5), np.float32)
    feat[:n, 0], feat[n:2 * n, 1], feat[2 * n:, 2] = 1.0, 1.0, 1.0
    for occ in (1.0, 0.5):
        want = lc.render_points(np.eye(4), _K(fx, W, H), pts, feat, H, W, occ=occ, scale=0.05)
        got = render_points_hip(np.eye(4), _K(fx, W, H), pts, feat, H, W, occ=occ, scale=0.05).cpu().numpy()
        if occ == 1.0:
            np.testing.assert_array_equal(got, want)
            cov = got[0, ..., 3] > 0
            assert cov.any() and (got[0][cov][:, 0] == 1.0).all()     # the first copy (red) owns every pixel
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


def test_edges_empty_culled_border_and_subpixel():
    from street_crafter_amd.point_render import render_points_hip
    H, W, fx = 50, 70, 60.0                                  # not multiples of 16: partial tiles on two sides
    K = _K(fx, W, H)
    z0 = np.zeros((0, 3), np.float32)
    out = render_points_hip(np.eye(4), K, z0, np.zeros((0, 5), np.float32), H, W)
    assert out.shape == (1, H, W, 4) and float(out.abs().sum()) == 0.0
    far = np.array([[0, 0, 150.0], [0, 0, 0.5], [0, 0, -3.0], [1, 1, 100.0], [0, 0, 1.0]], np.float32)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    out = render_points_hip(np.eye(4), K, far, np.ones((5, 5), np.float32), H, W, bg=bg).cpu().numpy()
    assert (out[0, ..., 3] == 0).all() and np.allclose(out[0, ..., :3], bg)
    # discs straddling the border, on every side and the corners
    rng = np.random.default_rng(7)
    uv = np.concatenate([np.stack([rng.uniform(-3, 3, 40), rng.uniform(0, H, 40)], 1),
                         np.stack([rng.uniform(W - 3, W + 3, 40), rng.uniform(0, H, 40)], 1),
                         np.stack([rng.uniform(0, W, 40), rng.uniform(-3, 3, 40)], 1),
                         np.stack([rng.uniform(0, W, 40), rng.uniform(H - 3, H + 3, 40)], 1),
                         np.array([[0, 0], [W, 0], [0, H], [W, H]], float)])
    z = rng.uniform(3, 10, uv.shape[0])
    pts = np.stack([(uv[:, 0] - W / 2) * z / fx, (uv[:, 1] - H / 2) * z / fx, z], 1).astype(np.float32)
    feat = np.concatenate([rng.uniform(0, 1, (len(z), 3)), np.ones((len(z), 2))], 1).astype(np.float32)
    got, _, _ = _check(np.eye(4), K, pts, feat, H, W, scale=0.2)
    assert got[0, 0, :, 3].any() and got[0, -1, :, 3].any() and got[0, :, 0, 3].any() and got[0, :, -1, 3].any()
    # r < 0.5 px: a disc covers a pixel only when its centre is that close to the pixel centre
    pts_s, feat_s = _cloud(4_000, 8, H, W, fx, zr=(5.0, 30.0))
    got, want, _ = _check(np.eye(4), K, pts_s, feat_s, H, W, scale=0.02)
    assert 0 < (got[0, ..., 3] > 0).sum() < 0.9 * H * W


def _projection_3dgs(znear, zfar, fovx, fovy):
    t, r = np.tan(fovy / 2) * znear, np.tan(fovx / 2) * znear
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 2 * znear / (2 * r), 2 * znear / (2 * t)
    P[3, 2], P[2, 2], P[2, 3] = 1.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return P


def test_drop_in_point_rasterizer():
    from diff_point_rasterization import PointRasterizationSettings, PointRasterizer
    from street_crafter_amd.point_render import render_points_hip
    H, W, fx = 160, 240, 200.0
    K = _K(fx, W, H)
    # a camera whose matrices are exact in fp32: axis permutation + integer translation
    w2c = np.eye(4)
    w2c[:3, :3] = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], float)
    w2c[:3, 3] = [1.0, -2.0, 3.0]
    c2w = np.linalg.inv(w2c)
    pc, feat = _cloud(8_000, 9, H, W, fx, zr=(2.0, 90.0))
    pts = ((pc.astype(np.float64) - w2c[:3, 3]) @ w2c[:3, :3]).astype(np.float32)      # camera -> world
    fovx, fovy = 2 * np.arctan(W / (2 * fx)), 2 * np.arctan(H / (2 * fx))
    V = w2c.T
    F = V @ _projection_3dgs(1.0, 100.0, fovx, fovy).T
    dev = "cuda"
    s = PointRasterizationSettings(image_height=H, image_width=W, tanfovx=float(np.tan(fovx / 2)),
                                   tanfovy=float(np.tan(fovy / 2)), bg=torch.zeros(3, device=dev), scale_modifier=1.0,
                                   viewmatrix=torch.tensor(V, dtype=torch.float32, device=dev),
                                   projmatrix=torch.tensor(F, dtype=torch.float32, device=dev), sh_degree=0,
                                   max_hit=10, campos=torch.tensor(c2w[:3, 3], dtype=torch.float32, device=dev),
                                   prefiltered=False, debug=False)
    scale, occ = 0.03, 0.7
    xyz = torch.from_numpy(pts).to(dev)
    rgb = torch.from_numpy(feat[:, :3].copy()).to(dev)
    image, depth, alpha, radii = PointRasterizer(raster_settings=s)(
        means3D=xyz, means2D=torch.zeros_like(xyz, requires_grad=True) + 0, colors_precomp=rgb,
        opacities=torch.full_like(xyz[:, :1], occ), radius=torch.full_like(xyz[:, :1], scale))
    assert image.shape == (3, H, W) and depth.shape == (1, H, W) and alpha.shape == (1, H, W)
    assert radii.shape == (pts.shape[0],) and radii.dtype == torch.int32 and not image.requires_grad
    got = torch.cat([image.permute(1, 2, 0), alpha.permute(1, 2, 0)], -1).cpu().numpy()
    hip = render_points_hip(c2w, K, pts, feat, H, W, occ=occ, scale=scale).cpu().numpy()[0]
    want = lc.render_points(c2w, K, pts, feat, H, W, occ=occ, scale=scale)[0]
    u, v, z, rad, idx = _geometry(c2w, K, pts, H, W, scale, False, 1.0, 100.0)
    bad = _undecidable(u, v, z, rad, H, W, 10)
    _verdict(got, want, bad, 1e-5)
    _verdict(got, hip, bad, 1e-5)
    want_r = np.zeros(pts.shape[0], np.int64)
    want_r[idx] = np.ceil(rad)
    r = radii.cpu().numpy()
    sure = np.ones(pts.shape[0], bool)
    sure[idx] = np.abs(rad - np.round(rad)) > 1e-5
    np.testing.assert_array_equal(r[sure], want_r[sure])
    assert (r[np.setdiff1d(np.arange(pts.shape[0]), idx)] == 0).all() and (r[idx] > 0).all()


def _synthetic_log(num_frames=6, seed=0):
    # test_lidar_condition_cpu.py's synthetic log
    rng = np.random.default_rng(seed)
    ego = []
    for f in range(num_frames):
        p = np.eye(4)
        p[:3, 3] = [2.0 * f, 0.1 * f, 0.0]
        ego.append(p)
    bk = {f: np.concatenate([rng.uniform([5, -10, -1], [60, 10, 4], size=(400, 3)) + ego[f][:3, 3],
                             rng.uniform(0, 1, size=(400, 3))], axis=1) for f in range(num_frames)}
    car = {f: np.concatenate([rng.uniform(-1, 1, size=(50, 3)) * [2.2, 0.9, 0.7], np.tile([1.0, 0.0, 0.0], (50, 1))],
                             axis=1) for f in (1, 2, 3)}
    return ego, {"background": bk, "car_1": car}


def test_condition_frame_uint8():
    from street_crafter_amd.point_render import render_condition_frame_hip
    ego, ply = _synthetic_log()
    ext = np.eye(4)
    ext[:3, :3] = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], float)
    ixt = np.array([[150.0, 0, 96.0], [0, 150.0, 64.0], [0, 0, 1.0]])
    track = {"car_1": {"camera_box": None,
                       "lidar_box": {"heading": 0.0, "center_x": 12.0, "center_y": 0.0, "center_z": 0.0}}}
    h, w = 128, 192
    for shift in (0.0, 2.0):
        rgb, mask = render_condition_frame_hip(ply, track, ego, ego[2], 2, ext, ixt, h, w, delta_frames=2, shift=shift)
        rgb0, mask0 = lc.render_condition_frame(ply, track, ego, ego[2], 2, ext, ixt, h, w, delta_frames=2, shift=shift)
        assert rgb.dtype == np.uint8 and rgb.shape == (h, w, 3) and mask.shape == (h, w)
        cloud = lc.assemble_frame(ply, track, ego[2], 2, len(ego), 2, shift)
        c2w = lc.shifted_camera(ego[2], ego, 2, ext, shift)
        xyz, _ = lc.filter_visible(cloud[:, :3], cloud[:, 3:], c2w, ixt, h, w)
        u, v, z, rad, _ = _geometry(c2w, ixt, xyz, h, w, 0.01, True, 1.0, 100.0)
        bad = _undecidable(u, v, z, rad, h, w, 10)
        _verdict(np.concatenate([rgb, mask[..., None]], -1), np.concatenate([rgb0, mask0[..., None]], -1), bad, 0)
        assert (mask == 255).any()


def _demo():
    spec = importlib.util.spec_from_file_location("bench_point_render", os.path.join(ROOT, "tools",
                                                                                     "bench_point_render.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_full_size_demo_workload_unfiltered():
    from street_crafter_amd.point_render import render_points_hip
    demo = _demo().demo_workload()
    pts = torch.from_numpy(demo["cloud"][:, :3].astype(np.float32)).cuda()
    feat = torch.from_numpy(demo["cloud"][:, 3:].astype(np.float32)).cuda()
    assert pts.shape[0] > 3_000_000
    a = render_points_hip(demo["c2w"], demo["ixt"], pts, feat, demo["H"], demo["W"], use_ndc_scale=True, scale=0.01)
    b = render_points_hip(demo["c2w"], demo["ixt"], pts, feat, demo["H"], demo["W"], use_ndc_scale=True, scale=0.01)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    cov = (a[0, ..., 3] > 0).float().mean().item()
    assert 0.3 < cov < 1.0, cov
    assert set(torch.unique(a[0, ..., 3]).tolist()) <= {0.0, 1.0}
    assert float(a[0, ..., :3].max()) <= 1.0 and float(a[0, ..., :3].min()) >= 0.0


def test_one_and_four_waves_per_tile_agree_bit_for_bit():
    from street_crafter_amd import _lib
    from street_crafter_amd.point_render import render_points_hip
    H, W, fx = 200, 300, 250.0
    pts, feat = _cloud(20_000, 10, H, W, fx)
    out = {}
    for waves in (1, 4):
        prev = _lib.set_option("point_raster_waves", waves)
        try:
            out[waves] = [render_points_hip(np.eye(4), _K(fx, W, H), pts, feat, H, W, occ=occ, scale=0.03,
                                            return_depth=True) for occ in (1.0, 0.3)]
        finally:
            _lib.set_option("point_raster_waves", prev)
    for (a, da), (b, db) in zip(out[1], out[4]):
        assert torch.equal(a, b) and torch.equal(da, db)
