"""The whole point-render pipeline on exact scenes, and `sc_point_project` row by row (csrc/point_raster.hip through
street_crafter_amd/point_render.py and the drop-in diff_point_rasterization).

Exact scenes (tests/point_raster_ref.scene_runs): the camera is an axis permutation plus an integer translation, fx = fy =
64, z in {2, 4, 8, 16}, u and v are multiples of 1/8 and r is dyadic, so every coverage decision is the same in fp32 and
in float64 (point_raster_ref.assert_exact holds after project_f64) and NO pixel is left out: the image is bit-equal to
the float32 replay of the contract's walk over lists_from(project_f64(...)) and within the float64 bars of
tests/test_point_raster_walk_gpu.py; radii, tile lists, offsets and n_isects equal the reference's exactly.  "hip" runs go
through render_points_hip (one occ, radius mode 0), "dropin" runs through PointRasterizer with per-point opacities, a
per-point radius array and scale_modifier = 1/2.

sc_point_project rows: a general float64 camera (rotation about a skew axis, translation of tens of metres), all four
radius modes, N on both sides of the launch block of 256.  Inputs are redrawn until, in float64, no z lies within
relative 1e-9 of near, far or 0 and no r within relative 1e-9 of an integer (asserted on the finished inputs), so keep
and ceil(r) are decided and no row is excluded.  Per row: keep equal; u, v, z, r^2 within 2^-24 |x| (1 + 2^-20) of
float64 (one fp32 rounding of the fp64 value; mode 2: r^2 within 3 * 2^-23 r^2, the fp32 radius rule adds up to 1 ulp on
r before the square); radii == max(ceil(min(r, 2^30)), 1); means2d / depths equal the record's fields where kept and are
0 where culled; colour and alpha are copied bit for bit.  Rows whose float64 geometry is not finite (NaN / inf inputs)
are held to keep, the zeros and the copied fields.
"""
import numpy as np
import pytest
import torch

import point_raster_ref as PR
from guard_arena import Arena

pytestmark = pytest.mark.gpu

RUNS = {r["name"]: r for r in PR.scene_runs()}
EPS24 = PR.EPS24


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _project(run_args, N, pts, colors, opac, occ, radius_in):
    """sc_point_project through the C entry, outputs in a guarded arena -> numpy radii, means2d, depths, records."""
    from street_crafter_amd import _lib, isect
    lib = _lib.load()
    vm, fx, fy, cx, cy, focal, W, H, near, far, mode, scale, ksd = run_args
    dev = lambda x, dt=np.float32: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    d_pts, d_col, d_op, d_rin, d_vm = dev(pts), dev(colors), dev(opac), dev(radius_in), dev(vm, np.float64)
    ar = Arena({"radii": 4 * N, "means2d": 8 * N, "depths": 4 * N, "records": 32 * N})
    _lib.check(lib.sc_point_project(d_pts.data_ptr(), d_col.data_ptr(), None if d_op is None else d_op.data_ptr(),
                                    float(occ), None if d_rin is None else d_rin.data_ptr(), N, d_vm.data_ptr(), fx, fy,
                                    cx, cy, focal, W, H, near, far, mode, scale, ksd, ar.ptr("radii"), ar.ptr("means2d"),
                                    ar.ptr("depths"), ar.ptr("records"), isect._stream(d_pts)), "sc_point_project")
    torch.cuda.synchronize()
    assert ar.broken_guards() == []
    return (ar.view("radii", torch.int32).cpu().numpy(), ar.view("means2d", torch.float32).cpu().numpy().reshape(N, 2),
            ar.view("depths", torch.float32).cpu().numpy(), ar.view("records", torch.float32).cpu().numpy().reshape(N, 8))


def _projection_3dgs(fx, fy, W, H, znear, zfar):
    """3DGS getProjectionMatrix (column form) of a centred pinhole."""
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 2 * fx / W, 2 * fy / H
    P[3, 2], P[2, 2], P[2, 3] = 1.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return P


def _dropin(run):
    import diff_point_rasterization as dpr
    W, H = run["W"], run["H"]
    V = PR.W2C.T.copy()
    F = V @ _projection_3dgs(PR.FOCAL, PR.FOCAL, W, H, run["near"], run["far"]).T
    s = dpr.PointRasterizationSettings(
        image_height=H, image_width=W, tanfovx=W / (2 * PR.FOCAL), tanfovy=H / (2 * PR.FOCAL),
        bg=None if run["bg"] is None else torch.from_numpy(run["bg"]).cuda(), scale_modifier=PR.HALF,
        viewmatrix=torch.from_numpy(V), projmatrix=torch.from_numpy(F), sh_degree=0, max_hit=run["max_hit"],
        campos=torch.zeros(3), prefiltered=False, debug=False)
    # the settings must hand the kernel the lattice camera exactly (float64 matrices; the planes are far from every z)
    w2c, fx, fy, cx, cy, zn, zf, focal = dpr.camera_from_settings(s)
    assert np.array_equal(w2c, PR.W2C) and (fx, fy, cx, cy, focal) == (PR.FOCAL, PR.FOCAL, W / 2, H / 2, PR.FOCAL)
    assert abs(zn - run["near"]) < 1e-9 and abs(zf - run["far"]) < 1e-6
    xyz = torch.from_numpy(run["points"]).cuda()
    image, depth, alpha, radii = dpr.PointRasterizer(raster_settings=s)(
        means3D=xyz, means2D=torch.zeros_like(xyz), colors_precomp=torch.from_numpy(run["colors"]).cuda(),
        opacities=torch.from_numpy(run["opacities"]).cuda()[:, None], radius=torch.from_numpy(run["radius_in"]).cuda()[:, None])
    assert image.shape == (3, H, W) and depth.shape == (1, H, W) and alpha.shape == (1, H, W)
    return (image.permute(1, 2, 0).cpu().numpy(), alpha[0].cpu().numpy(), depth[0].cpu().numpy(), radii.cpu().numpy())


def _hip(run):
    from street_crafter_amd.point_render import render_points_hip
    W, H = run["W"], run["H"]
    K = np.array([[PR.FOCAL, 0, W / 2], [0, PR.FOCAL, H / 2], [0, 0, 1.0]])
    c2w = np.linalg.inv(PR.W2C)
    assert np.array_equal(np.linalg.inv(c2w), PR.W2C)
    kw = dict(occ=run["occ"], scale=run["scale"], max_hit=run["max_hit"], near=run["near"], far=run["far"], bg=run["bg"],
              return_depth=True)
    img, depth = render_points_hip(c2w, K, torch.from_numpy(run["points"]).cuda(), torch.from_numpy(run["colors"]).cuda(),
                                   H, W, **kw)
    assert img.shape == (1, H, W, 4) and depth.shape == (1, H, W)
    # host points take the route through the camera centre (exact on the lattice): the same image
    img_h, depth_h = render_points_hip(c2w, K, run["points"].astype(np.float64), run["colors"], H, W, **kw)
    assert torch.equal(img, img_h) and torch.equal(depth, depth_h)
    img = img.cpu().numpy()[0]
    return img[..., :3], img[..., 3], depth[0].cpu().numpy(), None


@pytest.mark.parametrize("name", RUNS)
def test_exact_scene_lists_and_every_pixel(name):
    from street_crafter_amd import isect
    run = RUNS[name]
    ref = PR.reference_render(run)
    PR.assert_exact(ref)
    proj, W, H, N = ref["proj"], run["W"], run["H"], run["points"].shape[0]
    tw, th = PR.tiles_of(W, H)
    # -- projection and binning, step by step as point_render._render chains them
    radii, means2d, depths, records = _project((PR.W2C, PR.FOCAL, PR.FOCAL, W / 2, H / 2, PR.FOCAL, W, H, run["near"],
                                                run["far"], run["mode"], run["scale"], 1.0), N, run["points"],
                                               run["colors"], run["opacities"], run["occ"], run["radius_in"])
    keep = proj["keep"]
    assert np.array_equal(radii, proj["R"]) and np.array_equal(radii > 0, keep)
    assert np.array_equal(_bits(records[keep]), _bits(ref["records"][keep]))
    assert np.array_equal(_bits(records[:, 4:]), _bits(ref["records"][:, 4:]))
    assert np.array_equal(means2d, np.where(keep[:, None], records[:, :2], 0)) and \
        np.array_equal(depths, np.where(keep, records[:, 3], 0))
    dv = lambda x: torch.from_numpy(x).cuda()
    d_m, d_r, d_d = dv(means2d.reshape(1, N, 2)), dv(radii.reshape(1, N)), dv(depths.reshape(1, N))
    _, isect_ids, flatten_ids = isect._isect_tiles_radix(d_m, d_r, d_d, 1, N, PR.TILE, tw, th, True, isect._stream(d_m))
    assert int(flatten_ids.numel()) == ref["n_isects"]
    assert np.array_equal(flatten_ids.cpu().numpy(), ref["flatten_ids"])
    if ref["n_isects"]:
        offsets = isect.isect_offset_encode(isect_ids, 1, tw, th)
        assert np.array_equal(offsets.cpu().numpy().reshape(-1), ref["offsets"])
    # -- the public entry
    rgb, alpha, depth, got_radii = (_hip if run["kind"] == "hip" else _dropin)(run)
    if got_radii is not None:
        assert got_radii.dtype == np.int32 and np.array_equal(got_radii, proj["R"])      # ceil(r) kept, 0 culled
    f64, f32 = ref["f64"], ref["f32"]
    assert np.array_equal(_bits(rgb), _bits(f32["rgb"])), name
    assert np.array_equal(_bits(alpha), _bits(f32["alpha"])), name
    assert np.array_equal(_bits(depth), _bits(f32["depth"])), name
    worst = PR.judge(rgb, alpha, depth, f64, name)
    print(f"[point_render_exact] {name}: I = {ref['n_isects']}, worst |hip - f64| / bar = {worst:.3f}")


# ---- sc_point_project, row by row ---------------------------------------------------------------------------------------
NEAR, FAR = 1.0, 100.0
ROW_W, ROW_H, ROW_F = 640, 400, 300.0
MODES = {0: dict(scale=0.05, ksd=1.0), 1: dict(scale=0.0137, ksd=1.0), 2: dict(scale=0.2, ksd=0.75), 3: dict(scale=0.8, ksd=1.0)}


def _camera():
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    ang = 0.7
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    vm = np.eye(4)
    vm[:3, :3], vm[:3, 3] = R, [31.7, -48.2, 22.9]
    return vm


def _rows(N, mode, seed):
    """Inputs with the cull rows mixed in; redrawn until keep and ceil(r) are decided in float64."""
    vm = _camera()
    cfg = MODES[mode]
    for attempt in range(50):
        rng = np.random.default_rng(seed + 1000 * attempt)
        zc = rng.uniform(0.3, 125.0, N) if N > 1 else rng.uniform(5.0, 50.0, N)     # (the single row is a kept one)
        cam = np.stack([rng.uniform(-0.7, 0.7, N) * zc, rng.uniform(-0.5, 0.5, N) * zc, zc], 1)
        pts = ((cam - vm[:3, 3]) @ vm[:3, :3]).astype(np.float32)
        colors = rng.uniform(0, 1, (N, 3)).astype(np.float32)
        opac = rng.uniform(0.05, 1.0, N).astype(np.float32)
        rin = None
        if mode == 2:
            rin = (10.0 ** rng.uniform(-8, 0, N)).astype(np.float32)
        elif mode == 3:
            rin = rng.uniform(0.0, 0.3, N).astype(np.float32)
        bad = {}
        if N >= 255:
            behind = ((np.array([0.1, -0.2, -5.0]) - vm[:3, 3]) @ vm[:3, :3]).astype(np.float32)
            pts[3] = behind
            pts[17, 0], pts[100, 1], pts[101, 2], pts[130] = np.nan, np.inf, -np.inf, np.nan
            opac[200], opac[201], opac[202] = 0.0, 1.5, np.nan
            opac[N - 1] = -0.5                              # the last row of the launch's tail
            bad = {3, 17, 100, 101, 130, 200, 201, 202, N - 1}
            if mode == 3:
                rin[50], rin[51] = -0.1, 3.0e38             # negative; finite in fp64, infinite once in pixels and fp32
                bad |= {50, 51}
        p = PR.project_f64(pts, colors, opac, 1.0, rin, vm, ROW_F, ROW_F, ROW_W / 2, ROW_H / 2, ROW_F, NEAR, FAR, mode,
                           cfg["scale"], cfg["ksd"], ROW_H, ROW_W)
        fin = np.isfinite(p["z"]) & np.isfinite(p["r"])
        z, r = p["z"][fin], p["r"][fin]
        rel = lambda x, y: np.abs(x - y) <= 1e-9 * np.maximum(np.abs(y), 1e-300)
        near_int = rel(r, np.round(r)) & (np.round(r) > 0) & (r < 2.0 ** 30)      # (beyond: negative, or held at 2^30)
        if not (rel(z, NEAR).any() or rel(z, FAR).any() or (np.abs(z) < 1e-9).any() or near_int.any()):
            break
    else:
        raise AssertionError("no decided draw in 50 attempts")
    # asserted on the finished inputs: keep and ceil(r) are decided
    assert not (rel(z, NEAR).any() or rel(z, FAR).any() or (np.abs(z) < 1e-9).any() or near_int.any())
    for i in bad:
        assert not p["keep"][i], i
    return vm, cfg, pts, colors, opac, rin, p, bad


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 4099])
def test_project_rows(N, mode):
    vm, cfg, pts, colors, opac, rin, p, bad = _rows(N, mode, seed=N * 10 + mode)
    use_occ = N == 1                                      # the occ route of the entry: one alpha, no array
    if use_occ:
        p = PR.project_f64(pts, colors, None, 0.625, rin, vm, ROW_F, ROW_F, ROW_W / 2, ROW_H / 2, ROW_F, NEAR, FAR, mode,
                           cfg["scale"], cfg["ksd"], ROW_H, ROW_W)
    radii, means2d, depths, records = _project((vm, ROW_F, ROW_F, ROW_W / 2, ROW_H / 2, ROW_F, ROW_W, ROW_H, NEAR, FAR,
                                                mode, cfg["scale"], cfg["ksd"]), N, pts, colors,
                                               None if use_occ else opac, 0.625, rin)
    keep = p["keep"]
    assert np.array_equal(radii > 0, keep), np.nonzero((radii > 0) != keep)[0]
    assert np.array_equal(radii, p["R"]), np.nonzero(radii != p["R"])[0]
    if N >= 255:
        assert keep.sum() > N // 2 and (~keep).sum() > len(bad)          # the depth window culls rows of its own
        nb = np.array(sorted(bad))
        for j in (nb - 1, nb + 1):                                       # kept neighbours of the cull rows stay kept
            j = j[(j >= 0) & (j < N)]
            j = j[~np.isin(j, nb)]
            assert np.array_equal(radii[j] > 0, keep[j])
    worst = 0.0
    with np.errstate(all="ignore"):
        for k, name in enumerate(("u", "v", "r2", "z")):
            want = p[name]
            fin = np.isfinite(want) & np.isfinite(want.astype(np.float32))
            assert fin[keep].all()
            bar = (3 * 2.0 ** -23 if (name == "r2" and mode == 2) else EPS24 * (1 + 2.0 ** -20)) * np.abs(want[fin])
            err = np.abs(records[fin, k].astype(np.float64) - want[fin])
            assert (err <= bar).all(), (name, np.nonzero(fin)[0][err > bar][:5], err.max())
            worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max(initial=0.0)))
    assert np.array_equal(_bits(means2d), _bits(np.where(keep[:, None], records[:, :2], np.float32(0))))
    assert np.array_equal(_bits(depths), _bits(np.where(keep, records[:, 3], np.float32(0))))
    assert np.array_equal(_bits(records[:, 4:7]), _bits(colors))
    assert np.array_equal(_bits(records[:, 7]), _bits(p["a"]))
    print(f"[point_project_rows] N = {N} mode {mode}: kept {int(keep.sum())}, worst error / bar = {worst:.3f}")
