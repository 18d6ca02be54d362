"""numpy-only helpers of the resident LiDAR sequence tests (street_crafter_amd/lidar_sequence.py,
csrc/point_assemble.hip): the kernel's float64 steps restated element by element, and two synthetic logs.

Restatements (every product and sum written out, left to right, so that numpy rounds exactly where the kernel does;
no BLAS):
  assemble      w = p, or w_r = P[r][0] x + P[r][1] y + P[r][2] z + P[r][3]          (kernel step 3)
  visible_mask  cam_r = M[r][0] w_x + M[r][1] w_y + M[r][2] w_z + M[r][3], pix_r = K[r][0] cam_x + K[r][1] cam_y +
                K[r][2] cam_z; kept iff cam_z > 1e-3, 0 <= pix_0 / pix_2 < W, 0 <= pix_1 / pix_2 < H   (step 4)
  camera_centred  q = (float32)(w - origin)                                           (step 5)
`assemble` takes the points from lidar_condition.make_lidar_ply, not from the resident arrays, so it also checks the
packing of whoever made the plan.

Logs: dict(ply, track_info {frame: {track: boxes}}, ego [F] of 4x4, ext, ixt, H, W, F).
  random_log   ego poses that rotate about z, world origin thousands of metres away, 5 actors with non-zero headings
               that miss some frames, one of them with a camera_box.
  dyadic_log   every coordinate, pose entry and intrinsic is a short binary fraction, headings are 0, poses are
               translations and exact axis permutations: every sum and product of the assembly, the filter and the
               camera-centre subtraction is exact in any evaluation order, so BLAS and the element-wise forms agree
               bit for bit.  Two one-point actors, "tie_a" and "tie_b", put their point at the same world position
               (pixel centre (72.5, 68.5), depth 4 from every frame's camera: the ego does not move along its x).
"""
import numpy as np

from street_crafter_amd import lidar_condition as lc

H, W = 128, 192
EXT = np.eye(4)
EXT[:3, :3] = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], float)      # camera z = ego x, x = -ego y, y = -ego z
EXT[:3, 3] = [1.5, 0.0, 0.25]


def _rows(A, x, y, z, with_t):
    out = []
    for r in range(3):
        v = A[r, 0] * x + A[r, 1] * y + A[r, 2] * z
        out.append(v + A[r, 3] if with_t else v)
    return out


def assemble(ply_dict, plan):
    """-> (world xyz float64 [N,3], rgb float64 [N,3]) of a FramePlan, element-wise."""
    per_track = lc.make_lidar_ply(ply_dict, plan.window[0], plan.window[1])
    xyz, rgb = [], []
    for track, seg in zip(plan.tracks, plan.segments):
        cloud = per_track[track]
        assert cloud.shape[0] == int(seg["count"]), track
        x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
        if seg["pose"] >= 0:
            x, y, z = _rows(plan.poses[int(seg["pose"])], x, y, z, True)
        xyz.append(np.stack([x, y, z], axis=1))
        rgb.append(cloud[:, 3:6])
    if not xyz:
        return np.zeros((0, 3)), np.zeros((0, 3))
    return np.concatenate(xyz, axis=0), np.concatenate(rgb, axis=0)


def visible_mask(w, c2w, ixt, h, width):
    M = np.linalg.inv(c2w)
    cx, cy, cz = _rows(M, w[:, 0], w[:, 1], w[:, 2], True)
    p0, p1, p2 = _rows(np.asarray(ixt, np.float64), cx, cy, cz, False)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = p0 / p2, p1 / p2
        return (cz > 1e-3) & (u >= 0) & (u < width) & (v >= 0) & (v < h)


def camera_centred(w, c2w):
    return (w - c2w[:3, 3]).astype(np.float32)


def centred_camera(c2w):
    """(view [4,4] of the points moved by -origin, origin): the two lines of render_points_hip's host-array branch."""
    origin = c2w[:3, 3].copy()
    view = np.linalg.inv(c2w)
    view[:3, 3] += view[:3, :3] @ origin
    return view, origin


def _box(heading, x, y, z):
    return {"heading": float(heading), "center_x": float(x), "center_y": float(y), "center_z": float(z)}


def random_log(seed, n_bg=300, n_actor=60, frames=8):
    rng = np.random.default_rng(seed)
    ego = []
    base = np.array([3000.0 + 500.0 * rng.uniform(), -2500.0 + 300.0 * rng.uniform(), 40.0 + rng.uniform()])
    for f in range(frames):
        yaw = 0.3 + 0.04 * f
        p = np.eye(4)
        p[:3, :3] = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        p[:3, 3] = base + np.array([1.4 * f * np.cos(0.3), 1.4 * f * np.sin(0.3), 0.01 * f])
        ego.append(p)

    def background(f):
        local = np.stack([rng.uniform(-10, 60, n_bg), rng.uniform(-12, 12, n_bg), rng.uniform(-1.8, 5, n_bg),
                          np.ones(n_bg)], axis=1)
        return np.concatenate([(local @ ego[f].T)[:, :3], rng.uniform(0, 1, (n_bg, 3))], axis=1)
    ply = {"background": {f: background(f) for f in range(frames)}}
    track_info = {f: {} for f in range(frames)}
    for k in range(5):
        name = f"veh_{k}"
        seen = [f for f in range(frames) if (f + k) % 4 != 1]           # every actor misses some frames
        ply[name] = {f: np.concatenate([rng.uniform(-1, 1, (n_actor + k, 3)) * [2.3, 1.0, 0.8],
                                        np.tile(rng.uniform(0, 1, 3), (n_actor + k, 1))], axis=1) for f in seen}
        for f in range(frames):
            if (f + 2 * k) % 7 == 3:                                    # ... and is untracked in some
                continue
            lidar = _box(0.2 + 0.15 * k + 0.01 * f, 8.0 + 7.0 * k + 0.3 * f, -5.0 + 2.5 * k, -0.9)
            camera = _box(lidar["heading"] + 0.02, lidar["center_x"] + 0.1, lidar["center_y"] - 0.05, -0.85) \
                if k == 2 else None
            track_info[f][name] = {"camera_box": camera, "lidar_box": lidar}
    ixt = np.array([[210.0, 0, 96.0], [0, 205.0, 64.0], [0, 0, 1.0]])
    return {"ply": ply, "track_info": track_info, "ego": ego, "ext": EXT.copy(), "ixt": ixt, "H": H, "W": W,
            "F": frames}


TIE_PIXEL = (72, 68)          # the pixel whose centre the tie point projects to
TIE_A_RGB, TIE_B_RGB = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)


def dyadic_log(frames=6, n_bg=400, n_actor=50, seed=5):
    rng = np.random.default_rng(seed)
    ego = []
    for f in range(frames):
        p = np.eye(4)
        p[:3, 3] = [4096.0, -2048.0 + 0.5 * f, 64.0]                    # the ego slides sideways: depths stay put
        ego.append(p)

    def lattice(n, lo, hi, step):
        return rng.integers(int(lo / step), int(hi / step) + 1, n).astype(np.float64) * step

    def colours(n):
        return rng.integers(0, 257, (n, 3)).astype(np.float64) / 256.0

    def background(f):
        # depths (ego x - 1.5) are powers of two from 8 up: nothing sits in front of the tie point at depth 4
        x = 1.5 + 2.0 ** rng.integers(3, 7, n_bg)
        local = np.stack([x, lattice(n_bg, -8, 8, 0.125), lattice(n_bg, -2, 4, 0.125)], axis=1)
        return np.concatenate([local + ego[f][:3, 3], colours(n_bg)], axis=1)
    ply = {"background": {f: background(f) for f in range(frames)}}
    track_info = {f: {} for f in range(frames)}
    for k in range(3):
        name = f"veh_{k}"
        seen = [f for f in range(frames) if (f + k) % 3 != 1]
        ply[name] = {f: np.concatenate([np.stack([lattice(n_actor, -2, 2, 0.25), lattice(n_actor, -1, 1, 0.125),
                                                  lattice(n_actor, -0.75, 0.75, 0.125)], axis=1),
                                        np.tile(colours(1), (n_actor, 1))], axis=1) for f in seen}
        for f in range(frames):
            lidar = _box(0.0, 9.5 + 8.0 * k, -3.0 + 2.0 * k + 0.25 * f, -0.5)
            camera = _box(0.0, 9.5 + 8.0 * k, -3.0 + 2.0 * k + 0.25 * f + 0.125, -0.5) if k == 1 else None
            track_info[f][name] = {"camera_box": camera, "lidar_box": lidar}
    # the tie: camera frame (x, y, z) = ((72.5 - 96) 4 / 64, (68.5 - 64) 4 / 64, 4) -> ego (5.5, 1.46875, -0.03125)
    for name, rgb, cy, py in (("tie_a", TIE_A_RGB, 1.0, 0.46875), ("tie_b", TIE_B_RGB, 2.0, -0.53125)):
        ply[name] = {f: np.array([[0.0, py, 0.0, *rgb]]) for f in range(frames)}
        for f in range(frames):
            track_info[f][name] = {"camera_box": None, "lidar_box": _box(0.0, 5.5, cy, -0.03125)}
    ixt = np.array([[64.0, 0, 96.0], [0, 64.0, 64.0], [0, 0, 1.0]])
    log = {"ply": ply, "track_info": track_info, "ego": ego, "ext": EXT.copy(), "ixt": ixt, "H": H, "W": W,
           "F": frames}
    for f in range(frames):                                            # the camera inverts exactly
        c2w = ego[f] @ EXT
        assert np.array_equal(np.linalg.inv(c2w) @ c2w, np.eye(4))
    return log


def actor_poses(log, frame, box="lidar_box"):
    """{track: ego_pose @ box pose} of the actors tracked in `frame`: what the training-time caller passes."""
    return {t: log["ego"][frame] @ lc.box_pose(info[box]) for t, info in log["track_info"][frame].items()}
