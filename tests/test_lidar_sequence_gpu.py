"""The resident LiDAR sequence on the GPU (street_crafter_amd/lidar_sequence.py, csrc/point_assemble.hip).

Everything here is an equality of bits.  `sc_point_assemble_project` is held, row by row, to the shipped
`sc_point_project` run on the element-wise float64 restatement of its first steps (tests/lidar_sequence_ref.py, whose
agreement with lidar_condition's host route tests/test_lidar_sequence_cpu.py pins on these very logs); the two public
calls are held to the shipped pipeline (`render_points_hip`, `render_condition_frame_hip`) fed that restatement.
"""
import numpy as np
import pytest
import torch

import lidar_sequence_ref as LR
from guard_arena import Arena

pytestmark = pytest.mark.gpu

MODES = {"const": (0, 0.05), "ndc": (1, 0.01), "knn": (2, 0.08)}          # radius mode, scale
KNN_SCALE_DOWN = 0.05


def _lds_capacity():
    from street_crafter_amd import _lib
    return _lib.load().sc_point_assemble_lds_segments()


def _segment_cases():
    cap = _lds_capacity()
    return {
        "single": [300],
        "edges": [1, 63, 64, 65, 255, 256, 257, 0, 1000],
        "empties": [0, 5, 0, 0, 7, 0],
        "one_block_many_segments": [10, 20, 30, 40, 500],
        "beyond_lds": [(k % 4 + 3) % 4 for k in range(cap + 1)],            # cap + 1 segments of 3, 0, 1, 2 points
        "no_points": [0, 0],
        "no_segments": [],
    }


CASES = ["single", "edges", "empties", "one_block_many_segments", "beyond_lds", "no_points", "no_segments"]


@pytest.fixture(scope="module")
def world():
    """A resident cloud around the random log's camera, and that camera."""
    from street_crafter_amd import lidar_condition as lc
    log = LR.random_log(11)
    rng = np.random.default_rng(3)
    M = 3000
    local = np.stack([rng.uniform(-5, 60, M), rng.uniform(-14, 14, M), rng.uniform(-3, 6, M), np.ones(M)], axis=1)
    xyz = np.ascontiguousarray((local @ log["ego"][2].T)[:, :3])
    rgb = rng.uniform(0, 1, (M, 3)).astype(np.float32)
    c2w = lc.shifted_camera(log["ego"][2], log["ego"], 2, log["ext"])
    return {"xyz": xyz, "rgb": rgb, "c2w": c2w, "ixt": log["ixt"], "H": log["H"], "W": log["W"],
            "d_xyz": torch.from_numpy(xyz).cuda(), "d_rgb": torch.from_numpy(rgb).cuda()}


def _table(counts, M, rng):
    """Segments over random resident ranges, a pose on every second one (small motions: the points stay in view)."""
    from street_crafter_amd.lidar_sequence import SEGMENT_DTYPE
    seg = np.zeros(len(counts), dtype=SEGMENT_DTYPE)
    poses, at = [], 0
    for k, n in enumerate(counts):
        slot = -1
        if k % 2 == 1:
            yaw = rng.uniform(-0.05, 0.05)
            P = np.array([[np.cos(yaw), -np.sin(yaw), 0, 0], [np.sin(yaw), np.cos(yaw), 0, 0], [0, 0, 1, 0.0]])
            pivot = np.array([3200.0, -2400.0, 40.0])
            P[:, 3] = pivot - P[:, :3] @ pivot + rng.uniform(-1, 1, 3)
            slot = len(poses)
            poses.append(P)
        seg[k] = (int(rng.integers(0, M - n + 1)), at, n, slot, 0)
        at += n
    return seg, (np.stack(poses) if poses else np.zeros((0, 3, 4))), at


def _expected_inputs(world, seg, poses):
    """The restatement: world points (element-wise float64), gathered colours."""
    w, c = [], []
    for s in seg:
        a, n = int(s["src_begin"]), int(s["count"])
        p = world["xyz"][a:a + n]
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        if s["pose"] >= 0:
            x, y, z = LR._rows(np.concatenate([poses[int(s["pose"])], [[0, 0, 0, 1.0]]]), x, y, z, True)
        w.append(np.stack([x, y, z], axis=1))
        c.append(world["rgb"][a:a + n])
    if not w:
        return np.zeros((0, 3)), np.zeros((0, 3), np.float32)
    return np.concatenate(w), np.concatenate(c)


def _camera_args(world, mode, scale):
    K = world["ixt"]
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 0], world["W"], world["H"], 1.0, 100.0, mode, scale,
            KNN_SCALE_DOWN)


def _shipped_rows(world, q, colours, radius_in, mode, scale):
    """sc_point_project on float32 points -> numpy radii, means2d, depths, records."""
    from street_crafter_amd import _lib, isect
    lib = _lib.load()
    N = q.shape[0]
    view, _ = LR.centred_camera(world["c2w"])
    d_q, d_c, d_v = torch.from_numpy(q).cuda(), torch.from_numpy(colours).cuda(), torch.from_numpy(view).cuda()
    d_r = None if radius_in is None else torch.from_numpy(radius_in).cuda()
    radii = torch.zeros(N, dtype=torch.int32, device="cuda")
    means2d, depths = torch.zeros((N, 2), device="cuda"), torch.zeros(N, device="cuda")
    records = torch.zeros((N, 8), device="cuda")
    fx, fy, cx, cy, focal, W, H, near, far, mode, scale, ksd = _camera_args(world, mode, scale)
    _lib.check(lib.sc_point_project(d_q.data_ptr(), d_c.data_ptr(), None, 1.0, None if d_r is None else d_r.data_ptr(),
                                    N, d_v.data_ptr(), fx, fy, cx, cy, focal, W, H, near, far, mode, scale, ksd,
                                    radii.data_ptr(), means2d.data_ptr(), depths.data_ptr(), records.data_ptr(),
                                    isect._stream(radii)), "sc_point_project")
    return radii.cpu().numpy(), means2d.cpu().numpy(), depths.cpu().numpy(), records.cpu().numpy()


def _fused_rows(world, seg, poses, N, radius_in, mode, scale, filt, want_world, project=True):
    """sc_point_assemble_project through the C entry, outputs in a guarded arena."""
    from street_crafter_amd import _lib, isect
    from street_crafter_amd.lidar_sequence import HEADER_WORDS
    lib = _lib.load()
    view, origin = LR.centred_camera(world["c2w"])
    head = np.zeros(HEADER_WORDS + 12 * poses.shape[0])
    head[0:16] = view.reshape(16)
    head[16:19] = origin
    head[20:32] = np.linalg.inv(world["c2w"])[:3].reshape(12)
    head[32:41] = world["ixt"].reshape(9)
    head[HEADER_WORDS:] = poses.reshape(-1)
    block = np.concatenate([head.view(np.uint8), seg.view(np.uint8)])
    d_block = torch.from_numpy(block).cuda()
    d_r = None if radius_in is None else torch.from_numpy(radius_in).cuda()
    ar = Arena({"radii": 4 * N, "means2d": 8 * N, "depths": 4 * N, "records": 32 * N, "world": 12 * N})
    fx, fy, cx, cy, focal, W, H, near, far, mode, scale, ksd = _camera_args(world, mode, scale)
    outs = [ar.ptr(k) if project else None for k in ("radii", "means2d", "depths", "records")]
    _lib.check(lib.sc_point_assemble_project(
        world["d_xyz"].data_ptr(), world["d_rgb"].data_ptr(), world["xyz"].shape[0], block.ctypes.data,
        d_block.data_ptr(), len(seg), poses.shape[0], N, int(filt), 1.0, None if d_r is None else d_r.data_ptr(), fx, fy,
        cx, cy, focal, W, H, near, far, mode, scale, ksd, *outs, ar.ptr("world") if want_world else None,
        isect._stream(d_block)), "sc_point_assemble_project")
    torch.cuda.synchronize()
    assert ar.broken_guards() == []
    return (ar.view("radii", torch.int32).cpu().numpy(), ar.view("means2d", torch.float32).cpu().numpy().reshape(N, 2),
            ar.view("depths", torch.float32).cpu().numpy(), ar.view("records", torch.float32).cpu().numpy().reshape(N, 8),
            ar.view("world", torch.float32).cpu().numpy().reshape(N, 3), ar)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("mode_name", list(MODES))
@pytest.mark.parametrize("case", CASES)
def test_rows_equal_shipped_projection(world, case, mode_name):
    mode, scale = MODES[mode_name]
    rng = np.random.default_rng(CASES.index(case))
    counts = _segment_cases()[case]
    seg, poses, N = _table(counts, world["xyz"].shape[0], rng)
    assert N == sum(counts)
    if case == "edges":
        assert N % 256 != 0 and len(poses) == 4
    if case == "beyond_lds":
        assert len(seg) == _lds_capacity() + 1
    w, colours = _expected_inputs(world, seg, poses)
    q = LR.camera_centred(w, world["c2w"])
    # (at least one entry: an empty tensor has no address, and mode 2 without an array is an argument error)
    radius_in = rng.uniform(1e-4, 4.0, max(N, 1)).astype(np.float32) if mode == 2 else None
    want = _shipped_rows(world, q, colours, radius_in, mode, scale)
    if N:
        assert (want[0] > 0).any()
    # filter off: every row; points_world alongside
    got = _fused_rows(world, seg, poses, N, radius_in, mode, scale, False, True)
    for g, x, what in zip(got[:4], want, ("radii", "means2d", "depths", "records")):
        assert _same_bits(g, x), what
    assert _same_bits(got[4], w.astype(np.float32))
    # filter on: dropped rows are all zero, kept rows unchanged; points_world not asked for and not written
    mask = LR.visible_mask(w, world["c2w"], world["ixt"], world["H"], world["W"])
    if N > 100:
        assert 0 < mask.sum() < N
    got = _fused_rows(world, seg, poses, N, radius_in, mode, scale, True, False)
    for g, x, what in zip(got[:4], want, ("radii", "means2d", "depths", "records")):
        x = x.copy()
        x[~mask] = 0
        assert _same_bits(g, x), what
    assert bool((got[5].view("world") == 0xA5).all())
    # points_world alone (the knn radius rule's first launch): nothing else is touched
    got = _fused_rows(world, seg, poses, N, None, 0, scale, False, True, project=False)
    assert _same_bits(got[4], w.astype(np.float32))
    for k in ("radii", "means2d", "depths", "records"):
        assert bool((got[5].view(k) == 0xA5).all())


# ---- the public calls ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def logs():
    from street_crafter_amd.lidar_sequence import LidarSequence
    out = {}
    for name, log in (("random", LR.random_log(11)), ("dyadic", LR.dyadic_log())):
        log["seq"] = LidarSequence(log["ply"])
        out[name] = log
    return out


def _frame_args(log, frame):
    return (log["track_info"][frame], log["ego"], log["ego"][frame], frame, log["ext"], log["ixt"], log["H"], log["W"])


def _restated_frame(log, frame, delta, shift):
    """The shipped pipeline fed the element-wise assembly and the restated filter -> uint8 rgb, mask."""
    from street_crafter_amd import lidar_condition as lc
    from street_crafter_amd.point_render import render_points_hip
    plan = log["seq"].plan_offline(log["track_info"][frame], log["ego"][frame], frame, log["F"], delta, shift)
    w, rgb = LR.assemble(log["ply"], plan)
    c2w = lc.shifted_camera(log["ego"][frame], log["ego"], frame, log["ext"], shift)
    m = LR.visible_mask(w, c2w, log["ixt"], log["H"], log["W"])
    r = render_points_hip(c2w, log["ixt"], w[m], rgb[m], log["H"], log["W"], use_ndc_scale=True, scale=0.01)
    r = r.cpu().numpy()
    return (r[0, ..., :3] * 255).astype(np.uint8), (r[0, ..., 3] * 255).astype(np.uint8)


@pytest.mark.parametrize("shift", [0.0, 2.0])
def test_frame_equals_shipped_pipeline_on_the_random_log(logs, shift):
    from street_crafter_amd.point_render import render_condition_frame_resident
    log = logs["random"]
    for frame in (0, 4):
        rgb, mask = render_condition_frame_resident(log["seq"], *_frame_args(log, frame), delta_frames=3, shift=shift)
        want_rgb, want_mask = _restated_frame(log, frame, 3, shift)
        assert rgb.dtype == np.uint8 and rgb.shape == (log["H"], log["W"], 3) and mask.shape == (log["H"], log["W"])
        assert (want_mask == 255).any() and (want_mask == 0).any()
        assert np.array_equal(mask, want_mask)
        assert np.array_equal(rgb, want_rgb)


@pytest.mark.parametrize("shift", [0.0, 2.0])
def test_frame_equals_host_route_on_the_dyadic_log(logs, shift):
    from street_crafter_amd.point_render import render_condition_frame_hip, render_condition_frame_resident
    log = logs["dyadic"]
    for frame in (0, 3):
        rgb, mask = render_condition_frame_resident(log["seq"], *_frame_args(log, frame), delta_frames=2, shift=shift)
        want_rgb, want_mask = render_condition_frame_hip(log["ply"], *_frame_args(log, frame), delta_frames=2,
                                                         shift=shift)
        assert (want_mask == 255).any() and (want_mask == 0).any()
        assert np.array_equal(mask, want_mask)
        assert np.array_equal(rgb, want_rgb)


TRAINING = {
    "ndc": dict(use_ndc_scale=True, scale=0.01),
    "const": dict(use_ndc_scale=False, scale=0.05, bg=np.array([0.25, 0.5, 0.75], np.float32)),
    "knn": dict(use_ndc_scale=False, use_knn_scale=True, scale=0.08, knn_scale_down=KNN_SCALE_DOWN),
    "translucent": dict(use_ndc_scale=False, scale=0.3, occ=0.4, max_hit=3),
    "depth": dict(use_ndc_scale=True, scale=0.02, return_depth=True),
}


@pytest.mark.parametrize("name", list(TRAINING))
def test_training_form_equals_render_points_hip(logs, name):
    from street_crafter_amd.point_render import render_points_hip
    log, frame, kw = logs["random"], 4, TRAINING[name]
    seq = log["seq"]
    plan = seq.plan_training(LR.actor_poses(log, frame), 2, 6)
    assert len(plan.tracks) > 3
    c2w = log["ego"][frame] @ log["ext"]
    got = seq.render_condition(c2w, log["ixt"], log["H"], log["W"], plan, **kw)
    w, rgb = LR.assemble(log["ply"], plan)
    want = render_points_hip(c2w, log["ixt"], w, rgb, log["H"], log["W"], **kw)
    if kw.get("return_depth"):
        assert torch.equal(got[1], want[1]) and bool((want[1] > 0).any())
        got, want = got[0], want[0]
    assert got.shape == (1, log["H"], log["W"], 4) and got.dtype == torch.float32 and got.is_cuda
    assert bool((want[..., 3] > 0).any()) and bool((want[..., 3] == 0).any())
    if name == "translucent":                                              # the hit cap is reached somewhere
        assert bool(torch.isclose(want[..., 3], torch.tensor(1 - 0.6 ** 3, device="cuda")).any())
    assert torch.equal(got, want)
    if name == "knn":
        with pytest.raises(NotImplementedError):
            seq.render_condition(c2w, log["ixt"], log["H"], log["W"], plan, visible_filter=True, **kw)


def test_listed_first_owns_a_depth_tie(logs):
    log, frame = logs["dyadic"], 2
    seq = log["seq"]
    poses = LR.actor_poses(log, frame)
    c2w = log["ego"][frame] @ log["ext"]
    x, y = LR.TIE_PIXEL
    plan = seq.plan_training(poses, 1, 3)
    assert plan.tracks.index("tie_a") < plan.tracks.index("tie_b")
    img = seq.render_condition(c2w, log["ixt"], log["H"], log["W"], plan)
    assert img[0, y, x].tolist() == [*LR.TIE_A_RGB, 1.0]
    back = seq.plan_training(poses, 1, 3, order=list(reversed(plan.tracks[1:])))
    assert back.tracks.index("tie_b") < back.tracks.index("tie_a")
    img = seq.render_condition(c2w, log["ixt"], log["H"], log["W"], back)
    assert img[0, y, x].tolist() == [*LR.TIE_B_RGB, 1.0]


def test_alternating_frames_repeat_their_first_result(logs):
    from street_crafter_amd.point_render import render_condition_frame_resident
    log = logs["random"]
    seq = log["seq"]
    frames = {"a": dict(frame=0, delta_frames=1, shift=0.0), "b": dict(frame=6, delta_frames=3, shift=2.0)}
    plans = {k: seq.plan_offline(log["track_info"][f["frame"]], log["ego"][f["frame"]], f["frame"], log["F"],
                                 f["delta_frames"], f["shift"]) for k, f in frames.items()}
    assert plans["a"].n_points != plans["b"].n_points and len(plans["a"].tracks) != len(plans["b"].tracks)
    first = {}
    for _ in range(3):
        for k, f in frames.items():
            rgb, mask = render_condition_frame_resident(seq, *_frame_args(log, f["frame"]),
                                                        delta_frames=f["delta_frames"], shift=f["shift"])
            if k not in first:
                first[k] = (rgb.copy(), mask.copy())
            assert np.array_equal(rgb, first[k][0]) and np.array_equal(mask, first[k][1]), k
    assert not np.array_equal(first["a"][1], first["b"][1])
