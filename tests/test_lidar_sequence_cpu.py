"""No-GPU checks of the resident LiDAR sequence (street_crafter_amd/lidar_sequence.py, csrc/point_assemble.hip): the
packing and the plans against lidar_condition's host route, the element-wise restatements of tests/lidar_sequence_ref.py
against that route (which pins the inputs the GPU tests compare on), and the entry point's argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lidar_sequence_ref as LR
from street_crafter_amd import lidar_condition as lc
from street_crafter_amd.lidar_sequence import HEADER_WORDS, SEGMENT_DTYPE, LidarSequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (11, 12, 13, 14)
FRAMES = (0, 3, 7)


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def logs():
    return {"random": LR.random_log(SEEDS[0]), "dyadic": LR.dyadic_log()}


def _resident_host(ply, seq):
    """The resident arrays as the constructor lays them out, on the host (no device here)."""
    return np.concatenate([ply[t][int(f)] for t in seq.tracks for f in seq._table[t][0]], axis=0)


@pytest.mark.parametrize("name", ["random", "dyadic"])
def test_packing_equals_make_lidar_ply(logs, name):
    log = logs[name]
    ply = dict(log["ply"])
    ply["background_visible"] = {0: np.zeros((3, 6))}                      # ignored
    seq = LidarSequence(ply, upload=False)
    assert seq.tracks == tuple(log["ply"])
    res = _resident_host(log["ply"], seq)
    assert seq.n_resident == res.shape[0] == sum(a.shape[0] for t in log["ply"].values() for a in t.values())
    F = log["F"]
    for start, end in [(0, F - 1), (0, 0), (F - 1, F - 1), (2, 4), (1, F - 2), (3, 3)]:
        per_track = lc.make_lidar_ply(log["ply"], start, end)
        for t in seq.tracks:
            a, b = seq.window_range(t, start, end)
            if t in per_track:
                assert np.array_equal(res[a:b].view(np.uint64), per_track[t].view(np.uint64)), (t, start, end)
            else:
                assert a == b, (t, start, end)                              # an actor unseen in the whole window
    with pytest.raises(KeyError):
        seq.window_range("background", F - 1, F)                            # as make_lidar_ply: no such sweep


@pytest.mark.parametrize("name", ["random", "dyadic"])
@pytest.mark.parametrize("shift", [0.0, 2.0])
def test_plan_offline_reproduces_assemble_frame(logs, name, shift):
    log = logs[name]
    seq = LidarSequence(log["ply"], upload=False)
    for frame in range(log["F"]):
        info, ego = log["track_info"][frame], log["ego"][frame]
        plan = seq.plan_offline(info, ego, frame, log["F"], delta_frames=2, shift=shift)
        start, end = max(0, frame - 2), min(log["F"] - 1, frame + 2)
        assert plan.window == (start, end)
        per_track = lc.make_lidar_ply(log["ply"], start, end)
        want = ["background"] + [t for t in per_track if t != "background" and t in info]
        assert list(plan.tracks) == want                                    # skipped tracks, ply_dict order
        seg = plan.segments
        assert seg.dtype == SEGMENT_DTYPE and seg["pose"][0] == -1
        assert np.array_equal(seg["pose"][1:], np.arange(len(want) - 1))
        assert np.array_equal(seg["out_begin"], np.concatenate([[0], np.cumsum(seg["count"])[:-1]]))
        for k, t in enumerate(want[1:]):
            box = info[t]["lidar_box"] if shift != 0 or info[t]["camera_box"] is None else info[t]["camera_box"]
            assert np.array_equal(plan.poses[k], (ego @ lc.box_pose(box))[:3])
        cloud = lc.assemble_frame(log["ply"], info, ego, frame, log["F"], 2, shift)
        assert plan.n_points == cloud.shape[0] == int(seg["count"].sum())
        w, rgb = LR.assemble(log["ply"], plan)
        c2w = lc.shifted_camera(ego, log["ego"], frame, log["ext"], shift)
        assert np.array_equal(LR.camera_centred(w, c2w).view(np.uint32),
                              LR.camera_centred(cloud[:, :3], c2w).view(np.uint32))
        assert np.array_equal(rgb, cloud[:, 3:])
    if name == "random":                                                   # the camera box is used at shift 0 only
        assert any(i["camera_box"] is not None for fr in log["track_info"].values() for i in fr.values())


def test_plan_training_rules_and_order(logs):
    log = logs["random"]
    seq = LidarSequence(log["ply"], upload=False)
    frame = 4
    poses = LR.actor_poses(log, frame)
    poses.pop("veh_1")                                                     # the caller leaves an actor out
    plan = seq.plan_training(poses, 2, 6)
    per_track = lc.make_lidar_ply(log["ply"], 2, 6)
    want = ["background"] + [t for t in per_track if t in poses]
    assert list(plan.tracks) == want and "veh_1" not in plan.tracks
    for k, t in enumerate(want[1:]):
        assert np.array_equal(plan.poses[k], poses[t][:3])
        assert plan.segments["count"][k + 1] == per_track[t].shape[0]
    order = [t for t in reversed(want[1:])] + ["veh_1"]                     # a permutation; an id without a pose
    rev = seq.plan_training(poses, 2, 6, order=order)
    assert list(rev.tracks) == ["background"] + list(reversed(want[1:]))
    assert rev.n_points == plan.n_points
    assert np.array_equal(rev.poses, plan.poses[::-1])
    with pytest.raises(ValueError):
        seq.plan_training(poses, 2, 6, order=[want[1], want[1]])
    with pytest.raises(KeyError):
        seq.plan((2, 6), [("no_such_track", np.eye(4))])
    # a pose of None: the actor's points are taken as they are
    raw = seq.plan((2, 6), [(want[1], None)])
    assert list(raw.segments["pose"]) == [-1, -1] and raw.poses.shape == (0, 3, 4)
    # a window in which an actor has no sweep: no segment for it
    only = LidarSequence.from_counts({"background": {0: 5, 1: 5, 2: 5}, "a": {0: 3}, "b": {2: 4}})
    p = only.plan((1, 2), [("a", np.eye(4)), ("b", np.eye(4))])
    assert p.tracks == ("background", "b") and p.n_points == 14 and list(p.segments["src_begin"]) == [5, 18]


@pytest.mark.parametrize("seed", SEEDS)
def test_restated_filter_equals_filter_visible(seed):
    """Unconditional equality on these seeds: a property of the inputs (no point within an ulp of an image edge), which
    is what lets the GPU tests compare the kernel's filter against the restatement."""
    log = LR.random_log(seed, n_bg=22000, n_actor=600)
    seq = LidarSequence(log["ply"], upload=False)
    for frame in FRAMES:
        info, ego = log["track_info"][frame], log["ego"][frame]
        for shift in (0.0, 2.0):
            plan = seq.plan_offline(info, ego, frame, log["F"], shift=shift)
            assert 110_000 <= plan.n_points <= 200_000
            w, _ = LR.assemble(log["ply"], plan)
            c2w = lc.shifted_camera(ego, log["ego"], frame, log["ext"], shift)
            cloud = lc.assemble_frame(log["ply"], info, ego, frame, log["F"], 10, shift)
            kept_xyz, _ = lc.filter_visible(cloud[:, :3], cloud[:, 3:], c2w, log["ixt"], log["H"], log["W"])
            mask = LR.visible_mask(w, c2w, log["ixt"], log["H"], log["W"])
            assert 0 < mask.sum() < mask.size
            assert mask.sum() == kept_xyz.shape[0]
            assert np.array_equal(LR.camera_centred(w[mask], c2w), LR.camera_centred(kept_xyz, c2w))


def test_restated_filter_equals_filter_visible_on_the_small_logs(logs):
    """The logs the GPU tests render, every frame and both shifts."""
    for log in logs.values():
        seq = LidarSequence(log["ply"], upload=False)
        for frame in range(log["F"]):
            info, ego = log["track_info"][frame], log["ego"][frame]
            for shift in (0.0, 2.0):
                plan = seq.plan_offline(info, ego, frame, log["F"], shift=shift)
                w, _ = LR.assemble(log["ply"], plan)
                c2w = lc.shifted_camera(ego, log["ego"], frame, log["ext"], shift)
                cloud = lc.assemble_frame(log["ply"], info, ego, frame, log["F"], 10, shift)
                kept_xyz, _ = lc.filter_visible(cloud[:, :3], cloud[:, 3:], c2w, log["ixt"], log["H"], log["W"])
                mask = LR.visible_mask(w, c2w, log["ixt"], log["H"], log["W"])
                assert mask.sum() == kept_xyz.shape[0]
                assert np.array_equal(LR.camera_centred(w[mask], c2w), LR.camera_centred(kept_xyz, c2w))


def test_dyadic_log_is_exact(logs):
    """The dyadic log's premise: BLAS and the element-wise forms agree in float64, not only after the rounding."""
    log = logs["dyadic"]
    seq = LidarSequence(log["ply"], upload=False)
    for frame in range(log["F"]):
        plan = seq.plan_offline(log["track_info"][frame], log["ego"][frame], frame, log["F"])
        w, _ = LR.assemble(log["ply"], plan)
        cloud = lc.assemble_frame(log["ply"], log["track_info"][frame], log["ego"][frame], frame, log["F"])
        assert np.array_equal(w, cloud[:, :3])
        a, b = plan.tracks.index("tie_a"), plan.tracks.index("tie_b")
        assert a < b
        pa, pb = (w[int(plan.segments["out_begin"][k])] for k in (a, b))
        assert np.array_equal(pa, pb)                                       # the same world point, from two actors
        c2w = lc.shifted_camera(log["ego"][frame], log["ego"], frame, log["ext"])
        cam = np.linalg.inv(c2w) @ np.append(pa, 1.0)
        assert cam[2] == 4.0
        assert (64.0 * cam[0] / 4.0 + 96.0, 64.0 * cam[1] / 4.0 + 64.0) == (LR.TIE_PIXEL[0] + 0.5, LR.TIE_PIXEL[1] + 0.5)


# ---- the entry point -------------------------------------------------------------------------------------------------
NEW = ("sc_point_assemble_project", "sc_point_assemble_lds_segments")


def test_entry_point_declared_exported_and_bound(lib):
    from street_crafter_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "street_crafter_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", src), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert "point_assemble.hip" in build.SOURCES
    assert lib.sc_point_assemble_lds_segments() >= 64
    assert ctypes.sizeof(ctypes.c_int64) * 3 == SEGMENT_DTYPE.itemsize == 24
    assert int(re.search(r"#define\s+SC_POINT_FRAME_HEADER_WORDS\s+(\d+)", src).group(1)) == HEADER_WORDS
    from street_crafter_amd import point_render
    assert point_render.LidarSequence is LidarSequence
    assert "render_condition_frame_resident" in point_render.__all__


def _block(segments, n_poses=1):
    """A host frame block: zero header and poses, then the segments (src_begin, out_begin, count, pose)."""
    seg = np.zeros(len(segments), dtype=SEGMENT_DTYPE)
    for k, (a, o, n, p) in enumerate(segments):
        seg[k] = (a, o, n, p, 0)
    buf = np.concatenate([np.zeros(8 * (HEADER_WORDS + 12 * n_poses), np.uint8), seg.view(np.uint8)])
    return buf


def _assemble(lib, segments=((0, 0, 4, -1),), N=4, n_poses=1, n_resident=100, ptr=0x10000, host="block", occ=1.0,
              mode=0, radius_in=None, width=64, height=48, focal=100.0, scale=0.01, filt=0, outs=None, world=None,
              n_segments=None, dev=None):
    buf = _block(segments, max(n_poses, 0))
    host_ptr = buf.ctypes.data if host == "block" else host
    outs = (ptr, ptr, ptr, ptr) if outs is None else outs
    rc = lib.sc_point_assemble_project(ptr, ptr, n_resident, host_ptr, ptr if dev is None else dev,
                                       len(segments) if n_segments is None else n_segments, n_poses, N, filt, occ,
                                       radius_in, 100.0, 100.0, 32.0, 24.0, focal, width, height, 1.0, 100.0, mode,
                                       scale, 1.0, *outs, world, None)
    del buf
    return rc


def test_entry_point_refuses_bad_arguments_before_launching(lib):
    # `ptr` is a non-null address that is never dereferenced: every call below is answered on the host
    fake = 0x10000
    assert _assemble(lib, ptr=None) == -1                                          # null pointers
    assert _assemble(lib, N=-1) == -1
    assert _assemble(lib, n_poses=-1) == -1
    assert _assemble(lib, n_resident=-1) == -1
    assert _assemble(lib, n_segments=-1) == -1
    assert _assemble(lib, segments=((0, 0, -1, -1), (0, -1, 5, -1))) == -1         # a negative count
    assert _assemble(lib, segments=((0, 0, 3, -1),)) == -1                         # ranges that stop short of N
    assert _assemble(lib, segments=((0, 0, 5, -1),)) == -1                         # ... or run past it
    assert _assemble(lib, segments=((0, 1, 4, -1),), N=5) == -1                    # ... or do not start at 0
    assert _assemble(lib, segments=((0, 0, 2, -1), (9, 3, 1, -1)), N=4) == -1      # a gap
    assert _assemble(lib, segments=((0, 0, 2, -1), (9, 1, 2, -1)), N=4) == -1      # an overlap
    assert _assemble(lib, segments=((0, 2, 2, -1), (9, 0, 2, -1)), N=4) == -1      # out of order
    assert _assemble(lib, segments=((0, 0, 4, 1),)) == -1                          # a pose slot out of range
    assert _assemble(lib, segments=((0, 0, 4, -2),)) == -1
    assert _assemble(lib, segments=((0, 0, 4, 0),), n_poses=0) == -1
    assert _assemble(lib, segments=((97, 0, 4, -1),)) == -1                        # past the resident rows
    assert _assemble(lib, segments=((-1, 0, 4, -1),)) == -1
    assert _assemble(lib, host=None) == -1                                         # a table nobody can check
    assert _assemble(lib, filt=2) == -1
    assert _assemble(lib, occ=0.0) == -1                                           # what sc_point_project refuses
    assert _assemble(lib, occ=1.5) == -1
    assert _assemble(lib, occ=float("nan")) == -1
    assert _assemble(lib, mode=3) == -1                                            # the fused route has modes 0..2
    assert _assemble(lib, mode=-1) == -1
    assert _assemble(lib, mode=2) == -1                                            # knn mode without distances
    assert _assemble(lib, width=0) == -1
    assert _assemble(lib, height=0) == -1
    assert _assemble(lib, focal=0.0) == -1
    assert _assemble(lib, scale=-1.0) == -1
    assert _assemble(lib, outs=(fake, fake, fake, None)) == -1                     # some of the four outputs
    assert _assemble(lib, outs=(None,) * 4) == -1                                  # nothing to write at all
    assert _assemble(lib, outs=(fake, fake, fake, fake + 4)) == -1                 # records not 16-B aligned
    assert _assemble(lib, dev=fake + 4) == -1                                      # block not 8-B aligned
    # nothing to do: no launch, no device pointer read -- with a table of empty segments or none at all
    assert _assemble(lib, segments=((0, 0, 0, -1), (5, 0, 0, 0)), N=0, ptr=None) == 0
    assert _assemble(lib, segments=(), N=0, ptr=None, host=None) == 0
    assert _assemble(lib, segments=(), N=1) == -1


def test_cpu_devices_and_oversized_frames_are_refused(logs):
    from street_crafter_amd.point_render import render_condition_frame_resident
    log = logs["random"]
    with pytest.raises(RuntimeError, match="HIP device"):
        LidarSequence(log["ply"], device="cpu")
    as_tensors = {t: {f: torch.from_numpy(a) for f, a in fr.items()} for t, fr in log["ply"].items()}
    with pytest.raises(RuntimeError, match="HIP device"):
        LidarSequence(as_tensors)
    seq = LidarSequence(log["ply"], upload=False)                               # a table without points
    plan = seq.plan_offline(log["track_info"][0], log["ego"][0], 0, log["F"])
    with pytest.raises(RuntimeError, match="HIP device"):
        seq.render_condition(log["ego"][0] @ log["ext"], log["ixt"], log["H"], log["W"], plan)
    with pytest.raises(RuntimeError, match="HIP device"):
        render_condition_frame_resident(seq, log["track_info"][0], log["ego"], log["ego"][0], 0, log["ext"],
                                        log["ixt"], log["H"], log["W"])
    with pytest.raises(TypeError):
        render_condition_frame_resident(log["ply"], log["track_info"][0], log["ego"], log["ego"][0], 0, log["ext"],
                                        log["ixt"], log["H"], log["W"])
    # 2^31 - 1 points fit the int32 point index, one more does not: decided on the table alone
    big = LidarSequence.from_counts({"background": {0: 2 ** 30, 1: 2 ** 30 - 1, 2: 1}, "a": {1: 7}})
    assert big.n_resident == 2 ** 31 + 7
    assert big.plan((0, 1), []).n_points == 2 ** 31 - 1
    with pytest.raises(ValueError, match="int32"):
        big.plan((0, 2), [])
    with pytest.raises(ValueError, match="int32"):
        big.plan((0, 1), [("a", np.eye(4))])
    far = big.plan((2, 2), [("a", None)])                                       # resident indices are int64
    assert far.n_points == 1 and far.segments["src_begin"][0] == 2 ** 31 - 1


def test_new_module_never_imports_oracle():
    src = open(os.path.join(ROOT, "street_crafter_amd", "lidar_sequence.py")).read()
    assert "oracle" not in re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, flags=re.M)
