"""Resident LiDAR sequence: the sweeps of a log are uploaded once and every condition frame is assembled on the GPU
(csrc/point_assemble.hip, `sc_point_assemble_project`), in front of the shipped point-render pipeline.

What the reference does per frame x camera x shift on the host (data_processor/waymo_processor/
waymo_render_lidar_pcd.py:207-267) and per novel-view camera at every diffusion sampling iteration
(WaymoPointCloudProcessor.render_condition, street_gaussian/pointcloud_processor/waymo_processor.py:178-242) --
concatenate the sweeps of frame +- delta, push every actor's points through its pose, filter by visibility, move to
the camera centre -- happens here in one launch over points that never leave the device.  Between frames only the
window, the actor poses and the camera change: a frame costs one small pinned host-to-device copy (the segment
table, the 3x4 poses and the camera; a few kilobytes).

    seq = LidarSequence(ply_dict)                               # once per log
    rgb, mask = render_condition_frame_resident(seq, ...)       # the offline script's frame loop
    img = seq.render_condition(c2w, ixt, h, w, seq.plan_training(poses, start, end))     # the training-time call

Layout: tracks in `ply_dict` order (background first), each track's frames contiguous in ascending frame order, so the
window [start, end] of a track is ONE range of resident rows, bit for bit what lidar_condition.make_lidar_ply
concatenates.  xyz stays float64 on the device (Waymo world coordinates sit kilometres from the origin; the camera
origin is subtracted in float64 before the rounding to float32, as point_render.render_points_hip does for host
arrays), rgb is float32.  Everything behind the projection is point_render's pipeline, unchanged.  No CPU path.

One host thread per LidarSequence: the pinned staging block is the sequence's own.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import lidar_condition as _lc
from . import point_render as _pr
from . import rendering as _r

__all__ = ["LidarSequence", "FramePlan", "render_condition_frame_resident"]

# sc_point_segment and the frame block of include/street_crafter_amd.h
SEGMENT_DTYPE = np.dtype(_lib.PointSegment)
HEADER_WORDS = _lib.CONSTANTS["SC_POINT_FRAME_HEADER_WORDS"]
_HDR_VIEW, _HDR_ORIGIN, _HDR_FILT_M, _HDR_FILT_K = 0, 16, 20, 32
INT32_MAX = 0x7fffffff


@dataclass(frozen=True)
class FramePlan:
    """One frame's assembly, host side only.  segments: SEGMENT_DTYPE [S] (resident begin, output begin, count, pose
    slot; -1 = no pose), background first, then the actors in the order given; poses: float64 [A,3,4]; n_points: N;
    tracks: the track id of every segment; window: (start_frame, end_frame); camera: whatever the caller attached."""
    segments: np.ndarray
    poses: np.ndarray
    n_points: int
    tracks: Tuple[str, ...]
    window: Tuple[int, int]
    camera: object = None


class LidarSequence:
    """`ply_dict` = {"background": {frame: [n,6]}, track_id: {frame: [n,6]}} (xyz + rgb, the shape
    lidar_condition.make_lidar_ply reads; a "background_visible" entry is ignored), uploaded once to `device` (default:
    the current HIP device).  `upload=False` keeps only the host-side table: the plans work, the renders do not."""

    def __init__(self, ply_dict: Dict[str, Dict[int, np.ndarray]], device=None, upload: bool = True):
        if "background" not in ply_dict:
            raise KeyError("ply_dict has no 'background' entry")
        tracks = [t for t in ply_dict if t != "background_visible"]
        self._set_table({t: {int(f): int(np.shape(ply_dict[t][f])[0]) for f in ply_dict[t]} for t in tracks})
        self.device = None
        self.xyz = self.rgb = None
        self._stage = self._stage_event = None
        if not upload:
            return
        for t in tracks:
            for f, a in ply_dict[t].items():
                if isinstance(a, torch.Tensor):
                    raise RuntimeError(f"ply_dict[{t!r}][{f}] is a torch tensor on {a.device}: the sweeps are numpy "
                                       "[n,6] arrays and go to a HIP device here; street_crafter_amd has no CPU path")
        self.device = _pr._device(device)
        M = self.n_resident
        self.xyz = torch.empty((M, 3), dtype=torch.float64, device=self.device)
        self.rgb = torch.empty((M, 3), dtype=torch.float32, device=self.device)
        for t in tracks:
            frames, begins = self._table[t]
            if begins[-1] == begins[0]:
                continue
            cloud = np.concatenate([np.asarray(ply_dict[t][int(f)], dtype=np.float64).reshape(-1, 6) for f in frames],
                                   axis=0)
            a, b = int(begins[0]), int(begins[-1])
            self.xyz[a:b] = torch.from_numpy(np.ascontiguousarray(cloud[:, :3]))
            self.rgb[a:b] = torch.from_numpy(np.ascontiguousarray(cloud[:, 3:6], dtype=np.float32))

    @classmethod
    def from_counts(cls, counts: Dict[str, Dict[int, int]]) -> "LidarSequence":
        """A table-only sequence from {track: {frame: point count}}: nothing is allocated; plans only."""
        self = cls.__new__(cls)
        if "background" not in counts:
            raise KeyError("counts has no 'background' entry")
        self._set_table({t: {int(f): int(n) for f, n in fr.items()} for t, fr in counts.items()
                         if t != "background_visible"})
        self.device = None
        self.xyz = self.rgb = None
        self._stage = self._stage_event = None
        return self

    # ---- the host table: (track, frame) -> [begin, end) of resident rows (int64) -------------------------------------
    def _set_table(self, counts: Dict[str, Dict[int, int]]):
        self.tracks = ("background",) + tuple(t for t in counts if t != "background")
        self._table = {}
        at = 0
        for t in self.tracks:
            frames = np.array(sorted(counts[t]), dtype=np.int64)
            n = np.array([counts[t][int(f)] for f in frames], dtype=np.int64)
            if (n < 0).any():
                raise ValueError(f"negative point count in track {t!r}")
            begins = at + np.concatenate([np.zeros(1, np.int64), np.cumsum(n, dtype=np.int64)])
            self._table[t] = (frames, begins)
            at = int(begins[-1])
        self.n_resident = at

    def window_range(self, track: str, start_frame: int, end_frame: int) -> Tuple[int, int]:
        """[begin, end) of the track's sweeps of frames start..end (inclusive): the rows make_lidar_ply concatenates.
        The background must have every frame of the window (KeyError otherwise, as make_lidar_ply)."""
        frames, begins = self._table[track]
        k0 = int(np.searchsorted(frames, start_frame, side="left"))
        k1 = int(np.searchsorted(frames, end_frame, side="right"))
        if track == "background" and end_frame >= start_frame and k1 - k0 != end_frame - start_frame + 1:
            have = set(int(f) for f in frames[k0:k1])
            raise KeyError(next(f for f in range(start_frame, end_frame + 1) if f not in have))
        k1 = max(k1, k0)
        return int(begins[k0]), int(begins[k1])

    # ---- plans (host only) -----------------------------------------------------------------------------------------
    def plan(self, window: Tuple[int, int], actors: Iterable[Tuple[str, Optional[np.ndarray]]], camera=None) -> FramePlan:
        """window = (start_frame, end_frame), inclusive; actors = ordered (track_id, 4x4 float64 pose | None).
        Background first, without a pose; then the actors in the order given.  An actor without a point in the window
        gets no segment (make_lidar_ply leaves it out too).  ValueError when the frame exceeds 2^31 - 1 points."""
        start, end = int(window[0]), int(window[1])
        rows, poses, names = [], [], []
        total = 0
        for track, pose in [("background", None), *actors]:
            if track not in self._table:
                raise KeyError(track)
            a, b = self.window_range(track, start, end)
            if b == a and track != "background":
                continue
            slot = -1
            if pose is not None:
                pose = np.asarray(pose, dtype=np.float64)
                if pose.shape not in ((4, 4), (3, 4)):
                    raise ValueError(f"pose of {track!r} must be 4x4 (or 3x4), got {pose.shape}")
                slot = len(poses)
                poses.append(pose[:3, :4])
            rows.append((a, total, b - a, slot))
            names.append(track)
            total += b - a
            if total > INT32_MAX:
                raise ValueError(f"the frame has more than {INT32_MAX} points (window {start}..{end}): the tile lists "
                                 "index points with int32")
        seg = np.zeros(len(rows), dtype=SEGMENT_DTYPE)
        for k, (a, o, n, slot) in enumerate(rows):
            seg[k] = (a, o, n, slot, 0)
        P = np.stack(poses).astype(np.float64) if poses else np.zeros((0, 3, 4), np.float64)
        return FramePlan(seg, np.ascontiguousarray(P), int(total), tuple(names), (start, end), camera)

    def plan_offline(self, track_info_frame: Dict[str, dict], ego_cam_pose: np.ndarray, frame: int, num_frames: int,
                     delta_frames: int = 10, shift: float = 0.0) -> FramePlan:
        """lidar_condition.assemble_frame's rules: the window frame +- delta clipped to the log; every track of the
        sequence, in its order, that is tracked in THIS frame; pose = ego_pose @ box_pose(box) with the camera box
        when present and the view is not shifted, the LiDAR box otherwise."""
        start, end = max(0, frame - delta_frames), min(num_frames - 1, frame + delta_frames)
        actors = []
        for track in self.tracks[1:]:
            if track not in track_info_frame:
                continue
            info = track_info_frame[track]
            if shift == 0:
                box = info["camera_box"] if info.get("camera_box") is not None else info["lidar_box"]
            else:
                box = info["lidar_box"]
            actors.append((track, ego_cam_pose @ _lc.box_pose(box)))
        return self.plan((start, end), actors)

    def plan_training(self, actor_poses: Dict[str, np.ndarray], start_frame: int, end_frame: int,
                      order: Optional[Sequence[str]] = None) -> FramePlan:
        """WaymoPointCloudProcessor.render_condition's rules: `actor_poses` = {track_id: camera.meta['ego_pose'] @
        pose_vehicle} for the actors alive and tracked in the camera's frame; the actors follow the background in the
        sequence's track order, or in `order` (cfg.diffusion.shuffle_actors: the caller's permutation of the track
        ids; ids without a pose are skipped, as the reference skips untracked actors)."""
        names = [t for t in self.tracks[1:]] if order is None else list(order)
        if order is not None and len(set(names)) != len(names):
            raise ValueError("order names a track twice")
        return self.plan((start_frame, end_frame), [(t, actor_poses[t]) for t in names if t in actor_poses])

    # ---- the device side -------------------------------------------------------------------------------------------
    def _need_device(self):
        if self.xyz is None:
            raise RuntimeError("this LidarSequence holds no points on a HIP device (built with upload=False or "
                               "from_counts); street_crafter_amd has no CPU path")

    def _send_block(self, plan: FramePlan, view: np.ndarray, origin: np.ndarray, filt_m: np.ndarray,
                    filt_k: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
        """Writes the frame block into the pinned staging buffer and copies it to the device on the current stream.
        -> (pinned block, device block)."""
        A, S = int(plan.poses.shape[0]), int(plan.segments.shape[0])
        head = 8 * (HEADER_WORDS + 12 * A)
        nbytes = head + SEGMENT_DTYPE.itemsize * S
        if self._stage_event is not None:
            # the previous frame's copy must have left the buffer (it has: the binning's count read-back followed it)
            self._stage_event.synchronize()
        if self._stage is None or self._stage.numel() < nbytes:
            self._stage = torch.empty(max(4096, 2 * nbytes), dtype=torch.uint8, pin_memory=True)
            self._stage_event = torch.cuda.Event()
        buf = self._stage.numpy()
        words = buf[:head].view(np.float64)
        words[:HEADER_WORDS] = 0.0
        words[_HDR_VIEW:_HDR_VIEW + 16] = np.asarray(view, np.float64).reshape(16)
        words[_HDR_ORIGIN:_HDR_ORIGIN + 3] = origin
        words[_HDR_FILT_M:_HDR_FILT_M + 12] = np.asarray(filt_m, np.float64).reshape(12)
        words[_HDR_FILT_K:_HDR_FILT_K + 9] = np.asarray(filt_k, np.float64).reshape(9)
        words[HEADER_WORDS:] = plan.poses.reshape(-1)
        buf[head:nbytes].view(SEGMENT_DTYPE)[:] = plan.segments
        block = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            block.copy_(self._stage[:nbytes], non_blocking=True)
            self._stage_event.record()
        return self._stage, block

    def _launch(self, plan: FramePlan, blocks, filt: bool, occ: float, radius_in, fx, fy, cx, cy, focal_r, W, H, near,
                far, mode, scale, knn_scale_down, radii, means2d, depths, records, points_world, st):
        host, dev = blocks
        lib = _lib.load()
        _lib.check(lib.sc_point_assemble_project(
            _r._p(self.xyz), _r._p(self.rgb), int(self.n_resident), host.data_ptr(), dev.data_ptr(),
            int(plan.segments.shape[0]), int(plan.poses.shape[0]), int(plan.n_points), int(bool(filt)), float(occ),
            _r._p(radius_in), float(fx), float(fy), float(cx), float(cy), float(focal_r), int(W), int(H), float(near),
            float(far), int(mode), float(scale), float(knn_scale_down), _r._p(radii), _r._p(means2d), _r._p(depths),
            _r._p(records), _r._p(points_world), st), "sc_point_assemble_project")

    @torch.no_grad()
    def render_condition(self, c2w, ixt, h: int, w: int, plan: FramePlan, scale: float = 0.01,
                         use_ndc_scale: bool = True, use_knn_scale: bool = False, knn_scale_down: float = 1.0,
                         occ: float = 1.0, max_hit: int = 10, near: float = 1.0, far: float = 100.0,
                         visible_filter: bool = False, bg=None, return_depth: bool = False):
        """`point_render.render_points_hip` on the cloud `plan` assembles: float32 [1,h,w,4] (rgb over `bg` + alpha) on
        the device, with return_depth also the depth [1,h,w].  visible_filter: lidar_condition.filter_visible in
        front of the render (the offline script); use_knn_scale (without use_ndc_scale): distCUDA2 of the assembled
        world points, on the device -- not together with the filter (the neighbour set would need a compaction)."""
        self._need_device()
        H, W = int(h), int(w)
        if H <= 0 or W <= 0:
            raise ValueError(f"image size must be positive, got {H}x{W}")
        if not 0.0 < float(occ) <= 1.0:
            raise ValueError(f"occ must lie in (0, 1], got {occ}")
        if int(max_hit) < 1:
            raise ValueError(f"max_hit must be >= 1, got {max_hit}")
        knn = bool(use_knn_scale) and not use_ndc_scale
        if knn and visible_filter:
            raise NotImplementedError("use_knn_scale with visible_filter: the nearest-neighbour set would need a "
                                      "compaction of the kept points")
        dev = self.device
        K = _pr._host64(ixt)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        c2w = _pr._host64(c2w)
        w2c = np.linalg.inv(c2w)
        # the points move to the camera centre in float64 before the float32 rounding; the camera transform follows
        # (the same two lines as render_points_hip's host-array branch)
        origin = c2w[:3, 3].copy()
        view = w2c.copy()
        view[:3, 3] += view[:3, :3] @ origin
        bg_t = None
        if bg is not None:
            bg_t = _pr._on(bg, dev, "bg").reshape(-1).contiguous()
            if bg_t.numel() != 3:
                raise ValueError(f"bg must have 3 entries, got {bg_t.numel()}")
        N = plan.n_points
        with torch.cuda.device(dev):
            st = _r._stream(self.xyz)
            mode, radius_in = _pr.RADIUS_CONST, None
            blocks = self._send_block(plan, view, origin, w2c[:3, :4], K[:3, :3]) if N else None
            if use_ndc_scale:
                mode = _pr.RADIUS_NDC
            elif knn and N:
                from .knn import distCUDA2
                mode = _pr.RADIUS_KNN
                world = torch.empty((N, 3), dtype=torch.float32, device=dev)
                self._launch(plan, blocks, False, occ, None, fx, fy, cx, cy, fx, W, H, near, far, _pr.RADIUS_CONST,
                             scale, knn_scale_down, None, None, None, None, world, st)
                radius_in = distCUDA2(world)

            def project(radii, means2d, depths, records):
                self._launch(plan, blocks, visible_filter, occ, radius_in, fx, fy, cx, cy, fx, W, H, near, far, mode,
                             scale, knn_scale_down, radii, means2d, depths, records, None, st)
            img, _, depth, _ = _pr._bin_and_blend(project, N, dev, st, H, W, int(max_hit), bg_t, planar=False,
                                                  want_depth=return_depth)
        return (img, depth) if return_depth else img


def render_condition_frame_resident(seq: LidarSequence, track_info_frame, ego_frame_poses, ego_cam_pose: np.ndarray,
                                    frame: int, extrinsic: np.ndarray, ixt: np.ndarray, h: int, w: int,
                                    delta_frames: int = 10, shift: float = 0.0, lane_shift_sign: float = 1.0
                                    ) -> Tuple[np.ndarray, np.ndarray]:
    """`point_render.render_condition_frame_hip` with `seq` in place of `ply_dict`: the frame assembly and the
    visibility filter run on the device, the image is quantised there and 4 bytes per pixel come back.
    -> (uint8 rgb [h,w,3], uint8 mask [h,w]), `(x * 255).astype(np.uint8)` for colours in [0, 1]."""
    if not isinstance(seq, LidarSequence):
        raise TypeError(f"seq must be a LidarSequence, got {type(seq)}")
    seq._need_device()
    plan = seq.plan_offline(track_info_frame, ego_cam_pose, frame, len(ego_frame_poses), delta_frames, shift)
    c2w = _lc.shifted_camera(ego_cam_pose, ego_frame_poses, frame, extrinsic, shift, lane_shift_sign)
    img = seq.render_condition(c2w, ixt, h, w, plan, scale=0.01, use_ndc_scale=True, visible_filter=True)
    h, w = int(h), int(w)
    with torch.cuda.device(seq.device):
        out = torch.empty(4 * h * w, dtype=torch.uint8, device=seq.device)
        _lib.check(_lib.load().sc_frame_composite_u8(img.data_ptr(), 4, None, None, 0, h * w, 0, out.data_ptr(),
                                                     _r._stream(img)), "sc_frame_composite_u8")
        out[3 * h * w:].view(h, w).copy_(img[0, ..., 3] * 255.0)
        host = out.cpu().numpy()
    return host[:3 * h * w].reshape(h, w, 3), host[3 * h * w:].reshape(h, w)
