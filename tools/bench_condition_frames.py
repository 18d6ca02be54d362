"""A/B of the two condition-frame routes on the demo log of tools/bench_point_render.py (21 sweeps x 150 k points + 4
tracked vehicles, 1920x1280, frame 10 +- 10 sweeps: 3.2 M points), in one process:

    A  point_render.render_condition_frame_hip        frame assembly and visibility filter in numpy, upload, GPU render
    B  lidar_sequence.render_condition_frame_resident sweeps resident, assembly + filter + projection in one launch

    python tools/bench_condition_frames.py [--frames-hip 4] [--frames-resident 30] [--kernel-reps 30] [--out FILE]

Wall clock per condition frame (time.perf_counter around a call that ends in the image's download, so the device has
finished): A before, B, A again -- the second A run shows whether the machine drifted.  Then the HIP-event time of
sc_point_assemble_project alone (filter on, as B launches it) against sc_point_project alone on the frame's filtered
float32 points (as A launches it), alternating.  Every timed shape is warmed up first.  The one-off upload of the
sequence is reported separately.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402


def _stats(ts):
    ts = np.asarray(ts) * 1e3
    return f"median {np.median(ts):9.3f} ms   p10 {np.percentile(ts, 10):9.3f}   p90 {np.percentile(ts, 90):9.3f}   n {len(ts)}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-hip", type=int, default=4)
    ap.add_argument("--frames-resident", type=int, default=30)
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--ppf", type=int, default=150_000, help="points per sweep")
    ap.add_argument("--out", default=None, help="file the report is written to as well")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_condition_frames needs a GPU")
    from bench_point_render import demo_log
    from street_crafter_amd import _lib, lidar_condition as lc, point_render as pr, rendering as R
    from street_crafter_amd.lidar_sequence import LidarSequence, render_condition_frame_resident

    log = demo_log(args.ppf)
    ply, track, ego, ext, ixt, H, W, frame = (log[k] for k in ("ply", "track", "ego", "ext", "ixt", "H", "W", "frame"))
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def route_a():
        return pr.render_condition_frame_hip(ply, track, ego, ego[frame], frame, ext, ixt, H, W)

    t0 = time.perf_counter()
    seq = LidarSequence(ply)
    torch.cuda.synchronize()
    t_upload = time.perf_counter() - t0

    def route_b():
        return render_condition_frame_resident(seq, track, ego, ego[frame], frame, ext, ixt, H, W)

    def wall(fn, n):
        ts = []
        for _ in range(n):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return ts

    a, b = route_a(), route_b()                      # warm-up of both routes, and the comparison of their images
    route_b()
    plan = seq.plan_offline(track, ego[frame], frame, len(ego))
    say(f"demo log: {seq.n_resident} resident points, frame {frame}: N = {plan.n_points} assembled points, "
        f"{len(plan.tracks)} segments, image {W}x{H}")
    say(f"images A vs B: rgb differs in {int((a[0] != b[0]).any(-1).sum())} pixels, mask in {int((a[1] != b[1]).sum())} "
        f"of {H * W} (A assembles through BLAS, B element by element: last-bit differences of float64 coordinates)")
    say(f"one-off upload of the sequence (LidarSequence(ply_dict)): {t_upload * 1e3:.1f} ms")
    say("wall clock per condition frame, download included:")
    say(f"  A render_condition_frame_hip       (before)  {_stats(wall(route_a, args.frames_hip))}")
    say(f"  B render_condition_frame_resident            {_stats(wall(route_b, args.frames_resident))}")
    say(f"  A render_condition_frame_hip       (after)   {_stats(wall(route_a, args.frames_hip))}")

    # ---- the projection kernels alone ---------------------------------------------------------------------------
    lib = _lib.load()
    dev = seq.device
    c2w = lc.shifted_camera(ego[frame], ego, frame, ext)
    cloud = lc.assemble_frame(ply, track, ego[frame], frame, len(ego))
    xyz, feat = lc.filter_visible(cloud[:, :3], cloud[:, 3:], c2w, ixt, H, W)
    origin = c2w[:3, 3].copy()
    w2c = np.linalg.inv(c2w)
    view = w2c.copy()
    view[:3, 3] += view[:3, :3] @ origin
    pts = torch.from_numpy((xyz - origin).astype(np.float32)).to(dev)
    cols = torch.from_numpy(np.ascontiguousarray(feat[:, :3], dtype=np.float32)).to(dev)
    vm = torch.from_numpy(view).to(dev)
    st = R._stream(pts)
    fx, fy, cx, cy = ixt[0, 0], ixt[1, 1], ixt[0, 2], ixt[1, 2]

    def outputs(n):
        return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), device=dev),
                torch.empty(n, device=dev), torch.empty((n, 8), device=dev))
    out_a, out_b = outputs(pts.shape[0]), outputs(plan.n_points)
    blocks = seq._send_block(plan, view, origin, w2c[:3, :4], ixt)

    def kernel_a():
        _lib.check(lib.sc_point_project(R._p(pts), R._p(cols), None, 1.0, None, pts.shape[0], R._p(vm), fx, fy, cx, cy,
                                        fx, W, H, 1.0, 100.0, pr.RADIUS_NDC, 0.01, 1.0, *(R._p(t) for t in out_a), st),
                   "sc_point_project")

    def kernel_b():
        seq._launch(plan, blocks, True, 1.0, None, fx, fy, cx, cy, fx, W, H, 1.0, 100.0, pr.RADIUS_NDC, 0.01, 1.0,
                    *out_b, None, st)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3
    for _ in range(5):
        kernel_a(), kernel_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.kernel_reps):
        ta.append(events(kernel_a))
        tb.append(events(kernel_b))
    bytes_a = pts.shape[0] * (12 + 12 + 48)
    bytes_b = plan.n_points * (24 + 12 + 48)
    say("projection kernels alone, HIP events around one launch:")
    say(f"  A sc_point_project          on {pts.shape[0]:8d} filtered points  {_stats(ta)}   "
        f"{bytes_a / np.median(ta) / 1e9:8.1f} GB/s of {bytes_a / 1e6:.1f} MB")
    say(f"  B sc_point_assemble_project on {plan.n_points:8d} resident points  {_stats(tb)}   "
        f"{bytes_b / np.median(tb) / 1e9:8.1f} GB/s of {bytes_b / 1e6:.1f} MB")
    say("(bytes: xyz + rgb read, radii + means2d + depths + records written, computed from the shapes)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
