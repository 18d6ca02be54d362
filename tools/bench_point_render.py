"""Times the LiDAR condition render on the GPU (street_crafter_amd/point_render.py) on the workload of
tools/lidar_condition_demo.py (same seed): 21 sweeps x 150 k points + 4 tracked vehicles, use_ndc_scale, scale 0.01,
at 1920x1280 and at the reference's training resolution 1600x1066 (intrinsics scaled), each both after
filter_visible (the offline script) and unfiltered (the training-time render_condition).

    python tools/bench_point_render.py [--frames 50] [--warmup 5] [--cpu] [--out DIR]

Per case: ms per condition frame (HIP events, median over --frames after --warmup), the split into project /
count+emit / radix sort / offsets / blend (events around each step of the same pipeline), intersections I, the
blend's compulsory bytes over HBM peak, and with --cpu one run of the numpy contract `render_points`.
Kernel names and times: run it under `rocprofv3 --kernel-trace --stats` separately (fewer frames suffice).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X spec


def demo_log(ppf: int = 150_000):
    """The log of tools/lidar_condition_demo.py, generated in the same order from the same seed.
    -> dict(ply, track (one frame's boxes, the same for every frame), ego [F], ext, ixt, H, W, F, frame)."""
    rng = np.random.default_rng(20250404)
    F, H, W = 21, 1280, 1920
    ego = []
    for f in range(F):
        p = np.eye(4)
        p[:3, 3] = [1.5 * f, 0.0, 0.0]
        ego.append(p)

    def cloud(f):
        n_g = ppf // 2
        g = np.stack([rng.uniform(-20, 75, n_g) + ego[f][0, 3], rng.uniform(-15, 15, n_g), rng.normal(-1.8, 0.02, n_g)], 1)
        n_w = ppf - n_g
        side = rng.choice([-12.0, 12.0], n_w)
        wl = np.stack([rng.uniform(-20, 75, n_w) + ego[f][0, 3], side + rng.normal(0, 0.05, n_w),
                       rng.uniform(-1.8, 8, n_w)], 1)
        xyz = np.concatenate([g, wl])
        rgb = np.clip(0.5 + 0.1 * rng.normal(size=(ppf, 3)) + 0.3 * np.sin(xyz[:, :1] * 0.3), 0, 1)
        return np.concatenate([xyz, rgb], 1)
    ply = {"background": {f: cloud(f) for f in range(F)}}
    for k in range(4):
        ply[f"veh_{k}"] = {f: np.concatenate([rng.uniform(-1, 1, (800, 3)) * [2.3, 1.0, 0.8],
                                              np.tile(rng.uniform(0, 1, 3), (800, 1))], 1) for f in range(F)}
    track = {f"veh_{k}": {"camera_box": None, "lidar_box": {"heading": 0.1 * k, "center_x": 12.0 + 9 * k,
                                                             "center_y": -3.0 + 2.0 * k, "center_z": -1.0}} for k in range(4)}
    ext = np.eye(4)
    ext[:3, :3] = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], float)
    ext[:3, 3] = [1.5, 0.0, 0.3]
    ixt = np.array([[2050.0, 0, 960.0], [0, 2050.0, 640.0], [0, 0, 1.0]])
    return {"ply": ply, "track": track, "ego": ego, "ext": ext, "ixt": ixt, "H": H, "W": W, "F": F, "frame": 10}


def demo_workload(ppf: int = 150_000, scale_to_width: int = 1920):
    """The demo log's frame 10.  -> dict(cloud [N,6] world xyz + rgb (unfiltered), c2w, ixt, H, W)."""
    from street_crafter_amd import lidar_condition as lc
    log = demo_log(ppf)
    ply, track, ego, ext, ixt, H, W, F, frame = (log[k] for k in ("ply", "track", "ego", "ext", "ixt", "H", "W", "F", "frame"))
    cloud_w = lc.assemble_frame(ply, track, ego[frame], frame, F, delta_frames=10)
    c2w = lc.shifted_camera(ego[frame], ego, frame, ext)
    if scale_to_width != W:
        s = scale_to_width / W
        ixt = ixt.copy()
        ixt[:2] *= s
        W, H = scale_to_width, int(H * s)
    return {"cloud": cloud_w, "c2w": c2w, "ixt": ixt, "H": H, "W": W}


def _phases(pr, pts, colors, w2c, ixt, H, W, ev):
    """One frame of render_points_hip's pipeline (use_ndc_scale, scale 0.01) with an event after every step."""
    import torch
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    lib = _lib.load()
    dev, st, N = pts.device, R._stream(pts), pts.shape[0]
    tw, th = (W + 15) // 16, (H + 15) // 16
    fx, fy, cx, cy = ixt[0, 0], ixt[1, 1], ixt[0, 2], ixt[1, 2]
    radii = torch.empty((1, N), dtype=torch.int32, device=dev)
    means2d = torch.empty((1, N, 2), dtype=torch.float32, device=dev)
    depths = torch.empty((1, N), dtype=torch.float32, device=dev)
    records = torch.empty((N, 8), dtype=torch.float32, device=dev)
    img = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
    vm = torch.as_tensor(w2c).to(dev)
    ev[0].record()
    _lib.check(lib.sc_point_project(R._p(pts), R._p(colors), None, 1.0, None, N, R._p(vm), fx, fy, cx, cy, fx, W, H,
                                    1.0, 100.0, pr.RADIUS_NDC, 0.01, 1.0, R._p(radii), R._p(means2d), R._p(depths),
                                    R._p(records), st), "sc_point_project")
    ev[1].record()
    tpg = torch.empty((1, N), dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = R._ws(lib.sc_isect_workspace_bytes(N), dev)
    _lib.check(lib.sc_isect_count(R._p(means2d), R._p(radii), 1, N, 16, tw, th, R._p(tpg), R._p(total), R._p(ws),
                                  ws.numel(), st), "sc_isect_count")
    n = int(total.item())
    ids = torch.empty(n, dtype=torch.int64, device=dev)
    fids = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(lib.sc_isect_emit(R._p(means2d), R._p(radii), R._p(depths), 1, N, 16, tw, th, R._p(tpg), n, R._p(ids),
                                 R._p(fids), R._p(ws), ws.numel(), st), "sc_isect_emit")
    ev[2].record()
    tk, tv = torch.empty_like(ids), torch.empty_like(fids)
    sws = R._ws(lib.sc_radix_sort_workspace_bytes(n), dev)
    bits = 32 + int(math.floor(math.log2(tw * th))) + 1 + 1
    _lib.check(lib.sc_radix_sort_pairs_u64_i32(R._p(ids), R._p(fids), R._p(tk), R._p(tv), n, bits, R._p(sws),
                                               sws.numel(), st), "sc_radix_sort_pairs_u64_i32")
    ev[3].record()
    offs = torch.empty((1, th, tw), dtype=torch.int32, device=dev)
    _lib.check(lib.sc_isect_offsets(R._p(ids), n, 1, tw, th, R._p(offs), st), "sc_isect_offsets")
    ev[4].record()
    _lib.check(lib.sc_point_rasterize_fwd(R._p(records), N, W, H, tw, th, R._p(offs), R._p(fids), n, 10, None,
                                          R._p(img), 4, 1, R._p(img[..., 3]), 4, None, st), "sc_point_rasterize_fwd")
    ev[5].record()
    return n, img


def run_case(name, demo, filtered, frames, warmup, cpu):
    import torch
    from street_crafter_amd import lidar_condition as lc
    from street_crafter_amd import point_render as pr
    H, W, c2w, ixt = demo["H"], demo["W"], demo["c2w"], demo["ixt"]
    cl = demo["cloud"]
    if filtered:
        xyz, feat = lc.filter_visible(cl[:, :3], cl[:, 3:], c2w, ixt, H, W)
    else:
        xyz, feat = cl[:, :3], np.concatenate([cl[:, 3:], np.ones((cl.shape[0], 2))], 1)
    # device inputs (the training-time caller holds its points on the device); world coordinates moved to the camera
    # centre in float64 first, as render_points_hip does for host arrays
    origin = c2w[:3, 3]
    pts = torch.from_numpy((xyz - origin).astype(np.float32)).cuda()
    colors = torch.from_numpy(np.ascontiguousarray(feat[:, :3], dtype=np.float32)).cuda()
    c2w_c = c2w.copy()
    c2w_c[:3, 3] = 0.0
    w2c_c = np.linalg.inv(c2w_c)

    def frame():
        return pr.render_points_hip(c2w_c, ixt, pts, colors, H, W, use_ndc_scale=True, scale=0.01)
    for _ in range(warmup):
        frame()
    torch.cuda.synchronize()
    ts = []
    for _ in range(frames):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = frame()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ph = []
    for _ in range(max(frames // 2, 5)):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        n, img = _phases(pr, pts, colors, w2c_c, ixt, H, W, ev)
        ev[5].synchronize()
        ph.append([ev[i].elapsed_time(ev[i + 1]) for i in range(5)])
    ph = np.median(np.array(ph), axis=0)
    assert torch.equal(img, out), "phase-timed pipeline differs from render_points_hip"
    blend_bytes = n * (32 + 4) + H * W * 16          # records + flatten_ids gathered once, rgba written
    res = {"case": name, "H": H, "W": W, "points": int(xyz.shape[0]), "isects": n,
           "ms_per_frame_median": float(np.median(ts)), "ms_p10": float(np.percentile(ts, 10)),
           "ms_p90": float(np.percentile(ts, 90)), "frames": frames,
           "phase_ms": {"project": ph[0], "count_emit": ph[1], "radix_sort": ph[2], "offsets": ph[3], "blend": ph[4]},
           "blend_bytes": blend_bytes, "blend_hbm_floor_ms": blend_bytes / HBM_PEAK * 1e3,
           "blend_floor_over_measured": blend_bytes / HBM_PEAK * 1e3 / ph[4],
           "coverage": float((out[0, ..., 3] > 0).float().mean())}
    if cpu:
        t0 = time.perf_counter()
        lc.render_points(c2w, ixt, xyz, feat, H, W, use_ndc_scale=True, scale=0.01)
        res["cpu_render_points_s"] = time.perf_counter() - t0
    res["phase_ms"] = {k: float(v) for k, v in res["phase_ms"].items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="also time one numpy render_points per case")
    ap.add_argument("--out", default=None, help="directory for point_render_bench.json")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_render needs a GPU")
    results = []
    for width in (1920, 1600):
        demo = demo_workload(scale_to_width=width)
        for filtered in (True, False):
            name = f"{demo['W']}x{demo['H']} {'filtered' if filtered else 'unfiltered'}"
            r = run_case(name, demo, filtered, args.frames, args.warmup, args.cpu)
            results.append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "point_render_bench.json"), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
