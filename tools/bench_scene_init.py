"""A/B of scene initialisation: street_crafter_amd.scene_init (voxel down-sample + radius outlier filter in HIP) against
the host restatement of the same two steps, in one process, on a synthetic street-shaped LiDAR accumulation.

    python tools/bench_scene_init.py [--points 20000000] [--iters 3] [--out profiles/scene_init_ab.txt]
    python tools/bench_scene_init.py --fused-only --iters 1          # what a kernel trace is taken of
    python tools/bench_scene_init.py --kernel-trace DIR [--out ...]   # per-kernel table from a rocprofv3 --kernel-trace csv

The cloud: the surfaces of scenes.make_street_scene (ground, facades, kerb clutter, far field) sampled once, then
"scanned" --points / surface-points times with 1 cm of jitter, moved to world coordinates of kilometres: voxels of 0.1 m
hold tens to hundreds of points.  float64, as the reference's sweeps are after the ego-pose multiply.

Host route: the numpy restatement of the down-sample (packed int64 voxel keys, np.unique, np.add.at in input order:
tests/scene_init_ref.py's arithmetic with a one-dimensional key) and scipy's cKDTree radius count (16 workers) on the
down-sampled points.  It is NOT open3d, which a ROCm image does not have: open3d's own two calls are single-threaded and
were not measured.  The host route is timed before and after the fused one.  Wall clock; the fused calls include their
host reads (the bounds, the voxel count) and the allocation of their outputs and workspaces.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
VOXEL, NB, RADIUS = 0.1, 10, 0.5
PEAK = 8.0e12            # MI355X HBM3E, bytes/s


def make_cloud(n_points, surface_points, seed=0):
    import torch
    from street_crafter_amd.scenes import make_street_scene
    fg, _ = make_street_scene(surface_points, n_sky=0, seed=seed)
    base = fg.means.double().to(DEV)
    sweeps = max(1, n_points // surface_points)
    g = torch.Generator(device=DEV).manual_seed(seed)
    parts = [base + 0.01 * torch.randn(base.shape, generator=g, device=DEV, dtype=torch.float64) for _ in range(sweeps)]
    xyz = torch.cat(parts) + torch.tensor([3.1e3, -1.7e3, 40.0], dtype=torch.float64, device=DEV)
    del parts
    rgb = torch.rand(xyz.shape, generator=g, device=DEV, dtype=torch.float64)
    return xyz, rgb, sweeps


def host_voxels(xyz, rgb, v):
    import numpy as np
    vmin = xyz.min(axis=0) - 0.5 * v
    idx = np.floor((xyz - vmin) / v).astype(np.int64)
    bits = [int(idx[:, a].max()).bit_length() for a in range(3)]
    key = (idx[:, 0] << (bits[1] + bits[2])) | (idx[:, 1] << bits[2]) | idx[:, 2]
    _, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    m = counts.shape[0]
    sp, sc = np.zeros((m, 3)), np.zeros((m, 3))
    for a in range(3):
        np.add.at(sp[:, a], inv, xyz[:, a])
        np.add.at(sc[:, a], inv, rgb[:, a])
    c = counts[:, None].astype(np.float64)
    return sp / c, sc / c, counts.astype(np.int32)


def host_radius(pts, nb, radius):
    from scipy.spatial import cKDTree
    return cKDTree(pts).query_ball_point(pts, radius, return_length=True, workers=16) > nb


BYTES = {   # algorithmic bytes per launch: N input points, M voxels (for the filter's kernels N = M)
    "pc_bounds_kernel": lambda n, m: 24 * n,
    "pc_key_kernel": lambda n, m: 24 * n + 12 * n,
    "rs_hist_kernel": lambda n, m: 8 * n,
    "rs_scatter_kernel": lambda n, m: 24 * n,
    "pc_head_count_kernel": lambda n, m: 8 * n,
    "pc_head_scatter_kernel": lambda n, m: 8 * n + 4 * m,
    "pc_voxel_reduce_kernel": lambda n, m: 52 * n + 52 * m,
    "pc_gather_kernel": lambda n, m: 52 * n,
}


def kernel_table(trace_dir, n, m):
    """Per kernel of the two calls: launches, mean time, algorithmic bytes/s.  The trace holds one down-sample (N points)
    followed by one filter (M points): launches of a kernel are split between the two by their order in time."""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    ours = [(s, e, k) for s, e, k in rows if "pc_" in k or "rs_" in k]
    if not ours:
        return ["no pc_* / rs_* kernels in " + trace_dir]
    cut = max((s for s, e, k in ours if "pc_voxel_reduce_kernel" in k), default=None)
    out = [f"{'call':8} {'kernel':26} {'launches':>8} {'mean us':>10} {'total us':>10} {'GB/s':>9} {'of 8 TB/s':>9}"]
    for call, part, size in (("voxel", [r for r in ours if cut is None or r[0] <= cut], n),
                             ("radius", [r for r in ours if cut is not None and r[0] > cut], m)):
        names = []
        for _, _, k in part:
            short = next((b for b in list(BYTES) + ["pc_bounds_finish_kernel", "pc_scan_blocks_kernel", "rs_scan_rows_kernel",
                                                    "pc_longest_segment_kernel", "pc_radius_count_kernel"] if b in k), k[:26])
            if "pc_bounds_finish" in k:
                short = "pc_bounds_finish_kernel"
            if short not in names:
                names.append(short)
        for short in names:
            d = [(e - s) / 1e3 for s, e, k in part if short in k and not (short == "pc_bounds_kernel" and "finish" in k)]
            model = BYTES.get(short)
            if model:
                bps = model(size, m) / (sum(d) / len(d) * 1e-6)
                out.append(f"{call:8} {short:26} {len(d):8d} {sum(d) / len(d):10.1f} {sum(d):10.1f} {bps / 1e9:9.1f} {100 * bps / PEAK:8.1f}%")
            else:
                out.append(f"{call:8} {short:26} {len(d):8d} {sum(d) / len(d):10.1f} {sum(d):10.1f} {'-':>9} {'-':>9}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--surface-points", type=int, default=200_000)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 --kernel-trace csv of a --fused-only --iters 1 run")
    ap.add_argument("--sizes", default=None, help="N,M of the traced run (with --kernel-trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        n, m = (int(v) for v in a.sizes.split(","))
        text = "\n".join([f"per kernel, from a rocprofv3 --kernel-trace of one down-sample (N = {n}) and one filter (M = {m}); "
                          "algorithmic bytes over the kernel's mean time"] + kernel_table(a.kernel_trace, n, m)) + "\n"
        print(text, end="")
        if a.out:
            with open(a.out, "a") as f:
                f.write(text)
        return
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_init.py measures on the GPU: none found")
    from street_crafter_amd import scene_init

    xyz, rgb, sweeps = make_cloud(a.points, a.surface_points)
    n = xyz.shape[0]
    torch.cuda.synchronize()
    lines = [f"tools/bench_scene_init.py --points {a.points} --surface-points {a.surface_points} --iters {a.iters}",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; one run on one box",
             f"cloud: {a.surface_points} surface points of make_street_scene x {sweeps} sweeps with 1 cm jitter = N = {n} float64 points",
             f"voxel_size {VOXEL}, nb_points {NB}, radius {RADIUS}; wall clock, seconds"]

    def fused():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vx, vc, cnt, info = scene_init.voxel_down_sample(xyz, rgb, VOXEL, return_info=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        keep = scene_init.radius_outlier_mask(vx, NB, RADIUS)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0, t2 - t1), (vx, vc, cnt, keep, info)

    if a.fused_only:
        for _ in range(a.iters):
            t, res = fused()
        print(f"N,M = {n},{res[0].shape[0]}  voxel {t[0]:.4f} s  radius {t[1]:.4f} s")
        return

    def host():
        hx, hr = xyz.cpu().numpy(), rgb.cpu().numpy()
        t0 = time.perf_counter()
        p, c, cnt = host_voxels(hx, hr, VOXEL)
        t1 = time.perf_counter()
        keep = host_radius(p, NB, RADIUS)
        t2 = time.perf_counter()
        return (t1 - t0, t2 - t1), (p, c, cnt, keep)

    before, want = host()
    fused()                                                       # warm: library load, allocator
    times = []
    for _ in range(a.iters):
        t, got = fused()
        times.append(t)
    after, _ = host()
    vx, vc, cnt, keep, info = got
    m, kept = vx.shape[0], int(keep.sum())
    same = (np.array_equal(vx.cpu().numpy().view(np.uint64), want[0].view(np.uint64))
            and np.array_equal(vc.cpu().numpy().view(np.uint64), want[1].view(np.uint64))
            and np.array_equal(cnt.cpu().numpy(), want[2]))
    diff = int((keep.cpu().numpy() != want[3]).sum())
    lines.append(f"N = {n}  M = {m} voxels  kept = {kept}  key bits {info['key_bits']} = {sum(info['key_bits'])} "
                 f"-> {info['sort_passes']} sort passes of 8 bits  longest segment {info['longest_segment']} points")
    lines.append(f"fused result vs host restatement: voxel points / colours / counts bit-equal: {same}; "
                 f"masks differing from cKDTree's `<=` count: {diff} of {m}")
    lines.append(f"{'route':34} {'down-sample':>12} {'radius filter':>14} {'both':>9}")
    lines.append(f"{'host: numpy + cKDTree (before)':34} {before[0]:12.3f} {before[1]:14.3f} {sum(before):9.3f}")
    for i, t in enumerate(times):
        lines.append(f"{'scene_init (HIP), run %d' % (i + 1):34} {t[0]:12.4f} {t[1]:14.4f} {sum(t):9.4f}")
    lines.append(f"{'host: numpy + cKDTree (after)':34} {after[0]:12.3f} {after[1]:14.3f} {sum(after):9.3f}")
    best = min(times, key=sum)
    hv, hr_ = 0.5 * (before[0] + after[0]), 0.5 * (before[1] + after[1])
    lines.append(f"host / fused (means of the two host rows over the fastest fused run): down-sample {hv / best[0]:.0f}x, "
                 f"radius filter {hr_ / best[1]:.0f}x")
    lines.append(f"down-sample: {n * 48 / best[0] / 1e9:.1f} GB/s of input (48 B per point) end to end, "
                 f"{100 * n * 48 / best[0] / PEAK:.2f}% of 8 TB/s; the host reads included")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
