"""Times the fused regularizers (street_crafter_amd/regularizers.py) against the reference's torch expressions
(train.py:194-220: the trimmed LiDAR depth loss with its boolean index and sorted topk, the sky and object accumulation
losses) on the same GPU.

    python tools/bench_regularizers.py [--iters 100] [--warmup 10] [--out FILE.json]

Cases: 1600x1066 and 1920x1280; the depth loss at LiDAR densities of 5, 20 and 100 %, on the rasterizer's depth view;
the sky and object losses together on a [1,H,W] acc with a [1,H,W] sky mask and a [1,H,W] object mask.
Per case and path: forward, backward and forward+backward in ms (HIP events around each, median over --iters after
--warmup), and for the fused path the compulsory bytes and their fraction of 8 TB/s.  The kernel split comes from a
separate `rocprofv3 --kernel-trace --stats -- python tools/bench_regularizers.py --iters 20` run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # B/s, MI355X spec


def torch_depth(depth, lidar_depth, mask):
    """train.py:213-218."""
    import torch
    depth_mask = torch.logical_and((lidar_depth > 0.), mask)
    depth_error = torch.abs((depth[depth_mask] - lidar_depth[depth_mask]))
    depth_error, _ = torch.topk(depth_error, int(0.95 * depth_error.size(0)), largest=False)
    return depth_error.mean()


def torch_acc(acc, sky_mask, obj_bound):
    """train.py:194-196 + 205-206 (the object loss on the same acc)."""
    import torch
    a = torch.clamp(acc, min=1e-6, max=1. - 1e-6)
    sky = torch.where(sky_mask, -torch.log(1 - a), -(a * torch.log(a) + (1. - a) * torch.log(1. - a))).mean()
    obj = torch.where(obj_bound, -(a * torch.log(a) + (1. - a) * torch.log(1. - a)), -torch.log(1. - a)).mean()
    return sky, obj


def fused_bytes(H, W, term):
    """Compulsory HBM bytes of the fused path.  Depth: the forward reads depth, lidar, mask (9 B/pixel; depth is a view
    of the [1,H,W,4] render, so its cache lines carry 16 B/pixel), writes and re-reads the 4-byte keys three times
    (two more histogram passes, the sum); the backward reads the inputs again and writes grad_depth.
    Accumulation (both losses): each forward reads acc + its mask, each backward reads them and writes grad_acc."""
    P = H * W
    if term == "depth":
        inputs = 16 * P + 4 * P + P
        return inputs + 4 * P + 3 * 4 * P, inputs + 4 * P
    return 2 * (4 * P + P), 2 * (4 * P + P + 4 * P)


def time_case(H, W, term, density, iters, warmup, path):
    import torch
    from street_crafter_amd import regularizers as R
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    rc = 1 + 50 * torch.rand(1, H, W, 4, device=dev, generator=g)
    lidar = rc[..., 3] + torch.randn(1, H, W, device=dev, generator=g)
    lidar[torch.rand(1, H, W, device=dev, generator=g) >= density] = 0.0
    mask = torch.rand(1, H, W, device=dev, generator=g) > 0.1
    ra = torch.rand(1, H, W, 1, device=dev, generator=g)
    sky = torch.rand(1, H, W, device=dev, generator=g) > 0.7
    obj = torch.rand(1, H, W, device=dev, generator=g) > 0.5
    fw_t, bw_t, tot_t = [], [], []
    for i in range(warmup + iters):
        src = (rc if term == "depth" else ra).detach().clone().requires_grad_(True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        if term == "depth":
            depth = src[..., 3]
            loss = 0.01 * (R.lidar_depth_loss(depth, lidar, mask) if path == "hip" else torch_depth(depth, lidar, mask))
        else:
            acc = src[..., 0]
            if path == "hip":
                loss = 0.05 * R.sky_loss(acc, sky) + 0.1 * R.obj_acc_loss(acc, obj)
            else:
                s, o = torch_acc(acc, sky, obj)
                loss = 0.05 * s + 0.1 * o
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw_t.append(e[0].elapsed_time(e[1]))
            bw_t.append(e[1].elapsed_time(e[2]))
            tot_t.append(e[0].elapsed_time(e[2]))
    return {"fwd_ms": statistics.median(fw_t), "bwd_ms": statistics.median(bw_t), "fwd_bwd_ms": statistics.median(tot_t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from street_crafter_amd import _lib
    _lib.load()
    rows = []
    for (W, H) in ((1600, 1066), (1920, 1280)):
        for term, density in (("depth", 0.05), ("depth", 0.2), ("depth", 1.0), ("acc", None)):
            r = {"W": W, "H": H, "term": term, "density": density}
            for path in ("hip", "torch"):
                r[path] = time_case(H, W, term, density if density is not None else 1.0, a.iters, a.warmup, path)
            fb, bb = fused_bytes(H, W, term)
            r["hip"]["fwd_MB"], r["hip"]["bwd_MB"] = fb / 1e6, bb / 1e6
            r["hip"]["fwd_frac_hbm"] = fb / (r["hip"]["fwd_ms"] * 1e-3) / HBM_PEAK
            r["hip"]["bwd_frac_hbm"] = bb / (r["hip"]["bwd_ms"] * 1e-3) / HBM_PEAK
            r["speedup_fwd_bwd"] = r["torch"]["fwd_bwd_ms"] / r["hip"]["fwd_bwd_ms"]
            rows.append(r)
            print(json.dumps(r), flush=True)
    print(f"{'case':<24}{'hip fwd':>9}{'bwd':>8}{'f+b':>8}{'torch fwd':>11}{'bwd':>8}{'f+b':>8}{'x':>7}"
          f"{'fwd MB':>8}{'%HBM':>6}{'bwd MB':>8}{'%HBM':>6}")
    for r in rows:
        h, t = r["hip"], r["torch"]
        name = f"{r['W']}x{r['H']} " + (f"depth {int(100 * r['density'])}%" if r["term"] == "depth" else "sky+obj")
        print(f"{name:<24}{h['fwd_ms']:9.3f}{h['bwd_ms']:8.3f}{h['fwd_bwd_ms']:8.3f}{t['fwd_ms']:11.3f}{t['bwd_ms']:8.3f}"
              f"{t['fwd_bwd_ms']:8.3f}{r['speedup_fwd_bwd']:7.1f}{h['fwd_MB']:8.1f}{100 * h['fwd_frac_hbm']:6.1f}"
              f"{h['bwd_MB']:8.1f}{100 * h['bwd_frac_hbm']:6.1f}")
    print("device:", torch.cuda.get_device_name(0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
