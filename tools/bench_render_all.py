"""Times `harness.caller.render_all` -- StreetGaussianRenderer.render_all, the body of `render.py mode trajectory` -- as
the reference spells it (three whole operator sequences: all models, background, objects) against the one-pass form
that ends in `rasterize_to_pixels_grouped`, in ONE process on the same GPU.

    python tools/bench_render_all.py [--frames 50] [--warmup 10] [--out FILE.json]

Scene: make_street_scene(1_000_000) at 1920x1280.  Object Gaussians: those whose means fall inside 32 car-sized boxes
(2 x 1.5 x 4.5 m) standing on the road, placed from a fixed seed; everything else is background.
Blocks A1 / B / A2 of --frames frames each after a warm-up of both: A = render_all(grouped=False), which runs only
code the grouped path does not touch; B = grouped=True.  A frame is timed by HIP events around the call, with the
device drained between frames; medians are reported.  B counts as faster only if its median is below min(A1, A2) by
more than |A1 - A2|, the spread of the unchanged path measured in the same call.
The seven outputs of A and B are asserted `torch.equal` once.  The two kernels of the grouped rasterizer are then timed
alone, through the C ABI, with events around each launch.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_GAUSS = 1_000_000
N_BOXES = 32
BOX_HALF = (1.0, 0.75, 2.25)      # a car: 2 x 1.5 x 4.5 m
BOX_SEED = 7


def object_ids(means, road_half_width=9.0, cam_height=1.6, depth=160.0):
    """uint8 [N]: 1 inside one of the boxes, else 0.  The boxes stand on the road plane (y is down: the ground is at
    y = cam_height), 6 m to three quarters of the mapped depth ahead."""
    import torch
    g = torch.Generator().manual_seed(BOX_SEED)
    u = torch.rand(N_BOXES, 2, generator=g)
    cx = (u[:, 0] * 2 - 1) * (road_half_width - BOX_HALF[0])
    cz = 6.0 + u[:, 1] * (0.75 * depth - 6.0)
    centre = torch.stack([cx, torch.full((N_BOXES,), cam_height - BOX_HALF[1]), cz], -1)
    half = torch.tensor(BOX_HALF)
    ids = torch.zeros(means.shape[0], dtype=torch.uint8)
    for b in range(N_BOXES):
        ids |= ((means - centre[b]).abs() <= half).all(-1).to(torch.uint8)
    return ids


def time_block(fn, frames):
    import torch
    ms = []
    for _ in range(frames):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def kernel_split(scene, cam, gids, frames):
    """group_extents and the grouped rasterizer alone: the operators in front of them once, then each C entry point
    `frames` times with events around the launch.  -> (extents ms, raster ms, intersections, object intersections)"""
    import torch
    from gsplat.rendering import fully_fused_projection, isect_offset_encode, isect_tiles, spherical_harmonics
    from street_crafter_amd import _lib
    from street_crafter_amd.isect import _stream
    lib = _lib.load()
    W, H = cam.width, cam.height
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    with torch.no_grad():
        radii, means2d, depths, conics, comp = fully_fused_projection(
            scene.means, None, scene.quats, scene.scales, cam.viewmat[None], cam.K[None], W, H, packed=False,
            near_plane=cam.znear, far_plane=cam.zfar, calc_compensations=True)
        opac = (scene.opacities[None, :, 0] * comp).contiguous()
        _, isect_ids, fids = isect_tiles(means2d, radii, depths, 16, tw, th, packed=False, n_cameras=1)
        offs = isect_offset_encode(isect_ids, 1, tw, th)
        fids = fids.plain() if hasattr(fids, "plain") else fids
        dirs = scene.means[None] - cam.camera_center
        col = spherical_harmonics(scene.sh_degree, dirs, scene.sh.expand(1, -1, -1, -1), masks=radii > 0)
        col = torch.cat((torch.clamp_min(col + 0.5, 0.0), depths[..., None]), dim=-1).contiguous()
    N, n = scene.n, fids.numel()
    dev = means2d.device
    gend = torch.empty(tw * th, 2, dtype=torch.int32, device=dev)
    rc_ = torch.empty(1, H, W, 4, device=dev)
    ra = torch.empty(1, H, W, 1, device=dev)
    gc = torch.empty(2, 1, H, W, 4, device=dev)
    ga = torch.empty(2, 1, H, W, 1, device=dev)
    st = _stream(means2d)

    def extents():
        _lib.check(lib.sc_group_extents(offs.data_ptr(), fids.data_ptr(), n, gids.data_ptr(), 1, N, 2, tw, th,
                                        gend.data_ptr(), st), "sc_group_extents")

    def raster():
        _lib.check(lib.sc_rasterize_fwd_groups(means2d.data_ptr(), conics.data_ptr(), col.data_ptr(), opac.data_ptr(),
                                               gids.data_ptr(), gend.data_ptr(), 1, N, 4, 2, W, H, 16, tw, th,
                                               offs.data_ptr(), fids.data_ptr(), n, rc_.data_ptr(), ra.data_ptr(),
                                               gc.data_ptr(), ga.data_ptr(), st), "sc_rasterize_fwd_groups")

    extents()
    raster()
    t_ext, t_ras = time_block(extents, frames), time_block(raster, frames)
    n_obj = int((gids[fids.to(torch.int64)] == 1).sum())
    return t_ext, t_ras, n, n_obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=N_GAUSS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from harness.caller import render_all
    from street_crafter_amd.scenes import make_camera, make_street_scene
    dev = "cuda:0"
    fg, _ = make_street_scene(a.n)
    gids = object_ids(fg.means)
    scene, cam, gids = fg.to(dev), make_camera().to(dev), gids.to(dev)
    share_n = float(gids.float().mean())
    print(f"object share of N: {100 * share_n:.2f} % ({int(gids.sum())} of {a.n} Gaussians)", flush=True)

    def run_a():
        return render_all(scene, cam, gids, grouped=False)

    def run_b():
        return render_all(scene, cam, gids, grouped=True)

    out_a, out_b = run_a(), run_b()
    for k in ("rgb", "acc", "depth", "rgb_background", "acc_background", "rgb_object", "acc_object"):
        assert torch.equal(out_a[k], out_b[k]), f"{k}: the grouped render differs from the three renders"
    print("outputs: all seven torch.equal", flush=True)
    del out_a, out_b
    for _ in range(a.warmup):
        run_a()
        run_b()
    a1 = time_block(run_a, a.frames)
    b = time_block(run_b, a.frames)
    a2 = time_block(run_a, a.frames)
    t_ext, t_ras, n_isects, n_obj = kernel_split(scene, cam, gids, a.frames)
    print(f"object share of the intersections: {100 * n_obj / max(n_isects, 1):.2f} % ({n_obj} of {n_isects})")
    spread = abs(a1 - a2)
    faster = b < min(a1, a2) - spread
    res = {"n": a.n, "width": cam.width, "height": cam.height, "frames": a.frames, "object_share_n": share_n,
           "object_share_isects": n_obj / max(n_isects, 1), "n_isects": n_isects, "A1_ms": a1, "B_ms": b, "A2_ms": a2,
           "spread_ms": spread, "B_faster": bool(faster), "group_extents_ms": t_ext, "raster_groups_ms": t_ras,
           "device": torch.cuda.get_device_name(0)}
    print(f"render_all, median ms per frame: A1 {a1:.3f}  B {b:.3f}  A2 {a2:.3f}  (spread of A {spread:.3f}) -> "
          + ("B is faster" if faster else "B is NOT faster by the rule"))
    print(f"kernels alone, median ms: group_extents {t_ext:.3f}  grouped rasterizer {t_ras:.3f}")
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
