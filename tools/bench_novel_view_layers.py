"""Times the novel-view frame -- StreetGaussianRenderer.render_novel_view, the body of `render.py mode novel_view`, for a
scene with a sky sub-model -- as shipped (two fused `rasterization()` passes and the composite kernel:
`harness.caller.render_novel_view_u8(fused=True)`) against the one-pass form `street_crafter_amd.layers.novel_view_frame`,
in ONE process on the same GPU.

    python tools/bench_novel_view_layers.py [--frames 50] [--warmup 10] [--n 1000000] [--scenes s1m,street] [--out FILE.json]

Scenes, bench.py's own novel-view pair at 1920x1280: "s1m" = make_scene(n) with a sky of max(1000, n // 32) Gaussians
from make_street_scene; "street" = make_street_scene(n) with its own sky.
Blocks A1 / B / A2 of --frames frames each after a warm-up of both: A = the two-pass frame, which runs only code the
one-pass form does not touch; B = novel_view_frame(output="u8") with its default lift, the smallest power of two the
camera's planes allow (B with the lift 2^64 is timed once more behind A2: the frame is the same, isect_tiles' time is
not).  A frame is timed by HIP events around the call, with the device drained between frames; medians are reported.
B counts as faster only if its median is below min(A1, A2) by more than |A1 - A2|, the spread of the unchanged path
measured in the same call.
The frames of A and B are asserted `torch.equal` once.  Then the kernels alone, through the C ABI, with events around
each launch: the layered rasterizer (uint8 epilogue; the boundary search is part of it) against the two single-image
launches plus the composite, and `isect_tiles` on the merged set with layered keys (both lifts) against the two
separate calls.
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


def _concat(fg, sky):
    import torch
    cat = lambda name: torch.cat([getattr(fg, name), getattr(sky, name)]).contiguous()
    return cat("means"), cat("quats"), cat("scales"), cat("opacities").reshape(-1).contiguous(), cat("sh")


def kernel_split(fg, sky, cam, frames, lift):
    """The rasterizer launches and the intersection stage alone.  -> dict of median ms and list sizes."""
    import torch
    from street_crafter_amd import _lib
    from street_crafter_amd.dist import to_uint8_frame
    from street_crafter_amd.isect import _stream, isect_tiles
    from street_crafter_amd.layers import layered_depths
    from street_crafter_amd.rendering import rasterize_to_pixels
    lib, b = _lib.load(), _lib.binding()
    W, H = cam.width, cam.height
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    st = _stream(fg.means)

    def project(means, quats, scales, opac, sh):
        rc, radii, means2d, depths, _, conics, op, cols = b.projection_sh_fwd(
            means, quats, scales, opac, sh, cam.viewmat[None].contiguous(), cam.K[None].contiguous(),
            cam.camera_center.reshape(1, 3).contiguous(), fg.sh_degree, W, H, 0.3, cam.znear, cam.zfar, 0.0, True, False, st)
        _lib.check(rc, "sc_projection_sh_fwd")
        return radii, means2d, depths, conics, op, cols

    def lists(radii, means2d, keys):
        from street_crafter_amd.isect import isect_offset_encode
        _, ids, fids = isect_tiles(means2d, radii, keys, 16, tw, th, packed=False, n_cameras=1)
        offs = isect_offset_encode(ids, 1, tw, th)
        return offs.as_subclass(torch.Tensor), (fids.plain() if hasattr(fids, "plain") else fids)

    with torch.no_grad():
        one = lambda sc: (sc.means, sc.quats, sc.scales, sc.opacities.reshape(-1).contiguous(), sc.sh)
        pf, ps, pm = project(*one(fg)), project(*one(sky)), project(*_concat(fg, sky))
        keys, keys64 = layered_depths(pm[2], fg.n, lift), layered_depths(pm[2], fg.n)
        lf, ls, lm = lists(pf[0], pf[1], pf[2]), lists(ps[0], ps[1], ps[2]), lists(pm[0], pm[1], keys)
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=fg.means.device)

        def raster_layers():
            rc = b.rasterize_fwd_layers(pm[1], pm[3], pm[5], pm[4], fg.n, W, H, 16, lm[0], lm[1], 2, 0, False, out, st)[0]
            _lib.check(rc, "sc_rasterize_fwd_layers")

        def raster_two():
            rc_f, ra_f = rasterize_to_pixels(pf[1], pf[3], pf[5], pf[4], W, H, 16, lf[0], lf[1], packed=False)
            rc_s, _ = rasterize_to_pixels(ps[1], ps[3], ps[5], ps[4], W, H, 16, ls[0], ls[1], packed=False)
            to_uint8_frame(rc_f[0, ..., :3].permute(2, 0, 1), acc=ra_f[0, ..., 0],
                           sky_rgb_chw=rc_s[0, ..., :3].permute(2, 0, 1), out=out)

        def isect_merged():
            isect_tiles(pm[1], pm[0], keys, 16, tw, th, packed=False, n_cameras=1)[2].shape

        def isect_merged_64():
            isect_tiles(pm[1], pm[0], keys64, 16, tw, th, packed=False, n_cameras=1)[2].shape

        def isect_two():
            isect_tiles(pf[1], pf[0], pf[2], 16, tw, th, packed=False, n_cameras=1)[2].shape
            isect_tiles(ps[1], ps[0], ps[2], 16, tw, th, packed=False, n_cameras=1)[2].shape

        raster_two()
        want = out.clone()
        raster_layers()
        assert torch.equal(out, want), "the layered rasterizer's frame differs from the two launches + composite"
        for fn in (isect_merged, isect_merged_64, isect_two):
            for _ in range(3):
                fn()
        res = {"raster_layers_ms": time_block(raster_layers, frames), "raster_two_plus_composite_ms": time_block(raster_two, frames),
               "isect_merged_ms": time_block(isect_merged, frames), "isect_two_calls_ms": time_block(isect_two, frames),
               "isect_merged_lift_2p64_ms": time_block(isect_merged_64, frames),
               "n_isects_front": lf[1].numel(), "n_isects_back": ls[1].numel(), "n_isects_merged": lm[1].numel()}
    assert res["n_isects_merged"] == res["n_isects_front"] + res["n_isects_back"]
    return res


def bench_scene(name, fg, sky, cam, frames, warmup):
    import torch
    from harness.caller import render_novel_view_u8
    from street_crafter_amd.layers import LIFT, novel_view_frame, smallest_lift
    merged = _concat(fg, sky)
    lift = smallest_lift(cam.znear, cam.zfar)
    kw = dict(near_plane=cam.znear, far_plane=cam.zfar, sh_degree=fg.sh_degree, camera_center=cam.camera_center,
              output="u8")
    out_a = torch.empty(cam.height, cam.width, 3, dtype=torch.uint8, device=fg.means.device)
    out_b = torch.empty_like(out_a)

    def run_a():
        return render_novel_view_u8(fg, sky, cam, out=out_a, fused=True)

    def run_b(lift=None):
        return novel_view_frame(*merged, cam.viewmat, cam.K, cam.width, cam.height, fg.n, out=out_b, lift=lift, **kw)

    def run_b64():
        return run_b(LIFT)

    run_a()
    run_b()
    assert torch.equal(out_a, out_b), f"{name}: the one-pass frame differs from the two-pass frame"
    print(f"{name}: frames torch.equal ({fg.n} + {sky.n} Gaussians)", flush=True)
    for _ in range(warmup):
        run_a()
        run_b()
    a1 = time_block(run_a, frames)
    b = time_block(run_b, frames)
    a2 = time_block(run_a, frames)
    for _ in range(3):
        run_b64()
    assert torch.equal(out_a, out_b), f"{name}: the one-pass frame with lift 2^64 differs from the two-pass frame"
    b64 = time_block(run_b64, frames)
    spread = abs(a1 - a2)
    faster = b < min(a1, a2) - spread
    res = {"scene": name, "n_front": fg.n, "n_back": sky.n, "width": cam.width, "height": cam.height, "frames": frames,
           "lift_log2": math.log2(lift), "A1_ms": a1, "B_ms": b, "A2_ms": a2, "spread_ms": spread, "B_faster": bool(faster),
           "B_lift_2p64_ms": b64}
    print(f"{name}, median ms per frame: A1 {a1:.3f}  B {b:.3f}  A2 {a2:.3f}  (spread of A {spread:.3f}) -> "
          + ("B is faster" if faster else "B is NOT faster by the rule") + f"; B with lift 2^64 {b64:.3f}", flush=True)
    res.update(kernel_split(fg, sky, cam, frames, lift))
    print(f"{name}, kernels alone, median ms: layered rasterizer {res['raster_layers_ms']:.3f} vs two launches + "
          f"composite {res['raster_two_plus_composite_ms']:.3f}; isect_tiles merged {res['isect_merged_ms']:.3f} vs two "
          f"calls {res['isect_two_calls_ms']:.3f} (merged with lift 2^64: {res['isect_merged_lift_2p64_ms']:.3f})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--scenes", default="s1m,street")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from street_crafter_amd.scenes import make_camera, make_scene, make_street_scene
    dev = "cuda:0"
    W, H = a.width, a.height
    cam = make_camera(W, H, 2050.0 * W / 1920.0, 2050.0 * W / 1920.0).to(dev)
    results = []
    for name in a.scenes.split(","):
        if name == "s1m":
            fg = make_scene(a.n, sh_degree=1)
            _, sky = make_street_scene(64, n_sky=max(1000, a.n // 32), sh_degree=1)
        elif name == "street":
            fg, sky = make_street_scene(a.n, sh_degree=1)
        else:
            raise SystemExit(f"unknown scene {name!r}")
        results.append(bench_scene(name, fg.to(dev), sky.to(dev), cam, a.frames, a.warmup))
    res = {"device": torch.cuda.get_device_name(0), "scenes": results}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
