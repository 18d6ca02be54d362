"""Times a training step through `rasterization()` with the fused training route off and on (rendering.set_fused_training,
SC_FUSED_TRAIN): the README's training configuration -- S-1M (1 000 000 Gaussians, sh_degree 1), 1600x1066, antialiased,
RGB+ED, absgrad=True, all five parameter groups requiring grad -- forward and backward under a FIXED sum-of-weights loss
(sum(w_rgb rgb) + sum(w_acc acc) + sum(w_depth depth), weights drawn once), so that everything timed is the route and
nothing is the loss.

    python tools/bench_fused_train.py [--steps 50] [--windows 5] [--warmup 5] [--out FILE.json]
    python tools/bench_fused_train.py --only on --steps 20 --windows 1      # one setting, for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_fused_train.py --only off --steps 20 --windows 1

Both settings run in the same process, alternating window by window (off, on, off, on, ...): each window is --steps
steps between two device events, after --warmup steps of that setting.  Reported per setting: steps/s of every window,
the median, and the spread (max - min) / median; the ratio on / off of the medians is only meaningful against that
spread.  With --check the gradients of one step per setting are compared (largest |on - off| / max|off| per leaf).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-gauss", type=int, default=1_000_000)
    ap.add_argument("--sh-degree", type=int, default=1)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1066)
    ap.add_argument("--steps", type=int, default=50, help="steps per timed window (>= 50 for a number to quote)")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per setting")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("off", "on"), default=None, help="one setting only (kernel traces)")
    ap.add_argument("--check", action="store_true", help="compare the two settings' gradients on one step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from street_crafter_amd import _lib, rendering
    from street_crafter_amd.scenes import make_camera, make_scene
    assert torch.cuda.is_available(), "bench_fused_train.py needs a GPU: a CPU run says nothing about speed"
    _lib.load()
    dev = "cuda:0"
    W, H = a.width, a.height
    cam = make_camera(W, H, 2050.0 * W / 1920.0, 2050.0 * W / 1920.0).to(dev)
    scene = make_scene(a.n_gauss, sh_degree=a.sh_degree).to(dev)
    params = {"means": scene.means, "quats": scene.quats, "scales": scene.scales, "opacities": scene.opacities, "sh": scene.sh}
    for t in params.values():
        t.requires_grad_(True)
    V, K, ctr = cam.viewmat[None].contiguous(), cam.K[None].contiguous(), cam.camera_center[None].contiguous()
    g = torch.Generator(device=dev).manual_seed(0)
    w_rgb = torch.randn(1, H, W, 3, device=dev, generator=g)
    w_acc = torch.randn(1, H, W, 1, device=dev, generator=g)
    w_depth = 0.1 * torch.randn(1, H, W, device=dev, generator=g)

    def step(fused):
        for t in params.values():
            t.grad = None
        prev = rendering.set_fused_training(fused)
        try:
            rc, ra, meta = rendering.rasterization(params["means"], params["quats"], params["scales"],
                                                   params["opacities"].reshape(-1), params["sh"], V, K, W, H,
                                                   near_plane=cam.znear, far_plane=cam.zfar, sh_degree=a.sh_degree,
                                                   render_mode="RGB+ED", absgrad=True, rasterize_mode="antialiased",
                                                   camera_centers_=ctr)
            assert meta["fused"] is fused
            meta["means2d"].retain_grad()
            ((rc[..., :3] * w_rgb).sum() + (ra * w_acc).sum() + (rc[..., 3] * w_depth).sum()).backward()
        finally:
            rendering.set_fused_training(prev)
        return meta

    settings = [s == "on" for s in (("off", "on") if a.only is None else (a.only,))]
    name = {False: "off", True: "on"}
    for fused in settings:                       # every shape either setting allocates, before anything is timed
        for _ in range(a.warmup):
            step(fused)
    torch.cuda.synchronize()
    rate = {name[f]: [] for f in settings}
    for _ in range(a.windows):
        for fused in settings:                   # alternating: a drift of the box hits both settings alike
            step(fused)                          # (the first step after a switch is not timed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(fused)
            e1.record()
            torch.cuda.synchronize()
            rate[name[fused]].append(a.steps / (e0.elapsed_time(e1) * 1e-3))
    res = {"device": torch.cuda.get_device_name(0), "n_gauss": a.n_gauss, "sh_degree": a.sh_degree, "width": W, "height": H,
           "steps_per_window": a.steps, "windows": a.windows, "settings": {}}
    for k, v in rate.items():
        med = statistics.median(v)
        res["settings"][k] = {"steps_per_s_windows": [round(x, 1) for x in v], "steps_per_s_median": round(med, 1),
                              "spread": round((max(v) - min(v)) / med, 4)}
    if len(settings) == 2:
        res["on_over_off"] = round(res["settings"]["on"]["steps_per_s_median"] / res["settings"]["off"]["steps_per_s_median"], 4)
    if a.check and len(settings) == 2:
        grads = {}
        for fused in settings:
            meta = step(fused)
            torch.cuda.synchronize()
            grads[fused] = {**{k: t.grad.clone() for k, t in params.items()}, "means2d": meta["means2d"].grad.clone()}
        res["grad_max_abs_diff_over_max_abs"] = {
            k: float((grads[True][k] - grads[False][k]).abs().max() / grads[False][k].abs().max().clamp_min(1e-30))
            for k in grads[False]}
    print(json.dumps(res), flush=True)
    for k, r in res["settings"].items():
        print(f"fused_train {k:>3}: {r['steps_per_s_median']:8.1f} steps/s (median of {a.windows} windows of {a.steps} steps; "
              f"spread {100 * r['spread']:.1f} %)  windows {r['steps_per_s_windows']}")
    if "on_over_off" in res:
        print(f"on / off: {res['on_over_off']:.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
