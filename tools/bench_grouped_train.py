"""Times what a training iteration with the object accumulation loss renders and differentiates (train.py:154 and
:202-208) -- `harness.caller.render_train_objects` -- as the reference spells it (two whole operator sequences under
grad: all models, then pc.obj_list) against the one-pass form that ends in `rasterize_to_pixels_grouped_train`, in ONE
process on the same GPU.

    python tools/bench_grouped_train.py [--steps 50] [--warmup 10] [--out FILE.json]

Scene: make_street_scene(1_000_000) at 1600x1066 with the 32 car-sized object boxes of tools/bench_render_all.py.
A step: forward, composite loss (mean of rgb and of acc against fixed targets) + `obj_acc_loss(acc_object, obj_bound)`,
backward to the Gaussian parameters.  Blocks A1 / B / A2 of --steps steps each after a warm-up of both: A = two renders,
which runs only operators this form does not touch; B = grouped.  A step is timed by HIP events around it, with the
device drained between steps; medians are reported.  B counts as faster only if its median is below min(A1, A2) by more
than |A1 - A2|, the spread of the unchanged path measured in the same call.
The images of A and B are asserted `torch.equal` once and the parameter gradients are compared.  The grouped forward and
backward kernels are then timed alone, through the C ABI, with events around each launch.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render_all import N_GAUSS, object_ids, time_block      # noqa: E402  (the same boxes, the same timer)

WIDTH, HEIGHT = 1600, 1066
PARAMS = ("means", "quats", "scales", "opacities", "sh")


def kernel_split(scene, cam, gids, steps):
    """The grouped forward with last positions and the grouped backward alone (training form: composite colours and alphas
    + the object group's alphas): the operators in front of them once, then each C entry point `steps` times.
    -> (forward ms, backward ms, intersections)"""
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
    gend = torch.empty(tw * th, 1, dtype=torch.int32, device=dev)
    rc_ = torch.empty(1, H, W, 4, device=dev)
    ra = torch.empty(1, H, W, 1, device=dev)
    gc = torch.empty(1, 1, H, W, 4, device=dev)
    ga = torch.empty(1, 1, H, W, 1, device=dev)
    last = torch.empty(2, 1, H, W, dtype=torch.int32, device=dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    v_rc = torch.randn(1, H, W, 4, generator=g).to(dev)
    v_ra = torch.randn(1, H, W, 1, generator=g).to(dev)
    v_ga = torch.randn(1, 1, H, W, 1, generator=g).to(dev)
    grads = torch.zeros(N * (2 + 3 + 4 + 1 + 2), device=dev)
    v_m, v_c, v_col, v_o, v_abs = torch.split(grads, (2 * N, 3 * N, 4 * N, N, 2 * N))
    st = _stream(means2d)
    _lib.check(lib.sc_group_extents(offs.data_ptr(), fids.data_ptr(), n, gids.data_ptr(), 1, N, 1, tw, th,
                                    gend.data_ptr(), st), "sc_group_extents")

    def forward():
        _lib.check(lib.sc_rasterize_fwd_groups_ids(means2d.data_ptr(), conics.data_ptr(), col.data_ptr(), opac.data_ptr(),
                                                   gids.data_ptr(), gend.data_ptr(), 1, N, 4, 1, W, H, 16, tw, th,
                                                   offs.data_ptr(), fids.data_ptr(), n, rc_.data_ptr(), ra.data_ptr(),
                                                   gc.data_ptr(), ga.data_ptr(), last.data_ptr(), st),
                   "sc_rasterize_fwd_groups_ids")

    def backward():      # (the gradients pile up across the timed launches: nothing reads them)
        _lib.check(lib.sc_rasterize_bwd_groups(means2d.data_ptr(), conics.data_ptr(), col.data_ptr(), opac.data_ptr(),
                                               gids.data_ptr(), 1, N, 4, 1, W, H, 16, tw, th, offs.data_ptr(),
                                               fids.data_ptr(), n, ra.data_ptr(), ga.data_ptr(), last.data_ptr(),
                                               v_rc.data_ptr(), v_ra.data_ptr(), None, v_ga.data_ptr(), v_abs.data_ptr(),
                                               v_m.data_ptr(), v_c.data_ptr(), v_col.data_ptr(), v_o.data_ptr(), st),
                   "sc_rasterize_bwd_groups")

    forward()
    backward()
    return time_block(forward, steps), time_block(backward, steps), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", type=int, default=N_GAUSS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from harness.caller import render_train_objects
    from street_crafter_amd.regularizers import obj_acc_loss
    from street_crafter_amd.scenes import make_camera, make_street_scene
    dev = "cuda:0"
    fg, _ = make_street_scene(a.n)
    obj = object_ids(fg.means).bool()
    f = 2050.0 * WIDTH / 1920.0
    scene, cam, obj = fg.to(dev), make_camera(WIDTH, HEIGHT, f, f).to(dev), obj.to(dev)
    for name in PARAMS:
        getattr(scene, name).requires_grad_(True)
    print(f"object share of N: {100 * float(obj.float().mean()):.2f} % ({int(obj.sum())} of {a.n} Gaussians)", flush=True)
    g = torch.Generator(device="cpu").manual_seed(5)
    target = torch.rand(3, HEIGHT, WIDTH, generator=g).to(dev)
    obj_bound = (torch.rand(1, HEIGHT, WIDTH, generator=g) < 0.3).to(dev)

    def step(grouped):
        for name in PARAMS:
            getattr(scene, name).grad = None
        out = render_train_objects(scene, cam, obj, grouped=grouped)
        loss = (out["rgb"] - target).abs().mean() + out["acc"].mean() + 0.1 * obj_acc_loss(out["acc_object"], obj_bound)
        loss.backward()
        return out

    out_a = step(False)
    grads_a = {n: getattr(scene, n).grad.clone() for n in PARAMS}
    grads_a["absgrad"] = out_a["viewspace_points"].absgrad
    out_b = step(True)
    for k in ("rgb", "acc", "depth", "acc_object"):
        assert torch.equal(out_a[k].detach(), out_b[k].detach()), f"{k}: the grouped render differs from the two renders"
    grads_b = {n: getattr(scene, n).grad for n in PARAMS}
    grads_b["absgrad"] = out_b["viewspace_points"].absgrad
    worst = {n: float((grads_b[n] - grads_a[n]).abs().max() / grads_a[n].abs().max().clamp(min=1e-30)) for n in grads_a}
    print("outputs: rgb, acc, depth, acc_object torch.equal; largest |grad B - grad A| / max|grad A|: "
          + ", ".join(f"{n} {v:.1e}" for n, v in worst.items()), flush=True)
    assert max(worst.values()) < 1e-3, worst
    del out_a, out_b, grads_a, grads_b
    for _ in range(a.warmup):
        step(False)
        step(True)
    a1 = time_block(lambda: step(False), a.steps)
    b = time_block(lambda: step(True), a.steps)
    a2 = time_block(lambda: step(False), a.steps)
    gids = torch.where(obj, 0, 255).to(torch.uint8)
    with torch.no_grad():
        t_fwd, t_bwd, n_isects = kernel_split(scene, cam, gids, a.steps)
    spread = abs(a1 - a2)
    faster = b < min(a1, a2) - spread
    res = {"n": a.n, "width": WIDTH, "height": HEIGHT, "steps": a.steps, "object_share_n": float(obj.float().mean()),
           "n_isects": n_isects, "A1_ms": a1, "B_ms": b, "A2_ms": a2, "spread_ms": spread, "B_faster": bool(faster),
           "raster_groups_ids_fwd_ms": t_fwd, "raster_groups_bwd_ms": t_bwd, "grad_rel_diff": worst,
           "device": torch.cuda.get_device_name(0)}
    print(f"forward + backward, median ms per step: A1 {a1:.3f}  B {b:.3f}  A2 {a2:.3f}  (spread of A {spread:.3f}) -> "
          + ("B is faster" if faster else "B is NOT faster by the rule"))
    print(f"kernels alone, median ms: grouped forward with last positions {t_fwd:.3f}  grouped backward {t_bwd:.3f}")
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            json.dump(res, f_, indent=1)


if __name__ == "__main__":
    main()
