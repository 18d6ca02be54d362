"""What the cameras' gradient costs: sc_projection_bwd against sc_projection_bwd_cam (the same pass plus 12 wave sums per
camera, an LDS step, one partial row per block and the per-camera reduction kernel), and a train step through
`rasterization()` with and without `viewmats.requires_grad`.

    python tools/bench_camera_grad.py [--iters 50] [--warmup 10] [--gaussians 1000000] [--out profiles/camera_grad_ab.txt]

One process, HIP events around each call, medians (and minima) of --iters calls after --warmup.  sc_projection_bwd is
timed BEFORE and AFTER the new entry.  The kernel rows run at N = --gaussians with C = 1 and C = 3 on a random scene under
the cameras of tests/camera_grad_ref.py; the train step renders 1600x1066 with one camera.  No threshold: the numbers are
the report.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--train-gaussians", type=int, default=300_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera_grad.py measures on the GPU: none found")
    import camera_grad_ref as CR
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    from street_crafter_amd.scenes import make_camera, make_scene
    lib = _lib.load()
    st = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ms), min(ms)

    N = a.gaussians
    lines = [f"tools/bench_camera_grad.py --iters {a.iters} --warmup {a.warmup} --gaussians {N} --train-gaussians {a.train_gaussians}",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"HIP events, microseconds, medians (minima) of {a.iters} calls after {a.warmup}",
             f"{'C':>2} {'entry':46} {'median':>9} {'min':>9}"]
    sc = make_scene(N, seed=5, x_span=0.8, y_span=0.5, z_range=(1.0, 40.0), scale_range=(0.002, 0.5)).to(DEV)
    cams = CR.operator_cameras()
    g = torch.Generator(device=DEV).manual_seed(1)
    for C in (1, 3):
        V = torch.stack([c.viewmat for c in cams[:C]]).to(DEV).contiguous()
        K = torch.stack([c.K for c in cams[:C]]).to(DEV).contiguous()
        radii = torch.empty((C, N), dtype=torch.int32, device=DEV)
        m2, d, con, comp = (torch.empty((C, N) + s, device=DEV) for s in ((2,), (), (3,), ()))
        _lib.check(lib.sc_projection_fwd(p(sc.means), p(sc.quats), p(sc.scales), p(V), p(K), C, N, CR.W0, CR.H0, 0.3, 0.001, 1000.0,
                                         0.0, p(radii), p(m2), p(d), p(con), p(comp), st()), "sc_projection_fwd")
        up = [torch.randn((C, N) + s, device=DEV, generator=g) for s in ((2,), (), (3,), ())]
        vm, vq, vs = (torch.empty((N, k), device=DEV) for k in (3, 4, 3))
        vV = torch.empty((C, 4, 4), device=DEV)
        ws = torch.empty(max(lib.sc_projection_bwd_cam_workspace_bytes(C, N), 16), dtype=torch.uint8, device=DEV)
        args = (p(sc.means), p(sc.quats), p(sc.scales), p(V), p(K), C, N, CR.W0, CR.H0, 0.3, p(radii), p(con), p(comp),
                p(up[0]), p(up[1]), p(up[2]), p(up[3]))
        plain = lambda: _lib.check(lib.sc_projection_bwd(*args, p(vm), p(vq), p(vs), st()), "sc_projection_bwd")
        cam = lambda: _lib.check(lib.sc_projection_bwd_cam(*args, p(vm), p(vq), p(vs), p(vV), p(ws), st()), "sc_projection_bwd_cam")
        only = lambda: _lib.check(lib.sc_projection_bwd_cam(*args, None, None, None, p(vV), p(ws), st()), "sc_projection_bwd_cam")
        rows = [("sc_projection_bwd (before)", timed(plain)), ("sc_projection_bwd_cam", timed(cam)),
                ("sc_projection_bwd_cam, v_viewmats only", timed(only)), ("sc_projection_bwd (after)", timed(plain))]
        for name, (med, mn) in rows:
            lines.append(f"{C:>2} {name:46} {med:9.1f} {mn:9.1f}")
        base = 0.5 * (rows[0][1][0] + rows[3][1][0])
        lines.append(f"{C:>2} visible rows {int((radii > 0).sum())} of {C * N}; sc_projection_bwd_cam / sc_projection_bwd = "
                     f"{rows[1][1][0] / base:.3f} (+{rows[1][1][0] - base:.1f} us; mean of the two plain rows)")
    # ---- a train step through rasterization()
    scene = make_scene(a.train_gaussians, sh_degree=3, seed=1, z_range=(1.0, 40.0), scale_range=(0.01, 0.3)).to(DEV)
    camera = make_camera(1600, 1066, 1200.0, 1200.0).to(DEV)
    leaves = [t.clone().requires_grad_(True) for t in (scene.means, scene.quats, scene.scales, scene.opacities.reshape(-1), scene.sh)]
    Ks, ctr = camera.K[None].contiguous(), camera.camera_center[None].contiguous()

    def step(cam_grad, own_centers):
        V = camera.viewmat[None].clone().requires_grad_(cam_grad)
        for t in leaves:
            t.grad = None
        rc, ra, _ = R.rasterization(*leaves, V, Ks, 1600, 1066, near_plane=camera.znear, far_plane=camera.zfar, sh_degree=3,
                                    render_mode="RGB+ED", rasterize_mode="antialiased",
                                    camera_centers_=None if own_centers else ctr)
        (rc.sum() + ra.sum()).backward()

    lines.append(f"train step through rasterization(): {a.train_gaussians} Gaussians, 1600x1066, SH degree 3, antialiased, RGB+ED, "
                 "loss = sum; forward + backward")
    rows = [("viewmats without grad (before)", timed(lambda: step(False, False))),
            ("viewmats.requires_grad, camera_centers_ given", timed(lambda: step(True, False))),
            ("viewmats.requires_grad, centres derived", timed(lambda: step(True, True))),
            ("viewmats without grad (after)", timed(lambda: step(False, False)))]
    for name, (med, mn) in rows:
        lines.append(f"   {name:46} {med:9.1f} {mn:9.1f}")
    base = 0.5 * (rows[0][1][0] + rows[3][1][0])
    lines.append(f"   with camera grad / without = {rows[1][1][0] / base:.3f} (camera_centers_ given), {rows[2][1][0] / base:.3f} (derived)")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
