"""A/B of the actor poses of a frame: street_crafter_amd.actor_pose (TrackTable.plan on the host + one HIP launch, one more
and two memsets backward) against a plain-torch restatement of the reference's per-actor loop (ActorPose.get_tracking_rotation
/ get_tracking_translation, street_gaussian/models/actor_pose.py:83-144, stacked as parse_camera does) WITH its device-side
asserts -- two host waits per actor are part of what that loop costs.

    python tools/bench_actor_pose.py [--iters 50] [--warmup 5] [--out profiles/actor_pose_ab.txt]

Per A in {8, 32} actors, with grad (forward + backward from given upstream gradients into fresh opt_trans / opt_rots
gradients) and under no_grad, and per queue state:
  idle    the stream is empty when the step starts
  busy    one rasterizer frame (300 k Gaussians, 1066x1600, eval) has just been enqueued in front: every host wait of the
          torch loop now waits for that frame first
a step is timed on the host clock: "host" from the call to its return, "done" from the call until the device has finished
everything queued (the frame in front included; "frame alone" is that frame without any pose work behind it).  Medians of
--iters steps after --warmup.  The torch route runs BEFORE and AFTER the fused one in the same process.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
CAMS, FRAMES, MAX_OBJ = 3, 40, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=300_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_actor_pose.py measures on the GPU: none found")
    import actor_pose_ref as ref                                    # tests/: the torch restatement
    from harness.caller import render_gaussians
    from street_crafter_amd import actor_pose
    from street_crafter_amd.scenes import make_camera, make_scene

    tr, ts, ot, th = ref.make_table(CAMS, FRAMES, MAX_OBJ, seed=2)
    table = actor_pose.TrackTable(tr, ts, device=DEV)
    opt_trans = torch.from_numpy(ot).to(DEV).requires_grad_(True)
    opt_rots = torch.from_numpy(th).to(DEV).requires_grad_(True)
    mod = ref.TorchActorPose(tr, ts, opt_trans, opt_rots, DEV)
    cam_, frame = 1, 17
    stamp = ts[cam_][frame]
    scene = make_scene(a.gaussians, seed=1, z_range=(1.0, 40.0), scale_range=(0.01, 0.3)).to(DEV)
    camera = make_camera(1600, 1066, 1200.0, 1200.0).to(DEV)

    def frame_in_front():
        with torch.no_grad():
            render_gaussians(scene, camera, mode="eval")

    def timed(step, busy):
        torch.cuda.synchronize()
        if busy:
            frame_in_front()
        t0 = time.perf_counter()
        step()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3

    def measure(step, busy):
        host, done = [], []
        for i in range(a.warmup + a.iters):
            h, d = timed(step, busy)
            if i >= a.warmup:
                host.append(h); done.append(d)
        return statistics.median(host), statistics.median(done), min(done)

    lines = [f"tools/bench_actor_pose.py --iters {a.iters} --warmup {a.warmup} --gaussians {a.gaussians}",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"table: {CAMS} cameras x {FRAMES} frames x {MAX_OBJ} objects; wall clock, ms, medians of {a.iters}",
             "host = call to return; done = call until the device has finished everything queued (busy: the frame in front included)"]
    for _ in range(3):
        frame_in_front()
    fa = measure(lambda: None, True)
    lines.append(f"frame alone (enqueued before the clock starts, nothing behind it): done {fa[1]:.3f} (min {fa[2]:.3f})")
    lines.append(f"{'A':>3} {'mode':8} {'queue':5} {'route':22} {'host':>9} {'done':>9} {'min done':>9}")
    for A in (8, 32):
        ids = list(range(0, 2 * A, 2))
        g = torch.Generator(device=DEV).manual_seed(A)
        g_rots, g_trans = torch.randn(A, 4, device=DEV, generator=g), torch.randn(A, 3, device=DEV, generator=g)

        def clear():
            opt_trans.grad = opt_rots.grad = None

        def torch_grad():
            clear()
            torch.autograd.backward(mod.poses(ids, cam_, frame, stamp), [g_rots, g_trans])

        def hip_grad():
            clear()
            plan = table.plan(ids, cam_, frame, stamp)
            torch.autograd.backward(actor_pose.actor_poses(table, plan, opt_trans, opt_rots), [g_rots, g_trans])

        def torch_eval():
            with torch.no_grad():
                return mod.poses(ids, cam_, frame, stamp)

        def hip_eval():
            with torch.no_grad():
                return actor_pose.actor_poses(table, table.plan(ids, cam_, frame, stamp), opt_trans, opt_rots)

        # the two routes give the same poses and gradients
        torch_grad()
        want = (opt_trans.grad.clone(), opt_rots.grad.clone())
        hip_grad()
        dq = float((torch_eval()[0] - hip_eval()[0]).abs().max())
        dg = max(float((want[0] - opt_trans.grad).abs().max()), float((want[1] - opt_rots.grad).abs().max()))
        lines.append(f"{A:>3} largest difference between the routes: rotations {dq:.2e}, gradients {dg:.2e}")
        for mode, t_step, h_step in (("grad", torch_grad, hip_grad), ("no_grad", torch_eval, hip_eval)):
            for busy in (False, True):
                rows = [("torch loop (before)", measure(t_step, busy)), ("actor_pose.py", measure(h_step, busy)),
                        ("torch loop (after)", measure(t_step, busy))]
                for name, (h, d, mn) in rows:
                    lines.append(f"{A:>3} {mode:8} {'busy' if busy else 'idle':5} {name:22} {h:9.3f} {d:9.3f} {mn:9.3f}")
                ref_h = 0.5 * (rows[0][1][0] + rows[2][1][0])
                ref_d = 0.5 * (rows[0][1][1] + rows[2][1][1])
                lines.append(f"{A:>3} {mode:8} {'busy' if busy else 'idle':5} torch loop / actor_pose.py: host "
                             f"{ref_h / rows[1][1][0]:.1f}x, done {ref_d / rows[1][1][1]:.2f}x (means of the two torch rows)")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
