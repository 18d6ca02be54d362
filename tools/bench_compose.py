"""Times the head of a frame on the GPU: street_crafter_amd.compose.compose_frame (one HIP launch per 16 sub-models,
forward and backward) against a plain-torch restatement of the reference's sequence -- parse_camera's pose expansion and
the five get_* properties of StreetGaussianModel (street_gaussian_model.py:243-407), walked back by autograd.

    python tools/bench_compose.py [--iters 20] [--warmup 5] [--actors 32] [--out FILE.json]

Scene (as tools/bench_train_tail.py): a background of 1 M Gaussians with 16 SH bases, --actors actors of 20 k Gaussians
each (fourier_dim 5, half of the rows flipped, as in training with flip_prob 0.5) and a 100 k sky model.  A step is the
forward plus the backward from given upstream gradients of all five outputs, into fresh .grad tensors.
The torch route runs BEFORE and AFTER the fused one in the same process (clocks and allocator drift show as a difference
between the two).  Per route and step:
  device ms   HIP events around the step (median over --iters after --warmup; includes the gaps a host-bound route leaves)
  host ms     host clock from the call to its return, before any synchronise
  ops         aten operators dispatched per step that are not views (each is at least one launch); for the fused route the
              launches are counted from the plan: one forward and one backward kernel per 16 non-empty sub-models, plus the
              two memsets of the pose gradients
"kernels" is the two entry points alone, called on a prebuilt table with preallocated outputs: device time of the launches
without the Python around them, and the bytes they must move (every raw parameter and output once forward; the upstream
gradients, the four small raw fields and every gradient once backward) against that time and 8 TB/s.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # B/s, MI355X spec
DEV = "cuda:0"
K, F = 16, 5
FRAME = 7
VIEWS = ("view", "reshape", "expand", "unbind", "select", "slice", "transpose", "unsqueeze", "squeeze", "detach",
         "alias", "as_strided", "permute", "unsafe_view", "t.default", "split")


def make_scene(n_actors, seed=0, scale=1.0):
    import torch
    from street_crafter_amd import compose
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.randn(s, device=DEV, generator=gen) * scale).requires_grad_(True)

    def model(name, kind, n, f, **kw):
        return compose.FrameModel(name=name, kind=kind, xyz=rnd(n, 3, scale=3.0), scaling=rnd(n, 3, scale=0.7),
                                  rotation=rnd(n, 4), opacity=rnd(n, 1, scale=2.0), features_dc=rnd(n, f, 3, scale=0.6),
                                  features_rest=rnd(n, K - 1, 3, scale=0.2), **kw)
    models = [model("background", compose.STATIC, int(1_000_000 * scale), 1)]
    models += [model(f"obj_{i:03d}", compose.ACTOR, int(20_000 * scale), F, start_frame=0, end_frame=40) for i in range(n_actors)]
    sky = model("sky", compose.SKY, int(100_000 * scale), 1, centre=(1.0, -2.0, 0.5), radius=40.0)
    with torch.no_grad():
        sky.xyz.mul_(20.0)
    models.append(sky)
    rots = torch.randn(n_actors, 4, device=DEV, generator=gen).requires_grad_(True)
    trans = (torch.randn(n_actors, 3, device=DEV, generator=gen) * 10).requires_grad_(True)
    flip = {m.name: torch.rand(m.n, device=DEV, generator=gen) < 0.5 for m in models if m.kind == compose.ACTOR}
    N = sum(m.n for m in models)
    ups = [torch.randn((N,) + s, device=DEV, generator=gen) for s in ((3,), (4,), (3,), (1,), (K, 3))]
    return models, rots, trans, flip, ups


def leaves(models, rots, trans):
    from street_crafter_amd import compose
    return [getattr(m, a) for m in models for a in compose._RAW] + [rots, trans]


def torch_forward(models, rots, trans, flip, flip_q):
    """the reference's sequence, op for op: street_gaussian_model.py:243-407"""
    import torch
    import torch.nn.functional as Fn
    from street_crafter_amd import compose, scene_io
    bg = [m for m in models if m.kind == compose.STATIC]
    actors = [m for m in models if m.kind == compose.ACTOR]
    sky = [m for m in models if m.kind == compose.SKY]
    if actors:                                                                       # parse_camera :243-271
        obj_rots = torch.cat([rots[i].expand(m.n, -1) for i, m in enumerate(actors)], dim=0)
        obj_trans = torch.cat([trans[i].unsqueeze(0).expand(m.n, -1) for i, m in enumerate(actors)], dim=0)
        flip_mask = torch.cat([flip[m.name] for m in actors], dim=0)
    scal = [torch.exp(m.scaling) for m in bg + actors] + [torch.clamp(torch.exp(m.scaling), max=m.radius) for m in sky]
    rot = [Fn.normalize(m.rotation) for m in bg]
    xyz = [m.xyz for m in bg]
    if actors:
        local = torch.cat([Fn.normalize(m.rotation) for m in actors], dim=0).clone()    # :304-321
        flipped = local[flip_mask]
        if len(flipped) > 0:
            local[flip_mask] = scene_io.quaternion_raw_multiply(flip_q, flipped)
        rot.append(Fn.normalize(scene_io.quaternion_raw_multiply(obj_rots, local)))
        xl = torch.cat([m.xyz for m in actors], dim=0).clone()                           # :337-353
        xl[flip_mask, 1] *= -1
        xyz.append(torch.einsum("bij, bj -> bi", scene_io.quaternion_to_matrix(obj_rots), xl) + obj_trans)
    rot += [Fn.normalize(m.rotation) for m in sky]
    for m in sky:                                                                        # gaussian_model_sky.py:68-76
        centre = torch.tensor(m.centre, device=DEV)
        ratios = torch.linalg.norm(m.xyz - centre, dim=1, keepdim=True) / (2 * m.radius)
        xyz.append(torch.where(ratios < 1., centre + (m.xyz - centre) / ratios, m.xyz))
    feat = [torch.cat((m.features_dc, m.features_rest), dim=1) for m in bg]
    for m in actors:                                                                     # gaussian_model_actor.py:67-76
        t = m.fourier_scale * (FRAME - m.start_frame) / (m.end_frame - m.start_frame)
        base = scene_io.idft(t, F)[0].to(DEV, non_blocking=True)
        dc = torch.sum(m.features_dc * base[..., None], dim=1, keepdim=True)
        feat.append(torch.cat((dc, m.features_rest), dim=1))
    feat += [torch.cat((m.features_dc, m.features_rest), dim=1) for m in sky]
    opac = [torch.sigmoid(m.opacity) for m in bg + actors + sky]
    return (torch.cat(xyz, dim=0), torch.cat(rot, dim=0), torch.cat(scal, dim=0), torch.cat(opac, dim=0),
            torch.cat(feat, dim=0))


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), host


def measure(fn, iters, warmup):
    d, h = [], []
    for i in range(warmup + iters):
        dev, host = timed(fn)
        if i >= warmup:
            d.append(dev); h.append(host)
    q = statistics.quantiles(d, n=10) if len(d) >= 10 else [min(d)] * 9
    return {"device_ms": statistics.median(d), "device_ms_p10": q[0], "device_ms_p90": q[-1],
            "host_ms": statistics.median(h)}


def count_ops(fn):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if not any(v in str(func) for v in VIEWS):
                Count.n += 1
            return func(*args, **(kwargs or {}))
    with Count():
        fn()
    return Count.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--actors", type=int, default=32)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks every sub-model (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_compose.py measures on the GPU: none found")
    from street_crafter_amd import _ctypes_binding as cb
    from street_crafter_amd import _lib, compose
    lib = _lib.load()
    models, rots, trans, flip, ups = make_scene(a.actors, scale=a.scale)
    params = leaves(models, rots, trans)
    flip_q = torch.tensor(compose.DEFAULT_FLIP_Q, device=DEV)
    N = ups[0].shape[0]

    def clear():
        for p in params:
            p.grad = None

    def torch_step():
        clear()
        torch.autograd.backward(torch_forward(models, rots, trans, flip, flip_q), ups)

    def hip_step():
        clear()
        outs = compose.compose_frame(models, rots, trans, FRAME, flip=flip)[:5]
        torch.autograd.backward(outs, ups)

    r = {"rows": N, "sub_models": len(models), "actors": a.actors, "K": K, "fourier_dim": F}
    r["torch_before"] = measure(torch_step, a.iters, a.warmup)
    ref_grads = [p.grad.clone() for p in params]
    r["hip"] = measure(hip_step, a.iters, a.warmup)
    worst = 0.0
    for g, p in zip(ref_grads, params):
        if g.numel():
            worst = max(worst, float((g - p.grad).abs().max() / g.abs().max().clamp_min(1e-30)))
    r["max_rel_difference_of_gradients"] = worst
    r["torch_after"] = measure(torch_step, a.iters, a.warmup)
    r["torch_before"]["ops"] = count_ops(torch_step)
    n_launch = -(-sum(1 for m in models if m.n) // lib.sc_compose_max_segments())
    r["hip"]["launches"] = {"forward_kernels": n_launch, "backward_kernels": n_launch, "memsets": 2 if a.actors else 0}
    r["hip"]["ops"] = count_ops(hip_step)

    # the two entry points alone, on a prebuilt table
    with torch.no_grad():
        plan = compose.plan_frame(models, {m.name: i for i, m in enumerate(m for m in models if m.kind == compose.ACTOR)})
        lists = [[getattr(m, k).detach() for m in models] for k in compose._RAW]
        none = torch.empty(0, dtype=torch.uint8, device=DEV)
        flips = [flip[m.name].view(torch.uint8) if m.name in flip else none for m in models]
        ranges = [v for s in plan.segments for v in (s["start"], s["end"])]
        fparams = []
        for m in models:
            b = [0.0] * 8
            if m.kind == compose.ACTOR:
                from street_crafter_amd import scene_io
                t = m.fourier_scale * (FRAME - m.start_frame) / (m.end_frame - m.start_frame)
                b[:F] = scene_io.idft(float(t), F)[0].tolist()
            fparams += b + [float(v) for v in m.centre] + [float(m.radius)]
        table = cb._compose_table(*lists, flips, ranges, [s["kind"] for s in plan.segments],
                                  [max(s["pose_row"], 0) for s in plan.segments], fparams)
        import ctypes
        fq = (ctypes.c_float * 4)(*compose.DEFAULT_FLIP_Q)
        new = lambda *s: torch.empty(s, device=DEV)
        outs = [new(N, 3), new(N, 4), new(N, 3), new(N, 1), new(N, K, 3)]
        grads = [[torch.empty_like(t) for t in lst] for lst in lists]
        gtab = (_lib.ComposeGrads * len(models))()
        for k, row in enumerate(gtab):
            row.xyz, row.scaling, row.rotation, row.opacity, row.features_dc, row.features_rest = \
                (lst[k].data_ptr() for lst in grads)
        g_rots, g_trans = new(max(a.actors, 1), 4), new(max(a.actors, 1), 3)
        stream = torch.cuda.current_stream().cuda_stream
        S, A = len(models), a.actors
        rp, tp = (rots.data_ptr(), trans.data_ptr()) if A else (None, None)

        def fwd():
            rc = lib.sc_compose_fwd(table, S, N, K, rp, tp, A, fq, *(o.data_ptr() for o in outs), stream)
            assert rc == 0, rc

        def bwd():
            rc = lib.sc_compose_bwd(table, gtab, S, N, K, rp, tp, A, fq, *(u.data_ptr() for u in ups),
                                    g_rots.data_ptr() if A else None, g_trans.data_ptr() if A else None, stream)
            assert rc == 0, rc
        raw = sum(t.numel() for lst in lists for t in lst) * 4
        out_b = sum(o.numel() for o in outs) * 4
        small = sum(t.numel() for lst in lists[:4] for t in lst) * 4
        kern = {}
        for name, fn, nbytes in (("forward", fwd, raw + out_b), ("backward", bwd, out_b + small + raw)):
            m = measure(fn, a.iters, a.warmup)
            m["bytes"] = nbytes
            m["bytes_per_s"] = nbytes / (m["device_ms"] * 1e-3)
            m["frac_hbm"] = m["bytes_per_s"] / HBM_PEAK
            kern[name] = m
        r["kernels"] = kern
    r["speedup_device_vs_before"] = r["torch_before"]["device_ms"] / r["hip"]["device_ms"]
    r["speedup_device_vs_after"] = r["torch_after"]["device_ms"] / r["hip"]["device_ms"]
    r["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(r), flush=True)
    for name in ("torch_before", "hip", "torch_after"):
        m = r[name]
        print(f"{name:<14}{m['device_ms']:10.3f} ms dev  (p10 {m['device_ms_p10']:.3f}, p90 {m['device_ms_p90']:.3f})"
              f"{m['host_ms']:10.3f} ms host   ops {m.get('ops', '-')}")
    for name, m in r["kernels"].items():
        print(f"kernel {name:<9}{m['device_ms']:8.3f} ms  {m['bytes'] / 1e9:6.3f} GB  {m['bytes_per_s'] / 1e12:5.2f} TB/s "
              f"({100 * m['frac_hbm']:.1f} % of 8 TB/s)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
