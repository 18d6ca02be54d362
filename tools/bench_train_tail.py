"""Times the tail of the training step on the GPU: the fused Adam step (street_crafter_amd.optim.step_many) against the
reference's loop of torch.optim.Adam.step() per sub-model (its default route), and the fused densification statistics
(densify_stats.accumulate_fused) against the torch mirror DensificationStats (the reference's boolean-mask indexing).

    python tools/bench_train_tail.py [--iters 30] [--warmup 5] [--out FILE.json]

Scenes: one background of 1 M Gaussians with 16 SH bases (xyz 3, f_dc 3, f_rest 45, opacity 1, scaling 3, rotation 4,
semantic 0 values each: 59 M parameters), plus 0, 8 and 32 actors of 20 k Gaussians each, plus a 100 k sky model; one
optimizer with seven groups per sub-model, as gaussian_model.py:293-305.
Both routes of a pair run in the same process on the same GPU, alternating iteration by iteration.  Per route and step:
  device ms   HIP events around the call (median over --iters after --warmup; includes the gaps a host-bound route leaves)
  host ms     host clock from the call to its return, before any synchronise: what the Python thread is busy for
For the fused Adam the compulsory traffic is 28 B per element (read p, g, m, v; write p, m, v); its rate is that over
the device time, also as a fraction of 8 TB/s.  The kernel split comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_train_tail.py --iters 10` run.
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
ROW_SHAPES = (("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("opacity", (1,)), ("scaling", (3,)),
              ("rotation", (4,)), ("semantic", (0,)))
LRS = (1.6e-4, 2.5e-3, 2.5e-3 / 20, 5e-2, 5e-3, 1e-3, 1e-2)


def sub_models(n_actors):
    return [1_000_000] + [20_000] * n_actors + [100_000]


def make_optimizers(cls, sizes, seed):
    import torch
    gen = torch.Generator(device=DEV).manual_seed(seed)
    opts = []
    for n in sizes:
        groups = []
        for (name, tail), lr in zip(ROW_SHAPES, LRS):
            p = torch.nn.Parameter(torch.randn((n,) + tail, device=DEV, generator=gen))
            p.grad = torch.randn((n,) + tail, device=DEV, generator=gen) * 1e-3
            groups.append({"params": [p], "lr": lr, "name": name})
        opts.append(cls(groups, lr=0.0, eps=1e-15))
    return opts


def timed(fn):
    """-> (device ms, host ms) of one call."""
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


def interleaved(routes, iters, warmup):
    """routes: name -> callable; alternates them per iteration -> name -> {"device_ms", "host_ms", spreads}."""
    samples = {name: ([], []) for name in routes}
    for i in range(warmup + iters):
        for name, fn in routes.items():
            d, h = timed(fn)
            if i >= warmup:
                samples[name][0].append(d)
                samples[name][1].append(h)
    out = {}
    for name, (d, h) in samples.items():
        q = statistics.quantiles(d, n=10) if len(d) >= 10 else [min(d)] * 9
        out[name] = {"device_ms": statistics.median(d), "device_ms_p10": q[0], "device_ms_p90": q[-1],
                     "host_ms": statistics.median(h)}
    return out


def bench_adam(n_actors, iters, warmup):
    import torch
    from street_crafter_amd import optim
    sizes = sub_models(n_actors)
    hip = make_optimizers(optim.Adam, sizes, 0)
    ref = make_optimizers(torch.optim.Adam, sizes, 0)

    def torch_route():
        for o in ref:                      # street_gaussian_model.py:467-484 (zero_grad left out on both sides)
            o.step()

    r = interleaved({"hip": lambda: optim.step_many(hip), "torch": torch_route}, iters, warmup)
    numel = sum(p.numel() for o in hip for g in o.param_groups for p in g["params"])
    r["numel"], r["tensors"] = numel, 7 * len(sizes)
    r["hip"]["bytes"] = 28 * numel
    r["hip"]["bytes_per_s"] = 28 * numel / (r["hip"]["device_ms"] * 1e-3)
    r["hip"]["frac_hbm"] = r["hip"]["bytes_per_s"] / HBM_PEAK
    r["torch"]["bytes_per_s_at_28B"] = 28 * numel / (r["torch"]["device_ms"] * 1e-3)
    r["speedup_device"] = r["torch"]["device_ms"] / r["hip"]["device_ms"]
    # the two routes have walked the same trajectory (same seeds): report how far apart they ended
    worst = 0.0
    for a, b in zip(hip, ref):
        for ga, gb in zip(a.param_groups, b.param_groups):
            pa, pb = ga["params"][0].detach(), gb["params"][0].detach()
            if pa.numel():
                worst = max(worst, float((pa - pb).abs().max() / pb.abs().max().clamp_min(1e-30)))
    r["max_rel_difference_of_parameters"] = worst
    return r


def bench_stats(n_actors, iters, warmup, W=1600, H=1066):
    import torch
    from street_crafter_amd import densify_stats as DS
    sizes = sub_models(n_actors)[:-1]                  # the sky model has its own render and call: one segment
    ranges, start = {}, 0
    for k, n in enumerate(sizes):
        ranges["background" if k == 0 else f"obj_{k:03d}"] = (start, start + n)
        start += n
    N = start
    gen = torch.Generator(device=DEV).manual_seed(1)
    vp = torch.zeros(1, N, 2, device=DEV)
    vp.grad = torch.randn(1, N, 2, device=DEV, generator=gen) * 1e-5
    vp.absgrad = vp.grad.abs() * 1.5
    out = {"viewspace_points": vp, "visibility_filter": torch.rand(N, device=DEV, generator=gen) < 0.4,
           "radii": torch.randint(0, 60, (N,), device=DEV, generator=gen).float() / 1600.0}
    fused, mirror = DS.DensificationStats(ranges, device=DEV), DS.DensificationStats(ranges, device=DEV)
    r = interleaved({"hip": lambda: fused.accumulate_from_render_fused(out, W, H),
                     "torch": lambda: DS.accumulate_from_render(mirror, out, W, H)}, iters, warmup)
    r["rows"], r["segments"] = N, len(sizes)
    same = all(torch.equal(fused.denom[k], mirror.denom[k]) and torch.equal(fused.max_radii2D[k], mirror.max_radii2D[k])
               for k in ranges)
    r["denom_and_max_radii_identical"] = bool(same)
    r["speedup_device"] = r["torch"]["device_ms"] / r["hip"]["device_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--actors", type=int, nargs="*", default=[0, 8, 32])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_tail.py measures on the GPU: none found")
    from street_crafter_amd import _lib
    _lib.load()
    rows = []
    for n_actors in a.actors:
        for term, fn in (("adam", bench_adam), ("stats", bench_stats)):
            r = {"term": term, "actors": n_actors, **fn(n_actors, a.iters, a.warmup)}
            rows.append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    print(f"{'case':<22}{'hip dev ms':>11}{'p10':>8}{'p90':>8}{'host ms':>9}{'torch dev ms':>14}{'host ms':>9}{'x dev':>7}"
          f"{'TB/s':>7}{'%HBM':>6}")
    for r in rows:
        h, t = r["hip"], r["torch"]
        rate = f"{h['bytes_per_s'] / 1e12:7.2f}{100 * h['frac_hbm']:6.1f}" if "bytes_per_s" in h else ""
        print(f"{r['term'] + ' ' + str(r['actors']) + ' actors':<22}{h['device_ms']:11.3f}{h['device_ms_p10']:8.3f}"
              f"{h['device_ms_p90']:8.3f}{h['host_ms']:9.3f}{t['device_ms']:14.3f}{t['host_ms']:9.3f}"
              f"{r['speedup_device']:7.2f}{rate}")
    print("device:", torch.cuda.get_device_name(0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
