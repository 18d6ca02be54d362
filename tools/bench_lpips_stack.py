"""Times the perceptual loss with its convolution stack in HIP (street_crafter_amd/lpips_stack.py) against the same
criterion with the stack on torch, by the protocol of tools/bench_lpips.py (whose helpers it uses): one process, forward +
backward to the image, HIP events round the whole step, the median over --iters steps after --warmup, and the time inside
the convolution stack taken the same way ("stack ms").  Order of the blocks:

    plain torch | torch stack: both images, cached target | hip stack: both, target | torch stack again | plain torch

The yardstick is the torch stack measured before and after the hip blocks in this process.  The hip stack counts as
faster only if its stack ms is below the smaller of the two torch blocks by more than those two differ from each other.

    python tools/bench_lpips_stack.py [--iters 50] [--warmup 5] [--sizes 1600x1066,1920x1280] [--out FILE.json]
    python tools/bench_lpips_stack.py --layers      # also: every stage of the hip stack on its own, ms and TFLOP/s
    python tools/bench_lpips_stack.py --stages-only # that table alone
    python tools/bench_lpips_stack.py --against-torch   # no timing: every hip stage against torch's float32 stage and,
                                                        # where the device runs it, torch's float64 stage, on the same input
    python tools/bench_lpips_stack.py --steps-only N [--sizes ...]   # N hip steps (cached target) and nothing else:
                                                                     # the workload for a kernel trace taken from outside

FLOP of a convolution: 2 * Cout * oh * ow * Cin * kh * kw, forward and data gradient alike; the peak they are set against
is the part's 157.3 TFLOP/s of exact-f32 MFMA.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench_lpips as B  # noqa: E402

PEAK_TFLOPS = 157.3
FORMS = ("plain_before", "torch_both_before", "torch_target_before", "hip_both", "hip_target", "torch_both_after",
         "torch_target_after", "plain_after")


def make_scene(Hh, Ww, dev):
    import torch
    from street_crafter_amd import lpips as L
    g = torch.Generator().manual_seed(Hh)
    gt = torch.rand(3, Hh, Ww, generator=g).to(dev)
    render = (gt + 0.1 * torch.randn(3, Hh, Ww, generator=g).to(dev)).clamp(0, 1)
    mask = (torch.rand(1, Hh, Ww, generator=g) >= B.MASK_FALSE).to(dev)
    net, lin = B.make_weights(dev)
    return gt, render, mask, net, lin, L


def run_case(Hh, Ww, iters, warmup, dev):
    import torch
    gt, render, mask, net, lin, L = make_scene(Hh, Ww, dev)
    maskf = mask.to(torch.float32)
    plain = B.PlainTorch(net, lin, L.MEAN, L.STD, dev)
    crit = L.LPIPS.from_state_dicts("alex", net, lin)

    def step_plain(marks):
        img = render.clone().requires_grad_(True)
        plain(img, gt, maskf, marks).backward()
        return img.grad

    def crit_step(second):
        def step(marks):
            img = render.clone().requires_grad_(True)
            if marks is None:
                crit(img, second, mask).backward()
            else:                                   # the same call with the stack wrapped
                stack = crit._stack
                crit._stack = lambda z: marks.around_stack(z, stack)
                try:
                    crit(img, second, mask).backward()
                finally:
                    crit._stack = stack
            return img.grad
        return step

    res = {"height": Hh, "width": Ww}
    grads = {}
    for form in FORMS:
        if form.startswith("plain"):
            res[form] = B.timed_steps(step_plain, iters, warmup)
            continue
        route, second = form.split("_")[0], form.split("_")[1]
        crit.set_stack(route)
        other = gt if second == "both" else crit.target(gt, mask)
        res[form] = B.timed_steps(crit_step(other), iters, warmup)
        grads[form] = crit_step(other)(None)
        if route == "hip":
            res[form]["two_runs_equal"] = bool(torch.equal(grads[form], crit_step(other)(None)))
    ref = grads["torch_both_before"]
    res["grad_rel_diff_hip_vs_torch"] = float((grads["hip_both"] - ref).norm() / ref.norm())
    res["grad_equal_hip_target_vs_both"] = bool(torch.equal(grads["hip_both"], grads["hip_target"]))
    # the verdict, per form, on the stack ms
    for second in ("both", "target"):
        a, b = res[f"torch_{second}_before"]["stack_ms"], res[f"torch_{second}_after"]["stack_ms"]
        h = res[f"hip_{second}"]["stack_ms"]
        res[f"verdict_{second}"] = {"torch_stack_ms": [a, b], "hip_stack_ms": h, "torch_blocks_differ_ms": round(abs(a - b), 4),
                                    "hip_below_smaller_torch_ms": round(min(a, b) - h, 4),
                                    "hip_faster": bool(min(a, b) - h > abs(a - b))}
    return res


def stage_times(Hh, Ww, iters, warmup, dev):
    """Every stage of the hip stack on its own (one kernel each), forward and backward: median ms over `iters` calls
    between HIP events after `warmup`, and for the convolutions the achieved TFLOP/s."""
    import torch
    from street_crafter_amd import lpips_stack as S
    gt, render, mask, net, lin, L = make_scene(Hh, Ww, dev)
    crit = L.LPIPS.from_state_dicts("alex", net, lin, stack="hip")
    packed = S.pack(crit.layers)
    x = L.prepare(render, mask)[0]
    gen = torch.Generator().manual_seed(1)

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    rows, i, n_conv = [], 0, 0
    while i < len(crit.layers):
        layer = crit.layers[i]
        if isinstance(layer, L.Conv):
            pk = packed[i]
            n_conv += 1
            y = S.conv_relu(x, pk)
            g = torch.randn(y.shape, generator=gen).to(dev)
            hw = tuple(x.shape[1:])
            flop = 2.0 * pk.cout * y.shape[1] * y.shape[2] * pk.cin * pk.kernel[0] * pk.kernel[1]
            for name, fn in ((f"conv{n_conv} forward", lambda: S.conv_relu(x, pk)),
                             (f"conv{n_conv} data gradient" + ("" if pk.dgrad is not None else " (gather)"),
                              lambda: S.conv_dgrad(g, y, pk, hw))):
                ms = timed(fn)
                rows.append({"stage": name, "shape": f"{pk.cin}x{hw[0]}x{hw[1]} -> {pk.cout}x{y.shape[1]}x{y.shape[2]}, "
                                                      f"{pk.kernel[0]}x{pk.kernel[1]}/{pk.stride[0]}",
                             "ms": round(ms, 4), "gflop": round(flop / 1e9, 2), "tflops": round(flop / ms / 1e9, 1),
                             "of_peak": round(flop / ms / 1e9 / PEAK_TFLOPS, 3)})
            i += 2
        else:
            k, s = tuple(layer.kernel), tuple(layer.stride)
            y = S.max_pool(x, k, s)
            g = torch.randn(y.shape, generator=gen).to(dev)
            for name, fn in ((f"pool {k[0]}x{k[1]}/{s[0]} forward", lambda: S.max_pool(x, k, s)),
                             (f"pool {k[0]}x{k[1]}/{s[0]} backward", lambda: S.max_pool_bwd(g, x, k, s))):
                rows.append({"stage": name, "shape": f"{tuple(x.shape)} -> {tuple(y.shape)}", "ms": round(timed(fn), 4)})
            i += 1
        x = y
    return rows


def against_torch(Hh, Ww, dev):
    """Every stage of the hip stack against the torch stage on the same input: the convolutions' forward and data
    gradient against torch in float32 and (when the device's convolution library takes float64) in float64, the pools
    for equality; then the whole term's image gradient, hip against torch and torch against itself."""
    import torch
    import torch.nn.functional as F
    from street_crafter_amd import lpips_stack as S
    gt, render, mask, net, lin, L = make_scene(Hh, Ww, dev)
    crit = L.LPIPS.from_state_dicts("alex", net, lin, stack="hip")
    packed = S.pack(crit.layers)
    x = L.prepare(render, mask)[0]
    gen = torch.Generator().manual_seed(1)

    def rel(a, b):
        return f"({float((a - b).abs().max() / b.abs().max()):.2e}, {float((a - b).norm() / b.norm()):.2e})"

    i = 0
    while i < len(crit.layers):
        layer = crit.layers[i]
        if isinstance(layer, L.Conv):
            pk = packed[i]
            y = S.conv_relu(x, pk)
            g = torch.randn(y.shape, generator=gen).to(dev)
            gi = S.conv_dgrad(g, y, pk, tuple(x.shape[1:]))
            xt = x.clone().requires_grad_(True)
            yt = F.relu(F.conv2d(xt[None], layer.weight, layer.bias, layer.stride, layer.padding))[0]
            (git,) = torch.autograd.grad(yt, xt, g)
            line = (f"    conv {tuple(x.shape)} -> {tuple(y.shape)}: hip vs torch f32 forward {rel(y, yt.detach())} "
                    f"data gradient {rel(gi, git)}")
            try:
                x64 = x.double().requires_grad_(True)
                pre64 = F.conv2d(x64[None], layer.weight.double(), layer.bias.double(), layer.stride, layer.padding)[0]
                y64 = F.relu(pre64).detach()
                g64 = torch.where(y > 0, g.double(), torch.zeros((), dtype=torch.float64, device=dev))    # the same mask
                (gi64,) = torch.autograd.grad(pre64, x64, g64)
                line += (f" | vs torch f64: forward hip {rel(y.double(), y64)} torch f32 {rel(yt.detach().double(), y64)}, "
                         f"data gradient hip {rel(gi.double(), gi64)} torch f32 {rel(git.double(), gi64)}")
            except RuntimeError as e:
                line += f" | torch f64 convolution not available here ({str(e).splitlines()[0][:60]})"
            print(line, flush=True)
            i += 2
        else:
            k, s = tuple(layer.kernel), tuple(layer.stride)
            y = S.max_pool(x, k, s)
            xt = x.clone().requires_grad_(True)
            yt = F.max_pool2d(xt[None], k, s)[0]
            g = torch.randn(y.shape, generator=gen).to(dev)
            (git,) = torch.autograd.grad(yt, xt, g)
            print(f"    pool {tuple(x.shape)}: forward equal {torch.equal(y, yt.detach())}, backward equal "
                  f"{torch.equal(S.max_pool_bwd(g, x, k, s), git)}", flush=True)
            i += 1
        x = y

    def image_gradient():
        img = render.clone().requires_grad_(True)
        crit(img, gt, mask).backward()
        return img.grad

    crit.set_stack("torch")
    a, b = image_gradient(), image_gradient()
    crit.set_stack("hip")
    print(f"    whole term, image gradient: torch vs torch {rel(b, a)}, hip vs torch {rel(image_gradient(), a)}", flush=True)


def print_stages(rows):
    for row in rows:
        rate = f"  {row['gflop']:6.2f} GFLOP  {row['tflops']:6.1f} TFLOP/s  {100 * row['of_peak']:5.1f} % of peak" if "tflops" in row else ""
        print(f"    {row['stage']:32s} {row['ms']:7.4f} ms{rate}   {row['shape']}", flush=True)


def steps_only(Hh, Ww, n, dev):
    import torch
    gt, render, mask, net, lin, L = make_scene(Hh, Ww, dev)
    crit = L.LPIPS.from_state_dicts("alex", net, lin, stack="hip")
    target = crit.target(gt, mask)
    for _ in range(n):
        img = render.clone().requires_grad_(True)
        crit(img, target, mask).backward()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1600x1066,1920x1280")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--stages-only", action="store_true", help="the per-stage table and nothing else")
    ap.add_argument("--steps-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--against-torch", action="store_true", help="accuracy of every stage against torch, no timing")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips_stack: no GPU; this tool measures on a device only")
    dev = torch.device("cuda", 0)
    results = []
    for size in args.sizes.split(","):
        Ww, Hh = (int(v) for v in size.split("x"))
        if args.steps_only:
            steps_only(Hh, Ww, args.steps_only, dev)
            print(f"{Ww}x{Hh}: {args.steps_only} hip steps done")
            continue
        if args.against_torch:
            print(f"{Ww}x{Hh}: (max |a - b| / max |b|, relative L2)")
            against_torch(Hh, Ww, dev)
            continue
        if args.stages_only:
            print(f"{Ww}x{Hh}:")
            print_stages(stage_times(Hh, Ww, args.iters, args.warmup, dev))
            continue
        r = run_case(Hh, Ww, args.iters, args.warmup, dev)
        print(f"{Ww}x{Hh}: hip vs torch gradient rel diff {r['grad_rel_diff_hip_vs_torch']:.2e}, hip target == both: "
              f"{r['grad_equal_hip_target_vs_both']}")
        for form in FORMS:
            t = r[form]
            split = f"  stack {t['stack_ms']:.3f} ms + rest {t['rest_ms']:.3f} ms" if "stack_ms" in t else ""
            rep = f"  two runs equal: {t['two_runs_equal']}" if "two_runs_equal" in t else ""
            print(f"  {form:20s} {t['ms']:8.3f} ms  [{t['ms_min']:.3f}, {t['ms_max']:.3f}]{split}  peak "
                  f"{t['peak_bytes'] / 1e6:.1f} MB{rep}", flush=True)
        for second in ("both", "target"):
            v = r[f"verdict_{second}"]
            print(f"  {second:6s}: torch stack {v['torch_stack_ms'][0]:.3f} / {v['torch_stack_ms'][1]:.3f} ms (differ by "
                  f"{v['torch_blocks_differ_ms']:.3f}), hip stack {v['hip_stack_ms']:.3f} ms -> "
                  f"{'faster' if v['hip_faster'] else 'NOT faster'} by the rule above", flush=True)
        if args.layers:
            r["stages"] = stage_times(Hh, Ww, args.iters, args.warmup, dev)
            print_stages(r["stages"])
        results.append(r)
    if args.out and results:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"iters": args.iters, "warmup": args.warmup, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
