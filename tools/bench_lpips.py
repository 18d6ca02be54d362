"""Times the perceptual loss of a training step, forward + backward to the image, in three forms on the same GPU:

    (i)   plain torch: the reference's lpips(image * mask, gt * mask) restated here (z-score, the AlexNet stack, per tap
          normalise / difference / square / 1x1 convolution / spatial mean, cat and sum), autograd's backward
    (ii)  street_crafter_amd.lpips.LPIPS with both images: prep kernel, the stack on torch, the fused head
    (iii) the same with a cached target: the ground truth's network pass is not run

    python tools/bench_lpips.py [--iters 50] [--warmup 5] [--out FILE.json]

Cases: 1600x1066 and 1920x1280, random AlexNet-shaped weights (the timing does not depend on their values), a 30 %-false
mask.  All three forms run in one process; (i) is timed before and after the fused forms and both numbers are printed.
Per form: the median over --iters steps after --warmup, HIP events round the whole step.  For (i) and (ii) also the split
into the time inside the convolution stack (events round the stack's forward, both images, and round its backward, found
by hooks on the stack's input and outputs) and everything else, and the peak of allocated memory during a step above
what is allocated before it.
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

ALEX = [("conv", 3, 64, 11, 4, 2), ("relu",), ("pool", 3, 2), ("conv", 64, 192, 5, 1, 2), ("relu",), ("pool", 3, 2),
        ("conv", 192, 384, 3, 1, 1), ("relu",), ("conv", 384, 256, 3, 1, 1), ("relu",), ("conv", 256, 256, 3, 1, 1), ("relu",)]
TAPS = (2, 5, 8, 10, 12)
CHANNELS = (64, 192, 384, 256, 256)
MASK_FALSE = 0.3


def make_weights(dev, seed=0):
    """-> (torchvision-keyed state dict of random AlexNet-shaped weights, LPIPS-keyed lin weights)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    net, lin = {}, {}
    for pos, row in enumerate(ALEX):
        if row[0] == "conv":
            fan_in = row[1] * row[3] * row[3]
            net[f"features.{pos}.weight"] = ((torch.rand(row[2], row[1], row[3], row[3], generator=g) * 2 - 1)
                                             * (3.0 / fan_in) ** 0.5).to(dev)
            net[f"features.{pos}.bias"] = ((torch.rand(row[2], generator=g) * 2 - 1) * 0.05).to(dev)
    for k, c in enumerate(CHANNELS):
        lin[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g).to(dev)
    return net, lin


class PlainTorch:
    """Form (i).  `marks` (optional) receives events round the stack: forward start / end per image."""

    def __init__(self, net, lin, mean, std, dev):
        import torch
        self.net, self.lin = net, [lin[f"lin{k}.model.1.weight"] for k in range(len(CHANNELS))]
        self.mean = torch.tensor(mean, device=dev)[None, :, None, None]
        self.std = torch.tensor(std, device=dev)[None, :, None, None]

    def stack(self, x):
        import torch.nn.functional as F
        out = []
        for pos, row in enumerate(ALEX):
            if row[0] == "conv":
                x = F.conv2d(x, self.net[f"features.{pos}.weight"], self.net[f"features.{pos}.bias"], row[4], row[5])
            elif row[0] == "relu":
                x = F.relu(x, inplace=True)
            else:
                x = F.max_pool2d(x, row[1], row[2])
            if pos + 1 in TAPS:
                out.append(x)
        return out

    def taps(self, x, marks=None):
        z = (x - self.mean) / self.std
        if marks is not None:
            z = marks.around_stack(z, self.stack)
        else:
            z = self.stack(z)
        return z

    def __call__(self, image, gt, mask, marks=None):
        """Per tap: unit-normalise both feature maps over channels, square the difference, weight the channels with a
        1x1 convolution, average over the pixels; the per-tap numbers are joined and added."""
        import torch
        import torch.nn.functional as F
        taps_x = self.taps((image * mask).unsqueeze(0), marks)
        taps_y = self.taps((gt * mask).unsqueeze(0), marks)
        per_tap = []
        for xt, yt, weight in zip(taps_x, taps_y, self.lin):
            unit_x = xt / (xt.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            unit_y = yt / (yt.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            weighted = F.conv2d((unit_x - unit_y).pow(2), weight=weight, bias=None)
            per_tap.append(weighted.mean(dim=(2, 3), keepdim=True))
        return torch.cat(per_tap, dim=0).sum(dim=0, keepdim=True)


class StackMarks:
    """HIP events round the convolution stack: its forward directly, its backward through hooks (the backward of the
    stack starts when the first tap gradient arrives and ends when the gradient of its input is there)."""

    def __init__(self):
        self.fwd, self.bwd = [], []

    def _event(self):
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def around_stack(self, z, stack):
        first = []
        if z.requires_grad:
            z.register_hook(lambda g: self.bwd.append((first[0], self._event())) if first else None)
        e0 = self._event()
        taps = stack(z)
        self.fwd.append((e0, self._event()))
        if z.requires_grad:
            def on_tap_grad(g):
                if not first:
                    first.append(self._event())
            for t in taps:
                t.register_hook(on_tap_grad)
        return taps

    def ms(self):
        return sum(a.elapsed_time(b) for a, b in self.fwd + self.bwd)


def timed_steps(step, iters, warmup):
    """step(marks | None) runs forward + backward.  -> dict: total ms (median), stack ms (median, from a second set of
    steps with the marks on, so that the events do not sit in the timed steps), peak bytes above the starting level."""
    import torch
    for _ in range(warmup):
        step(None)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(None)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    stack = []
    for _ in range(max(iters // 5, 3)):
        marks = StackMarks()
        step(marks)
        torch.cuda.synchronize()
        if marks.fwd:
            stack.append(marks.ms())
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(None)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    total = statistics.median(times)
    out = {"ms": round(total, 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "peak_bytes": int(peak)}
    if stack:
        out["stack_ms"] = round(statistics.median(stack), 4)
        out["rest_ms"] = round(total - out["stack_ms"], 4)
    return out


def run_case(Hh, Ww, iters, warmup, dev):
    import torch
    from street_crafter_amd import lpips as L
    g = torch.Generator().manual_seed(Hh)
    gt = torch.rand(3, Hh, Ww, generator=g).to(dev)
    render = (gt + 0.1 * torch.randn(3, Hh, Ww, generator=g).to(dev)).clamp(0, 1)
    mask = (torch.rand(1, Hh, Ww, generator=g) >= MASK_FALSE).to(dev)
    maskf = mask.to(torch.float32)
    net, lin = make_weights(dev)
    plain = PlainTorch(net, lin, L.MEAN, L.STD, dev)
    crit = L.LPIPS.from_state_dicts("alex", net, lin)
    target = crit.target(gt, mask)

    def step_plain(marks):
        img = render.clone().requires_grad_(True)
        plain(img, gt, maskf, marks).backward()
        return img.grad

    def fused_step(second):
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

    res = {"height": Hh, "width": Ww, "target_bytes": target.nbytes()}
    res["plain_before"] = timed_steps(step_plain, iters, warmup)
    res["fused_both"] = timed_steps(fused_step(gt), iters, warmup)
    res["fused_target"] = timed_steps(fused_step(target), iters, warmup)
    res["plain_after"] = timed_steps(step_plain, iters, warmup)
    # the three forms compute the same thing
    gp, gb, gc = step_plain(None), fused_step(gt)(None), fused_step(target)(None)
    res["grad_rel_diff_fused_vs_plain"] = float((gb - gp).norm() / gp.norm())
    res["grad_equal_target_vs_both"] = bool(torch.equal(gb, gc))
    # (the convolutions' backward belongs to the library under torch; whether IT repeats bit for bit is told apart here)
    res["grad_equal_two_runs_both"] = bool(torch.equal(gb, fused_step(gt)(None)))
    res["grad_equal_two_runs_plain"] = bool(torch.equal(gp, step_plain(None)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1600x1066,1920x1280")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: no GPU; this tool measures on a device only")
    dev = torch.device("cuda", 0)
    results = []
    for size in args.sizes.split(","):
        Ww, Hh = (int(v) for v in size.split("x"))
        r = run_case(Hh, Ww, args.iters, args.warmup, dev)
        results.append(r)
        print(f"{Ww}x{Hh}: target cache {r['target_bytes'] / 1e6:.1f} MB, fused vs plain gradient rel diff "
              f"{r['grad_rel_diff_fused_vs_plain']:.2e}, target == both: {r['grad_equal_target_vs_both']}, two runs equal: "
              f"fused {r['grad_equal_two_runs_both']}, plain {r['grad_equal_two_runs_plain']}")
        for form in ("plain_before", "fused_both", "fused_target", "plain_after"):
            t = r[form]
            split = f"  stack {t['stack_ms']:.3f} ms + rest {t['rest_ms']:.3f} ms" if "stack_ms" in t else ""
            print(f"  {form:13s} {t['ms']:8.3f} ms  [{t['ms_min']:.3f}, {t['ms_max']:.3f}]{split}  peak "
                  f"{t['peak_bytes'] / 1e6:.1f} MB", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"iters": args.iters, "warmup": args.warmup, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
