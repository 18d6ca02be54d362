"""Times the fused frame tail (street_crafter_amd/frame_tail.py) against the plain-torch restatement of the reference's
lines (street_gaussian_renderer.py:282-300, :116-132, color_correction.py:135-138) on the same GPU.

    python tools/bench_frame_tail.py [--iters 200] [--warmup 20] [--out profiles/frame_tail_ab.txt]

Cases: 1066x1600 and 1280x1920, D = 4, the sky as the `[..., :3]` view of a 4-channel sky render, with the affine.  The
upstream gradient is a fixed random g (of rgb) and h (of depth).  Per case, in ONE process and in this order: torch, fused,
torch again (the two torch rows bracket the fused one, so that a drifting clock or a busy host shows as a difference
between them) -- forward, backward and forward + backward in ms through autograd (HIP events, median over --iters after
--warmup).  Then the host entries, back to back: the binding's forward and backward entry points called without autograd,
per-call time from one event pair around --iters calls, against the algorithmic bytes of each launch and their share of
8 TB/s.  A call allocates its outputs and the backward's workspace as well as launching, so where the host is the slower
side the figure is an upper bound on the kernels' own time, not that time.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # B/s, MI355X spec


def torch_tail(render_colors, render_alphas, sky_colors, affine):
    """The reference's lines as they stand (cfg.mode == 'train')."""
    import torch
    rendered_color = render_colors[..., :-1]
    rendered_depth = render_colors[..., -1:] / render_alphas.clamp(min=1e-10)
    rgb = rendered_color[0].permute(2, 0, 1)
    acc = render_alphas[..., 0]
    depth = rendered_depth[..., 0]
    sky_rgb = sky_colors[..., :-1][0].permute(2, 0, 1)
    rgb = rgb + sky_rgb * (1 - acc)
    rgb = torch.einsum('ij, jhw -> ihw', affine[:3, :3], rgb) + affine[:3, 3].unsqueeze(-1).unsqueeze(-1)
    return rgb, acc, depth


def fused_tail(render_colors, render_alphas, sky_colors, affine):
    from street_crafter_amd.frame_tail import frame_tail
    return frame_tail(render_colors, render_alphas, sky_colors[..., :3], affine)


def algorithmic_bytes(H, W):
    """(forward, backward) bytes the launches must move for D = 4, a sky of 3 used channels and the affine: the forward
    reads colours (16 B/pixel), alpha (4), sky (12) and writes rgb (12) and depth (4); the backward reads the same inputs
    plus g (12) and h (4) and writes the gradients of colours (16), alpha (4) and sky (12).  (The sky view's cache lines
    carry its unused fourth channel: 4 B/pixel more in each direction of each pass, not counted.)"""
    P = H * W
    return 48 * P, 80 * P


def make_inputs(H, W, dev):
    import torch
    gen = torch.Generator(device=dev).manual_seed(0)
    rc = 1.2 * torch.rand(1, H, W, 4, device=dev, generator=gen)
    ra = torch.rand(1, H, W, 1, device=dev, generator=gen)
    rc[..., 3:] = ra * (1 + 60 * torch.rand(1, H, W, 1, device=dev, generator=gen))
    sky = 1.2 * torch.rand(1, H, W, 4, device=dev, generator=gen)
    A = torch.eye(3, 4, device=dev) + 0.1 * torch.randn(3, 4, device=dev, generator=gen)
    g = torch.randn(3, H, W, device=dev, generator=gen) / (H * W)
    h = 0.01 * torch.randn(1, H, W, device=dev, generator=gen) / (H * W)
    return rc, ra, sky, A, g, h


def time_autograd(tail, inputs, iters, warmup):
    import torch
    rc0, ra0, sky0, A0, g, h = inputs
    fw, bw, tot = [], [], []
    for i in range(warmup + iters):
        rc, ra, sky, A = (t.detach().clone().requires_grad_(True) for t in (rc0, ra0, sky0, A0))
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        rgb, _acc, depth = tail(rc, ra, sky, A)
        e[1].record()
        torch.autograd.backward([rgb, depth], [g, h])
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
            tot.append(e[0].elapsed_time(e[2]))
    return statistics.median(fw), statistics.median(bw), statistics.median(tot)


def time_kernels(inputs, iters, warmup):
    """Per-call ms of the forward entry and of the backward entry (one launch + the finishing launch), back to back: the
    allocation of the outputs and the workspace included, so an upper bound on the kernels."""
    import torch
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    rc, ra, sky4, A, g, h = inputs
    _, H, W, _ = rc.shape
    sky = sky4[..., :3]
    st = [sky.stride(3), sky.stride(1), sky.stride(2)]
    b, stream = _lib.binding(), R._stream(rc)
    out = []
    for call in (lambda: b.frame_tail_fwd(rc, False, ra, sky, st, A, H, W, False, stream),
                 lambda: b.frame_tail_bwd(rc, False, ra, sky, st, A, H, W, g, h, True, True, True, False, True, stream)):
        for _ in range(warmup):
            assert call()[0] == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_tail_ab.txt"))
    a = ap.parse_args()
    import torch
    from street_crafter_amd import _lib
    _lib.load()
    dev = "cuda:0"
    lines = [f"tools/bench_frame_tail.py --iters {a.iters} --warmup {a.warmup}", f"device: {torch.cuda.get_device_name(0)}",
             "forward + backward through autograd, ms (median); D = 4, sky = [..., :3] of a 4-channel render, affine given",
             f"{'case':<12}{'path':<16}{'fwd':>9}{'bwd':>9}{'fwd+bwd':>10}"]
    kern = [f"host entries, back to back: ms per call (mean of {a.iters} calls, output allocation included: an upper bound "
            "on the kernels), algorithmic bytes and share of 8 TB/s",
            f"{'case':<12}{'entry':<22}{'ms':>9}{'MB':>9}{'TB/s':>8}{'% HBM':>8}"]
    for (H, W) in ((1066, 1600), (1280, 1920)):
        inputs = make_inputs(H, W, dev)
        name = f"{H}x{W}"
        rows = [("torch (before)", time_autograd(torch_tail, inputs, a.iters, a.warmup)),
                ("fused", time_autograd(fused_tail, inputs, a.iters, a.warmup)),
                ("torch (after)", time_autograd(torch_tail, inputs, a.iters, a.warmup))]
        for path, (f, b, t) in rows:
            lines.append(f"{name:<12}{path:<16}{f:9.3f}{b:9.3f}{t:10.3f}")
        t_torch = 0.5 * (rows[0][1][2] + rows[2][1][2])
        lines.append(f"{name:<12}fused / torch fwd+bwd: {rows[1][1][2] / t_torch:.2f} "
                     f"(torch / fused {t_torch / rows[1][1][2]:.2f}x)")
        for entry, ms, nbytes in zip(("sc_frame_tail_fwd", "sc_frame_tail_bwd"), time_kernels(inputs, a.iters, a.warmup),
                                     algorithmic_bytes(H, W)):
            rate = nbytes / (ms * 1e-3)
            kern.append(f"{name:<12}{entry:<22}{ms:9.4f}{nbytes / 1e6:9.1f}{rate / 1e12:8.2f}{100 * rate / HBM_PEAK:8.1f}")
    text = "\n".join(lines + [""] + kern) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
