"""Times sky_color (street_crafter_amd/cubemap.py: ray generation, mask, per-tap sigmoid, cube sampling, fill, clamp and
layout in one launch, with its backward) against a plain-torch restatement of SkyCubeMap.forward (sky_cubemap.py:92-127)
on the same GPU.

    python tools/bench_cubemap.py [--iters 50] [--warmup 5] [--resolution 1024] [--out FILE.json]

Cases: 1600x1066 and 1920x1280, a cube map of 6 x R x R x 3 logits, a 30 % sky mask, perturbed rays (training).
The torch path, written here: sigmoid of the whole map, rays from meshgrid + matmuls in fp32 (origin added and
subtracted, then normalised), boolean-mask indexing of the rays, bilinear sampling by index gathers (taps clamped to
their face: it is a timing baseline, not a seamless sampler), boolean-mask scatter into the fill image, permute, clamp.
It is timed before and after the fused path in the same process; both numbers are printed.

Per case: forward, backward and forward+backward in ms (HIP events, median over --iters after --warmup).  For the fused
path also the compulsory bytes per pixel and the fraction of 8 TB/s they amount to:
    forward   1 B mask + 12 B output per pixel; per masked pixel 8 B perturbation + 12 B of texels (about one new texel
              per sky pixel at R = 1024; the four taps of neighbouring pixels overlap)
    backward  1 B mask per pixel; per masked pixel 12 B upstream gradient + 8 B perturbation + 12 B texels + 4 taps x 12 B
              of atomic adds; plus the dense gradient's zero fill, 6 R R 3 x 4 B, which autograd's dense gradient makes
              compulsory whatever the mask covers (75 MB at R = 1024: it dominates)
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

HBM_PEAK = 8.0e12          # B/s, MI355X spec
SKY_SHARE = 0.3


def torch_rays(H, W, K, R, T, perturb):
    """graphics_utils.py:200-221 with the perturbation handed in."""
    import torch
    rays_o = -torch.matmul(R.T, T).squeeze()
    i, j = torch.meshgrid(torch.arange(W, dtype=torch.float32, device=K.device),
                          torch.arange(H, dtype=torch.float32, device=K.device), indexing="xy")
    xy1 = torch.stack([i + perturb[..., 0], j + perturb[..., 1], torch.ones_like(i)], dim=2)
    pixel_camera = torch.matmul(xy1, torch.linalg.inv(K).T)
    pixel_world = torch.matmul(pixel_camera - T.squeeze(), R)
    rays_d = pixel_world - rays_o[None, None]
    return rays_d / torch.norm(rays_d, dim=2, keepdim=True)


def torch_cube_sample(tex, d):
    """tex [6,R,R,3] activated, d [N,3] -> [N,3]: face rule + bilinear by index gathers, taps clamped to the face."""
    import torch
    Rr = tex.shape[1]
    x, y, z = d.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    isz = az > torch.maximum(ax, ay)
    isy = ~isz & (ay > ax)
    isx = ~isz & ~isy
    face = torch.where(isz, torch.where(z > 0, 4, 5), torch.where(isy, torch.where(y > 0, 2, 3), torch.where(x > 0, 0, 1)))
    ma = torch.where(isz, az, torch.where(isy, ay, ax))
    sc = torch.where(isx, torch.where(x > 0, -z, z), torch.where(isy, x, torch.where(z > 0, x, -x)))
    tc = torch.where(isy, torch.where(y > 0, z, -z), -y)
    fu = (sc / ma + 1) * (0.5 * Rr) - 0.5
    fv = (tc / ma + 1) * (0.5 * Rr) - 0.5
    x0, y0 = fu.floor(), fv.floor()
    fx, fy = (fu - x0)[:, None], (fv - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(0, Rr - 1), (y0 + 1).clamp(0, Rr - 1)
    x0, y0 = x0.clamp(0, Rr - 1), y0.clamp(0, Rr - 1)
    flat = tex.reshape(-1, tex.shape[-1])
    base = face * Rr
    t00, t01 = flat[(base + y0) * Rr + x0], flat[(base + y0) * Rr + x1]
    t10, t11 = flat[(base + y1) * Rr + x0], flat[(base + y1) * Rr + x1]
    return (t00 * (1 - fx) + t01 * fx) * (1 - fy) + (t10 * (1 - fx) + t11 * fx) * fy


def torch_sky(cube, K, R, T, H, W, mask, perturb, white):
    """sky_cubemap.py:92-127, training branch with a sky mask."""
    import torch
    rays_d = torch_rays(H, W, K, R, T, perturb)
    sky = (torch.ones if white else torch.zeros)((H, W, 3), device=cube.device, dtype=torch.float)
    sel = rays_d[mask]
    sky[mask] = torch_cube_sample(cube.sigmoid(), sel)
    return sky.permute(2, 0, 1).clamp(0., 1.)


def fused_bytes(H, W, Rr, share):
    P = H * W
    fwd = P * (1 + 12) + share * P * (8 + 12)
    bwd_pix = P * 1 + share * P * (12 + 8 + 12 + 4 * 12)
    return fwd, bwd_pix, 6 * Rr * Rr * 3 * 4


def time_path(path, H, W, Rr, iters, warmup):
    import numpy as np
    import torch
    from street_crafter_amd import cubemap
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(6, Rr, Rr, 3, device=dev, generator=g)
    # a sky band over the top 30 % of the image with a ragged lower edge, as a street scene has it
    rows = torch.arange(H, device=dev)[:, None] + 40 * torch.rand(1, W, device=dev, generator=g)
    mask = rows < SKY_SHARE * H + 20
    Kh = np.array([[2050.0 * W / 1920, 0, W / 2], [0, 2050.0 * W / 1920, H / 2], [0, 0, 1]])
    Rh = np.array([[0.96, 0.0, -0.28], [0.0, 1.0, 0.0], [0.28, 0.0, 0.96]])
    Th = np.array([310.0, -2.0, 1500.0])
    Kd, Rd, Td = (torch.tensor(v, dtype=torch.float32, device=dev) for v in (Kh, Rh, Th))
    gout = torch.randn(3, H, W, device=dev, generator=g)
    fw_t, bw_t, tot_t = [], [], []
    for i in range(warmup + iters):
        cube = logits.detach().clone().requires_grad_(True)
        perturb = torch.rand(H, W, 2, device=dev, generator=g)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        if path == "hip":
            img = cubemap.sky_color(cube, Kh, Rh, Th, H, W, sky_mask=mask, perturb=perturb, white_background=False)
        else:
            img = torch_sky(cube, Kd, Rd, Td, H, W, mask, perturb, False)
        e[1].record()
        img.backward(gout)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw_t.append(e[0].elapsed_time(e[1]))
            bw_t.append(e[1].elapsed_time(e[2]))
            tot_t.append(e[0].elapsed_time(e[2]))
    return {"fwd_ms": statistics.median(fw_t), "bwd_ms": statistics.median(bw_t), "fwd_bwd_ms": statistics.median(tot_t),
            "sky_share": float(mask.float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from street_crafter_amd import _lib
    _lib.load()
    rows = []
    for (W, H) in ((1600, 1066), (1920, 1280)):
        r = {"W": W, "H": H, "R": a.resolution}
        r["torch_before"] = time_path("torch", H, W, a.resolution, a.iters, a.warmup)
        r["hip"] = time_path("hip", H, W, a.resolution, a.iters, a.warmup)
        r["torch_after"] = time_path("torch", H, W, a.resolution, a.iters, a.warmup)
        fb, bb, fill = fused_bytes(H, W, a.resolution, r["hip"]["sky_share"])
        h = r["hip"]
        h["fwd_B_per_pixel"], h["bwd_B_per_pixel"], h["grad_fill_MB"] = fb / (H * W), bb / (H * W), fill / 1e6
        h["fwd_frac_hbm"] = fb / (h["fwd_ms"] * 1e-3) / HBM_PEAK
        h["bwd_frac_hbm"] = (bb + fill) / (h["bwd_ms"] * 1e-3) / HBM_PEAK
        r["speedup_fwd_bwd"] = min(r["torch_before"]["fwd_bwd_ms"], r["torch_after"]["fwd_bwd_ms"]) / h["fwd_bwd_ms"]
        rows.append(r)
        print(json.dumps(r), flush=True)
    print(f"{'case':<12}{'hip fwd':>9}{'bwd':>8}{'f+b':>8}{'torch f+b before':>18}{'after':>9}{'x':>7}{'fwd B/px':>10}{'%HBM':>6}"
          f"{'bwd B/px':>10}{'+fill MB':>9}{'%HBM':>6}")
    for r in rows:
        h = r["hip"]
        print(f"{r['W']}x{r['H']:<7}{h['fwd_ms']:9.3f}{h['bwd_ms']:8.3f}{h['fwd_bwd_ms']:8.3f}"
              f"{r['torch_before']['fwd_bwd_ms']:18.3f}{r['torch_after']['fwd_bwd_ms']:9.3f}{r['speedup_fwd_bwd']:7.1f}"
              f"{h['fwd_B_per_pixel']:10.1f}{100 * h['fwd_frac_hbm']:6.1f}{h['bwd_B_per_pixel']:10.1f}{h['grad_fill_MB']:9.1f}"
              f"{100 * h['bwd_frac_hbm']:6.1f}")
    print("device:", torch.cuda.get_device_name(0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
