"""Times the fused photometric loss (street_crafter_amd/losses.py l1_and_ssim) against the reference's torch formula
(loss_utils.l1_loss + loss_utils.ssim, restated op for op: boolean-indexed L1, five grouped 11x11 conv2d) on the same GPU.

    python tools/bench_losses.py [--iters 100] [--warmup 10] [--out FILE.json]

Cases: 1600x1066 (the reference's training size) and 1920x1280; contiguous [3,H,W] input and the train-mode view
rc[0, ..., :3].permute(2, 0, 1) of an [1,H,W,4] render (pixel stride 4); with and without a [1,H,W] mask.
Per case and path: forward, backward and forward+backward in ms (HIP events around each, median over --iters after
--warmup), and for the fused path the compulsory bytes of each launch and their fraction of 8 TB/s.
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
# loss_utils.gaussian(11, 1.5) in fp32 (the reference's window is their outer product)
TAPS = ("0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.106560p-2",
        "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d956cp-10")


def torch_formula(image, gt, mask):
    """loss_utils.l1_loss + loss_utils.ssim, as train.py calls them (fp32, the reference's op sequence)."""
    import torch
    import torch.nn.functional as F
    C = image.shape[0]
    g32 = torch.tensor([float.fromhex(h) for h in TAPS], dtype=torch.float32)
    w = torch.outer(g32, g32).to(image.device).expand(C, 1, 11, 11).contiguous()
    a, b = image.permute(1, 2, 0), gt.permute(1, 2, 0)
    if mask is not None:
        a, b = a[mask.squeeze(0)], b[mask.squeeze(0)]
    l1 = (a - b).abs().mean()
    x, y = image, gt
    if mask is not None:
        x, y = torch.where(mask, x, torch.zeros_like(x)), torch.where(mask, y, torch.zeros_like(y))
    mu1, mu2 = F.conv2d(x, w, padding=5, groups=C), F.conv2d(y, w, padding=5, groups=C)
    s1 = F.conv2d(x * x, w, padding=5, groups=C) - mu1.pow(2)
    s2 = F.conv2d(y * y, w, padding=5, groups=C) - mu2.pow(2)
    s12 = F.conv2d(x * y, w, padding=5, groups=C) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1.pow(2) + mu2.pow(2) + C1) * (s1 + s2 + C2))
    return l1, m.mean()


def fused_bytes(C, H, W, layout, mask):
    """Compulsory HBM bytes per launch of the fused path (maps a1, b, c: only img1 requires a gradient)."""
    n = C * H * W
    img = 4 * n * (4 if layout == "view4" else 3) // 3       # the view's cache lines carry the 4th channel too
    msk = H * W if mask else 0
    fwd = img + 4 * n + msk + 3 * 4 * n                      # read render + gt (+ mask), write 3 maps
    bwd = img + 4 * n + msk + 3 * 4 * n + 4 * n              # read render + gt (+ mask) + 3 maps, write grad
    return fwd, bwd


def time_case(H, W, layout, mask, iters, warmup, path):
    import torch
    from street_crafter_amd import losses
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    rc = torch.rand(1, H, W, 4, device=dev, generator=g)
    gt = torch.rand(3, H, W, device=dev, generator=g)
    m = (torch.rand(1, H, W, device=dev, generator=g) > 0.2) if mask else None
    if layout == "contig":
        rc = rc[0, ..., :3].permute(2, 0, 1).contiguous()[None].permute(0, 2, 3, 1)   # [1,H,W,3] view of a [3,H,W] tensor
    fw_t, bw_t, tot_t = [], [], []
    for i in range(warmup + iters):
        src = rc.detach().clone().requires_grad_(True)
        image = src[0, ..., :3].permute(2, 0, 1)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        if path == "hip":
            l1, s = losses.l1_and_ssim(image, gt, m)
        else:
            l1, s = torch_formula(image, gt, m)
        loss = 0.8 * l1 + 0.2 * (1.0 - s)
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw_t.append(e[0].elapsed_time(e[1]))
            bw_t.append(e[1].elapsed_time(e[2]))
            tot_t.append(e[0].elapsed_time(e[2]))
    return {"fwd_ms": statistics.median(fw_t), "bwd_ms": statistics.median(bw_t), "fwd_bwd_ms": statistics.median(tot_t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from street_crafter_amd import _lib
    _lib.load()
    rows = []
    for (W, H) in ((1600, 1066), (1920, 1280)):
        for layout in ("contig", "view4"):
            for mask in (False, True):
                r = {"W": W, "H": H, "layout": layout, "mask": mask}
                for path in ("hip", "torch"):
                    r[path] = time_case(H, W, layout, mask, a.iters, a.warmup, path)
                fb, bb = fused_bytes(3, H, W, layout, mask)
                r["hip"]["fwd_MB"], r["hip"]["bwd_MB"] = fb / 1e6, bb / 1e6
                r["hip"]["fwd_frac_hbm"] = fb / (r["hip"]["fwd_ms"] * 1e-3) / HBM_PEAK
                r["hip"]["bwd_frac_hbm"] = bb / (r["hip"]["bwd_ms"] * 1e-3) / HBM_PEAK
                r["speedup_fwd_bwd"] = r["torch"]["fwd_bwd_ms"] / r["hip"]["fwd_bwd_ms"]
                rows.append(r)
                print(json.dumps(r), flush=True)
    print(f"{'case':<28}{'hip fwd':>9}{'bwd':>8}{'f+b':>8}{'torch fwd':>11}{'bwd':>8}{'f+b':>8}{'x':>7}"
          f"{'fwd MB':>8}{'%HBM':>6}{'bwd MB':>8}{'%HBM':>6}")
    for r in rows:
        h, t = r["hip"], r["torch"]
        name = f"{r['W']}x{r['H']} {r['layout']} {'mask' if r['mask'] else 'nomask'}"
        print(f"{name:<28}{h['fwd_ms']:9.3f}{h['bwd_ms']:8.3f}{h['fwd_bwd_ms']:8.3f}{t['fwd_ms']:11.3f}{t['bwd_ms']:8.3f}"
              f"{t['fwd_bwd_ms']:8.3f}{r['speedup_fwd_bwd']:7.1f}{h['fwd_MB']:8.1f}{100 * h['fwd_frac_hbm']:6.1f}"
              f"{h['bwd_MB']:8.1f}{100 * h['bwd_frac_hbm']:6.1f}")
    print("device:", torch.cuda.get_device_name(0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
