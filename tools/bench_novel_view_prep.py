"""Times novel_view_inputs (street_crafter_amd/resize.py: crop, antialiased resize of the render and of its mask, rows
`upper:` only, with the backward) against the literal torch sequence of train.py:160-169 on the same GPU.

    python tools/bench_novel_view_prep.py [--iters 50] [--warmup 5] [--out FILE.json]

Cases: 1066x1600 and 1280x1920 -> 576x1024.  The image is the [3,H,W] view of a [1,H,W,4] tensor (the rasterizer's
output), the mask is 30 % false, the upstream gradient of the rows `upper:` is random.
The torch path, written here: preprocess_tensor's crop, then what torchvision's Resize does to a tensor,
`F.interpolate(mode="bilinear", align_corners=False, antialias=True)` (the bool mask cast to float32 and back), the
`mask[..., :upper, :] = 0` and the three row slices.  It is timed before and after the fused path in the same process; both
numbers are printed.  The fused path counts as faster only where it beats both by more than they differ from each other.

Per case: forward, backward and forward+backward in ms (HIP events, median over --iters after --warmup); the backward
runs to the [1,H,W,4] leaf in both paths.  For the fused path also its compulsory bytes (the crop rows that outputs
`upper:` read, 16 B per pixel as the image lies in memory, plus 1 B of mask; 13 B per output pixel; the reverse plus the
dense [3,H,W] gradient backward) and the fraction of 8 TB/s they amount to.
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
TARGET = (576, 1024)
MASK_FALSE = 0.3


def torch_preprocess(x, target_height, target_width):
    """diffusion_utils.py:99-115 with Resize spelled out."""
    import torch
    import torch.nn.functional as F
    ori_h, ori_w = x.shape[-2:]
    if ori_w / ori_h > target_width / target_height:
        tmp_w = int(target_width / target_height * ori_h)
        left = (ori_w - tmp_w) // 2
        right = (ori_w + tmp_w) // 2
        x = x[..., :, left:right]
    elif ori_w / ori_h < target_width / target_height:
        tmp_h = int(target_height / target_width * ori_w)
        x = x[..., ori_h - tmp_h:ori_h, :]
    dtype = x.dtype
    y = x if dtype == torch.float32 else x.to(torch.float32)
    y = F.interpolate(y[None], size=(target_height, target_width), mode="bilinear", align_corners=False, antialias=True)[0]
    return y if dtype == torch.float32 else y.to(dtype)


def torch_novel_view(image, mask):
    """train.py:160-169."""
    image = torch_preprocess(image, *TARGET)
    mask = torch_preprocess(mask, *TARGET)
    upper = int(mask.shape[-2] * 0.4)
    mask[..., :upper, :] = 0
    return image[:, upper:, :], mask[:, upper:, :], upper


def fused_bytes(H, W):
    from street_crafter_amd import resize
    top, bottom, left, right = resize.crop_box(H, W, *TARGET)
    upper = int(TARGET[0] * 0.4)
    t = resize.tap_table(bottom - top, TARGET[0], True)
    rows_read = (bottom - top) - int(t.start[upper])
    read = rows_read * (right - left) * (16 + 1)
    out = (TARGET[0] - upper) * TARGET[1] * (12 + 1)
    fwd = read + out
    bwd = (TARGET[0] - upper) * TARGET[1] * 12 + 3 * H * W * 4
    return fwd, bwd


def time_path(path, H, W, iters, warmup):
    import torch
    from street_crafter_amd import resize
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    render = torch.rand(1, H, W, 4, device=dev, generator=g)
    mask = torch.rand(1, H, W, device=dev, generator=g) >= MASK_FALSE
    upper = int(TARGET[0] * 0.4)
    gout = torch.randn(3, TARGET[0] - upper, TARGET[1], device=dev, generator=g)
    fw_t, bw_t, tot_t = [], [], []
    for i in range(warmup + iters):
        leaf = render.detach().clone().requires_grad_(True)
        image = leaf[0, :, :, :3].permute(2, 0, 1)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        if path == "hip":
            image_loss, mask_loss, _u = resize.novel_view_inputs(image, mask, *TARGET)
        else:
            image_loss, mask_loss, _u = torch_novel_view(image, mask)
        e[1].record()
        image_loss.backward(gout)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw_t.append(e[0].elapsed_time(e[1]))
            bw_t.append(e[1].elapsed_time(e[2]))
            tot_t.append(e[0].elapsed_time(e[2]))
    assert image_loss.shape == gout.shape and mask_loss.shape == (1,) + tuple(gout.shape[1:]) and leaf.grad is not None
    return {"fwd_ms": statistics.median(fw_t), "bwd_ms": statistics.median(bw_t), "fwd_bwd_ms": statistics.median(tot_t)}


def agreement(H, W):
    """The two paths on the same input: the largest difference of the images, of the gradients, and the mask pixels that
    differ (fp32 torch against the fused fp32 sums)."""
    import torch
    from street_crafter_amd import resize
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    render = torch.rand(1, H, W, 4, device=dev, generator=g)
    mask = torch.rand(1, H, W, device=dev, generator=g) >= MASK_FALSE
    out = []
    for path in ("hip", "torch"):
        leaf = render.detach().clone().requires_grad_(True)
        image = leaf[0, :, :, :3].permute(2, 0, 1)
        il, ml, _u = resize.novel_view_inputs(image, mask, *TARGET) if path == "hip" else torch_novel_view(image, mask)
        if path == "hip":
            gout = torch.randn(il.shape, device=dev, generator=g)
        il.backward(gout)
        out.append((il.detach(), ml, leaf.grad))
    (a, am, ag), (b, bm, bg) = out
    return {"image_max_abs_diff": float((a - b).abs().max()), "grad_max_abs_diff": float((ag - bg).abs().max()),
            "mask_pixels_differing": int((am != bm).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from street_crafter_amd import _lib
    _lib.load()
    rows = []
    for (H, W) in ((1066, 1600), (1280, 1920)):
        r = {"H": H, "W": W, "target": list(TARGET), "agreement": agreement(H, W)}
        r["torch_before"] = time_path("torch", H, W, a.iters, a.warmup)
        r["hip"] = time_path("hip", H, W, a.iters, a.warmup)
        r["torch_after"] = time_path("torch", H, W, a.iters, a.warmup)
        fb, bb = fused_bytes(H, W)
        h = r["hip"]
        h["fwd_MB"], h["bwd_MB"] = fb / 1e6, bb / 1e6
        h["fwd_frac_hbm"] = fb / (h["fwd_ms"] * 1e-3) / HBM_PEAK
        h["bwd_frac_hbm"] = bb / (h["bwd_ms"] * 1e-3) / HBM_PEAK
        for key in ("fwd_ms", "bwd_ms", "fwd_bwd_ms"):
            before, after = r["torch_before"][key], r["torch_after"][key]
            r["faster_" + key[:-3]] = bool(min(before, after) - h[key] > abs(before - after))
        r["speedup_fwd_bwd"] = min(r["torch_before"]["fwd_bwd_ms"], r["torch_after"]["fwd_bwd_ms"]) / h["fwd_bwd_ms"]
        rows.append(r)
        print(json.dumps(r), flush=True)
    print(f"{'case':<12}{'hip fwd':>9}{'bwd':>8}{'f+b':>8}{'torch fwd before':>18}{'after':>8}{'bwd before':>12}{'after':>8}"
          f"{'f+b before':>12}{'after':>8}{'x':>6}{'faster':>8}{'fwd MB':>8}{'%HBM':>6}{'bwd MB':>8}{'%HBM':>6}")
    for r in rows:
        h, tb, ta = r["hip"], r["torch_before"], r["torch_after"]
        print(f"{r['H']}x{r['W']:<7}{h['fwd_ms']:9.3f}{h['bwd_ms']:8.3f}{h['fwd_bwd_ms']:8.3f}{tb['fwd_ms']:18.3f}{ta['fwd_ms']:8.3f}"
              f"{tb['bwd_ms']:12.3f}{ta['bwd_ms']:8.3f}{tb['fwd_bwd_ms']:12.3f}{ta['fwd_bwd_ms']:8.3f}{r['speedup_fwd_bwd']:6.1f}"
              f"{str(r['faster_fwd_bwd']):>8}{h['fwd_MB']:8.1f}{100 * h['fwd_frac_hbm']:6.1f}{h['bwd_MB']:8.1f}"
              f"{100 * h['bwd_frac_hbm']:6.1f}")
    print("device:", torch.cuda.get_device_name(0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
