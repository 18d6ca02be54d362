"""Times what the visualizer does to one rendered frame -- download and conversion to the uint8 video frames -- as the
reference spells it (street_gaussian_visualizer.py:49-132 and summarize(); visualize_depth_numpy) against
street_crafter_amd.visualize on the same GPU, and the two new kernels alone.

    python tools/bench_visualize.py [--iters 30] [--warmup 5] [--kernel-iters 300] [--out profiles/visualize_ab.txt]

Cases: 1280x1920 and 1066x1600, one novel-view frame and one trajectory frame.  The render is resident on the GPU, as the
renderer leaves it: rgb the permuted view of an [H,W,4] image, depth / acc dense [1,H,W], background / object images as
planes.  The camera's ground-truth image and mask are resident on both sides (a host copy for the reference's lines, a
device copy for the new path): neither transfer is timed, and the constant `rgb_gt` frame is left out of both.

Per case, in ONE process and in this order: reference, new, reference again (the two reference rows bracket the new one:
a drifting clock or a busy host shows as a difference between them).  A frame's time is the host's wall clock from a
synchronised device to the moment every uint8 frame of it is a numpy array in host memory -- downloads included -- median
and minimum over --iters frames after --warmup.  `cv2.applyColorMap(x, cmap)` is restated as `lut[x]` with a fixed random
table (the library ships no copy of OpenCV's tables); the outputs of the two paths are compared byte for byte before
anything is timed.  Then the two kernels alone: ms per launch from one event pair around --kernel-iters launches into
preallocated outputs, the algorithmic bytes of each launch and their share of 8 TB/s.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # B/s, MI355X spec


def visualize_depth_numpy(depth, lut):
    """img_utils.py:239-252 with lut[...] for cv2.applyColorMap (the table is RGB already: no [..., [2, 1, 0]])."""
    x = np.nan_to_num(depth)
    mi = np.min(x[x > 0])
    ma = np.max(x)
    x = (x - mi) / (ma - mi + 1e-8)
    x = (255 * x).astype(np.uint8)
    return lut[x[..., 0]]


def reference_novel_view(result, lut):
    """visualize_novel_view's save_video branch (:82-101) and summarize()'s depth video for one frame."""
    rgb, acc, depth = result['rgb'], result['acc'], result['depth']
    depth = depth.permute(1, 2, 0).detach().cpu().numpy()
    rgb = (rgb.detach().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
    acc = (acc.detach().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
    return {"rgb": rgb, "acc": acc, "depth": visualize_depth_numpy(depth, lut)}


def reference_trajectory(result, gt_host, mask_host, depth_lut, diff_lut):
    """visualize()'s save_video branch (:65-76), visualize_diff (:103-120), visualize_depth (:122-132) and summarize()'s
    depth / diff videos for one frame."""
    import torch
    out = {}
    for key in ("rgb_background", "rgb", "rgb_object"):
        out[key] = (result[key].detach().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
    out["acc_object"] = (result["acc_object"].detach().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8)
    rgb = result['rgb'].detach().cpu()
    rgb = torch.where(mask_host, rgb, torch.zeros_like(rgb))
    rgb_gt = torch.where(mask_host, gt_host, torch.zeros_like(gt_host))
    rgb = rgb.permute(1, 2, 0).numpy()
    rgb_gt = rgb_gt.permute(1, 2, 0).numpy()
    diff = ((rgb - rgb_gt) ** 2).sum(axis=-1, keepdims=True)
    depth = result['depth'].detach().permute(1, 2, 0).detach().cpu().numpy()
    out["depth"] = visualize_depth_numpy(depth, depth_lut)
    out["diff"] = visualize_depth_numpy(diff, diff_lut)
    return out


def new_novel_view(result, lut_dev):
    from street_crafter_amd import visualize as V
    return {k: v.cpu().numpy() for k, v in V.novel_view_frames(result, lut_dev).items()}


def new_trajectory(result, gt_dev, mask_dev, depth_lut_dev, diff_lut_dev):
    from street_crafter_amd import visualize as V
    return {k: v.cpu().numpy() for k, v in V.trajectory_frames(result, gt_dev, mask_dev, depth_lut_dev, diff_lut_dev).items()}


def make_frame(H, W, dev):
    import torch
    gen = torch.Generator(device=dev).manual_seed(0)
    four = torch.rand(H, W, 4, device=dev, generator=gen)
    acc = torch.rand(1, H, W, device=dev, generator=gen)
    depth = 1.5 + 80.0 * torch.rand(1, H, W, device=dev, generator=gen)
    depth[acc < 0.03] = 0.0                                   # pixels no Gaussian reached
    result = {"rgb": four.permute(2, 0, 1)[:3], "acc": acc, "depth": depth,
              "rgb_background": torch.rand(3, H, W, device=dev, generator=gen),
              "rgb_object": torch.rand(3, H, W, device=dev, generator=gen),
              "acc_object": torch.rand(1, H, W, device=dev, generator=gen)}
    gt = (result["rgb"] + 0.1 * torch.randn(3, H, W, device=dev, generator=gen)).clamp(0, 1).contiguous()
    mask = torch.rand(1, H, W, device=dev, generator=gen) < 0.9
    return result, gt, mask


def wall(fn, iters, warmup):
    import torch
    ts = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            ts.append(1e3 * (t1 - t0))
    return statistics.median(ts), min(ts)


def time_kernels(result, gt, mask, luts, iters, warmup):
    """[(label, ms per launch, algorithmic bytes)] of sc_frame_viz_range and sc_frame_viz_u8 in the novel-view and the
    trajectory configuration, outputs and workspace preallocated."""
    import torch
    from street_crafter_amd import _lib
    from street_crafter_amd import visualize as V
    lib = _lib.load()
    _, H, W = result["depth"].shape
    P = H * W
    dev = gt.device
    ws = torch.empty(int(lib.sc_frame_viz_workspace_bytes()), dtype=torch.uint8, device=dev)
    o3a, o3b = (torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(2))
    o1 = torch.empty(H, W, 1, dtype=torch.uint8, device=dev)
    st = V._stream(gt)
    rgb, _, _, rpx, rch = V._image(result["rgb"], "rgb")
    m8 = mask[0].contiguous().view(torch.uint8)
    d, a, ao = result["depth"].data_ptr(), result["acc"].data_ptr(), result["acc_object"].data_ptr()
    diff_src = (rgb.data_ptr(), rpx, rch, gt.data_ptr(), 1, P, m8.data_ptr())
    none_src = (None, 1, 1, None, 1, 1, None)
    calls = [
        ("novel view  sc_frame_viz_range (depth)", 4 * P,
         lambda: lib.sc_frame_viz_range(d, 1, *none_src, P, ws.data_ptr(), ws.numel(), st)),
        ("novel view  sc_frame_viz_u8 (depth, acc)", 12 * P,
         lambda: lib.sc_frame_viz_u8(d, 1, *none_src, a, None, P, luts[0].data_ptr(), None, None, ws.data_ptr(), ws.numel(),
                                     o3a.data_ptr(), None, o1.data_ptr(), None, st)),
        ("trajectory  sc_frame_viz_range (depth, diff)", 29 * P,
         lambda: lib.sc_frame_viz_range(d, 1, *diff_src, P, ws.data_ptr(), ws.numel(), st)),
        ("trajectory  sc_frame_viz_u8 (depth, diff, acc_object)", 40 * P,
         lambda: lib.sc_frame_viz_u8(d, 1, *diff_src, None, ao, P, luts[0].data_ptr(), luts[1].data_ptr(), None, ws.data_ptr(),
                                     ws.numel(), o3a.data_ptr(), o3b.data_ptr(), None, o1.data_ptr(), st)),
    ]
    out = []
    for label, nbytes, call in calls:
        for _ in range(warmup):
            assert call() == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append((label, e0.elapsed_time(e1) / iters, nbytes))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visualize_ab.txt"))
    a = ap.parse_args()
    import torch
    from street_crafter_amd import _lib
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visualize.py needs a GPU: nothing is measured without one")
    dev = "cuda:0"
    g = np.random.default_rng(0)
    luts_np = [g.integers(0, 256, size=(256, 3), dtype=np.uint8) for _ in range(2)]
    luts = [torch.from_numpy(t).to(dev) for t in luts_np]
    lines = [f"tools/bench_visualize.py --iters {a.iters} --warmup {a.warmup} --kernel-iters {a.kernel_iters}",
             f"device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             "one frame, render resident on the GPU -> every uint8 video frame of it as a numpy array on the host; wall clock, ms",
             f"{'case':<12}{'frame':<13}{'path':<20}{'median':>9}{'min':>9}{'MB down':>9}"]
    kern = [f"kernels alone: ms per launch (mean of {a.kernel_iters} launches between two events, outputs preallocated), "
            "algorithmic bytes and share of 8 TB/s",
            f"{'case':<12}{'launch':<56}{'ms':>9}{'MB':>8}{'TB/s':>7}{'% HBM':>7}"]
    for (H, W) in ((1280, 1920), (1066, 1600)):
        result, gt, mask = make_frame(H, W, dev)
        gt_host, mask_host = gt.cpu(), mask.cpu()
        name, P = f"{H}x{W}", H * W
        frames = {
            "novel view": (lambda: reference_novel_view(result, luts_np[0]), lambda: new_novel_view(result, luts[0]),
                           (12 + 4 + 4) * P, (3 + 1 + 3) * P),
            "trajectory": (lambda: reference_trajectory(result, gt_host, mask_host, luts_np[0], luts_np[1]),
                           lambda: new_trajectory(result, gt, mask, luts[0], luts[1]),
                           (3 * 12 + 4 + 12 + 4) * P, (3 * 3 + 1 + 3 + 3) * P),
        }
        for frame, (ref, new, ref_bytes, new_bytes) in frames.items():
            want, got = ref(), new()
            assert sorted(want) == sorted(got)
            for k in want:
                assert np.array_equal(want[k], got[k]), (name, frame, k, int((want[k] != got[k]).sum()))
            rows = [("reference (before)", wall(ref, a.iters, a.warmup), ref_bytes),
                    ("visualize.py", wall(new, a.iters, a.warmup), new_bytes),
                    ("reference (after)", wall(ref, a.iters, a.warmup), ref_bytes)]
            for path, (med, lo), nbytes in rows:
                lines.append(f"{name:<12}{frame:<13}{path:<20}{med:9.3f}{lo:9.3f}{nbytes / 1e6:9.1f}")
            t_ref = 0.5 * (rows[0][1][0] + rows[2][1][0])
            lines.append(f"{name:<12}{frame:<13}reference / visualize.py: {t_ref / rows[1][1][0]:.2f}x (medians; outputs equal byte for byte)")
        for label, ms, nbytes in time_kernels(result, gt, mask, luts, a.kernel_iters, 20):
            rate = nbytes / (ms * 1e-3)
            kern.append(f"{name:<12}{label:<56}{ms:9.4f}{nbytes / 1e6:8.1f}{rate / 1e12:7.2f}{100 * rate / HBM_PEAK:7.1f}")
    text = "\n".join(lines + [""] + kern) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
