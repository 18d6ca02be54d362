"""Writes tests/golden/losses_ref.npz: small inputs and the reference's own photometric loss on them
(street_gaussian/utils/loss_utils.py ssim / l1_loss, imported from the reference checkout), in float64 and float32,
with gradients through autograd.  Consumed by tests/test_losses_cpu.py (the float64 restatement) and
tests/test_losses_gpu.py (the HIP operators).

    python tools/make_golden_losses.py

Every case stores its float32 inputs and, for the loss of train.py:168-188 with lambda_l1 = 1, lambda_dssim = 0.2,
    L = 0.8 * l1_loss(x, y, mask) + 0.2 * (1 - ssim(x, y, mask=mask)),
the values ssim / l1 and one input gradient, each as <case>_<what>_f64 and <case>_<what>_f32 (<case>_m: the same images as
<case>, with <case>_m_mask).
Cases: rand / rand_m ([3,48,64] noise, unmasked / masked; gradient for img1), smooth / smooth_m ([3,48,64] smooth images
with flat regions; gradient for img2), batch ([2,3,32,40], ssim size_average=False; gradient of the sum for img1),
crop (the train-mode view rc[0, ..., :3].permute(2, 0, 1) of an [1,40,56,4] image cut to [:, upper:, :] with its
mask, as the novel-view branch does; gradient for img1 through the view).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("STREET_CRAFTER_REF", "/root/reference")


def smooth_pair(g, shape):
    C, H, W = shape
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64),
                            indexing="ij")
    a = torch.stack([0.5 + 0.3 * torch.sin(3 * xx + k) * torch.cos(2 * yy) for k in range(C)])
    a[:, : H // 3, : W // 2] = 0.4                                     # flat: sigma -> 0, C2 dominates
    b = a + 0.02 * torch.sin(7 * xx + 5 * yy)
    b[:, : H // 3, : W // 2] = 0.4                                     # equal and flat
    b[:, H // 2:, W // 2:] += 0.01 * torch.rand(C, H - H // 2, W - W // 2, generator=g, dtype=torch.float64)
    return a.float(), b.float()


def main():
    sys.path.insert(0, REF)
    from street_gaussian.utils.loss_utils import l1_loss, ssim     # noqa: E402
    g = torch.Generator().manual_seed(23)
    out = {}

    def record(name, x, y, mask, grad_of, batched=False, view=None):
        if not name.endswith("_m"):                                  # (<case>_m reuses <case>'s images)
            out[f"{name}_img1"], out[f"{name}_img2"] = x.numpy(), y.numpy()
        if mask is not None:
            out[f"{name}_mask"] = mask.numpy()
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            a = x.to(dt).clone().requires_grad_(True)
            b = y.to(dt).clone().requires_grad_(True)
            va, vb = (view(a), view(b)) if view is not None else (a, b)
            if batched:
                s = ssim(va, vb, size_average=False, mask=mask)
                s.sum().backward()
                out[f"{name}_ssim_{tag}"] = s.detach().numpy()
            else:
                s = ssim(va, vb, mask=mask)
                l = l1_loss(va, vb, mask)
                (0.8 * l + 0.2 * (1.0 - s)).backward()
                out[f"{name}_ssim_{tag}"] = np.float64(s.item())
                out[f"{name}_l1_{tag}"] = np.float64(l.item())
            gt = a if grad_of == 1 else b
            out[f"{name}_grad{grad_of}_{tag}"] = gt.grad.numpy()

    x = torch.rand(3, 48, 64, generator=g)
    y = (x + 0.1 * torch.randn(3, 48, 64, generator=g)).clamp(0, 1)
    m = torch.rand(1, 48, 64, generator=g) > 0.3
    m[:, :5, :] = False                                               # whole false rows at the image edge
    record("rand", x, y, None, 1)
    record("rand_m", x, y, m, 1)
    xs, ys = smooth_pair(g, (3, 48, 64))
    record("smooth", xs, ys, None, 2)
    record("smooth_m", xs, ys, m, 2)
    xb = torch.rand(2, 3, 32, 40, generator=g)
    yb = (xb + 0.05 * torch.randn(2, 3, 32, 40, generator=g)).clamp(0, 1)
    record("batch", xb, yb, None, 1, batched=True)
    rc = torch.rand(1, 40, 56, 4, generator=g)
    gtc = (rc + 0.1 * torch.randn(1, 40, 56, 4, generator=g)).clamp(0, 1)
    upper = int(40 * 0.4)
    mc = torch.rand(1, 40, 56, generator=g) > 0.2
    mc[..., :upper, :] = False
    out["crop_upper"] = np.int64(upper)
    record("crop", rc, gtc, mc[:, upper:, :], 1, view=lambda t: t[0, ..., :3].permute(2, 0, 1)[:, upper:, :])
    out["crop_full_mask"] = mc.numpy()
    sys.path.remove(REF)
    path = os.path.join(GOLD, "losses_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
