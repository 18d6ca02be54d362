"""Photometric loss of the training step on the GPU: `loss_utils.ssim` and `loss_utils.l1_loss`
(street_gaussian/utils/loss_utils.py:21-37, 95-131, called at train.py:168-188) through the fused HIP kernels of
csrc/losses.hip, with their backward.

Drop-in: `from street_crafter_amd.losses import l1_loss, ssim` in train.py gives the same signatures and results.
`l1_and_ssim(image, gt, mask)` returns both terms from one forward launch sequence and one backward: the form train.py's
loss line wants.  Inputs are read through their strides (the rasterizer's [H,W,4] image viewed as [3,H,W], a row crop
`img[:, upper:, :]`): no contiguous copy is made.  Nothing synchronises with the host.

fp32 and window 11 only (the reference never passes another size).  No CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from . import rendering as _r

__all__ = ["ssim", "l1_loss", "l1_and_ssim", "loss_forward", "LossForward"]

WINDOW = 11


class LossForward(NamedTuple):
    """What one fused forward returns: ssim [B+1] (per image, then the mean over all), l1 [B], kept [B] (kept
    (pixel, channel) entries), and the gradient maps [B,C,H,W] (None when no gradient was asked for)."""
    ssim: Tensor
    l1: Tensor
    kept: Tensor
    a1: Optional[Tensor]
    a2: Optional[Tensor]
    b: Optional[Tensor]
    c: Optional[Tensor]


def _check(img1: Tensor, img2: Tensor, mask: Optional[Tensor], window_size: int, what: str):
    """-> (batched, B, C, H, W, mask as a [Bm,1,H,W]-shaped view or None, mask_b)."""
    for name, t in (("img1", img1), ("img2", img2), ("mask", mask)):
        if t is None:
            continue
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must live on a HIP device (got {t.device}); "
                               "street_crafter_amd has no CPU path")
    if window_size != WINDOW:
        raise ValueError(f"{what}: window_size {window_size} is not supported (only {WINDOW}, the reference's size)")
    for name, t in (("img1", img1), ("img2", img2)):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if img1.shape != img2.shape:
        raise ValueError(f"{what}: shape mismatch {tuple(img1.shape)} vs {tuple(img2.shape)}")
    if img1.dim() not in (3, 4):
        raise ValueError(f"{what}: expected [C,H,W] or [B,C,H,W] images, got {tuple(img1.shape)}")
    if img2.device != img1.device or (mask is not None and mask.device != img1.device):
        raise ValueError(f"{what}: inputs live on different devices")
    batched = img1.dim() == 4
    B = img1.shape[0] if batched else 1
    Cc, H, W = img1.shape[-3:]
    if B == 0 or Cc == 0 or H == 0 or W == 0:
        raise ValueError(f"{what}: empty image {tuple(img1.shape)}")
    mb = 1
    if mask is not None:
        if mask.dtype != torch.bool:
            raise ValueError(f"{what}: mask must be a bool tensor (torch.where's condition), got {mask.dtype}")
        shp = tuple(mask.shape)
        ok = (shp == (H, W) or shp == (1, H, W) or
              (len(shp) == 4 and shp[1:] == (1, H, W) and shp[0] in (1, B)))
        if not ok:
            raise ValueError(f"{what}: mask of shape {shp} does not broadcast over images {tuple(img1.shape)} "
                             "(expected [1,H,W], or [B,1,H,W] for a batch)")
        mb = shp[0] if len(shp) == 4 else 1
        mask = mask.reshape(mb, 1, H, W) if mask.dim() != 4 else mask
    return batched, B, Cc, H, W, mask, mb


def _strides(img1: Tensor, img2: Tensor, mask: Optional[Tensor], batched: bool):
    s1 = img1.stride() if batched else (0,) + img1.stride()
    s2 = img2.stride() if batched else (0,) + img2.stride()
    sm = (0, 0, 0) if mask is None else (mask.stride(0), mask.stride(2), mask.stride(3))
    return [int(v) for v in (*s1, *s2, *sm)]


def loss_forward(img1: Tensor, img2: Tensor, mask: Optional[Tensor] = None, want_grad1: bool = False,
                 want_grad2: bool = False) -> LossForward:
    """The fused forward (sc_loss_fwd) without autograd; the gradient maps are written only for a wanted gradient."""
    batched, B, Cc, H, W, m, mb = _check(img1, img2, mask, WINDOW, "loss_forward")
    return _fwd(img1, img2, m, _strides(img1, img2, m, batched), B, Cc, H, W, mb, want_grad1, want_grad2)


def _fwd(img1, img2, m, st, B, Cc, H, W, mb, want1, want2) -> LossForward:
    rc, s, l1, kept, a1, a2, bm, cm = _lib.binding().loss_fwd(img1, img2, m, st, B, Cc, H, W, mb, H, W, WINDOW, want1,
                                                              want2, _r._stream(img1))
    if rc:
        _lib.check(rc, "sc_loss_fwd")
    return LossForward(s, l1, kept, a1, a2, bm, cm)


def _bwd(img1, img2, m, st, B, Cc, H, W, mb, fw: LossForward, g_ssim, g_l1, need1, need2):
    rc, g1, g2 = _lib.binding().loss_bwd(img1, img2, m, st, B, Cc, H, W, mb, H, W, WINDOW, fw.a1, fw.a2, fw.b, fw.c,
                                         g_ssim, g_l1, fw.kept, need1, need2, _r._stream(img1))
    if rc:
        _lib.check(rc, "sc_loss_bwd")
    return g1, g2


class _FusedLoss(torch.autograd.Function):
    """(img1, img2) -> (ssim [B+1], l1 [B]).  `mask` and the layout travel as non-tensor state; `want1` / `want2` say
    which gradients the caller may ask for (decided outside, where grad mode is visible), and only those maps are written."""

    @staticmethod
    def forward(ctx, img1, img2, mask, meta, want1, want2):
        batched, B, Cc, H, W, mb, st = meta
        fw = _fwd(img1, img2, mask, st, B, Cc, H, W, mb, want1, want2)
        ctx.set_materialize_grads(False)
        # (the maps and counts are intermediates, kept on ctx; the outputs themselves must not be, or they would hold
        #  their own graph alive)
        ctx.meta, ctx.mask, ctx.fw = meta, mask, fw._replace(ssim=None, l1=None)
        ctx.save_for_backward(img1, img2)
        return fw.ssim, fw.l1

    @staticmethod
    def backward(ctx, g_s, g_l):
        img1, img2 = ctx.saved_tensors
        batched, B, Cc, H, W, mb, st = ctx.meta
        fw = ctx.fw
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need1 or need2) or (g_s is None and g_l is None):
            return None, None, None, None, None, None
        gs = None
        if g_s is not None:     # ssim[B] is the mean of the B per-image values: it reaches each image as g / B
            gs = (g_s[:B] + g_s[B] / B).contiguous()
        gl = None if g_l is None else g_l.contiguous()
        g1, g2 = _bwd(img1, img2, ctx.mask, st, B, Cc, H, W, mb, fw, gs, gl, need1, need2)
        if not batched:
            g1 = None if g1 is None else g1[0]
            g2 = None if g2 is None else g2[0]
        return g1, g2, None, None, None, None


def _apply(img1, img2, mask, window_size, what):
    batched, B, Cc, H, W, m, mb = _check(img1, img2, mask, window_size, what)
    grad = torch.is_grad_enabled()
    want1, want2 = grad and img1.requires_grad, grad and img2.requires_grad
    meta = (batched, B, Cc, H, W, mb, _strides(img1, img2, m, batched))
    return _FusedLoss.apply(img1, img2, m, meta, want1, want2), B, batched


def ssim(img1: Tensor, img2: Tensor, window_size: int = 11, size_average: bool = True,
         mask: Optional[Tensor] = None) -> Tensor:
    """loss_utils.ssim: [C,H,W] -> the scalar mean; [B,C,H,W] -> the scalar mean, or with size_average=False the
    per-image means [B] (the reference's .mean(1).mean(1).mean(1)).  size_average=False on a [C,H,W] input is refused
    with ValueError; the reference raises there too (its third .mean(1) has no dimension left)."""
    if size_average is False and isinstance(img1, Tensor) and img1.dim() == 3:
        raise ValueError("ssim: size_average=False needs [B,C,H,W] input (the reference raises on [C,H,W] too)")
    (s, _l), B, _batched = _apply(img1, img2, mask, window_size, "ssim")
    return s[B] if size_average else s[:B]


def l1_loss(network_output: Tensor, gt: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """loss_utils.l1_loss: [C,H,W] images, mask [1,H,W]: the mean of |x - y| over the kept (pixel, channel) entries
    (NaN when the mask keeps none, as torch's mean of an empty selection).  Runs the fused forward (the SSIM sums come
    along); train.py's loss line is cheaper through l1_and_ssim."""
    if isinstance(network_output, Tensor) and network_output.dim() != 3:
        raise ValueError(f"l1_loss: expected [C,H,W] images, got {tuple(network_output.shape)}")
    (_s, l), _B, _batched = _apply(network_output, gt, mask, WINDOW, "l1_loss")
    return l[0]


def l1_and_ssim(image: Tensor, gt: Tensor, mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(l1_loss(image, gt, mask), ssim(image, gt, mask=mask)) from one fused forward and one backward: [C,H,W] images."""
    if isinstance(image, Tensor) and image.dim() != 3:
        raise ValueError(f"l1_and_ssim: expected [C,H,W] images, got {tuple(image.shape)}")
    (s, l), _B, _batched = _apply(image, gt, mask, WINDOW, "l1_and_ssim")
    return l[0], s[1]
