"""The novel-view training inputs on the GPU: `DiffusionRunner.preprocess_tensor`
(street_gaussian/utils/diffusion_utils.py:99-115: an integer crop to the diffusion aspect ratio, then
`torchvision.transforms.Resize`) and the row slice train.py:164-169 takes of its result, through the fused HIP kernels of
csrc/resize.hip, with their backward.  Opt-in: nothing imports this module by default.

What `Resize` does to a tensor is `torch.nn.functional.interpolate(x, size, mode="bilinear", align_corners=False,
antialias=A)`, A = True from torchvision 0.17 on and False for tensors before it; a non-float input is cast to float32 and
back, so a bool mask comes out True wherever the interpolated value is non-zero.  Here both are one weighted gather per
output from per-axis tap tables built on the host in float64 (`tap_table`: ATen's rule for either `antialias`), with the
crop folded into the read and the rows nobody asks for (`row_begin`) never computed.  The input is read through its
strides (the rasterizer's [H,W,4] image viewed as [3,H,W] takes one 16-byte load per tap); the backward is a gather
through the transposed tables that writes every element of a contiguous gradient once: no atomics, bit-identical runs.

fp32 and bool only.  No CPU path: tensors must live on a HIP device (the host-side helpers `crop_box` and `tap_table`
need no device).
"""
from __future__ import annotations

from collections import OrderedDict
from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .isect import _stream

__all__ = ["crop_box", "tap_table", "TapTable", "resize", "preprocess_tensor", "novel_view_inputs"]

AFFINE, PACKED4 = _lib.CONSTANTS["SC_RESIZE_AFFINE"], _lib.CONSTANTS["SC_RESIZE_PACKED4"]
MAX_SIDE = 1 << 16
MAX_PLANES = 65535
_CACHE_ENTRIES = 16


# ---- host side ----------------------------------------------------------------------------------------------------------
def _int(name: str, v, what: str, low: int = 1) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    if v < low:
        raise ValueError(f"{what}: {name} must be >= {low}, got {v}")
    return int(v)


def crop_box(h: int, w: int, target_h: int, target_w: int) -> Tuple[int, int, int, int]:
    """(top, bottom, left, right) of preprocess_tensor's crop, its arithmetic literally (diffusion_utils.py:100-111): a
    wider input keeps `int(target_w / target_h * h)` centred columns, a taller one the bottom `int(target_h / target_w * w)`
    rows, an equal ratio everything."""
    h, w = _int("h", h, "crop_box"), _int("w", w, "crop_box")
    target_h, target_w = _int("target_h", target_h, "crop_box"), _int("target_w", target_w, "crop_box")
    top, bottom, left, right = 0, h, 0, w
    if w / h > target_w / target_h:
        tmp_w = int(target_w / target_h * h)
        left = (w - tmp_w) // 2
        right = (w + tmp_w) // 2
    elif w / h < target_w / target_h:
        tmp_h = int(target_h / target_w * w)
        top = h - tmp_h
        bottom = h
    if not (0 <= top < bottom <= h and 0 <= left < right <= w):
        raise ValueError(f"crop_box: a {h}x{w} input leaves nothing at the ratio of {target_h}x{target_w}")
    return top, bottom, left, right


class TapTable(NamedTuple):
    """The taps of one axis.  Output i reads inputs start[i] .. start[i] + count - 1, count = offset[i+1] - offset[i],
    with the weights weight[offset[i]:offset[i+1]] (fp32; weight64 holds them before that rounding).  Transposed: input k
    is read by the outputs t_start[k] .. t_start[k] + (t_offset[k+1] - t_offset[k]) - 1, with t_weight[t_offset[k]:...]."""
    n_in: int
    n_out: int
    antialias: bool
    start: np.ndarray        # int32 [n_out]
    offset: np.ndarray       # int32 [n_out + 1]
    weight: np.ndarray       # float32 [offset[-1]]
    weight64: np.ndarray     # float64 [offset[-1]]
    t_start: np.ndarray      # int32 [n_in]
    t_offset: np.ndarray     # int32 [n_in + 1]
    t_weight: np.ndarray     # float32 [t_offset[-1]]

    def counts(self) -> np.ndarray:
        return np.diff(self.offset)

    def t_counts(self) -> np.ndarray:
        return np.diff(self.t_offset)


def _taps_antialias(n_in: int, n_out: int):
    """ATen's _compute_indices_min_size_weights_aa with the triangle filter, in float64: -> (xmin [n_out], w [n_out,K],
    zero past each row's size)."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    invscale = 1.0 / scale if scale >= 1.0 else 1.0          # (ATen multiplies by this, it does not divide by the support)
    i = np.arange(n_out, dtype=np.float64)
    center = scale * (i + 0.5)
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xsize = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    xsize = np.clip(xsize, 0, int(np.ceil(support)) * 2 + 1)
    j = np.arange(int(xsize.max()), dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((j + xmin[:, None] - center[:, None] + 0.5) * invscale))
    w = np.where(j < xsize[:, None], w, 0.0)
    total = w.sum(axis=1, keepdims=True)
    return xmin, w / np.where(total != 0.0, total, 1.0)


def _taps_bilinear(n_in: int, n_out: int):
    """The two taps of align_corners=False bilinear (ATen's compute_source_index_and_lambda), in float64; the second
    tap is clamped to n_in - 1, and where that makes it the first tap the two are one tap of weight 1."""
    i = np.arange(n_out, dtype=np.float64)
    if n_in == n_out:
        return i.astype(np.int64), np.ones((n_out, 1))
    src = np.maximum(n_in / n_out * (i + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    lam1 = np.clip(src - i0, 0.0, 1.0)
    last = i0 >= n_in - 1
    w = np.stack([np.where(last, 1.0, 1.0 - lam1), np.where(last, 0.0, lam1)], axis=1)
    return i0, w


@lru_cache(maxsize=64)
def _tap_table(n_in: int, n_out: int, antialias: bool) -> TapTable:
    first, w = (_taps_antialias if antialias else _taps_bilinear)(n_in, n_out)
    keep = w != 0.0                                            # taps of weight exactly zero are not taps
    rows, cols = np.nonzero(keep)                              # row-major: table order
    counts = keep.sum(axis=1)
    if (counts == 0).any():
        raise ValueError(f"tap_table: {n_in} -> {n_out} leaves an output without a tap")
    head = keep.argmax(axis=1)
    tail = keep.shape[1] - 1 - keep[:, ::-1].argmax(axis=1)
    if not np.array_equal(tail - head + 1, counts):
        raise ValueError(f"tap_table: {n_in} -> {n_out} has a zero weight between two taps")
    lo = first + head
    offset = np.zeros(n_out + 1, dtype=np.int64)
    np.cumsum(counts, out=offset[1:])
    w64 = w[rows, cols]
    w32 = w64.astype(np.float32)
    # transposed: sort the (input, output) pairs by input, outputs ascending inside an input
    src = first[rows] + cols
    order = np.lexsort((rows, src))
    t_src, t_out = src[order], rows[order]
    t_counts = np.bincount(t_src, minlength=n_in)
    t_offset = np.zeros(n_in + 1, dtype=np.int64)
    np.cumsum(t_counts, out=t_offset[1:])
    t_start = np.zeros(n_in, dtype=np.int64)
    has = t_counts > 0
    t_start[has] = t_out[t_offset[:-1][has]]
    run = t_out - np.repeat(t_start, t_counts) - (np.arange(len(t_out)) - np.repeat(t_offset[:-1], t_counts))
    if run.any():
        raise ValueError(f"tap_table: {n_in} -> {n_out}: the outputs that read one input are not one run")
    arrays = [a for a in (lo.astype(np.int32), offset.astype(np.int32), w32, w64, t_start.astype(np.int32),
                          t_offset.astype(np.int32), w32[order])]
    for a in arrays:
        a.setflags(write=False)
    return TapTable(n_in, n_out, antialias, *arrays)


def tap_table(n_in: int, n_out: int, antialias: bool = True) -> TapTable:
    """The taps `interpolate(mode="bilinear", align_corners=False, antialias=antialias)` gives each of n_out outputs along
    an axis of n_in inputs, and their transpose (which outputs read each input).
    antialias: ATen's _compute_indices_min_size_weights_aa: scale = n_in / n_out, support = max(scale, 1), center =
      scale (i + 0.5), xmin = max(int(center - support + 0.5), 0), xsize = min(int(center + support + 0.5), n_in) - xmin,
      w_j = max(0, 1 - |(j + xmin - center + 0.5) / support|) over their sum.
    else: src = max(scale (i + 0.5) - 0.5, 0), taps int(src) and the next (clamped to n_in - 1), weights 1 - frac, frac.
    Computed in float64, stored as fp32; taps whose float64 weight is exactly zero are dropped (what makes "any tap set"
    the mask's rule).  Any ratio, no tap cap.  The arrays are read-only and shared between calls."""
    n_in, n_out = _int("n_in", n_in, "tap_table"), _int("n_out", n_out, "tap_table")
    if n_in > MAX_SIDE or n_out > MAX_SIDE:
        raise ValueError(f"tap_table: sizes above {MAX_SIDE} are not supported ({n_in} -> {n_out})")
    return _tap_table(n_in, n_out, bool(antialias))


class _DeviceTable(NamedTuple):
    idx: Tensor      # int32 [2 n_out + 1]: start | offset
    w: Tensor        # fp32
    t_idx: Tensor    # int32 [2 n_in + 1]: t_start | t_offset
    t_w: Tensor


_device_tables: "OrderedDict[tuple, _DeviceTable]" = OrderedDict()


def _device_table(n_in: int, n_out: int, antialias: bool, device: torch.device) -> _DeviceTable:
    key = (n_in, n_out, antialias, device.type, device.index)
    hit = _device_tables.get(key)
    if hit is not None:
        _device_tables.move_to_end(key)
        return hit
    t = tap_table(n_in, n_out, antialias)
    # one buffer up, four views of it (the int32 words travel as their bit patterns)
    parts = [np.concatenate([t.start, t.offset]), t.weight.view(np.int32), np.concatenate([t.t_start, t.t_offset]),
             t.t_weight.view(np.int32)]
    flat = torch.from_numpy(np.concatenate(parts)).to(device)
    cuts = np.cumsum([0] + [len(p) for p in parts])
    views = [flat[cuts[k]:cuts[k + 1]] for k in range(4)]
    entry = _DeviceTable(views[0], views[1].view(torch.float32), views[2], views[3].view(torch.float32))
    _device_tables[key] = entry
    while len(_device_tables) > _CACHE_ENTRIES:
        _device_tables.popitem(last=False)
    return entry


# ---- device side --------------------------------------------------------------------------------------------------------
class _Geometry(NamedTuple):
    B: int
    C: int
    H: int
    W: int
    top: int
    left: int
    in_h: int
    in_w: int
    h_out: int
    w_out: int
    row_begin: int
    antialias: bool
    flags: int
    a: float
    b: float


def _strides4(x4: Tensor):
    """The four element strides the kernels get; a batch of one has no batch stride (a view's may be anything)."""
    sb, sc, sh, sw = (int(s) for s in x4.stride())
    return [0 if x4.shape[0] == 1 else sb, sc, sh, sw]


def _packed4(x4: Tensor) -> bool:
    """The rasterizer's layout: channel stride 1, pixel stride 4, at most 4 channels, 16-byte aligned, and the 16 bytes
    of the last pixel inside the storage.  (A crop keeps all of it: it moves the origin by whole rows and pixels.)"""
    B, C, H, W = x4.shape
    sb, sc, sh, sw = _strides4(x4)
    if not (C <= 4 and sc == 1 and sw == 4 and sb % 4 == 0 and sh % 4 == 0 and x4.data_ptr() % 16 == 0):
        return False
    last = x4.storage_offset() + (B - 1) * sb + (H - 1) * sh + (W - 1) * sw + 4
    return last * 4 <= x4.untyped_storage().nbytes()


def _forward(x4: Tensor, g: _Geometry) -> Tensor:
    ty = _device_table(g.in_h, g.h_out, g.antialias, x4.device)
    tx = _device_table(g.in_w, g.w_out, g.antialias, x4.device)
    view = x4[:, :, g.top:g.top + g.in_h, g.left:g.left + g.in_w]
    strides = _strides4(x4)
    if x4.dtype is torch.bool:
        rc, out = _lib.binding().resize_mask_fwd(view, strides, g.B, g.C, g.in_h, g.in_w, ty.idx, tx.idx, g.h_out, g.w_out,
                                                 g.row_begin, _stream(x4))
        what = "sc_resize_mask_fwd"
    else:
        flags = g.flags | (PACKED4 if _packed4(x4) else 0)
        rc, out = _lib.binding().resize_fwd(view, strides, g.B, g.C, g.in_h, g.in_w, ty.idx, ty.w, tx.idx, tx.w, g.h_out,
                                            g.w_out, g.row_begin, flags, g.a, g.b, _stream(x4))
        what = "sc_resize_fwd"
    if rc:
        _lib.check(rc, what)
    return out


class _Resize(torch.autograd.Function):
    """x [B,C,H,W] fp32 (any strides) -> [B,C,h_out - row_begin,w_out]; the geometry travels as non-tensor state."""

    @staticmethod
    def forward(ctx, x4, g):
        ctx.g = g
        ctx.set_materialize_grads(False)
        return _forward(x4, g)

    @staticmethod
    def backward(ctx, grad):
        g = ctx.g
        if grad is None or not ctx.needs_input_grad[0]:
            return None, None
        uy = _device_table(g.in_h, g.h_out, g.antialias, grad.device)
        ux = _device_table(g.in_w, g.w_out, g.antialias, grad.device)
        rc, gx = _lib.binding().resize_bwd(grad.contiguous(), g.B, g.C, g.H, g.W, g.top, g.left, g.in_h, g.in_w, uy.t_idx,
                                           uy.t_w, ux.t_idx, ux.t_w, g.h_out, g.w_out, g.row_begin, g.flags & AFFINE, g.a,
                                           _stream(grad))
        if rc:
            _lib.check(rc, "sc_resize_bwd")
        return gx, None


def _check_tensor(x, name: str, what: str, min_dim: int):
    if not isinstance(x, Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: {name} must live on a HIP device (got {x.device}); street_crafter_amd has no CPU path")
    if x.dtype not in (torch.float32, torch.bool):
        raise ValueError(f"{what}: {name} must be float32 or bool, got {x.dtype}")
    if x.dim() < min_dim:
        raise ValueError(f"{what}: {name} needs at least {min_dim} dimensions, got {tuple(x.shape)}")
    if 0 in x.shape:
        raise ValueError(f"{what}: empty {name} {tuple(x.shape)}")
    if x.shape[-2] > MAX_SIDE or x.shape[-1] > MAX_SIDE:
        raise ValueError(f"{what}: {name} of {tuple(x.shape)} is larger than {MAX_SIDE} along an image axis")


def _size(size, what: str) -> Tuple[int, int]:
    if isinstance(size, (tuple, list)) and len(size) == 2:
        h, w = _int("size[0]", size[0], what), _int("size[1]", size[1], what)
        if h > MAX_SIDE or w > MAX_SIDE:
            raise ValueError(f"{what}: size {size} is larger than {MAX_SIDE}")
        return h, w
    raise ValueError(f"{what}: size must be (height, width), got {size!r} (the smaller-edge form of Resize is not supported)")


def _run(x: Tensor, box, h_out: int, w_out: int, antialias: bool, row_begin: int, scale: float, shift: float,
         what: str) -> Tensor:
    """The common body: x [..., H, W], `box` the crop; returns [..., h_out - row_begin, w_out]."""
    H, W = x.shape[-2:]
    top, bottom, left, right = box
    lead = x.shape[:-2]
    x4 = x.reshape((1, 1, H, W)) if x.dim() == 2 else x.reshape((-1,) + tuple(x.shape[-3:])) if x.dim() != 3 else x[None]
    B, C = x4.shape[:2]
    if B * C > MAX_PLANES:
        raise ValueError(f"{what}: {B * C} image planes in one call (at most {MAX_PLANES})")
    scale, shift = float(scale), float(shift)
    affine = scale != 1.0 or shift != 0.0
    if affine and x.dtype is torch.bool:
        raise ValueError(f"{what}: scale / shift do not apply to a bool mask")
    g = _Geometry(B, C, H, W, top, left, bottom - top, right - left, h_out, w_out, row_begin, bool(antialias),
                  AFFINE if affine else 0, scale, shift)
    if x.dtype is torch.float32 and x.requires_grad and torch.is_grad_enabled():
        out = _Resize.apply(x4, g)
    else:
        out = _forward(x4.detach(), g)
    return out.reshape(tuple(lead) + (h_out - row_begin, w_out))


def resize(x: Tensor, size, antialias: bool = True) -> Tensor:
    """`torchvision.transforms.Resize(size)` of a tensor [..., H, W], size = (height, width): fp32 (differentiable) or
    bool (True wherever the interpolated value is non-zero)."""
    _check_tensor(x, "x", "resize", 2)
    h_out, w_out = _size(size, "resize")
    H, W = x.shape[-2:]
    return _run(x, (0, H, 0, W), h_out, w_out, antialias, 0, 1.0, 0.0, "resize")


def preprocess_tensor(x: Tensor, target_height: int, target_width: int, antialias: bool = True, row_begin: int = 0,
                      scale: float = 1.0, shift: float = 0.0) -> Tensor:
    """`DiffusionRunner.preprocess_tensor` for [C,H,W] or [B,C,H,W] (fp32 or bool): the crop of `crop_box`, then the
    resize to (target_height, target_width).  With the defaults a drop-in.  row_begin > 0 returns only the rows
    row_begin: of that result (the others are not computed, and get no gradient); scale, shift return
    `result * scale + shift` (fp32 only: the `* 2 - 1` of the diffusion inputs)."""
    _check_tensor(x, "x", "preprocess_tensor", 3)
    if x.dim() > 4:
        raise ValueError(f"preprocess_tensor: expected [C,H,W] or [B,C,H,W], got {tuple(x.shape)}")
    h_out, w_out = _size((target_height, target_width), "preprocess_tensor")
    row_begin = _int("row_begin", row_begin, "preprocess_tensor", low=0)
    if row_begin >= h_out:
        raise ValueError(f"preprocess_tensor: row_begin {row_begin} leaves no row of {h_out}")
    box = crop_box(x.shape[-2], x.shape[-1], h_out, w_out)
    return _run(x, box, h_out, w_out, antialias, row_begin, scale, shift, "preprocess_tensor")


def novel_view_inputs(image: Tensor, mask: Optional[Tensor], target_height: int, target_width: int,
                      antialias: bool = True, upper_frac: float = 0.4) -> Tuple[Tensor, Optional[Tensor], int]:
    """train.py:160-169 in one call: -> (image_loss, mask_loss, upper), upper = int(target_height * upper_frac), the
    tensors being rows upper: of the preprocessed image [3,H,W] and mask [1,H,W] (bool): what the reference hands to
    l1_loss / ssim / lpips.  The rows above `upper` are never computed.  mask=None gives None (the reference's all-ones
    mask resizes to all ones)."""
    _check_tensor(image, "image", "novel_view_inputs", 3)
    if image.dim() != 3 or image.dtype is not torch.float32:
        raise ValueError(f"novel_view_inputs: image must be float32 [C,H,W], got {image.dtype} {tuple(image.shape)}")
    h_out, _w = _size((target_height, target_width), "novel_view_inputs")
    if not 0.0 <= upper_frac < 1.0:
        raise ValueError(f"novel_view_inputs: upper_frac must be in [0, 1), got {upper_frac}")
    upper = int(h_out * upper_frac)
    if mask is not None:
        _check_tensor(mask, "mask", "novel_view_inputs", 3)
        if mask.dtype is not torch.bool or mask.dim() != 3 or mask.shape[-2:] != image.shape[-2:]:
            raise ValueError(f"novel_view_inputs: mask must be bool [1,H,W] over the image, got {mask.dtype} "
                             f"{tuple(mask.shape)} for image {tuple(image.shape)}")
        if mask.device != image.device:
            raise ValueError("novel_view_inputs: inputs live on different devices")
    image_loss = preprocess_tensor(image, target_height, target_width, antialias, row_begin=upper)
    mask_loss = None if mask is None else preprocess_tensor(mask, target_height, target_width, antialias, row_begin=upper)
    return image_loss, mask_loss, upper
