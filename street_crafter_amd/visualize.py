"""The visualizer's video frames as uint8 on the GPU (csrc/frame_viz.hip; include/street_crafter_amd.h, "visualizer
frames"): the depth / squared-error colour maps of `visualize_depth_numpy` (street_gaussian/utils/img_utils.py:239-252)
and the `* 255` casts of street_gaussian_visualizer.py:49-132, which the reference computes on the host after
downloading every map as float32.

    value_range / diff_range          (mi, ma) of a map: the smallest positive value and the maximum after nan_to_num
    colorize / colorize_diff          uint8 [H,W,3] = lut[(255 * (x - mi) / (ma - mi + 1e-8)).astype(uint8)]
    gray_u8                           uint8 [H,W,1] = (a * 255).astype(uint8)
    novel_view_frames                 what visualize_novel_view + summarize() keep of one frame
    trajectory_frames                 what visualize() + summarize() keep of one frame

`lut` is the caller's uint8 [256,3] table on the device (INTEGRATION.md has the cv2 line that builds it).  The results
equal the reference's under NumPy >= 2 (float32 throughout) byte for byte, `.astype(np.uint8)` of an out-of-range value
included (the low 8 bits of the truncated value, as on x86).  A map without a positive value has mi = 0 where
`np.min` raises.  Opt-in: nothing else in the package calls this module.  Every function runs under no_grad and
raises ValueError on the host, before any launch, for a wrong shape, dtype or device; there is no CPU path.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _lib
from .dist import ROUNDING, to_uint8_frame

MinMax = Union[Tensor, Sequence[float]]


def _stream(t: Tensor):
    from .isect import _stream as raw
    return raw(t)


def _hip_f32(t, name: str) -> Tensor:
    if not isinstance(t, Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    return t.detach()


def _need_hip(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")


def _plane(x, name: str) -> Tuple[Tensor, int, int, int]:
    """A one-channel map [H,W], [1,H,W] or [H,W,1] -> (tensor whose first element is pixel 0, H, W, element stride);
    a view whose pixels are not evenly spaced is copied."""
    t = _hip_f32(x, name)
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    elif t.dim() == 3 and t.shape[2] == 1:
        t = t[..., 0]
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name} must be [H,W], [1,H,W] or [H,W,1] with H, W >= 1, got {tuple(x.shape)}")
    _need_hip(t, name)
    H, W = int(t.shape[0]), int(t.shape[1])
    s = t.stride(1) if W > 1 else (t.stride(0) if H > 1 else 1)
    if s < 1 or (H > 1 and W > 1 and t.stride(0) != W * s):
        t, s = t.contiguous(), 1
    return t, H, W, int(s)


def _image(x, name: str, hw: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, int, int, int, int]:
    """A colour image [3,H,W] (planes, or the permuted view of an [H,W,C>=3] render) -> (tensor, H, W, pixel stride,
    channel stride)."""
    t = _hip_f32(x, name)
    if t.dim() != 3 or t.shape[0] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
        raise ValueError(f"{name} must be [3,H,W] with H, W >= 1, got {tuple(x.shape)}")
    H, W = int(t.shape[1]), int(t.shape[2])
    if hw is not None and (H, W) != hw:
        raise ValueError(f"{name} must be [3,{hw[0]},{hw[1]}], got {tuple(x.shape)}")
    _need_hip(t, name)
    s0, s1, s2 = t.stride()
    px = s2 if W > 1 else (s1 if H > 1 else 1)
    if px < 1 or s0 < 1 or (H > 1 and W > 1 and s1 != W * px):
        t = t.contiguous()
        px, s0 = 1, H * W
    return t, H, W, int(px), int(s0)


def _mask(mask, hw: Tuple[int, int], device) -> Optional[Tensor]:
    if mask is None:
        return None
    if not isinstance(mask, Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mask must be a bool or uint8 tensor")
    if mask.device != device:
        raise ValueError(f"mask must be on {device}, got {mask.device}")
    m = mask[0] if mask.dim() == 3 and mask.shape[0] == 1 else mask
    if m.dim() != 2 or tuple(m.shape) != hw:
        raise ValueError(f"mask must be [{hw[0]},{hw[1]}] or [1,{hw[0]},{hw[1]}], got {tuple(mask.shape)}")
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _lut(lut, name: str, device) -> Tensor:
    if (not isinstance(lut, Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3) or not lut.is_contiguous()
            or lut.device != device):
        raise ValueError(f"{name} must be a contiguous uint8 [256,3] tensor on {device}")
    return lut


def _out(out, shape: Tuple[int, ...], device) -> Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if (not isinstance(out, Tensor) or tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous()
            or out.device != device):
        raise ValueError(f"out must be a contiguous uint8 {list(shape)} tensor on {device}")
    return out


def _range4(minmax: Optional[MinMax], device) -> Optional[Tensor]:
    """(mi, ma) as the device float[4] sc_frame_viz_u8 takes (the pair in both maps' places), or None."""
    if minmax is None:
        return None
    if isinstance(minmax, Tensor):
        if minmax.dtype != torch.float32 or tuple(minmax.shape) != (2,) or minmax.device != device:
            raise ValueError(f"minmax must be a pair of floats or a float32 [2] tensor on {device}")
        return minmax.detach().repeat(2)
    try:
        mi, ma = (float(v) for v in minmax)
    except (TypeError, ValueError):
        raise ValueError("minmax must be a pair of floats or a float32 [2] device tensor") from None
    return torch.tensor([mi, ma, mi, ma], dtype=torch.float32, device=device)


def _workspace(device) -> Tensor:
    return torch.empty(int(_lib.load().sc_frame_viz_workspace_bytes()), dtype=torch.uint8, device=device)


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _launch(n: int, like: Tensor, depth=None, rgb=None, gt=None, mask=None, acc=None, acc_object=None, depth_lut=None,
            diff_lut=None, range4=None, want_range: int = 0, depth_u8=None, diff_u8=None, acc_u8=None, acc_object_u8=None):
    """depth: (tensor, stride); rgb / gt: (tensor, pixel stride, channel stride).  Runs the range launch when a colour
    output has no range4 (or want_range, a bit mask of maps, asks for the numbers) and then the uint8 launch when an
    output is given.  -> the device float[4] of sc_frame_viz_range_finish when want_range, else None."""
    lib = _lib.load()
    st = _stream(like)
    d_p, d_s = (depth[0].data_ptr(), depth[1]) if depth is not None else (None, 1)
    r_p, r_px, r_ch = (rgb[0].data_ptr(), rgb[1], rgb[2]) if rgb is not None else (None, 1, 1)
    g_p, g_px, g_ch = (gt[0].data_ptr(), gt[1], gt[2]) if gt is not None else (None, 1, 1)
    ws = None
    nums = None
    colour = depth_u8 is not None or diff_u8 is not None
    if want_range or (colour and range4 is None):
        ws = _workspace(like.device)
        _lib.check(lib.sc_frame_viz_range(d_p, d_s, r_p, r_px, r_ch, g_p, g_px, g_ch, _p(mask), n, ws.data_ptr(),
                                          ws.numel(), st), "sc_frame_viz_range")
        if want_range:
            nums = torch.empty(4, dtype=torch.float32, device=like.device)
            _lib.check(lib.sc_frame_viz_range_finish(ws.data_ptr(), ws.numel(), n, int(want_range), nums.data_ptr(), st),
                       "sc_frame_viz_range_finish")
    if colour or acc_u8 is not None or acc_object_u8 is not None:
        _lib.check(lib.sc_frame_viz_u8(d_p, d_s, r_p, r_px, r_ch, g_p, g_px, g_ch, _p(mask), _p(acc), _p(acc_object), n,
                                       _p(depth_lut), _p(diff_lut), _p(range4), _p(ws), 0 if ws is None else ws.numel(),
                                       _p(depth_u8), _p(diff_u8), _p(acc_u8), _p(acc_object_u8), st), "sc_frame_viz_u8")
    return nums


def _diff_sources(rgb, gt, mask):
    r, H, W, r_px, r_ch = _image(rgb, "rgb")
    g, _, _, g_px, g_ch = _image(gt, "gt", (H, W))
    if g.device != r.device:
        raise ValueError(f"gt must be on {r.device}, got {g.device}")
    return (r, r_px, r_ch), (g, g_px, g_ch), _mask(mask, (H, W), r.device), H, W


@torch.no_grad()
def value_range(x: Tensor) -> Tensor:
    """float32 [2] device tensor (mi, ma) of a one-channel map ([H,W], [1,H,W] or [H,W,1], any even element stride):
    after nan_to_num, the smallest value > 0 (0 if there is none) and the maximum.  The range of frames joined side by
    side is the min of their mi and the max of their ma."""
    t, H, W, s = _plane(x, "x")
    return _launch(H * W, t, depth=(t, s), want_range=1)[0:2]


@torch.no_grad()
def diff_range(rgb: Tensor, gt: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """float32 [2] device tensor (mi, ma) of visualize_diff's map `((where(mask, rgb, 0) - where(mask, gt, 0)) ** 2)
    .sum(-1)`; rgb, gt [3,H,W], mask bool / uint8 [H,W] or [1,H,W] (None: all true)."""
    r, g, m, H, W = _diff_sources(rgb, gt, mask)
    return _launch(H * W, r[0], rgb=r, gt=g, mask=m, want_range=2)[2:4]


@torch.no_grad()
def colorize(x: Tensor, lut: Tensor, minmax: Optional[MinMax] = None, out: Optional[Tensor] = None) -> Tensor:
    """uint8 [H,W,3]: `visualize_depth_numpy(x, minmax, cmap)[0][..., ::-1]` with lut the RGB table of cmap.  minmax: a
    pair of floats or a float32 [2] device tensor (value_range's); None: the map's own range.  out: a preallocated
    contiguous uint8 [H,W,3]."""
    t, H, W, s = _plane(x, "x")
    lut = _lut(lut, "lut", t.device)
    r4 = _range4(minmax, t.device)
    out = _out(out, (H, W, 3), t.device)
    _launch(H * W, t, depth=(t, s), depth_lut=lut, range4=r4, depth_u8=out)
    return out


@torch.no_grad()
def colorize_diff(rgb: Tensor, gt: Tensor, lut: Tensor, mask: Optional[Tensor] = None, minmax: Optional[MinMax] = None,
                  out: Optional[Tensor] = None) -> Tensor:
    """uint8 [H,W,3]: the colour map of diff_range's map, which is recomputed in the kernel and never stored."""
    r, g, m, H, W = _diff_sources(rgb, gt, mask)
    lut = _lut(lut, "lut", r[0].device)
    r4 = _range4(minmax, r[0].device)
    out = _out(out, (H, W, 3), r[0].device)
    _launch(H * W, r[0], rgb=r, gt=g, mask=m, diff_lut=lut, range4=r4, diff_u8=out)
    return out


def _plane_hw(x, name: str, hw: Tuple[int, int]):
    t, H, W, s = _plane(x, name)
    if (H, W) != hw:
        raise ValueError(f"{name} must have {hw[0]} x {hw[1]} pixels, got {tuple(x.shape)}")
    return t, H, W, s


def _same_device(dev, **tensors):
    for name, t in tensors.items():
        if t.device != dev:
            raise ValueError(f"{name} must be on {dev}, got {t.device}")


def _dense_plane(a, name: str, hw: Optional[Tuple[int, int]] = None) -> Tuple[Tensor, int, int]:
    if isinstance(a, Tensor) and a.dtype == torch.bool:
        a = a.float()                       # (the visualizer itself spells acc_obj.float())
    t, H, W, s = _plane(a, name)
    if hw is not None and (H, W) != hw:
        raise ValueError(f"{name} must have {hw[0]} x {hw[1]} pixels, got {tuple(a.shape)}")
    return (t if s == 1 else t.contiguous()), H, W


@torch.no_grad()
def gray_u8(a: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """uint8 [H,W,1]: `(a * 255).astype(np.uint8)` of an accumulation map [H,W], [1,H,W] or [H,W,1]."""
    t, H, W = _dense_plane(a, "a")
    out = _out(out, (H, W, 1), t.device)
    _launch(H * W, t, acc=t, acc_u8=out)
    return out


def _slots(out: Optional[Dict[str, Tensor]], keys: Sequence[str]) -> Dict[str, Optional[Tensor]]:
    if out is None:
        return {k: None for k in keys}
    if not isinstance(out, dict) or set(out) - set(keys):
        raise ValueError(f"out must be a dict with keys among {list(keys)}")
    return {k: out.get(k) for k in keys}


@torch.no_grad()
def novel_view_frames(result: Dict[str, Tensor], depth_lut: Tensor, rounding: str = "video",
                      out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """What visualize_novel_view (street_gaussian_visualizer.py:82-101) and summarize() keep of one camera's frame, as
    uint8 on the device: {'rgb' [H,W,3], 'acc' [H,W,1], 'depth' [H,W,3]} from result['rgb'] [3,H,W], result['acc'] and
    result['depth'] ([1,H,W]; the dict layers.novel_view_frame returns).  depth is coloured over its own range, as
    summarize() does for one camera.  Two launches plus dist.to_uint8_frame's.  out: optional {'rgb' | 'acc' | 'depth':
    preallocated contiguous uint8 tensor} to write into."""
    if rounding not in ROUNDING:
        raise ValueError(f"rounding must be one of {sorted(ROUNDING)}, got {rounding!r}")
    for k in ("rgb", "acc", "depth"):
        if not isinstance(result, dict) or k not in result:
            raise ValueError(f"result must be a dict with 'rgb', 'acc' and 'depth' (missing {k!r})")
    rgb, H, W, _, _ = _image(result["rgb"], "result['rgb']")
    d, _, _, ds = _plane_hw(result["depth"], "result['depth']", (H, W))
    a, _, _ = _dense_plane(result["acc"], "result['acc']", (H, W))
    _same_device(rgb.device, **{"result['depth']": d, "result['acc']": a})
    lut = _lut(depth_lut, "depth_lut", rgb.device)
    slots = _slots(out, ("rgb", "acc", "depth"))
    o = {"rgb": _out(slots["rgb"], (H, W, 3), rgb.device), "acc": _out(slots["acc"], (H, W, 1), rgb.device),
         "depth": _out(slots["depth"], (H, W, 3), rgb.device)}
    to_uint8_frame(result["rgb"].detach(), rounding=rounding, out=o["rgb"])
    _launch(H * W, d, depth=(d, ds), acc=a, depth_lut=lut, depth_u8=o["depth"], acc_u8=o["acc"])
    return o


@torch.no_grad()
def trajectory_frames(result: Dict[str, Tensor], gt: Tensor, mask: Optional[Tensor], depth_lut: Tensor, diff_lut: Tensor,
                      out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """What visualize() (street_gaussian_visualizer.py:49-80, 103-132) and summarize() keep of one camera's frame, as
    uint8 on the device: 'rgb', 'rgb_background', 'rgb_object' [H,W,3] (dist.to_uint8_frame, truncating), 'acc_object'
    [H,W,1], 'depth' [H,W,3] (depth_lut, own range) and 'diff' [H,W,3] (diff_lut, own range; gt [3,H,W] the camera's
    original image, mask its guidance mask or None).  result: the [3,H,W] / [1,H,W] images the renderer returns, planes
    or permuted views of the rasterizers' [H,W,C] outputs (groups.py, layers.py).  Two launches plus three
    to_uint8_frame calls.  out: optional {key: preallocated contiguous uint8 tensor}."""
    keys = ("rgb", "rgb_background", "rgb_object", "acc_object", "depth")
    for k in keys:
        if not isinstance(result, dict) or k not in result:
            raise ValueError(f"result must be a dict with {list(keys)} (missing {k!r})")
    r, g, m, H, W = _diff_sources(result["rgb"], gt, mask)
    dev = r[0].device
    for k in ("rgb_background", "rgb_object"):
        _image(result[k], f"result[{k!r}]", (H, W))
    d, _, _, ds = _plane_hw(result["depth"], "result['depth']", (H, W))
    a, _, _ = _dense_plane(result["acc_object"], "result['acc_object']", (H, W))
    _same_device(dev, **{"result['depth']": d, "result['acc_object']": a})
    dl, fl = _lut(depth_lut, "depth_lut", dev), _lut(diff_lut, "diff_lut", dev)
    names = ("rgb", "rgb_background", "rgb_object", "acc_object", "depth", "diff")
    slots = _slots(out, names)
    o = {k: _out(slots[k], (H, W, 1 if k == "acc_object" else 3), dev) for k in names}
    for k in ("rgb", "rgb_background", "rgb_object"):
        to_uint8_frame(result[k].detach(), rounding="video", out=o[k])
    _launch(H * W, r[0], depth=(d, ds), rgb=r, gt=g, mask=m, acc_object=a, depth_lut=dl, diff_lut=fl,
            depth_u8=o["depth"], diff_u8=o["diff"], acc_object_u8=o["acc_object"])
    return o
