"""The convolution stack of the perceptual loss in HIP (csrc/lpips_stack.hip; include/street_crafter_amd.h, "perceptual
loss: the convolution stack"): what lpips.LPIPS._stack runs on torch by default, the reference's `x = layer(x)` loop over
AlexNet / VGG16 features (lpipsPyTorch/modules/networks.py:53-63, reached from train.py:172,185), forward and backward to
the image.  Opt-in: `LPIPS(..., stack="hip")` or `crit.set_stack("hip")`.

    supported(layers, taps)                          None, or the reason the route does not take this sequence
    plan(layers, C, H, W)                            the [C,h,w] after every layer, by the kernels' size arithmetic
    pack(layers, cache=None)                         packed weights per Conv (forward and data-gradient forms)
    conv_relu(x, packed, relu=True)                  convolution + bias + ReLU, exact-f32 MFMA
    conv_dgrad(g, relu_out, packed, in_hw, add=None) data gradient behind the ReLU mask (+ the tap's own gradient)
    max_pool(x, kernel, stride)                      floor mode, no padding
    max_pool_bwd(g, x, kernel, stride, add=None)     gather backward: torch's first-maximum rule, no index tensor
    feature_stack(layers, taps, z, packed=None)      prepared input [1,3,H,W] -> the raw taps, one autograd node

The weights are frozen in the reference (set_requires_grad(False)), so the backward is the data gradient only.  Tensors
are fp32 planes [C,h,w] or [1,C,h,w] on a HIP device; there is no CPU path and no fall-back to torch: a sequence the
kernels do not cover is refused by supported() before anything runs.  Rounding contract and order of the fused adds: the
header of csrc/lpips_stack.hip.  Layer records are lpips.Conv / Relu / MaxPool, recognised by their class names (lpips.py
imports this module, not the other way round).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib

__all__ = ["supported", "plan", "pack", "PackedConv", "conv_relu", "conv_dgrad", "max_pool", "max_pool_bwd",
           "feature_stack", "conv_out_hw", "pool_out_hw", "MAX_KERNEL", "MAX_STRIDE", "POOL_MAX_KERNEL"]

MAX_KERNEL = 11
MAX_STRIDE = 4
MAX_CHANNELS = 32767
POOL_MAX_KERNEL = 16


def _stream(t: Tensor):
    from .isect import _stream as raw
    return raw(t)


def _kind(layer) -> str:
    return type(layer).__name__


# ---- the size arithmetic ---------------------------------------------------------------------------------------------
def conv_out_hw(h: int, w: int, kernel, stride, padding) -> Tuple[int, int]:
    (kh, kw), (sy, sx), (py, px) = kernel, stride, padding
    return ((h + 2 * py - kh) // sy + 1 if h + 2 * py >= kh else 0, (w + 2 * px - kw) // sx + 1 if w + 2 * px >= kw else 0)


def pool_out_hw(h: int, w: int, kernel, stride) -> Tuple[int, int]:
    (kh, kw), (sy, sx) = kernel, stride
    return ((h - kh) // sy + 1 if h >= kh else 0, (w - kw) // sx + 1 if w >= kw else 0)


def _conv_geometry(layer, what: str):
    w = layer.weight
    if not isinstance(w, Tensor) or w.dim() != 4:
        raise ValueError(f"{what}: a Conv's weight must be a [Cout,Cin,kh,kw] tensor")
    cout, cin, kh, kw = (int(v) for v in w.shape)
    return cin, cout, (kh, kw), (int(layer.stride[0]), int(layer.stride[1])), (int(layer.padding[0]), int(layer.padding[1]))


def supported(layers: Sequence, taps: Sequence[int]) -> Optional[str]:
    """None when the HIP route takes the sequence, else the reason it does not.  It takes: every Conv followed by a Relu,
    every Relu behind a Conv, every MaxPool behind a Relu; taps (positions from 1) on Relu or MaxPool outputs; plain
    convolutions (no dilation) of kernel <= 11, stride <= 4, padding < kernel; pools without padding, in floor mode."""
    taps = [int(t) for t in taps]
    n = len(layers)
    for pos, layer in enumerate(layers, 1):
        kind = _kind(layer)
        nxt = _kind(layers[pos]) if pos < n else None
        prev = _kind(layers[pos - 2]) if pos > 1 else None
        if kind == "Conv":
            if pos in taps:
                return f"layer {pos}: a tap on a Conv's output (before its ReLU); the kernel writes ReLU outputs only"
            if nxt != "Relu":
                return f"layer {pos}: a Conv that is not followed by a Relu"
            if tuple(getattr(layer, "dilation", (1, 1))) != (1, 1):
                return f"layer {pos}: a dilated convolution {tuple(layer.dilation)}"
            w = layer.weight
            if not isinstance(w, Tensor) or w.dim() != 4 or w.dtype != torch.float32:
                return f"layer {pos}: the weight must be a float32 [Cout,Cin,kh,kw] tensor"
            cin, cout, (kh, kw), (sy, sx), (py, px) = _conv_geometry(layer, "supported")
            if layer.bias is not None and (layer.bias.dtype != torch.float32 or tuple(layer.bias.shape) != (cout,)):
                return f"layer {pos}: the bias must be a float32 [{cout}] tensor"
            if not (1 <= kh <= MAX_KERNEL and 1 <= kw <= MAX_KERNEL):
                return f"layer {pos}: kernel {kh}x{kw} (up to {MAX_KERNEL}x{MAX_KERNEL})"
            if not (1 <= sy <= MAX_STRIDE and 1 <= sx <= MAX_STRIDE):
                return f"layer {pos}: stride {sy}x{sx} (1 to {MAX_STRIDE})"
            if not (0 <= py < kh and 0 <= px < kw):
                return f"layer {pos}: padding {py}x{px} must be smaller than the kernel {kh}x{kw}"
            if not (1 <= cin <= MAX_CHANNELS and 1 <= cout <= MAX_CHANNELS):
                return f"layer {pos}: {cin} -> {cout} channels (1 to {MAX_CHANNELS})"
        elif kind == "Relu":
            if prev != "Conv":
                return f"layer {pos}: a Relu that does not follow a Conv"
        elif kind == "MaxPool":
            if prev != "Relu":
                return f"layer {pos}: a MaxPool that does not follow a Relu"
            if tuple(layer.padding) != (0, 0):
                return f"layer {pos}: a padded max-pool {tuple(layer.padding)}"
            if layer.ceil_mode:
                return f"layer {pos}: a max-pool in ceil_mode"
            if tuple(getattr(layer, "dilation", (1, 1))) != (1, 1):
                return f"layer {pos}: a dilated max-pool"
            (kh, kw), (sy, sx) = layer.kernel, layer.stride
            if not (1 <= kh <= POOL_MAX_KERNEL and 1 <= kw <= POOL_MAX_KERNEL and sy >= 1 and sx >= 1):
                return f"layer {pos}: max-pool window {kh}x{kw} stride {sy}x{sx} (window up to {POOL_MAX_KERNEL})"
        else:
            return f"layer {pos}: a {kind} record (Conv, Relu and MaxPool only)"
    for t in taps:
        if not 1 <= t <= n:
            return f"tap {t} outside the {n} layers"
    return None


def plan(layers: Sequence, C: int, H: int, W: int) -> List[Tuple[int, int, int]]:
    """The [C,h,w] after every layer of the sequence for a [C,H,W] input, by the arithmetic the kernels check."""
    out = []
    for pos, layer in enumerate(layers, 1):
        kind = _kind(layer)
        if kind == "Conv":
            cin, cout, k, s, p = _conv_geometry(layer, "plan")
            if cin != C:
                raise ValueError(f"plan: layer {pos} takes {cin} channels, its input has {C}")
            C, (H, W) = cout, conv_out_hw(H, W, k, s, p)
        elif kind == "MaxPool":
            H, W = pool_out_hw(H, W, layer.kernel, layer.stride)
        out.append((C, H, W))
    return out


# ---- checks (shapes and dtypes first, then the device: all before anything is launched) ------------------------------
def _planes(t, name: str, what: str, channels: Optional[int] = None) -> Tuple[Tensor, bool]:
    """-> (the contiguous [C,h,w] tensor without autograd history, whether it came as [1,C,h,w])"""
    if not isinstance(t, Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    four = t.dim() == 4
    if four and t.shape[0] != 1:
        raise NotImplementedError(f"{what}: one image only, {name} is a batch of {t.shape[0]}")
    if t.dim() not in (3, 4):
        raise ValueError(f"{what}: {name} must be [C,h,w] or [1,C,h,w], got {tuple(t.shape)}")
    t3 = t[0] if four else t
    if channels is not None and t3.shape[0] != channels:
        raise ValueError(f"{what}: {name} must have {channels} channels, got {tuple(t.shape)}")
    return t3.detach(), four


def _same(t, name: str, what: str, like: Tensor) -> Tensor:
    t3, _ = _planes(t, name, what)
    if t3.shape != like.shape:
        raise ValueError(f"{what}: {name} must be {tuple(like.shape)}, got {tuple(t.shape)}")
    return t3


def _on_device(what: str, *named):
    dev = None
    for name, t in named:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must live on a HIP device (got {t.device}); "
                               "street_crafter_amd has no CPU path")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{what}: inputs live on different devices")


def _pair_arg(v, name: str, what: str) -> Tuple[int, int]:
    if isinstance(v, int):
        return v, v
    try:
        a, b = v
        return int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be an int or a pair of ints, got {v!r}") from None


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


# ---- packed weights --------------------------------------------------------------------------------------------------
class PackedConv:
    """One Conv's weights in the kernels' layouts: `fwd` for the forward, `dgrad` for the stride-1 data gradient (None
    for a strided convolution, whose gather kernel reads `weight` itself).  `key` tells pack() when to repack.  The
    packs are written on the stream that is current when pack() runs; the stage calls that read them must run on that
    stream, or the caller orders the two streams."""
    __slots__ = ("weight", "bias", "cin", "cout", "kernel", "stride", "padding", "fwd", "dgrad", "key")

    def __init__(self, layer):
        what = "lpips_stack.pack"
        cin, cout, kernel, stride, padding = _conv_geometry(layer, what)
        w, b = layer.weight, layer.bias
        if w.dtype != torch.float32:
            raise ValueError(f"{what}: the weight must be float32, got {w.dtype}")
        if b is not None and (not isinstance(b, Tensor) or b.dtype != torch.float32 or tuple(b.shape) != (cout,)):
            raise ValueError(f"{what}: the bias must be a float32 [{cout}] tensor")
        _on_device(what, ("weight", w), ("bias", b))
        lib = _lib.load()
        self.key = _pack_key(layer)
        self.weight = w.detach().contiguous()
        self.bias = None if b is None else b.detach().contiguous()
        self.cin, self.cout, self.kernel, self.stride, self.padding = cin, cout, kernel, stride, padding
        st = _stream(self.weight)
        forms = [("fwd", 0, lib.sc_conv_pack_fwd)]
        self.dgrad = None
        if stride == (1, 1):
            forms.append(("dgrad", 1, lib.sc_conv_pack_dgrad))
        for attr, flag, fn in forms:
            nbytes = int(lib.sc_conv_pack_bytes(cin, cout, kernel[0], kernel[1], flag))
            if nbytes == 0:
                raise ValueError(f"{what}: {cin} -> {cout} channels, kernel {kernel}: outside the kernels' limits")
            buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
            _lib.check(fn(self.weight.data_ptr(), cin, cout, kernel[0], kernel[1], buf.data_ptr(), nbytes, st),
                       "sc_conv_pack_" + attr)
            setattr(self, attr, buf)


def _pack_key(layer):
    w, b = layer.weight, layer.bias
    return (w.data_ptr(), w._version, tuple(w.shape), tuple(layer.stride), tuple(layer.padding),
            None if b is None else (b.data_ptr(), b._version))


def pack(layers: Sequence, cache: Optional[Sequence] = None) -> List[Optional[PackedConv]]:
    """Packed weights per layer (None where the layer is not a Conv), both forms.  `cache`: an earlier result for the
    same sequence; an entry is packed again only where the weight's or bias's `_version` or `data_ptr()` changed."""
    out = []
    for i, layer in enumerate(layers):
        if _kind(layer) != "Conv":
            out.append(None)
            continue
        old = cache[i] if cache is not None and i < len(cache) else None
        out.append(old if isinstance(old, PackedConv) and old.key == _pack_key(layer) else PackedConv(layer))
    return out


# ---- the stages ------------------------------------------------------------------------------------------------------
def _check_packed(packed, what: str) -> PackedConv:
    if not isinstance(packed, PackedConv):
        raise TypeError(f"{what}: packed must be a PackedConv (lpips_stack.pack), got {type(packed).__name__}")
    return packed


def _conv_relu3(x3: Tensor, pk: PackedConv, relu: bool) -> Tensor:
    h, w = int(x3.shape[1]), int(x3.shape[2])
    oh, ow = conv_out_hw(h, w, pk.kernel, pk.stride, pk.padding)
    y = torch.empty((pk.cout, oh, ow), dtype=torch.float32, device=x3.device)
    rc = _lib.load().sc_conv2d_relu_fwd(x3.data_ptr(), pk.fwd.data_ptr(), pk.fwd.numel(), _p(pk.bias), pk.cin, h, w, pk.cout,
                                        pk.kernel[0], pk.kernel[1], pk.stride[0], pk.stride[1], pk.padding[0],
                                        pk.padding[1], oh, ow, 1 if relu else 0, y.data_ptr(), _stream(x3))
    if rc:
        _lib.check(rc, "sc_conv2d_relu_fwd")
    return y


def conv_relu(x: Tensor, packed: PackedConv, relu: bool = True) -> Tensor:
    """max(conv(x) + bias, 0) (relu=False: without the max) of one image, x [Cin,h,w] or [1,Cin,h,w] -> the same rank.
    Exact f32 on the matrix core; the pre-activation is never stored."""
    what = "lpips_stack.conv_relu"
    pk = _check_packed(packed, what)
    x3, four = _planes(x, "x", what, pk.cin)
    _on_device(what, ("x", x3), ("packed", pk.fwd))
    y = _conv_relu3(x3.contiguous(), pk, bool(relu))
    return y[None] if four else y


def _conv_dgrad3(g3: Tensor, r3: Optional[Tensor], pk: PackedConv, in_hw: Tuple[int, int], add3: Optional[Tensor]) -> Tensor:
    h, w = in_hw
    oh, ow = int(g3.shape[1]), int(g3.shape[2])
    gi = torch.empty((pk.cin, h, w), dtype=torch.float32, device=g3.device)
    lib, st = _lib.load(), _stream(g3)
    if pk.dgrad is not None:
        rc = lib.sc_conv2d_dgrad(g3.data_ptr(), _p(r3), pk.dgrad.data_ptr(), pk.dgrad.numel(), _p(add3), pk.cin, h, w,
                                 pk.cout, pk.kernel[0], pk.kernel[1], pk.padding[0], pk.padding[1], oh, ow, gi.data_ptr(), st)
        name = "sc_conv2d_dgrad"
    else:
        rc = lib.sc_conv2d_dgrad_strided(g3.data_ptr(), _p(r3), pk.weight.data_ptr(), _p(add3), pk.cin, h, w, pk.cout,
                                         pk.kernel[0], pk.kernel[1], pk.stride[0], pk.stride[1], pk.padding[0],
                                         pk.padding[1], oh, ow, gi.data_ptr(), st)
        name = "sc_conv2d_dgrad_strided"
    if rc:
        _lib.check(rc, name)
    return gi


def conv_dgrad(g: Tensor, relu_out: Optional[Tensor], packed: PackedConv, in_hw: Tuple[int, int],
               add: Optional[Tensor] = None) -> Tensor:
    """The gradient of a convolution's input [Cin,h,w] (in_hw = (h, w)) from the gradient g of its ReLU's output
    [Cout,oh,ow]: g counts where relu_out (the SAVED output, same shape; None: no mask) is > 0.  `add` [Cin,h,w]
    (the gradient the input receives as a tap) is added once, after the sum.  Stride 1 runs on the matrix core, a
    strided convolution by gather."""
    what = "lpips_stack.conv_dgrad"
    pk = _check_packed(packed, what)
    g3, four = _planes(g, "g", what, pk.cout)
    h, w = _pair_arg(in_hw, "in_hw", what)
    if h < 0 or w < 0 or conv_out_hw(h, w, pk.kernel, pk.stride, pk.padding) != (int(g3.shape[1]), int(g3.shape[2])):
        raise ValueError(f"{what}: an input of {h}x{w} does not give a gradient of {tuple(g3.shape[1:])}")
    r3 = None if relu_out is None else _same(relu_out, "relu_out", what, g3)
    a3 = None
    if add is not None:
        a3, _ = _planes(add, "add", what, pk.cin)
        if tuple(a3.shape[1:]) != (h, w):
            raise ValueError(f"{what}: add must be [{pk.cin},{h},{w}], got {tuple(add.shape)}")
    _on_device(what, ("g", g3), ("relu_out", r3), ("add", a3), ("packed", pk.fwd))
    gi = _conv_dgrad3(g3.contiguous(), None if r3 is None else r3.contiguous(), pk, (h, w),
                      None if a3 is None else a3.contiguous())
    return gi[None] if four else gi


def _pool_args(kernel, stride, what: str):
    k, s = _pair_arg(kernel, "kernel", what), _pair_arg(stride, "stride", what)
    if not (1 <= k[0] <= POOL_MAX_KERNEL and 1 <= k[1] <= POOL_MAX_KERNEL and s[0] >= 1 and s[1] >= 1):
        raise ValueError(f"{what}: window {k} (1 to {POOL_MAX_KERNEL}) stride {s} (>= 1)")
    return k, s


def _max_pool3(x3: Tensor, k, s) -> Tensor:
    c, h, w = (int(v) for v in x3.shape)
    oh, ow = pool_out_hw(h, w, k, s)
    y = torch.empty((c, oh, ow), dtype=torch.float32, device=x3.device)
    rc = _lib.load().sc_maxpool2d_fwd(x3.data_ptr(), c, h, w, k[0], k[1], s[0], s[1], oh, ow, y.data_ptr(), _stream(x3))
    if rc:
        _lib.check(rc, "sc_maxpool2d_fwd")
    return y


def max_pool(x: Tensor, kernel, stride) -> Tensor:
    """torch's max_pool2d(x, kernel, stride) (no padding, no dilation, floor mode) of [C,h,w] or [1,C,h,w], bit for bit."""
    what = "lpips_stack.max_pool"
    x3, four = _planes(x, "x", what)
    k, s = _pool_args(kernel, stride, what)
    _on_device(what, ("x", x3))
    y = _max_pool3(x3.contiguous(), k, s)
    return y[None] if four else y


def _max_pool_bwd3(g3: Tensor, x3: Tensor, k, s, add3: Optional[Tensor]) -> Tensor:
    c, h, w = (int(v) for v in x3.shape)
    gi = torch.empty_like(x3)
    rc = _lib.load().sc_maxpool2d_bwd(g3.data_ptr(), x3.data_ptr(), _p(add3), c, h, w, k[0], k[1], s[0], s[1],
                                      int(g3.shape[1]), int(g3.shape[2]), gi.data_ptr(), _stream(x3))
    if rc:
        _lib.check(rc, "sc_maxpool2d_bwd")
    return gi


def max_pool_bwd(g: Tensor, x: Tensor, kernel, stride, add: Optional[Tensor] = None) -> Tensor:
    """The gradient of max_pool's input x from the gradient g of its output: each window's gradient goes to its first
    maximum in row-major order (torch's rule), recomputed from x; `add` (x's shape) is added once, after the sum."""
    what = "lpips_stack.max_pool_bwd"
    x3, four = _planes(x, "x", what)
    k, s = _pool_args(kernel, stride, what)
    g3, _ = _planes(g, "g", what, int(x3.shape[0]))
    if pool_out_hw(int(x3.shape[1]), int(x3.shape[2]), k, s) != (int(g3.shape[1]), int(g3.shape[2])):
        raise ValueError(f"{what}: an input of {tuple(x3.shape[1:])} does not give a gradient of {tuple(g3.shape[1:])}")
    a3 = None if add is None else _same(add, "add", what, x3)
    _on_device(what, ("g", g3), ("x", x3), ("add", a3))
    gi = _max_pool_bwd3(g3.contiguous(), x3.contiguous(), k, s, None if a3 is None else a3.contiguous())
    return gi[None] if four else gi


# ---- the whole stack -------------------------------------------------------------------------------------------------
def _forward(layers, taps, packed, z3: Tensor, keep: bool):
    """-> (the taps as [C,h,w], the stages for the backward when `keep`: (kind, layer index, input [h,w], its ReLU
    output or the pool's input, tap slot of the stage's output or None))"""
    outs, stages = [], []
    x, i, n = z3, 0, len(layers)
    while i < n:
        layer, hw = layers[i], (int(x.shape[1]), int(x.shape[2]))
        if _kind(layer) == "Conv":                   # ... and the Relu behind it: supported() saw to that
            y = _conv_relu3(x, packed[i], True)
            stage = ("conv", i, hw, y)
            i += 2
        else:
            k, s = tuple(layer.kernel), tuple(layer.stride)
            y = _max_pool3(x, k, s)
            stage = ("pool", i, hw, x)
            i += 1
        slot = None
        if i in taps:                                # i is now the 1-based position of the stage's last layer
            slot = len(outs)
            outs.append(y)
        if keep:
            stages.append(stage + (slot,))
        x = y
    return outs, stages


class _FeatureStack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, layers, taps, packed):
        outs, stages = _forward(layers, taps, packed, z.detach()[0].contiguous(), True)
        ctx.set_materialize_grads(False)
        ctx.layers, ctx.packed = layers, packed
        ctx.meta = [(kind, i, hw, slot) for kind, i, hw, _t, slot in stages]
        ctx.save_for_backward(*[t for _k, _i, _hw, t, _s in stages])          # the ReLU outputs, nothing else
        return tuple(o[None] for o in outs)

    @staticmethod
    def backward(ctx, *tap_grads):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        saved = ctx.saved_tensors
        grads = [None if g is None else g.detach()[0].contiguous() for g in tap_grads]
        G = None                                     # the gradient of the current stage's output, its tap's share included
        for s in range(len(ctx.meta) - 1, -1, -1):
            kind, i, hw, slot = ctx.meta[s]
            if s == len(ctx.meta) - 1:
                G = grads[slot] if slot is not None else None
            below = ctx.meta[s - 1][3] if s > 0 else None        # the tap slot of this stage's input
            add = grads[below] if below is not None else None
            if G is None:                            # nothing reaches this stage from above
                G = add
                continue
            if kind == "conv":
                G = _conv_dgrad3(G, saved[s], ctx.packed[i], hw, add)
            else:
                layer = ctx.layers[i]
                G = _max_pool_bwd3(G, saved[s], tuple(layer.kernel), tuple(layer.stride), add)
        return (None if G is None else G[None]), None, None, None


def feature_stack(layers: Sequence, taps: Sequence[int], z: Tensor, packed: Optional[Sequence] = None) -> List[Tensor]:
    """The raw taps ([1,C,h,w] each) of the prepared input z [1,3,H,W] through `layers`, as ONE autograd node whose
    backward runs from the taps' gradients to z's.  It keeps the ReLU outputs only (the taps among them live on in the
    head anyway); under no_grad, or when z needs no gradient, it keeps nothing and the taps carry no graph.  `packed`:
    pack(layers), kept by the caller between calls (None: packed here, every call)."""
    what = "lpips_stack.feature_stack"
    taps = [int(t) for t in taps]
    why = supported(layers, taps)
    if why is not None:
        raise NotImplementedError(f"{what}: {why}")
    if not isinstance(z, Tensor):
        raise TypeError(f"{what}: z must be a torch.Tensor, got {type(z).__name__}")
    if z.dtype != torch.float32:
        raise ValueError(f"{what}: z must be float32, got {z.dtype}")
    layers = list(layers[:taps[-1]]) if taps else list(layers)
    cin = int(layers[0].weight.shape[1]) if layers and _kind(layers[0]) == "Conv" else None
    if z.dim() != 4 or z.shape[0] != 1 or (cin is not None and z.shape[1] != cin):
        raise ValueError(f"{what}: z must be [1,{cin if cin is not None else 'C'},H,W], got {tuple(z.shape)}")
    _on_device(what, ("z", z))
    return _feature_stack_checked(layers, taps, z, pack(layers, packed))


def _feature_stack_checked(layers, taps, z: Tensor, packed) -> List[Tensor]:
    """feature_stack behind its checks, for a caller that has made them: lpips.LPIPS validates the sequence when the
    route is chosen, prepares z itself and keeps `packed` = pack(layers) current; layers end at the last tap."""
    if torch.is_grad_enabled() and z.requires_grad:
        return list(_FeatureStack.apply(z, layers, taps, packed))
    outs, _ = _forward(layers, taps, packed, z.detach()[0].contiguous(), False)
    return [o[None] for o in outs]
