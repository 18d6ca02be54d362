"""The perceptual loss of the training step on the GPU: the reference's `lpips(image * mask, gt * mask)` (train.py:172,185;
street_gaussian/utils/lpipsPyTorch) with everything but its convolutions in the fused HIP kernels of csrc/lpips.hip.

    prepare(img, mask, mean, std)               z = (where(mask, img, 0) - mean) / std  from the strided render -> [1,3,H,W]
    lpips_distance(feats_x, feats_y, lin_w)     all taps of both images -> the distance [1,1,1,1], one launch (+ a tiny sum)
    LPIPS                                       the criterion: prep kernel, the convolution stack, head kernel
    lpips(x, y, net_type='alex', version='0.1') the reference's free function over a criterion registered by the caller

The weights are the caller's, as the optimizer's parameters are: `LPIPS.from_reference(criterion)` reads a loaded
reference module (its weight loading stays as it is), `LPIPS.from_state_dicts` takes torchvision-keyed weights and the
LPIPS v0.1 linear layers.  Nothing here downloads anything.  The convolutions, ReLU and max-pool run on torch by
default; `stack="hip"` (or `crit.set_stack("hip")`) runs them in the kernels of csrc/lpips_stack.hip instead
(lpips_stack.py: exact-f32 MFMA convolutions with fused bias / ReLU, data gradient, max-pool), for the sequences
lpips_stack.supported() takes: AlexNet and VGG16 as the tables below build them.

`crit.target(gt, mask)` computes the ground truth's features once per camera (about 70 MB at 1600x1066 for AlexNet);
`crit(image, target, mask)` then skips the second network pass.

Deviation from the reference, on purpose: where every feature of a pixel is zero (n == 0) the reference's autograd gives
NaN in that pixel's feature gradients (the derivative of sqrt at 0 meets a zero); the head's backward returns the finite
limit of its closed form (include/street_crafter_amd.h).  Behind a tap that is a ReLU's output, as all of AlexNet's and
VGG16's are, torch's ReLU backward drops that NaN again, so the image gradient of the reference is finite there too; a
tap taken anywhere else spreads it.  One image only: the reference's cat / sum adds batch entries into
one number and train.py never passes a batch.  fp32 only; no CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor

from . import _lib
from . import lpips_stack
from .isect import _stream

__all__ = ["prepare", "lpips_distance", "LPIPS", "LPIPSTarget", "Conv", "Relu", "MaxPool", "lpips", "set_criterion",
           "MEAN", "STD", "MAX_TAPS"]

MAX_TAPS = _lib.CONSTANTS["SC_LPIPS_MAX_TAPS"]
# the scaling layer of LPIPS v0.1 (Zhang et al. 2018; networks.py:41-44 holds the same numbers)
MEAN = (-0.030, -0.088, -0.188)
STD = (0.458, 0.448, 0.450)


# ---- checks (shapes and dtypes first, then the device: all before anything is launched) ------------------------------
def _is_tensor(name: str, t, what: str):
    if not isinstance(t, Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")


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


def _host3(name: str, v, what: str) -> Tuple[float, float, float]:
    if isinstance(v, Tensor):
        v = v.detach().reshape(-1).tolist()       # (a device tensor makes the host wait here: hand over host numbers)
    v = tuple(float(x) for x in v)
    if len(v) != 3:
        raise ValueError(f"{what}: {name} must hold 3 numbers, got {len(v)}")
    return v


def _check_image(img, mask, what: str):
    """-> (the [3,H,W] view, the [H,W] bool mask or None, H, W)"""
    _is_tensor("img", img, what)
    if img.dtype != torch.float32:
        raise ValueError(f"{what}: img must be float32, got {img.dtype}")
    if img.dim() == 4:
        if img.shape[0] != 1:
            raise NotImplementedError(f"{what}: one image only, got a batch of {img.shape[0]} (the reference adds batch "
                                      "entries into one number and train.py never passes one)")
        img = img[0]
    if img.dim() != 3 or img.shape[0] != 3:
        raise ValueError(f"{what}: expected a [3,H,W] or [1,3,H,W] image, got {tuple(img.shape)}")
    H, W = int(img.shape[1]), int(img.shape[2])
    if H == 0 or W == 0:
        raise ValueError(f"{what}: empty image {tuple(img.shape)}")
    if mask is not None:
        _is_tensor("mask", mask, what)
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"{what}: mask must be bool or uint8, got {mask.dtype}")
        if tuple(mask.shape) not in ((H, W), (1, H, W)):
            raise ValueError(f"{what}: mask of shape {tuple(mask.shape)} does not fit an image of {H}x{W} "
                             "(expected [1,H,W])")
        if mask.dim() == 3:
            mask = mask[0]
    return img, mask, H, W


# ---- prep ----------------------------------------------------------------------------------------------------------
class _Prep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, mask, mean, std):
        H, W = int(img.shape[1]), int(img.shape[2])
        sm = (0, 0) if mask is None else mask.stride()
        strides = [int(v) for v in (*img.stride(), *sm)]
        rc, z = _lib.binding().lpips_prep_fwd(img, mask, strides, H, W, list(mean), list(std), _stream(img))
        if rc:
            _lib.check(rc, "sc_lpips_prep_fwd")
        ctx.mask, ctx.meta = mask, (strides, H, W, std)
        return z

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        strides, H, W, std = ctx.meta
        rc, gi = _lib.binding().lpips_prep_bwd(g.contiguous(), ctx.mask, strides, H, W, list(std), _stream(g))
        if rc:
            _lib.check(rc, "sc_lpips_prep_bwd")
        return gi, None, None, None


def _prepare_checked(img3: Tensor, m: Optional[Tensor], mean, std, what: str) -> Tensor:
    """prepare() behind _check_image: img3 [3,H,W], m [H,W] or None, mean / std three host numbers each."""
    if any(s == 0.0 for s in std):
        raise ValueError(f"{what}: std must not be zero, got {std}")
    _on_device(what, ("img", img3), ("mask", m))
    if m is not None and m.dtype != torch.bool:
        m = m.ne(0)
    return _Prep.apply(img3, m, mean, std)


def prepare(img: Tensor, mask: Optional[Tensor] = None, mean: Sequence[float] = MEAN,
            std: Sequence[float] = STD) -> Tensor:
    """The network input of LPIPS from the render as it lies in memory: z = (where(mask, img, 0) - mean_c) / std_c,
    contiguous [1,3,H,W], in one launch.  img fp32 [3,H,W] or [1,3,H,W], read through its strides (the rasterizer's
    [H,W,4] image viewed as [3,H,W], a row crop img[:, upper:, :]); mask bool or uint8 [1,H,W] (read through its strides
    too) or None; mean, std three host numbers each.  For finite images bit-identical to ((img * mask) - mean) / std,
    and so is the gradient."""
    what = "lpips.prepare"
    img3, m, _H, _W = _check_image(img, mask, what)
    return _prepare_checked(img3, m, _host3("mean", mean, what), _host3("std", std, what), what)


# ---- head ----------------------------------------------------------------------------------------------------------
def _tap_view(f: Tensor) -> Tuple[Tensor, int]:
    """-> ([C,h,w] tensor the kernel can read in place, its channel stride): pixels contiguous, channel stride >= h*w."""
    C, h, w = f.shape
    P = h * w
    if C == 1 and f[0].is_contiguous():
        return f, P
    if f.stride(2) == 1 and (h == 1 or f.stride(1) == w) and f.stride(0) >= P:
        return f, int(f.stride(0))
    return f.contiguous(), P


def _check_taps(feats_x, feats_y, lin_weights, what: str):
    for name, seq in (("feats_x", feats_x), ("feats_y", feats_y), ("lin_weights", lin_weights)):
        if not isinstance(seq, (list, tuple)):
            raise TypeError(f"{what}: {name} must be a list of tensors, got {type(seq).__name__}")
    n = len(feats_x)
    if len(feats_y) != n or len(lin_weights) != n:
        raise ValueError(f"{what}: mismatched tap lists ({n} feats_x, {len(feats_y)} feats_y, {len(lin_weights)} "
                         "lin_weights)")
    if not 1 <= n <= MAX_TAPS:
        raise ValueError(f"{what}: 1 to {MAX_TAPS} taps, got {n}")
    fx3, fy3, ws = [], [], []
    for k in range(n):
        pair = []
        for name, f in (("feats_x", feats_x[k]), ("feats_y", feats_y[k])):
            _is_tensor(f"{name}[{k}]", f, what)
            if f.dtype != torch.float32:
                raise ValueError(f"{what}: {name}[{k}] must be float32, got {f.dtype}")
            if f.dim() == 4:
                if f.shape[0] != 1:
                    raise NotImplementedError(f"{what}: one image only, {name}[{k}] is a batch of {f.shape[0]}")
                f = f[0]
            if f.dim() != 3 or f.numel() == 0:
                raise ValueError(f"{what}: {name}[{k}] must be a non-empty [C,h,w] or [1,C,h,w], got {tuple(f.shape)}")
            pair.append(f)
        if pair[0].shape != pair[1].shape:
            raise ValueError(f"{what}: tap {k}: shape mismatch {tuple(pair[0].shape)} vs {tuple(pair[1].shape)}")
        w = lin_weights[k]
        _is_tensor(f"lin_weights[{k}]", w, what)
        C = pair[0].shape[0]
        if w.dtype != torch.float32:
            raise ValueError(f"{what}: lin_weights[{k}] must be float32, got {w.dtype}")
        if tuple(w.shape) not in ((C,), (1, C, 1, 1)):
            raise ValueError(f"{what}: lin_weights[{k}] must be [{C}] or [1,{C},1,1], got {tuple(w.shape)}")
        fx3.append(pair[0])
        fy3.append(pair[1])
        ws.append(w.detach().reshape(-1))
    _on_device(what, *[(f"feats_x[{k}]", f) for k, f in enumerate(fx3)], *[(f"feats_y[{k}]", f) for k, f in enumerate(fy3)],
               *[(f"lin_weights[{k}]", w) for k, w in enumerate(ws)])
    return fx3, fy3, ws


class _Head(torch.autograd.Function):
    """(feats_x..., feats_y...) -> (total [1], per tap [n]); only the total carries a gradient.  geom = (C, P, stride_x,
    stride_y) lists; `want` says whether anybody may ask for a gradient: only then are the norms written and kept."""

    @staticmethod
    def forward(ctx, weights, geom, want, *feats):
        n = len(feats) // 2
        fx, fy = list(feats[:n]), list(feats[n:])
        C, P, sx, sy = geom
        rc, out, nx, ny = _lib.binding().lpips_head_fwd(fx, fy, weights, C, P, sx, sy, want, _stream(fx[0]))
        if rc:
            _lib.check(rc, "sc_lpips_head_fwd")
        ctx.n = n
        if want:
            ctx.weights, ctx.geom = weights, geom
            ctx.save_for_backward(*feats, *nx, *ny)
        total, taps = out[n:], out[:n]
        ctx.mark_non_differentiable(taps)
        return total, taps

    @staticmethod
    def backward(ctx, g, _g_taps):
        n = ctx.n
        none = (None, None, None) + (None,) * (2 * n)
        need = ctx.needs_input_grad[3:]
        if g is None or not any(need):
            return none
        saved = ctx.saved_tensors
        fx, fy = list(saved[:n]), list(saved[n:2 * n])
        nx, ny = list(saved[2 * n:3 * n]), list(saved[3 * n:])
        C, P, sx, sy = ctx.geom
        rc, gx, gy = _lib.binding().lpips_head_bwd(fx, fy, ctx.weights, C, P, sx, sy, nx, ny, g.contiguous(),
                                                   [bool(v) for v in need[:n]], [bool(v) for v in need[n:]], _stream(g))
        if rc:
            _lib.check(rc, "sc_lpips_head_bwd")
        grads = [None if t is None else t.view(f.shape) for t, f in zip(gx + gy, fx + fy)]
        return (None, None, None, *grads)


def lpips_distance(feats_x: Sequence[Tensor], feats_y: Sequence[Tensor], lin_weights: Sequence[Tensor],
                   return_taps: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """The distance head of LPIPS over raw (not normalised) features: per tap l, with fh = f / (sqrt(sum_c f^2) + 1e-10),
    d_l = mean over pixels of sum_c w_lc (fhx - fhy)^2; returns sum_l d_l as [1,1,1,1], the reference's output shape
    (return_taps=True: also the d_l, [n], without a gradient).  Features [C,h,w] or [1,C,h,w] fp32, any channel counts,
    up to 8 taps; lin_weights [C] or the reference's [1,C,1,1].  Differentiable in both feature lists (a gradient nobody
    needs is not computed); the weights carry none.  Under no_grad nothing is kept."""
    what = "lpips_distance"
    fx3, fy3, ws = _check_taps(feats_x, feats_y, lin_weights, what)
    vx, vy = [_tap_view(f) for f in fx3], [_tap_view(f) for f in fy3]
    C = [int(f.shape[0]) for f in fx3]
    P = [int(f.shape[1] * f.shape[2]) for f in fx3]
    geom = (C, P, [s for _f, s in vx], [s for _f, s in vy])
    feats = [f for f, _s in vx] + [f for f, _s in vy]
    want = torch.is_grad_enabled() and any(f.requires_grad for f in feats)
    total, taps = _Head.apply([w.contiguous() for w in ws], geom, want, *feats)
    total = total.view(1, 1, 1, 1)
    return (total, taps) if return_taps else total


# ---- the criterion ---------------------------------------------------------------------------------------------------
class Conv(NamedTuple):
    weight: Tensor
    bias: Optional[Tensor]
    stride: Tuple[int, int]
    padding: Tuple[int, int]
    # (1, 1) in every record the constructors below build (they refuse a dilated module).  The field exists so that
    # lpips_stack.supported() can name a dilated record; a hand-built one runs on the torch route, which passes it on.
    dilation: Tuple[int, int] = (1, 1)


class Relu(NamedTuple):
    pass


class MaxPool(NamedTuple):
    kernel: Tuple[int, int]
    stride: Tuple[int, int]
    padding: Tuple[int, int]
    ceil_mode: bool


def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


# The feature stacks of torchvision's alexnet and vgg16 by their published hyper-parameters (Krizhevsky 2014, "One weird
# trick"; Simonyan & Zisserman 2015, configuration D): position in `features` -> layer.  Taps are counted from 1, after
# the layer of that position, as the reference counts them (networks.py:57-60).
def _alex_table():
    c, r, p = "conv", ("relu",), ("maxpool", 3, 2, 0, False)
    return [(c, 4, 2), r, p, (c, 1, 2), r, p, (c, 1, 1), r, (c, 1, 1), r, (c, 1, 1), r], [2, 5, 8, 10, 12]


def _vgg16_table():
    table = []
    for block in (2, 2, 3, 3, 3):
        table += [("conv", 1, 1), ("relu",)] * block + [("maxpool", 2, 2, 0, False)]
    return table, [4, 9, 16, 23, 30]


_TABLES = {"alex": _alex_table, "vgg": _vgg16_table}


class LPIPSTarget:
    """The ground truth's side of the criterion, computed once: the raw taps of gt (under no_grad) and the image size."""

    def __init__(self, feats: List[Tensor], size: Tuple[int, int]):
        self.feats, self.size = feats, size

    def nbytes(self) -> int:
        return sum(f.numel() * f.element_size() for f in self.feats)


class LPIPS:
    """The criterion as plain records: `layers` (Conv / Relu / MaxPool up to the last tap), `taps` (positions counted
    from 1: the tap is the output of that layer), `mean` / `std` (host numbers) and `lin_weights` ([C] per tap)."""

    def __init__(self, layers: Sequence[NamedTuple], taps: Sequence[int], mean: Sequence[float], std: Sequence[float],
                 lin_weights: Sequence[Tensor], net_type: Optional[str] = None, stack: str = "torch"):
        what = "LPIPS"
        taps = [int(t) for t in taps]
        if not 1 <= len(taps) <= MAX_TAPS or sorted(set(taps)) != taps or taps[0] < 1 or taps[-1] > len(layers):
            raise ValueError(f"{what}: taps must be 1 to {MAX_TAPS} increasing layer positions in [1, {len(layers)}], "
                             f"got {taps}")
        if len(lin_weights) != len(taps):
            raise ValueError(f"{what}: {len(taps)} taps but {len(lin_weights)} lin weights")
        for layer in layers:
            if not isinstance(layer, (Conv, Relu, MaxPool)):
                raise TypeError(f"{what}: a layer must be a Conv, Relu or MaxPool record, got {type(layer).__name__}")
        self.layers = list(layers[:taps[-1]])
        self.taps = taps
        self.mean, self.std = _host3("mean", mean, what), _host3("std", std, what)
        self.lin_weights = [w.detach().reshape(-1) for w in lin_weights]
        self.net_type = net_type
        self.stack, self._packed = "torch", None
        self.set_stack(stack)

    def set_stack(self, stack: str) -> str:
        """Where the convolution stack runs: "torch" (the default) or "hip" (lpips_stack.py).  Returns the previous
        value.  "hip" on a sequence the kernels do not cover raises here, with lpips_stack.supported()'s reason, never
        in the middle of a step."""
        if stack not in ("torch", "hip"):
            raise ValueError(f"LPIPS: stack must be 'torch' or 'hip', got {stack!r}")
        if stack == "hip":
            why = lpips_stack.supported(self.layers, self.taps)
            if why is not None:
                raise NotImplementedError(f"LPIPS: stack='hip' does not take this network: {why}")
        prev, self.stack = self.stack, stack
        return prev

    # -- construction ------------------------------------------------------------------------------------------------
    @classmethod
    def from_reference(cls, criterion, stack: str = "torch") -> "LPIPS":
        """From a loaded reference module (lpipsPyTorch.modules.lpips.LPIPS, 'alex' or 'vgg'): walks criterion.net.layers
        (Conv2d / ReLU / MaxPool2d), reads criterion.net.target_layers, .net.mean, .net.std and criterion.lin[i][1].weight.
        The weight tensors are shared, not copied."""
        import torch.nn as nn
        what = "LPIPS.from_reference"
        net = criterion.net
        layers = []
        for name, m in net.layers._modules.items():
            if isinstance(m, nn.Conv2d):
                if _pair(m.dilation) != (1, 1) or m.groups != 1 or m.padding_mode != "zeros" or isinstance(m.padding, str):
                    raise NotImplementedError(f"{what}: layer {name}: only plain zero-padded convolutions, got {m}")
                layers.append(Conv(m.weight.detach(), None if m.bias is None else m.bias.detach(), _pair(m.stride),
                                   _pair(m.padding)))
            elif isinstance(m, nn.ReLU):
                layers.append(Relu())
            elif isinstance(m, nn.MaxPool2d):
                if _pair(m.dilation) != (1, 1):
                    raise NotImplementedError(f"{what}: layer {name}: dilated max-pool, got {m}")
                layers.append(MaxPool(_pair(m.kernel_size), _pair(m.stride if m.stride is not None else m.kernel_size),
                                      _pair(m.padding), bool(m.ceil_mode)))
            else:
                raise NotImplementedError(f"{what}: layer {name} is a {type(m).__name__}, which this module does not run "
                                          "(Conv2d, ReLU and MaxPool2d only: 'alex' and 'vgg'); compute the features "
                                          "yourself and call lpips_distance")
        taps = [int(t) for t in net.target_layers]
        lin = [criterion.lin[i][1].weight for i in range(len(taps))]
        return cls(layers, taps, net.mean, net.std, lin, stack=stack)

    @classmethod
    def from_state_dicts(cls, net_type: str, net_state_dict: Dict[str, Tensor], lin_state_dict: Dict[str, Tensor],
                         stack: str = "torch") -> "LPIPS":
        """From torchvision-keyed weights ('features.0.weight', ... or '0.weight', ...) of alexnet / vgg16 and the LPIPS v0.1
        linear layers, keyed as published ('lin0.model.1.weight') or as the reference renames them ('0.1.weight')."""
        what = "LPIPS.from_state_dicts"
        if net_type not in _TABLES:
            raise NotImplementedError(f"{what}: net_type {net_type!r}: 'alex' and 'vgg' only (compute other networks' "
                                      "features yourself and call lpips_distance)")
        table, taps = _TABLES[net_type]()

        def get(sd, keys):
            for k in keys:
                if k in sd:
                    return sd[k]
            raise ValueError(f"{what}: none of the keys {keys} is in the state dict")

        layers = []
        for pos, row in enumerate(table):
            if row[0] == "conv":
                w = get(net_state_dict, (f"features.{pos}.weight", f"{pos}.weight"))
                b = get(net_state_dict, (f"features.{pos}.bias", f"{pos}.bias"))
                layers.append(Conv(w.detach(), b.detach(), _pair(row[1]), _pair(row[2])))
            elif row[0] == "relu":
                layers.append(Relu())
            else:
                layers.append(MaxPool(_pair(row[1]), _pair(row[2]), _pair(row[3]), row[4]))
        lin = [get(lin_state_dict, (f"lin{k}.model.1.weight", f"{k}.1.weight")) for k in range(len(taps))]
        return cls(layers, taps, MEAN, STD, lin, net_type, stack)

    # -- evaluation --------------------------------------------------------------------------------------------------
    def _stack(self, x: Tensor) -> List[Tensor]:
        """The convolution stack over a prepared input -> the raw taps: on torch, or in HIP when stack == "hip"."""
        if self.stack == "hip":
            # (the sequence was checked when the route was chosen, x comes from the prep kernel: no second validation)
            self._packed = lpips_stack.pack(self.layers, self._packed)
            return lpips_stack._feature_stack_checked(self.layers, self.taps, x, self._packed)
        out, prev = [], None
        for pos, layer in enumerate(self.layers, 1):
            if isinstance(layer, Conv):
                x = F.conv2d(x, layer.weight, layer.bias, layer.stride, layer.padding, layer.dilation)
            elif isinstance(layer, Relu):
                # in place on a convolution's output only: a tap, or the prepared input, must stay as it is
                x = F.relu_(x) if isinstance(prev, Conv) and (pos - 1) not in self.taps else F.relu(x)
            else:
                x = F.max_pool2d(x, layer.kernel, layer.stride, layer.padding, 1, layer.ceil_mode)
            prev = layer
            if pos in self.taps:
                out.append(x)
        return out

    def _features(self, img3: Tensor, m: Optional[Tensor], what: str) -> List[Tensor]:
        return self._stack(_prepare_checked(img3, m, self.mean, self.std, what))

    def features(self, img: Tensor, mask: Optional[Tensor] = None) -> List[Tensor]:
        """The raw taps ([1,C,h,w] each) of where(mask, img, 0): the prep kernel, then the convolution stack."""
        what = "LPIPS.features"
        img3, m, _H, _W = _check_image(img, mask, what)
        return self._features(img3, m, what)

    def target(self, gt: Tensor, mask: Optional[Tensor] = None) -> LPIPSTarget:
        """The ground truth's taps, once per camera: gt * mask does not change between steps."""
        what = "LPIPS.target"
        img3, m, H, W = _check_image(gt, mask, what)
        with torch.no_grad():
            return LPIPSTarget(self._features(img3, m, what), (H, W))

    def __call__(self, image: Tensor, gt_or_target: Union[Tensor, LPIPSTarget], mask: Optional[Tensor] = None) -> Tensor:
        """lpips(image * mask, gt * mask) of the reference -> [1,1,1,1].  With a target() the second pass is skipped."""
        what = "LPIPS"
        img3, m, H, W = _check_image(image, mask, what)
        gt3 = None
        if isinstance(gt_or_target, LPIPSTarget):
            if gt_or_target.size != (H, W):
                raise ValueError(f"{what}: the target was computed for {gt_or_target.size[0]}x{gt_or_target.size[1]}, the "
                                 f"image is {H}x{W}")
            fy = gt_or_target.feats
        else:
            gt3, _m, Hg, Wg = _check_image(gt_or_target, None, what)
            if (Hg, Wg) != (H, W):
                raise ValueError(f"{what}: shape mismatch {tuple(image.shape)} vs {tuple(gt_or_target.shape)}")
        fx = self._features(img3, m, what)
        if gt3 is not None:
            fy = self._features(gt3, m, what)
        return lpips_distance(fx, fy, self.lin_weights)


# ---- the reference's free function -------------------------------------------------------------------------------------
_CRITERIA: Dict[str, LPIPS] = {}


def set_criterion(net_type: str, criterion: Optional[LPIPS]) -> Optional[LPIPS]:
    """Registers the criterion lpips(x, y, net_type) uses (None forgets it); returns the previous one."""
    if criterion is not None and not isinstance(criterion, LPIPS):
        raise TypeError(f"set_criterion: an LPIPS object, got {type(criterion).__name__}")
    prev = _CRITERIA.pop(net_type, None)
    if criterion is not None:
        _CRITERIA[net_type] = criterion
    return prev


def lpips(x: Tensor, y: Tensor, net_type: str = "alex", version: str = "0.1") -> Tensor:
    """lpipsPyTorch.lpips(x, y, net_type, version) over a registered criterion.  Never downloads anything: the caller
    loads the weights and registers them, set_criterion(net_type, LPIPS.from_reference(...))."""
    if version != "0.1":
        raise ValueError(f"lpips: only version '0.1' exists, got {version!r}")
    crit = _CRITERIA.get(net_type)
    if crit is None:
        raise RuntimeError(f"lpips: no criterion registered for net_type {net_type!r}; load the weights yourself and call "
                           f"street_crafter_amd.lpips.set_criterion({net_type!r}, LPIPS.from_reference(reference_module)) "
                           "or LPIPS.from_state_dicts(...): this library ships and fetches none")
    return crit(x, y)
