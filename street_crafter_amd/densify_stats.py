"""Densification statistics: the consumer of the rasterizer's backward side outputs.

Host-side torch mirror of what the reference's training loop does with `viewspace_points.grad`,
`viewspace_points.absgrad`, `visibility_filter` and `radii` after every `loss.backward()`:

    StreetGaussianModel.set_max_radii2D          street_gaussian/models/street_gaussian_model.py:487-497
    StreetGaussianModel.add_densification_stats  street_gaussian/models/street_gaussian_model.py:504-521
    GaussianModelBkgd.densify_and_prune (grads)  street_gaussian/models/gaussian_model_bkgd.py:100-106

It is plain torch (the reference's own code there is plain torch too); it exists so that the
train-path contract of the HIP operators -- `.grad` on a non-leaf projection output, `.absgrad`
attached to the same tensor object, integer `radii` -- is exercised end to end by tests and by the
training benchmark, with the same per-model slicing (`graph_gaussian_range`) the scene graph uses.

The training loop's route is `accumulate_fused` / `DensificationStats.accumulate_from_render_fused`: the same two
updates for every sub-model in one HIP launch (csrc/optim.hip), without the boolean-mask indexing that makes the host
wait for the device five times per sub-model.  The torch methods stay as the statement of the reference's lines that
the kernel is tested against.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from . import _lib
from . import rendering as _r


class DensificationStats:
    """Per sub-model accumulators with the reference's shapes: `xyz_gradient_accum` [n,2]
    (column 0: absgrad norm, column 1: grad norm -- street_gaussian_model.py:518-519), `denom` [n,1],
    `max_radii2D` [n]."""

    def __init__(self, graph_gaussian_range: Dict[str, Tuple[int, int]], device="cuda"):
        self.graph_gaussian_range = dict(graph_gaussian_range)
        self.device = torch.device(device)
        self.xyz_gradient_accum: Dict[str, torch.Tensor] = {}
        self.denom: Dict[str, torch.Tensor] = {}
        self.max_radii2D: Dict[str, torch.Tensor] = {}
        self.reset()

    def reset(self):
        """gaussian_model_bkgd.py:151-153 (after every densify_and_prune)."""
        for name, (start, end) in self.graph_gaussian_range.items():
            n = end - start
            self.xyz_gradient_accum[name] = torch.zeros((n, 2), device=self.device)
            self.denom[name] = torch.zeros((n, 1), device=self.device)
            self.max_radii2D[name] = torch.zeros((n,), device=self.device)

    @torch.no_grad()
    def set_max_radii2D(self, radii: torch.Tensor, visibility_filter: torch.Tensor):
        """radii: what the renderer returns under "radii" (= radii[0] / max(H, W), renderer.py:299)."""
        radii = radii.float()
        for name, (start, end) in self.graph_gaussian_range.items():
            vis = visibility_filter[start:end]
            r = radii[start:end]
            m = self.max_radii2D[name]
            m[vis] = torch.max(m[vis], r[vis])

    @torch.no_grad()
    def add_densification_stats(self, viewspace_point_tensor: torch.Tensor, visibility_filter: torch.Tensor,
                                image_width: int, image_height: int):
        if hasattr(viewspace_point_tensor, "absgrad"):
            g = torch.cat([viewspace_point_tensor.absgrad, viewspace_point_tensor.grad], dim=-1)
            if g.ndim == 3:
                g = g[0]
            g = g * 0.5 * torch.as_tensor([image_width, image_height, image_width, image_height]).to(g)
        else:
            g = viewspace_point_tensor.grad
            if g.ndim == 3:
                g = g[0]
        for name, (start, end) in self.graph_gaussian_range.items():
            vis = visibility_filter[start:end]
            gm = g[start:end]
            acc = self.xyz_gradient_accum[name]
            acc[vis, 0:1] += torch.norm(gm[vis, :2], dim=-1, keepdim=True)
            acc[vis, 1:2] += torch.norm(gm[vis, 2:], dim=-1, keepdim=True)
            self.denom[name][vis] += 1

    def accumulate_from_render_fused(self, out: Dict[str, torch.Tensor], image_width: int, image_height: int):
        """accumulate_from_render through the HIP kernel: both reference calls for every sub-model in one launch."""
        segments = [(start, end, self.xyz_gradient_accum[name], self.denom[name], self.max_radii2D[name])
                    for name, (start, end) in self.graph_gaussian_range.items()]
        accumulate_fused(segments, out["radii"], out["visibility_filter"], out["viewspace_points"], image_width,
                         image_height)

    @torch.no_grad()
    def mean_grads(self, name: str, use_abs: bool = False) -> torch.Tensor:
        """The quantity compared with `densify_grad_threshold` (gaussian_model_bkgd.py:100-105)."""
        col = 1 if use_abs else 0
        grads = self.xyz_gradient_accum[name][:, col:col + 1] / self.denom[name]
        grads[grads.isnan()] = 0.0
        return grads

    @torch.no_grad()
    def clone_split_masks(self, name: str, max_grad: float, scaling_max: torch.Tensor, extent: float,
                          percent_dense: float = 0.01, use_abs: bool = False
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Which Gaussians the next densification step would clone / split
        (selection rules of gaussian_model.py:493-498 densify_and_clone and :452-463
        densify_and_split: gradient over the threshold, size below / above percent_dense * extent)."""
        g = self.mean_grads(name, use_abs).squeeze(-1)
        hot = g >= max_grad
        small = scaling_max <= percent_dense * extent
        return hot & small, hot & ~small


def accumulate_from_render(stats: DensificationStats, out: Dict[str, torch.Tensor], image_width: int,
                           image_height: int):
    """The two calls train.py makes after backward (train.py:283-284): max radii, then the gradient
    statistics, on the renderer's result dict."""
    stats.set_max_radii2D(out["radii"], out["visibility_filter"])
    stats.add_densification_stats(out["viewspace_points"], out["visibility_filter"], image_width, image_height)


def _rows(name: str, t, N=None) -> torch.Tensor:
    """[N,2] or [1,N,2] fp32 on a HIP device -> contiguous [N,2]."""
    what = "accumulate_fused"
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must live on a HIP device (got {t.device}); street_crafter_amd has no CPU path")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2 or t.shape[1] != 2 or (N is not None and t.shape[0] != N):
        raise ValueError(f"{what}: {name} must be [N,2] or [1,N,2]" + (f" with N = {N}" if N is not None else "") +
                         f", got {tuple(t.shape)}")
    return t.contiguous()


@torch.no_grad()
def accumulate_fused(segments: Sequence[Tuple[int, int, torch.Tensor, torch.Tensor, torch.Tensor]], radii: torch.Tensor,
                     visibility_filter: torch.Tensor, viewspace_points: torch.Tensor, image_width: int,
                     image_height: int):
    """set_max_radii2D + add_densification_stats of every sub-model of one render in one HIP launch (csrc/optim.hip,
    sc_densify_stats), without the reference's boolean-mask indexing (five `nonzero`s, i.e. five host waits, per
    sub-model).  `segments`: one (start, end, xyz_gradient_accum [n,2], denom [n,1], max_radii2D [n]) per sub-model,
    n = end - start, rows [start, end) of the render (graph_gaussian_range; the sky model is the same call with its one
    segment); the accumulators are updated in place.  `radii` [N] int32 or fp32 (what the renderer returns under
    "radii"), `visibility_filter` bool [N], `viewspace_points` carries .grad and, if the rasterizer attached it,
    .absgrad, each [N,2] or [1,N,2].  Same values as DensificationStats.set_max_radii2D / add_densification_stats:
    denom and max_radii2D bit for bit, the norms to fp32 rounding.  fp32 on a HIP device only."""
    what = "accumulate_fused"
    if getattr(viewspace_points, "grad", None) is None:
        raise RuntimeError(f"{what}: viewspace_points has no .grad (call after loss.backward())")
    grad = _rows("viewspace_points.grad", viewspace_points.grad)
    N = grad.shape[0]
    absgrad = getattr(viewspace_points, "absgrad", None)
    if absgrad is not None:
        absgrad = _rows("viewspace_points.absgrad", absgrad, N)
    for name, t, dtypes in (("radii", radii, (torch.int32, torch.float32)),
                            ("visibility_filter", visibility_filter, (torch.bool,))):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must live on a HIP device (got {t.device}); "
                               "street_crafter_amd has no CPU path")
        if t.dtype not in dtypes:
            raise ValueError(f"{what}: {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
        if t.numel() != N or t.dim() not in (1, 2) or t.shape[-1] != N:
            raise ValueError(f"{what}: {name} must be [N] or [1,N] with N = {N}, got {tuple(t.shape)}")
        if t.device != grad.device:
            raise ValueError(f"{what}: inputs live on different devices")
    radii, visibility_filter = radii.contiguous(), visibility_filter.contiguous()
    if absgrad is not None and absgrad.device != grad.device:
        raise ValueError(f"{what}: inputs live on different devices")
    ranges, accs, denoms, maxr = [], [], [], []
    for k, seg in enumerate(segments):
        start, end, acc, den, mr = seg
        start, end = int(start), int(end)
        if not 0 <= start <= end <= N:
            raise ValueError(f"{what}: segment {k}: rows [{start}, {end}) do not lie in [0, {N}]")
        n = end - start
        for name, t, shape in (("xyz_gradient_accum", acc, (n, 2)), ("denom", den, (n, 1)), ("max_radii2D", mr, (n,))):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{what}: segment {k}: {name} must be a torch.Tensor, got {type(t).__name__}")
            if not t.is_cuda or t.device != grad.device:
                raise RuntimeError(f"{what}: segment {k}: {name} must live on the render's HIP device {grad.device} "
                                   f"(got {t.device})")
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what}: segment {k}: {name} must be a contiguous float32 {shape}, got {t.dtype} "
                                 f"{tuple(t.shape)} with strides {t.stride()}")
        ranges += [start, end]
        accs.append(acc)
        denoms.append(den)
        maxr.append(mr)
    if not accs:
        return
    rc = _lib.binding().densify_stats(grad, absgrad, radii, visibility_filter, N, 0.5 * float(image_width),
                                      0.5 * float(image_height), ranges, accs, denoms, maxr, _r._stream(grad))
    if rc:
        _lib.check(rc, "sc_densify_stats")
