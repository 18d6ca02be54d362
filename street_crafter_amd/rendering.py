"""gsplat.rendering operator mirror for MI355X.

Same names, argument meaning, return shapes and error behaviour as the six gsplat (v1.0-v1.4
API family) operators StreetCrafter imports at
``street_gaussian/models/street_gaussian_renderer.py:204`` and calls at ``:219-280``.  Every op
launches hand-written HIP kernels through the C ABI (``include/street_crafter_amd.h``) on torch's
current stream; torch is used only for device memory, the stream handle and autograd wiring.
There is no CPU path: non-HIP tensors raise.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .lazy import LazyTensor as _LazyTensor
# a3 / a4 and what the operators share -- the switches, the state kept between calls, the argument helpers -- live in
# isect.py; every name stays reachable here (the same objects)
from .isect import (_ISECT_MODE, _PINNED_META, _RAW_STREAM, _STATE, _SWITCH, _BinCall, _MetaSlot,  # noqa: F401
                    _OperatorState, _PendingIsect, _Switches, _bin_launch_ran, _check_isect_count, _isect_tiles_bin,
                    _isect_tiles_radix, _p, _req, _stream, _tile_work, _view_registry, _warn_once, _ws,
                    isect_offset_encode, isect_tiles, set_deferred_isect, set_isect_mode, set_lazy_isect_ids)

__all__ = ["fully_fused_projection", "isect_tiles", "isect_offset_encode", "spherical_harmonics",
           "rasterize_to_pixels", "rasterization"]


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
class _NoGradCtx:
    """Stands in for the autograd context when no gradient can be required: the forward bodies run
    directly, without torch.autograd.Function.apply's bookkeeping (~10 us of host time per operator,
    which is what bounds small scenes)."""
    needs_input_grad = (False,) * 16

    def save_for_backward(self, *tensors):
        pass

    def mark_non_differentiable(self, *tensors):
        pass

    def __setattr__(self, name, value):      # ctx.meta = ... etc.: nothing is kept
        pass


_NO_GRAD_CTX = _NoGradCtx()
_EMPTY = {}            # device -> a zero-element tensor (placeholder for None in save_for_backward)


def _needs_grad(*args) -> bool:
    return torch.is_grad_enabled() and any(isinstance(a, Tensor) and a.requires_grad for a in args)


def _call(fn, *args):
    """fn.apply(*args), or fn.forward on a dummy context when autograd has nothing to record."""
    if _needs_grad(*args):
        return fn.apply(*args)
    return fn.forward(_NO_GRAD_CTX, *args)


_NATIVE_AUTOGRAD = {"on": True}


def set_native_autograd(enabled: bool) -> bool:
    """The three differentiable operators' autograd plumbing: True (default) = the C++ autograd functions of the compiled
    binding layer (csrc/binding.cpp: forward and backward without a Python frame; the training step is host-bound on a busy
    box), False = the Python torch.autograd.Functions of this module (also what the ctypes path uses and what runs while a
    backward probe is set).  Same kernels, same gradients.  Returns the previous setting."""
    prev, _NATIVE_AUTOGRAD["on"] = _NATIVE_AUTOGRAD["on"], bool(enabled)
    return prev


def _native():
    """The compiled binding layer if ITS autograd functions are to be used for this call, else None."""
    if not _NATIVE_AUTOGRAD["on"] or _BACKWARD_PROBE["events"] is not None or _RAW_STREAM is None:
        return None
    return _lib.fast()


# Measurement hook (bench.py's train-step roofline): autograd calls the backward operators itself, so a harness
# cannot bracket them.  With a dict set here, every backward operator appends a (start, end) pair of HIP events,
# recorded on the current stream around its kernel launch, under its own name.  None (the default): nothing.
_BACKWARD_PROBE = {"events": None}


def set_backward_probe(events):
    """events: dict name -> list to append (torch.cuda.Event, torch.cuda.Event) pairs to, or None.  Returns the old one."""
    prev, _BACKWARD_PROBE["events"] = _BACKWARD_PROBE["events"], events
    return prev


class _probe:
    __slots__ = ("name", "ev")

    def __init__(self, name):
        self.name, self.ev = name, None

    def __enter__(self):
        if _BACKWARD_PROBE["events"] is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev[1].record()
            _BACKWARD_PROBE["events"].setdefault(self.name, []).append(self.ev)
        return False


# ------------------------------------------------------------------------------------------
# a1 fully_fused_projection  (renderer.py:219-232)
# ------------------------------------------------------------------------------------------
class _Projection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane,
                far_plane, radius_clip, calc_compensations):
        rc, radii, means2d, depths, conics, comps = _lib.binding().projection_fwd(
            means, quats, scales, viewmats, Ks, int(width), int(height), float(eps2d), float(near_plane),
            float(far_plane), float(radius_clip), bool(calc_compensations), _stream(means))
        if rc:
            _lib.check(rc, "sc_projection_fwd")
        ctx.save_for_backward(means, quats, scales, viewmats, Ks, radii, conics,
                              comps if comps is not None else torch.empty(0, device=means.device))
        ctx.dims = (int(width), int(height), float(eps2d), bool(calc_compensations))
        ctx.mark_non_differentiable(radii)
        if comps is None:
            return radii, means2d, depths, conics
        return radii, means2d, depths, conics, comps

    @staticmethod
    def backward(ctx, v_radii, v_means2d, v_depths, v_conics, v_comps=None):
        means, quats, scales, viewmats, Ks, radii, conics, comps = ctx.saved_tensors
        width, height, eps2d, has_comp = ctx.dims
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device

        def z(t, shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev) if t is None else t.contiguous()

        v_means2d = z(v_means2d, (C, N, 2))
        v_depths = z(v_depths, (C, N))
        v_conics = z(v_conics, (C, N, 3))
        if has_comp:
            v_comps = z(v_comps, (C, N))
        if ctx.needs_input_grad[3]:
            return _projection_bwd_cam(ctx, means, quats, scales, viewmats, Ks, radii, conics, comps if has_comp else None,
                                       v_means2d, v_depths, v_conics, v_comps if has_comp else None)
        with _probe("projection_bwd"):
            rc, v_means, v_quats, v_scales = _lib.binding().projection_bwd(
                means, quats, scales, viewmats, Ks, width, height, eps2d, radii, conics, comps if has_comp else None,
                v_means2d, v_depths, v_conics, v_comps if has_comp else None, _stream(means))
        if rc:
            _lib.check(rc, "sc_projection_bwd")
        return (v_means if ctx.needs_input_grad[0] else None,
                v_quats if ctx.needs_input_grad[1] else None,
                v_scales if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None, None, None, None)


def _projection_bwd_cam(ctx, means, quats, scales, viewmats, Ks, radii, conics, comps, v_means2d, v_depths, v_conics,
                        v_comps):
    """_Projection.backward when the cameras require grad: sc_projection_bwd_cam (csrc/projection_cam.hip) -- the
    per-Gaussian gradients anybody needs (sc_projection_bwd's kernel: the same bits) and v_viewmats [C,4,4], summed
    without float atomics.  Ks gets no gradient, as in gsplat."""
    lib = _lib.load()
    width, height, eps2d, _ = ctx.dims
    C, N = viewmats.shape[0], means.shape[0]
    dev = means.device
    need = ctx.needs_input_grad

    def out(k, cols):
        return torch.empty((N, cols), dtype=torch.float32, device=dev) if need[k] else None

    v_means, v_quats, v_scales = out(0, 3), out(1, 4), out(2, 3)
    v_viewmats = torch.empty((C, 4, 4), dtype=torch.float32, device=dev)
    ws = _ws(lib.sc_projection_bwd_cam_workspace_bytes(C, N), dev)
    with _probe("projection_bwd_cam"):
        rc = lib.sc_projection_bwd_cam(_p(means), _p(quats), _p(scales), _p(viewmats), _p(Ks), C, N, width, height, eps2d,
                                       _p(radii), _p(conics), _p(comps), _p(v_means2d), _p(v_depths), _p(v_conics),
                                       _p(v_comps), _p(v_means), _p(v_quats), _p(v_scales), _p(v_viewmats), _p(ws),
                                       _stream(means))
    if rc:
        _lib.check(rc, "sc_projection_bwd_cam")
    return (v_means, v_quats, v_scales, v_viewmats, None, None, None, None, None, None, None, None)


def fully_fused_projection(means: Tensor, covars: Optional[Tensor], quats: Optional[Tensor],
                           scales: Optional[Tensor], viewmats: Tensor, Ks: Tensor, width: int,
                           height: int, eps2d: float = 0.3, near_plane: float = 0.01,
                           far_plane: float = 1e10, radius_clip: float = 0.0, packed: bool = False,
                           sparse_grad: bool = False, calc_compensations: bool = False):
    """means [N,3], quats [N,4] (wxyz), scales [N,3], viewmats [C,4,4], Ks [C,3,3] ->
    (radii i32[C,N], means2d [C,N,2], depths [C,N], conics [C,N,3], compensations [C,N] | None).
    Differentiable in means, quats, scales and viewmats (gsplat's v_viewmats; bottom row of the gradient +0); not in Ks."""
    if covars is not None:
        raise NotImplementedError("covars= is not supported: the reference passes quats/scales "
                                  "(street_gaussian_renderer.py:219-224)")
    if packed:
        raise NotImplementedError("packed=True is not supported: the reference passes packed=False "
                                  "(street_gaussian_renderer.py:228)")
    assert quats is not None and scales is not None, "quats and scales are required"
    means = _req(means, "means")
    quats = _req(quats, "quats")
    scales = _req(scales, "scales")
    viewmats = _req(viewmats, "viewmats")
    Ks = _req(Ks, "Ks")
    N = means.shape[0]
    C = viewmats.shape[0]
    assert means.shape == (N, 3), means.shape
    assert quats.shape == (N, 4), quats.shape
    assert scales.shape == (N, 3), scales.shape
    assert viewmats.shape == (C, 4, 4), viewmats.shape
    assert Ks.shape == (C, 3, 3), Ks.shape
    # cameras under grad (pose optimisation): the Python Function, whose backward returns v_viewmats as well
    cam_grad = viewmats.requires_grad and torch.is_grad_enabled()
    nat = _native() if not cam_grad and _needs_grad(means, quats, scales) else None
    if nat is not None:
        out = nat.projection_autograd(means, quats, scales, viewmats, Ks, int(width), int(height), float(eps2d),
                                      float(near_plane), float(far_plane), float(radius_clip), bool(calc_compensations),
                                      _RAW_STREAM)
    else:
        out = _call(_Projection, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane,
                                far_plane, radius_clip, calc_compensations)
    if N and C:
        # means2d carries the cameras to isect_tiles (view slots); detached, so that a means2d somebody keeps (meta) does
        # not hold the graph behind a camera under grad any longer than its own grad_fn does
        out[1]._sc_viewmats = viewmats.detach() if viewmats.requires_grad else viewmats
    if calc_compensations:
        return out
    return (*out, None)


def set_tile_order(enabled: bool) -> bool:
    """Longest-running-tile-first dispatch of the rasterizer (A/B switch; results are identical either way).
    Returns the previous setting."""
    return _SWITCH.flip("tile_order", enabled)


def set_packed_records(enabled: bool) -> bool:
    """A/B switch of the fused forward's packed rasterizer records (results are identical either way).  Returns the
    previous setting."""
    return _SWITCH.flip("packed_records", enabled)


def set_view_slots(enabled: bool) -> bool:
    """The rasterizer's work hint per VIEW (A/B switch; results are identical either way): a rig's cameras rendered
    in turn each find the hint their own last frame left.  Returns the previous setting."""
    return _SWITCH.flip("view_slots", enabled)


# ------------------------------------------------------------------------------------------
# a6 spherical_harmonics  (renderer.py:259)
# ------------------------------------------------------------------------------------------
class _SphericalHarmonics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degree, dirs, coeffs, masks):
        rc, colors = _lib.binding().sh_fwd(int(degree), dirs, coeffs, masks, _stream(dirs))
        if rc:
            _lib.check(rc, "sc_sh_fwd")
        ctx.save_for_backward(dirs, coeffs, masks if masks is not None else torch.empty(0, device=dirs.device))
        ctx.meta = (int(degree), masks is not None)
        return colors

    @staticmethod
    def backward(ctx, v_colors):
        dirs, coeffs, masks = ctx.saved_tensors
        degree, has_mask = ctx.meta
        v_colors = v_colors.contiguous()
        with _probe("spherical_harmonics_bwd"):
            rc, v_coeffs, v_dirs = _lib.binding().sh_bwd(degree, dirs, coeffs, masks if has_mask else None, v_colors,
                                                         bool(ctx.needs_input_grad[1]), _stream(dirs))
        if rc:
            _lib.check(rc, "sc_sh_bwd")
        return None, v_dirs, (v_coeffs if ctx.needs_input_grad[2] else None), None


def spherical_harmonics(degrees_to_use: int, dirs: Tensor, coeffs: Tensor,
                        masks: Optional[Tensor] = None) -> Tensor:
    """dirs [...,3] (not normalised by the caller, renderer.py:256), coeffs [...,K,3], masks [...]."""
    assert 0 <= degrees_to_use <= 4, degrees_to_use
    assert (degrees_to_use + 1) ** 2 <= coeffs.shape[-2], coeffs.shape
    assert dirs.shape[:-1] == coeffs.shape[:-2], (dirs.shape, coeffs.shape)
    assert dirs.shape[-1] == 3 and coeffs.shape[-1] == 3, (dirs.shape, coeffs.shape)
    dirs = _req(dirs, "dirs")
    coeffs = _req(coeffs, "coeffs")
    if masks is not None:
        assert masks.shape == dirs.shape[:-1], masks.shape
        if not masks.is_cuda:
            raise RuntimeError("masks must live on a HIP device")
        if masks.dtype == torch.bool:
            masks = masks.contiguous().view(torch.uint8)      # same bytes (0/1), no conversion kernel
        elif masks.dtype != torch.uint8:
            masks = masks.to(torch.uint8).contiguous()
        else:
            masks = masks.contiguous()
    nat = _native() if _needs_grad(dirs, coeffs) else None
    if nat is not None:
        return nat.sh_autograd(int(degrees_to_use), dirs, coeffs, masks, _RAW_STREAM)
    return _call(_SphericalHarmonics, int(degrees_to_use), dirs, coeffs, masks)


# ------------------------------------------------------------------------------------------
# a9 rasterize_to_pixels  (renderer.py:267-280)
# ------------------------------------------------------------------------------------------
def set_planar_output(enabled: bool) -> bool:
    """Storage of rasterize_to_pixels' `render_colors` under no_grad (tile_size 16, 3 or 4 channels): True (default) = one plane
    per channel, [C][D][H][W], returned as the permuted [C,H,W,D] view; False = interleaved as before.  Values, shapes and every
    indexing expression are the same; what the reference's caller does with the result right behind the operator
    (renderer.py:282-300: `[..., :-1]`, `[..., -1:] / alpha`, clamp, `.permute(2, 0, 1)`) becomes dense kernels instead of
    strided ones (-10 us per 1920x1280 frame, tools/exp_glue_layout.py).  The tensor is not `is_contiguous()` in this form
    (`.view(-1)` on it needs `.reshape`).  Training (anything requires grad) always takes the interleaved form.  Returns the
    previous setting."""
    return _SWITCH.flip("planar_out", enabled)


_RASTER_SIDE = {}      # device index -> {raw handle of the caller's stream (None = any): torch stream the rasterizer runs on}


def set_raster_side_stream(device, side, main=None):
    """Frame-loop option (dist.make_stream; bench.py --raster-cus / --raster-priority): the INFERENCE rasterizer of `device`
    is launched on the stream `side` -- typically one confined to a subset of the CUs or of lower priority -- instead of on
    the caller's current stream, fenced by events on both sides, so that the results and their ordering are unchanged.
    With several frames in flight the one-wave workgroups of the VALU-bound rasterizer otherwise take every free wave slot
    and the next frame's latency-bound intersection kernels (8..16-wave workgroups) wait for whole CUs to drain.
    `main`: only rasterizer calls issued under this stream (a torch stream) use `side`; None = calls under any stream.
    side=None removes the entry.  Returns the previous side stream of that (device, main)."""
    idx = device if isinstance(device, int) else torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    tab = _RASTER_SIDE.setdefault(idx, {})
    key = None if main is None else int(main.cuda_stream)
    prev = tab.get(key)
    if side is None:
        tab.pop(key, None)
        if not tab:
            _RASTER_SIDE.pop(idx, None)
    else:
        tab[key] = side
    return prev


def reset_state(device=None) -> dict:
    """Forgets everything the operators remember BETWEEN calls -- the size predictions and their history, the
    rasterizer's per-view work hints and view registries, the last counts -- for `device` (an index or torch.device;
    None = all devices).  None of it is ever needed for a correct result (every piece is a hint that the kernels verify
    or that only orders work); a long-running process that is done with a scene may call this to hand the hint buffers
    (32 B x tiles per frame shape, at most 8 shapes) back, and tests use it to start from a cold state.  The A/B
    switches (set_tile_order, set_deferred_isect, ...) are not state and keep their values.  Call it between frames:
    an isect_tiles call whose outputs have not been looked at yet is settled first.
    tests/test_call_history_gpu.py holds this promise to its word: every call of scripted call histories (shapes, scenes,
    cameras, modes and switches in turn, deferred calls settled late, by someone else or never) returns bit for bit what
    the same call returns right after reset_state().
    -> how many entries of each table were dropped."""
    idx = None if device is None else (device if isinstance(device, int) else torch.device(device).index)
    for d, slot in getattr(_PINNED_META, "slots", {}).items():
        if idx is None or d == idx:
            slot.settle_pending("settle_reset", "reset_state: settling a never observed isect_tiles call failed (%s: %s)")
    return _STATE.reset(idx)


def _sched_of(isect_offsets, n_tiles):
    """(tile_order, tile_work) the intersection stage left on this isect_offsets tensor, or (None, None)."""
    sched = getattr(isect_offsets, "_sc_sched", None) if _SWITCH.tile_order else None
    if sched is None:
        return None, None
    want = _STATE.sched_sizes.get(n_tiles)
    if want is None:       # (two foreign calls per frame otherwise)
        if len(_STATE.sched_sizes) > 64:
            _STATE.sched_sizes.clear()
        want = _STATE.sched_sizes[n_tiles] = (_lib.load().sc_view_slots() * n_tiles, _lib.load().sc_tile_order_len(n_tiles))
    if sched[1].numel() != want[0] or sched[0].device != isect_offsets.device or sched[0].numel() != want[1]:
        return None, None
    return sched


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2d, conics, colors, opacities, backgrounds, masks, width, height, tile_size,
                isect_offsets, flatten_ids, absgrad, means2d_obj):
        C = opacities.shape[0]
        D = colors.shape[-1]
        th, tw = isect_offsets.shape[1], isect_offsets.shape[2]
        dev = means2d.device
        # last_ids only feeds the backward replay: inference (no input requires grad) skips it
        needs_bwd = any(ctx.needs_input_grad[:5])
        order, work = _sched_of(isect_offsets, C * tw * th)
        b = _lib.binding()
        st = _stream(means2d)
        side = cur = None
        if _RASTER_SIDE and not needs_bwd:         # set_raster_side_stream: the kernel runs on another stream, fenced by events
            tab = _RASTER_SIDE.get(dev.index)
            side = (tab.get(st) or tab.get(None)) if tab else None
            if side is not None:
                # (the outputs are allocated under the caller's stream as always: every later use of them on that stream is
                #  behind the second event, and the inputs outlive the kernel for the same reason)
                cur = torch.cuda.current_stream(dev)
                ev = torch.cuda.Event()
                ev.record(cur)
                side.wait_event(ev)
                st = side.cuda_stream
        rc = _lib.SC_EUNSUPPORTED
        last_ids = None
        if _SWITCH.planar_out and not needs_bwd and int(tile_size) == 16 and D in (3, 4):
            # inference: one plane per channel behind the same [C,H,W,D] indexing (set_planar_output); SC_EUNSUPPORTED = not this kernel
            rc, render_colors, render_alphas = b.rasterize_fwd_planar(
                means2d, conics, colors, opacities, backgrounds, masks, int(width), int(height), int(tile_size),
                isect_offsets, flatten_ids, order, work, st)
            if rc not in (0, _lib.SC_EUNSUPPORTED):
                _lib.check(rc, "sc_rasterize_fwd_planar")
        if rc == _lib.SC_EUNSUPPORTED:
            rc, render_colors, render_alphas, last_ids = b.rasterize_fwd(
                means2d, conics, colors, opacities, backgrounds, masks, int(width), int(height), int(tile_size),
                isect_offsets, flatten_ids, bool(needs_bwd), order, work, st)
            if rc:
                _lib.check(rc, "sc_rasterize_fwd")
        if side is not None:
            ev = torch.cuda.Event()
            ev.record(side)
            cur.wait_event(ev)
        e = _EMPTY.get(dev)
        if e is None:
            e = _EMPTY[dev] = torch.empty(0, device=dev)
        ctx.save_for_backward(means2d, conics, colors, opacities, backgrounds if backgrounds is not None else e,
                              masks if masks is not None else e, isect_offsets, flatten_ids, render_alphas,
                              last_ids if last_ids is not None else e)
        ctx.meta = (int(width), int(height), int(tile_size), bool(absgrad), backgrounds is not None,
                    masks is not None)
        ctx.means2d_obj = means2d_obj
        ctx.tile_order = order
        return render_colors, render_alphas

    @staticmethod
    def backward(ctx, v_render_colors, v_render_alphas):
        (means2d, conics, colors, opacities, backgrounds, masks, isect_offsets, flatten_ids, render_alphas,
         last_ids) = ctx.saved_tensors
        width, height, tile_size, absgrad, has_bg, has_mask = ctx.meta
        v_render_colors = v_render_colors.contiguous()
        v_render_alphas = v_render_alphas.contiguous()
        # (the five gradient buffers share ONE zero-fill, inside the call: the kernel accumulates with float atomics)
        with _probe("rasterize_to_pixels_bwd"):
            rc, v_means2d, v_conics, v_colors, v_opacities, v_abs = _lib.binding().rasterize_bwd(
                means2d, conics, colors, opacities, backgrounds if has_bg else None, masks if has_mask else None,
                width, height, tile_size, isect_offsets, flatten_ids, render_alphas, last_ids, v_render_colors,
                v_render_alphas, bool(absgrad), ctx.tile_order, _stream(means2d))
        if rc:
            _lib.check(rc, "sc_rasterize_bwd")
        if absgrad:
            # gsplat contract: the tensor object the CALLER passed gets an `.absgrad` attribute
            # (read at street_gaussian/models/street_gaussian_model.py:505-506)
            ctx.means2d_obj.tensor.absgrad = v_abs
        v_bg = None
        if has_bg and ctx.needs_input_grad[4]:
            v_bg = (v_render_colors * (1.0 - render_alphas)).sum(dim=(1, 2))
        return (v_means2d, v_conics, v_colors, v_opacities, v_bg, None, None, None, None, None, None, None, None)


class _AbsgradTarget:
    """Carries the caller's means2d tensor OBJECT through autograd untouched, so that backward can
    attach `.absgrad` to it (gsplat's contract, relied on at street_gaussian_model.py:505-506)."""
    __slots__ = ("tensor",)

    def __init__(self, tensor):
        self.tensor = tensor


def rasterize_to_pixels(means2d: Tensor, conics: Tensor, colors: Tensor, opacities: Tensor,
                        image_width: int, image_height: int, tile_size: int, isect_offsets: Tensor,
                        flatten_ids: Tensor, backgrounds: Optional[Tensor] = None,
                        masks: Optional[Tensor] = None, packed: bool = False,
                        absgrad: bool = False) -> Tuple[Tensor, Tensor]:
    """-> (render_colors [C,H,W,D], render_alphas [C,H,W,1])."""
    if packed:
        raise NotImplementedError("packed=True is not supported (reference passes packed=False)")
    caller_means2d = means2d
    means2d_c = _req(means2d, "means2d")
    conics = _req(conics, "conics")
    colors = _req(colors, "colors")
    opacities = _req(opacities, "opacities")
    isect_offsets = _req(isect_offsets, "isect_offsets", torch.int32)
    if type(flatten_ids) is _LazyTensor:      # isect_tiles' deferred list: the frame's counts are settled here (lazy.py)
        flatten_ids = flatten_ids.plain()
    flatten_ids = _req(flatten_ids, "flatten_ids", torch.int32)
    C, N = opacities.shape
    D = colors.shape[-1]
    assert means2d_c.shape == (C, N, 2), means2d_c.shape
    assert conics.shape == (C, N, 3), conics.shape
    assert colors.shape == (C, N, D), colors.shape
    assert isect_offsets.ndim == 3 and isect_offsets.shape[0] == C, isect_offsets.shape
    th, tw = isect_offsets.shape[1], isect_offsets.shape[2]
    assert tw * tile_size >= image_width, "image_width must fit in tile_width * tile_size"
    assert th * tile_size >= image_height, "image_height must fit in tile_height * tile_size"
    if not 1 <= D <= 32:
        raise NotImplementedError(f"colour channels must be in 1..32, got {D}")
    if backgrounds is not None:
        backgrounds = _req(backgrounds, "backgrounds")
        assert backgrounds.shape == (C, D), backgrounds.shape
    if masks is not None:
        assert masks.shape == isect_offsets.shape, masks.shape
        if not masks.is_cuda:
            raise RuntimeError("masks must live on a HIP device")
        masks = masks.to(torch.uint8).contiguous()

    nat = _native() if _needs_grad(means2d_c, conics, colors, opacities, backgrounds) else None
    if nat is not None:
        order, work = _sched_of(isect_offsets, C * tw * th)
        return nat.rasterize_autograd(means2d_c, conics, colors, opacities, backgrounds, masks, int(image_width),
                                      int(image_height), int(tile_size), isect_offsets, flatten_ids, bool(absgrad), order,
                                      work, caller_means2d, _RAW_STREAM)
    return _call(_Rasterize, means2d_c, conics, colors, opacities, backgrounds, masks, int(image_width),
                            int(image_height), int(tile_size), isect_offsets, flatten_ids, bool(absgrad),
                            _AbsgradTarget(caller_means2d))


# ------------------------------------------------------------------------------------------
# a13 rasterization  (imported at renderer.py:204, never called there): thin composition
# ------------------------------------------------------------------------------------------
def camera_centers(viewmats: Tensor) -> Tensor:
    """[C,3] camera positions -R^T t of rigid world-to-camera matrices [C,4,4] (what the reference keeps
    as Camera.camera_center, camera_utils.py:51, and gsplat takes from inverse(viewmats)).  Carries a graph when
    `viewmats` requires grad (pose optimisation); plain otherwise."""
    viewmats = _req(viewmats, "viewmats")
    if viewmats.requires_grad and torch.is_grad_enabled():
        return _CameraCenters.apply(viewmats)
    return _CameraCenters.forward(_NO_GRAD_CTX, viewmats)


class _CameraCenters(torch.autograd.Function):
    """sc_camera_centers and its VJP sc_camera_centers_bwd (csrc/projection_cam.hip): one launch each, no host wait."""

    @staticmethod
    def forward(ctx, viewmats):
        lib = _lib.load()
        out = torch.empty((viewmats.shape[0], 3), dtype=torch.float32, device=viewmats.device)
        _lib.check(lib.sc_camera_centers(_p(viewmats), viewmats.shape[0], _p(out), _stream(viewmats)),
                   "sc_camera_centers")
        ctx.save_for_backward(viewmats)
        return out

    @staticmethod
    def backward(ctx, v_centers):
        viewmats, = ctx.saved_tensors
        C = viewmats.shape[0]
        v_centers = v_centers.contiguous()
        v_viewmats = torch.empty((C, 4, 4), dtype=torch.float32, device=viewmats.device)
        with _probe("camera_centers_bwd"):
            rc = _lib.load().sc_camera_centers_bwd(_p(viewmats), _p(v_centers), C, _p(v_viewmats), _stream(viewmats))
        if rc:
            _lib.check(rc, "sc_camera_centers_bwd")
        return v_viewmats


_FUSED_RASTERIZATION = True


def set_fused_rasterization(enabled: bool) -> bool:
    """A/B switch for `rasterization()`'s fused forward (tests compare both); returns the old value."""
    global _FUSED_RASTERIZATION
    prev, _FUSED_RASTERIZATION = _FUSED_RASTERIZATION, bool(enabled)
    return prev


def _fused_forward_ok(tensors, sh_degree, render_mode, tile_size, colors) -> bool:
    if not _FUSED_RASTERIZATION or sh_degree is None or render_mode not in ("RGB+D", "RGB+ED"):
        return False
    if tile_size != 16 or colors.dim() != 3 or colors.shape[-1] != 3:
        return False
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        return False         # the fused path is forward-only; training goes through the autograd operators
    return True


def set_fused_training(enabled: bool) -> bool:
    """`rasterization()` under grad: True = projection, opacity x compensation, dirs, SH, clamp and the depth channel as one
    forward and one backward kernel (_ProjectionSh), False (default, SC_FUSED_TRAIN) = the operator composition.  Same
    forward bit for bit; gradients equal within rounding.  Returns the previous setting."""
    return _SWITCH.flip("fused_train", enabled)


def _fused_train_ok(leaves, cameras, sh_degree, render_mode, tile_size, colors) -> bool:
    """The training form of _fused_forward_ok: its conditions on the call, a leaf that requires grad, cameras that do not."""
    if not _SWITCH.fused_train or not _FUSED_RASTERIZATION or sh_degree is None or render_mode not in ("RGB+D", "RGB+ED"):
        return False
    if tile_size != 16 or colors.dim() != 3 or colors.shape[-1] != 3:
        return False
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in leaves):
        return False
    return not any(t is not None and t.requires_grad for t in cameras)


class _ProjectionSh(torch.autograd.Function):
    """sc_projection_sh_fwd (the four separate arrays, no records) and its one-kernel VJP sc_projection_sh_bwd with
    respect to means, quats, scales, opacities [N] and sh [N,K,3]; the cameras carry no gradient."""

    @staticmethod
    def forward(ctx, means, quats, scales, opacities, sh, viewmats, Ks, centers, sh_degree, width, height, eps2d,
                near_plane, far_plane, radius_clip, antialiased):
        rc, radii, means2d, depths, _, conics, opac, cols = _lib.binding().projection_sh_fwd(
            means, quats, scales, opacities, sh, viewmats, Ks, centers, int(sh_degree), int(width), int(height),
            float(eps2d), float(near_plane), float(far_plane), float(radius_clip), bool(antialiased), False,
            _stream(means))
        if rc:
            _lib.check(rc, "sc_projection_sh_fwd")
        ctx.save_for_backward(means, quats, scales, opacities, sh, viewmats, Ks, centers, radii, conics)
        ctx.dims = (int(sh_degree), int(width), int(height), float(eps2d), bool(antialiased))
        ctx.mark_non_differentiable(radii)
        return radii, means2d, depths, conics, opac, cols

    @staticmethod
    def backward(ctx, v_radii, v_means2d, v_depths, v_conics, v_opac, v_cols):
        means, quats, scales, opacities, sh, viewmats, Ks, centers, radii, conics = ctx.saved_tensors
        sh_degree, width, height, eps2d, antialiased = ctx.dims
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device

        def z(t, shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev) if t is None else t.contiguous()

        v_means2d = z(v_means2d, (C, N, 2))
        v_conics = z(v_conics, (C, N, 3))
        v_opac = z(v_opac, (C, N))
        v_cols = z(v_cols, (C, N, 4))
        v_depths = None if v_depths is None else v_depths.contiguous()     # (the depth usually arrives as colour channel 3)
        need = tuple(bool(g) for g in ctx.needs_input_grad[:5])
        with _probe("projection_sh_bwd"):
            rc, *grads = _lib.binding().projection_sh_bwd(
                means, quats, scales, opacities, sh, viewmats, Ks, centers, sh_degree, width, height, eps2d, antialiased,
                radii, conics, v_means2d, v_depths, v_conics, v_opac, v_cols, *need, _stream(means))
        if rc:
            _lib.check(rc, "sc_projection_sh_bwd")
        return (*grads, None, None, None, None, None, None, None, None, None, None, None)


def _rasterization_fused_train(means, quats, scales, opacities, colors, viewmats, Ks, width, height, near_plane,
                               far_plane, radius_clip, eps2d, sh_degree, tile_size, backgrounds, render_mode,
                               antialiased, centers, absgrad):
    """The training route of `rasterization()` (set_fused_training): the per-Gaussian part is ONE autograd node
    (_ProjectionSh); a3 / a4 and the rasterizer are the operators the composition calls, so the dispatch list, last_ids
    and the `.absgrad` contract are theirs, and `means2d` stays a tensor between two nodes -- `meta["means2d"]
    .retain_grad()`, `.grad` and `.absgrad` work as the reference's densification reads them."""
    means, quats, scales = _req(means, "means"), _req(quats, "quats"), _req(scales, "scales")
    viewmats, Ks = _req(viewmats, "viewmats"), _req(Ks, "Ks")
    opacities = _req(opacities, "opacities").reshape(-1)
    colors = _req(colors, "colors")
    C, N = viewmats.shape[0], means.shape[0]
    assert means.shape == (N, 3) and quats.shape == (N, 4) and scales.shape == (N, 3), (means.shape, quats.shape, scales.shape)
    assert opacities.shape[0] == N and colors.shape[0] == N, (opacities.shape, colors.shape)
    assert viewmats.shape == (C, 4, 4) and Ks.shape == (C, 3, 3), (viewmats.shape, Ks.shape)
    centers = camera_centers(viewmats) if centers is None else _req(centers, "camera_centers").reshape(C, 3)
    radii, means2d, depths, conics, opac, cols = _ProjectionSh.apply(
        means, quats, scales, opacities, colors, viewmats, Ks, centers, sh_degree, width, height, eps2d, near_plane,
        far_plane, radius_clip, antialiased)
    if N and C:
        means2d._sc_viewmats = viewmats          # means2d carries the cameras to isect_tiles (view slots)
    tile_width = math.ceil(width / float(tile_size))
    tile_height = math.ceil(height / float(tile_size))
    tiles_per_gauss, isect_ids, flatten_ids = isect_tiles(means2d, radii, depths, tile_size, tile_width,
                                                          tile_height, packed=False, n_cameras=C)
    isect_offsets = isect_offset_encode(isect_ids, C, tile_width, tile_height)
    if backgrounds is not None:
        backgrounds = torch.cat([backgrounds, torch.zeros(C, 1, device=backgrounds.device)], dim=-1)
    render_colors, render_alphas = rasterize_to_pixels(means2d, conics, cols, opac, width, height, tile_size,
                                                       isect_offsets, flatten_ids, backgrounds=backgrounds, packed=False,
                                                       absgrad=absgrad)
    if render_mode == "RGB+ED":
        render_colors = torch.cat([render_colors[..., :-1],
                                   render_colors[..., -1:] / render_alphas.clamp(min=1e-10)], dim=-1)
    meta = {"radii": radii, "means2d": means2d, "depths": depths, "conics": conics, "opacities": opac,
            "tile_width": tile_width, "tile_height": tile_height, "tiles_per_gauss": tiles_per_gauss,
            "isect_ids": isect_ids, "flatten_ids": flatten_ids, "isect_offsets": isect_offsets,
            "width": width, "height": height, "tile_size": tile_size, "n_cameras": C, "colors": cols,
            "fused": True}
    return render_colors, render_alphas, meta


class _FusedMeta(dict):
    """gsplat's meta dict.  The fused forward does not materialise `isect_ids` (8 B x I of keys nothing on
    this path reads); `meta["isect_ids"]` builds them on first access from the tensors already here.  Likewise
    `conics` / `opacities` / `colors` when the rasterizer gathered from packed records: first access unpacks them."""

    _FROM_RECORDS = ("conics", "opacities", "colors")

    def get(self, key, default=None):
        try:
            return self[key]
        except KeyError:
            return default

    def __contains__(self, key):
        return (dict.__contains__(self, key) or key == "isect_ids"
                or (key in self._FROM_RECORDS and getattr(self, "_sc_records", None) is not None))

    def __missing__(self, key):
        if key in self._FROM_RECORDS and getattr(self, "_sc_records", None) is not None:
            # the fused frame gathered these from the rasterizer's packed records and never wrote the arrays:
            # one kernel rebuilds all three on first access, on the current stream
            rec, (C, N), producer = self._sc_records          # (kept as an attribute: not one of gsplat's keys)
            dev = rec.device
            out = {"conics": torch.empty((C, N, 3), dtype=torch.float32, device=dev),
                   "opacities": torch.empty((C, N), dtype=torch.float32, device=dev),
                   "colors": torch.empty((C, N, 4), dtype=torch.float32, device=dev)}
            cur = torch.cuda.current_stream(dev)
            if cur != producer:
                cur.wait_stream(producer)
            _lib.check(_lib.load().sc_records_unpack(rec.data_ptr(), C * N, out["conics"].data_ptr(),
                                                     out["opacities"].data_ptr(), out["colors"].data_ptr(),
                                                     cur.cuda_stream), "sc_records_unpack")
            for k, v in out.items():
                self[k] = v
            return out[key]
        if key != "isect_ids":
            raise KeyError(key)
        with torch.no_grad():
            _, ids, _ = isect_tiles(self["means2d"], self["radii"], self["depths"], self["tile_size"],
                                    self["tile_width"], self["tile_height"], packed=False,
                                    n_cameras=self["n_cameras"])
        self[key] = ids
        return ids


@torch.no_grad()
def _rasterization_fused(means, quats, scales, opacities, colors, viewmats, Ks, width, height, near_plane,
                         far_plane, radius_clip, eps2d, sh_degree, tile_size, backgrounds, render_mode,
                         antialiased, centers):
    """a1 + a2 + a5 + a6 + a7 in one kernel, a3/a4 unchanged, a9 with the depth-normalising
    epilogue of renderer.py:284 -- three operator-level launches and no torch elementwise kernels."""
    lib = _lib.load()
    means, quats, scales = _req(means, "means"), _req(quats, "quats"), _req(scales, "scales")
    viewmats, Ks = _req(viewmats, "viewmats"), _req(Ks, "Ks")
    opacities = _req(opacities, "opacities").reshape(-1)
    colors = _req(colors, "colors")
    C, N = viewmats.shape[0], means.shape[0]
    assert opacities.shape[0] == N and colors.shape[0] == N, (opacities.shape, colors.shape)
    dev = means.device
    centers = camera_centers(viewmats) if centers is None else _req(centers, "camera_centers").reshape(C, 3)
    st = _stream(means)
    b = _lib.binding()
    # the rasterizer's 48-B record per (camera, Gaussian): one gather line per splat instead of four.  With it the
    # conics / opacities / colours arrays of `meta` are not written at all (32 B per Gaussian the frame never reads):
    # _FusedMeta rebuilds them from the records on first access
    use_records = _SWITCH.packed_records and int(tile_size) == 16 and N > 0 and C > 0
    rc, radii, means2d, depths, records, conics, opac, cols = b.projection_sh_fwd(
        means, quats, scales, opacities, colors, viewmats, Ks, centers, int(sh_degree), int(width), int(height),
        float(eps2d), float(near_plane), float(far_plane), float(radius_clip), bool(antialiased), bool(use_records), st)
    if rc:
        _lib.check(rc, "sc_projection_sh_fwd")
    tile_width = math.ceil(width / float(tile_size))
    tile_height = math.ceil(height / float(tile_size))
    res = None
    if _ISECT_MODE["mode"] == "bin":
        res = _isect_tiles_bin(means2d, radii, depths, C, N, tile_size, tile_width, tile_height, st, want_ids=False,
                               viewmats=viewmats)
    if res is not None:
        tiles_per_gauss, isect_ids, flatten_ids, isect_offsets = res
    else:
        tiles_per_gauss, isect_ids, flatten_ids = isect_tiles(means2d, radii, depths, tile_size, tile_width,
                                                              tile_height, packed=False, n_cameras=C)
        isect_offsets = isect_offset_encode(isect_ids, C, tile_width, tile_height)
    if backgrounds is not None:
        backgrounds = torch.cat([_req(backgrounds, "backgrounds"),
                                 torch.zeros(C, 1, device=dev)], dim=-1).contiguous()
    order, work = _sched_of(isect_offsets, C * tile_width * tile_height)
    if records is not None:
        rc, render_colors, render_alphas = b.rasterize_fwd_packed(records, backgrounds, int(width), int(height),
                                                                  isect_offsets, flatten_ids, order, work,
                                                                  render_mode == "RGB+ED", st)
        if rc == _lib.SC_EUNSUPPORTED:          # the reference-shaped raster kernel is selected: it reads the separate arrays
            conics = torch.empty((C, N, 3), dtype=torch.float32, device=dev)
            opac = torch.empty((C, N), dtype=torch.float32, device=dev)
            cols = torch.empty((C, N, 4), dtype=torch.float32, device=dev)
            _lib.check(lib.sc_records_unpack(_p(records), C * N, _p(conics), _p(opac), _p(cols), st), "sc_records_unpack")
            records = None
        elif rc:
            _lib.check(rc, "sc_rasterize_fwd_packed")
    if records is None:
        # the separate-array kernels write into one pair of buffers, through the ctypes table on either host route
        # (the depth-normalising sc_rasterize_fwd_ed has no entry in the binding layer)
        render_colors = torch.empty((C, height, width, 4), dtype=torch.float32, device=dev)
        render_alphas = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
        sch = (_p(order), _p(work))
        args = (_p(means2d), _p(conics), _p(cols), _p(opac), _p(backgrounds), None, C, N, 4, int(width), int(height),
                int(tile_size), tile_width, tile_height, _p(isect_offsets), _p(flatten_ids), flatten_ids.numel(),
                _p(render_colors), _p(render_alphas))
        if render_mode == "RGB+ED":
            rc = lib.sc_rasterize_fwd_ed(*args, *sch, st)
            if rc == _lib.SC_EUNSUPPORTED:          # the reference-shaped raster kernel is selected: plain launch + the torch post-step
                _lib.check(lib.sc_rasterize_fwd(*args, None, *sch, st), "sc_rasterize_fwd")
                render_colors = torch.cat([render_colors[..., :-1],
                                           render_colors[..., -1:] / render_alphas.clamp(min=1e-10)], dim=-1)
            else:
                _lib.check(rc, "sc_rasterize_fwd_ed")
        else:
            _lib.check(lib.sc_rasterize_fwd(*args, None, *sch, st), "sc_rasterize_fwd")
    meta = _FusedMeta({"radii": radii, "means2d": means2d, "depths": depths,
                       "tile_width": tile_width, "tile_height": tile_height, "tiles_per_gauss": tiles_per_gauss,
                       "flatten_ids": flatten_ids, "isect_offsets": isect_offsets,
                       "width": width, "height": height, "tile_size": tile_size, "n_cameras": C, "fused": True})
    if records is not None:          # conics / opacities / colors: rebuilt from the records on first access
        meta._sc_records = (records, (C, N), torch.cuda.current_stream(dev))
    else:
        meta.update({"conics": conics, "opacities": opac, "colors": cols})
    if isect_ids is not None:
        meta["isect_ids"] = isect_ids
    return render_colors, render_alphas, meta


def rasterization(means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Tensor,
                  viewmats: Tensor, Ks: Tensor, width: int, height: int, near_plane: float = 0.01,
                  far_plane: float = 1e10, radius_clip: float = 0.0, eps2d: float = 0.3,
                  sh_degree: Optional[int] = None, packed: bool = False, tile_size: int = 16,
                  backgrounds: Optional[Tensor] = None, render_mode: str = "RGB",
                  sparse_grad: bool = False, absgrad: bool = False, rasterize_mode: str = "classic",
                  channel_chunk: int = 32, distributed: bool = False, camera_model: str = "pinhole",
                  covars: Optional[Tensor] = None, camera_centers_: Optional[Tensor] = None):
    """gsplat's one-call API (imported at renderer.py:204).  means [N,3], quats [N,4], scales [N,3],
    opacities [N], colors [N,D] | [N,K,3] (with sh_degree), viewmats [C,4,4], Ks [C,3,3].  Returns
    (render_colors [C,H,W,*], render_alphas [C,H,W,1], meta).

    With `sh_degree` set, `render_mode` "RGB+D"/"RGB+ED" and no gradient required -- i.e. exactly what
    render_kernel_gsplat (renderer.py:186-302) spells out by hand: sh_degree=max_sh_degree,
    rasterize_mode="antialiased", render_mode="RGB+ED" -- the forward runs FUSED (see
    _rasterization_fused); results are bit-identical to the composition a1 -> a3 -> a4 -> a6 -> a9 below,
    which remains the path for training and for every other mode.  With set_fused_training(True) / SC_FUSED_TRAIN=1
    (off by default) the same call under grad runs its per-Gaussian part as one forward and one backward kernel
    (_rasterization_fused_train): same forward, gradients equal within rounding, `meta["fused"]` True.
    `camera_centers_` (not in gsplat): optional precomputed [C,3] camera positions, e.g. the reference's
    Camera.camera_center; by default they are derived from `viewmats` (rigid inverse).
    Cameras under grad (`viewmats.requires_grad`, or a `camera_centers_` that requires grad) take the composition and
    receive their gradients -- through the projection and, with derived or differentiable centres, through the SH
    directions; `Ks` gets none ("Camera gradients / pose optimisation")."""
    assert render_mode in ("RGB", "D", "ED", "RGB+D", "RGB+ED"), render_mode
    assert rasterize_mode in ("classic", "antialiased"), rasterize_mode
    if camera_model != "pinhole" or distributed or covars is not None:
        raise NotImplementedError("only pinhole, single-process, quats/scales input is supported")
    if packed:
        raise NotImplementedError("packed=True is not supported (reference passes packed=False)")
    C = viewmats.shape[0]
    N = means.shape[0]
    aa = rasterize_mode == "antialiased"
    if _fused_forward_ok((means, quats, scales, opacities, colors, viewmats, Ks, backgrounds), sh_degree,
                         render_mode, tile_size, colors):
        return _rasterization_fused(means, quats, scales, opacities, colors, viewmats, Ks, width, height,
                                    near_plane, far_plane, radius_clip, eps2d, sh_degree, tile_size,
                                    backgrounds, render_mode, aa, camera_centers_)
    if _fused_train_ok((means, quats, scales, opacities, colors), (viewmats, Ks, camera_centers_), sh_degree,
                       render_mode, tile_size, colors):
        return _rasterization_fused_train(means, quats, scales, opacities, colors, viewmats, Ks, width, height,
                                          near_plane, far_plane, radius_clip, eps2d, sh_degree, tile_size,
                                          backgrounds, render_mode, aa, camera_centers_, absgrad)
    radii, means2d, depths, conics, comps = fully_fused_projection(
        means, None, quats, scales, viewmats, Ks, width, height, eps2d=eps2d, near_plane=near_plane,
        far_plane=far_plane, radius_clip=radius_clip, calc_compensations=aa)
    opac = opacities.reshape(1, N).expand(C, N)
    if comps is not None:
        opac = opac * comps
    tile_width = math.ceil(width / float(tile_size))
    tile_height = math.ceil(height / float(tile_size))
    tiles_per_gauss, isect_ids, flatten_ids = isect_tiles(means2d, radii, depths, tile_size, tile_width,
                                                          tile_height, packed=False, n_cameras=C)
    isect_offsets = isect_offset_encode(isect_ids, C, tile_width, tile_height)
    if sh_degree is None:
        cols = colors.reshape(1, N, colors.shape[-1]).expand(C, N, -1) if colors.dim() == 2 else colors
    else:
        campos = camera_centers(viewmats) if camera_centers_ is None else camera_centers_.reshape(C, 3)
        dirs = means[None, :, :] - campos[:, None, :]
        shs = colors.reshape(1, N, colors.shape[-2], 3).expand(C, N, -1, 3)
        cols = spherical_harmonics(sh_degree, dirs, shs, masks=radii > 0)
        cols = torch.clamp_min(cols + 0.5, 0.0)
    if render_mode in ("RGB+D", "RGB+ED"):
        cols = torch.cat([cols, depths[..., None]], dim=-1)
        if backgrounds is not None:
            backgrounds = torch.cat([backgrounds, torch.zeros(C, 1, device=backgrounds.device)], dim=-1)
    elif render_mode in ("D", "ED"):
        cols = depths[..., None]
        if backgrounds is not None:
            backgrounds = torch.zeros(C, 1, device=backgrounds.device)
    render_colors, render_alphas = rasterize_to_pixels(means2d, conics, cols.contiguous(), opac.contiguous(),
                                                       width, height, tile_size, isect_offsets, flatten_ids,
                                                       backgrounds=backgrounds, packed=False, absgrad=absgrad)
    if render_mode in ("ED", "RGB+ED"):
        render_colors = torch.cat([render_colors[..., :-1],
                                   render_colors[..., -1:] / render_alphas.clamp(min=1e-10)], dim=-1)
    meta = {"radii": radii, "means2d": means2d, "depths": depths, "conics": conics, "opacities": opac,
            "tile_width": tile_width, "tile_height": tile_height, "tiles_per_gauss": tiles_per_gauss,
            "isect_ids": isect_ids, "flatten_ids": flatten_ids, "isect_offsets": isect_offsets,
            "width": width, "height": height, "tile_size": tile_size, "n_cameras": C, "colors": cols,
            "fused": False}
    return render_colors, render_alphas, meta
