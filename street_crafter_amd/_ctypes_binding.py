"""The ctypes route to the C ABI, behind the interface of the compiled binding layer (csrc/binding.cpp -> _sc_fast).

One function per host call of `_sc_fast`, with the same name, the same positional parameters and the same return tuple
(`rc` first; the same elements None under the same flags): each allocates its outputs and scratch with torch and calls
the entry point through the ctypes table of `_lib.py`.  `_lib.binding()` hands this module to the operators wherever the
compiled module is not in use (set_fast_binding(False), or a diagnostic / experiment build: the compiled module is linked
against the shipped library only), so an operator body is written once and does not know which of the two it holds.

Nothing is validated here (the operators' `_req` has done that) and no return code is turned into an exception: the
caller decides what `rc` means (SC_EUNSUPPORTED selects another kernel at several sites).  The three `*_autograd`
functions and `abi_version` exist in the compiled module only.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _ws(nbytes: int, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ---- a1 ---------------------------------------------------------------------------------------------------------
def projection_fwd(means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip,
                   calc_comp, stream):
    """-> (rc, radii, means2d, depths, conics, compensations | None)"""
    C, N = viewmats.shape[0], means.shape[0]
    dev = means.device
    radii = torch.empty((C, N), dtype=torch.int32, device=dev)
    means2d = torch.empty((C, N, 2), dtype=torch.float32, device=dev)
    depths = torch.empty((C, N), dtype=torch.float32, device=dev)
    conics = torch.empty((C, N, 3), dtype=torch.float32, device=dev)
    comps = torch.empty((C, N), dtype=torch.float32, device=dev) if calc_comp else None
    rc = _lib.load().sc_projection_fwd(_p(means), _p(quats), _p(scales), _p(viewmats), _p(Ks), C, N, int(width),
                                       int(height), float(eps2d), float(near_plane), float(far_plane),
                                       float(radius_clip), _p(radii), _p(means2d), _p(depths), _p(conics), _p(comps),
                                       stream)
    return rc, radii, means2d, depths, conics, comps


def projection_bwd(means, quats, scales, viewmats, Ks, width, height, eps2d, radii, conics, comps, v_means2d,
                   v_depths, v_conics, v_comps, stream):
    """-> (rc, v_means, v_quats, v_scales)"""
    C, N = viewmats.shape[0], means.shape[0]
    v_means = torch.empty_like(means)
    v_quats = torch.empty_like(quats)
    v_scales = torch.empty_like(scales)
    rc = _lib.load().sc_projection_bwd(_p(means), _p(quats), _p(scales), _p(viewmats), _p(Ks), C, N, width, height,
                                       eps2d, _p(radii), _p(conics), _p(comps), _p(v_means2d), _p(v_depths),
                                       _p(v_conics), _p(v_comps), _p(v_means), _p(v_quats), _p(v_scales), stream)
    return rc, v_means, v_quats, v_scales


# ---- a3 (tile-bucketed route) -------------------------------------------------------------------------------------
def isect_bin_count(means2d, radii, depths, tile_size, tile_width, tile_height, tile_work, viewmats, registry,
                    want_order, meta_host_ptr, seq, stream):
    """-> (rc, tiles_per_gauss, offsets, meta_dev, count_ws, tile_order | None)"""
    lib = _lib.load()
    C, N = radii.shape
    dev = means2d.device
    tiles_per_gauss = torch.empty((C, N), dtype=torch.int32, device=dev)
    offsets = torch.empty((C, tile_height, tile_width), dtype=torch.int32, device=dev)
    meta_dev = torch.empty(4, dtype=torch.int64, device=dev)
    ws0 = _ws(lib.sc_isect_bin_workspace_bytes(C * N, C, tile_width, tile_height, -1), dev)
    order = (torch.empty(lib.sc_tile_order_len(C * tile_width * tile_height), dtype=torch.int32, device=dev)
             if want_order else None)
    rc = lib.sc_isect_bin_count(_p(means2d), _p(radii), _p(depths), C, N, int(tile_size), int(tile_width),
                                int(tile_height), _p(tiles_per_gauss), _p(offsets), _p(meta_dev), meta_host_ptr, seq,
                                _p(ws0), ws0.numel(), _p(tile_work) if want_order else None, _p(viewmats),
                                _p(registry), _p(order), stream)
    return rc, tiles_per_gauss, offsets, meta_dev, ws0, order


def isect_bin_sort(means2d, radii, depths, tile_size, tile_width, tile_height, offsets, meta_dev, ws0, capacity,
                   rec_capacity, super_capacity, want_ids, stream):
    """-> (rc, isect_ids | None, flatten_ids)"""
    lib = _lib.load()
    C, N = radii.shape
    dev = means2d.device
    ids = torch.empty(capacity, dtype=torch.int64, device=dev) if want_ids else None
    fids = torch.empty(capacity, dtype=torch.int32, device=dev)
    ws = _ws(lib.sc_isect_bin_workspace_bytes(C * N, C, tile_width, tile_height, rec_capacity), dev)
    rc = lib.sc_isect_bin_sort(_p(means2d), _p(radii), _p(depths), C, N, int(tile_size), int(tile_width),
                               int(tile_height), _p(offsets), _p(meta_dev), _p(ws0), capacity, rec_capacity,
                               super_capacity, _p(ids), _p(fids), _p(ws), ws.numel(), stream)
    return rc, ids, fids


def wait_i64(addr, value, timeout_us):
    """-> 0 = the word at `addr` reached `value`, 1 = timed out (ctypes releases the GIL for the call)."""
    return _lib.load().sc_wait_i64(addr, value, timeout_us)


# ---- a6 ---------------------------------------------------------------------------------------------------------
def sh_fwd(degree, dirs, coeffs, masks, stream):
    """-> (rc, colors)"""
    M = dirs.numel() // 3
    K = coeffs.shape[-2]
    colors = torch.empty(dirs.shape, dtype=torch.float32, device=dirs.device)
    rc = _lib.load().sc_sh_fwd(int(degree), _p(dirs), _p(coeffs), _p(masks), M, K, _p(colors), stream)
    return rc, colors


def sh_bwd(degree, dirs, coeffs, masks, v_colors, need_dirs, stream):
    """-> (rc, v_coeffs, v_dirs | None)"""
    M = dirs.numel() // 3
    K = coeffs.shape[-2]
    v_coeffs = torch.empty_like(coeffs)
    v_dirs = torch.empty_like(dirs) if need_dirs else None
    rc = _lib.load().sc_sh_bwd(degree, _p(dirs), _p(coeffs), _p(masks), M, K, _p(v_colors), _p(v_coeffs), _p(v_dirs),
                               stream)
    return rc, v_coeffs, v_dirs


# ---- a9 / a11 -----------------------------------------------------------------------------------------------------
def rasterize_fwd(means2d, conics, colors, opacities, backgrounds, masks, width, height, tile_size, offsets,
                  flatten_ids, want_last, order, work, stream):
    """-> (rc, render_colors, render_alphas, last_ids | None)"""
    C, N = opacities.shape
    D = colors.shape[-1]
    th, tw = offsets.shape[1], offsets.shape[2]
    dev = means2d.device
    render_colors = torch.empty((C, height, width, D), dtype=torch.float32, device=dev)
    render_alphas = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
    last_ids = torch.empty((C, height, width), dtype=torch.int32, device=dev) if want_last else None
    rc = _lib.load().sc_rasterize_fwd(_p(means2d), _p(conics), _p(colors), _p(opacities), _p(backgrounds), _p(masks),
                                      C, N, D, int(width), int(height), int(tile_size), tw, th, _p(offsets),
                                      _p(flatten_ids), flatten_ids.numel(), _p(render_colors), _p(render_alphas),
                                      _p(last_ids), _p(order), _p(work), stream)
    return rc, render_colors, render_alphas, last_ids


def rasterize_fwd_planar(means2d, conics, colors, opacities, backgrounds, masks, width, height, tile_size, offsets,
                         flatten_ids, order, work, stream):
    """render_colors as planes [C][D][H][W], handed out as the permuted [C,H,W,D] view; rc == SC_EUNSUPPORTED: nothing
    was launched.  -> (rc, render_colors, render_alphas)"""
    C, N = opacities.shape
    D = colors.shape[-1]
    th, tw = offsets.shape[1], offsets.shape[2]
    dev = means2d.device
    planes = torch.empty((C, D, height, width), dtype=torch.float32, device=dev)
    render_alphas = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
    rc = _lib.load().sc_rasterize_fwd_planar(_p(means2d), _p(conics), _p(colors), _p(opacities), _p(backgrounds),
                                             _p(masks), C, N, D, int(width), int(height), int(tile_size), tw, th,
                                             _p(offsets), _p(flatten_ids), flatten_ids.numel(), _p(planes),
                                             _p(render_alphas), _p(order), _p(work), stream)
    return rc, planes.permute(0, 2, 3, 1), render_alphas


def rasterize_fwd_groups(means2d, conics, colors, opacities, group_ids, n_groups, width, height, tile_size, offsets,
                         flatten_ids, stream):
    """render_all in one pass: sc_group_extents, then sc_rasterize_fwd_groups on the extents it wrote.
    -> (rc, render_colors [C,H,W,D], render_alphas [C,H,W,1], group_colors [G,C,H,W,D], group_alphas [G,C,H,W,1],
    group_end i32 [C*tiles,G]); rc != 0: the first call that failed, nothing after it ran."""
    lib = _lib.load()
    C, N = opacities.shape
    D = colors.shape[-1]
    th, tw = offsets.shape[1], offsets.shape[2]
    G = max(int(n_groups), 0)
    dev = means2d.device
    render_colors = torch.empty((C, height, width, D), dtype=torch.float32, device=dev)
    render_alphas = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
    group_colors = torch.empty((G, C, height, width, D), dtype=torch.float32, device=dev)
    group_alphas = torch.empty((G, C, height, width, 1), dtype=torch.float32, device=dev)
    group_end = torch.empty((C * th * tw, G), dtype=torch.int32, device=dev)
    rc = lib.sc_group_extents(_p(offsets), _p(flatten_ids), flatten_ids.numel(), _p(group_ids), C, N, int(n_groups), tw,
                              th, _p(group_end), stream)
    if rc == 0:
        rc = lib.sc_rasterize_fwd_groups(_p(means2d), _p(conics), _p(colors), _p(opacities), _p(group_ids),
                                         _p(group_end), C, N, D, int(n_groups), int(width), int(height),
                                         int(tile_size), tw, th, _p(offsets), _p(flatten_ids), flatten_ids.numel(),
                                         _p(render_colors), _p(render_alphas), _p(group_colors), _p(group_alphas),
                                         stream)
    return rc, render_colors, render_alphas, group_colors, group_alphas, group_end


def rasterize_fwd_layers(means2d, conics, colors, opacities, n_front, width, height, tile_size, offsets, flatten_ids,
                         epilogue, rounding, want_layer_begin, out, stream):
    """render_novel_view's foreground and sky in one pass (sc_rasterize_fwd_layers); lb = layer_begin i32 [C*tiles] or None.
    epilogue 0 -> (rc, front_colors [C,H,W,D], front_alphas [C,H,W,1], back_colors [C,H,W,3], back_alphas [C,H,W,1], lb)
    epilogue 1 -> (rc, rgb [C,H,W,3], acc [C,H,W,1], depth [C,H,W,1] | None (D == 3), None, lb)
    epilogue 2 -> (rc, frame u8 [C,H,W,3] (`out` when given), None, None, None, lb)"""
    C, N = opacities.shape
    D = colors.shape[-1]
    th, tw = offsets.shape[1], offsets.shape[2]
    dev = means2d.device

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    o0 = o1 = o2 = o3 = None
    if epilogue == 0:
        o0, o1, o2, o3 = f32(C, height, width, D), f32(C, height, width, 1), f32(C, height, width, 3), f32(C, height, width, 1)
    elif epilogue == 1:
        o0, o1 = f32(C, height, width, 3), f32(C, height, width, 1)
        o2 = f32(C, height, width, 1) if D == 4 else None
    elif epilogue == 2:
        if out is not None:
            if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() != C * height * width * 3:
                raise RuntimeError("out must be a contiguous uint8 tensor of C*H*W*3 bytes on a HIP device")
            o0 = out
        else:
            o0 = torch.empty((C, height, width, 3), dtype=torch.uint8, device=dev)
    lb = torch.empty(C * th * tw, dtype=torch.int32, device=dev) if want_layer_begin else None
    u8_out = epilogue == 2
    rc = _lib.load().sc_rasterize_fwd_layers(_p(means2d), _p(conics), _p(colors), _p(opacities), C, N, D, int(n_front),
                                             int(width), int(height), int(tile_size), tw, th, _p(offsets),
                                             _p(flatten_ids), flatten_ids.numel(), int(epilogue), int(rounding),
                                             None if u8_out else _p(o0), _p(o1), _p(o2), _p(o3),
                                             _p(o0) if u8_out else None, _p(lb), stream)
    return rc, o0, o1, o2, o3, lb


def rasterize_fwd_groups_ids(means2d, conics, colors, opacities, group_ids, n_groups, width, height, tile_size, offsets,
                             flatten_ids, stream):
    """The training forward of the grouped rasterizer: sc_group_extents, then sc_rasterize_fwd_groups_ids.
    -> (rc, render_colors, render_alphas, group_colors, group_alphas, last_pos i32 [G+1,C,H,W]); images as
    rasterize_fwd_groups'."""
    lib = _lib.load()
    C, N = opacities.shape
    D = colors.shape[-1]
    th, tw = offsets.shape[1], offsets.shape[2]
    G = max(int(n_groups), 0)
    dev = means2d.device
    render_colors = torch.empty((C, height, width, D), dtype=torch.float32, device=dev)
    render_alphas = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
    group_colors = torch.empty((G, C, height, width, D), dtype=torch.float32, device=dev)
    group_alphas = torch.empty((G, C, height, width, 1), dtype=torch.float32, device=dev)
    last_pos = torch.empty((G + 1, C, height, width), dtype=torch.int32, device=dev)
    group_end = torch.empty((C * th * tw, G), dtype=torch.int32, device=dev)
    rc = lib.sc_group_extents(_p(offsets), _p(flatten_ids), flatten_ids.numel(), _p(group_ids), C, N, int(n_groups), tw,
                              th, _p(group_end), stream)
    if rc == 0:
        rc = lib.sc_rasterize_fwd_groups_ids(_p(means2d), _p(conics), _p(colors), _p(opacities), _p(group_ids),
                                             _p(group_end), C, N, D, int(n_groups), int(width), int(height),
                                             int(tile_size), tw, th, _p(offsets), _p(flatten_ids),
                                             flatten_ids.numel(), _p(render_colors), _p(render_alphas),
                                             _p(group_colors), _p(group_alphas), _p(last_pos), stream)
    return rc, render_colors, render_alphas, group_colors, group_alphas, last_pos


def rasterize_bwd_groups(means2d, conics, colors, opacities, group_ids, n_groups, width, height, tile_size, offsets,
                         flatten_ids, render_alphas, group_alphas, last_pos, v_render_colors, v_render_alphas,
                         v_group_colors, v_group_alphas, absgrad, stream):
    """The four upstream gradients are None where nobody differentiates the output (a null pointer: the set is off).
    -> (rc, v_means2d, v_conics, v_colors, v_opacities, v_means2d_abs | None)"""
    C, N = opacities.shape
    D = colors.shape[-1]
    th, tw = offsets.shape[1], offsets.shape[2]
    # the kernel accumulates with float atomics: ONE zero-fill for all five gradient buffers
    sizes = (2 * C * N, 3 * C * N, D * C * N, C * N, 2 * C * N if absgrad else 0)
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=means2d.device)
    parts = torch.split(flat, sizes)
    v_means2d = parts[0].view(C, N, 2)
    v_conics = parts[1].view(C, N, 3)
    v_colors = parts[2].view(C, N, D)
    v_opacities = parts[3].view(C, N)
    v_abs = parts[4].view(C, N, 2) if absgrad else None
    rc = _lib.load().sc_rasterize_bwd_groups(_p(means2d), _p(conics), _p(colors), _p(opacities), _p(group_ids), C, N, D,
                                             int(n_groups), int(width), int(height), int(tile_size), tw, th,
                                             _p(offsets), _p(flatten_ids), flatten_ids.numel(), _p(render_alphas),
                                             _p(group_alphas), _p(last_pos), _p(v_render_colors), _p(v_render_alphas),
                                             _p(v_group_colors), _p(v_group_alphas), _p(v_abs), _p(v_means2d),
                                             _p(v_conics), _p(v_colors), _p(v_opacities), stream)
    return rc, v_means2d, v_conics, v_colors, v_opacities, v_abs


def rasterize_bwd(means2d, conics, colors, opacities, backgrounds, masks, width, height, tile_size, offsets,
                  flatten_ids, render_alphas, last_ids, v_render_colors, v_render_alphas, absgrad, order, stream):
    """-> (rc, v_means2d, v_conics, v_colors, v_opacities, v_means2d_abs | None)"""
    C, N = opacities.shape
    D = colors.shape[-1]
    th, tw = offsets.shape[1], offsets.shape[2]
    # the kernel accumulates with float atomics: ONE zero-fill for all five gradient buffers
    sizes = (2 * C * N, 3 * C * N, D * C * N, C * N, 2 * C * N if absgrad else 0)
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=means2d.device)
    parts = torch.split(flat, sizes)
    v_means2d = parts[0].view(C, N, 2)
    v_conics = parts[1].view(C, N, 3)
    v_colors = parts[2].view(C, N, D)
    v_opacities = parts[3].view(C, N)
    v_abs = parts[4].view(C, N, 2) if absgrad else None
    rc = _lib.load().sc_rasterize_bwd(_p(means2d), _p(conics), _p(colors), _p(opacities), _p(backgrounds), _p(masks),
                                      C, N, D, width, height, tile_size, tw, th, _p(offsets), _p(flatten_ids),
                                      flatten_ids.numel(), _p(render_alphas), _p(last_ids), _p(v_render_colors),
                                      _p(v_render_alphas), _p(v_abs), _p(v_means2d), _p(v_conics), _p(v_colors),
                                      _p(v_opacities), _p(order), stream)
    return rc, v_means2d, v_conics, v_colors, v_opacities, v_abs


# ---- the fused per-Gaussian stage behind rasterization() --------------------------------------------------------------
def projection_sh_fwd(means, quats, scales, opacities, sh, viewmats, Ks, centers, sh_degree, width, height, eps2d,
                      near_plane, far_plane, radius_clip, antialiased, want_records, stream):
    """-> (rc, radii, means2d, depths, records | None, conics | None, opacities | None, colors4 | None): the packed
    records or the three separate arrays, never both."""
    C, N, K = viewmats.shape[0], means.shape[0], sh.shape[1]
    dev = means.device
    radii = torch.empty((C, N), dtype=torch.int32, device=dev)
    means2d = torch.empty((C, N, 2), dtype=torch.float32, device=dev)
    depths = torch.empty((C, N), dtype=torch.float32, device=dev)
    records = conics = opac = cols = None
    if want_records:
        records = torch.empty((C, N, 12), dtype=torch.float32, device=dev)
    else:
        conics = torch.empty((C, N, 3), dtype=torch.float32, device=dev)
        opac = torch.empty((C, N), dtype=torch.float32, device=dev)
        cols = torch.empty((C, N, 4), dtype=torch.float32, device=dev)
    rc = _lib.load().sc_projection_sh_fwd(_p(means), _p(quats), _p(scales), _p(opacities), _p(sh), _p(viewmats),
                                          _p(Ks), _p(centers), C, N, K, int(sh_degree), int(width), int(height),
                                          float(eps2d), float(near_plane), float(far_plane), float(radius_clip),
                                          int(antialiased), _p(radii), _p(means2d), _p(depths), _p(conics), _p(opac),
                                          _p(cols), _p(records), stream)
    return rc, radii, means2d, depths, records, conics, opac, cols


def projection_sh_bwd(means, quats, scales, opacities, sh, viewmats, Ks, centers, sh_degree, width, height, eps2d,
                      antialiased, radii, conics, v_means2d, v_depths, v_conics, v_opac, v_colors4, need_means,
                      need_quats, need_scales, need_opacities, need_sh, stream):
    """-> (rc, v_means | None, v_quats | None, v_scales | None, v_opacities | None, v_sh | None)"""
    C, N, K = viewmats.shape[0], means.shape[0], sh.shape[1]
    need = (need_means, need_quats, need_scales, need_opacities, need_sh)
    grads = [torch.empty_like(t) if n else None for t, n in zip((means, quats, scales, opacities, sh), need)]
    rc = _lib.load().sc_projection_sh_bwd(_p(means), _p(quats), _p(scales), _p(opacities), _p(sh), _p(viewmats),
                                          _p(Ks), _p(centers), C, N, K, sh_degree, width, height, eps2d,
                                          int(antialiased), _p(radii), _p(conics), _p(v_means2d), _p(v_depths),
                                          _p(v_conics), _p(v_opac), _p(v_colors4), *(_p(g) for g in grads), stream)
    return (rc, *grads)


def rasterize_fwd_packed(records, backgrounds, width, height, offsets, flatten_ids, order, work, depth_normalise,
                         stream):
    """-> (rc, render_colors [C,H,W,4], render_alphas [C,H,W,1])"""
    C, N = records.shape[0], records.shape[1]
    th, tw = offsets.shape[1], offsets.shape[2]
    dev = records.device
    render_colors = torch.empty((C, height, width, 4), dtype=torch.float32, device=dev)
    render_alphas = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
    rc = _lib.load().sc_rasterize_fwd_packed(_p(records), _p(backgrounds), None, C, N, int(width), int(height), tw, th,
                                             _p(offsets), _p(flatten_ids), flatten_ids.numel(), _p(render_colors),
                                             _p(render_alphas), _p(order), _p(work), int(depth_normalise), stream)
    return rc, render_colors, render_alphas


# ---- frame export -------------------------------------------------------------------------------------------------
# (images travel as addresses here: 0 = absent)
def frame_composite_u8(fg_ptr, fg_stride, acc_ptr, sky_ptr, sky_stride, n_pixels, rounding, out, stream):
    return _lib.load().sc_frame_composite_u8(fg_ptr, fg_stride, acc_ptr or None, sky_ptr or None, sky_stride,
                                             n_pixels, rounding, out.data_ptr(), stream)


def frame_composite_u8_strided(fg_ptr, fg_pix, fg_ch, acc_ptr, sky_ptr, sky_pix, sky_ch, n_pixels, rounding, out,
                               stream):
    return _lib.load().sc_frame_composite_u8_strided(fg_ptr, fg_pix, fg_ch, acc_ptr or None, sky_ptr or None,
                                                     sky_pix, sky_ch, n_pixels, rounding, out.data_ptr(), stream)


# ---- photometric loss ---------------------------------------------------------------------------------------------
def loss_fwd(img1, img2, mask, strides, B, C, H, W, mask_b, mask_h, mask_w, window, want_a1, want_a2, stream):
    """-> (rc, ssim [B+1], l1 [B], kept i64[B], a1 | None, a2 | None, b | None, c | None)"""
    lib = _lib.load()
    dev = img1.device
    s = torch.empty(B + 1, device=dev, dtype=torch.float32)
    l1 = torch.empty(B, device=dev, dtype=torch.float32)
    kept = torch.empty(B, device=dev, dtype=torch.int64)
    ws_bytes = lib.sc_loss_workspace_bytes(B, C, H, W)
    ws = torch.empty(max(ws_bytes, 8), device=dev, dtype=torch.uint8)
    a1 = a2 = bm = cm = None
    if want_a1 or want_a2:
        bm = torch.empty(B, C, H, W, device=dev, dtype=torch.float32)
        cm = torch.empty_like(bm)
        a1 = torch.empty_like(bm) if want_a1 else None
        a2 = torch.empty_like(bm) if want_a2 else None
    rc = lib.sc_loss_fwd(img1.data_ptr(), img2.data_ptr(), _p(mask), (ctypes.c_int64 * 11)(*strides), B, C, H, W,
                         mask_b, mask_h, mask_w, window, s.data_ptr(), l1.data_ptr(), kept.data_ptr(), _p(a1), _p(a2),
                         _p(bm), _p(cm), ws.data_ptr(), ws_bytes, stream)
    return rc, s, l1, kept, a1, a2, bm, cm


def loss_bwd(img1, img2, mask, strides, B, C, H, W, mask_b, mask_h, mask_w, window, a1, a2, bm, cm, g_ssim, g_l1,
             kept, need1, need2, stream):
    """-> (rc, grad1 | None, grad2 | None), contiguous [B,C,H,W]"""
    dev = img1.device
    g1 = torch.empty(B, C, H, W, device=dev, dtype=torch.float32) if need1 else None
    g2 = torch.empty(B, C, H, W, device=dev, dtype=torch.float32) if need2 else None
    rc = _lib.load().sc_loss_bwd(img1.data_ptr(), img2.data_ptr(), _p(mask), (ctypes.c_int64 * 11)(*strides), B, C, H,
                                 W, mask_b, mask_h, mask_w, window, _p(a1), _p(a2), _p(bm), _p(cm), _p(g_ssim),
                                 _p(g_l1), _p(kept), _p(g1), _p(g2), stream)
    return rc, g1, g2


# ---- regularizers -------------------------------------------------------------------------------------------------
def depth_trim_fwd(depth, lidar, mask, strides, H, W, keep, stream):
    """-> (rc, value 0-d, threshold 0-d, counts i64[3] = {n, k, below}, workspace u8): the backward reads the workspace."""
    lib = _lib.load()
    dev = depth.device
    value = torch.empty((), device=dev, dtype=torch.float32)
    thr = torch.empty((), device=dev, dtype=torch.float32)
    counts = torch.empty(3, device=dev, dtype=torch.int64)
    ws_bytes = lib.sc_depth_trim_workspace_bytes(H, W)
    ws = torch.empty(max(ws_bytes, 8), device=dev, dtype=torch.uint8)
    rc = lib.sc_depth_trim_fwd(depth.data_ptr(), lidar.data_ptr(), _p(mask), (ctypes.c_int64 * 6)(*strides), H, W,
                               float(keep), value.data_ptr(), thr.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                               ws_bytes, stream)
    return rc, value, thr, counts, ws


def depth_trim_bwd(depth, lidar, mask, strides, H, W, g, ws, need_depth, need_lidar, stream):
    """-> (rc, grad_depth | None, grad_lidar | None), contiguous [1,H,W]"""
    dev = depth.device
    gd = torch.empty(1, H, W, device=dev, dtype=torch.float32) if need_depth else None
    gl = torch.empty(1, H, W, device=dev, dtype=torch.float32) if need_lidar else None
    rc = _lib.load().sc_depth_trim_bwd(depth.data_ptr(), lidar.data_ptr(), _p(mask), (ctypes.c_int64 * 6)(*strides),
                                       H, W, g.data_ptr(), ws.data_ptr(), ws.numel(), _p(gd), _p(gl), stream)
    return rc, gd, gl


def acc_reg_fwd(acc, mask, strides, Cm, H, W, mode, stream):
    """-> (rc, value 0-d)"""
    lib = _lib.load()
    value = torch.empty((), device=acc.device, dtype=torch.float32)
    ws_bytes = lib.sc_acc_reg_workspace_bytes(H, W)
    ws = torch.empty(max(ws_bytes, 8), device=acc.device, dtype=torch.uint8)
    rc = lib.sc_acc_reg_fwd(acc.data_ptr(), mask.data_ptr(), (ctypes.c_int64 * 5)(*strides), Cm, H, W, mode,
                            value.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    return rc, value


def acc_reg_bwd(acc, mask, strides, Cm, H, W, mode, g, stream):
    """-> (rc, grad_acc), contiguous [1,H,W]"""
    ga = torch.empty(1, H, W, device=acc.device, dtype=torch.float32)
    rc = _lib.load().sc_acc_reg_bwd(acc.data_ptr(), mask.data_ptr(), (ctypes.c_int64 * 5)(*strides), Cm, H, W, mode,
                                    g.data_ptr(), ga.data_ptr(), stream)
    return rc, ga


# ---- frame tail -----------------------------------------------------------------------------------------------------
def frame_tail_fwd(colors, colors_planar, alphas, sky, sky_strides, affine, H, W, clamp, stream):
    """-> (rc, rgb [3,H,W], depth [1,H,W] | None (D == 3))"""
    D = colors.shape[-1]
    rgb = torch.empty(3, H, W, device=colors.device, dtype=torch.float32)
    depth = torch.empty(1, H, W, device=colors.device, dtype=torch.float32) if D == 4 else None
    rc = _lib.load().sc_frame_tail_fwd(colors.data_ptr(), D, int(colors_planar), alphas.data_ptr(), _p(sky),
                                       (ctypes.c_int64 * 3)(*sky_strides), _p(affine), H, W, int(clamp), rgb.data_ptr(),
                                       _p(depth), stream)
    return rc, rgb, depth


def frame_tail_bwd(colors, colors_planar, alphas, sky, sky_strides, affine, H, W, g, h, need_colors, need_alphas, need_sky,
                   sky_planar, need_affine, stream):
    """-> (rc, grad_colors [1,H,W,D] | None, grad_alphas [1,H,W,1] | None, grad_sky ([3,H,W] if sky_planar else
    [1,H,W,3]) | None, grad_affine [3,4] | None)"""
    lib = _lib.load()
    dev, D = colors.device, colors.shape[-1]
    gc = torch.empty(1, H, W, D, device=dev, dtype=torch.float32) if need_colors else None
    ga = torch.empty(1, H, W, 1, device=dev, dtype=torch.float32) if need_alphas else None
    gs = torch.empty((3, H, W) if sky_planar else (1, H, W, 3), device=dev, dtype=torch.float32) if need_sky else None
    gA = torch.empty(3, 4, device=dev, dtype=torch.float32) if need_affine else None
    ws_bytes = lib.sc_frame_tail_workspace_bytes(H, W) if need_affine else 0
    ws = torch.empty(max(ws_bytes, 8), device=dev, dtype=torch.uint8) if need_affine else None
    rc = lib.sc_frame_tail_bwd(colors.data_ptr(), D, int(colors_planar), alphas.data_ptr(), _p(sky),
                               (ctypes.c_int64 * 3)(*sky_strides), _p(affine), H, W, _p(g), _p(h), _p(gc), _p(ga), _p(gs), int(sky_planar), _p(gA), _p(ws),
                               ws_bytes, stream)
    return rc, gc, ga, gs, gA


# ---- sky cube map ---------------------------------------------------------------------------------------------------
def _ray_m(ray_m):
    return None if ray_m is None else (ctypes.c_float * 9)(*ray_m)


def cubemap_fwd(tex, dirs, ray_m, perturb, mask, acc, R, C, n, width, flags, fill, stream):
    """-> (rc, out): [C,n] with the planar flag (4), else [n,C]"""
    out = torch.empty((C, n) if flags & 4 else (n, C), device=tex.device, dtype=torch.float32)
    rc = _lib.load().sc_cubemap_fwd(tex.data_ptr(), R, C, _p(dirs), _ray_m(ray_m), _p(perturb), _p(mask), _p(acc), n,
                                    width, flags, float(fill), out.data_ptr(), stream)
    return rc, out


def cubemap_bwd(tex, dirs, ray_m, perturb, mask, acc, R, C, n, width, flags, fill, grad_out, stream):
    """-> (rc, grad_tex [6,R,R,C])"""
    gt = torch.empty(6, R, R, C, device=tex.device, dtype=torch.float32)
    rc = _lib.load().sc_cubemap_bwd(tex.data_ptr(), R, C, _p(dirs), _ray_m(ray_m), _p(perturb), _p(mask), _p(acc), n,
                                    width, flags, float(fill), grad_out.data_ptr(), gt.data_ptr(), stream)
    return rc, gt


# ---- perceptual loss ------------------------------------------------------------------------------------------------
def lpips_prep_fwd(img, mask, strides, H, W, mean, std, stream):
    """-> (rc, z [1,3,H,W])"""
    out = torch.empty((1, 3, H, W), device=img.device, dtype=torch.float32)
    rc = _lib.load().sc_lpips_prep_fwd(img.data_ptr(), _p(mask), (ctypes.c_int64 * 5)(*strides), H, W,
                                       (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), out.data_ptr(), stream)
    return rc, out


def lpips_prep_bwd(grad_out, mask, strides, H, W, std, stream):
    """-> (rc, grad_img [3,H,W])"""
    gi = torch.empty((3, H, W), device=grad_out.device, dtype=torch.float32)
    rc = _lib.load().sc_lpips_prep_bwd(grad_out.data_ptr(), _p(mask), (ctypes.c_int64 * 5)(*strides), H, W,
                                       (ctypes.c_float * 3)(*std), gi.data_ptr(), stream)
    return rc, gi


def _lpips_table(fx, fy, weight, channels, pixels, stride_x, stride_y):
    table = (_lib.LpipsTap * max(len(fx), 1))()
    for k in range(len(fx)):
        row = table[k]
        row.fx, row.fy, row.weight = fx[k].data_ptr(), fy[k].data_ptr(), weight[k].data_ptr()
        row.stride_x, row.stride_y, row.channels, row.pixels = stride_x[k], stride_y[k], channels[k], pixels[k]
    return table


def lpips_head_fwd(fx, fy, weight, channels, pixels, stride_x, stride_y, want_norms, stream):
    """-> (rc, out [n_taps + 1] = the taps' distances, then their sum, [norm_x [P]] | None, [norm_y [P]] | None)"""
    lib = _lib.load()
    n = len(fx)
    dev = fx[0].device
    table = _lpips_table(fx, fy, weight, channels, pixels, stride_x, stride_y)
    out = torch.empty(n + 1, device=dev, dtype=torch.float32)
    nx = ny = None
    if want_norms:
        nx = [torch.empty(pixels[k], device=dev, dtype=torch.float32) for k in range(n)]
        ny = [torch.empty(pixels[k], device=dev, dtype=torch.float32) for k in range(n)]
        for k in range(n):
            table[k].norm_x, table[k].norm_y = nx[k].data_ptr(), ny[k].data_ptr()
    ws_bytes = lib.sc_lpips_head_workspace_bytes(table, n)
    ws = torch.empty(max(ws_bytes // 8, 1), device=dev, dtype=torch.float64)
    rc = lib.sc_lpips_head_fwd(table, n, out.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    return rc, out, nx, ny


def lpips_head_bwd(fx, fy, weight, channels, pixels, stride_x, stride_y, norm_x, norm_y, grad, need_x, need_y, stream):
    """-> (rc, [grad_fx [C,P] | None], [grad_fy [C,P] | None])"""
    n = len(fx)
    dev = fx[0].device
    table = _lpips_table(fx, fy, weight, channels, pixels, stride_x, stride_y)
    gx, gy = [None] * n, [None] * n
    for k in range(n):
        table[k].norm_x, table[k].norm_y = norm_x[k].data_ptr(), norm_y[k].data_ptr()
        if need_x[k]:
            gx[k] = torch.empty((channels[k], pixels[k]), device=dev, dtype=torch.float32)
            table[k].grad_fx = gx[k].data_ptr()
        if need_y[k]:
            gy[k] = torch.empty((channels[k], pixels[k]), device=dev, dtype=torch.float32)
            table[k].grad_fy = gy[k].data_ptr()
    rc = _lib.load().sc_lpips_head_bwd(table, n, grad.data_ptr(), stream)
    return rc, gx, gy


# ---- crop + resize of the novel-view inputs -----------------------------------------------------------------------
def resize_fwd(x, strides, B, C, in_h, in_w, ty_idx, ty_w, tx_idx, tx_w, h_out, w_out, row_begin, flags, a, b, stream):
    """-> (rc, out [B,C,h_out - row_begin,w_out])"""
    out = torch.empty((B, C, max(h_out - row_begin, 0), w_out), device=x.device, dtype=torch.float32)
    rc = _lib.load().sc_resize_fwd(x.data_ptr(), (ctypes.c_int64 * 4)(*strides), B, C, in_h, in_w, ty_idx.data_ptr(),
                                   ty_w.data_ptr(), tx_idx.data_ptr(), tx_w.data_ptr(), h_out, w_out, row_begin, flags,
                                   float(a), float(b), out.data_ptr(), stream)
    return rc, out


def resize_mask_fwd(x, strides, B, C, in_h, in_w, ty_idx, tx_idx, h_out, w_out, row_begin, stream):
    """-> (rc, out bool [B,C,h_out - row_begin,w_out])"""
    out = torch.empty((B, C, max(h_out - row_begin, 0), w_out), device=x.device, dtype=torch.bool)
    rc = _lib.load().sc_resize_mask_fwd(x.data_ptr(), (ctypes.c_int64 * 4)(*strides), B, C, in_h, in_w, ty_idx.data_ptr(),
                                        tx_idx.data_ptr(), h_out, w_out, row_begin, out.data_ptr(), stream)
    return rc, out


def resize_bwd(grad_out, B, C, H, W, top, left, in_h, in_w, uy_idx, uy_w, ux_idx, ux_w, h_out, w_out, row_begin, flags, a,
               stream):
    """-> (rc, grad_x [B,C,H,W]): every element written"""
    gx = torch.empty((B, C, H, W), device=grad_out.device, dtype=torch.float32)
    rc = _lib.load().sc_resize_bwd(grad_out.data_ptr(), B, C, H, W, top, left, in_h, in_w, uy_idx.data_ptr(),
                                   uy_w.data_ptr(), ux_idx.data_ptr(), ux_w.data_ptr(), h_out, w_out, row_begin, flags,
                                   float(a), gx.data_ptr(), stream)
    return rc, gx


# ---- training tail ------------------------------------------------------------------------------------------------
def adam_step(params, grads, exp_avg, exp_avg_sq, step_size, bias2_sqrt, one_minus_beta1, beta2, one_minus_beta2,
              eps, stream):
    """-> rc"""
    table = (_lib.AdamTensor * len(params))()
    for row, p, g, m, v, s, b in zip(table, params, grads, exp_avg, exp_avg_sq, step_size, bias2_sqrt):
        row.param, row.grad, row.exp_avg, row.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        row.numel, row.step_size, row.bias2_sqrt = p.numel(), s, b
    return _lib.load().sc_adam_step(table, len(params), one_minus_beta1, beta2, one_minus_beta2, eps, stream)


def densify_stats(grad, absgrad, radii, visible, N, half_width, half_height, ranges, grad_accum, denom, max_radii,
                  stream):
    """segments: (start, end) pairs in `ranges` (2 per segment) with their accumulators; empty ones are left out of the
    table (an empty tensor has no data pointer to hand over).  -> rc"""
    live = [k for k in range(len(grad_accum)) if ranges[2 * k + 1] > ranges[2 * k]]
    table = (_lib.StatsSegment * max(len(live), 1))()
    for row, k in zip(table, live):
        row.start, row.end = ranges[2 * k], ranges[2 * k + 1]
        row.grad_accum, row.denom, row.max_radii = grad_accum[k].data_ptr(), denom[k].data_ptr(), max_radii[k].data_ptr()
    return _lib.load().sc_densify_stats(grad.data_ptr(), _p(absgrad), radii.data_ptr(),
                                        int(radii.dtype == torch.float32), visible.data_ptr(), N, half_width,
                                        half_height, table, len(live), stream)


# ---- the head of a frame --------------------------------------------------------------------------------------------
def _compose_table(xyz, scaling, rotation, opacity, features_dc, features_rest, flips, ranges, kinds, pose_rows, fparams):
    table = (_lib.ComposeSegment * len(xyz))()
    for k, row in enumerate(table):
        row.start, row.end = ranges[2 * k], ranges[2 * k + 1]
        row.xyz, row.scaling, row.rotation, row.opacity = _p(xyz[k]), _p(scaling[k]), _p(rotation[k]), _p(opacity[k])
        row.features_dc, row.features_rest = _p(features_dc[k]), _p(features_rest[k])
        row.flip = _p(flips[k]) if flips[k].numel() else None
        row.kind, row.pose_row, row.fourier_dim = kinds[k], pose_rows[k], features_dc[k].shape[1]
        row.basis = (ctypes.c_float * 8)(*fparams[12 * k:12 * k + 8])
        row.centre = (ctypes.c_float * 3)(*fparams[12 * k + 8:12 * k + 11])
        row.radius = fparams[12 * k + 11]
    return table


def compose_fwd(xyz, scaling, rotation, opacity, features_dc, features_rest, flips, ranges, kinds, pose_rows, fparams,
                N, K, obj_rots, obj_trans, A, flip_q, stream):
    """ranges: (start, end) pairs; flips: uint8 [n], numel 0 = no mask; fparams: 12 per segment (basis[8], centre[3],
    radius).  -> (rc, means [N,3], quats [N,4], scales [N,3], opacities [N,1], sh [N,K,3])"""
    table = _compose_table(xyz, scaling, rotation, opacity, features_dc, features_rest, flips, ranges, kinds, pose_rows,
                           fparams)
    dev = xyz[0].device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    means, quats, scales, opac, sh = new(N, 3), new(N, 4), new(N, 3), new(N, 1), new(N, K, 3)
    fq = (ctypes.c_float * 4)(*flip_q) if len(flip_q) else None
    rc = _lib.load().sc_compose_fwd(table, len(xyz), N, K, _p(obj_rots), _p(obj_trans), A, fq, _p(means), _p(quats),
                                    _p(scales), _p(opac), _p(sh), stream)
    return rc, means, quats, scales, opac, sh


def compose_bwd(xyz, scaling, rotation, opacity, features_dc, features_rest, flips, ranges, kinds, pose_rows, fparams,
                N, K, obj_rots, obj_trans, A, flip_q, g_means, g_quats, g_scales, g_opacities, g_sh, want_rots,
                want_trans, stream):
    """-> (rc, [g_xyz], [g_scaling], [g_rotation], [g_opacity], [g_features_dc], [g_features_rest],
    grad_obj_rots | None, grad_obj_trans | None): every gradient written in full"""
    table = _compose_table(xyz, scaling, rotation, opacity, features_dc, features_rest, flips, ranges, kinds, pose_rows,
                           fparams)
    lists = [[torch.empty_like(t) for t in src] for src in (xyz, scaling, rotation, opacity, features_dc, features_rest)]
    grads = (_lib.ComposeGrads * len(xyz))()
    for k, row in enumerate(grads):
        row.xyz, row.scaling, row.rotation, row.opacity, row.features_dc, row.features_rest = \
            (_p(lst[k]) for lst in lists)
    dev = xyz[0].device
    grots = torch.empty((A, 4), dtype=torch.float32, device=dev) if want_rots else None
    gtrans = torch.empty((A, 3), dtype=torch.float32, device=dev) if want_trans else None
    fq = (ctypes.c_float * 4)(*flip_q) if len(flip_q) else None
    rc = _lib.load().sc_compose_bwd(table, grads, len(xyz), N, K, _p(obj_rots), _p(obj_trans), A, fq, _p(g_means),
                                    _p(g_quats), _p(g_scales), _p(g_opacities), _p(g_sh), _p(grots), _p(gtrans), stream)
    return (rc, *lists, grots, gtrans)


# ---- densify and prune ----------------------------------------------------------------------------------------------
def densify_plan(xyz, scaling, rotation, opacity, grad_accum, denom, max_radii, split_noise, box_noise, fparams,
                 iparams, stream):
    """fparams: 11 per job (max_grad, dense_size, min_opacity, big_size, max_screen_size, region_a[3], region_b[3]);
    iparams: 3 per job (grad_col, prune_big, region).
    -> (rc, counters i32[J,8], [src_row i32[2n]], [slot u8[2n]], [child_xyz [2,n,3]], [child_scaling [2,n,3]])"""
    lib = _lib.load()
    J = len(xyz)
    dev = xyz[0].device
    counters = torch.zeros((J, 8), dtype=torch.int32, device=dev)
    src_row, slot, child_xyz, child_scaling = [], [], [], []
    table = (_lib.DensifyJob * J)()
    for k, row in enumerate(table):
        n = xyz[k].shape[0]
        src_row.append(torch.empty(2 * n, dtype=torch.int32, device=dev))
        slot.append(torch.empty(2 * n, dtype=torch.uint8, device=dev))
        child_xyz.append(torch.empty((2, n, 3), dtype=torch.float32, device=dev))
        child_scaling.append(torch.empty((2, n, 3), dtype=torch.float32, device=dev))
        row.n = n
        row.xyz, row.scaling, row.rotation, row.opacity = _p(xyz[k]), _p(scaling[k]), _p(rotation[k]), _p(opacity[k])
        row.grad_accum, row.denom, row.max_radii = _p(grad_accum[k]), _p(denom[k]), _p(max_radii[k])
        row.split_noise, row.box_noise = _p(split_noise[k]), _p(box_noise[k])
        row.src_row, row.slot = _p(src_row[k]), _p(slot[k])
        row.child_xyz, row.child_scaling = _p(child_xyz[k]), _p(child_scaling[k])
        row.counters = counters.data_ptr() + 32 * k
        f = fparams[11 * k:11 * k + 11]
        row.max_grad, row.dense_size, row.min_opacity, row.big_size, row.max_screen_size = f[:5]
        row.region_a, row.region_b = (ctypes.c_float * 3)(*f[5:8]), (ctypes.c_float * 3)(*f[8:11])
        row.grad_col, row.prune_big, row.region = (int(v) for v in iparams[3 * k:3 * k + 3])
    ws_bytes = lib.sc_densify_plan_workspace_bytes(table, J)
    ws = _ws(ws_bytes, dev)
    rc = lib.sc_densify_plan(table, J, ws.data_ptr(), ws_bytes, stream)
    return rc, counters, src_row, slot, child_xyz, child_scaling


def densify_apply(src_param, src_exp_avg, src_exp_avg_sq, child, src_row, slot, n, n_out, width, stream):
    """one entry per parameter group; moments and child None where absent
    -> (rc, [dst_param [n_out,width]], [dst_exp_avg | None], [dst_exp_avg_sq | None])"""
    G = len(src_param)
    dst_param, dst_m, dst_v = [], [], []
    table = (_lib.DensifyGroup * max(G, 1))()
    for k in range(G):
        row = table[k]
        shape = (n_out[k], width[k])
        dst_param.append(torch.empty(shape, dtype=torch.float32, device=src_param[k].device))
        has = src_exp_avg[k] is not None
        dst_m.append(torch.empty_like(dst_param[k]) if has else None)
        dst_v.append(torch.empty_like(dst_param[k]) if has else None)
        row.src_param, row.dst_param = _p(src_param[k]), _p(dst_param[k])
        if has and n_out[k] * width[k] > 0:      # (an empty tensor may have no data pointer; such a group moves nothing)
            row.src_exp_avg, row.src_exp_avg_sq = _p(src_exp_avg[k]), _p(src_exp_avg_sq[k])
            row.dst_exp_avg, row.dst_exp_avg_sq = _p(dst_m[k]), _p(dst_v[k])
        row.child = _p(child[k])
        row.src_row, row.slot = _p(src_row[k]), _p(slot[k])
        row.n, row.n_out, row.width = n[k], n_out[k], width[k]
    rc = _lib.load().sc_densify_apply(table, G, stream)
    return rc, dst_param, dst_m, dst_v
