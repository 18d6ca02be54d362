// Host-side binding layer: Python <-> the C ABI of include/street_crafter_amd.h, compiled (g++, no device code).
//
// WHY.  The operators keep the reference's Python signatures (gsplat.rendering.*, called one by one from
// street_gaussian/models/street_gaussian_renderer.py:219-280), so every frame crosses Python -> native five times.
// Through ctypes a crossing costs ~6-8 us of argument conversion, and every output / workspace tensor a separate
// ~3-4 us torch.empty from Python: ~150 us of host time per frame (tools/exp_host.py), which is what bounds small
// scenes (S-100k: 0.24-0.30 ms per frame, all of it host) and makes the training step's rate depend on how busy the
// box's host is (BENCH_r02: 786 steps/s on the driver's box, 1060 on a quiet one, for 0.78 ms of kernels).
// Here one call per operator validates its tensors, allocates ALL of its outputs and scratch through torch's
// caching allocator (at::empty: stream-ordered reuse, no hipMalloc) and calls the SAME C-ABI entry point.  Nothing
// else moves: the C ABI stays the boundary, kernels and results are untouched, autograd wiring stays in
// rendering.py.  torch is used for what it is here for: device memory.
//
// The library's entry points are resolved at link time (libstreet_crafter_hip.so, rpath $ORIGIN).  Streams arrive as
// the raw hipStream_t value (torch._C._cuda_getCurrentRawStream), so no HIP header is needed.
#include <torch/extension.h>

#include <algorithm>
#include <cstdint>
#include <tuple>
#include <vector>

#include "../../include/street_crafter_amd.h"

#ifndef SC_ABI_HASH
#define SC_ABI_HASH "unhashed"
#endif

namespace {

using at::Tensor;
using OptT = c10::optional<Tensor>;

inline sc_stream_t S(int64_t s) { return reinterpret_cast<sc_stream_t>(static_cast<uintptr_t>(s)); }

inline void req(const Tensor& t, at::ScalarType dt, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must live on a HIP device (got ", t.device(), "); street_crafter_amd has no CPU path");
    TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
inline const float* fp(const Tensor& t) { return static_cast<const float*>(t.data_ptr()); }
inline float* fpw(const Tensor& t) { return static_cast<float*>(t.data_ptr()); }
inline const float* fpo(const OptT& t) { return t.has_value() ? static_cast<const float*>(t->data_ptr()) : nullptr; }
inline const int32_t* ip(const Tensor& t) { return static_cast<const int32_t*>(t.data_ptr()); }
inline at::TensorOptions f32(const Tensor& like) { return like.options().dtype(at::kFloat); }
inline at::TensorOptions i32(const Tensor& like) { return like.options().dtype(at::kInt); }
inline at::TensorOptions u8(const Tensor& like) { return like.options().dtype(at::kByte); }

// ---- a1 ---------------------------------------------------------------------------------------------------
// -> (rc, radii, means2d, depths, conics, compensations | None)
struct ProjOutT { int rc; Tensor radii, means2d, depths, conics; OptT comps; };
ProjOutT projection_fwd_c(const Tensor& means, const Tensor& quats, const Tensor& scales, const Tensor& viewmats,
                          const Tensor& Ks, int64_t width, int64_t height, double eps2d, double near_plane,
                          double far_plane, double radius_clip, bool calc_comp, int64_t stream) {
    req(means, at::kFloat, "means"); req(quats, at::kFloat, "quats"); req(scales, at::kFloat, "scales");
    req(viewmats, at::kFloat, "viewmats"); req(Ks, at::kFloat, "Ks");
    const int64_t C = viewmats.size(0), N = means.size(0);
    Tensor radii = at::empty({C, N}, i32(means));
    Tensor means2d = at::empty({C, N, 2}, f32(means));
    Tensor depths = at::empty({C, N}, f32(means));
    Tensor conics = at::empty({C, N, 3}, f32(means));
    OptT comps;
    if (calc_comp) comps = at::empty({C, N}, f32(means));
    const int rc = sc_projection_fwd(fp(means), fp(quats), fp(scales), fp(viewmats), fp(Ks), (int)C, (int)N, (int)width,
                                     (int)height, (float)eps2d, (float)near_plane, (float)far_plane, (float)radius_clip,
                                     static_cast<int32_t*>(radii.data_ptr()), fpw(means2d), fpw(depths), fpw(conics),
                                     comps ? fpw(*comps) : nullptr, S(stream));
    return {rc, radii, means2d, depths, conics, comps};
}
py::tuple projection_fwd(const Tensor& means, const Tensor& quats, const Tensor& scales, const Tensor& viewmats,
                         const Tensor& Ks, int64_t width, int64_t height, double eps2d, double near_plane,
                         double far_plane, double radius_clip, bool calc_comp, int64_t stream) {
    ProjOutT o = projection_fwd_c(means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane,
                                  radius_clip, calc_comp, stream);
    return py::make_tuple(o.rc, o.radii, o.means2d, o.depths, o.conics, o.comps);
}

// -> (rc, v_means, v_quats, v_scales)
struct ProjBwdT { int rc; Tensor v_means, v_quats, v_scales; };
ProjBwdT projection_bwd_c(const Tensor& means, const Tensor& quats, const Tensor& scales, const Tensor& viewmats,
                          const Tensor& Ks, int64_t width, int64_t height, double eps2d, const Tensor& radii,
                          const Tensor& conics, const OptT& comps, const Tensor& v_means2d, const Tensor& v_depths,
                          const Tensor& v_conics, const OptT& v_comps, int64_t stream) {
    req(v_means2d, at::kFloat, "v_means2d"); req(v_depths, at::kFloat, "v_depths"); req(v_conics, at::kFloat, "v_conics");
    if (v_comps) req(*v_comps, at::kFloat, "v_compensations");
    const int64_t C = viewmats.size(0), N = means.size(0);
    Tensor v_means = at::empty_like(means), v_quats = at::empty_like(quats), v_scales = at::empty_like(scales);
    const int rc = sc_projection_bwd(fp(means), fp(quats), fp(scales), fp(viewmats), fp(Ks), (int)C, (int)N, (int)width,
                                     (int)height, (float)eps2d, ip(radii), fp(conics), fpo(comps), fp(v_means2d),
                                     fp(v_depths), fp(v_conics), fpo(v_comps), fpw(v_means), fpw(v_quats),
                                     fpw(v_scales), S(stream));
    return {rc, v_means, v_quats, v_scales};
}
py::tuple projection_bwd(const Tensor& means, const Tensor& quats, const Tensor& scales, const Tensor& viewmats,
                         const Tensor& Ks, int64_t width, int64_t height, double eps2d, const Tensor& radii,
                         const Tensor& conics, const OptT& comps, const Tensor& v_means2d, const Tensor& v_depths,
                         const Tensor& v_conics, const OptT& v_comps, int64_t stream) {
    ProjBwdT o = projection_bwd_c(means, quats, scales, viewmats, Ks, width, height, eps2d, radii, conics, comps, v_means2d,
                                  v_depths, v_conics, v_comps, stream);
    return py::make_tuple(o.rc, o.v_means, o.v_quats, o.v_scales);
}

// ---- a3 (tile-bucketed route) -------------------------------------------------------------------------------
// count phase: allocates tiles_per_gauss, isect_offsets, meta_dev, the count workspace and (want_order) the dispatch
// list.  -> (rc, tiles_per_gauss, offsets, meta_dev, count_ws, tile_order | None)
py::tuple isect_bin_count(const Tensor& means2d, const Tensor& radii, const Tensor& depths, int64_t tile_size,
                          int64_t tile_width, int64_t tile_height, const OptT& tile_work, const OptT& viewmats,
                          const OptT& registry, bool want_order, int64_t meta_host_ptr, int64_t seq, int64_t stream) {
    req(means2d, at::kFloat, "means2d"); req(radii, at::kInt, "radii"); req(depths, at::kFloat, "depths");
    const int64_t C = radii.size(0), N = radii.size(1);
    Tensor tpg = at::empty({C, N}, i32(means2d));
    Tensor offsets = at::empty({C, tile_height, tile_width}, i32(means2d));
    Tensor meta_dev = at::empty({4}, means2d.options().dtype(at::kLong));
    size_t wsb = sc_isect_bin_workspace_bytes(C * N, (int)C, (int)tile_width, (int)tile_height, -1);
    if (wsb < 256) wsb = 256;
    Tensor ws0 = at::empty({(int64_t)wsb}, u8(means2d));
    OptT order;
    if (want_order) order = at::empty({(int64_t)sc_tile_order_len((int)(C * tile_width * tile_height))}, i32(means2d));
    const int rc = sc_isect_bin_count(
        fp(means2d), ip(radii), fp(depths), (int)C, (int)N, (int)tile_size, (int)tile_width, (int)tile_height,
        static_cast<int32_t*>(tpg.data_ptr()), static_cast<int32_t*>(offsets.data_ptr()),
        static_cast<int64_t*>(meta_dev.data_ptr()), reinterpret_cast<int64_t*>(static_cast<uintptr_t>(meta_host_ptr)), seq,
        ws0.data_ptr(), wsb, (want_order && tile_work) ? ip(*tile_work) : nullptr, viewmats ? fp(*viewmats) : nullptr,
        registry ? static_cast<int32_t*>(registry->data_ptr()) : nullptr,
        order ? static_cast<int32_t*>(order->data_ptr()) : nullptr, S(stream));
    return py::make_tuple(rc, tpg, offsets, meta_dev, ws0, order);
}

// sort phase: allocates flatten_ids (+ isect_ids when want_ids) for `capacity` elements and the sort workspace (freed
// on return: the caching allocator reuses a block only for LATER work of the same stream).
// -> (rc, isect_ids | None, flatten_ids)
py::tuple isect_bin_sort(const Tensor& means2d, const Tensor& radii, const Tensor& depths, int64_t tile_size,
                         int64_t tile_width, int64_t tile_height, const Tensor& offsets, const Tensor& meta_dev,
                         const Tensor& ws0, int64_t capacity, int64_t rec_capacity, int64_t super_capacity, bool want_ids,
                         int64_t stream) {
    const int64_t C = radii.size(0), N = radii.size(1);
    OptT ids;
    if (want_ids) ids = at::empty({capacity}, means2d.options().dtype(at::kLong));
    Tensor fids = at::empty({capacity}, i32(means2d));
    size_t wsb = sc_isect_bin_workspace_bytes(C * N, (int)C, (int)tile_width, (int)tile_height, rec_capacity);
    if (wsb < 256) wsb = 256;
    Tensor ws = at::empty({(int64_t)wsb}, u8(means2d));
    const int rc = sc_isect_bin_sort(fp(means2d), ip(radii), fp(depths), (int)C, (int)N, (int)tile_size, (int)tile_width,
                                     (int)tile_height, ip(offsets), static_cast<const int64_t*>(meta_dev.data_ptr()),
                                     ws0.data_ptr(), capacity, rec_capacity, super_capacity,
                                     ids ? static_cast<int64_t*>(ids->data_ptr()) : nullptr,
                                     static_cast<int32_t*>(fids.data_ptr()), ws.data_ptr(), wsb, S(stream));
    return py::make_tuple(rc, ids, fids);
}

// host-side wait for the counts (the GIL is released: another host thread keeps launching)
int wait_i64(int64_t addr, int64_t value, int64_t timeout_us) {
    py::gil_scoped_release nogil;
    return sc_wait_i64(reinterpret_cast<const int64_t*>(static_cast<uintptr_t>(addr)), value, timeout_us);
}

// ---- a6 ---------------------------------------------------------------------------------------------------
struct ShFwdT { int rc; Tensor colors; };
ShFwdT sh_fwd_c(int64_t degree, const Tensor& dirs, const Tensor& coeffs, const OptT& masks, int64_t stream) {
    req(dirs, at::kFloat, "dirs"); req(coeffs, at::kFloat, "coeffs");
    if (masks) req(*masks, at::kByte, "masks");
    const int64_t M = dirs.numel() / 3, K = coeffs.size(-2);
    Tensor colors = at::empty(dirs.sizes(), f32(dirs));
    const int rc = sc_sh_fwd((int)degree, fp(dirs), fp(coeffs), masks ? static_cast<const uint8_t*>(masks->data_ptr()) : nullptr,
                             M, (int)K, fpw(colors), S(stream));
    return {rc, colors};
}
py::tuple sh_fwd(int64_t degree, const Tensor& dirs, const Tensor& coeffs, const OptT& masks, int64_t stream) {
    ShFwdT o = sh_fwd_c(degree, dirs, coeffs, masks, stream);
    return py::make_tuple(o.rc, o.colors);
}

struct ShBwdT { int rc; Tensor v_coeffs; OptT v_dirs; };
ShBwdT sh_bwd_c(int64_t degree, const Tensor& dirs, const Tensor& coeffs, const OptT& masks, const Tensor& v_colors,
                bool need_dirs, int64_t stream) {
    req(v_colors, at::kFloat, "v_colors");
    const int64_t M = dirs.numel() / 3, K = coeffs.size(-2);
    Tensor v_coeffs = at::empty_like(coeffs);
    OptT v_dirs;
    if (need_dirs) v_dirs = at::empty_like(dirs);
    const int rc = sc_sh_bwd((int)degree, fp(dirs), fp(coeffs), masks ? static_cast<const uint8_t*>(masks->data_ptr()) : nullptr,
                             M, (int)K, fp(v_colors), fpw(v_coeffs), v_dirs ? fpw(*v_dirs) : nullptr, S(stream));
    return {rc, v_coeffs, v_dirs};
}
py::tuple sh_bwd(int64_t degree, const Tensor& dirs, const Tensor& coeffs, const OptT& masks, const Tensor& v_colors,
                 bool need_dirs, int64_t stream) {
    ShBwdT o = sh_bwd_c(degree, dirs, coeffs, masks, v_colors, need_dirs, stream);
    return py::make_tuple(o.rc, o.v_coeffs, o.v_dirs);
}

// ---- a9 / a11 ------------------------------------------------------------------------------------------------
// -> (rc, render_colors, render_alphas, last_ids | None)
struct RasterFwdT { int rc; Tensor colors, alphas; OptT last; };
RasterFwdT rasterize_fwd_c(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                           const OptT& backgrounds, const OptT& masks, int64_t width, int64_t height, int64_t tile_size,
                           const Tensor& offsets, const Tensor& flatten_ids, bool want_last, const OptT& order,
                           const OptT& work, int64_t stream) {
    req(means2d, at::kFloat, "means2d"); req(conics, at::kFloat, "conics"); req(colors, at::kFloat, "colors");
    req(opacities, at::kFloat, "opacities"); req(offsets, at::kInt, "isect_offsets"); req(flatten_ids, at::kInt, "flatten_ids");
    const int64_t C = opacities.size(0), N = opacities.size(1), D = colors.size(-1);
    const int64_t th = offsets.size(1), tw = offsets.size(2);
    Tensor rc_ = at::empty({C, height, width, D}, f32(means2d));
    Tensor ra = at::empty({C, height, width, 1}, f32(means2d));
    OptT last;
    if (want_last) last = at::empty({C, height, width}, i32(means2d));
    const int rc = sc_rasterize_fwd(fp(means2d), fp(conics), fp(colors), fp(opacities), fpo(backgrounds),
                                    masks ? static_cast<const uint8_t*>(masks->data_ptr()) : nullptr, (int)C, (int)N, (int)D,
                                    (int)width, (int)height, (int)tile_size, (int)tw, (int)th, ip(offsets), ip(flatten_ids),
                                    flatten_ids.numel(), fpw(rc_), fpw(ra),
                                    last ? static_cast<int32_t*>(last->data_ptr()) : nullptr,
                                    order ? ip(*order) : nullptr, work ? static_cast<int32_t*>(work->data_ptr()) : nullptr,
                                    S(stream));
    return {rc, rc_, ra, last};
}
// render_colors as planes [C][D][H][W], handed out as the permuted [C,H,W,D] view (sc_rasterize_fwd_planar; inference only).
// rc == SC_EUNSUPPORTED: nothing was launched, the caller takes rasterize_fwd.
py::tuple rasterize_fwd_planar(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                               const OptT& backgrounds, const OptT& masks, int64_t width, int64_t height, int64_t tile_size,
                               const Tensor& offsets, const Tensor& flatten_ids, const OptT& order, const OptT& work,
                               int64_t stream) {
    req(means2d, at::kFloat, "means2d"); req(conics, at::kFloat, "conics"); req(colors, at::kFloat, "colors");
    req(opacities, at::kFloat, "opacities"); req(offsets, at::kInt, "isect_offsets"); req(flatten_ids, at::kInt, "flatten_ids");
    const int64_t C = opacities.size(0), N = opacities.size(1), D = colors.size(-1);
    const int64_t th = offsets.size(1), tw = offsets.size(2);
    Tensor planes = at::empty({C, D, height, width}, f32(means2d));
    Tensor ra = at::empty({C, height, width, 1}, f32(means2d));
    const int rc = sc_rasterize_fwd_planar(fp(means2d), fp(conics), fp(colors), fp(opacities), fpo(backgrounds),
                                           masks ? static_cast<const uint8_t*>(masks->data_ptr()) : nullptr, (int)C, (int)N,
                                           (int)D, (int)width, (int)height, (int)tile_size, (int)tw, (int)th, ip(offsets),
                                           ip(flatten_ids), flatten_ids.numel(), fpw(planes), fpw(ra),
                                           order ? ip(*order) : nullptr,
                                           work ? static_cast<int32_t*>(work->data_ptr()) : nullptr, S(stream));
    return py::make_tuple(rc, planes.permute({0, 2, 3, 1}), ra);
}
// render_all in one pass (sc_group_extents, then sc_rasterize_fwd_groups on the extents it wrote): the composite and one
// image per group.  -> (rc, render_colors [C,H,W,D], render_alphas [C,H,W,1], group_colors [G,C,H,W,D],
// group_alphas [G,C,H,W,1], group_end i32 [C*tiles,G]); rc != 0: the first call that failed, nothing after it ran.
py::tuple rasterize_fwd_groups(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                               const Tensor& group_ids, int64_t n_groups, int64_t width, int64_t height, int64_t tile_size,
                               const Tensor& offsets, const Tensor& flatten_ids, int64_t stream) {
    req(means2d, at::kFloat, "means2d"); req(conics, at::kFloat, "conics"); req(colors, at::kFloat, "colors");
    req(opacities, at::kFloat, "opacities"); req(offsets, at::kInt, "isect_offsets"); req(flatten_ids, at::kInt, "flatten_ids");
    req(group_ids, at::kByte, "group_ids");
    const int64_t C = opacities.size(0), N = opacities.size(1), D = colors.size(-1);
    const int64_t th = offsets.size(1), tw = offsets.size(2), G = std::max<int64_t>(n_groups, 0);
    Tensor rc_ = at::empty({C, height, width, D}, f32(means2d));
    Tensor ra = at::empty({C, height, width, 1}, f32(means2d));
    Tensor gc = at::empty({G, C, height, width, D}, f32(means2d));
    Tensor ga = at::empty({G, C, height, width, 1}, f32(means2d));
    Tensor ge = at::empty({C * th * tw, G}, i32(means2d));
    const uint8_t* gid = static_cast<const uint8_t*>(group_ids.data_ptr());
    int rc = sc_group_extents(ip(offsets), ip(flatten_ids), flatten_ids.numel(), gid, (int)C, (int)N, (int)n_groups, (int)tw,
                              (int)th, static_cast<int32_t*>(ge.data_ptr()), S(stream));
    if (rc == 0)
        rc = sc_rasterize_fwd_groups(fp(means2d), fp(conics), fp(colors), fp(opacities), gid, ip(ge), (int)C, (int)N, (int)D,
                                     (int)n_groups, (int)width, (int)height, (int)tile_size, (int)tw, (int)th, ip(offsets),
                                     ip(flatten_ids), flatten_ids.numel(), fpw(rc_), fpw(ra), fpw(gc), fpw(ga), S(stream));
    return py::make_tuple(rc, rc_, ra, gc, ga, ge);
}
// render_novel_view's foreground and sky in one pass (sc_rasterize_fwd_layers): rows [0, n_front) are the front layer,
// the rest the back layer; the lists come from isect_tiles on layered depth keys (street_crafter_amd/layers.py).
// epilogue 0 -> (rc, front_colors [C,H,W,D], front_alphas [C,H,W,1], back_colors [C,H,W,3], back_alphas [C,H,W,1], lb)
// epilogue 1 -> (rc, rgb [C,H,W,3], acc [C,H,W,1], depth [C,H,W,1] | None (D == 3), None, lb)
// epilogue 2 -> (rc, frame u8 [C,H,W,3] (`out` when given), None, None, None, lb)
// lb: layer_begin i32 [C*tiles] when want_layer_begin, else None.
py::tuple rasterize_fwd_layers(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                               int64_t n_front, int64_t width, int64_t height, int64_t tile_size, const Tensor& offsets,
                               const Tensor& flatten_ids, int64_t epilogue, int64_t rounding, bool want_layer_begin,
                               const OptT& out, int64_t stream) {
    req(means2d, at::kFloat, "means2d"); req(conics, at::kFloat, "conics"); req(colors, at::kFloat, "colors");
    req(opacities, at::kFloat, "opacities"); req(offsets, at::kInt, "isect_offsets"); req(flatten_ids, at::kInt, "flatten_ids");
    const int64_t C = opacities.size(0), N = opacities.size(1), D = colors.size(-1);
    const int64_t th = offsets.size(1), tw = offsets.size(2);
    OptT o0, o1, o2, o3, lb;
    if (epilogue == 0) {
        o0 = at::empty({C, height, width, D}, f32(means2d));
        o1 = at::empty({C, height, width, 1}, f32(means2d));
        o2 = at::empty({C, height, width, 3}, f32(means2d));
        o3 = at::empty({C, height, width, 1}, f32(means2d));
    } else if (epilogue == 1) {
        o0 = at::empty({C, height, width, 3}, f32(means2d));
        o1 = at::empty({C, height, width, 1}, f32(means2d));
        if (D == 4) o2 = at::empty({C, height, width, 1}, f32(means2d));
    } else if (epilogue == 2) {
        if (out) {
            req(*out, at::kByte, "out");
            TORCH_CHECK(out->numel() == C * height * width * 3, "out must hold C*H*W*3 bytes");
            o0 = *out;
        } else {
            o0 = at::empty({C, height, width, 3}, u8(means2d));
        }
    }
    if (want_layer_begin) lb = at::empty({C * th * tw}, i32(means2d));
    auto w = [](const OptT& t) { return t ? static_cast<float*>(t->data_ptr()) : nullptr; };
    const bool u8_out = epilogue == 2;
    const int rc = sc_rasterize_fwd_layers(
        fp(means2d), fp(conics), fp(colors), fp(opacities), (int)C, (int)N, (int)D, (int)n_front, (int)width, (int)height,
        (int)tile_size, (int)tw, (int)th, ip(offsets), ip(flatten_ids), flatten_ids.numel(), (int)epilogue, (int)rounding,
        u8_out ? nullptr : w(o0), w(o1), w(o2), w(o3), (u8_out && o0) ? static_cast<uint8_t*>(o0->data_ptr()) : nullptr,
        lb ? static_cast<int32_t*>(lb->data_ptr()) : nullptr, S(stream));
    return py::make_tuple(rc, o0, o1, o2, o3, lb);
}
// the training forward of the grouped rasterizer (sc_group_extents, then sc_rasterize_fwd_groups_ids): the same images
// plus, per pixel and accumulator set, where the set stopped.  -> (rc, render_colors, render_alphas, group_colors,
// group_alphas, last_pos i32 [G+1,C,H,W])
py::tuple rasterize_fwd_groups_ids(const Tensor& means2d, const Tensor& conics, const Tensor& colors,
                                   const Tensor& opacities, const Tensor& group_ids, int64_t n_groups, int64_t width,
                                   int64_t height, int64_t tile_size, const Tensor& offsets, const Tensor& flatten_ids,
                                   int64_t stream) {
    req(means2d, at::kFloat, "means2d"); req(conics, at::kFloat, "conics"); req(colors, at::kFloat, "colors");
    req(opacities, at::kFloat, "opacities"); req(offsets, at::kInt, "isect_offsets"); req(flatten_ids, at::kInt, "flatten_ids");
    req(group_ids, at::kByte, "group_ids");
    const int64_t C = opacities.size(0), N = opacities.size(1), D = colors.size(-1);
    const int64_t th = offsets.size(1), tw = offsets.size(2), G = std::max<int64_t>(n_groups, 0);
    Tensor rc_ = at::empty({C, height, width, D}, f32(means2d));
    Tensor ra = at::empty({C, height, width, 1}, f32(means2d));
    Tensor gc = at::empty({G, C, height, width, D}, f32(means2d));
    Tensor ga = at::empty({G, C, height, width, 1}, f32(means2d));
    Tensor lp = at::empty({G + 1, C, height, width}, i32(means2d));
    Tensor ge = at::empty({C * th * tw, G}, i32(means2d));
    const uint8_t* gid = static_cast<const uint8_t*>(group_ids.data_ptr());
    int rc = sc_group_extents(ip(offsets), ip(flatten_ids), flatten_ids.numel(), gid, (int)C, (int)N, (int)n_groups, (int)tw,
                              (int)th, static_cast<int32_t*>(ge.data_ptr()), S(stream));
    if (rc == 0)
        rc = sc_rasterize_fwd_groups_ids(fp(means2d), fp(conics), fp(colors), fp(opacities), gid, ip(ge), (int)C, (int)N,
                                         (int)D, (int)n_groups, (int)width, (int)height, (int)tile_size, (int)tw, (int)th,
                                         ip(offsets), ip(flatten_ids), flatten_ids.numel(), fpw(rc_), fpw(ra), fpw(gc),
                                         fpw(ga), static_cast<int32_t*>(lp.data_ptr()), S(stream));
    return py::make_tuple(rc, rc_, ra, gc, ga, lp);
}
// its backward: ONE zero-filled buffer for the gradient outputs; an upstream gradient nobody asked for arrives as None
// and travels as a null pointer.  -> (rc, v_means2d, v_conics, v_colors, v_opacities, v_means2d_abs | None)
py::tuple rasterize_bwd_groups(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                               const Tensor& group_ids, int64_t n_groups, int64_t width, int64_t height, int64_t tile_size,
                               const Tensor& offsets, const Tensor& flatten_ids, const Tensor& render_alphas,
                               const Tensor& group_alphas, const Tensor& last_pos, const OptT& v_render_colors,
                               const OptT& v_render_alphas, const OptT& v_group_colors, const OptT& v_group_alphas,
                               bool absgrad, int64_t stream) {
    req(means2d, at::kFloat, "means2d"); req(conics, at::kFloat, "conics"); req(colors, at::kFloat, "colors");
    req(opacities, at::kFloat, "opacities"); req(offsets, at::kInt, "isect_offsets"); req(flatten_ids, at::kInt, "flatten_ids");
    req(group_ids, at::kByte, "group_ids"); req(render_alphas, at::kFloat, "render_alphas");
    req(group_alphas, at::kFloat, "group_alphas"); req(last_pos, at::kInt, "last_pos");
    if (v_render_colors) req(*v_render_colors, at::kFloat, "v_render_colors");
    if (v_render_alphas) req(*v_render_alphas, at::kFloat, "v_render_alphas");
    if (v_group_colors) req(*v_group_colors, at::kFloat, "v_group_colors");
    if (v_group_alphas) req(*v_group_alphas, at::kFloat, "v_group_alphas");
    const int64_t C = opacities.size(0), N = opacities.size(1), D = colors.size(-1), CN = C * N;
    const int64_t th = offsets.size(1), tw = offsets.size(2);
    const int64_t sizes[5] = {2 * CN, 3 * CN, D * CN, CN, absgrad ? 2 * CN : 0};
    Tensor flat = at::zeros({sizes[0] + sizes[1] + sizes[2] + sizes[3] + sizes[4]}, f32(means2d));
    int64_t o = 0;
    Tensor v_m = flat.narrow(0, o, sizes[0]).view({C, N, 2}); o += sizes[0];
    Tensor v_c = flat.narrow(0, o, sizes[1]).view({C, N, 3}); o += sizes[1];
    Tensor v_col = flat.narrow(0, o, sizes[2]).view({C, N, D}); o += sizes[2];
    Tensor v_o = flat.narrow(0, o, sizes[3]).view({C, N}); o += sizes[3];
    OptT v_abs;
    if (absgrad) v_abs = flat.narrow(0, o, sizes[4]).view({C, N, 2});
    const int rc = sc_rasterize_bwd_groups(
        fp(means2d), fp(conics), fp(colors), fp(opacities), static_cast<const uint8_t*>(group_ids.data_ptr()), (int)C, (int)N,
        (int)D, (int)n_groups, (int)width, (int)height, (int)tile_size, (int)tw, (int)th, ip(offsets), ip(flatten_ids),
        flatten_ids.numel(), fp(render_alphas), fp(group_alphas), ip(last_pos), fpo(v_render_colors), fpo(v_render_alphas),
        fpo(v_group_colors), fpo(v_group_alphas), v_abs ? fpw(*v_abs) : nullptr, fpw(v_m), fpw(v_c), fpw(v_col), fpw(v_o),
        S(stream));
    return py::make_tuple(rc, v_m, v_c, v_col, v_o, v_abs);
}
py::tuple rasterize_fwd(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                        const OptT& backgrounds, const OptT& masks, int64_t width, int64_t height, int64_t tile_size,
                        const Tensor& offsets, const Tensor& flatten_ids, bool want_last, const OptT& order,
                        const OptT& work, int64_t stream) {
    RasterFwdT o = rasterize_fwd_c(means2d, conics, colors, opacities, backgrounds, masks, width, height, tile_size, offsets,
                                   flatten_ids, want_last, order, work, stream);
    return py::make_tuple(o.rc, o.colors, o.alphas, o.last);
}

// ONE zero-filled buffer for the five gradient outputs (the kernel accumulates with float atomics).
// -> (rc, v_means2d, v_conics, v_colors, v_opacities, v_means2d_abs | None)
struct RasterBwdT { int rc; Tensor v_m, v_c, v_col, v_o; OptT v_abs; };
RasterBwdT rasterize_bwd_c(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                           const OptT& backgrounds, const OptT& masks, int64_t width, int64_t height, int64_t tile_size,
                           const Tensor& offsets, const Tensor& flatten_ids, const Tensor& render_alphas, const Tensor& last_ids,
                           const Tensor& v_render_colors, const Tensor& v_render_alphas, bool absgrad, const OptT& order,
                           int64_t stream) {
    req(v_render_colors, at::kFloat, "v_render_colors"); req(v_render_alphas, at::kFloat, "v_render_alphas");
    req(last_ids, at::kInt, "last_ids");
    const int64_t C = opacities.size(0), N = opacities.size(1), D = colors.size(-1), CN = C * N;
    const int64_t th = offsets.size(1), tw = offsets.size(2);
    const int64_t sizes[5] = {2 * CN, 3 * CN, D * CN, CN, absgrad ? 2 * CN : 0};
    Tensor flat = at::zeros({sizes[0] + sizes[1] + sizes[2] + sizes[3] + sizes[4]}, f32(means2d));
    int64_t o = 0;
    Tensor v_m = flat.narrow(0, o, sizes[0]).view({C, N, 2}); o += sizes[0];
    Tensor v_c = flat.narrow(0, o, sizes[1]).view({C, N, 3}); o += sizes[1];
    Tensor v_col = flat.narrow(0, o, sizes[2]).view({C, N, D}); o += sizes[2];
    Tensor v_o = flat.narrow(0, o, sizes[3]).view({C, N}); o += sizes[3];
    OptT v_abs;
    if (absgrad) v_abs = flat.narrow(0, o, sizes[4]).view({C, N, 2});
    const int rc = sc_rasterize_bwd(fp(means2d), fp(conics), fp(colors), fp(opacities), fpo(backgrounds),
                                    masks ? static_cast<const uint8_t*>(masks->data_ptr()) : nullptr, (int)C, (int)N, (int)D,
                                    (int)width, (int)height, (int)tile_size, (int)tw, (int)th, ip(offsets), ip(flatten_ids),
                                    flatten_ids.numel(), fp(render_alphas), ip(last_ids), fp(v_render_colors),
                                    fp(v_render_alphas), v_abs ? fpw(*v_abs) : nullptr, fpw(v_m), fpw(v_c), fpw(v_col),
                                    fpw(v_o), order ? ip(*order) : nullptr, S(stream));
    return {rc, v_m, v_c, v_col, v_o, v_abs};
}
py::tuple rasterize_bwd(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                        const OptT& backgrounds, const OptT& masks, int64_t width, int64_t height, int64_t tile_size,
                        const Tensor& offsets, const Tensor& flatten_ids, const Tensor& render_alphas, const Tensor& last_ids,
                        const Tensor& v_render_colors, const Tensor& v_render_alphas, bool absgrad, const OptT& order,
                        int64_t stream) {
    RasterBwdT o = rasterize_bwd_c(means2d, conics, colors, opacities, backgrounds, masks, width, height, tile_size, offsets,
                                   flatten_ids, render_alphas, last_ids, v_render_colors, v_render_alphas, absgrad, order, stream);
    return py::make_tuple(o.rc, o.v_m, o.v_c, o.v_col, o.v_o, o.v_abs);
}

// ---- the fused forward behind gsplat.rendering.rasterization() --------------------------------------
// -> (rc, radii, means2d, depths, records | None, conics | None, opacities | None, colors4 | None)
py::tuple projection_sh_fwd(const Tensor& means, const Tensor& quats, const Tensor& scales, const Tensor& opacities,
                            const Tensor& sh, const Tensor& viewmats, const Tensor& Ks, const Tensor& centers,
                            int64_t sh_degree, int64_t width, int64_t height, double eps2d, double near_plane,
                            double far_plane, double radius_clip, bool antialiased, bool want_records, int64_t stream) {
    req(means, at::kFloat, "means"); req(quats, at::kFloat, "quats"); req(scales, at::kFloat, "scales");
    req(opacities, at::kFloat, "opacities"); req(sh, at::kFloat, "colors"); req(viewmats, at::kFloat, "viewmats");
    req(Ks, at::kFloat, "Ks"); req(centers, at::kFloat, "camera_centers");
    const int64_t C = viewmats.size(0), N = means.size(0), K = sh.size(1);
    Tensor radii = at::empty({C, N}, i32(means));
    Tensor means2d = at::empty({C, N, 2}, f32(means));
    Tensor depths = at::empty({C, N}, f32(means));
    OptT records, conics, opac, cols;
    if (want_records) {
        records = at::empty({C, N, 12}, f32(means));
    } else {
        conics = at::empty({C, N, 3}, f32(means));
        opac = at::empty({C, N}, f32(means));
        cols = at::empty({C, N, 4}, f32(means));
    }
    const int rc = sc_projection_sh_fwd(fp(means), fp(quats), fp(scales), fp(opacities), fp(sh), fp(viewmats), fp(Ks),
                                        fp(centers), (int)C, (int)N, (int)K, (int)sh_degree, (int)width, (int)height,
                                        (float)eps2d, (float)near_plane, (float)far_plane, (float)radius_clip,
                                        antialiased ? 1 : 0, static_cast<int32_t*>(radii.data_ptr()), fpw(means2d),
                                        fpw(depths), conics ? fpw(*conics) : nullptr, opac ? fpw(*opac) : nullptr,
                                        cols ? fpw(*cols) : nullptr, records ? fpw(*records) : nullptr, S(stream));
    return py::make_tuple(rc, radii, means2d, depths, records, conics, opac, cols);
}

// The backward of the above for training through rasterization(): allocates the gradients asked for (need_*) and
// calls the one kernel.  -> (rc, v_means | None, v_quats | None, v_scales | None, v_opacities | None, v_sh | None)
py::tuple projection_sh_bwd(const Tensor& means, const Tensor& quats, const Tensor& scales, const Tensor& opacities,
                            const Tensor& sh, const Tensor& viewmats, const Tensor& Ks, const Tensor& centers,
                            int64_t sh_degree, int64_t width, int64_t height, double eps2d, bool antialiased,
                            const Tensor& radii, const Tensor& conics, const Tensor& v_means2d, const OptT& v_depths,
                            const Tensor& v_conics, const Tensor& v_opac, const Tensor& v_colors4, bool need_means,
                            bool need_quats, bool need_scales, bool need_opacities, bool need_sh, int64_t stream) {
    req(v_means2d, at::kFloat, "v_means2d"); req(v_conics, at::kFloat, "v_conics");
    req(v_opac, at::kFloat, "v_opacities"); req(v_colors4, at::kFloat, "v_colors");
    if (v_depths) req(*v_depths, at::kFloat, "v_depths");
    const int64_t C = viewmats.size(0), N = means.size(0), K = sh.size(1);
    TORCH_CHECK(v_means2d.numel() == C * N * 2 && v_conics.numel() == C * N * 3 && v_opac.numel() == C * N &&
                v_colors4.numel() == C * N * 4 && (!v_depths || v_depths->numel() == C * N),
                "projection_sh_bwd: upstream gradients do not match [C, N]");
    OptT v_means, v_quats, v_scales, v_opacities, v_sh;
    if (need_means) v_means = at::empty_like(means);
    if (need_quats) v_quats = at::empty_like(quats);
    if (need_scales) v_scales = at::empty_like(scales);
    if (need_opacities) v_opacities = at::empty_like(opacities);
    if (need_sh) v_sh = at::empty_like(sh);
    const int rc = sc_projection_sh_bwd(fp(means), fp(quats), fp(scales), fp(opacities), fp(sh), fp(viewmats), fp(Ks),
                                        fp(centers), (int)C, (int)N, (int)K, (int)sh_degree, (int)width, (int)height,
                                        (float)eps2d, antialiased ? 1 : 0, ip(radii), fp(conics), fp(v_means2d),
                                        fpo(v_depths), fp(v_conics), fp(v_opac), fp(v_colors4),
                                        v_means ? fpw(*v_means) : nullptr, v_quats ? fpw(*v_quats) : nullptr,
                                        v_scales ? fpw(*v_scales) : nullptr, v_opacities ? fpw(*v_opacities) : nullptr,
                                        v_sh ? fpw(*v_sh) : nullptr, S(stream));
    return py::make_tuple(rc, v_means, v_quats, v_scales, v_opacities, v_sh);
}

// -> (rc, render_colors [C,H,W,4], render_alphas [C,H,W,1])
py::tuple rasterize_fwd_packed(const Tensor& records, const OptT& backgrounds, int64_t width, int64_t height,
                               const Tensor& offsets, const Tensor& flatten_ids, const OptT& order, const OptT& work,
                               bool depth_normalise, int64_t stream) {
    req(records, at::kFloat, "records"); req(offsets, at::kInt, "isect_offsets"); req(flatten_ids, at::kInt, "flatten_ids");
    const int64_t C = records.size(0), N = records.size(1);
    const int64_t th = offsets.size(1), tw = offsets.size(2);
    Tensor rc_ = at::empty({C, height, width, 4}, f32(records));
    Tensor ra = at::empty({C, height, width, 1}, f32(records));
    const int rc = sc_rasterize_fwd_packed(fp(records), fpo(backgrounds), nullptr, (int)C, (int)N, (int)width, (int)height,
                                           (int)tw, (int)th, ip(offsets), ip(flatten_ids), flatten_ids.numel(), fpw(rc_),
                                           fpw(ra), order ? ip(*order) : nullptr,
                                           work ? static_cast<int32_t*>(work->data_ptr()) : nullptr,
                                           depth_normalise ? 1 : 0, S(stream));
    return py::make_tuple(rc, rc_, ra);
}

// ---- the three differentiable operators as C++ autograd functions ------------------------------------------------
// The training step (train.py:236) is bound by HOST time on a busy box (BENCH_r02: 786 steps/s on the driver's box, 1060 on a
// quiet one, same kernels): per step torch.autograd.Function.apply costs ~15 us of Python per operator on the way forward
// and a Python call from the autograd engine's thread (GIL, argument wrapping) per operator on the way back.  Here forward
// and backward are the C++ cores above: no Python frame, and in the backward the GIL is taken only to ask torch for the
// current raw stream (the engine runs a backward on its forward's stream) and for gsplat's `.absgrad` contract (one
// attribute assignment on the caller's tensor object).  The Python autograd.Functions of rendering.py stay: they are the
// ctypes path's, the A/B (`rendering.set_native_autograd(False)`), and what runs while a backward probe is set.
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

struct PyRef : torch::CustomClassHolder {      // a Python object kept alive by an autograd node
    PyObject* p;
    explicit PyRef(PyObject* o) : p(o) { Py_XINCREF(p); }
    ~PyRef() override {
        if (p && Py_IsInitialized()) { py::gil_scoped_acquire g; Py_DECREF(p); }
    }
};
inline c10::IValue keep(const py::object& o) { return c10::IValue::make_capsule(c10::make_intrusive<PyRef>(o.ptr())); }
inline PyObject* kept(const c10::IValue& v) { return c10::static_intrusive_pointer_cast<PyRef>(v.toCapsule())->p; }
// torch._C._cuda_getCurrentRawStream(device index), asked under the GIL
inline int64_t raw_stream_of(const c10::IValue& stream_fn, const Tensor& like) {
    py::gil_scoped_acquire g;
    return py::reinterpret_borrow<py::object>(kept(stream_fn))((int)like.get_device()).cast<int64_t>();
}
inline void check_rc(int rc, const char* what) {
    TORCH_CHECK(rc == 0, what, " failed: ", sc_error_string(rc), " (code ", rc, ")");
}
inline Tensor or_empty(const OptT& t, const Tensor& like) { return t.has_value() ? *t : at::empty({0}, f32(like)); }

struct ProjectionFn : public torch::autograd::Function<ProjectionFn> {
    static variable_list forward(AutogradContext* ctx, const Tensor& means, const Tensor& quats, const Tensor& scales,
                                 const Tensor& viewmats, const Tensor& Ks, int64_t width, int64_t height, double eps2d,
                                 double near_plane, double far_plane, double radius_clip, bool calc_comp,
                                 py::object stream_fn) {
        const c10::IValue sf = keep(stream_fn);
        ProjOutT o = projection_fwd_c(means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane,
                                      radius_clip, calc_comp, raw_stream_of(sf, means));
        check_rc(o.rc, "sc_projection_fwd");
        ctx->save_for_backward({means, quats, scales, viewmats, Ks, o.radii, o.conics, or_empty(o.comps, means)});
        ctx->saved_data["w"] = width; ctx->saved_data["h"] = height; ctx->saved_data["eps"] = eps2d;
        ctx->saved_data["comp"] = calc_comp; ctx->saved_data["sf"] = sf;
        ctx->mark_non_differentiable({o.radii});
        if (calc_comp) return {o.radii, o.means2d, o.depths, o.conics, *o.comps};
        return {o.radii, o.means2d, o.depths, o.conics};
    }
    static variable_list backward(AutogradContext* ctx, variable_list g) {
        const auto sv = ctx->get_saved_variables();
        const Tensor &means = sv[0], &quats = sv[1], &scales = sv[2], &viewmats = sv[3], &Ks = sv[4];
        const bool has_comp = ctx->saved_data["comp"].toBool();
        const int64_t C = viewmats.size(0), N = means.size(0);
        auto z = [&](const Tensor& t, at::IntArrayRef shape) {
            return t.defined() ? t.contiguous() : at::zeros(shape, f32(means));
        };
        const Tensor v_m2 = z(g[1], {C, N, 2}), v_d = z(g[2], {C, N}), v_c = z(g[3], {C, N, 3});
        OptT v_comp, comps;
        if (has_comp) { v_comp = z(g.size() > 4 ? g[4] : Tensor(), {C, N}); comps = sv[7]; }
        ProjBwdT o = projection_bwd_c(means, quats, scales, viewmats, Ks, ctx->saved_data["w"].toInt(),
                                      ctx->saved_data["h"].toInt(), ctx->saved_data["eps"].toDouble(), sv[5], sv[6], comps,
                                      v_m2, v_d, v_c, v_comp, raw_stream_of(ctx->saved_data["sf"], means));
        check_rc(o.rc, "sc_projection_bwd");
        return {ctx->needs_input_grad(0) ? o.v_means : Tensor(), ctx->needs_input_grad(1) ? o.v_quats : Tensor(),
                ctx->needs_input_grad(2) ? o.v_scales : Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(),
                Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

struct ShFn : public torch::autograd::Function<ShFn> {
    static Tensor forward(AutogradContext* ctx, int64_t degree, const Tensor& dirs, const Tensor& coeffs, const OptT& masks,
                          py::object stream_fn) {
        const c10::IValue sf = keep(stream_fn);
        ShFwdT o = sh_fwd_c(degree, dirs, coeffs, masks, raw_stream_of(sf, dirs));
        check_rc(o.rc, "sc_sh_fwd");
        ctx->save_for_backward({dirs, coeffs, or_empty(masks, dirs)});
        ctx->saved_data["deg"] = degree; ctx->saved_data["mask"] = masks.has_value(); ctx->saved_data["sf"] = sf;
        return o.colors;
    }
    static variable_list backward(AutogradContext* ctx, variable_list g) {
        const auto sv = ctx->get_saved_variables();
        OptT masks;
        if (ctx->saved_data["mask"].toBool()) masks = sv[2];
        const Tensor v_colors = g[0].defined() ? g[0].contiguous() : at::zeros_like(sv[0]);
        // (needs_input_grad counts the TENSOR inputs of forward: dirs 0, coeffs 1)
        ShBwdT o = sh_bwd_c(ctx->saved_data["deg"].toInt(), sv[0], sv[1], masks, v_colors, ctx->needs_input_grad(0),
                            raw_stream_of(ctx->saved_data["sf"], sv[0]));
        check_rc(o.rc, "sc_sh_bwd");
        return {Tensor(), o.v_dirs.has_value() ? *o.v_dirs : Tensor(), ctx->needs_input_grad(1) ? o.v_coeffs : Tensor(),
                Tensor(), Tensor()};
    }
};

struct RasterFn : public torch::autograd::Function<RasterFn> {
    static variable_list forward(AutogradContext* ctx, const Tensor& means2d, const Tensor& conics, const Tensor& colors,
                                 const Tensor& opacities, const OptT& backgrounds, const OptT& masks, int64_t width,
                                 int64_t height, int64_t tile_size, const Tensor& offsets, const Tensor& flatten_ids,
                                 bool absgrad, const OptT& order, const OptT& work, py::object absgrad_target,
                                 py::object stream_fn) {
        const c10::IValue sf = keep(stream_fn);
        const bool needs_bwd = means2d.requires_grad() || conics.requires_grad() || colors.requires_grad() ||
                               opacities.requires_grad() || (backgrounds.has_value() && backgrounds->requires_grad());
        RasterFwdT o = rasterize_fwd_c(means2d, conics, colors, opacities, backgrounds, masks, width, height, tile_size, offsets,
                                       flatten_ids, needs_bwd, order, work, raw_stream_of(sf, means2d));
        check_rc(o.rc, "sc_rasterize_fwd");
        ctx->save_for_backward({means2d, conics, colors, opacities, or_empty(backgrounds, means2d),
                                masks.has_value() ? *masks : at::empty({0}, u8(means2d)), offsets, flatten_ids, o.alphas,
                                o.last.has_value() ? *o.last : at::empty({0}, i32(means2d)),
                                order.has_value() ? *order : at::empty({0}, i32(means2d))});
        ctx->saved_data["w"] = width; ctx->saved_data["h"] = height; ctx->saved_data["tile"] = tile_size;
        ctx->saved_data["abs"] = absgrad; ctx->saved_data["bg"] = backgrounds.has_value();
        ctx->saved_data["mask"] = masks.has_value(); ctx->saved_data["order"] = order.has_value();
        ctx->saved_data["sf"] = sf; ctx->saved_data["target"] = keep(absgrad_target);
        return {o.colors, o.alphas};
    }
    static variable_list backward(AutogradContext* ctx, variable_list g) {
        const auto sv = ctx->get_saved_variables();
        const Tensor &means2d = sv[0], &colors = sv[2], &render_alphas = sv[8];
        OptT bg, masks, order;
        if (ctx->saved_data["bg"].toBool()) bg = sv[4];
        if (ctx->saved_data["mask"].toBool()) masks = sv[5];
        if (ctx->saved_data["order"].toBool()) order = sv[10];
        const bool absgrad = ctx->saved_data["abs"].toBool();
        const Tensor v_rc = g[0].defined() ? g[0].contiguous()
                                           : at::zeros({render_alphas.size(0), render_alphas.size(1), render_alphas.size(2),
                                                        colors.size(-1)}, f32(means2d));
        const Tensor v_ra = g[1].defined() ? g[1].contiguous() : at::zeros_like(render_alphas);
        RasterBwdT o = rasterize_bwd_c(means2d, sv[1], colors, sv[3], bg, masks, ctx->saved_data["w"].toInt(),
                                       ctx->saved_data["h"].toInt(), ctx->saved_data["tile"].toInt(), sv[6], sv[7], render_alphas,
                                       sv[9], v_rc, v_ra, absgrad, order, raw_stream_of(ctx->saved_data["sf"], means2d));
        check_rc(o.rc, "sc_rasterize_bwd");
        if (absgrad && o.v_abs.has_value()) {
            // gsplat's contract (street_gaussian_model.py:505-506): the tensor OBJECT the caller passed as means2d gets `.absgrad`
            py::gil_scoped_acquire gil;
            py::reinterpret_borrow<py::object>(kept(ctx->saved_data["target"])).attr("absgrad") = py::cast(*o.v_abs);
        }
        Tensor v_bg;
        if (bg.has_value() && ctx->needs_input_grad(4)) v_bg = (v_rc * (1.0 - render_alphas)).sum(at::IntArrayRef({1, 2}));
        return {o.v_m, o.v_c, o.v_col, o.v_o, v_bg, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(),
                Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

py::tuple projection_autograd(const Tensor& means, const Tensor& quats, const Tensor& scales, const Tensor& viewmats,
                              const Tensor& Ks, int64_t width, int64_t height, double eps2d, double near_plane,
                              double far_plane, double radius_clip, bool calc_comp, py::object stream_fn) {
    variable_list o = ProjectionFn::apply(means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane,
                                          radius_clip, calc_comp, stream_fn);
    if (calc_comp) return py::make_tuple(o[0], o[1], o[2], o[3], o[4]);
    return py::make_tuple(o[0], o[1], o[2], o[3]);
}
Tensor sh_autograd(int64_t degree, const Tensor& dirs, const Tensor& coeffs, const OptT& masks, py::object stream_fn) {
    return ShFn::apply(degree, dirs, coeffs, masks, stream_fn);
}
py::tuple rasterize_autograd(const Tensor& means2d, const Tensor& conics, const Tensor& colors, const Tensor& opacities,
                             const OptT& backgrounds, const OptT& masks, int64_t width, int64_t height, int64_t tile_size,
                             const Tensor& offsets, const Tensor& flatten_ids, bool absgrad, const OptT& order,
                             const OptT& work, py::object absgrad_target, py::object stream_fn) {
    variable_list o = RasterFn::apply(means2d, conics, colors, opacities, backgrounds, masks, width, height, tile_size, offsets,
                                      flatten_ids, absgrad, order, work, absgrad_target, stream_fn);
    return py::make_tuple(o[0], o[1]);
}

// ---- frame export ---------------------------------------------------------------------------------------------
int frame_composite_u8_strided(int64_t fg_ptr, int64_t fg_pix, int64_t fg_ch, int64_t acc_ptr, int64_t sky_ptr, int64_t sky_pix,
                               int64_t sky_ch, int64_t n_pixels, int64_t rounding, const Tensor& out, int64_t stream) {
    return sc_frame_composite_u8_strided(reinterpret_cast<const float*>(static_cast<uintptr_t>(fg_ptr)), fg_pix, fg_ch,
                                         reinterpret_cast<const float*>(static_cast<uintptr_t>(acc_ptr)),
                                         reinterpret_cast<const float*>(static_cast<uintptr_t>(sky_ptr)), sky_pix, sky_ch,
                                         n_pixels, (int)rounding, static_cast<uint8_t*>(out.data_ptr()), S(stream));
}
int frame_composite_u8(int64_t fg_ptr, int64_t fg_stride, int64_t acc_ptr, int64_t sky_ptr, int64_t sky_stride,
                       int64_t n_pixels, int64_t rounding, const Tensor& out, int64_t stream) {
    return sc_frame_composite_u8(reinterpret_cast<const float*>(static_cast<uintptr_t>(fg_ptr)), (int)fg_stride,
                                 reinterpret_cast<const float*>(static_cast<uintptr_t>(acc_ptr)),
                                 reinterpret_cast<const float*>(static_cast<uintptr_t>(sky_ptr)), (int)sky_stride, n_pixels,
                                 (int)rounding, static_cast<uint8_t*>(out.data_ptr()), S(stream));
}


// ---- photometric loss (csrc/losses.hip) ------------------------------------------------------------------------
// The images and the mask are taken as the (possibly strided) views they are: strides travel in `strides` (11 elements,
// include/street_crafter_amd.h sc_loss_fwd).  -> (rc, ssim [B+1], l1 [B], kept i64[B], a1 | None, a2 | None, b | None,
// c | None); the maps are written only when a gradient is wanted.
inline void req_view(const Tensor& t, at::ScalarType dt, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must live on a HIP device (got ", t.device(), "); street_crafter_amd has no CPU path");
    TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
}
py::tuple loss_fwd(const Tensor& img1, const Tensor& img2, const OptT& mask, const std::vector<int64_t>& strides,
                   int64_t B, int64_t C, int64_t H, int64_t W, int64_t mask_b, int64_t mask_h, int64_t mask_w,
                   int64_t window, bool want_a1, bool want_a2, int64_t stream) {
    req_view(img1, at::kFloat, "img1"); req_view(img2, at::kFloat, "img2");
    if (mask) req_view(*mask, at::kBool, "mask");
    TORCH_CHECK(strides.size() == 11, "loss_fwd: 11 strides expected");
    Tensor ssim = at::empty({B + 1}, f32(img1));
    Tensor l1 = at::empty({B}, f32(img1));
    Tensor kept = at::empty({B}, img1.options().dtype(at::kLong));
    const size_t ws_bytes = sc_loss_workspace_bytes((int)B, (int)C, (int)H, (int)W);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes, 8)}, u8(img1));
    OptT a1, a2, bm, cm;
    if (want_a1 || want_a2) {
        bm = at::empty({B, C, H, W}, f32(img1));
        cm = at::empty({B, C, H, W}, f32(img1));
        if (want_a1) a1 = at::empty({B, C, H, W}, f32(img1));
        if (want_a2) a2 = at::empty({B, C, H, W}, f32(img1));
    }
    const int rc = sc_loss_fwd(fp(img1), fp(img2), mask ? static_cast<const uint8_t*>(mask->data_ptr()) : nullptr,
                               strides.data(), (int)B, (int)C, (int)H, (int)W, (int)mask_b, (int)mask_h, (int)mask_w,
                               (int)window, fpw(ssim), fpw(l1), static_cast<int64_t*>(kept.data_ptr()),
                               a1 ? fpw(*a1) : nullptr, a2 ? fpw(*a2) : nullptr, bm ? fpw(*bm) : nullptr,
                               cm ? fpw(*cm) : nullptr, ws.data_ptr(), ws_bytes, S(stream));
    return py::make_tuple(rc, ssim, l1, kept, a1, a2, bm, cm);
}
// -> (rc, grad1 | None, grad2 | None), contiguous [B,C,H,W]
py::tuple loss_bwd(const Tensor& img1, const Tensor& img2, const OptT& mask, const std::vector<int64_t>& strides,
                   int64_t B, int64_t C, int64_t H, int64_t W, int64_t mask_b, int64_t mask_h, int64_t mask_w,
                   int64_t window, const OptT& a1, const OptT& a2, const OptT& bm, const OptT& cm, const OptT& g_ssim,
                   const OptT& g_l1, const OptT& kept, bool need1, bool need2, int64_t stream) {
    req_view(img1, at::kFloat, "img1"); req_view(img2, at::kFloat, "img2");
    if (mask) req_view(*mask, at::kBool, "mask");
    TORCH_CHECK(strides.size() == 11, "loss_bwd: 11 strides expected");
    if (g_ssim) req(*g_ssim, at::kFloat, "g_ssim");
    if (g_l1) req(*g_l1, at::kFloat, "g_l1");
    OptT g1, g2;
    if (need1) g1 = at::empty({B, C, H, W}, f32(img1));
    if (need2) g2 = at::empty({B, C, H, W}, f32(img1));
    const int rc = sc_loss_bwd(fp(img1), fp(img2), mask ? static_cast<const uint8_t*>(mask->data_ptr()) : nullptr,
                               strides.data(), (int)B, (int)C, (int)H, (int)W, (int)mask_b, (int)mask_h, (int)mask_w,
                               (int)window, fpo(a1), fpo(a2), fpo(bm), fpo(cm), fpo(g_ssim), fpo(g_l1),
                               kept ? static_cast<const int64_t*>(kept->data_ptr()) : nullptr, g1 ? fpw(*g1) : nullptr,
                               g2 ? fpw(*g2) : nullptr, S(stream));
    return py::make_tuple(rc, g1, g2);
}

// ---- regularizers (csrc/regularizers.hip) --------------------------------------------------------------------
// Inputs are the [1,H,W] views they are; strides travel in `strides` (6 for the depth loss, 5 for the accumulation
// losses: include/street_crafter_amd.h).  Nothing here waits for the device.
// -> (rc, value 0-d, threshold 0-d, counts i64[3] = {n, k, below}, workspace u8): the backward reads the workspace.
py::tuple depth_trim_fwd(const Tensor& depth, const Tensor& lidar, const OptT& mask, const std::vector<int64_t>& strides,
                         int64_t H, int64_t W, double keep, int64_t stream) {
    req_view(depth, at::kFloat, "depth"); req_view(lidar, at::kFloat, "lidar_depth");
    if (mask) req_view(*mask, at::kBool, "mask");
    TORCH_CHECK(strides.size() == 6, "depth_trim_fwd: 6 strides expected");
    Tensor value = at::empty({}, f32(depth));
    Tensor threshold = at::empty({}, f32(depth));
    Tensor counts = at::empty({3}, depth.options().dtype(at::kLong));
    const size_t ws_bytes = sc_depth_trim_workspace_bytes((int)H, (int)W);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes, 8)}, u8(depth));
    const int rc = sc_depth_trim_fwd(fp(depth), fp(lidar), mask ? static_cast<const uint8_t*>(mask->data_ptr()) : nullptr,
                                     strides.data(), (int)H, (int)W, keep, fpw(value), fpw(threshold),
                                     static_cast<int64_t*>(counts.data_ptr()), ws.data_ptr(), ws_bytes, S(stream));
    return py::make_tuple(rc, value, threshold, counts, ws);
}
// -> (rc, grad_depth | None, grad_lidar | None), contiguous [1,H,W]
py::tuple depth_trim_bwd(const Tensor& depth, const Tensor& lidar, const OptT& mask, const std::vector<int64_t>& strides,
                         int64_t H, int64_t W, const Tensor& g, const Tensor& ws, bool need_depth, bool need_lidar,
                         int64_t stream) {
    req_view(depth, at::kFloat, "depth"); req_view(lidar, at::kFloat, "lidar_depth");
    if (mask) req_view(*mask, at::kBool, "mask");
    req(g, at::kFloat, "grad"); req(ws, at::kByte, "workspace");
    TORCH_CHECK(strides.size() == 6, "depth_trim_bwd: 6 strides expected");
    OptT gd, gl;
    if (need_depth) gd = at::empty({1, H, W}, f32(depth));
    if (need_lidar) gl = at::empty({1, H, W}, f32(depth));
    const int rc = sc_depth_trim_bwd(fp(depth), fp(lidar), mask ? static_cast<const uint8_t*>(mask->data_ptr()) : nullptr,
                                     strides.data(), (int)H, (int)W, fp(g), ws.data_ptr(), (size_t)ws.numel(),
                                     gd ? fpw(*gd) : nullptr, gl ? fpw(*gl) : nullptr, S(stream));
    return py::make_tuple(rc, gd, gl);
}
// -> (rc, value 0-d)
py::tuple acc_reg_fwd(const Tensor& acc, const Tensor& mask, const std::vector<int64_t>& strides, int64_t Cm, int64_t H,
                      int64_t W, int64_t mode, int64_t stream) {
    req_view(acc, at::kFloat, "acc"); req_view(mask, at::kBool, "mask");
    TORCH_CHECK(strides.size() == 5, "acc_reg_fwd: 5 strides expected");
    Tensor value = at::empty({}, f32(acc));
    const size_t ws_bytes = sc_acc_reg_workspace_bytes((int)H, (int)W);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes, 8)}, u8(acc));
    const int rc = sc_acc_reg_fwd(fp(acc), static_cast<const uint8_t*>(mask.data_ptr()), strides.data(), (int)Cm, (int)H,
                                  (int)W, (int)mode, fpw(value), ws.data_ptr(), ws_bytes, S(stream));
    return py::make_tuple(rc, value);
}
// -> (rc, grad_acc) contiguous [1,H,W]
py::tuple acc_reg_bwd(const Tensor& acc, const Tensor& mask, const std::vector<int64_t>& strides, int64_t Cm, int64_t H,
                      int64_t W, int64_t mode, const Tensor& g, int64_t stream) {
    req_view(acc, at::kFloat, "acc"); req_view(mask, at::kBool, "mask");
    req(g, at::kFloat, "grad");
    TORCH_CHECK(strides.size() == 5, "acc_reg_bwd: 5 strides expected");
    Tensor ga = at::empty({1, H, W}, f32(acc));
    const int rc = sc_acc_reg_bwd(fp(acc), static_cast<const uint8_t*>(mask.data_ptr()), strides.data(), (int)Cm, (int)H,
                                  (int)W, (int)mode, fp(g), fpw(ga), S(stream));
    return py::make_tuple(rc, ga);
}

// ---- frame tail (csrc/frame_tail.hip) ------------------------------------------------------------------------------
// colors [1,H,W,D] dense, or with colors_planar the permuted view of dense [1,D,H,W] planes; alphas [1,H,W,1] dense (a
// storage offset is fine); sky is the view it is, its (channel, row, column) strides travel in `sky_strides`; affine
// [3,4] dense.  -> (rc, rgb [3,H,W], depth [1,H,W] | None (D == 3))
py::tuple frame_tail_fwd(const Tensor& colors, bool colors_planar, const Tensor& alphas, const OptT& sky, const std::vector<int64_t>& sky_strides,
                         const OptT& affine, int64_t H, int64_t W, bool clamp, int64_t stream) {
    req_view(colors, at::kFloat, "render_colors"); req(alphas, at::kFloat, "render_alphas");
    if (sky) req_view(*sky, at::kFloat, "sky");
    if (affine) req(*affine, at::kFloat, "affine");
    TORCH_CHECK(sky_strides.size() == 3, "frame_tail_fwd: 3 sky strides expected");
    const int64_t D = colors.size(-1);
    Tensor rgb = at::empty({3, H, W}, f32(colors));
    OptT depth;
    if (D == 4) depth = at::empty({1, H, W}, f32(colors));
    const int rc = sc_frame_tail_fwd(fp(colors), (int)D, colors_planar ? 1 : 0, fp(alphas), fpo(sky), sky_strides.data(), fpo(affine), (int)H,
                                     (int)W, clamp ? 1 : 0, fpw(rgb), depth ? fpw(*depth) : nullptr, S(stream));
    return py::make_tuple(rc, rgb, depth);
}
// -> (rc, grad_colors [1,H,W,D] | None, grad_alphas [1,H,W,1] | None, grad_sky ([3,H,W] if sky_planar else [1,H,W,3]) |
//     None, grad_affine [3,4] | None)
py::tuple frame_tail_bwd(const Tensor& colors, bool colors_planar, const Tensor& alphas, const OptT& sky, const std::vector<int64_t>& sky_strides,
                         const OptT& affine, int64_t H, int64_t W, const OptT& g, const OptT& h, bool need_colors,
                         bool need_alphas, bool need_sky, bool sky_planar, bool need_affine, int64_t stream) {
    req_view(colors, at::kFloat, "render_colors"); req(alphas, at::kFloat, "render_alphas");
    if (sky) req_view(*sky, at::kFloat, "sky");
    if (affine) req(*affine, at::kFloat, "affine");
    if (g) req(*g, at::kFloat, "grad_rgb");
    if (h) req(*h, at::kFloat, "grad_depth");
    TORCH_CHECK(sky_strides.size() == 3, "frame_tail_bwd: 3 sky strides expected");
    const int64_t D = colors.size(-1);
    OptT gc, ga, gs, gA, ws;
    if (need_colors) gc = at::empty({1, H, W, D}, f32(colors));
    if (need_alphas) ga = at::empty({1, H, W, 1}, f32(colors));
    if (need_sky) gs = sky_planar ? at::empty({3, H, W}, f32(colors)) : at::empty({1, H, W, 3}, f32(colors));
    size_t ws_bytes = 0;
    if (need_affine) {
        gA = at::empty({3, 4}, f32(colors));
        ws_bytes = sc_frame_tail_workspace_bytes((int)H, (int)W);
        ws = at::empty({(int64_t)std::max<size_t>(ws_bytes, 8)}, u8(colors));
    }
    const int rc = sc_frame_tail_bwd(fp(colors), (int)D, colors_planar ? 1 : 0, fp(alphas), fpo(sky), sky_strides.data(), fpo(affine), (int)H,
                                     (int)W, fpo(g), fpo(h), gc ? fpw(*gc) : nullptr, ga ? fpw(*ga) : nullptr,
                                     gs ? fpw(*gs) : nullptr, sky_planar ? 1 : 0, gA ? fpw(*gA) : nullptr,
                                     ws ? ws->data_ptr() : nullptr, ws_bytes, S(stream));
    return py::make_tuple(rc, gc, ga, gs, gA);
}

// ---- sky cube map (csrc/cubemap.hip) ---------------------------------------------------------------------------------
// ray_m: the 9 floats of M = R^T K^-1 (host), or None with dirs.  -> (rc, out): [C,n] with the planar flag, else [n,C]
struct RayM {
    float m[9];
    const float* p = nullptr;
    explicit RayM(const c10::optional<std::vector<double>>& v) {
        if (!v) return;
        TORCH_CHECK(v->size() == 9, "cubemap: ray_m must hold 9 numbers");
        for (int k = 0; k < 9; ++k) m[k] = (float)(*v)[k];
        p = m;
    }
};
inline const uint8_t* u8o(const OptT& t) { return t.has_value() ? static_cast<const uint8_t*>(t->data_ptr()) : nullptr; }
void cubemap_req(const Tensor& tex, const OptT& dirs, const OptT& perturb, const OptT& mask, const OptT& acc) {
    req(tex, at::kFloat, "tex");
    if (dirs) req(*dirs, at::kFloat, "dirs");
    if (perturb) req(*perturb, at::kFloat, "perturb");
    if (mask) req(*mask, at::kBool, "mask");
    if (acc) req(*acc, at::kFloat, "acc");
}
py::tuple cubemap_fwd(const Tensor& tex, const OptT& dirs, const c10::optional<std::vector<double>>& ray_m,
                      const OptT& perturb, const OptT& mask, const OptT& acc, int64_t R, int64_t C, int64_t n,
                      int64_t width, int64_t flags, double fill, int64_t stream) {
    cubemap_req(tex, dirs, perturb, mask, acc);
    const RayM m(ray_m);
    Tensor out = (flags & SC_CUBE_PLANAR) ? at::empty({C, n}, f32(tex)) : at::empty({n, C}, f32(tex));
    const int rc = sc_cubemap_fwd(fp(tex), (int)R, (int)C, fpo(dirs), m.p, fpo(perturb), u8o(mask), fpo(acc), n, (int)width,
                                  (int)flags, (float)fill, fpw(out), S(stream));
    return py::make_tuple(rc, out);
}
// -> (rc, grad_tex [6,R,R,C])
py::tuple cubemap_bwd(const Tensor& tex, const OptT& dirs, const c10::optional<std::vector<double>>& ray_m,
                      const OptT& perturb, const OptT& mask, const OptT& acc, int64_t R, int64_t C, int64_t n,
                      int64_t width, int64_t flags, double fill, const Tensor& grad_out, int64_t stream) {
    cubemap_req(tex, dirs, perturb, mask, acc);
    req(grad_out, at::kFloat, "grad_out");
    const RayM m(ray_m);
    Tensor gt = at::empty({6, R, R, C}, f32(tex));
    const int rc = sc_cubemap_bwd(fp(tex), (int)R, (int)C, fpo(dirs), m.p, fpo(perturb), u8o(mask), fpo(acc), n, (int)width,
                                  (int)flags, (float)fill, fp(grad_out), fpw(gt), S(stream));
    return py::make_tuple(rc, gt);
}

// ---- perceptual loss (csrc/lpips.hip) ---------------------------------------------------------------------------------
// street_crafter_amd/lpips.py has validated shapes and strides; here outputs and the workspace are allocated and the
// entries called.  The image and the features are the views they are.  Nothing here waits for the device.
inline void lpips_host3(const std::vector<double>& v, float (&out)[3], const char* name) {
    TORCH_CHECK(v.size() == 3, "lpips: ", name, " must hold 3 numbers");
    for (int k = 0; k < 3; ++k) out[k] = (float)v[k];
}
// -> (rc, z [1,3,H,W])
py::tuple lpips_prep_fwd(const Tensor& img, const OptT& mask, const std::vector<int64_t>& strides, int64_t H, int64_t W,
                         const std::vector<double>& mean, const std::vector<double>& std_, int64_t stream) {
    req_view(img, at::kFloat, "img");
    if (mask) req_view(*mask, at::kBool, "mask");
    TORCH_CHECK(strides.size() == 5, "lpips_prep_fwd: 5 strides expected");
    float m[3], s[3];
    lpips_host3(mean, m, "mean"); lpips_host3(std_, s, "std");
    Tensor out = at::empty({1, 3, H, W}, f32(img));
    const int rc = sc_lpips_prep_fwd(fp(img), u8o(mask), strides.data(), (int)H, (int)W, m, s, fpw(out), S(stream));
    return py::make_tuple(rc, out);
}
// -> (rc, grad_img [3,H,W])
py::tuple lpips_prep_bwd(const Tensor& grad_out, const OptT& mask, const std::vector<int64_t>& strides, int64_t H, int64_t W,
                         const std::vector<double>& std_, int64_t stream) {
    req(grad_out, at::kFloat, "grad_out");
    if (mask) req_view(*mask, at::kBool, "mask");
    TORCH_CHECK(strides.size() == 5, "lpips_prep_bwd: 5 strides expected");
    TORCH_CHECK(grad_out.numel() == 3 * H * W, "lpips_prep_bwd: grad_out is not [3,H,W]");
    float s[3];
    lpips_host3(std_, s, "std");
    Tensor gi = at::empty({3, H, W}, f32(grad_out));
    const int rc = sc_lpips_prep_bwd(fp(grad_out), u8o(mask), strides.data(), (int)H, (int)W, s, fpw(gi), S(stream));
    return py::make_tuple(rc, gi);
}
std::vector<sc_lpips_tap> lpips_table(const std::vector<Tensor>& fx, const std::vector<Tensor>& fy,
                                      const std::vector<Tensor>& weight, const std::vector<int64_t>& channels,
                                      const std::vector<int64_t>& pixels, const std::vector<int64_t>& stride_x,
                                      const std::vector<int64_t>& stride_y) {
    const size_t n = fx.size();
    TORCH_CHECK(n > 0 && fy.size() == n && weight.size() == n && channels.size() == n && pixels.size() == n &&
                stride_x.size() == n && stride_y.size() == n, "lpips_head: lists of different length");
    std::vector<sc_lpips_tap> table(n);
    for (size_t k = 0; k < n; ++k) {
        req_view(fx[k], at::kFloat, "feats_x"); req_view(fy[k], at::kFloat, "feats_y"); req(weight[k], at::kFloat, "lin_weights");
        TORCH_CHECK(channels[k] > 0 && pixels[k] > 0 && channels[k] <= INT32_MAX && pixels[k] <= INT32_MAX &&
                    weight[k].numel() == channels[k], "lpips_head: tap ", k, ": bad sizes");
        sc_lpips_tap& t = table[k];
        t = sc_lpips_tap{};
        t.fx = fp(fx[k]); t.fy = fp(fy[k]); t.weight = fp(weight[k]);
        t.stride_x = stride_x[k]; t.stride_y = stride_y[k];
        t.channels = (int32_t)channels[k]; t.pixels = (int32_t)pixels[k];
    }
    return table;
}
// -> (rc, out [n_taps + 1] = the taps' distances, then their sum, [norm_x [P]] | None, [norm_y [P]] | None)
py::tuple lpips_head_fwd(const std::vector<Tensor>& fx, const std::vector<Tensor>& fy, const std::vector<Tensor>& weight,
                         const std::vector<int64_t>& channels, const std::vector<int64_t>& pixels,
                         const std::vector<int64_t>& stride_x, const std::vector<int64_t>& stride_y, bool want_norms,
                         int64_t stream) {
    std::vector<sc_lpips_tap> table = lpips_table(fx, fy, weight, channels, pixels, stride_x, stride_y);
    const size_t n = table.size();
    Tensor out = at::empty({(int64_t)n + 1}, f32(fx[0]));
    c10::optional<std::vector<Tensor>> nx, ny;
    if (want_norms) {
        nx = std::vector<Tensor>(n);
        ny = std::vector<Tensor>(n);
        for (size_t k = 0; k < n; ++k) {
            (*nx)[k] = at::empty({pixels[k]}, f32(fx[0]));
            (*ny)[k] = at::empty({pixels[k]}, f32(fx[0]));
            table[k].norm_x = fpw((*nx)[k]); table[k].norm_y = fpw((*ny)[k]);
        }
    }
    const size_t ws_bytes = sc_lpips_head_workspace_bytes(table.data(), (int)n);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes / 8, 1)}, fx[0].options().dtype(at::kDouble));
    const int rc = sc_lpips_head_fwd(table.data(), (int)n, fpw(out), ws.data_ptr(), ws_bytes, S(stream));
    return py::make_tuple(rc, out, nx, ny);
}
// -> (rc, [grad_fx [C,P] | None], [grad_fy [C,P] | None])
py::tuple lpips_head_bwd(const std::vector<Tensor>& fx, const std::vector<Tensor>& fy, const std::vector<Tensor>& weight,
                         const std::vector<int64_t>& channels, const std::vector<int64_t>& pixels,
                         const std::vector<int64_t>& stride_x, const std::vector<int64_t>& stride_y,
                         const std::vector<Tensor>& norm_x, const std::vector<Tensor>& norm_y, const Tensor& grad,
                         const std::vector<bool>& need_x, const std::vector<bool>& need_y, int64_t stream) {
    std::vector<sc_lpips_tap> table = lpips_table(fx, fy, weight, channels, pixels, stride_x, stride_y);
    const size_t n = table.size();
    TORCH_CHECK(norm_x.size() == n && norm_y.size() == n && need_x.size() == n && need_y.size() == n,
                "lpips_head_bwd: lists of different length");
    req(grad, at::kFloat, "grad");
    TORCH_CHECK(grad.numel() == 1, "lpips_head_bwd: grad must hold one number");
    std::vector<OptT> gx(n), gy(n);
    for (size_t k = 0; k < n; ++k) {
        req(norm_x[k], at::kFloat, "norm_x"); req(norm_y[k], at::kFloat, "norm_y");
        TORCH_CHECK(norm_x[k].numel() == pixels[k] && norm_y[k].numel() == pixels[k], "lpips_head_bwd: tap ", k, ": norms are not [P]");
        table[k].norm_x = fpw(norm_x[k]); table[k].norm_y = fpw(norm_y[k]);
        if (need_x[k]) { gx[k] = at::empty({channels[k], pixels[k]}, f32(fx[0])); table[k].grad_fx = fpw(*gx[k]); }
        if (need_y[k]) { gy[k] = at::empty({channels[k], pixels[k]}, f32(fx[0])); table[k].grad_fy = fpw(*gy[k]); }
    }
    const int rc = sc_lpips_head_bwd(table.data(), (int)n, fp(grad), S(stream));
    return py::make_tuple(rc, gx, gy);
}

// ---- crop + resize of the novel-view inputs (csrc/resize.hip) --------------------------------------------------------
// street_crafter_amd/resize.py has validated shapes and built the tap tables (int32 idx, fp32 weights, on the device); x is
// the cropped view it is.  -> (rc, out [B,C,h_out - row_begin,w_out])
py::tuple resize_fwd(const Tensor& x, const std::vector<int64_t>& strides, int64_t B, int64_t C, int64_t in_h, int64_t in_w,
                     const Tensor& ty_idx, const Tensor& ty_w, const Tensor& tx_idx, const Tensor& tx_w, int64_t h_out,
                     int64_t w_out, int64_t row_begin, int64_t flags, double a, double b, int64_t stream) {
    req_view(x, at::kFloat, "x");
    req(ty_idx, at::kInt, "ty_idx"); req(ty_w, at::kFloat, "ty_w"); req(tx_idx, at::kInt, "tx_idx"); req(tx_w, at::kFloat, "tx_w");
    TORCH_CHECK(strides.size() == 4, "resize_fwd: 4 strides expected");
    Tensor out = at::empty({B, C, std::max<int64_t>(h_out - row_begin, 0), w_out}, f32(x));
    const int rc = sc_resize_fwd(fp(x), strides.data(), (int)B, (int)C, (int)in_h, (int)in_w, ip(ty_idx), fp(ty_w), ip(tx_idx),
                                 fp(tx_w), (int)h_out, (int)w_out, (int)row_begin, (int)flags, (float)a, (float)b, fpw(out),
                                 S(stream));
    return py::make_tuple(rc, out);
}
// -> (rc, out bool [B,C,h_out - row_begin,w_out])
py::tuple resize_mask_fwd(const Tensor& x, const std::vector<int64_t>& strides, int64_t B, int64_t C, int64_t in_h,
                          int64_t in_w, const Tensor& ty_idx, const Tensor& tx_idx, int64_t h_out, int64_t w_out,
                          int64_t row_begin, int64_t stream) {
    req_view(x, at::kBool, "x");
    req(ty_idx, at::kInt, "ty_idx"); req(tx_idx, at::kInt, "tx_idx");
    TORCH_CHECK(strides.size() == 4, "resize_mask_fwd: 4 strides expected");
    Tensor out = at::empty({B, C, std::max<int64_t>(h_out - row_begin, 0), w_out}, x.options().dtype(at::kBool));
    const int rc = sc_resize_mask_fwd(static_cast<const uint8_t*>(x.data_ptr()), strides.data(), (int)B, (int)C, (int)in_h,
                                      (int)in_w, ip(ty_idx), ip(tx_idx), (int)h_out, (int)w_out, (int)row_begin,
                                      static_cast<uint8_t*>(out.data_ptr()), S(stream));
    return py::make_tuple(rc, out);
}
// -> (rc, grad_x [B,C,H,W]): every element written
py::tuple resize_bwd(const Tensor& grad_out, int64_t B, int64_t C, int64_t H, int64_t W, int64_t top, int64_t left,
                     int64_t in_h, int64_t in_w, const Tensor& uy_idx, const Tensor& uy_w, const Tensor& ux_idx,
                     const Tensor& ux_w, int64_t h_out, int64_t w_out, int64_t row_begin, int64_t flags, double a,
                     int64_t stream) {
    req(grad_out, at::kFloat, "grad_out");
    req(uy_idx, at::kInt, "uy_idx"); req(uy_w, at::kFloat, "uy_w"); req(ux_idx, at::kInt, "ux_idx"); req(ux_w, at::kFloat, "ux_w");
    TORCH_CHECK(grad_out.numel() == B * C * (h_out - row_begin) * w_out, "resize_bwd: grad_out is not [B,C,rows,w_out]");
    Tensor gx = at::empty({B, C, H, W}, f32(grad_out));
    const int rc = sc_resize_bwd(fp(grad_out), (int)B, (int)C, (int)H, (int)W, (int)top, (int)left, (int)in_h, (int)in_w,
                                 ip(uy_idx), fp(uy_w), ip(ux_idx), fp(ux_w), (int)h_out, (int)w_out, (int)row_begin, (int)flags,
                                 (float)a, fpw(gx), S(stream));
    return py::make_tuple(rc, gx);
}

// ---- training tail (csrc/optim.hip) ----------------------------------------------------------------------------------
// The tables are built here from lists of tensors (street_crafter_amd/optim.py, densify_stats.py have validated what
// needs a Python-side answer: which parameters step, their step counts).  Nothing here allocates or waits.
int64_t adam_step(const std::vector<Tensor>& params, const std::vector<Tensor>& grads, const std::vector<Tensor>& exp_avg,
                  const std::vector<Tensor>& exp_avg_sq, const std::vector<double>& step_size,
                  const std::vector<double>& bias2_sqrt, double one_minus_beta1, double beta2, double one_minus_beta2,
                  double eps, int64_t stream) {
    const size_t n = params.size();
    TORCH_CHECK(grads.size() == n && exp_avg.size() == n && exp_avg_sq.size() == n && step_size.size() == n &&
                bias2_sqrt.size() == n, "adam_step: lists of different length");
    std::vector<sc_adam_tensor> table(n);
    for (size_t i = 0; i < n; ++i) {
        req(params[i], at::kFloat, "param"); req(grads[i], at::kFloat, "grad");
        req(exp_avg[i], at::kFloat, "exp_avg"); req(exp_avg_sq[i], at::kFloat, "exp_avg_sq");
        const int64_t numel = params[i].numel();
        TORCH_CHECK(grads[i].numel() == numel && exp_avg[i].numel() == numel && exp_avg_sq[i].numel() == numel,
                    "adam_step: tensor ", i, ": param, grad and moments differ in size");
        table[i] = {fpw(params[i]), fp(grads[i]), fpw(exp_avg[i]), fpw(exp_avg_sq[i]), numel, (float)step_size[i],
                    (float)bias2_sqrt[i]};
    }
    return sc_adam_step(table.data(), (int)n, (float)one_minus_beta1, (float)beta2, (float)one_minus_beta2, (float)eps,
                        S(stream));
}
// segments: (start, end) pairs in `ranges` (2 per segment) with their accumulators [n,2], [n,1], [n]
int64_t densify_stats(const Tensor& grad, const OptT& absgrad, const Tensor& radii, const Tensor& visible, int64_t N,
                      double half_width, double half_height, const std::vector<int64_t>& ranges,
                      const std::vector<Tensor>& grad_accum, const std::vector<Tensor>& denom,
                      const std::vector<Tensor>& max_radii, int64_t stream) {
    req(grad, at::kFloat, "grad");
    if (absgrad) req(*absgrad, at::kFloat, "absgrad");
    req(visible, at::kBool, "visibility_filter");
    const bool radii_float = radii.scalar_type() == at::kFloat;
    req(radii, radii_float ? at::kFloat : at::kInt, "radii");
    TORCH_CHECK(grad.numel() == 2 * N && (!absgrad || absgrad->numel() == 2 * N) && radii.numel() == N &&
                visible.numel() == N, "densify_stats: inputs do not have N rows");
    const size_t n = grad_accum.size();
    TORCH_CHECK(ranges.size() == 2 * n && denom.size() == n && max_radii.size() == n,
                "densify_stats: lists of different length");
    std::vector<sc_stats_segment> seg;
    seg.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        req(grad_accum[i], at::kFloat, "xyz_gradient_accum"); req(denom[i], at::kFloat, "denom");
        req(max_radii[i], at::kFloat, "max_radii2D");
        const int64_t rows = ranges[2 * i + 1] - ranges[2 * i];
        TORCH_CHECK(rows >= 0 && grad_accum[i].numel() == 2 * rows && denom[i].numel() == rows &&
                    max_radii[i].numel() == rows, "densify_stats: segment ", i, ": accumulators do not have end - start rows");
        TORCH_CHECK(ranges[2 * i] >= 0 && ranges[2 * i + 1] <= N, "densify_stats: segment ", i, " lies outside [0, N)");
        if (rows == 0) continue;       // (an empty tensor has no data pointer to hand over, and nothing to do)
        seg.push_back({ranges[2 * i], ranges[2 * i + 1], fpw(grad_accum[i]), fpw(denom[i]), fpw(max_radii[i])});
    }
    return sc_densify_stats(fp(grad), absgrad ? fp(*absgrad) : nullptr, radii.data_ptr(), radii_float ? 1 : 0,
                            static_cast<const uint8_t*>(visible.data_ptr()), N, (float)half_width, (float)half_height,
                            seg.data(), (int)seg.size(), S(stream));
}

// ---- the head of a frame (csrc/compose.hip) -----------------------------------------------------------------------------
// street_crafter_amd/compose.py has validated dtypes, shapes and the plan; here the segment table is built from lists of
// tensors, the outputs are allocated and the entry is called.  ranges: (start, end) pairs; flips: uint8 [n], numel 0 = no
// mask; fparams: 12 per segment (basis[8], centre[3], radius).
std::vector<sc_compose_segment> compose_table(const std::vector<Tensor>& xyz, const std::vector<Tensor>& scaling,
                                              const std::vector<Tensor>& rotation, const std::vector<Tensor>& opacity,
                                              const std::vector<Tensor>& features_dc,
                                              const std::vector<Tensor>& features_rest, const std::vector<Tensor>& flips,
                                              const std::vector<int64_t>& ranges, const std::vector<int64_t>& kinds,
                                              const std::vector<int64_t>& pose_rows, const std::vector<double>& fparams,
                                              int64_t K) {
    const size_t n = xyz.size();
    TORCH_CHECK(scaling.size() == n && rotation.size() == n && opacity.size() == n && features_dc.size() == n &&
                features_rest.size() == n && flips.size() == n && ranges.size() == 2 * n && kinds.size() == n &&
                pose_rows.size() == n && fparams.size() == 12 * n, "compose: lists of different length");
    std::vector<sc_compose_segment> table(n);
    for (size_t i = 0; i < n; ++i) {
        req(xyz[i], at::kFloat, "xyz"); req(scaling[i], at::kFloat, "scaling"); req(rotation[i], at::kFloat, "rotation");
        req(opacity[i], at::kFloat, "opacity"); req(features_dc[i], at::kFloat, "features_dc");
        req(features_rest[i], at::kFloat, "features_rest"); req(flips[i], at::kByte, "flip");
        const int64_t rows = ranges[2 * i + 1] - ranges[2 * i];
        TORCH_CHECK(features_dc[i].dim() == 3, "compose: features_dc must be [n,F,3]");
        const int64_t F = features_dc[i].size(1);
        TORCH_CHECK(rows >= 0 && xyz[i].numel() == 3 * rows && scaling[i].numel() == 3 * rows &&
                    rotation[i].numel() == 4 * rows && opacity[i].numel() == rows && features_dc[i].numel() == 3 * F * rows &&
                    features_rest[i].numel() == 3 * (K - 1) * rows && (flips[i].numel() == 0 || flips[i].numel() == rows),
                    "compose: segment ", i, ": tensors do not have end - start rows");
        sc_compose_segment& s = table[i];
        s.start = ranges[2 * i]; s.end = ranges[2 * i + 1];
        s.xyz = fp(xyz[i]); s.scaling = fp(scaling[i]); s.rotation = fp(rotation[i]); s.opacity = fp(opacity[i]);
        s.features_dc = fp(features_dc[i]); s.features_rest = fp(features_rest[i]);
        s.flip = flips[i].numel() ? static_cast<const uint8_t*>(flips[i].data_ptr()) : nullptr;
        s.kind = (int32_t)kinds[i]; s.pose_row = (int32_t)pose_rows[i]; s.fourier_dim = (int32_t)F; s.reserved = 0;
        for (int k = 0; k < SC_COMPOSE_MAX_FOURIER; ++k) s.basis[k] = (float)fparams[12 * i + k];
        for (int k = 0; k < 3; ++k) s.centre[k] = (float)fparams[12 * i + 8 + k];
        s.radius = (float)fparams[12 * i + 11];
    }
    return table;
}
inline bool compose_flip_q(const std::vector<double>& flip_q, float (&out)[4]) {
    TORCH_CHECK(flip_q.empty() || flip_q.size() == 4, "compose: flip_q must have 4 values");
    for (size_t k = 0; k < flip_q.size(); ++k) out[k] = (float)flip_q[k];
    return !flip_q.empty();
}
// -> (rc, means [N,3], quats [N,4], scales [N,3], opacities [N,1], sh [N,K,3])
py::tuple compose_fwd(const std::vector<Tensor>& xyz, const std::vector<Tensor>& scaling,
                      const std::vector<Tensor>& rotation, const std::vector<Tensor>& opacity,
                      const std::vector<Tensor>& features_dc, const std::vector<Tensor>& features_rest,
                      const std::vector<Tensor>& flips, const std::vector<int64_t>& ranges,
                      const std::vector<int64_t>& kinds, const std::vector<int64_t>& pose_rows,
                      const std::vector<double>& fparams, int64_t N, int64_t K, const OptT& obj_rots,
                      const OptT& obj_trans, int64_t A, const std::vector<double>& flip_q, int64_t stream) {
    TORCH_CHECK(!xyz.empty(), "compose_fwd: no segment");
    const auto table = compose_table(xyz, scaling, rotation, opacity, features_dc, features_rest, flips, ranges, kinds,
                                     pose_rows, fparams, K);
    if (obj_rots) { req(*obj_rots, at::kFloat, "obj_rots"); TORCH_CHECK(obj_rots->numel() == 4 * A, "obj_rots is not [A,4]"); }
    if (obj_trans) { req(*obj_trans, at::kFloat, "obj_trans"); TORCH_CHECK(obj_trans->numel() == 3 * A, "obj_trans is not [A,3]"); }
    float fq[4];
    const bool has_fq = compose_flip_q(flip_q, fq);
    const auto o = f32(xyz[0]);
    Tensor means = at::empty({N, 3}, o), quats = at::empty({N, 4}, o), scales = at::empty({N, 3}, o);
    Tensor opac = at::empty({N, 1}, o), sh = at::empty({N, K, 3}, o);
    const int rc = sc_compose_fwd(table.data(), (int)table.size(), N, (int)K, fpo(obj_rots), fpo(obj_trans), (int)A,
                                  has_fq ? fq : nullptr, fpw(means), fpw(quats), fpw(scales), fpw(opac), fpw(sh), S(stream));
    return py::make_tuple(rc, means, quats, scales, opac, sh);
}
// -> (rc, [g_xyz], [g_scaling], [g_rotation], [g_opacity], [g_features_dc], [g_features_rest], grad_obj_rots | None,
//     grad_obj_trans | None): every gradient written in full
py::tuple compose_bwd(const std::vector<Tensor>& xyz, const std::vector<Tensor>& scaling,
                      const std::vector<Tensor>& rotation, const std::vector<Tensor>& opacity,
                      const std::vector<Tensor>& features_dc, const std::vector<Tensor>& features_rest,
                      const std::vector<Tensor>& flips, const std::vector<int64_t>& ranges,
                      const std::vector<int64_t>& kinds, const std::vector<int64_t>& pose_rows,
                      const std::vector<double>& fparams, int64_t N, int64_t K, const OptT& obj_rots,
                      const OptT& obj_trans, int64_t A, const std::vector<double>& flip_q, const OptT& g_means,
                      const OptT& g_quats, const OptT& g_scales, const OptT& g_opacities, const OptT& g_sh,
                      bool want_rots, bool want_trans, int64_t stream) {
    TORCH_CHECK(!xyz.empty(), "compose_bwd: no segment");
    const auto table = compose_table(xyz, scaling, rotation, opacity, features_dc, features_rest, flips, ranges, kinds,
                                     pose_rows, fparams, K);
    if (obj_rots) { req(*obj_rots, at::kFloat, "obj_rots"); TORCH_CHECK(obj_rots->numel() == 4 * A, "obj_rots is not [A,4]"); }
    if (obj_trans) { req(*obj_trans, at::kFloat, "obj_trans"); TORCH_CHECK(obj_trans->numel() == 3 * A, "obj_trans is not [A,3]"); }
    const OptT* ups[5] = {&g_means, &g_quats, &g_scales, &g_opacities, &g_sh};
    const int64_t per_row[5] = {3, 4, 3, 1, 3 * K};
    for (int k = 0; k < 5; ++k)
        if (*ups[k]) {
            req(**ups[k], at::kFloat, "upstream gradient");
            TORCH_CHECK((*ups[k])->numel() == per_row[k] * N, "compose_bwd: an upstream gradient does not have N rows");
        }
    float fq[4];
    const bool has_fq = compose_flip_q(flip_q, fq);
    const size_t n = table.size();
    std::vector<Tensor> gx(n), gs(n), gr(n), go(n), gd(n), gf(n);
    std::vector<sc_compose_grads> grads(n);
    for (size_t i = 0; i < n; ++i) {
        gx[i] = at::empty_like(xyz[i]); gs[i] = at::empty_like(scaling[i]); gr[i] = at::empty_like(rotation[i]);
        go[i] = at::empty_like(opacity[i]); gd[i] = at::empty_like(features_dc[i]); gf[i] = at::empty_like(features_rest[i]);
        grads[i] = {fpw(gx[i]), fpw(gs[i]), fpw(gr[i]), fpw(go[i]), fpw(gd[i]), fpw(gf[i])};
    }
    const auto o = f32(xyz[0]);
    OptT grots, gtrans;
    if (want_rots) grots = at::empty({A, 4}, o);
    if (want_trans) gtrans = at::empty({A, 3}, o);
    const int rc = sc_compose_bwd(table.data(), grads.data(), (int)n, N, (int)K, fpo(obj_rots), fpo(obj_trans), (int)A,
                                  has_fq ? fq : nullptr, fpo(g_means), fpo(g_quats), fpo(g_scales), fpo(g_opacities),
                                  fpo(g_sh), grots ? fpw(*grots) : nullptr, gtrans ? fpw(*gtrans) : nullptr, S(stream));
    return py::make_tuple(rc, gx, gs, gr, go, gd, gf, grots, gtrans);
}

// ---- densify and prune (csrc/densify.hip) ----------------------------------------------------------------------------------
// street_crafter_amd/densify.py has validated shapes and thresholds; here the tables are built, the plan's outputs and
// workspace / the new tensors are allocated, and the entry is called.  Neither waits for the device.
// fparams: 11 per job (max_grad, dense_size, min_opacity, big_size, max_screen_size, region_a[3], region_b[3]);
// iparams: 3 per job (grad_col, prune_big, region).
// -> (rc, counters i32[J,8], [src_row i32[2n]], [slot u8[2n]], [child_xyz [2,n,3]], [child_scaling [2,n,3]])
py::tuple densify_plan(const std::vector<Tensor>& xyz, const std::vector<Tensor>& scaling,
                       const std::vector<Tensor>& rotation, const std::vector<Tensor>& opacity,
                       const std::vector<Tensor>& grad_accum, const std::vector<Tensor>& denom,
                       const std::vector<Tensor>& max_radii, const std::vector<Tensor>& split_noise,
                       const std::vector<OptT>& box_noise, const std::vector<double>& fparams,
                       const std::vector<int64_t>& iparams, int64_t stream) {
    const size_t J = xyz.size();
    TORCH_CHECK(J > 0, "densify_plan: no jobs");
    TORCH_CHECK(scaling.size() == J && rotation.size() == J && opacity.size() == J && grad_accum.size() == J &&
                denom.size() == J && max_radii.size() == J && split_noise.size() == J && box_noise.size() == J &&
                fparams.size() == 11 * J && iparams.size() == 3 * J, "densify_plan: lists of different length");
    Tensor counters = at::zeros({(int64_t)J, 8}, i32(xyz[0]));
    std::vector<Tensor> src_row(J), slot(J), child_xyz(J), child_scaling(J);
    std::vector<sc_densify_job> jobs(J);
    for (size_t k = 0; k < J; ++k) {
        const int64_t n = xyz[k].size(0);
        req(xyz[k], at::kFloat, "xyz"); req(scaling[k], at::kFloat, "scaling"); req(rotation[k], at::kFloat, "rotation");
        req(opacity[k], at::kFloat, "opacity"); req(grad_accum[k], at::kFloat, "xyz_gradient_accum");
        req(denom[k], at::kFloat, "denom"); req(max_radii[k], at::kFloat, "max_radii2D");
        req(split_noise[k], at::kFloat, "split_noise");
        if (box_noise[k]) req(*box_noise[k], at::kFloat, "box_noise");
        TORCH_CHECK(xyz[k].numel() == 3 * n && scaling[k].numel() == 3 * n && rotation[k].numel() == 4 * n &&
                    opacity[k].numel() == n && grad_accum[k].numel() == 2 * n && denom[k].numel() == n &&
                    max_radii[k].numel() == n && split_noise[k].numel() == 6 * n &&
                    (!box_noise[k] || box_noise[k]->numel() == 24 * n), "densify_plan: job ", k, ": tensors do not have n rows");
        src_row[k] = at::empty({2 * n}, i32(xyz[k]));
        slot[k] = at::empty({2 * n}, u8(xyz[k]));
        child_xyz[k] = at::empty({2, n, 3}, f32(xyz[k]));
        child_scaling[k] = at::empty({2, n, 3}, f32(xyz[k]));
        sc_densify_job& j = jobs[k];
        j.n = n;
        j.xyz = fp(xyz[k]); j.scaling = fp(scaling[k]); j.rotation = fp(rotation[k]); j.opacity = fp(opacity[k]);
        j.grad_accum = fp(grad_accum[k]); j.denom = fp(denom[k]); j.max_radii = fp(max_radii[k]);
        j.split_noise = fp(split_noise[k]); j.box_noise = fpo(box_noise[k]);
        j.src_row = static_cast<int32_t*>(src_row[k].data_ptr()); j.slot = static_cast<uint8_t*>(slot[k].data_ptr());
        j.child_xyz = fpw(child_xyz[k]); j.child_scaling = fpw(child_scaling[k]);
        j.counters = static_cast<int32_t*>(counters.data_ptr()) + 8 * k;
        const double* f = &fparams[11 * k];
        j.max_grad = (float)f[0]; j.dense_size = (float)f[1]; j.min_opacity = (float)f[2]; j.big_size = (float)f[3];
        j.max_screen_size = (float)f[4];
        for (int d = 0; d < 3; ++d) { j.region_a[d] = (float)f[5 + d]; j.region_b[d] = (float)f[8 + d]; }
        j.grad_col = (int32_t)iparams[3 * k]; j.prune_big = (int32_t)iparams[3 * k + 1]; j.region = (int32_t)iparams[3 * k + 2];
    }
    const size_t ws_bytes = sc_densify_plan_workspace_bytes(jobs.data(), (int)J);
    Tensor ws = at::empty({(int64_t)std::max<size_t>(ws_bytes, 256)}, u8(xyz[0]));
    const int rc = sc_densify_plan(jobs.data(), (int)J, ws.data_ptr(), ws_bytes, S(stream));
    return py::make_tuple(rc, counters, src_row, slot, child_xyz, child_scaling);
}
// one entry per parameter group; moments and child None where absent
// -> (rc, [dst_param [n_out,width]], [dst_exp_avg | None], [dst_exp_avg_sq | None])
py::tuple densify_apply(const std::vector<Tensor>& src_param, const std::vector<OptT>& src_exp_avg,
                        const std::vector<OptT>& src_exp_avg_sq, const std::vector<OptT>& child,
                        const std::vector<Tensor>& src_row, const std::vector<Tensor>& slot, const std::vector<int64_t>& n,
                        const std::vector<int64_t>& n_out, const std::vector<int64_t>& width, int64_t stream) {
    const size_t G = src_param.size();
    TORCH_CHECK(src_exp_avg.size() == G && src_exp_avg_sq.size() == G && child.size() == G && src_row.size() == G &&
                slot.size() == G && n.size() == G && n_out.size() == G && width.size() == G,
                "densify_apply: lists of different length");
    std::vector<Tensor> dst_param(G);
    std::vector<OptT> dst_m(G), dst_v(G);
    std::vector<sc_densify_group> groups(G);
    for (size_t k = 0; k < G; ++k) {
        req(src_param[k], at::kFloat, "param"); req(src_row[k], at::kInt, "src_row"); req(slot[k], at::kByte, "slot");
        TORCH_CHECK(n[k] >= 0 && n_out[k] >= 0 && width[k] >= 0 && width[k] <= INT32_MAX &&
                    src_param[k].numel() == n[k] * width[k] && src_row[k].numel() >= n_out[k] && slot[k].numel() >= n_out[k],
                    "densify_apply: group ", k, ": sizes do not match");
        TORCH_CHECK(src_exp_avg[k].has_value() == src_exp_avg_sq[k].has_value(), "densify_apply: group ", k, ": one moment");
        sc_densify_group& g = groups[k];
        g = sc_densify_group{};
        dst_param[k] = at::empty({n_out[k], width[k]}, f32(src_param[k]));
        g.src_param = fp(src_param[k]); g.dst_param = fpw(dst_param[k]);
        if (src_exp_avg[k]) {
            req(*src_exp_avg[k], at::kFloat, "exp_avg"); req(*src_exp_avg_sq[k], at::kFloat, "exp_avg_sq");
            TORCH_CHECK(src_exp_avg[k]->numel() == n[k] * width[k] && src_exp_avg_sq[k]->numel() == n[k] * width[k],
                        "densify_apply: group ", k, ": moments differ in size from the parameter");
            dst_m[k] = at::empty({n_out[k], width[k]}, f32(src_param[k]));
            dst_v[k] = at::empty({n_out[k], width[k]}, f32(src_param[k]));
            // (an empty tensor may have no data pointer: such a group moves nothing, and one moment pointer without the
            //  others is refused by the entry)
            if (n_out[k] * width[k] > 0) {
                g.src_exp_avg = fp(*src_exp_avg[k]); g.src_exp_avg_sq = fp(*src_exp_avg_sq[k]);
                g.dst_exp_avg = fpw(*dst_m[k]); g.dst_exp_avg_sq = fpw(*dst_v[k]);
            }
        }
        if (child[k]) {
            req(*child[k], at::kFloat, "child");
            TORCH_CHECK(child[k]->numel() == 2 * n[k] * width[k], "densify_apply: group ", k, ": child rows are not [2,n,width]");
            g.child = fp(*child[k]);
        }
        g.src_row = ip(src_row[k]); g.slot = static_cast<const uint8_t*>(slot[k].data_ptr());
        g.n = n[k]; g.n_out = n_out[k]; g.width = (int32_t)width[k];
    }
    const int rc = sc_densify_apply(groups.data(), (int)G, S(stream));
    return py::make_tuple(rc, dst_param, dst_m, dst_v);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "street_crafter_amd: compiled Python <-> C-ABI binding layer (allocation + call per operator)";
    // (the header digest THIS binary was compiled against, not the loaded library's: _lib.py compares the two)
    m.def("abi_version", []() { return std::string("street_crafter_amd 0.4.0 (gfx950) abi:" SC_ABI_HASH); });
    m.def("projection_fwd", &projection_fwd);
    m.def("projection_bwd", &projection_bwd);
    m.def("isect_bin_count", &isect_bin_count);
    m.def("isect_bin_sort", &isect_bin_sort);
    m.def("wait_i64", &wait_i64);
    m.def("sh_fwd", &sh_fwd);
    m.def("sh_bwd", &sh_bwd);
    m.def("rasterize_fwd", &rasterize_fwd);
    m.def("rasterize_fwd_planar", &rasterize_fwd_planar);
    m.def("rasterize_fwd_groups", &rasterize_fwd_groups);
    m.def("rasterize_fwd_layers", &rasterize_fwd_layers);
    m.def("rasterize_fwd_groups_ids", &rasterize_fwd_groups_ids);
    m.def("rasterize_bwd_groups", &rasterize_bwd_groups);
    m.def("rasterize_bwd", &rasterize_bwd);
    m.def("projection_autograd", &projection_autograd);
    m.def("sh_autograd", &sh_autograd);
    m.def("rasterize_autograd", &rasterize_autograd);
    m.def("projection_sh_fwd", &projection_sh_fwd);
    m.def("projection_sh_bwd", &projection_sh_bwd);
    m.def("rasterize_fwd_packed", &rasterize_fwd_packed);
    m.def("frame_composite_u8", &frame_composite_u8);
    m.def("frame_composite_u8_strided", &frame_composite_u8_strided);
    m.def("loss_fwd", &loss_fwd);
    m.def("loss_bwd", &loss_bwd);
    m.def("depth_trim_fwd", &depth_trim_fwd);
    m.def("depth_trim_bwd", &depth_trim_bwd);
    m.def("acc_reg_fwd", &acc_reg_fwd);
    m.def("acc_reg_bwd", &acc_reg_bwd);
    m.def("frame_tail_fwd", &frame_tail_fwd);
    m.def("frame_tail_bwd", &frame_tail_bwd);
    m.def("cubemap_fwd", &cubemap_fwd);
    m.def("cubemap_bwd", &cubemap_bwd);
    m.def("lpips_prep_fwd", &lpips_prep_fwd);
    m.def("lpips_prep_bwd", &lpips_prep_bwd);
    m.def("lpips_head_fwd", &lpips_head_fwd);
    m.def("lpips_head_bwd", &lpips_head_bwd);
    m.def("resize_fwd", &resize_fwd);
    m.def("resize_mask_fwd", &resize_mask_fwd);
    m.def("resize_bwd", &resize_bwd);
    m.def("adam_step", &adam_step);
    m.def("densify_stats", &densify_stats);
    m.def("compose_fwd", &compose_fwd);
    m.def("compose_bwd", &compose_bwd);
    m.def("densify_plan", &densify_plan);
    m.def("densify_apply", &densify_apply);
}
