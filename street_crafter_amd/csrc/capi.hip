// Library-level entry points of the C ABI (include/street_crafter_amd.h).
#include "raster_common.h"
#include <stdlib.h>
#include <string.h>
#include <time.h>

// SC_ABI_HASH: a digest of include/street_crafter_amd.h, handed to BOTH binaries by build.py (this library and the binding
// layer, csrc/binding.cpp): a binding layer compiled against another edition of the header than the library beside it
// (signatures!) refuses to load (_lib.py) instead of calling through stale prototypes.
#ifndef SC_ABI_HASH
#define SC_ABI_HASH "unhashed"
#endif
#ifdef SC_DIAG
extern "C" const char* sc_version(void) { return "street_crafter_amd 0.4.0 (gfx950, DIAGNOSTIC build) abi:" SC_ABI_HASH; }
#else
extern "C" const char* sc_version(void) { return "street_crafter_amd 0.4.0 (gfx950) abi:" SC_ABI_HASH; }
#endif

extern "C" const char* sc_target_arch(void) { return "gfx950"; }

extern "C" const char* sc_error_string(int code) {
    switch (code) {
        case SC_OK: return "ok";
        case SC_EINVAL: return "street_crafter_amd: invalid argument (size / null pointer / unsupported parameter)";
        case SC_EWORKSPACE: return "street_crafter_amd: workspace too small";
        case SC_EUNSUPPORTED: return "street_crafter_amd: unsupported configuration";
        default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "street_crafter_amd: unknown error";
}

#ifdef SC_DIAG
int g_sc_debug[4] = {0, 0, 0, 0};       // diagnostic build only (sc_common.h)
#endif
int g_sc_proj_clamp = 0;        // sc_set_option "proj_clamp" (projection_common.h)
int g_sc_radius_floor = 0;      // sc_set_option "radius_floor"
extern int g_sc_point_raster_waves;     // sc_set_option "point_raster_waves" (point_raster.hip)

// Host-side wait for the sequence number that center_scatter_kernel publishes behind the frame's sizes
// (host-mapped pinned memory, include/street_crafter_amd.h sc_isect_bin_count).  A plain spin in C: a Python host
// calls it through ctypes.CDLL, which releases the GIL for the duration, so a second host thread (the other frame
// in flight) keeps launching while this one waits for its counts.
extern "C" int sc_wait_i64(const int64_t* addr, int64_t value, int64_t timeout_us) {
    if (!addr) return SC_EINVAL;
    struct timespec t0;
    bool have_t0 = false;
    for (unsigned spins = 1;; ++spins) {
        if (__atomic_load_n(addr, __ATOMIC_ACQUIRE) == value) return SC_OK;
        __builtin_ia32_pause();
        if ((spins & 1023u) == 0) {
            struct timespec now;
            clock_gettime(CLOCK_MONOTONIC, &now);
            if (!have_t0) { t0 = now; have_t0 = true; }
            const int64_t us = (int64_t)(now.tv_sec - t0.tv_sec) * 1000000 + (now.tv_nsec - t0.tv_nsec) / 1000;
            if (timeout_us >= 0 && us > timeout_us) return 1;       // timed out (not an error code of the library)
        }
    }
}

extern "C" int sc_stream_create(int priority, const uint32_t* cu_mask, int n_mask_words, sc_stream_t* out) {
    if (!out || n_mask_words < 0 || (n_mask_words > 0 && !cu_mask)) return SC_EINVAL;
    hipStream_t s = nullptr;
    if (n_mask_words > 0) {
        bool any = false;
        for (int i = 0; i < n_mask_words; ++i) any = any || cu_mask[i] != 0u;
        if (!any) return SC_EINVAL;                      // an empty mask would hang the first launch
        SC_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)n_mask_words, cu_mask));
    } else {
        SC_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
    }
    *out = (sc_stream_t)s;
    return SC_OK;
}

extern "C" int sc_stream_destroy(sc_stream_t stream) {
    if (!stream) return SC_EINVAL;
    SC_HIP(hipStreamDestroy(sc_s(stream)));
    return SC_OK;
}

extern "C" int sc_stream_priority_range(int* least, int* greatest) {
    if (!least || !greatest) return SC_EINVAL;
    SC_HIP(hipDeviceGetStreamPriorityRange(least, greatest));
    return SC_OK;
}

extern "C" int sc_set_option(const char* key, int value) {
    if (!key) return SC_EINVAL;
#ifdef SC_DIAG     // "debug0".."debug3" exist in the diagnostic build only: the shipped library answers SC_EINVAL
    if (strncmp(key, "debug", 5) == 0 && key[5] >= '0' && key[5] <= '3' && key[6] == 0) {
        if (value < 0) return SC_EINVAL;
        const int prev = g_sc_debug[key[5] - '0'];
        g_sc_debug[key[5] - '0'] = value;
        return prev;
    }
#endif
    if (strcmp(key, "raster_bwd") == 0) {
        if (value < 0 || value > 1) return SC_EINVAL;
        const int prev = g_sc_raster_bwd_variant;
        g_sc_raster_bwd_variant = value;
        return prev;
    }
    if (strcmp(key, "raster_bwd_split") == 0) {
        if (value < 0 || value > 1) return SC_EINVAL;
        const int prev = g_sc_raster_bwd_split;
        g_sc_raster_bwd_split = value;
        return prev;
    }
    if (strcmp(key, "raster_map") == 0) {
        if (value < 0 || value > 1) return SC_EINVAL;
        const int prev = g_sc_raster_map;
        g_sc_raster_map = value;
        return prev;
    }
    if (strcmp(key, "raster_hint_blend") == 0) {
        if (value < 0 || value > 4) return SC_EINVAL;
        const int prev = g_sc_raster_hint_blend;
        g_sc_raster_hint_blend = value;
        return prev;
    }
    if (strcmp(key, "raster_split") == 0) {
        if (value < 0 || value > 100) return SC_EINVAL;
        const int prev = g_sc_raster_split;
        g_sc_raster_split = value;
        return prev;
    }
    if (strcmp(key, "proj_clamp") == 0) {
        if (value < 0 || value > 1) return SC_EINVAL;
        const int prev = g_sc_proj_clamp;
        g_sc_proj_clamp = value;
        return prev;
    }
    if (strcmp(key, "radius_floor") == 0) {
        if (value < 0 || value > 1) return SC_EINVAL;
        const int prev = g_sc_radius_floor;
        g_sc_radius_floor = value;
        return prev;
    }
    if (strcmp(key, "point_raster_waves") == 0) {
        if (value != 1 && value != 4) return SC_EINVAL;
        const int prev = g_sc_point_raster_waves;
        g_sc_point_raster_waves = value;
        return prev;
    }
    if (strcmp(key, "raster_fwd") == 0) {
        if (value != 0 && value != 3) return SC_EINVAL;
        const int prev = g_sc_raster_fwd_variant;
        g_sc_raster_fwd_variant = value;
        return prev;
    }
    return SC_EINVAL;
}

// ---- frame export used by the multi-GPU gather (street_crafter_amd/dist.py) ---------------------
// The tail of render_novel_view (street_gaussian_renderer.py:151-163) plus the visualizer's uint8
// conversion, as ONE pass over the frame:
//     rgb = clamp(clamp(fg, 0, 1) + clamp(sky, 0, 1) * (1 - acc), 0, 1)     (sky / acc optional)
//     u8  = (uint8)(rgb * 255)          rounding 0: the video frames, (rgb * 255).astype(np.uint8)
//                                       (street_gaussian_visualizer.py:97, base_visualizer.py:37)
//     u8  = (uint8)(rgb * 255 + 0.5)    rounding 1: torchvision.utils.save_image's PNGs
// fg / sky are the rasterizer's raw [H,W,C>=3] images (the per-pass clamp of renderer.py:290-291 is
// folded in).  Every product / sum is a separately rounded fp32 op, so the result is bit-identical to
// the torch composition the reference spells out.
namespace {
__global__ __launch_bounds__(256) void frame_composite_u8_kernel(
    const float* __restrict__ fg, int64_t fg_stride, int64_t fg_ch, const float* __restrict__ acc,
    const float* __restrict__ sky, int64_t sky_stride, int64_t sky_ch, int64_t n_pix, int rounding,
    uint8_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pix) return;
    const float* p = fg + i * fg_stride;
    const float* q = sky ? sky + i * sky_stride : nullptr;
    const float keep = sky ? __fsub_rn(1.0f, acc[i]) : 0.0f;
    const float bias = rounding ? 0.5f : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = fminf(fmaxf(p[c * fg_ch], 0.0f), 1.0f);
        if (sky) {
            const float s = fminf(fmaxf(q[c * sky_ch], 0.0f), 1.0f);
            v = fminf(fmaxf(__fadd_rn(v, __fmul_rn(s, keep)), 0.0f), 1.0f);
        }
        dst[i * 3 + c] = (uint8_t)__fadd_rn(__fmul_rn(v, 255.0f), bias);
    }
}
}  // namespace

extern "C" int sc_frame_composite_u8(const float* fg, int fg_stride, const float* acc, const float* sky,
                                     int sky_stride, int64_t n_pixels, int rounding, uint8_t* out,
                                     sc_stream_t stream) {
    if (n_pixels < 0 || fg_stride < 3 || (sky && sky_stride < 3) || (rounding != 0 && rounding != 1)) return SC_EINVAL;
    if ((sky != nullptr) != (acc != nullptr)) return SC_EINVAL;
    if (n_pixels == 0) return SC_OK;
    if (!fg || !out) return SC_EINVAL;
    hipLaunchKernelGGL(frame_composite_u8_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0,
                       sc_s(stream), fg, (int64_t)fg_stride, (int64_t)1, acc, sky, (int64_t)sky_stride, (int64_t)1, n_pixels,
                       rounding, out);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

// The same with a channel stride: images stored as planes (sc_rasterize_fwd_planar: pixel stride 1, channel stride H * W).
extern "C" int sc_frame_composite_u8_strided(const float* fg, int64_t fg_pix_stride, int64_t fg_ch_stride, const float* acc,
                                             const float* sky, int64_t sky_pix_stride, int64_t sky_ch_stride,
                                             int64_t n_pixels, int rounding, uint8_t* out, sc_stream_t stream) {
    if (n_pixels < 0 || fg_pix_stride < 1 || fg_ch_stride < 1 || (rounding != 0 && rounding != 1)) return SC_EINVAL;
    if (sky && (sky_pix_stride < 1 || sky_ch_stride < 1)) return SC_EINVAL;
    if ((sky != nullptr) != (acc != nullptr)) return SC_EINVAL;
    if (n_pixels == 0) return SC_OK;
    if (!fg || !out) return SC_EINVAL;
    hipLaunchKernelGGL(frame_composite_u8_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0,
                       sc_s(stream), fg, fg_pix_stride, fg_ch_stride, acc, sky, sky_pix_stride, sky_ch_stride, n_pixels,
                       rounding, out);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

// ---- sky cube map (csrc/cubemap.hip) --------------------------------------------------------------------------
int sc_cubemap_run(const float* tex, int resolution, int channels, const float* dirs, const float* ray_matrix_host,
                   const float* perturb, const uint8_t* mask, const float* acc, int64_t n, int width, int flags, float fill,
                   float* out, const float* grad_out, float* grad_tex, sc_stream_t stream);

static int cubemap_check(const float* tex, int resolution, int channels, const float* dirs, const float* ray_matrix_host,
                         const float* perturb, const uint8_t* mask, const float* acc, int64_t n, int width, int flags) {
    if (resolution < 2 || resolution > 16384 || channels < 1 || channels > 4) return SC_EINVAL;
    if (n < 0 || n >= ((int64_t)1 << 38)) return SC_EINVAL;
    if (flags & ~(SC_CUBE_SIGMOID | SC_CUBE_CLAMP | SC_CUBE_PLANAR)) return SC_EINVAL;
    if ((dirs != nullptr) == (ray_matrix_host != nullptr)) return SC_EINVAL;
    if (perturb && !ray_matrix_host) return SC_EINVAL;
    if (ray_matrix_host && (width <= 0 || n % width != 0)) return SC_EINVAL;
    if (mask && acc) return SC_EINVAL;
    if (!tex) return SC_EINVAL;
    return SC_OK;
}

extern "C" int sc_cubemap_fwd(const float* tex, int resolution, int channels, const float* dirs,
                              const float* ray_matrix_host, const float* perturb, const uint8_t* mask, const float* acc,
                              int64_t n, int width, int flags, float fill, float* out, sc_stream_t stream) {
    const int rc = cubemap_check(tex, resolution, channels, dirs, ray_matrix_host, perturb, mask, acc, n, width, flags);
    if (rc != SC_OK) return rc;
    if (n == 0) return SC_OK;
    if (!out) return SC_EINVAL;
    return sc_cubemap_run(tex, resolution, channels, dirs, ray_matrix_host, perturb, mask, acc, n, width, flags, fill, out,
                          nullptr, nullptr, stream);
}

extern "C" int sc_cubemap_bwd(const float* tex, int resolution, int channels, const float* dirs,
                              const float* ray_matrix_host, const float* perturb, const uint8_t* mask, const float* acc,
                              int64_t n, int width, int flags, float fill, const float* grad_out, float* grad_tex,
                              sc_stream_t stream) {
    const int rc = cubemap_check(tex, resolution, channels, dirs, ray_matrix_host, perturb, mask, acc, n, width, flags);
    if (rc != SC_OK) return rc;
    if (!grad_tex || (n > 0 && !grad_out)) return SC_EINVAL;
    return sc_cubemap_run(tex, resolution, channels, dirs, ray_matrix_host, perturb, mask, acc, n, width, flags, fill,
                          nullptr, grad_out, grad_tex, stream);
}

// ---- the head of a frame (csrc/compose.hip) -----------------------------------------------------------------------
int sc_compose_fwd_run(const sc_compose_segment* segments_host, int n_segments, int K, const float* obj_rots,
                       const float* obj_trans, const float* flip_q_host, float* means, float* quats, float* scales,
                       float* opacities, float* sh, sc_stream_t stream);
int sc_compose_bwd_run(const sc_compose_segment* segments_host, const sc_compose_grads* grads_host, int n_segments, int K,
                       const float* obj_rots, const float* obj_trans, int A, const float* flip_q_host,
                       const float* g_means, const float* g_quats, const float* g_scales, const float* g_opacities,
                       const float* g_sh, float* grad_obj_rots, float* grad_obj_trans, sc_stream_t stream);

static int compose_check(const sc_compose_segment* seg, const sc_compose_grads* grads, bool want_grads, int n_segments,
                         int64_t N, int K, const float* obj_rots, const float* obj_trans, int A,
                         const float* flip_q_host) {
    if (n_segments < 0 || N < 0 || A < 0 || K < 1) return SC_EINVAL;
    if (n_segments > 0 && (seg == nullptr || (want_grads && grads == nullptr))) return SC_EINVAL;
    int64_t at = 0;
    for (int i = 0; i < n_segments; ++i) {
        const sc_compose_segment& s = seg[i];
        if (s.start != at || s.start > s.end) return SC_EINVAL;                     // in order, without gaps
        at = s.end;
        if (s.kind != SC_COMPOSE_STATIC && s.kind != SC_COMPOSE_ACTOR && s.kind != SC_COMPOSE_SKY) return SC_EINVAL;
        if (s.fourier_dim < 1 || s.fourier_dim > SC_COMPOSE_MAX_FOURIER) return SC_EINVAL;
        if (s.kind == SC_COMPOSE_ACTOR && (s.pose_row < 0 || s.pose_row >= A)) return SC_EINVAL;
        if (s.end == s.start) continue;
        if (!s.xyz || !s.scaling || !s.rotation || !s.opacity || !s.features_dc || (K > 1 && !s.features_rest))
            return SC_EINVAL;
        if (s.kind == SC_COMPOSE_ACTOR && (!obj_rots || !obj_trans || (s.flip && !flip_q_host))) return SC_EINVAL;
        if (want_grads) {
            const sc_compose_grads& g = grads[i];
            if (!g.xyz || !g.scaling || !g.rotation || !g.opacity || !g.features_dc || (K > 1 && !g.features_rest))
                return SC_EINVAL;
        }
    }
    if (at != N) return SC_EINVAL;
    return SC_OK;
}

extern "C" int sc_compose_fwd(const sc_compose_segment* segments_host, int n_segments, int64_t N, int K,
                              const float* obj_rots, const float* obj_trans, int A, const float* flip_q_host,
                              float* means, float* quats, float* scales, float* opacities, float* sh,
                              sc_stream_t stream) {
    const int rc = compose_check(segments_host, nullptr, false, n_segments, N, K, obj_rots, obj_trans, A, flip_q_host);
    if (rc != SC_OK) return rc;
    if (N == 0) return SC_OK;
    if (!means || !quats || !scales || !opacities || !sh) return SC_EINVAL;
    return sc_compose_fwd_run(segments_host, n_segments, K, obj_rots, obj_trans, flip_q_host, means, quats, scales,
                              opacities, sh, stream);
}

extern "C" int sc_compose_bwd(const sc_compose_segment* segments_host, const sc_compose_grads* grads_host, int n_segments,
                              int64_t N, int K, const float* obj_rots, const float* obj_trans, int A,
                              const float* flip_q_host, const float* g_means, const float* g_quats,
                              const float* g_scales, const float* g_opacities, const float* g_sh, float* grad_obj_rots,
                              float* grad_obj_trans, sc_stream_t stream) {
    const int rc = compose_check(segments_host, grads_host, true, n_segments, N, K, obj_rots, obj_trans, A, flip_q_host);
    if (rc != SC_OK) return rc;
    if (N == 0) return SC_OK;
    return sc_compose_bwd_run(segments_host, grads_host, n_segments, K, obj_rots, obj_trans, A, flip_q_host, g_means,
                              g_quats, g_scales, g_opacities, g_sh, grad_obj_rots, grad_obj_trans, stream);
}

// ---- the actor poses of a frame (csrc/actor_pose.hip) -----------------------------------------------------------------
int sc_actor_poses_fwd_run(const sc_actor_pose_item* items_host, int A, const float* input_trans, const float* input_rots,
                           const float* opt_trans, const float* opt_rots, float* obj_rots, float* obj_trans,
                           sc_stream_t stream);
int sc_actor_poses_bwd_run(const sc_actor_pose_item* items_host, int A, int64_t rows, const float* input_rots,
                           const float* opt_rots, const float* g_obj_rots, const float* g_obj_trans, float* grad_opt_trans,
                           float* grad_opt_rots, sc_stream_t stream);

// the table alone: sizes, flag bits, every row an item uses; *any_delta / *any_interp: what the caller's pointers must cover
static int actor_items_check(const sc_actor_pose_item* items, int A, int64_t rows, bool* any_delta, bool* any_interp) {
    *any_delta = *any_interp = false;
    if (A < 0 || rows < 0) return SC_EINVAL;
    if (A > 0 && items == nullptr) return SC_EINVAL;
    auto inside = [rows](int32_t r) { return r >= 0 && (int64_t)r < rows; };
    for (int i = 0; i < A; ++i) {
        const sc_actor_pose_item& it = items[i];
        if (it.flags & ~(SC_POSE_DELTA | SC_POSE_INTERP)) return SC_EINVAL;
        if (it.flags & SC_POSE_INTERP) {
            if (!inside(it.row_prev) || !inside(it.row_next)) return SC_EINVAL;
            *any_interp = true;
        } else if (!inside(it.row)) {
            return SC_EINVAL;
        }
        if (it.flags & SC_POSE_DELTA) *any_delta = true;
    }
    return SC_OK;
}

extern "C" int sc_actor_poses_fwd(const sc_actor_pose_item* items_host, int A, int64_t rows, const float* input_trans,
                                  const float* input_rots, const float* opt_trans, const float* opt_rots, float* obj_rots,
                                  float* obj_trans, sc_stream_t stream) {
    bool any_delta, any_interp;
    const int rc = actor_items_check(items_host, A, rows, &any_delta, &any_interp);
    if (rc != SC_OK) return rc;
    if (A == 0) return SC_OK;
    if (!input_trans || !input_rots || !obj_rots || !obj_trans) return SC_EINVAL;
    if (any_delta && (!opt_trans || !opt_rots)) return SC_EINVAL;
    return sc_actor_poses_fwd_run(items_host, A, input_trans, input_rots, opt_trans, opt_rots, obj_rots, obj_trans, stream);
}

extern "C" int sc_actor_poses_bwd(const sc_actor_pose_item* items_host, int A, int64_t rows, const float* input_rots,
                                  const float* opt_rots, const float* g_obj_rots, const float* g_obj_trans,
                                  float* grad_opt_trans, float* grad_opt_rots, sc_stream_t stream) {
    bool any_delta, any_interp;
    const int rc = actor_items_check(items_host, A, rows, &any_delta, &any_interp);
    if (rc != SC_OK) return rc;
    if (A == 0) return SC_OK;
    if (any_interp) return SC_EUNSUPPORTED;                 // no gradient through interpolated rows
    if (any_delta && grad_opt_rots && (!input_rots || !opt_rots)) return SC_EINVAL;
    if (any_delta) {                                        // plain stores: the rows must be distinct
        int32_t* seen = (int32_t*)malloc(sizeof(int32_t) * (size_t)A);
        if (!seen) return (int)hipErrorOutOfMemory;
        int n = 0;
        for (int i = 0; i < A; ++i)
            if (items_host[i].flags & SC_POSE_DELTA) seen[n++] = items_host[i].row;
        qsort(seen, (size_t)n, sizeof(int32_t), [](const void* x, const void* y) {
            const int32_t a = *(const int32_t*)x, b = *(const int32_t*)y;
            return a < b ? -1 : (a > b ? 1 : 0);
        });
        bool twice = false;
        for (int i = 1; i < n; ++i) twice = twice || seen[i] == seen[i - 1];
        free(seen);
        if (twice) return SC_EINVAL;
    }
    return sc_actor_poses_bwd_run(items_host, A, rows, input_rots, opt_rots, g_obj_rots, g_obj_trans, grad_opt_trans,
                                  grad_opt_rots, stream);
}

// ---- crop + resize of the novel-view training inputs (csrc/resize.hip) ------------------------------------------
int sc_resize_fwd_run(const float* x, const uint8_t* x_mask, const int64_t* strides, int batch, int channels, int in_h,
                      int in_w, const int32_t* ty_idx, const float* ty_w, const int32_t* tx_idx, const float* tx_w,
                      int h_out, int w_out, int row_begin, int flags, float a, float b, float* out, uint8_t* out_mask,
                      sc_stream_t stream);
int sc_resize_bwd_run(const float* grad_out, int batch, int channels, int height, int width, int top, int left, int in_h,
                      int in_w, const int32_t* uy_idx, const float* uy_w, const int32_t* ux_idx, const float* ux_w,
                      int h_out, int w_out, int row_begin, int flags, float a, float* grad_x, sc_stream_t stream);

constexpr int RESIZE_MAX_SIDE = 1 << 16;     // rows go four to a workgroup on gridDim.y
constexpr int RESIZE_MAX_PLANES = 65535;     // batch * channels on gridDim.z

static int resize_sizes_check(int batch, int channels, int in_h, int in_w, int h_out, int w_out, int row_begin) {
    if (batch <= 0 || channels <= 0 || (int64_t)batch * channels > RESIZE_MAX_PLANES) return SC_EINVAL;
    if (in_h <= 0 || in_w <= 0 || h_out <= 0 || w_out <= 0) return SC_EINVAL;
    if (in_h > RESIZE_MAX_SIDE || in_w > RESIZE_MAX_SIDE || h_out > RESIZE_MAX_SIDE || w_out > RESIZE_MAX_SIDE) return SC_EINVAL;
    if (row_begin < 0 || row_begin >= h_out) return SC_EINVAL;
    return SC_OK;
}

static int resize_strides_check(const int64_t* strides_host) {
    if (!strides_host) return SC_EINVAL;
    for (int k = 0; k < 4; ++k)
        if (strides_host[k] < 0) return SC_EINVAL;
    return SC_OK;
}

extern "C" int sc_resize_fwd(const float* x, const int64_t* strides_host, int batch, int channels, int in_h, int in_w,
                             const int32_t* ty_idx, const float* ty_w, const int32_t* tx_idx, const float* tx_w, int h_out,
                             int w_out, int row_begin, int flags, float a, float b, float* out, sc_stream_t stream) {
    int rc = resize_sizes_check(batch, channels, in_h, in_w, h_out, w_out, row_begin);
    if (rc == SC_OK) rc = resize_strides_check(strides_host);
    if (rc != SC_OK) return rc;
    if (flags & ~(SC_RESIZE_AFFINE | SC_RESIZE_PACKED4)) return SC_EINVAL;
    if (!x || !ty_idx || !ty_w || !tx_idx || !tx_w || !out) return SC_EINVAL;
    if (flags & SC_RESIZE_PACKED4) {
        const bool ok = channels <= 4 && strides_host[1] == 1 && strides_host[3] == 4 && strides_host[0] % 4 == 0 &&
                        strides_host[2] % 4 == 0 && ((uintptr_t)x & 15u) == 0;
        if (!ok) return SC_EINVAL;
    }
    return sc_resize_fwd_run(x, nullptr, strides_host, batch, channels, in_h, in_w, ty_idx, ty_w, tx_idx, tx_w, h_out, w_out,
                             row_begin, flags, a, b, out, nullptr, stream);
}

extern "C" int sc_resize_mask_fwd(const uint8_t* x, const int64_t* strides_host, int batch, int channels, int in_h, int in_w,
                                  const int32_t* ty_idx, const int32_t* tx_idx, int h_out, int w_out, int row_begin,
                                  uint8_t* out, sc_stream_t stream) {
    int rc = resize_sizes_check(batch, channels, in_h, in_w, h_out, w_out, row_begin);
    if (rc == SC_OK) rc = resize_strides_check(strides_host);
    if (rc != SC_OK) return rc;
    if (!x || !ty_idx || !tx_idx || !out) return SC_EINVAL;
    return sc_resize_fwd_run(nullptr, x, strides_host, batch, channels, in_h, in_w, ty_idx, nullptr, tx_idx, nullptr, h_out,
                             w_out, row_begin, 0, 1.0f, 0.0f, nullptr, out, stream);
}

extern "C" int sc_resize_bwd(const float* grad_out, int batch, int channels, int height, int width, int top, int left,
                             int in_h, int in_w, const int32_t* uy_idx, const float* uy_w, const int32_t* ux_idx,
                             const float* ux_w, int h_out, int w_out, int row_begin, int flags, float a, float* grad_x,
                             sc_stream_t stream) {
    const int rc = resize_sizes_check(batch, channels, in_h, in_w, h_out, w_out, row_begin);
    if (rc != SC_OK) return rc;
    if (height <= 0 || width <= 0 || height > RESIZE_MAX_SIDE || width > RESIZE_MAX_SIDE) return SC_EINVAL;
    if (top < 0 || left < 0 || top > height - in_h || left > width - in_w) return SC_EINVAL;
    if (flags & ~SC_RESIZE_AFFINE) return SC_EINVAL;
    if (!grad_out || !uy_idx || !uy_w || !ux_idx || !ux_w || !grad_x) return SC_EINVAL;
    return sc_resize_bwd_run(grad_out, batch, channels, height, width, top, left, in_h, in_w, uy_idx, uy_w, ux_idx, ux_w,
                             h_out, w_out, row_begin, flags, a, grad_x, stream);
}
