// Visualizer frames on the GPU (include/street_crafter_amd.h, "visualizer frames"): the depth / squared-error colour
// maps of visualize_depth_numpy and the `* 255` uint8 casts of the reference's visualizer, so that a frame leaves the
// GPU as uint8 instead of float32.
//
// Two launches per frame.  viz_range_kernel streams the map(s) once and leaves one {min positive, max} pair per block
// (at most VIZ_MAX_BLOCKS of them per map) in the workspace; viz_u8_kernel lets every block reduce those pairs itself
// (<= 16 KB out of L2), stages the colour table(s) in LDS as one packed word per entry, and streams the maps again:
// 4 consecutive pixels per lane, 16-byte loads where the source is dense and aligned, 32-bit stores where the output is
// 4-byte aligned, scalar accesses with the same results otherwise and for the last n mod 4 pixels.
//
// All arithmetic is float32, one rounding per operation (viz_sub / viz_mul / viz_add / viz_div: no contraction, no
// reciprocal-multiply).  Minimum and maximum are taken on order-preserving integer images of the floats: exact in any order
// (deterministic without atomics) and independent of how the float min / max instructions treat denormals.
#include "sc_common.h"
#include <float.h>

// Contraction is switched off for the whole file.  __fmul_rn / __fadd_rn are NOT used: they are inline functions of a
// header compiled with the default contraction, and a product and a sum that come out of them are fused into one
// multiply-add after inlining (seen in this file's assembly).  The plain operators below carry no such permission.
#pragma clang fp contract(off)

namespace {
__device__ __forceinline__ float viz_add(float a, float b) { return a + b; }
__device__ __forceinline__ float viz_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float viz_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float viz_div(float a, float b) { return a / b; }     // correctly rounded (hipcc's default)

constexpr int VIZ_BLK = 256;
constexpr int VIZ_CHUNK = VIZ_BLK * 4;           // pixels a block takes per step
constexpr int VIZ_MAX_BLOCKS = 1024;             // block partials per map
constexpr uint32_t VIZ_NONE = 0x7f800000u;       // "no positive pixel": +inf, which nan_to_num never leaves in a map

inline int viz_blocks(int64_t n_pixels) {
    const int64_t chunks = (n_pixels + VIZ_CHUNK - 1) / VIZ_CHUNK;
    return (int)(chunks < VIZ_MAX_BLOCKS ? chunks : VIZ_MAX_BLOCKS);
}

struct VizSrc {                                  // the maps' sources, by value in the kernel arguments
    const float* depth; int64_t depth_stride;
    const float* rgb; int64_t rgb_pix, rgb_ch;
    const float* gt; int64_t gt_pix, gt_ch;
    const uint8_t* mask;
};

__device__ __forceinline__ bool viz_al(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// np.nan_to_num: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float viz_nan_to_num(float v) {
    const uint32_t b = __float_as_uint(v), m = b & 0x7fffffffu;
    if (m > 0x7f800000u) return 0.0f;
    if (m == 0x7f800000u) return __uint_as_float((b & 0x80000000u) | 0x7f7fffffu);
    return v;
}
// float order as unsigned order (-FLT_MAX < ... < -0 < +0 < denormals < ... < FLT_MAX)
__device__ __forceinline__ uint32_t viz_key(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float viz_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// (uint8) of a float as the x86 hosts of the reference do it: the low 8 bits of trunc(t); NaN / inf -> 0.  A float of
// magnitude >= 2^31 is a multiple of 256, so its low 8 bits are 0 without asking the conversion instruction.
__device__ __forceinline__ uint32_t viz_q(float t) {
    if (!(fabsf(t) < 2147483648.0f)) return 0u;
    return (uint32_t)((int)t) & 255u;
}

// the depth map's values of pixels [p, p + cnt), cnt in 1..4
__device__ __forceinline__ void viz_depth4(const VizSrc& s, bool vec, int64_t p, int cnt, float v[4]) {
    if (vec && cnt == 4) {
        const float4 t = *reinterpret_cast<const float4*>(s.depth + p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < cnt ? s.depth[(p + k) * s.depth_stride] : 0.0f;
    }
}

// the squared-error map's values: d_c = (m ? rgb_c : 0) - (m ? gt_c : 0), v = (d_0 d_0 + d_1 d_1) + d_2 d_2
__device__ __forceinline__ void viz_diff4(const VizSrc& s, bool vec, bool mask_vec, int64_t p, int cnt, float v[4]) {
    bool m[4];
    if (!s.mask) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = k < cnt;
    } else if (mask_vec && cnt == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(s.mask + p);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = ((w >> (8 * k)) & 255u) != 0u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = k < cnt && s.mask[p + k] != 0;
    }
    float a[3][4], b[3][4];
    if (vec && cnt == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 x = *reinterpret_cast<const float4*>(s.rgb + c * s.rgb_ch + p);
            const float4 y = *reinterpret_cast<const float4*>(s.gt + c * s.gt_ch + p);
            a[c][0] = x.x; a[c][1] = x.y; a[c][2] = x.z; a[c][3] = x.w;
            b[c][0] = y.x; b[c][1] = y.y; b[c][2] = y.z; b[c][3] = y.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a[c][k] = m[k] ? s.rgb[(p + k) * s.rgb_pix + c * s.rgb_ch] : 0.0f;
                b[c][k] = m[k] ? s.gt[(p + k) * s.gt_pix + c * s.gt_ch] : 0.0f;
            }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d0 = viz_sub(a[0][k], b[0][k]), d1 = viz_sub(a[1][k], b[1][k]), d2 = viz_sub(a[2][k], b[2][k]);
        const float sq = viz_add(viz_add(viz_mul(d0, d0), viz_mul(d1, d1)), viz_mul(d2, d2));
        v[k] = m[k] ? sq : 0.0f;
    }
}

__device__ __forceinline__ bool viz_depth_vec(const VizSrc& s) { return s.depth && s.depth_stride == 1 && viz_al(s.depth, 16); }
__device__ __forceinline__ bool viz_diff_vec(const VizSrc& s) {
    return s.rgb && s.rgb_pix == 1 && s.gt_pix == 1 && viz_al(s.rgb, 16) && viz_al(s.gt, 16) && (s.rgb_ch & 3) == 0 &&
           (s.gt_ch & 3) == 0;
}

// block-wide min of mn and max of mx, to every lane; sm: 8 words of LDS
__device__ __forceinline__ void viz_block_minmax(uint32_t& mn, uint32_t& mx, uint32_t* sm) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t a = __shfl_xor(mn, d, 64), b = __shfl_xor(mx, d, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    __syncthreads();                             // (sm may still be read from the previous call)
    const int w = (int)(threadIdx.x >> 6);
    if (sc_lane() == 0) { sm[w] = mn; sm[4 + w] = mx; }
    __syncthreads();
    mn = sm[0]; mx = sm[4];
#pragma unroll
    for (int i = 1; i < VIZ_BLK / 64; ++i) {
        mn = sm[i] < mn ? sm[i] : mn;
        mx = sm[4 + i] > mx ? sm[4 + i] : mx;
    }
}

// partials of map m: float2 {min positive or +inf, max} x n_blocks at workspace + m * VIZ_MAX_BLOCKS
__device__ __forceinline__ void viz_reduce_partials(const float2* part, int n_blocks, uint32_t* sm, float& mi, float& ma) {
    uint32_t mn = VIZ_NONE, mx = 0u;
    for (int i = (int)threadIdx.x; i < n_blocks; i += VIZ_BLK) {
        const float2 t = part[i];
        const uint32_t a = __float_as_uint(t.x), b = viz_key(t.y);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    viz_block_minmax(mn, mx, sm);
    mi = mn == VIZ_NONE ? 0.0f : __uint_as_float(mn);
    ma = viz_unkey(mx);
}

__global__ __launch_bounds__(VIZ_BLK) void viz_range_kernel(VizSrc s, int64_t n, float2* __restrict__ partials) {
    __shared__ uint32_t sm[8];
    const bool dvec = viz_depth_vec(s), fvec = viz_diff_vec(s), mvec = s.mask && viz_al(s.mask, 4);
    uint32_t mn[2] = {VIZ_NONE, VIZ_NONE}, mx[2] = {0u, 0u};
    const int64_t chunks = (n + VIZ_CHUNK - 1) / VIZ_CHUNK;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t p = c * VIZ_CHUNK + (int64_t)threadIdx.x * 4;
        if (p >= n) break;
        const int cnt = n - p < 4 ? (int)(n - p) : 4;
        float v[4];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if (m == 0 ? s.depth == nullptr : s.rgb == nullptr) continue;
            if (m == 0) viz_depth4(s, dvec, p, cnt, v); else viz_diff4(s, fvec, mvec, p, cnt, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= cnt) continue;
                const float x = viz_nan_to_num(v[k]);
                const uint32_t b = __float_as_uint(x), key = viz_key(x);
                if ((int32_t)b > 0 && b < mn[m]) mn[m] = b;          // x > 0 (denormals included): bit order = value order
                if (key > mx[m]) mx[m] = key;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (m == 0 ? s.depth == nullptr : s.rgb == nullptr) continue;
        viz_block_minmax(mn[m], mx[m], sm);
        if (threadIdx.x == 0)
            partials[m * VIZ_MAX_BLOCKS + blockIdx.x] = make_float2(__uint_as_float(mn[m]), viz_unkey(mx[m]));
    }
}

__global__ __launch_bounds__(VIZ_BLK) void viz_range_finish_kernel(const float2* __restrict__ partials, int n_blocks, int maps,
                                                                   float* __restrict__ range4) {
    __shared__ uint32_t sm[8];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        float mi = 0.0f, ma = 0.0f;
        if (maps & (1 << m)) viz_reduce_partials(partials + m * VIZ_MAX_BLOCKS, n_blocks, sm, mi, ma);
        if (threadIdx.x == 0) { range4[2 * m] = mi; range4[2 * m + 1] = ma; }
    }
}

// 12 bytes of four packed table entries (r | g << 8 | b << 16)
__device__ __forceinline__ void viz_store_rgb(uint8_t* out, bool vec, int64_t p, int cnt, const uint32_t c[4]) {
    if (vec && cnt == 4) {
        uint32_t* o = reinterpret_cast<uint32_t*>(out + p * 3);
        o[0] = c[0] | (c[1] << 24);
        o[1] = (c[1] >> 8) | (c[2] << 16);
        o[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
        for (int k = 0; k < cnt; ++k) {
            out[(p + k) * 3 + 0] = (uint8_t)(c[k] & 255u);
            out[(p + k) * 3 + 1] = (uint8_t)((c[k] >> 8) & 255u);
            out[(p + k) * 3 + 2] = (uint8_t)((c[k] >> 16) & 255u);
        }
    }
}

__device__ __forceinline__ void viz_gray(const float* a, uint8_t* out, int64_t p, int cnt) {
    if (cnt == 4 && viz_al(a, 16) && viz_al(out, 4)) {
        const float4 t = *reinterpret_cast<const float4*>(a + p);
        *reinterpret_cast<uint32_t*>(out + p) = viz_q(viz_mul(t.x, 255.0f)) | (viz_q(viz_mul(t.y, 255.0f)) << 8) |
                                                (viz_q(viz_mul(t.z, 255.0f)) << 16) | (viz_q(viz_mul(t.w, 255.0f)) << 24);
    } else {
        for (int k = 0; k < cnt; ++k) out[p + k] = (uint8_t)viz_q(viz_mul(a[p + k], 255.0f));
    }
}

__global__ __launch_bounds__(VIZ_BLK) void viz_u8_kernel(
    VizSrc s, const float* __restrict__ acc, const float* __restrict__ acc_object, int64_t n,
    const uint8_t* __restrict__ depth_lut, const uint8_t* __restrict__ diff_lut, const float* __restrict__ range4,
    const float2* __restrict__ partials, int n_partials, uint8_t* __restrict__ depth_u8, uint8_t* __restrict__ diff_u8,
    uint8_t* __restrict__ acc_u8, uint8_t* __restrict__ acc_object_u8) {
    __shared__ uint32_t lut[2][256];
    __shared__ uint32_t sm[8];
    const uint8_t* luts[2] = {depth_u8 ? depth_lut : nullptr, diff_u8 ? diff_lut : nullptr};
    float mi[2] = {0.0f, 0.0f}, den[2] = {1.0f, 1.0f};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        if (!luts[m]) continue;
        const uint8_t* t = luts[m] + 3 * threadIdx.x;
        lut[m][threadIdx.x] = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16);
        float ma;
        if (range4) { mi[m] = range4[2 * m]; ma = range4[2 * m + 1]; }
        else viz_reduce_partials(partials + m * VIZ_MAX_BLOCKS, n_partials, sm, mi[m], ma);
        den[m] = viz_add(viz_sub(ma, mi[m]), 1e-8f);
    }
    __syncthreads();
    const bool dvec = viz_depth_vec(s), fvec = viz_diff_vec(s), mvec = s.mask && viz_al(s.mask, 4);
    const bool o0vec = viz_al(depth_u8, 4), o1vec = viz_al(diff_u8, 4);
    const int64_t chunks = (n + VIZ_CHUNK - 1) / VIZ_CHUNK;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t p = c * VIZ_CHUNK + (int64_t)threadIdx.x * 4;
        if (p >= n) break;
        const int cnt = n - p < 4 ? (int)(n - p) : 4;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if (!luts[m]) continue;
            float v[4];
            uint32_t col[4];
            if (m == 0) viz_depth4(s, dvec, p, cnt, v); else viz_diff4(s, fvec, mvec, p, cnt, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = viz_nan_to_num(v[k]);
                col[k] = lut[m][viz_q(viz_mul(255.0f, viz_div(viz_sub(x, mi[m]), den[m])))];
            }
            viz_store_rgb(m == 0 ? depth_u8 : diff_u8, m == 0 ? o0vec : o1vec, p, cnt, col);
        }
        if (acc_u8) viz_gray(acc, acc_u8, p, cnt);
        if (acc_object_u8) viz_gray(acc_object, acc_object_u8, p, cnt);
    }
}

// argument checks shared by sc_frame_viz_range and sc_frame_viz_u8
int viz_check_src(const VizSrc& s, int64_t n_pixels) {
    if (n_pixels < 0 || n_pixels >= ((int64_t)1 << 31)) return SC_EINVAL;
    if (s.depth_stride < 0 || s.rgb_pix < 0 || s.rgb_ch < 0 || s.gt_pix < 0 || s.gt_ch < 0) return SC_EINVAL;
    if ((s.rgb != nullptr) != (s.gt != nullptr)) return SC_EINVAL;          // a diff source given only in part
    if (s.mask && !s.rgb) return SC_EINVAL;
    return SC_OK;
}
}  // namespace

extern "C" size_t sc_frame_viz_workspace_bytes(void) { return (size_t)2 * VIZ_MAX_BLOCKS * sizeof(float2); }

extern "C" int sc_frame_viz_range(const float* depth, int64_t depth_stride, const float* rgb, int64_t rgb_pix_stride,
                                  int64_t rgb_ch_stride, const float* gt, int64_t gt_pix_stride, int64_t gt_ch_stride,
                                  const uint8_t* mask, int64_t n_pixels, void* workspace, size_t workspace_bytes,
                                  sc_stream_t stream) {
    const VizSrc s{depth, depth_stride, rgb, rgb_pix_stride, rgb_ch_stride, gt, gt_pix_stride, gt_ch_stride, mask};
    if (viz_check_src(s, n_pixels) != SC_OK) return SC_EINVAL;
    if (n_pixels == 0) return SC_OK;
    if ((!depth && !rgb) || !workspace) return SC_EINVAL;
    if (workspace_bytes < sc_frame_viz_workspace_bytes()) return SC_EWORKSPACE;
    hipLaunchKernelGGL(viz_range_kernel, dim3((unsigned)viz_blocks(n_pixels)), dim3(VIZ_BLK), 0, sc_s(stream), s, n_pixels,
                       reinterpret_cast<float2*>(workspace));
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_frame_viz_range_finish(const void* workspace, size_t workspace_bytes, int64_t n_pixels, int maps,
                                         float* range4, sc_stream_t stream) {
    if (n_pixels < 0 || n_pixels >= ((int64_t)1 << 31) || maps < 1 || maps > 3) return SC_EINVAL;
    if (n_pixels == 0) return SC_OK;
    if (!workspace || !range4) return SC_EINVAL;
    if (workspace_bytes < sc_frame_viz_workspace_bytes()) return SC_EWORKSPACE;
    hipLaunchKernelGGL(viz_range_finish_kernel, dim3(1), dim3(VIZ_BLK), 0, sc_s(stream),
                       reinterpret_cast<const float2*>(workspace), viz_blocks(n_pixels), maps, range4);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_frame_viz_u8(const float* depth, int64_t depth_stride, const float* rgb, int64_t rgb_pix_stride,
                               int64_t rgb_ch_stride, const float* gt, int64_t gt_pix_stride, int64_t gt_ch_stride,
                               const uint8_t* mask, const float* acc, const float* acc_object, int64_t n_pixels,
                               const uint8_t* depth_lut, const uint8_t* diff_lut, const float* range4,
                               const void* workspace, size_t workspace_bytes, uint8_t* depth_u8, uint8_t* diff_u8,
                               uint8_t* acc_u8, uint8_t* acc_object_u8, sc_stream_t stream) {
    const VizSrc s{depth, depth_stride, rgb, rgb_pix_stride, rgb_ch_stride, gt, gt_pix_stride, gt_ch_stride, mask};
    if (viz_check_src(s, n_pixels) != SC_OK) return SC_EINVAL;
    if (!depth_u8 && !diff_u8 && !acc_u8 && !acc_object_u8) return SC_EINVAL;         // no output requested
    if ((depth_u8 && (!depth || !depth_lut)) || (diff_u8 && (!rgb || !diff_lut))) return SC_EINVAL;
    if ((acc_u8 && !acc) || (acc_object_u8 && !acc_object)) return SC_EINVAL;
    if ((depth_u8 || diff_u8) && !range4) {
        if (!workspace) return SC_EINVAL;
        if (workspace_bytes < sc_frame_viz_workspace_bytes()) return SC_EWORKSPACE;
    }
    if (n_pixels == 0) return SC_OK;
    hipLaunchKernelGGL(viz_u8_kernel, dim3((unsigned)viz_blocks(n_pixels)), dim3(VIZ_BLK), 0, sc_s(stream), s, acc,
                       acc_object, n_pixels, depth_lut, diff_lut, range4, reinterpret_cast<const float2*>(workspace),
                       viz_blocks(n_pixels), depth_u8, diff_u8, acc_u8, acc_object_u8);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
