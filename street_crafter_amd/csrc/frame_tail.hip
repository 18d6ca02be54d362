// The pixel-wise tail of a training frame between the rasterizer and the losses (street_gaussian_renderer.py:282-300,
// :116-132, color_correction.py:135-138): depth = c_3 / max(a, 1e-10), the sky composite, the colour-correction affine
// and the permute to planes, as ONE launch forward and ONE launch (plus a one-block finishing stage for the affine's
// twelve sums) backward.  The formulas and their evaluation order are in include/street_crafter_amd.h.
//
// Shape.  A lane takes FT_PPL = 4 consecutive pixels: render_colors with D == 4 is four 16-byte loads, with D == 3
// three; render_alphas, every plane of rgb / depth / the upstream gradients one 16-byte access each.  A lane falls back
// to scalar accesses for an array whose address is not 16-byte aligned (a view with a storage offset; planes 1 and 2
// when H*W is not a multiple of 4) and for the last H*W mod 4 pixels.  The forward runs one such group per lane
// (FT_NT * FT_PPL = 1024 pixels per block); the backward FT_BWD_PASSES = 4 groups, FT_NT * FT_PPL pixels apart
// (4096 pixels per block), so that a lane adds at most 16 pixels into its twelve partial sums.
//
// The twelve sums.  No float atomics: lane-serial fp32 over its <= 16 pixels, a butterfly over the wave (6 levels) and
// over the block's 4 waves (2 levels), one ordinary store of 12 floats per block; frame_tail_finish_kernel adds the
// block partials in float64 (lane t takes blocks t, t + 256, ...; the same butterfly in float64) and rounds once.
#include "sc_common.h"

// Every product, sum and quotient below is rounded on its own.  hipcc contracts a * b + c into an FMA by default, and
// it does so through __fmul_rn / __fadd_rn as well (plain operators inside header functions that are compiled with
// contraction on, fused after inlining): the four operations are spelled here, under contract(off).  The fp32 quotient
// is hipcc's correctly rounded division.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float ft_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float ft_add(float a, float b) { return a + b; }
__device__ __forceinline__ float ft_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float ft_div(float a, float b) { return a / b; }

constexpr int FT_NT = 256;                                  // lanes per block
constexpr int FT_PPL = 4;                                    // consecutive pixels per lane and pass
constexpr int FT_GROUP = FT_NT * FT_PPL;                     // pixels per block and pass
constexpr int FT_BWD_PASSES = 4;                             // 16 pixels per lane
constexpr int FT_BWD_CHUNK = FT_GROUP * FT_BWD_PASSES;       // pixels per backward block
constexpr float FT_AMIN = 1e-10f;

enum { FT_SKY_NONE = 0, FT_SKY_PIX4 = 1, FT_SKY_PIX3 = 2, FT_SKY_PLANES = 3, FT_SKY_STRIDED = 4 };

struct FtSky {
    const float* p;
    int64_t sc, sh, sw;      // channel, row, column strides in elements (FT_SKY_STRIDED reads through all three)
    int mode;
};

__device__ __forceinline__ bool ft_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
__device__ __forceinline__ float ft_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }   // NaN stays NaN
__device__ __forceinline__ float ft_amax(float a) { return a < FT_AMIN ? FT_AMIN : a; }                      // clamp(min=)

// n pixels (1..4) of one plane starting at q: one 16-byte access when all four are there and q is aligned
__device__ __forceinline__ void ft_load_plane(const float* q, int n, float (&v)[4]) {
    if (n == 4 && ft_al16(q)) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < n ? q[k] : 0.0f;
    }
}
__device__ __forceinline__ void ft_store_plane(float* q, int n, const float (&v)[4]) {
    if (n == 4 && ft_al16(q)) {
        *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) q[k] = v[k];
    }
}

// n pixels of an interleaved image with 3 or 4 channels per pixel, dense, starting at pixel p of base
// (4 pixels are 3 or 4 whole 16-byte words: base aligned <=> every group aligned)
template <int CH>
__device__ __forceinline__ void ft_load_pixels(const float* base, int64_t p, int n, bool vec, float (&c)[4][4]) {
    const float* q = base + p * CH;
    if (vec) {
        float f[4 * CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const float4 t = reinterpret_cast<const float4*>(q)[k];
            f[4 * k] = t.x; f[4 * k + 1] = t.y; f[4 * k + 2] = t.z; f[4 * k + 3] = t.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) c[k][j] = j < CH ? f[k * CH + j] : 0.0f;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) c[k][j] = (k < n && j < CH) ? q[k * CH + j] : 0.0f;
    }
}
template <int CH>
__device__ __forceinline__ void ft_store_pixels(float* base, int64_t p, int n, const float (&c)[4][4]) {
    float* q = base + p * CH;
    if (n == 4 && ft_al16(base)) {
        float f[4 * CH];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < CH; ++j) f[k * CH + j] = c[k][j];
#pragma unroll
        for (int k = 0; k < CH; ++k)
            reinterpret_cast<float4*>(q)[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (k < n) q[k * CH + j] = c[k][j];
    }
}

// render_colors: [H,W,D] interleaved, or (planar) one plane per channel [D,H,W], as the rasterizer stores it under no_grad
__device__ __forceinline__ void ft_load_colors(const float* colors, int D, int planar, int64_t P, int64_t p, int n,
                                               float (&c)[4][4]) {
    if (planar) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (j < D) ft_load_plane(colors + j * P + p, n, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k][j] = v[k];
        }
        return;
    }
    const bool vec = n == 4 && ft_al16(colors);
    if (D == 4) ft_load_pixels<4>(colors, p, n, vec, c);
    else ft_load_pixels<3>(colors, p, n, vec, c);
}

// the sky's three channels of n pixels from p on
__device__ __forceinline__ void ft_load_sky(const FtSky& S, int64_t p, int n, int W, int64_t P, float (&s)[4][3]) {
    if (S.mode == FT_SKY_PIX4 || S.mode == FT_SKY_PIX3) {
        // pixel stride 4: the 16-byte word of the frame's LAST pixel reaches one element past the view's last channel, so
        // the group that holds it reads scalars and nothing outside the view is ever touched
        float t[4][4];
        if (S.mode == FT_SKY_PIX3) {
            ft_load_pixels<3>(S.p, p, n, n == 4 && ft_al16(S.p), t);
        } else if (n == 4 && p + 4 < P && ft_al16(S.p)) {
            ft_load_pixels<4>(S.p, p, n, true, t);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) t[k][j] = k < n ? S.p[(p + k) * 4 + j] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) s[k][j] = t[k][j];
    } else if (S.mode == FT_SKY_PLANES) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float v[4];
            ft_load_plane(S.p + j * P + p, n, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k][j] = v[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t q = p + k;
            const int64_t y = q / W, x = q - y * W;
#pragma unroll
            for (int j = 0; j < 3; ++j) s[k][j] = k < n ? S.p[j * S.sc + y * S.sh + x * S.sw] : 0.0f;
        }
    }
}

// v_j = c_j + s_j * keep (or c_j); clamp: both operands to [0,1] first
__device__ __forceinline__ void ft_composite(const float (&c)[4], const float (&s)[3], float keep, bool sky, bool clamp,
                                             float (&v)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float cj = clamp ? ft_clamp01(c[j]) : c[j];
        const float sj = clamp ? ft_clamp01(s[j]) : s[j];
        v[j] = sky ? ft_add(cj, ft_mul(sj, keep)) : cj;
    }
}

// grid (ceil(P / FT_GROUP))
__global__ __launch_bounds__(FT_NT) void frame_tail_fwd_kernel(const float* __restrict__ colors, int D, int planar,
                                                               const float* __restrict__ alphas, FtSky S,
                                                               const float* __restrict__ affine, int W, int64_t P,
                                                               int clamp, float* __restrict__ rgb,
                                                               float* __restrict__ depth) {
    const int64_t p = ((int64_t)blockIdx.x * FT_NT + threadIdx.x) * FT_PPL;
    if (p >= P) return;
    const int n = P - p < FT_PPL ? (int)(P - p) : FT_PPL;
    const bool sky = S.mode != FT_SKY_NONE;
    float A[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) A[i] = affine ? affine[i] : 0.0f;
    float c[4][4], a[4], s[4][3] = {};
    ft_load_colors(colors, D, planar, P, p, n, c);
    ft_load_plane(alphas + p, n, a);
    if (sky) ft_load_sky(S, p, n, W, P, s);
    float out[3][4], dep[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float keep = ft_sub(1.0f, a[k]);
        float v[3];
        ft_composite(c[k], s[k], keep, sky, clamp != 0, v);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float r = v[i];
            if (affine)
                r = ft_add(ft_add(ft_add(ft_mul(A[4 * i], v[0]), ft_mul(A[4 * i + 1], v[1])),
                                        ft_mul(A[4 * i + 2], v[2])), A[4 * i + 3]);
            out[i][k] = clamp ? ft_clamp01(r) : r;
        }
        dep[k] = ft_div(c[k][3], ft_amax(a[k]));
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) ft_store_plane(rgb + i * P + p, n, out[i]);
    if (depth) ft_store_plane(depth + p, n, dep);
}

// butterfly over the block: 6 levels in the wave, 2 over the 4 waves; every lane of wave 0 ends with the block's sum
__device__ __forceinline__ void ft_block_sum12(float (&acc)[12], float (*red)[12]) {
#pragma unroll
    for (int j = 0; j < 12; ++j)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[j] = ft_add(acc[j], __shfl_xor(acc[j], d, 64));
    const int wave = threadIdx.x >> 6;
    if (sc_lane() == 0) {
#pragma unroll
        for (int j = 0; j < 12; ++j) red[wave][j] = acc[j];
    }
    __syncthreads();
}

// grid (ceil(P / FT_BWD_CHUNK)).  Any of g, h, grad_* may be null; partials [gridDim.x, 12] non-null asks for the sums.
__global__ __launch_bounds__(FT_NT) void frame_tail_bwd_kernel(const float* __restrict__ colors, int D, int planar,
                                                               const float* __restrict__ alphas, FtSky S,
                                                               const float* __restrict__ affine, int W, int64_t P,
                                                               const float* __restrict__ g, const float* __restrict__ h,
                                                               float* __restrict__ grad_colors,
                                                               float* __restrict__ grad_alphas,
                                                               float* __restrict__ grad_sky, int grad_sky_planar,
                                                               float* __restrict__ partials) {
    __shared__ float red[FT_NT / 64][12];
    const bool sky = S.mode != FT_SKY_NONE;
    float A[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) A[i] = affine ? affine[i] : 0.0f;
    float acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int pass = 0; pass < FT_BWD_PASSES; ++pass) {
        const int64_t p = (((int64_t)blockIdx.x * FT_BWD_PASSES + pass) * FT_NT + threadIdx.x) * FT_PPL;
        if (p >= P) continue;
        const int n = P - p < FT_PPL ? (int)(P - p) : FT_PPL;
        float c[4][4], a[4], s[4][3] = {}, gg[3][4] = {}, hh[4] = {};
        ft_load_colors(colors, D, planar, P, p, n, c);
        ft_load_plane(alphas + p, n, a);
        if (sky) ft_load_sky(S, p, n, W, P, s);
        if (g) {
#pragma unroll
            for (int i = 0; i < 3; ++i) ft_load_plane(g + i * P + p, n, gg[i]);
        }
        if (h) ft_load_plane(h + p, n, hh);
        float dcol[4][4], dsky[4][4], dal[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float keep = ft_sub(1.0f, a[k]), m = ft_amax(a[k]);
            float gv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                gv[j] = affine ? ft_add(ft_add(ft_mul(A[j], gg[0][k]), ft_mul(A[4 + j], gg[1][k])),
                                           ft_mul(A[8 + j], gg[2][k]))
                               : gg[j][k];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                dcol[k][j] = gv[j];
                dsky[k][j] = ft_mul(gv[j], keep);
            }
            dcol[k][3] = ft_div(hh[k], m);
            dsky[k][3] = 0.0f;
            // -(gv . s) - [a >= 1e-10f] h c_3 / m^2
            float da = 0.0f;
            if (sky)
                da = -ft_add(ft_add(ft_mul(gv[0], s[k][0]), ft_mul(gv[1], s[k][1])), ft_mul(gv[2], s[k][2]));
            if (h && D == 4 && a[k] >= FT_AMIN) da = ft_sub(da, ft_div(ft_mul(hh[k], c[k][3]), ft_mul(m, m)));
            dal[k] = da;
            if (partials && k < n) {
                float v[3];
                ft_composite(c[k], s[k], keep, sky, false, v);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[4 * i + j] = ft_add(acc[4 * i + j], ft_mul(gg[i][k], v[j]));
                    acc[4 * i + 3] = ft_add(acc[4 * i + 3], gg[i][k]);
                }
            }
        }
        if (grad_colors) {
            if (D == 4) ft_store_pixels<4>(grad_colors, p, n, dcol);
            else ft_store_pixels<3>(grad_colors, p, n, dcol);
        }
        if (grad_alphas) ft_store_plane(grad_alphas + p, n, dal);
        if (grad_sky) {
            if (grad_sky_planar) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float v[4] = {dsky[0][j], dsky[1][j], dsky[2][j], dsky[3][j]};
                    ft_store_plane(grad_sky + j * P + p, n, v);
                }
            } else {
                ft_store_pixels<3>(grad_sky, p, n, dsky);
            }
        }
    }
    if (partials) {
        ft_block_sum12(acc, red);
        if (threadIdx.x < 12) {
            const int j = threadIdx.x;
            partials[(int64_t)blockIdx.x * 12 + j] = ft_add(ft_add(red[0][j], red[1][j]), ft_add(red[2][j], red[3][j]));
        }
    }
}

// one block: grad_affine[j] = (float) sum over the nblk block partials, in float64
__global__ __launch_bounds__(FT_NT) void frame_tail_finish_kernel(const float* __restrict__ partials, int nblk,
                                                                  float* __restrict__ grad_affine) {
    __shared__ double red[FT_NT / 64][12];
    double s[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) s[j] = 0.0;
    for (int b = threadIdx.x; b < nblk; b += FT_NT)
#pragma unroll
        for (int j = 0; j < 12; ++j) s[j] += (double)partials[(int64_t)b * 12 + j];
#pragma unroll
    for (int j = 0; j < 12; ++j)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[j] += __shfl_xor(s[j], d, 64);
    if (sc_lane() == 0) {
#pragma unroll
        for (int j = 0; j < 12; ++j) red[threadIdx.x >> 6][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int j = threadIdx.x;
        grad_affine[j] = (float)((red[0][j] + red[1][j]) + (red[2][j] + red[3][j]));
    }
}

bool ft_sizes_ok(int H, int W, int D) { return H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && (D == 3 || D == 4); }

// the sky's layout from its strides (channel, row, column; a size-1 axis carries no stride)
bool ft_sky(const float* sky, const int64_t* st, int H, int W, FtSky* out) {
    *out = FtSky{sky, 0, 0, 0, FT_SKY_NONE};
    if (!sky) return true;
    if (!st || st[0] < 0 || st[1] < 0 || st[2] < 0) return false;
    out->sc = st[0]; out->sh = st[1]; out->sw = st[2];
    const auto dense = [&](int64_t pix) { return (W == 1 || st[2] == pix) && (H == 1 || st[1] == pix * W); };
    if (st[0] == 1 && dense(4)) out->mode = FT_SKY_PIX4;
    else if (st[0] == 1 && dense(3)) out->mode = FT_SKY_PIX3;
    else if (st[0] == (int64_t)H * W && dense(1)) out->mode = FT_SKY_PLANES;
    else out->mode = FT_SKY_STRIDED;
    return true;
}

inline unsigned ft_blocks(int64_t P, int chunk) { return (unsigned)((P + chunk - 1) / chunk); }

}  // namespace

extern "C" size_t sc_frame_tail_workspace_bytes(int height, int width) {
    if (!ft_sizes_ok(height, width, 4)) return 0;
    return (size_t)ft_blocks((int64_t)height * width, FT_BWD_CHUNK) * 12 * sizeof(float);
}

extern "C" int sc_frame_tail_fwd(const float* colors, int channels, int colors_planar, const float* alphas, const float* sky,
                                 const int64_t* sky_strides_host, const float* affine, int height, int width, int clamp,
                                 float* rgb, float* depth, sc_stream_t stream) {
    if (!ft_sizes_ok(height, width, channels) || (clamp != 0 && clamp != 1)) return SC_EINVAL;
    if (colors_planar != 0 && colors_planar != 1) return SC_EINVAL;
    if (!colors || !alphas || !rgb || (depth && channels != 4)) return SC_EINVAL;
    FtSky S;
    if (!ft_sky(sky, sky_strides_host, height, width, &S)) return SC_EINVAL;
    const int64_t P = (int64_t)height * width;
    hipLaunchKernelGGL(frame_tail_fwd_kernel, dim3(ft_blocks(P, FT_GROUP)), dim3(FT_NT), 0, sc_s(stream), colors, channels,
                       colors_planar, alphas, S, affine, width, P, clamp, rgb, depth);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_frame_tail_bwd(const float* colors, int channels, int colors_planar, const float* alphas, const float* sky,
                                 const int64_t* sky_strides_host, const float* affine, int height, int width,
                                 const float* grad_rgb, const float* grad_depth, float* grad_colors, float* grad_alphas,
                                 float* grad_sky, int grad_sky_planar, float* grad_affine, void* workspace,
                                 size_t workspace_bytes, sc_stream_t stream) {
    if (!ft_sizes_ok(height, width, channels) || (grad_sky_planar != 0 && grad_sky_planar != 1)) return SC_EINVAL;
    if (colors_planar != 0 && colors_planar != 1) return SC_EINVAL;
    if (!colors || !alphas || (!grad_rgb && !grad_depth)) return SC_EINVAL;
    if (!grad_colors && !grad_alphas && !grad_sky && !grad_affine) return SC_EINVAL;
    if (grad_depth && channels != 4) return SC_EINVAL;
    if ((grad_sky && (!sky || !grad_rgb)) || (grad_affine && (!affine || !grad_rgb))) return SC_EINVAL;
    FtSky S;
    if (!ft_sky(sky, sky_strides_host, height, width, &S)) return SC_EINVAL;
    if (grad_affine && (!workspace || workspace_bytes < sc_frame_tail_workspace_bytes(height, width))) return SC_EWORKSPACE;
    const int64_t P = (int64_t)height * width;
    const unsigned nblk = ft_blocks(P, FT_BWD_CHUNK);
    float* partials = grad_affine ? static_cast<float*>(workspace) : nullptr;
    hipLaunchKernelGGL(frame_tail_bwd_kernel, dim3(nblk), dim3(FT_NT), 0, sc_s(stream), colors, channels, colors_planar, alphas, S,
                       affine,
                       width, P, grad_rgb, grad_depth, grad_colors, grad_alphas, grad_sky, grad_sky_planar, partials);
    SC_LAUNCH_CHECK();
    if (grad_affine) {
        hipLaunchKernelGGL(frame_tail_finish_kernel, dim3(1), dim3(FT_NT), 0, sc_s(stream), partials, (int)nblk, grad_affine);
        SC_LAUNCH_CHECK();
    }
    return SC_OK;
}
