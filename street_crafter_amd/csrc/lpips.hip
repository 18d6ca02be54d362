// The arithmetic around the LPIPS network (include/street_crafter_amd.h, sc_lpips_*): what the reference's
// lpips(image * mask, gt * mask) (train.py:172,185; street_gaussian/utils/lpipsPyTorch/modules/{lpips,networks,utils}.py)
// runs besides its ten convolutions.  Three kernels:
//
//   prep   z = (where(mask, img, 0) - mean_c) / std_c from the strided render, one thread per pixel, and its backward.
//          Every operation separately rounded (contraction off, IEEE division): bit-identical to the torch expression.
//   head   all taps of both images -> the distance.  A workgroup owns 64 adjacent pixels of one tap: the 64 lanes of a
//          wave sit on 64 adjacent pixels of one channel row (one 256-byte request per load), the HEAD_WAVES waves of the
//          workgroup split the channels between them and meet in LDS.  Pass 1 sums the squares (the per-pixel norms),
//          pass 2 reads the same rows again (L2: a tile is C x 256 B per image) and sums w_c (fx/(nx+eps) - fy/(ny+eps))^2:
//          the difference is formed before it is squared, so x == y gives exactly 0.  Nothing normalised, differenced
//          or squared is written; the norms (P floats per tap and image) are written for the backward when asked for.
//          One partial per workgroup goes to the workspace; a one-workgroup kernel adds them per tap in a fixed order.
//   head backward   the same tiling: pass 1 sums S = sum_c a_c f_c per pixel, pass 2 writes r a_k - f_k (r^2/n) S.
//          Every element has one writer: no atomics, bit-identical from run to run.
//
// All taps of a call travel BY VALUE in the kernel arguments with the running workgroup count per tap (optim.hip's table).
// Sums are carried in double and rounded to float once: a channel count of 512 must not show in the last bits.
#include "sc_common.h"

namespace {

constexpr int HEAD_WAVES = 8;                        // channel groups of a workgroup
constexpr int HEAD_THREADS = HEAD_WAVES * SC_WAVE;
constexpr int HEAD_TILE = SC_WAVE;                   // pixels of a workgroup
constexpr float LPIPS_EPS = 1e-10f;
constexpr int PREP_THREADS = 256;
constexpr int FINAL_THREADS = 256;

struct HeadArgs {
    sc_lpips_tap t[SC_LPIPS_MAX_TAPS];
    uint32_t chunk_end[SC_LPIPS_MAX_TAPS];           // workgroups of taps 0..i (inclusive running count)
    int n;
};

// ---- prep -------------------------------------------------------------------------------------------------------
struct PrepArgs {
    int64_t sc, sh, sw, mh, mw;                      // image (channel, row, column) and mask (row, column) strides
    int H, W;
    float mean[3], std[3];
};

#pragma clang fp contract(off)
__global__ __launch_bounds__(PREP_THREADS) void lpips_prep_fwd_kernel(const PrepArgs a, const float* __restrict__ img,
                                                                      const uint8_t* __restrict__ mask,
                                                                      float* __restrict__ out) {
    const int64_t n = (int64_t)a.H * a.W;
    const int64_t i = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t y = i / a.W, x = i - y * a.W;
    const bool keep = mask ? mask[y * a.mh + x * a.mw] != 0 : true;
    const float* p = img + y * a.sh + x * a.sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = keep ? p[c * a.sc] : 0.0f;
        out[c * n + i] = (v - a.mean[c]) / a.std[c];
    }
}

__global__ __launch_bounds__(PREP_THREADS) void lpips_prep_bwd_kernel(const PrepArgs a, const float* __restrict__ grad_out,
                                                                      const uint8_t* __restrict__ mask,
                                                                      float* __restrict__ grad_img) {
    const int64_t n = (int64_t)a.H * a.W;
    const int64_t i = (int64_t)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t y = i / a.W, x = i - y * a.W;
    const bool keep = mask ? mask[y * a.mh + x * a.mw] != 0 : true;
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_img[c * n + i] = keep ? grad_out[c * n + i] / a.std[c] : 0.0f;
}
#pragma clang fp contract(fast)

// ---- head -------------------------------------------------------------------------------------------------------
// The sum over the HEAD_WAVES channel groups of one pixel, in a fixed order; every wave computes the same number.
__device__ __forceinline__ double head_sum_groups(const double (*part)[HEAD_TILE], int lane) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < HEAD_WAVES; ++w) s += part[w][lane];
    return s;
}

__device__ __forceinline__ double head_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, SC_WAVE);
    return v;
}

__global__ __launch_bounds__(HEAD_THREADS) void lpips_head_fwd_kernel(const HeadArgs a, double* __restrict__ partials) {
    __shared__ double part_x[HEAD_WAVES][HEAD_TILE], part_y[HEAD_WAVES][HEAD_TILE], part_d[HEAD_WAVES];
    const uint32_t chunk = blockIdx.x;
    const int e = sc_find_entry(a.chunk_end, a.n, chunk);
    const sc_lpips_tap& t = a.t[e];
    const int lane = sc_lane(), wave = (int)(threadIdx.x >> 6);
    const int64_t p = (int64_t)(chunk - (e ? a.chunk_end[e - 1] : 0u)) * HEAD_TILE + lane;
    const bool on = p < t.pixels;
    const int C = t.channels;
    const float* __restrict__ fx = t.fx + p;
    const float* __restrict__ fy = t.fy + p;

    double sx = 0.0, sy = 0.0;
    if (on) {
#pragma unroll 4
        for (int c = wave; c < C; c += HEAD_WAVES) {
            const double x = (double)fx[c * t.stride_x], y = (double)fy[c * t.stride_y];
            sx = fma(x, x, sx);
            sy = fma(y, y, sy);
        }
    }
    part_x[wave][lane] = sx;
    part_y[wave][lane] = sy;
    __syncthreads();
    const float nx = sqrtf((float)head_sum_groups(part_x, lane)), ny = sqrtf((float)head_sum_groups(part_y, lane));
    if (on && wave == 0) {
        if (t.norm_x) t.norm_x[p] = nx;
        if (t.norm_y) t.norm_y[p] = ny;
    }
    const float dx = nx + LPIPS_EPS, dy = ny + LPIPS_EPS;
    double acc = 0.0;
    if (on) {
#pragma unroll 4
        for (int c = wave; c < C; c += HEAD_WAVES) {
            const float u = fx[c * t.stride_x] / dx - fy[c * t.stride_y] / dy;
            acc = fma((double)t.weight[c], (double)u * (double)u, acc);
        }
    }
    acc = head_wave_sum(acc);
    if (lane == 0) part_d[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < HEAD_WAVES; ++w) s += part_d[w];
        partials[chunk] = s;
    }
}

// out[l] = (1 / P_l) sum of tap l's partials, out[n] = out[0] + ... + out[n-1] in tap order.  One workgroup; a thread
// adds every FINAL_THREADS-th partial, the threads meet in a tree: the order is a function of the sizes alone.
__global__ __launch_bounds__(FINAL_THREADS) void lpips_head_final_kernel(const HeadArgs a, const double* __restrict__ partials,
                                                                         float* __restrict__ out) {
    __shared__ double tree[FINAL_THREADS];
    float total = 0.0f;
    for (int e = 0; e < a.n; ++e) {
        const uint32_t first = e ? a.chunk_end[e - 1] : 0u, last = a.chunk_end[e];
        double s = 0.0;
        for (uint32_t i = first + threadIdx.x; i < last; i += FINAL_THREADS) s += partials[i];
        tree[threadIdx.x] = s;
        __syncthreads();
        for (int d = FINAL_THREADS / 2; d >= 1; d >>= 1) {
            if ((int)threadIdx.x < d) tree[threadIdx.x] += tree[threadIdx.x + d];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float dl = (float)(tree[0] / (double)a.t[e].pixels);
            out[e] = dl;
            total += dl;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[a.n] = total;
}

__global__ __launch_bounds__(HEAD_THREADS) void lpips_head_bwd_kernel(const HeadArgs a, const float* __restrict__ grad) {
    __shared__ double part_x[HEAD_WAVES][HEAD_TILE], part_y[HEAD_WAVES][HEAD_TILE];
    const uint32_t chunk = blockIdx.x;
    const int e = sc_find_entry(a.chunk_end, a.n, chunk);
    const sc_lpips_tap& t = a.t[e];
    const int lane = sc_lane(), wave = (int)(threadIdx.x >> 6);
    const int64_t p = (int64_t)(chunk - (e ? a.chunk_end[e - 1] : 0u)) * HEAD_TILE + lane;
    const bool on = p < t.pixels;
    const int C = t.channels;
    const int64_t P = t.pixels;
    const float* __restrict__ fx = t.fx + p;
    const float* __restrict__ fy = t.fy + p;
    const float nx = on ? t.norm_x[p] : 1.0f, ny = on ? t.norm_y[p] : 1.0f;
    const float dx = nx + LPIPS_EPS, dy = ny + LPIPS_EPS;
    const float rx = 1.0f / dx, ry = 1.0f / dy;
    const float scale = 2.0f * grad[0] / (float)P;

    double sx = 0.0, sy = 0.0;
    if (on) {
#pragma unroll 4
        for (int c = wave; c < C; c += HEAD_WAVES) {
            const float x = fx[c * t.stride_x], y = fy[c * t.stride_y];
            const float ac = scale * t.weight[c] * (x / dx - y / dy);
            sx = fma((double)ac, (double)x, sx);
            sy = fma((double)ac, (double)y, sy);
        }
    }
    part_x[wave][lane] = sx;
    part_y[wave][lane] = sy;
    __syncthreads();
    if (!on) return;
    // (n == 0: every f of the pixel is 0 and the second term is taken as 0, the limit along f -> 0)
    const float kx = nx > 0.0f ? (rx * rx / nx) * (float)head_sum_groups(part_x, lane) : 0.0f;
    const float ky = ny > 0.0f ? (ry * ry / ny) * (float)head_sum_groups(part_y, lane) : 0.0f;
    float* __restrict__ gx = t.grad_fx ? t.grad_fx + p : nullptr;
    float* __restrict__ gy = t.grad_fy ? t.grad_fy + p : nullptr;
#pragma unroll 4
    for (int c = wave; c < C; c += HEAD_WAVES) {
        const float x = fx[c * t.stride_x], y = fy[c * t.stride_y];
        const float ac = scale * t.weight[c] * (x / dx - y / dy);
        if (gx) gx[c * P] = rx * ac - x * kx;
        if (gy) gy[c * P] = y * ky - ry * ac;
    }
}

// -> SC_OK and the filled table, or the error of the first bad entry; nothing is launched here.
int head_table(const sc_lpips_tap* taps_host, int n_taps, HeadArgs& a) {
    if (n_taps <= 0 || n_taps > SC_LPIPS_MAX_TAPS || !taps_host) return SC_EINVAL;
    uint64_t chunks = 0;
    for (int i = 0; i < n_taps; ++i) {
        const sc_lpips_tap& t = taps_host[i];
        if (t.channels <= 0 || t.pixels <= 0) return SC_EINVAL;
        if (t.stride_x < t.pixels || t.stride_y < t.pixels) return SC_EINVAL;
        if (!t.fx || !t.fy || !t.weight) return SC_EINVAL;
        chunks += ((uint64_t)t.pixels + HEAD_TILE - 1) / HEAD_TILE;
        if (chunks > 0x7fffffffull) return SC_EINVAL;
        a.t[i] = t;
        a.chunk_end[i] = (uint32_t)chunks;
    }
    a.n = n_taps;
    return SC_OK;
}

int prep_args(const int64_t* strides_host, int height, int width, const float* mean_host, const float* std_host,
              PrepArgs& a) {
    if (height <= 0 || width <= 0 || !strides_host || !std_host) return SC_EINVAL;
    for (int k = 0; k < 5; ++k)
        if (strides_host[k] < 0) return SC_EINVAL;
    a.sc = strides_host[0]; a.sh = strides_host[1]; a.sw = strides_host[2]; a.mh = strides_host[3]; a.mw = strides_host[4];
    a.H = height; a.W = width;
    for (int c = 0; c < 3; ++c) {
        if (std_host[c] == 0.0f) return SC_EINVAL;
        a.mean[c] = mean_host ? mean_host[c] : 0.0f;
        a.std[c] = std_host[c];
    }
    return SC_OK;
}

}  // namespace

extern "C" int sc_lpips_prep_fwd(const float* img, const uint8_t* mask, const int64_t* strides_host, int height, int width,
                                 const float* mean_host, const float* std_host, float* out, sc_stream_t stream) {
    PrepArgs a;
    if (!mean_host) return SC_EINVAL;
    const int rc = prep_args(strides_host, height, width, mean_host, std_host, a);
    if (rc != SC_OK) return rc;
    if (!img || !out) return SC_EINVAL;
    const int64_t n = (int64_t)height * width;
    hipLaunchKernelGGL(lpips_prep_fwd_kernel, dim3((unsigned)((n + PREP_THREADS - 1) / PREP_THREADS)), dim3(PREP_THREADS), 0,
                       sc_s(stream), a, img, mask, out);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_lpips_prep_bwd(const float* grad_out, const uint8_t* mask, const int64_t* strides_host, int height,
                                 int width, const float* std_host, float* grad_img, sc_stream_t stream) {
    PrepArgs a;
    const int rc = prep_args(strides_host, height, width, nullptr, std_host, a);
    if (rc != SC_OK) return rc;
    if (!grad_out || !grad_img) return SC_EINVAL;
    const int64_t n = (int64_t)height * width;
    hipLaunchKernelGGL(lpips_prep_bwd_kernel, dim3((unsigned)((n + PREP_THREADS - 1) / PREP_THREADS)), dim3(PREP_THREADS), 0,
                       sc_s(stream), a, grad_out, mask, grad_img);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" size_t sc_lpips_head_workspace_bytes(const sc_lpips_tap* taps_host, int n_taps) {
    if (n_taps <= 0 || n_taps > SC_LPIPS_MAX_TAPS || !taps_host) return 0;
    uint64_t chunks = 0;
    for (int i = 0; i < n_taps; ++i) {
        if (taps_host[i].pixels <= 0) return 0;
        chunks += ((uint64_t)taps_host[i].pixels + HEAD_TILE - 1) / HEAD_TILE;
    }
    return chunks > 0x7fffffffull ? 0 : (size_t)chunks * sizeof(double);
}

extern "C" int sc_lpips_head_fwd(const sc_lpips_tap* taps_host, int n_taps, float* out, void* workspace,
                                 size_t workspace_bytes, sc_stream_t stream) {
    HeadArgs a;
    const int rc = head_table(taps_host, n_taps, a);
    if (rc != SC_OK) return rc;
    if (!out) return SC_EINVAL;
    const uint32_t chunks = a.chunk_end[a.n - 1];
    if (!workspace || ((uintptr_t)workspace & 7u) || workspace_bytes < (size_t)chunks * sizeof(double)) return SC_EWORKSPACE;
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(lpips_head_fwd_kernel, dim3(chunks), dim3(HEAD_THREADS), 0, sc_s(stream), a, partials);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(lpips_head_final_kernel, dim3(1), dim3(FINAL_THREADS), 0, sc_s(stream), a, partials, out);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_lpips_head_bwd(const sc_lpips_tap* taps_host, int n_taps, const float* grad_value, sc_stream_t stream) {
    HeadArgs all;
    const int rc = head_table(taps_host, n_taps, all);
    if (rc != SC_OK) return rc;
    if (!grad_value) return SC_EINVAL;
    // taps nobody wants a gradient of are left out of the launch
    HeadArgs a;
    a.n = 0;
    uint32_t chunks = 0;
    for (int i = 0; i < n_taps; ++i) {
        const sc_lpips_tap& t = taps_host[i];
        if (!t.grad_fx && !t.grad_fy) continue;
        if (!t.norm_x || !t.norm_y) return SC_EINVAL;
        chunks += (uint32_t)(((uint64_t)t.pixels + HEAD_TILE - 1) / HEAD_TILE);
        a.t[a.n] = t;
        a.chunk_end[a.n] = chunks;
        ++a.n;
    }
    if (a.n == 0) return SC_OK;
    hipLaunchKernelGGL(lpips_head_bwd_kernel, dim3(chunks), dim3(HEAD_THREADS), 0, sc_s(stream), a, grad_value);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
