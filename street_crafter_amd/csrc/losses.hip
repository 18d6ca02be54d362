// Photometric loss of the training step: SSIM and masked L1 (street_gaussian/utils/loss_utils.py:21-37 and 95-131, called
// at train.py:168-188), fused into one pass over the two images, with a gather backward.
//
//   x = where(mask, img1, 0), y = where(mask, img2, 0)             (the reference masks BEFORE it filters)
//   mu1 = G*x, mu2 = G*y, Exx = G*(x x), Eyy = G*(y y), Exy = G*(x y)   G: 11 x 11 Gaussian, sigma 1.5, zero padding 5
//   S = A B / (C D),  A = 2 mu1 mu2 + C1,  B = 2 (Exy - mu1 mu2) + C2,  C = mu1^2 + mu2^2 + C1,  D = Exx - mu1^2 + Eyy - mu2^2 + C2
//   ssim = mean over C*H*W of S;   l1 = mean of |img1 - img2| over the (pixel, channel) entries the mask keeps.
//
// G is separable: each block stages a 64 x 16 output tile plus a 5-pixel halo of x and y in LDS (zero outside the image,
// as conv2d's padding), filters the five moments along rows into LDS, then along columns in registers (four output rows
// per thread), and loops over the channels of its tile.  The 1-D taps are the reference's own fp32 weights
// (loss_utils.gaussian(11, 1.5)); its 2-D window is their outer product.
//
// Backward (gather form, no atomics).  With the per-pixel partials of S, each scaled by 1/(C*H*W),
//   a1 = dS/dmu1 = 2 mu2 (B - A) / (C D) + 2 mu1 S (1/D - 1/C)      (= S (2mu2/A - 2mu2/B - 2mu1/C + 2mu1/D), but finite
//   a2 = dS/dmu2 = 2 mu1 (B - A) / (C D) + 2 mu2 S (1/D - 1/C)         where A or B is 0)
//   b  = dS/dExx = dS/dEyy = -S / D
//   c  = dS/dExy = 2 A / (C D)                                      (= 2 S / B)
// the forward writes the maps, and the backward filters them with the same (symmetric) window:
//   dL/dimg1 = g_ssim [G*a1 + 2 x G*b + y G*c] + g_l1 sign(x - y) / n_kept,    zero where the mask is false;
//   dL/dimg2 = g_ssim [G*a2 + 2 y G*b + x G*c] + g_l1 sign(y - x) / n_kept.
//
// Reductions are deterministic: each block writes its sums of S and |x - y| (double) and its kept count to a slab entry;
// loss_finalize_kernel sums the slab in a fixed order.  The images and the mask are read through element strides, so the
// rasterizer's [H,W,4] output viewed as [3,H,W] and a row crop are taken as they are.
#include "sc_common.h"

namespace {

constexpr int LOSS_WIN = 11;
constexpr int LOSS_R = LOSS_WIN / 2;
constexpr int LOSS_TX = 64;                     // output tile: 64 columns (one per lane) ...
constexpr int LOSS_TY = 16;                     // ... by 16 rows
constexpr int LOSS_HX = LOSS_TX + 2 * LOSS_R;   // staged halo: 74 x 26
constexpr int LOSS_HY = LOSS_TY + 2 * LOSS_R;
constexpr int LOSS_NT = 256;
constexpr int LOSS_RG = LOSS_NT / LOSS_TX;      // 4 row groups
constexpr int LOSS_RPT = LOSS_TY / LOSS_RG;     // 4 output rows per thread in the column pass
constexpr float LOSS_C1 = 0.01f * 0.01f;        // (fp32, as the reference's python floats meet its fp32 maps)
constexpr float LOSS_C2 = 0.03f * 0.03f;

// loss_utils.gaussian(11, 1.5) in fp32, bit for bit (symmetric)
__device__ __forceinline__ float loss_tap(int k) {
    constexpr float w[LOSS_WIN] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f,
                                   0x1.106560p-2f,  0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f,
                                   0x1.0d956cp-10f};
    return w[k];
}

struct LossImg {            // element (b, c, h, w) at p[b*sb + c*sc + h*sh + w*sw]
    const float* p;
    int64_t sb, sc, sh, sw;
};
struct LossMask {           // element (b, h, w) at p[b*sb + h*sh + w*sw]; sb = 0 broadcasts one mask; p null = all kept
    const uint8_t* p;
    int64_t sb, sh, sw;
};

__device__ __forceinline__ float loss_at(const LossImg& v, int b, int c, int y, int x) {
    return v.p[(int64_t)b * v.sb + (int64_t)c * v.sc + (int64_t)y * v.sh + (int64_t)x * v.sw];
}
__device__ __forceinline__ bool loss_kept(const LossMask& m, int b, int y, int x) {
    return m.p == nullptr || m.p[(int64_t)b * m.sb + (int64_t)y * m.sh + (int64_t)x * m.sw] != 0;
}

__device__ __forceinline__ double loss_block_sum(double v, double* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < LOSS_NT / 64; ++w) t += red[w];
    return t;
}

// grid (tiles, B); one block = one 64 x 16 tile of one image, all channels.
// slab[2 * (b * tiles + tile) + {0,1}] = sum S, sum |x - y|;  cnt[b * tiles + tile] = kept (pixel, channel) entries.
// a1 / a2 / bm / cm: [B,C,H,W] maps (null: not written); bm and cm come with a1 and / or a2.
__global__ __launch_bounds__(LOSS_NT) void loss_fwd_kernel(LossImg X, LossImg Y, LossMask M, int C, int H, int W,
                                                           int tiles_x, float inv_n, float* __restrict__ a1,
                                                           float* __restrict__ a2, float* __restrict__ bm,
                                                           float* __restrict__ cm, double* __restrict__ slab,
                                                           int64_t* __restrict__ cnt) {
    __shared__ float sx[LOSS_HY][LOSS_HX];
    __shared__ float sy[LOSS_HY][LOSS_HX];
    __shared__ float hm[5][LOSS_HY][LOSS_TX];
    __shared__ uint8_t sk[LOSS_HY][LOSS_HX];
    __shared__ double red[LOSS_NT / 64];

    const int tid = threadIdx.x;
    const int b = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
    const int ty0 = (tile / tiles_x) * LOSS_TY, tx0 = (tile % tiles_x) * LOSS_TX;
    const int col = tid % LOSS_TX, rg = tid / LOSS_TX;
    const int gx = tx0 + col;

    for (int i = tid; i < LOSS_HY * LOSS_HX; i += LOSS_NT) {
        const int r = i / LOSS_HX, c = i % LOSS_HX;
        const int y = ty0 - LOSS_R + r, x = tx0 - LOSS_R + c;
        sk[r][c] = (y >= 0 && y < H && x >= 0 && x < W && loss_kept(M, b, y, x)) ? 1 : 0;
    }
    double s_sum = 0.0, l_sum = 0.0;
    long long kept = 0;
    for (int ch = 0; ch < C; ++ch) {
        __syncthreads();        // sk is written / the previous channel's readers of sx, sy, hm are done
        for (int i = tid; i < LOSS_HY * LOSS_HX; i += LOSS_NT) {
            const int r = i / LOSS_HX, c = i % LOSS_HX;
            const bool k = sk[r][c] != 0;
            const int y = ty0 - LOSS_R + r, x = tx0 - LOSS_R + c;
            sx[r][c] = k ? loss_at(X, b, ch, y, x) : 0.0f;
            sy[r][c] = k ? loss_at(Y, b, ch, y, x) : 0.0f;
        }
        __syncthreads();
        for (int r = rg; r < LOSS_HY; r += LOSS_RG) {
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < LOSS_WIN; ++k) {
                const float w = loss_tap(k), xv = sx[r][col + k], yv = sy[r][col + k];
                m0 = fmaf(w, xv, m0);
                m1 = fmaf(w, yv, m1);
                m2 = fmaf(w, xv * xv, m2);
                m3 = fmaf(w, yv * yv, m3);
                m4 = fmaf(w, xv * yv, m4);
            }
            hm[0][r][col] = m0; hm[1][r][col] = m1; hm[2][r][col] = m2; hm[3][r][col] = m3; hm[4][r][col] = m4;
        }
        __syncthreads();
        float acc[LOSS_RPT][5];
#pragma unroll
        for (int o = 0; o < LOSS_RPT; ++o)
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[o][q] = 0.f;
#pragma unroll
        for (int k = 0; k < LOSS_RPT + 2 * LOSS_R; ++k) {
            float v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] = hm[q][rg * LOSS_RPT + k][col];
#pragma unroll
            for (int o = 0; o < LOSS_RPT; ++o) {
                const int t = k - o;
                if (t >= 0 && t < LOSS_WIN) {
#pragma unroll
                    for (int q = 0; q < 5; ++q) acc[o][q] = fmaf(loss_tap(t), v[q], acc[o][q]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < LOSS_RPT; ++o) {
            const int ly = rg * LOSS_RPT + o, gy = ty0 + ly;
            if (gy >= H || gx >= W) continue;
            const float mu1 = acc[o][0], mu2 = acc[o][1];
            const float s1 = fmaf(-mu1, mu1, acc[o][2]), s2 = fmaf(-mu2, mu2, acc[o][3]);
            const float s12 = fmaf(-mu1, mu2, acc[o][4]);
            const float A = fmaf(2.f * mu1, mu2, LOSS_C1), B = fmaf(2.f, s12, LOSS_C2);
            const float Cc = fmaf(mu1, mu1, fmaf(mu2, mu2, LOSS_C1)), D = (s1 + s2) + LOSS_C2;
            const float q = 1.0f / (Cc * D);
            const float S = (A * B) * q;
            s_sum += (double)S;
            const float xv = sx[ly + LOSS_R][col + LOSS_R], yv = sy[ly + LOSS_R][col + LOSS_R];
            if (sk[ly + LOSS_R][col + LOSS_R]) {
                l_sum += (double)fabsf(xv - yv);
                ++kept;
            }
            if (bm) {
                const int64_t e = (((int64_t)b * C + ch) * H + gy) * W + gx;
                const float BmA = (B - A) * q, rDC = 1.0f / D - 1.0f / Cc;
                if (a1) a1[e] = (2.f * mu2 * BmA + 2.f * mu1 * S * rDC) * inv_n;
                if (a2) a2[e] = (2.f * mu1 * BmA + 2.f * mu2 * S * rDC) * inv_n;
                bm[e] = (-S / D) * inv_n;
                cm[e] = (2.f * A * q) * inv_n;
            }
        }
    }
    const double ts = loss_block_sum(s_sum, red);
    const double tl = loss_block_sum(l_sum, red);
    const double tk = loss_block_sum((double)kept, red);       // (< 2^53: exact)
    if (tid == 0) {
        const int64_t e = (int64_t)b * tiles + tile;
        slab[2 * e] = ts;
        slab[2 * e + 1] = tl;
        cnt[e] = (int64_t)tk;
    }
}

// one block: per image b, ssim[b] = sum S / (C H W), l1[b] = sum |x - y| / kept (0 / 0 = NaN: torch's mean of an empty
// selection), kept_out[b]; ssim[B] = the mean over all B images.  Fixed summation order.
__global__ __launch_bounds__(LOSS_NT) void loss_finalize_kernel(const double* __restrict__ slab,
                                                                const int64_t* __restrict__ cnt, int B, int tiles,
                                                                double n_img, float* __restrict__ ssim,
                                                                float* __restrict__ l1, int64_t* __restrict__ kept_out) {
    __shared__ double red[LOSS_NT / 64];
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double s = 0.0, l = 0.0, k = 0.0;
        for (int i = threadIdx.x; i < tiles; i += LOSS_NT) {
            const int64_t e = (int64_t)b * tiles + i;
            s += slab[2 * e];
            l += slab[2 * e + 1];
            k += (double)cnt[e];
        }
        s = loss_block_sum(s, red);
        l = loss_block_sum(l, red);
        k = loss_block_sum(k, red);
        total += s;
        if (threadIdx.x == 0) {
            ssim[b] = (float)(s / n_img);
            l1[b] = (float)(l / k);
            if (kept_out) kept_out[b] = (int64_t)k;
        }
    }
    if (threadIdx.x == 0) ssim[B] = (float)(total / (n_img * B));
}

// grid (tiles, B).  WANT bit 0: dL/dimg1 (needs a1), bit 1: dL/dimg2 (needs a2).  g_ssim [B] (null: no SSIM term),
// g_l1 [B] + kept [B] (null: no L1 term); g1 / g2 contiguous [B,C,H,W].
template <int WANT>
__global__ __launch_bounds__(LOSS_NT) void loss_bwd_kernel(LossImg X, LossImg Y, LossMask M, int C, int H, int W,
                                                           int tiles_x, const float* __restrict__ a1,
                                                           const float* __restrict__ a2, const float* __restrict__ bm,
                                                           const float* __restrict__ cm, const float* __restrict__ g_ssim,
                                                           const float* __restrict__ g_l1,
                                                           const int64_t* __restrict__ kept, float* __restrict__ g1,
                                                           float* __restrict__ g2) {
    constexpr bool G1 = (WANT & 1) != 0, G2 = (WANT & 2) != 0;
    constexpr int NM = 2 + (G1 ? 1 : 0) + (G2 ? 1 : 0);     // maps: b, c, then a1 and / or a2
    __shared__ float sm[NM][LOSS_HY][LOSS_HX];
    __shared__ float hm[NM][LOSS_HY][LOSS_TX];

    const int tid = threadIdx.x;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / tiles_x) * LOSS_TY, tx0 = (tile % tiles_x) * LOSS_TX;
    const int col = tid % LOSS_TX, rg = tid / LOSS_TX;
    const int gx = tx0 + col;
    const bool ssim_term = g_ssim != nullptr;
    const float gs = ssim_term ? g_ssim[b] : 0.0f;
    const float gl = (g_l1 != nullptr) ? g_l1[b] / (float)kept[b] : 0.0f;     // torch: mean's g / n, then abs's sign * (.)

    for (int ch = 0; ch < C; ++ch) {
        if (ssim_term) {
            __syncthreads();
            const int64_t plane = ((int64_t)b * C + ch) * H;
            for (int i = tid; i < LOSS_HY * LOSS_HX; i += LOSS_NT) {
                const int r = i / LOSS_HX, c = i % LOSS_HX;
                const int y = ty0 - LOSS_R + r, x = tx0 - LOSS_R + c;
                const bool in = y >= 0 && y < H && x >= 0 && x < W;
                const int64_t e = (plane + y) * W + x;
                int m = 0;
                sm[m++][r][c] = in ? bm[e] : 0.0f;
                sm[m++][r][c] = in ? cm[e] : 0.0f;
                if (G1) sm[m++][r][c] = in ? a1[e] : 0.0f;
                if (G2) sm[m++][r][c] = in ? a2[e] : 0.0f;
            }
            __syncthreads();
            for (int r = rg; r < LOSS_HY; r += LOSS_RG) {
                float h[NM];
#pragma unroll
                for (int q = 0; q < NM; ++q) h[q] = 0.f;
#pragma unroll
                for (int k = 0; k < LOSS_WIN; ++k) {
                    const float w = loss_tap(k);
#pragma unroll
                    for (int q = 0; q < NM; ++q) h[q] = fmaf(w, sm[q][r][col + k], h[q]);
                }
#pragma unroll
                for (int q = 0; q < NM; ++q) hm[q][r][col] = h[q];
            }
            __syncthreads();
        }
        float acc[LOSS_RPT][NM];
#pragma unroll
        for (int o = 0; o < LOSS_RPT; ++o)
#pragma unroll
            for (int q = 0; q < NM; ++q) acc[o][q] = 0.f;
        if (ssim_term) {
#pragma unroll
            for (int k = 0; k < LOSS_RPT + 2 * LOSS_R; ++k) {
                float v[NM];
#pragma unroll
                for (int q = 0; q < NM; ++q) v[q] = hm[q][rg * LOSS_RPT + k][col];
#pragma unroll
                for (int o = 0; o < LOSS_RPT; ++o) {
                    const int t = k - o;
                    if (t >= 0 && t < LOSS_WIN) {
#pragma unroll
                        for (int q = 0; q < NM; ++q) acc[o][q] = fmaf(loss_tap(t), v[q], acc[o][q]);
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < LOSS_RPT; ++o) {
            const int gy = ty0 + rg * LOSS_RPT + o;
            if (gy >= H || gx >= W) continue;
            const int64_t e = (((int64_t)b * C + ch) * H + gy) * W + gx;
            const bool k = loss_kept(M, b, gy, gx);
            const float xv = k ? loss_at(X, b, ch, gy, gx) : 0.0f, yv = k ? loss_at(Y, b, ch, gy, gx) : 0.0f;
            const float sgn = (xv > yv) ? 1.0f : ((xv < yv) ? -1.0f : 0.0f);
            const float Gb = acc[o][0], Gc = acc[o][1];
            if (G1) {
                const float v = gs * (acc[o][2] + 2.f * xv * Gb + yv * Gc) + gl * sgn;
                g1[e] = k ? v : 0.0f;
            }
            if (G2) {
                const float v = gs * (acc[o][G1 ? 3 : 2] + 2.f * yv * Gb + xv * Gc) - gl * sgn;
                g2[e] = k ? v : 0.0f;
            }
        }
    }
}

bool loss_views(const int64_t* st, int B, int C, int H, int W, int mask_b, int mask_h, int mask_w, bool has_mask,
                LossImg* X, LossImg* Y, LossMask* M) {
    for (int i = 0; i < 11; ++i)
        if (st[i] < 0) return false;
    (void)C;
    if (has_mask && (mask_h != H || mask_w != W || (mask_b != 1 && mask_b != B))) return false;
    X->sb = st[0]; X->sc = st[1]; X->sh = st[2]; X->sw = st[3];
    Y->sb = st[4]; Y->sc = st[5]; Y->sh = st[6]; Y->sw = st[7];
    M->sb = (has_mask && mask_b == B && B > 1) ? st[8] : 0;
    M->sh = st[9]; M->sw = st[10];
    return true;
}

inline int loss_tiles_x(int W) { return (W + LOSS_TX - 1) / LOSS_TX; }
inline int loss_tiles(int H, int W) { return loss_tiles_x(W) * ((H + LOSS_TY - 1) / LOSS_TY); }

bool loss_sizes_ok(int B, int C, int H, int W, int window) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || window != LOSS_WIN) return false;
    // tiles per image and every element index of a [B,C,H,W] map must fit the kernels' arithmetic
    return (int64_t)loss_tiles(H, W) < (1ll << 31) && (int64_t)B < 65536 && (int64_t)B * C * H * W < (1ll << 62);
}

}  // namespace

extern "C" size_t sc_loss_workspace_bytes(int batch, int channels, int height, int width) {
    if (!loss_sizes_ok(batch, channels, height, width, LOSS_WIN)) return 0;
    const size_t entries = (size_t)batch * (size_t)loss_tiles(height, width);
    return entries * (2 * sizeof(double) + sizeof(int64_t));
}

extern "C" int sc_loss_fwd(const float* img1, const float* img2, const uint8_t* mask, const int64_t* strides_host,
                           int batch, int channels, int height, int width, int mask_batch, int mask_height,
                           int mask_width, int window, float* ssim_out, float* l1_out, int64_t* kept_out,
                           float* map_a1, float* map_a2, float* map_b, float* map_c, void* workspace,
                           size_t workspace_bytes, sc_stream_t stream) {
    if (!loss_sizes_ok(batch, channels, height, width, window)) return SC_EINVAL;
    if (!img1 || !img2 || !strides_host || !ssim_out || !l1_out || !workspace) return SC_EINVAL;
    // the maps come as a set: b and c with a1 and / or a2, or none at all
    const bool maps = map_b != nullptr;
    if ((map_c != nullptr) != maps || (map_a1 != nullptr || map_a2 != nullptr) != maps) return SC_EINVAL;
    LossImg X{img1, 0, 0, 0, 0}, Y{img2, 0, 0, 0, 0};
    LossMask M{mask, 0, 0, 0};
    if (!loss_views(strides_host, batch, channels, height, width, mask_batch, mask_height, mask_width, mask != nullptr,
                    &X, &Y, &M))
        return SC_EINVAL;
    if (workspace_bytes < sc_loss_workspace_bytes(batch, channels, height, width)) return SC_EWORKSPACE;
    const int tiles = loss_tiles(height, width);
    double* slab = static_cast<double*>(workspace);
    int64_t* cnt = reinterpret_cast<int64_t*>(slab + 2 * (size_t)batch * tiles);
    const double n_img = (double)channels * height * width;
    hipLaunchKernelGGL(loss_fwd_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(LOSS_NT), 0, sc_s(stream), X, Y, M,
                       channels, height, width, loss_tiles_x(width), (float)(1.0 / n_img), map_a1, map_a2, map_b, map_c,
                       slab, cnt);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(LOSS_NT), 0, sc_s(stream), slab, cnt, batch, tiles, n_img,
                       ssim_out, l1_out, kept_out);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_loss_bwd(const float* img1, const float* img2, const uint8_t* mask, const int64_t* strides_host,
                           int batch, int channels, int height, int width, int mask_batch, int mask_height,
                           int mask_width, int window, const float* map_a1, const float* map_a2, const float* map_b,
                           const float* map_c, const float* g_ssim, const float* g_l1, const int64_t* kept,
                           float* grad1, float* grad2, sc_stream_t stream) {
    if (!loss_sizes_ok(batch, channels, height, width, window)) return SC_EINVAL;
    if (!img1 || !img2 || !strides_host || (!grad1 && !grad2)) return SC_EINVAL;
    if (g_ssim && (!map_b || !map_c || (grad1 && !map_a1) || (grad2 && !map_a2))) return SC_EINVAL;
    if (g_l1 && !kept) return SC_EINVAL;
    LossImg X{img1, 0, 0, 0, 0}, Y{img2, 0, 0, 0, 0};
    LossMask M{mask, 0, 0, 0};
    if (!loss_views(strides_host, batch, channels, height, width, mask_batch, mask_height, mask_width, mask != nullptr,
                    &X, &Y, &M))
        return SC_EINVAL;
    const dim3 grid((unsigned)loss_tiles(height, width), (unsigned)batch);
    const int tx = loss_tiles_x(width);
    if (grad1 && grad2)
        hipLaunchKernelGGL(loss_bwd_kernel<3>, grid, dim3(LOSS_NT), 0, sc_s(stream), X, Y, M, channels, height, width, tx,
                           map_a1, map_a2, map_b, map_c, g_ssim, g_l1, kept, grad1, grad2);
    else if (grad1)
        hipLaunchKernelGGL(loss_bwd_kernel<1>, grid, dim3(LOSS_NT), 0, sc_s(stream), X, Y, M, channels, height, width, tx,
                           map_a1, map_a2, map_b, map_c, g_ssim, g_l1, kept, grad1, grad2);
    else
        hipLaunchKernelGGL(loss_bwd_kernel<2>, grid, dim3(LOSS_NT), 0, sc_s(stream), X, Y, M, channels, height, width, tx,
                           map_a1, map_a2, map_b, map_c, g_ssim, g_l1, kept, grad1, grad2);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
