// The convolution stack of the perceptual loss (include/street_crafter_amd.h, "perceptual loss: the convolution stack"):
// convolution + bias + ReLU as an implicit GEMM on the f32-input MFMA, its data gradient (the same kernel over a second
// packed form of the weights for stride 1, a VALU gather for a strided convolution), max-pool forward and backward.
//
// CONVOLUTION.  y[n][p] = sum_k Wp[k][n] * X[k][p] with p = oy * OW + ox an output pixel, n an output channel and
// k = (c * kh + ky) * kw + kx; X[k][p] = x[c][oy * sy - py + ky][ox * sx - px + kx], 0 outside the image: the im2col
// matrix is never stored, a workgroup gathers its BK x BM slice of it into LDS.  Wp is the weight tensor packed once per
// criterion: K-major [Kp][Np] (Kp = K rounded up to CONV_BK, Np = N rounded up to 128, zero filled), followed by one
// int32 per k that holds (c << 16 | ky << 8 | kx), -1 for the filled rows (never loaded, so they add exact zeros): no
// division in the K loop and no bounds check on the weight loads.  A thread gathers one pixel for the whole K loop.
// The data gradient of a stride-1 convolution is the same sum over the packed form with the channel roles swapped and
// the taps flipped, padding k - 1 - p; its gather multiplies by the ReLU mask.
//
// Tiles: 256 threads = 2 x 2 waves; a wave holds FN x FM accumulators of v_mfma_f32_16x16x4_f32 (16 output channels x
// 16 pixels each; at least 4 independent ones, which keeps the matrix core's issue rate), a workgroup
// BN = 32 FN channels x BM = 32 FM pixels.  The weights are the MFMA's A operand (rows = channels) and the pixels its B
// operand (columns), so that the 16 lanes of an accumulator register hold 16 CONSECUTIVE pixels of one channel and the
// epilogue's stores are 64-byte runs of the [C,h,w] planes the head kernel reads.  The shipped tile is 64 x 64 (FN = FM =
// 2): measured fastest on all five AlexNet layers at 1600 x 1066, forward and data gradient, against 64 x 128, 128 x 64
// and 128 x 128, and it gives the 65 x 99 layers 404 to 606 workgroups for 256 CUs.
// LDS rows are padded by 16 words: the 4 x 16 words a fragment load touches lie in 64 different banks.
// The next K slice is loaded into registers while the current one is multiplied (one LDS buffer, two barriers a slice).
//
// ROUNDING.  Every output element has ONE writer and a fixed order, so results repeat bit for bit.  What is promised
// about the sum itself is what the tests verify: float32 with ONE rounding per product-sum, in SOME fixed order over
// k = 0 .. Kp-1 (the MFMA's order over the 4 k of an instruction is the hardware's and is not relied upon; slices follow
// one another in k; the filled rows add exact zeros), hence within gamma(K) sum |x||w| of the exact sum, then
//     forward:   v = acc + bias[n]   (one rounded add, skipped without a bias),  then max(v, 0) when relu
//     dgrad:     v = acc + add[i]    (one rounded add, skipped without `add`: the tap's own gradient)
// The gather kernel runs its chain with fmaf in the order written above it (chunks of output channels, taps by
// increasing output position, the chunk's channels) and ends with the same single add.  The max-pool backward adds the
// (at most ceil(kh/sy) * ceil(kw/sx)) gradients of the windows that chose the element in increasing (oy, ox) order
// starting from +0, as torch's CPU kernel does, then `add`.
// No split of K across workgroups and no atomics anywhere: results are bit-identical from run to run.
//
// ReLU backward: an upstream gradient counts where the SAVED ReLU output is > 0 (torch's threshold rule), else it is +0.
// Max-pool: a window's value is the first maximum in row-major order under torch's comparison (v > best || isnan(v)); the
// backward recomputes it for every window that covers an element (in full: a scan that stops at the first value which
// rules the element out measured 1.4 times slower, its loads wait for one another), so no index tensor is stored.
#include "sc_common.h"
#include <math.h>

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CONV_THREADS = 256;
constexpr int CONV_BK = 32;
constexpr int CONV_NALIGN = 128;
constexpr int CONV_MAX_KERNEL = 11;
constexpr int CONV_MAX_STRIDE = 4;
constexpr int CONV_MAX_CHANNELS = 32767;       // (c << 16) stays positive in the k table
constexpr int POOL_MAX_KERNEL = 16;

struct ConvGeom {
    int C, H, W;          // the gathered operand: channels, rows, columns
    int N, OH, OW;        // the output: channels, rows, columns
    int kh, kw, sy, sx, py, px;
    int Kp, Np;
};

inline int conv_kp(int c, int kh, int kw) { return (c * kh * kw + CONV_BK - 1) / CONV_BK * CONV_BK; }
inline int conv_np(int n) { return (n + CONV_NALIGN - 1) / CONV_NALIGN * CONV_NALIGN; }

// weight [cout][cin][kh][kw] -> the packed form; dgrad: k runs over (cout, ky, kx), n over cin, taps flipped
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ w, int cin, int cout, int kh, int kw,
                                                        int dgrad, int K, int Kp, int Np, float* __restrict__ packed) {
    const int64_t total = (int64_t)Kp * Np;
    const int nc = dgrad ? cin : cout;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i / Np), n = (int)(i % Np);
        float v = 0.0f;
        if (k < K && n < nc) {
            const int c = k / (kh * kw), r = k % (kh * kw), ky = r / kw, kx = r % kw;
            v = dgrad ? w[(((int64_t)c * cin + n) * kh + (kh - 1 - ky)) * kw + (kw - 1 - kx)]
                      : w[(((int64_t)n * cin + c) * kh + ky) * kw + kx];
        }
        packed[i] = v;
        if (n == 0) {
            int e = -1;
            if (k < K) {
                const int c = k / (kh * kw), r = k % (kh * kw);
                e = (c << 16) | ((r / kw) << 8) | (r % kw);
            }
            reinterpret_cast<int*>(packed + total)[k] = e;
        }
    }
}

template <int FN, int FM>
__global__ __launch_bounds__(CONV_THREADS) void conv_mfma_kernel(
    const float* __restrict__ x, const float* __restrict__ mask, const float* __restrict__ packed,
    const float* __restrict__ bias, const float* __restrict__ add, ConvGeom g, int relu, float* __restrict__ y) {
    constexpr int BN = 32 * FN, BM = 32 * FM, BK = CONV_BK;
    constexpr int LDA = BN + 16, LDB = BM + 16;
    constexpr int NA = BK * BN / 4 / CONV_THREADS;          // float4 loads of the weight slice per thread
    constexpr int RS = CONV_THREADS / BM;                   // k rows the threads cover at once
    constexpr int NB = BK / RS;                             // gathered elements per thread
    __shared__ float As[BK * LDA];
    __shared__ float Bs[BK * LDB];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = g.OH * g.OW, HW = g.H * g.W;
    const int m0 = (int)blockIdx.x * BM, n0 = (int)blockIdx.y * BN;
    const int* __restrict__ ktab = reinterpret_cast<const int*>(packed + (size_t)g.Kp * g.Np);

    // the gather: one pixel per thread for the whole K loop
    const int pl = tid % BM;
    const int kr0 = __builtin_amdgcn_readfirstlane(tid / BM);
    const int p = m0 + pl;
    const bool p_ok = p < M;
    const int oy = p_ok ? p / g.OW : 0, ox = p_ok ? p % g.OW : 0;
    const int iy0 = oy * g.sy - g.py, ix0 = ox * g.sx - g.px;
    const int base = iy0 * g.W + ix0;

    float breg[NB];
    f32x4 areg[NA];
    auto load_slice = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int idx = tid + j * CONV_THREADS, k = idx / (BN / 4), n4 = idx % (BN / 4);
            areg[j] = *reinterpret_cast<const f32x4*>(packed + (size_t)(k0 + k) * g.Np + n0 + n4 * 4);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int e = ktab[k0 + kr0 + j * RS];                      // wave-uniform
            const int c = e >> 16, ky = (e >> 8) & 255, kx = e & 255;
            const bool ok = p_ok && e >= 0 && (unsigned)(iy0 + ky) < (unsigned)g.H && (unsigned)(ix0 + kx) < (unsigned)g.W;
            float v = 0.0f;
            if (ok) {
                const int off = c * HW + base + ky * g.W + kx;
                v = x[off];
                if (mask != nullptr && !(mask[off] > 0.0f)) v = 0.0f;
            }
            breg[j] = v;
        }
    };

    f32x4 acc[FN][FM];
#pragma unroll
    for (int a = 0; a < FN; ++a)
#pragma unroll
        for (int b = 0; b < FM; ++b) acc[a][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int wn0 = (wave >> 1) * (16 * FN), wm0 = (wave & 1) * (16 * FM);
    const int fr = lane >> 4, fc = lane & 15;

    if (g.Kp > 0) load_slice(0);
    for (int k0 = 0; k0 < g.Kp; k0 += BK) {
        __syncthreads();                                    // the previous slice has been read by every wave
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int idx = tid + j * CONV_THREADS, k = idx / (BN / 4), n4 = idx % (BN / 4);
            *reinterpret_cast<f32x4*>(&As[k * LDA + n4 * 4]) = areg[j];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) Bs[(kr0 + j * RS) * LDB + pl] = breg[j];
        __syncthreads();
        if (k0 + BK < g.Kp) load_slice(k0 + BK);            // in flight while this slice is multiplied
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            float a[FN], b[FM];
#pragma unroll
            for (int i = 0; i < FN; ++i) a[i] = As[(kk + fr) * LDA + wn0 + i * 16 + fc];
#pragma unroll
            for (int i = 0; i < FM; ++i) b[i] = Bs[(kk + fr) * LDB + wm0 + i * 16 + fc];
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
                for (int j = 0; j < FM; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // D: row (channel) = 4 (lane >> 4) + register, column (pixel) = lane & 15
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + wn0 + i * 16 + fr * 4 + r;
            if (n >= g.N) continue;
            const float bv = bias != nullptr ? bias[n] : 0.0f;
#pragma unroll
            for (int j = 0; j < FM; ++j) {
                const int q = m0 + wm0 + j * 16 + fc;
                if (q >= M) continue;
                float v = acc[i][j][r];
                if (bias != nullptr) v = v + bv;
                if (relu) v = v > 0.0f ? v : (v != v ? v : 0.0f);           // NaN passes, as in torch
                const int o = n * M + q;
                if (add != nullptr) v = v + add[o];
                y[o] = v;
            }
        }
}

// Data gradient by gather: one thread per input position (iy, ix) and GATHER_CH input channels, over the outputs
// (n, oy, ox) that read it.  A workgroup takes 256 positions of ONE phase (ty, tx) = ((iy + py) mod sy, (ix + px) mod sx):
// with u = iy + py = jy sy + ty the taps that reach the position are ky = ty + a sy, read at oy = jy - a, the same a for
// the whole workgroup.  So the trip counts are uniform, lanes with consecutive jx read consecutive ox, grad_out and the
// mask are read once for the thread's channels, and the phase's weights (at most ceil(kh/sy) ceil(kw/sx) taps) are staged
// in LDS per chunk of output channels, [tap][n][GATHER_CH], read back as one broadcast 16-byte word.
// Order of the chain: chunks of output channels upwards; inside a chunk the taps by increasing (oy, ox); inside a tap the
// chunk's channels upwards.
constexpr int GATHER_CH = 4;
constexpr int GATHER_LDS_BYTES = 48 * 1024;

__global__ __launch_bounds__(256) void conv_dgrad_gather_kernel(
    const float* __restrict__ go, const float* __restrict__ mask, const float* __restrict__ w,
    const float* __restrict__ add, ConvGeom g, int JH, int JW, int blocks_per_phase, int n_chunk, float* __restrict__ gi) {
    // here g.C, H, W describe grad_in (the convolution's input) and g.N, OH, OW grad_out
    extern __shared__ f32x4 wl[];                                    // [nky * nkx][n_chunk]
    const int phase = (int)blockIdx.x / blocks_per_phase;
    const int ty = phase / g.sx, tx = phase % g.sx;
    const int j = ((int)blockIdx.x % blocks_per_phase) * 256 + (int)threadIdx.x;
    const int c0 = (int)blockIdx.y * GATHER_CH;
    const int nky = ty < g.kh ? (g.kh - 1 - ty) / g.sy + 1 : 0, nkx = tx < g.kw ? (g.kw - 1 - tx) / g.sx + 1 : 0;
    const int jy = j / JW, jx = j % JW;
    const int iy = jy * g.sy + ty - g.py, ix = jx * g.sx + tx - g.px;
    const bool active = j < JH * JW && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;     // (no early return: barriers below)
    const int HW = g.H * g.W, OHW = g.OH * g.OW, KK = g.kh * g.kw;
    float acc[GATHER_CH];
#pragma unroll
    for (int q = 0; q < GATHER_CH; ++q) acc[q] = 0.0f;
    for (int nb0 = 0; nb0 < g.N; nb0 += n_chunk) {
        const int nb = g.N - nb0 < n_chunk ? g.N - nb0 : n_chunk;
        __syncthreads();                                             // the previous chunk has been read
        for (int t = (int)threadIdx.x; t < nky * nkx * nb * GATHER_CH; t += 256) {
            const int q = t % GATHER_CH, n = (t / GATHER_CH) % nb, tap = t / (GATHER_CH * nb);
            const int ky = ty + (tap / nkx) * g.sy, kx = tx + (tap % nkx) * g.sx;
            reinterpret_cast<float*>(wl)[(tap * n_chunk + n) * GATHER_CH + q] =
                c0 + q < g.C ? w[((size_t)(nb0 + n) * g.C + c0 + q) * KK + ky * g.kw + kx] : 0.0f;
        }
        __syncthreads();
        if (!active) continue;
        for (int a = nky - 1; a >= 0; --a) {                         // oy upwards
            const int oy = jy - a;
            if ((unsigned)oy >= (unsigned)g.OH) continue;
            for (int b = nkx - 1; b >= 0; --b) {                     // ox upwards
                const int ox = jx - b;
                if ((unsigned)ox >= (unsigned)g.OW) continue;
                const f32x4* wt = wl + (a * nkx + b) * n_chunk;
                const int o0 = nb0 * OHW + oy * g.OW + ox;
#pragma unroll 4
                for (int n = 0; n < nb; ++n) {
                    float v = go[o0 + n * OHW];
                    if (mask != nullptr && !(mask[o0 + n * OHW] > 0.0f)) v = 0.0f;
                    const f32x4 w4 = wt[n];
#pragma unroll
                    for (int q = 0; q < GATHER_CH; ++q) acc[q] = fmaf(v, w4[q], acc[q]);
                }
            }
        }
    }
    if (!active) return;
    const int at = iy * g.W + ix;
#pragma unroll
    for (int q = 0; q < GATHER_CH; ++q) {
        if (c0 + q >= g.C) break;
        const int o = (c0 + q) * HW + at;
        gi[o] = add != nullptr ? acc[q] + add[o] : acc[q];
    }
}

struct PoolGeom { int C, H, W, OH, OW, kh, kw, sy, sx; };

// the first maximum of window (oy, ox) of plane xp in row-major order -> its value, and its position iy * W + ix
__device__ __forceinline__ float pool_window(const float* __restrict__ xp, const PoolGeom& g, int oy, int ox, int& where) {
    const int y0 = oy * g.sy, x0 = ox * g.sx;
    float best = -INFINITY;
    where = y0 * g.W + x0;
    for (int dy = 0; dy < g.kh; ++dy)
        for (int dx = 0; dx < g.kw; ++dx) {
            const int at = (y0 + dy) * g.W + x0 + dx;
            const float v = xp[at];
            if (v > best || v != v) { best = v; where = at; }
        }
    return best;
}

__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, PoolGeom g, float* __restrict__ y) {
    const int OHW = g.OH * g.OW, total = g.C * OHW;
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= total) return;
    const int c = idx / OHW, rem = idx % OHW;
    int where;
    y[idx] = pool_window(x + (size_t)c * g.H * g.W, g, rem / g.OW, rem % g.OW, where);
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ go, const float* __restrict__ x,
                                                          const float* __restrict__ add, PoolGeom g, float* __restrict__ gi) {
    const int HW = g.H * g.W, total = g.C * HW;
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= total) return;
    const int c = idx / HW, rem = idx % HW, iy = rem / g.W, ix = rem % g.W;
    const float* xp = x + (size_t)c * HW;
    const float* gp = go + (size_t)c * g.OH * g.OW;
    // windows that cover the element: oy * sy <= iy <= oy * sy + kh - 1
    int oy_lo = iy - g.kh + 1 <= 0 ? 0 : (iy - g.kh + g.sy) / g.sy, oy_hi = iy / g.sy;
    int ox_lo = ix - g.kw + 1 <= 0 ? 0 : (ix - g.kw + g.sx) / g.sx, ox_hi = ix / g.sx;
    if (oy_hi > g.OH - 1) oy_hi = g.OH - 1;
    if (ox_hi > g.OW - 1) ox_hi = g.OW - 1;
    float acc = 0.0f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            int where;
            pool_window(xp, g, oy, ox, where);
            if (where == rem) acc = acc + gp[oy * g.OW + ox];
        }
    if (add != nullptr) acc = acc + add[idx];
    gi[idx] = acc;
}

// ---- host side -------------------------------------------------------------------------------------------------------
inline bool fits_i31(int64_t v) { return v >= 0 && v < ((int64_t)1 << 31); }

// 0: fine, with work; 1: fine, empty; < 0: rejected
int conv_check(int cin, int h, int w, int cout, int kh, int kw, int sy, int sx, int py, int px, int oh, int ow) {
    if (cin < 0 || h < 0 || w < 0 || cout < 0 || oh < 0 || ow < 0) return SC_EINVAL;
    if (kh < 1 || kw < 1 || kh > CONV_MAX_KERNEL || kw > CONV_MAX_KERNEL) return SC_EINVAL;
    if (sy < 1 || sx < 1 || sy > CONV_MAX_STRIDE || sx > CONV_MAX_STRIDE) return SC_EINVAL;
    if (py < 0 || px < 0 || py >= kh || px >= kw) return SC_EINVAL;
    if (cin > CONV_MAX_CHANNELS || cout > CONV_MAX_CHANNELS) return SC_EINVAL;
    if (cin == 0 || cout == 0 || h == 0 || w == 0) return (oh == 0 || ow == 0 || cin == 0 || cout == 0) ? 1 : SC_EINVAL;
    const int eh = h + 2 * py >= kh ? (h + 2 * py - kh) / sy + 1 : 0, ew = w + 2 * px >= kw ? (w + 2 * px - kw) / sx + 1 : 0;
    if (oh != eh || ow != ew) return SC_EINVAL;
    if (!fits_i31((int64_t)cin * h * w) || !fits_i31((int64_t)cout * oh * ow) || !fits_i31((int64_t)cin * cout * kh * kw))
        return SC_EINVAL;
    return (oh == 0 || ow == 0) ? 1 : 0;
}

size_t conv_pack_size(int kc, int nc, int kh, int kw) {
    const size_t kp = (size_t)conv_kp(kc, kh, kw), np = (size_t)conv_np(nc);
    return kp * np * sizeof(float) + kp * sizeof(int);
}

int conv_pack(const float* weight, int cin, int cout, int kh, int kw, int dgrad, void* packed, size_t bytes, sc_stream_t stream) {
    if (cin < 0 || cout < 0 || kh < 1 || kw < 1 || kh > CONV_MAX_KERNEL || kw > CONV_MAX_KERNEL) return SC_EINVAL;
    if (cin > CONV_MAX_CHANNELS || cout > CONV_MAX_CHANNELS) return SC_EINVAL;
    if (cin == 0 || cout == 0) return SC_OK;
    if (!weight || !packed || ((uintptr_t)packed & 15) != 0) return SC_EINVAL;
    const int kc = dgrad ? cout : cin, nc = dgrad ? cin : cout;
    if (!fits_i31((int64_t)conv_kp(kc, kh, kw) * conv_np(nc))) return SC_EINVAL;
    if (bytes < conv_pack_size(kc, nc, kh, kw)) return SC_EWORKSPACE;
    const int Kp = conv_kp(kc, kh, kw), Np = conv_np(nc);
    const int64_t total = (int64_t)Kp * Np;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, sc_s(stream), weight, cin, cout, kh, kw, dgrad,
                       kc * kh * kw, Kp, Np, reinterpret_cast<float*>(packed));
    SC_LAUNCH_CHECK();
    return SC_OK;
}

// the 64 x 64 tile everywhere (see the header)
void conv_launch(const float* x, const float* mask, const float* packed, const float* bias, const float* add,
                 const ConvGeom& g, int relu, float* y, hipStream_t s) {
    constexpr int FN = 2, FM = 2;
    const int M = g.OH * g.OW;
    const dim3 grid((unsigned)((M + 32 * FM - 1) / (32 * FM)), (unsigned)((g.N + 32 * FN - 1) / (32 * FN)));
    hipLaunchKernelGGL((conv_mfma_kernel<FN, FM>), grid, dim3(CONV_THREADS), 0, s, x, mask, packed, bias, add, g, relu, y);
}
}  // namespace

extern "C" size_t sc_conv_pack_bytes(int cin, int cout, int kh, int kw, int dgrad) {
    if (cin < 1 || cout < 1 || kh < 1 || kw < 1 || kh > CONV_MAX_KERNEL || kw > CONV_MAX_KERNEL) return 0;
    if (cin > CONV_MAX_CHANNELS || cout > CONV_MAX_CHANNELS) return 0;
    return dgrad ? conv_pack_size(cout, cin, kh, kw) : conv_pack_size(cin, cout, kh, kw);
}

extern "C" int sc_conv_pack_fwd(const float* weight, int cin, int cout, int kh, int kw, void* packed, size_t packed_bytes,
                                sc_stream_t stream) {
    return conv_pack(weight, cin, cout, kh, kw, 0, packed, packed_bytes, stream);
}

extern "C" int sc_conv_pack_dgrad(const float* weight, int cin, int cout, int kh, int kw, void* packed, size_t packed_bytes,
                                  sc_stream_t stream) {
    return conv_pack(weight, cin, cout, kh, kw, 1, packed, packed_bytes, stream);
}

extern "C" int sc_conv2d_relu_fwd(const float* x, const void* packed, size_t packed_bytes, const float* bias, int cin, int h,
                                  int w, int cout, int kh, int kw, int sy, int sx, int py, int px, int oh, int ow, int relu,
                                  float* y, sc_stream_t stream) {
    const int rc = conv_check(cin, h, w, cout, kh, kw, sy, sx, py, px, oh, ow);
    if (rc < 0) return rc;
    if (relu != 0 && relu != 1) return SC_EINVAL;
    if (rc == 1) return SC_OK;
    if (!x || !packed || !y || ((uintptr_t)packed & 15) != 0) return SC_EINVAL;
    if (packed_bytes < conv_pack_size(cin, cout, kh, kw)) return SC_EWORKSPACE;
    const ConvGeom g{cin, h, w, cout, oh, ow, kh, kw, sy, sx, py, px, conv_kp(cin, kh, kw), conv_np(cout)};
    conv_launch(x, nullptr, reinterpret_cast<const float*>(packed), bias, nullptr, g, relu, y, sc_s(stream));
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_conv2d_dgrad(const float* grad_out, const float* relu_out, const void* packed_dgrad, size_t packed_bytes,
                               const float* add, int cin, int h, int w, int cout, int kh, int kw, int py, int px, int oh,
                               int ow, float* grad_in, sc_stream_t stream) {
    const int rc = conv_check(cin, h, w, cout, kh, kw, 1, 1, py, px, oh, ow);
    if (rc < 0) return rc;
    if (cin == 0 || h == 0 || w == 0) return SC_OK;                 // no element of grad_in
    if (!grad_in) return SC_EINVAL;
    if (rc == 0) {
        if (!grad_out || !packed_dgrad || ((uintptr_t)packed_dgrad & 15) != 0) return SC_EINVAL;
        if (packed_bytes < conv_pack_size(cout, cin, kh, kw)) return SC_EWORKSPACE;
    }
    // the transposed convolution as a convolution of grad_out: channels swapped, padding k - 1 - p; an empty grad_out
    // (cout == 0 or no output position) leaves grad_in = add or +0, which the same kernel writes with Kp = 0
    const ConvGeom g{cout, oh, ow, cin, h, w, kh, kw, 1, 1, kh - 1 - py, kw - 1 - px,
                     (rc == 1 || cout == 0) ? 0 : conv_kp(cout, kh, kw), conv_np(cin)};
    conv_launch(grad_out, relu_out, reinterpret_cast<const float*>(packed_dgrad), nullptr, add, g, 0, grad_in, sc_s(stream));
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_conv2d_dgrad_strided(const float* grad_out, const float* relu_out, const float* weight, const float* add,
                                       int cin, int h, int w, int cout, int kh, int kw, int sy, int sx, int py, int px,
                                       int oh, int ow, float* grad_in, sc_stream_t stream) {
    const int rc = conv_check(cin, h, w, cout, kh, kw, sy, sx, py, px, oh, ow);
    if (rc < 0) return rc;
    if (cin == 0 || h == 0 || w == 0) return SC_OK;
    if (!grad_in) return SC_EINVAL;
    if (rc == 0 && (!grad_out || !weight)) return SC_EINVAL;
    const ConvGeom g{cin, h, w, rc == 1 ? 0 : cout, oh, ow, kh, kw, sy, sx, py, px, 0, 0};
    if (!fits_i31((int64_t)(h + py) * (w + px))) return SC_EINVAL;
    const int JH = (h + py - 1) / sy + 1, JW = (w + px - 1) / sx + 1, bpp = (JH * JW + 255) / 256;      // JH JW <= 2 h w
    // output channels per LDS chunk: the phase with the most taps has ceil(kh/sy) ceil(kw/sx) of them, 16 bytes each
    const int max_taps = ((kh + sy - 1) / sy) * ((kw + sx - 1) / sx);
    int n_chunk = GATHER_LDS_BYTES / (max_taps * (int)sizeof(f32x4));
    if (n_chunk > 64) n_chunk = 64;
    if (n_chunk > g.N) n_chunk = g.N > 0 ? g.N : 1;
    hipLaunchKernelGGL(conv_dgrad_gather_kernel, dim3((unsigned)(sy * sx * bpp), (unsigned)((cin + GATHER_CH - 1) / GATHER_CH)),
                       dim3(256), (size_t)max_taps * n_chunk * sizeof(f32x4), sc_s(stream), grad_out, relu_out, weight, add, g,
                       JH, JW, bpp, n_chunk, grad_in);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

static int pool_check(int c, int h, int w, int kh, int kw, int sy, int sx, int oh, int ow) {
    if (c < 0 || h < 0 || w < 0 || oh < 0 || ow < 0) return SC_EINVAL;
    if (kh < 1 || kw < 1 || kh > POOL_MAX_KERNEL || kw > POOL_MAX_KERNEL || sy < 1 || sx < 1) return SC_EINVAL;
    const int eh = h >= kh ? (h - kh) / sy + 1 : 0, ew = w >= kw ? (w - kw) / sx + 1 : 0;
    if (oh != eh || ow != ew) return SC_EINVAL;
    if (!fits_i31((int64_t)c * h * w)) return SC_EINVAL;
    return SC_OK;
}

extern "C" int sc_maxpool2d_fwd(const float* x, int channels, int h, int w, int kh, int kw, int sy, int sx, int oh, int ow,
                                float* y, sc_stream_t stream) {
    const int rc = pool_check(channels, h, w, kh, kw, sy, sx, oh, ow);
    if (rc != SC_OK) return rc;
    const int64_t total = (int64_t)channels * oh * ow;
    if (total == 0) return SC_OK;
    if (!x || !y) return SC_EINVAL;
    const PoolGeom g{channels, h, w, oh, ow, kh, kw, sy, sx};
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, sc_s(stream), x, g, y);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_maxpool2d_bwd(const float* grad_out, const float* x, const float* add, int channels, int h, int w, int kh,
                                int kw, int sy, int sx, int oh, int ow, float* grad_in, sc_stream_t stream) {
    const int rc = pool_check(channels, h, w, kh, kw, sy, sx, oh, ow);
    if (rc != SC_OK) return rc;
    const int64_t total = (int64_t)channels * h * w;
    if (total == 0) return SC_OK;
    if (!x || !grad_in || (!grad_out && oh > 0 && ow > 0)) return SC_EINVAL;
    const PoolGeom g{channels, h, w, oh, ow, kh, kw, sy, sx};
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, sc_s(stream), grad_out, x, add,
                       g, grad_in);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
