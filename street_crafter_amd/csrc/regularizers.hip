// Regularizers of the training step (train.py:194-220): the trimmed LiDAR depth loss and the sky / object accumulation
// losses, each with its backward.  Nothing here synchronises with the host, and every result is bit-identical from run to
// run: float sums go to a per-block slab (double) that one finalize block adds in a fixed order; the only atomics are
// integer histogram counts, whose result does not depend on arrival order.
//
// Pixel -> block map (all kernels): block b owns the row-major pixels [b * RG_CHUNK, (b + 1) * RG_CHUNK), visited as
// RG_PPT rounds of RG_NT consecutive pixels.  It depends on H and W only, so the backward can rebuild a tie's row-major rank.
//
// LiDAR depth loss (train.py:211-218).  kept = (lidar > 0) && mask, e = fabsf(depth - lidar) in fp32, n = #kept,
// k = (long long)(keep * (double)n): Python's int(0.95 * n).  The value is the mean of the k smallest e (NaN above +inf).
//   dt_key_kernel     one u32 key per pixel into the workspace: the bits of e (non-negative floats order as unsigned
//                     integers), RG_KEY_NAN for every NaN, RG_KEY_OUT for a pixel that is not kept; plus the histogram of
//                     the top 11 key bits (LDS, merged into the global one with integer atomics)
//   dt_select_kernel  one block: the digit that holds rank k - 1; keeps {n, k, prefix, below, rank} in DtState
//   dt_hist_kernel    the next 11 / 10 bits of the keys that match the prefix so far
//   dt_sum_kernel     per block: the double sum of e < t and the count of e == t (t = the k-th smallest key)
//   dt_finalize_kernel  value = (sum_below + (k - below) t) / k in double, rounded once; the exclusive prefix of the
//                     per-block tie counts for the backward
// Tie rule: every pixel with e < t is selected, then the first k - below pixels with e == t in row-major order.
// Backward: grad_depth = 0 + sign(d - l) * (g * (1 / (float)k)) on the selected pixels, +0 elsewhere; grad_lidar the
// negation.  That is torch's MeanBackward (a division by a scalar, which its GPU kernel runs as a multiplication by the
// reciprocal) -> TopK scatter -> Abs (grad * sgn) -> index_put(accumulate) into zeros, op for op in fp32.
//
// Accumulation losses (train.py:194-196 sky, 205-206 object): a = clamp(acc, 1e-6f, 0x1.ffffdep-1f) (NaN passes), per
// mask channel c: sel_c ? -log(1 - a) : -(a log a + (1 - a) log(1 - a)) for the sky loss, the branches swapped for the
// object loss; the mean over Cm * H * W.  Backward: g / (Cm H W) * sum_c (log-branch ? 1 / (1 - a) : log(1 - a) - log a),
// evaluated in double and rounded once, zero outside the inclusive clamp range (torch's clamp_backward).
#include "sc_common.h"

namespace {

constexpr int RG_NT = 256;
constexpr int RG_PPT = 8;                            // pixels per thread
constexpr int RG_CHUNK = RG_NT * RG_PPT;             // pixels per block
constexpr uint32_t RG_KEY_NAN = 0x7F800001u;         // every NaN error: one key above +inf (0x7F800000)
constexpr uint32_t RG_KEY_OUT = 0xFFFFFFFFu;         // a pixel that is not kept (above every kept key)
constexpr int RG_HIST_WORDS = 2048 + 2048 + 1024;    // the three digit histograms, side by side
constexpr float AR_LO = 1e-6f;                       // (float)1e-6 and (float)(1 - 1e-6): torch.clamp's fp32 bounds
constexpr float AR_HI = 0x1.ffffdep-1f;

__host__ __device__ constexpr int rg_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ constexpr int rg_bins(int pass) { return pass == 2 ? 1024 : 2048; }
__host__ __device__ constexpr int rg_hist_off(int pass) { return pass == 0 ? 0 : (pass == 1 ? 2048 : 4096); }

struct RgView {             // element (y, x) at p[y * sh + x * sw]
    const float* p;
    int64_t sh, sw;
};
struct RgMask {             // element (c, y, x) at p[c * sc + y * sh + x * sw]; p null = every pixel kept
    const uint8_t* p;
    int64_t sc, sh, sw;
};

struct DtState {
    long long n;            // kept pixels
    long long k;            // how many of them the loss averages
    long long below;        // kept pixels whose key is below the current bucket
    unsigned int prefix;    // the key bits fixed so far; after the last pass, the k-th smallest key t
    unsigned int rank;      // rank of the k-th smallest key inside the current bucket
    int done;               // k == 0: nothing is selected, the value is NaN
    int pad;
};

// workspace of the depth loss: state | histograms | slab | tie counts | tie offsets | keys
struct DtLayout {
    size_t state, hist, slab, tcnt, toff, keys, total;
    int nblk;
    DtLayout(int H, int W) {
        const int64_t P = (int64_t)H * W;
        nblk = (int)((P + RG_CHUNK - 1) / RG_CHUNK);
        state = 0;
        hist = 256;
        slab = hist + sc_align_up(RG_HIST_WORDS * sizeof(uint32_t), 256);
        tcnt = slab + sc_align_up((size_t)nblk * sizeof(double), 256);
        toff = tcnt + sc_align_up((size_t)nblk * sizeof(uint32_t), 256);
        keys = toff + sc_align_up((size_t)nblk * sizeof(uint32_t), 256);
        total = keys + (size_t)P * sizeof(uint32_t);
    }
};

__device__ __forceinline__ double rg_block_sum(double v, double* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < RG_NT / 64; ++w) t += red[w];
    return t;
}

__device__ __forceinline__ long long rg_block_sum_i(long long v, long long* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = 0;
#pragma unroll
    for (int w = 0; w < RG_NT / 64; ++w) t += red[w];
    return t;
}

// inclusive block scan (256 threads) of a non-negative count; *total = the block's sum
__device__ __forceinline__ long long rg_block_scan(long long v, long long* red, long long* total) {
    long long s = sc_wave_incl_scan64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = s;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RG_NT / 64; ++w) {
        if (w < (int)(threadIdx.x >> 6)) before += red[w];
        all += red[w];
    }
    *total = all;
    return s + before;
}

// row and column of pixel p (H * W < 2^31: a 32-bit division, not the 64-bit one the compiler emulates)
__device__ __forceinline__ void rg_yx(int64_t p, int W, int* y, int* x) {
    const uint32_t pu = (uint32_t)p, r = pu / (uint32_t)W;
    *y = (int)r;
    *x = (int)(pu - r * (uint32_t)W);
}

__device__ __forceinline__ bool rg_kept(const RgMask& m, int c, int y, int x) {
    return m.p == nullptr || m.p[(int64_t)c * m.sc + (int64_t)y * m.sh + (int64_t)x * m.sw] != 0;
}

// the key of pixel (y, x), and its fp32 difference d - l (the sign source of the backward)
__device__ __forceinline__ uint32_t dt_key(const RgView& D, const RgView& L, const RgMask& M, int y, int x, float* diff) {
    const float l = L.p[(int64_t)y * L.sh + (int64_t)x * L.sw];
    const bool kept = (l > 0.0f) && rg_kept(M, 0, y, x);      // (NaN > 0 is false)
    if (!kept) {
        *diff = 0.0f;
        return RG_KEY_OUT;
    }
    const float df = D.p[(int64_t)y * D.sh + (int64_t)x * D.sw] - l;
    *diff = df;
    const float e = fabsf(df);
    return (e != e) ? RG_KEY_NAN : __float_as_uint(e);
}

// grid (nblk): keys of every pixel, histogram of the top digit
__global__ __launch_bounds__(RG_NT) void dt_key_kernel(RgView D, RgView L, RgMask M, int H, int W,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[rg_bins(0)];
    for (int i = threadIdx.x; i < rg_bins(0); i += RG_NT) h[i] = 0u;
    __syncthreads();
    const int64_t P = (int64_t)H * W, base = (int64_t)blockIdx.x * RG_CHUNK;
#pragma unroll
    for (int j = 0; j < RG_PPT; ++j) {
        const int64_t p = base + j * RG_NT + threadIdx.x;
        if (p < P) {
            int y, x;
            rg_yx(p, W, &y, &x);
            float df;
            const uint32_t key = dt_key(D, L, M, y, x, &df);
            keys[p] = key;
            if (key != RG_KEY_OUT) atomicAdd(&h[key >> rg_shift(0)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rg_bins(0); i += RG_NT)
        if (h[i]) atomicAdd(&hist[rg_hist_off(0) + i], h[i]);
}

// grid (nblk), PASS 1 or 2: histogram of digit PASS over the keys whose higher bits equal the prefix so far
template <int PASS>
__global__ __launch_bounds__(RG_NT) void dt_hist_kernel(const uint32_t* __restrict__ keys, int64_t P,
                                                        const DtState* __restrict__ st, uint32_t* __restrict__ hist) {
    constexpr int NB = rg_bins(PASS), HS = rg_shift(PASS - 1);
    __shared__ uint32_t h[NB];
    if (st->done) return;                           // (uniform over the grid)
    const uint32_t want = st->prefix >> HS;
    for (int i = threadIdx.x; i < NB; i += RG_NT) h[i] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RG_CHUNK;
#pragma unroll
    for (int j = 0; j < RG_PPT; ++j) {
        const int64_t p = base + j * RG_NT + threadIdx.x;
        if (p < P) {
            const uint32_t key = keys[p];           // (RG_KEY_OUT never matches: a kept key has its top bit clear)
            if ((key >> HS) == want) atomicAdd(&h[(key >> rg_shift(PASS)) & (NB - 1)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NB; i += RG_NT)
        if (h[i]) atomicAdd(&hist[rg_hist_off(PASS) + i], h[i]);
}

// one block: the digit of pass PASS that holds rank k - 1.  Pass 0 also sets n and k.
template <int PASS>
__global__ __launch_bounds__(RG_NT) void dt_select_kernel(const uint32_t* __restrict__ hist, DtState* __restrict__ st,
                                                          double keep) {
    constexpr int NB = rg_bins(PASS), PER = NB / RG_NT;
    __shared__ long long red[RG_NT / 64];
    __shared__ long long s_below;
    __shared__ unsigned int s_digit, s_rank;
    uint32_t c[PER];
    long long mine = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        c[i] = hist[rg_hist_off(PASS) + threadIdx.x * PER + i];
        mine += c[i];
    }
    long long total;
    const long long incl = rg_block_scan(mine, red, &total), excl = incl - mine;
    long long n, k, below;
    unsigned int prefix;
    long long rank;
    int done;
    if (PASS == 0) {
        n = total;
        k = (long long)(keep * (double)n);          // Python's int(keep * n): a double product, truncated
        done = k == 0;
        below = 0;
        prefix = 0u;
        rank = k - 1;
    } else {
        n = st->n; k = st->k; below = st->below; prefix = st->prefix; rank = st->rank; done = st->done;
        if (done) return;
    }
    if (threadIdx.x == 0) { s_below = 0; s_digit = 0u; s_rank = 0u; }
    __syncthreads();
    if (!done && excl <= rank && rank < incl) {     // exactly one thread holds the rank
        long long r = rank - excl;
        int d = (int)threadIdx.x * PER;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (r < (long long)c[i]) break;
            r -= c[i];
            ++d;
        }
        s_digit = (unsigned int)d;
        s_rank = (unsigned int)r;
        s_below = rank - r;                         // keys of this bucket in lower digits
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        DtState o;
        o.n = n; o.k = k; o.done = done; o.pad = 0;
        o.below = below + s_below;
        o.prefix = prefix | (s_digit << rg_shift(PASS));
        o.rank = s_rank;
        *st = o;
    }
}

// grid (nblk): slab[b] = sum of e over the keys below t, tcnt[b] = how many keys equal t
__global__ __launch_bounds__(RG_NT) void dt_sum_kernel(const uint32_t* __restrict__ keys, int64_t P,
                                                       const DtState* __restrict__ st, double* __restrict__ slab,
                                                       uint32_t* __restrict__ tcnt) {
    __shared__ double red[RG_NT / 64];
    __shared__ long long redi[RG_NT / 64];
    const bool done = st->done != 0;
    const uint32_t t = st->prefix;
    double s = 0.0;
    long long ties = 0;
    const int64_t base = (int64_t)blockIdx.x * RG_CHUNK;
    if (!done) {
#pragma unroll
        for (int j = 0; j < RG_PPT; ++j) {
            const int64_t p = base + j * RG_NT + threadIdx.x;
            if (p < P) {
                const uint32_t key = keys[p];
                if (key < t) s += (double)__uint_as_float(key);
                else if (key == t) ++ties;
            }
        }
    }
    s = rg_block_sum(s, red);
    ties = rg_block_sum_i(ties, redi);
    if (threadIdx.x == 0) {
        slab[blockIdx.x] = s;
        tcnt[blockIdx.x] = (uint32_t)ties;
    }
}

// one block: the value (NaN when k == 0), the threshold, {n, k, below}; toff[b] = ties in blocks before b
__global__ __launch_bounds__(RG_NT) void dt_finalize_kernel(const double* __restrict__ slab,
                                                            const uint32_t* __restrict__ tcnt,
                                                            uint32_t* __restrict__ toff, int nblk,
                                                            const DtState* __restrict__ st, float* __restrict__ value,
                                                            float* __restrict__ threshold, int64_t* __restrict__ counts) {
    __shared__ double red[RG_NT / 64];
    __shared__ long long redi[RG_NT / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += RG_NT) s += slab[i];
    s = rg_block_sum(s, red);
    // exclusive prefix of the tie counts: thread i owns the contiguous blocks [i * per, (i + 1) * per)
    const int per = (nblk + RG_NT - 1) / RG_NT;
    const int b0 = (int)threadIdx.x * per, b1 = min(nblk, b0 + per);
    long long mine = 0;
    for (int b = b0; b < b1; ++b) mine += tcnt[b];
    long long total;
    long long run = rg_block_scan(mine, redi, &total) - mine;
    for (int b = b0; b < b1; ++b) {
        toff[b] = (uint32_t)run;
        run += tcnt[b];
    }
    if (threadIdx.x == 0) {
        const DtState q = *st;
        const uint32_t t = q.prefix;
        const float tf = (t == RG_KEY_NAN || q.done) ? __builtin_nanf("") : __uint_as_float(t);
        value[0] = q.done ? __builtin_nanf("") : (float)((s + (double)(q.k - q.below) * (double)tf) / (double)q.k);
        if (threshold) threshold[0] = tf;
        if (counts) {
            counts[0] = q.n;
            counts[1] = q.k;
            counts[2] = q.below;
        }
    }
}

// grid (nblk): the gradient of the selected pixels, +0 elsewhere (gd / gl contiguous [H, W], either nullable)
__global__ __launch_bounds__(RG_NT) void dt_bwd_kernel(RgView D, RgView L, RgMask M, int H, int W,
                                                       const DtState* __restrict__ st, const uint32_t* __restrict__ tcnt,
                                                       const uint32_t* __restrict__ toff, const float* __restrict__ g,
                                                       float* __restrict__ gd, float* __restrict__ gl) {
    __shared__ uint32_t wtot[RG_NT / 64];
    const DtState q = *st;
    const bool done = q.done != 0;
    const uint32_t t = q.prefix;
    const float gk = done ? 0.0f : g[0] * (1.0f / (float)q.k);
    // ties this block takes: the first `take` of its own, in row-major order (block-uniform)
    const long long cnt = tcnt[blockIdx.x], need = done ? 0 : q.k - q.below - (long long)toff[blockIdx.x];
    const long long take = need < 0 ? 0 : (need > cnt ? cnt : need);
    const bool rank_ties = take > 0 && take < cnt;
    const int lane = sc_lane(), wave = (int)(threadIdx.x >> 6);
    const int64_t P = (int64_t)H * W, base = (int64_t)blockIdx.x * RG_CHUNK;
    long long run = 0;
    for (int j = 0; j < RG_PPT; ++j) {
        const int64_t p = base + j * RG_NT + threadIdx.x;
        const bool valid = p < P;
        uint32_t key = RG_KEY_OUT;
        float df = 0.0f;
        if (valid) {
            int y, x;
            rg_yx(p, W, &y, &x);
            key = dt_key(D, L, M, y, x, &df);
        }
        const bool tie = !done && key == t;
        bool sel = !done && key < t;
        if (rank_ties) {
            const unsigned long long bal = __ballot(tie);
            const long long in_wave = __popcll(bal & sc_lanemask_lt());
            if (lane == 0) wtot[wave] = (uint32_t)__popcll(bal);
            __syncthreads();
            long long before = run, all = 0;
#pragma unroll
            for (int w = 0; w < RG_NT / 64; ++w) {
                if (w < wave) before += wtot[w];
                all += wtot[w];
            }
            __syncthreads();
            sel = sel || (tie && before + in_wave < take);
            run += all;
        } else {
            sel = sel || (tie && take == cnt);
        }
        if (valid) {
            const float sgn = (df > 0.0f) ? 1.0f : ((df < 0.0f) ? -1.0f : 0.0f);
            const float v = gk * sgn;
            if (gd) gd[p] = sel ? 0.0f + v : 0.0f;
            if (gl) gl[p] = sel ? 0.0f + (-v) : 0.0f;
        }
    }
}

// ---- accumulation losses ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ar_clamp(float a) { return (a != a) ? a : fminf(fmaxf(a, AR_LO), AR_HI); }

// per pixel: the log branch -log(1 - a) and the entropy branch, op for op as torch forms them (no contraction)
__device__ __forceinline__ void ar_terms(float a, float* lg, float* ent) {
#pragma clang fp contract(off)
    const float la = logf(a), t1 = 1.0f - a, l1 = logf(t1);
    *lg = -l1;
    *ent = -(a * la + t1 * l1);
}

// grid (nblk): slab[b] = sum over the block's pixels and the Cm mask channels of the selected branch (double)
__global__ __launch_bounds__(RG_NT) void ar_fwd_kernel(RgView A, RgMask M, int Cm, int H, int W, int mode,
                                                       double* __restrict__ slab) {
    __shared__ double red[RG_NT / 64];
    const int64_t P = (int64_t)H * W, base = (int64_t)blockIdx.x * RG_CHUNK;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < RG_PPT; ++j) {
        const int64_t p = base + j * RG_NT + threadIdx.x;
        if (p < P) {
            int y, x;
            rg_yx(p, W, &y, &x);
            const float a = ar_clamp(A.p[(int64_t)y * A.sh + (int64_t)x * A.sw]);
            float lg, ent;
            ar_terms(a, &lg, &ent);
            for (int c = 0; c < Cm; ++c) {
                const bool m = rg_kept(M, c, y, x);
                // sky (mode 0): True -> the log branch; object (mode 1): True -> the entropy branch
                s += (double)((m != (mode == 1)) ? lg : ent);
            }
        }
    }
    s = rg_block_sum(s, red);
    if (threadIdx.x == 0) slab[blockIdx.x] = s;
}

// one block: value = sum of the slab (fixed order) / n_total, rounded once
__global__ __launch_bounds__(RG_NT) void ar_finalize_kernel(const double* __restrict__ slab, int nblk, double n_total,
                                                            float* __restrict__ value) {
    __shared__ double red[RG_NT / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += RG_NT) s += slab[i];
    s = rg_block_sum(s, red);
    if (threadIdx.x == 0) value[0] = (float)(s / n_total);
}

// grid (nblk): ga [H, W] contiguous
__global__ __launch_bounds__(RG_NT) void ar_bwd_kernel(RgView A, RgMask M, int Cm, int H, int W, int mode,
                                                       double n_total, const float* __restrict__ g,
                                                       float* __restrict__ ga) {
    const double gs = (double)g[0] / n_total;
    const int64_t P = (int64_t)H * W, base = (int64_t)blockIdx.x * RG_CHUNK;
#pragma unroll
    for (int j = 0; j < RG_PPT; ++j) {
        const int64_t p = base + j * RG_NT + threadIdx.x;
        if (p < P) {
            int y, x;
            rg_yx(p, W, &y, &x);
            const float raw = A.p[(int64_t)y * A.sh + (int64_t)x * A.sw];
            const bool pass = raw >= AR_LO && raw <= AR_HI;        // clamp_backward: inclusive, NaN -> 0
            int n_log = 0;
            for (int c = 0; c < Cm; ++c) n_log += (rg_kept(M, c, y, x) != (mode == 1)) ? 1 : 0;
            // (in double, rounded once: a and 1 - a are exact fp32 values)
            const float a = ar_clamp(raw), t1 = 1.0f - a;
            const double d = (double)n_log / (double)t1 + (double)(Cm - n_log) * (log((double)t1) - log((double)a));
            ga[p] = pass ? (float)(gs * d) : 0.0f;
        }
    }
}

bool rg_sizes_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < (1ll << 31); }
bool rg_strides_ok(const int64_t* st, int n) {
    for (int i = 0; i < n; ++i)
        if (st[i] < 0) return false;
    return true;
}
inline int rg_blocks(int H, int W) { return (int)(((int64_t)H * W + RG_CHUNK - 1) / RG_CHUNK); }

}  // namespace

extern "C" size_t sc_depth_trim_workspace_bytes(int height, int width) {
    if (!rg_sizes_ok(height, width)) return 0;
    return DtLayout(height, width).total;
}

extern "C" int sc_depth_trim_fwd(const float* depth, const float* lidar_depth, const uint8_t* mask,
                                 const int64_t* strides_host, int height, int width, double keep, float* value_out,
                                 float* threshold_out, int64_t* counts_out, void* workspace, size_t workspace_bytes,
                                 sc_stream_t stream) {
    if (!rg_sizes_ok(height, width)) return SC_EINVAL;
    if (!depth || !lidar_depth || !strides_host || !value_out || !workspace) return SC_EINVAL;
    if (!(keep > 0.0 && keep <= 1.0)) return SC_EINVAL;
    if (!rg_strides_ok(strides_host, 6)) return SC_EINVAL;
    if (workspace_bytes < sc_depth_trim_workspace_bytes(height, width)) return SC_EWORKSPACE;
    const DtLayout Lw(height, width);
    char* ws = static_cast<char*>(workspace);
    DtState* st = reinterpret_cast<DtState*>(ws + Lw.state);
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + Lw.hist);
    double* slab = reinterpret_cast<double*>(ws + Lw.slab);
    uint32_t* tcnt = reinterpret_cast<uint32_t*>(ws + Lw.tcnt);
    uint32_t* toff = reinterpret_cast<uint32_t*>(ws + Lw.toff);
    uint32_t* keys = reinterpret_cast<uint32_t*>(ws + Lw.keys);
    const RgView D{depth, strides_host[0], strides_host[1]}, L{lidar_depth, strides_host[2], strides_host[3]};
    const RgMask M{mask, 0, strides_host[4], strides_host[5]};
    const int64_t P = (int64_t)height * width;
    const hipStream_t s = sc_s(stream);
    SC_HIP(hipMemsetAsync(hist, 0, RG_HIST_WORDS * sizeof(uint32_t), s));
    hipLaunchKernelGGL(dt_key_kernel, dim3(Lw.nblk), dim3(RG_NT), 0, s, D, L, M, height, width, keys, hist);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(dt_select_kernel<0>, dim3(1), dim3(RG_NT), 0, s, hist, st, keep);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(dt_hist_kernel<1>, dim3(Lw.nblk), dim3(RG_NT), 0, s, keys, P, st, hist);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(dt_select_kernel<1>, dim3(1), dim3(RG_NT), 0, s, hist, st, keep);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(dt_hist_kernel<2>, dim3(Lw.nblk), dim3(RG_NT), 0, s, keys, P, st, hist);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(dt_select_kernel<2>, dim3(1), dim3(RG_NT), 0, s, hist, st, keep);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(dt_sum_kernel, dim3(Lw.nblk), dim3(RG_NT), 0, s, keys, P, st, slab, tcnt);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(dt_finalize_kernel, dim3(1), dim3(RG_NT), 0, s, slab, tcnt, toff, Lw.nblk, st, value_out,
                       threshold_out, counts_out);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_depth_trim_bwd(const float* depth, const float* lidar_depth, const uint8_t* mask,
                                 const int64_t* strides_host, int height, int width, const float* grad_value,
                                 const void* workspace, size_t workspace_bytes, float* grad_depth, float* grad_lidar,
                                 sc_stream_t stream) {
    if (!rg_sizes_ok(height, width)) return SC_EINVAL;
    if (!depth || !lidar_depth || !strides_host || !grad_value || !workspace || (!grad_depth && !grad_lidar))
        return SC_EINVAL;
    if (!rg_strides_ok(strides_host, 6)) return SC_EINVAL;
    if (workspace_bytes < sc_depth_trim_workspace_bytes(height, width)) return SC_EWORKSPACE;
    const DtLayout Lw(height, width);
    const char* ws = static_cast<const char*>(workspace);
    const RgView D{depth, strides_host[0], strides_host[1]}, L{lidar_depth, strides_host[2], strides_host[3]};
    const RgMask M{mask, 0, strides_host[4], strides_host[5]};
    hipLaunchKernelGGL(dt_bwd_kernel, dim3(Lw.nblk), dim3(RG_NT), 0, sc_s(stream), D, L, M, height, width,
                       reinterpret_cast<const DtState*>(ws + Lw.state), reinterpret_cast<const uint32_t*>(ws + Lw.tcnt),
                       reinterpret_cast<const uint32_t*>(ws + Lw.toff), grad_value, grad_depth, grad_lidar);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" size_t sc_acc_reg_workspace_bytes(int height, int width) {
    if (!rg_sizes_ok(height, width)) return 0;
    return (size_t)rg_blocks(height, width) * sizeof(double);
}

extern "C" int sc_acc_reg_fwd(const float* acc, const uint8_t* mask, const int64_t* strides_host, int mask_channels,
                              int height, int width, int mode, float* value_out, void* workspace,
                              size_t workspace_bytes, sc_stream_t stream) {
    if (!rg_sizes_ok(height, width) || mask_channels < 1 || (mode != 0 && mode != 1)) return SC_EINVAL;
    if (!acc || !mask || !strides_host || !value_out || !workspace) return SC_EINVAL;
    if (!rg_strides_ok(strides_host, 5)) return SC_EINVAL;
    if (workspace_bytes < sc_acc_reg_workspace_bytes(height, width)) return SC_EWORKSPACE;
    const RgView A{acc, strides_host[0], strides_host[1]};
    const RgMask M{mask, strides_host[2], strides_host[3], strides_host[4]};
    const int nblk = rg_blocks(height, width);
    const double n_total = (double)mask_channels * height * width;
    double* slab = static_cast<double*>(workspace);
    hipLaunchKernelGGL(ar_fwd_kernel, dim3(nblk), dim3(RG_NT), 0, sc_s(stream), A, M, mask_channels, height, width, mode,
                       slab);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(ar_finalize_kernel, dim3(1), dim3(RG_NT), 0, sc_s(stream), slab, nblk, n_total, value_out);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_acc_reg_bwd(const float* acc, const uint8_t* mask, const int64_t* strides_host, int mask_channels,
                              int height, int width, int mode, const float* grad_value, float* grad_acc,
                              sc_stream_t stream) {
    if (!rg_sizes_ok(height, width) || mask_channels < 1 || (mode != 0 && mode != 1)) return SC_EINVAL;
    if (!acc || !mask || !strides_host || !grad_value || !grad_acc) return SC_EINVAL;
    if (!rg_strides_ok(strides_host, 5)) return SC_EINVAL;
    const RgView A{acc, strides_host[0], strides_host[1]};
    const RgMask M{mask, strides_host[2], strides_host[3], strides_host[4]};
    const double n_total = (double)mask_channels * height * width;
    hipLaunchKernelGGL(ar_bwd_kernel, dim3(rg_blocks(height, width)), dim3(RG_NT), 0, sc_s(stream), A, M, mask_channels,
                       height, width, mode, n_total, grad_value, grad_acc);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
