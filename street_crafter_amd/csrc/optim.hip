// The tail of the training step (train.py:283-290, 319): multi-tensor Adam and the densification statistics.
//
// Both are elementwise streaming kernels over MANY tensors / row ranges of very different length (one 45 M-element
// f_rest next to tens of 20 k-row actors), so both use the same shape: the work of a call is cut into fixed-size chunks
// (4096 elements / 256 rows), the table of tensors travels BY VALUE in the kernel arguments together with the running
// chunk count per entry, and a grid of at most 2048 workgroups of 256 threads strides over the chunk list; a workgroup
// finds its chunk's entry with a wave-uniform binary search over the kernel arguments (scalar loads).  The grid is
// sized by chunks, never by entries: one large tensor fills the chip, a thousand tiny ones cost one chunk each.
// No workspace, no host-to-device copy, no atomics, no synchronisation.
#include "sc_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_GRID = 2048;                       // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int64_t MAX_CHUNKS = 0x7fffffff;           // per launch (the chunk counts are 32-bit)

// ---- Adam -------------------------------------------------------------------------------------------------------
constexpr int ADAM_MAX = 64;                         // entries per launch: 64 x 48 B + 64 x 4 B of kernel arguments
constexpr int ADAM_VEC_ITERS = 4;                    // 16-byte vectors per thread and chunk
constexpr int ADAM_CHUNK = BLOCK * 4 * ADAM_VEC_ITERS;

struct AdamArgs {
    sc_adam_tensor t[ADAM_MAX];
    uint32_t chunk_end[ADAM_MAX];                    // chunks of entries 0..i (inclusive running count)
    int n;
    float one_minus_beta1, beta2, one_minus_beta2, eps;
};

struct AdamConst { float step_size, bias2_sqrt, omb1, b2, omb2, eps; };

// torch's formula; each line is one or two roundings (the fused multiply-adds are explicit, so the vector and the
// scalar path give the same bits)
__device__ __forceinline__ void adam_one(float& p, const float g, float& m, float& v, const AdamConst& k) {
    m = __fmaf_rn(k.omb1, g - m, m);
    v = __fmaf_rn(k.omb2, g * g, k.b2 * v);
    const float denom = sqrtf(v) / k.bias2_sqrt + k.eps;
    p = __fmaf_rn(-k.step_size, m / denom, p);
}

__device__ __forceinline__ void adam_vec(float4& p, const float4& g, float4& m, float4& v, const AdamConst& k) {
    adam_one(p.x, g.x, m.x, v.x, k);
    adam_one(p.y, g.y, m.y, v.y, k);
    adam_one(p.z, g.z, m.z, v.z, k);
    adam_one(p.w, g.w, m.w, v.w, k);
}

__global__ void __launch_bounds__(BLOCK) adam_kernel(const AdamArgs a) {
    const uint32_t total = a.chunk_end[a.n - 1];
    const int tid = (int)threadIdx.x;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int e = sc_find_entry(a.chunk_end, a.n, c);
        const uint32_t first = e ? a.chunk_end[e - 1] : 0u;
        const int64_t base = (int64_t)(c - first) * ADAM_CHUNK;
        const int64_t left = a.t[e].numel - base;
        const int n = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;          // 1..ADAM_CHUNK elements of this chunk
        float* __restrict__ p = a.t[e].param + base;
        const float* __restrict__ g = a.t[e].grad + base;
        float* __restrict__ m = a.t[e].exp_avg + base;
        float* __restrict__ v = a.t[e].exp_avg_sq + base;
        const AdamConst k = {a.t[e].step_size, a.t[e].bias2_sqrt, a.one_minus_beta1, a.beta2, a.one_minus_beta2, a.eps};
        // (base is a multiple of 4096 elements: the chunk is as aligned as the tensor)
        const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15u) == 0;
        if (!aligned) {
            for (int i = tid; i < n; i += BLOCK) {
                float pi = p[i], mi = m[i], vi = v[i];
                adam_one(pi, g[i], mi, vi, k);
                p[i] = pi; m[i] = mi; v[i] = vi;
            }
            continue;
        }
        float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
        float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
        if (n == ADAM_CHUNK) {
            // a full chunk: all sixteen 16-byte loads of a thread are issued before the first is used
            float4 P[ADAM_VEC_ITERS], G[ADAM_VEC_ITERS], M[ADAM_VEC_ITERS], V[ADAM_VEC_ITERS];
#pragma unroll
            for (int j = 0; j < ADAM_VEC_ITERS; ++j) {
                const int i = tid + j * BLOCK;
                P[j] = p4[i]; G[j] = g4[i]; M[j] = m4[i]; V[j] = v4[i];
            }
#pragma unroll
            for (int j = 0; j < ADAM_VEC_ITERS; ++j) {
                const int i = tid + j * BLOCK;
                adam_vec(P[j], G[j], M[j], V[j], k);
                p4[i] = P[j]; m4[i] = M[j]; v4[i] = V[j];
            }
            continue;
        }
        const int nvec = n >> 2;
        for (int i = tid; i < nvec; i += BLOCK) {
            float4 P = p4[i], M = m4[i], V = v4[i];
            adam_vec(P, g4[i], M, V, k);
            p4[i] = P; m4[i] = M; v4[i] = V;
        }
        const int i = (nvec << 2) + tid;                                    // the ragged tail: at most 3 elements
        if (i < n) {
            float pi = p[i], mi = m[i], vi = v[i];
            adam_one(pi, g[i], mi, vi, k);
            p[i] = pi; m[i] = mi; v[i] = vi;
        }
    }
}

int adam_launch(const AdamArgs& a, hipStream_t stream) {
    const uint32_t total = a.chunk_end[a.n - 1];
    if (total == 0) return SC_OK;
    const unsigned grid = total < (uint32_t)MAX_GRID ? total : (uint32_t)MAX_GRID;
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(BLOCK), 0, stream, a);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

// ---- densification statistics ---------------------------------------------------------------------------------------
constexpr int STATS_MAX = 64;                        // segments per launch: 64 x 40 B + 64 x 4 B of kernel arguments
constexpr int STATS_CHUNK = BLOCK;                   // rows per chunk: one per thread

struct StatsArgs {
    sc_stats_segment s[STATS_MAX];
    uint32_t chunk_end[STATS_MAX];
    int n;
};

template <bool RADII_FLOAT>
__global__ void __launch_bounds__(BLOCK) densify_stats_kernel(const StatsArgs a, const float* __restrict__ grad,
                                                              const float* __restrict__ absgrad,
                                                              const void* __restrict__ radii,
                                                              const uint8_t* __restrict__ visible, const float half_w,
                                                              const float half_h) {
    const uint32_t total = a.chunk_end[a.n - 1];
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int e = sc_find_entry(a.chunk_end, a.n, c);
        const uint32_t first = e ? a.chunk_end[e - 1] : 0u;
        const int64_t start = a.s[e].start;
        const int64_t r = (int64_t)(c - first) * STATS_CHUNK + threadIdx.x;      // row of the segment
        const int64_t i = start + r;                                              // row of the render
        if (i >= a.s[e].end || !visible[i]) continue;
        const float rad = RADII_FLOAT ? static_cast<const float*>(radii)[i]
                                      : (float)static_cast<const int32_t*>(radii)[i];
        float* const mr = a.s[e].max_radii + r;
        const float m0 = *mr;
        *mr = (m0 != m0) ? m0 : ((rad > m0 || rad != rad) ? rad : m0);            // torch.max: NaN propagates
        a.s[e].denom[r] += 1.0f;
        float* const acc = a.s[e].grad_accum + 2 * r;
        const float gx = grad[2 * i], gy = grad[2 * i + 1];
        if (absgrad != nullptr) {
            // (g * 0.5) * W: the halving is exact, so one rounding per product, as the torch expression
            const float ax = absgrad[2 * i] * half_w, ay = absgrad[2 * i + 1] * half_h;
            const float sx = gx * half_w, sy = gy * half_h;
            acc[0] += sqrtf(__fmaf_rn(ax, ax, ay * ay));
            acc[1] += sqrtf(__fmaf_rn(sx, sx, sy * sy));
        } else {
            acc[0] += sqrtf(__fmaf_rn(gx, gx, gy * gy));
            acc[1] += 0.0f;
        }
    }
}

int stats_launch(const StatsArgs& a, const float* grad, const float* absgrad, const void* radii, int radii_is_float,
                 const uint8_t* visible, float half_w, float half_h, hipStream_t stream) {
    const uint32_t total = a.chunk_end[a.n - 1];
    if (total == 0) return SC_OK;
    const unsigned grid = total < (uint32_t)MAX_GRID ? total : (uint32_t)MAX_GRID;
    if (radii_is_float)
        hipLaunchKernelGGL(densify_stats_kernel<true>, dim3(grid), dim3(BLOCK), 0, stream, a, grad, absgrad, radii,
                           visible, half_w, half_h);
    else
        hipLaunchKernelGGL(densify_stats_kernel<false>, dim3(grid), dim3(BLOCK), 0, stream, a, grad, absgrad, radii,
                           visible, half_w, half_h);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

}  // namespace

extern "C" int sc_adam_max_tensors(void) { return ADAM_MAX; }

extern "C" int sc_adam_step(const sc_adam_tensor* table_host, int n_tensors, float one_minus_beta1, float beta2,
                            float one_minus_beta2, float eps, sc_stream_t stream) {
    if (n_tensors == 0) return SC_OK;
    if (n_tensors < 0 || table_host == nullptr) return SC_EINVAL;
    for (int i = 0; i < n_tensors; ++i) {
        const sc_adam_tensor& t = table_host[i];
        if (t.numel < 0 || (t.numel + ADAM_CHUNK - 1) / ADAM_CHUNK > MAX_CHUNKS) return SC_EINVAL;
        if (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return SC_EINVAL;
    }
    AdamArgs a;
    a.n = 0;
    a.one_minus_beta1 = one_minus_beta1; a.beta2 = beta2; a.one_minus_beta2 = one_minus_beta2; a.eps = eps;
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const int64_t c = (table_host[i].numel + ADAM_CHUNK - 1) / ADAM_CHUNK;
        if (c == 0) continue;
        if (a.n == ADAM_MAX || chunks + c > MAX_CHUNKS) {             // the piece is full: launch it, start the next
            const int rc = adam_launch(a, sc_s(stream));
            if (rc) return rc;
            a.n = 0; chunks = 0;
        }
        chunks += c;
        a.t[a.n] = table_host[i];
        a.chunk_end[a.n] = (uint32_t)chunks;
        ++a.n;
    }
    return a.n ? adam_launch(a, sc_s(stream)) : SC_OK;
}

extern "C" int sc_densify_stats(const float* grad, const float* absgrad, const void* radii, int radii_is_float,
                                const uint8_t* visible, int64_t N, float half_width, float half_height,
                                const sc_stats_segment* segments_host, int n_segments, sc_stream_t stream) {
    if (n_segments == 0) return SC_OK;
    if (n_segments < 0 || N < 0 || segments_host == nullptr) return SC_EINVAL;
    bool any = false;
    for (int i = 0; i < n_segments; ++i) {
        const sc_stats_segment& s = segments_host[i];
        if (s.start < 0 || s.start > s.end || s.end > N) return SC_EINVAL;
        if (!s.grad_accum || !s.denom || !s.max_radii) return SC_EINVAL;
        if ((s.end - s.start + STATS_CHUNK - 1) / STATS_CHUNK > MAX_CHUNKS) return SC_EINVAL;
        any = any || s.end > s.start;
    }
    if (!any) return SC_OK;
    if (!grad || !radii || !visible) return SC_EINVAL;
    StatsArgs a;
    a.n = 0;
    int64_t chunks = 0;
    for (int i = 0; i < n_segments; ++i) {
        const int64_t c = (segments_host[i].end - segments_host[i].start + STATS_CHUNK - 1) / STATS_CHUNK;
        if (c == 0) continue;
        if (a.n == STATS_MAX || chunks + c > MAX_CHUNKS) {
            const int rc = stats_launch(a, grad, absgrad, radii, radii_is_float, visible, half_width, half_height,
                                        sc_s(stream));
            if (rc) return rc;
            a.n = 0; chunks = 0;
        }
        chunks += c;
        a.s[a.n] = segments_host[i];
        a.chunk_end[a.n] = (uint32_t)chunks;
        ++a.n;
    }
    return a.n ? stats_launch(a, grad, absgrad, radii, radii_is_float, visible, half_width, half_height, sc_s(stream))
               : SC_OK;
}
