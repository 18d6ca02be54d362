// The head of a frame: StreetGaussianModel.parse_camera + the five get_* properties (street_gaussian_model.py:202-407,
// gaussian_model_actor.py:67-76, gaussian_model_sky.py:62-76) in one launch, and its backward in one launch.
//
// A streaming kernel over row ranges of very different length (a 1 M-row background next to tens of 20 k-row actors), so
// it has optim.hip's shape: the frame is cut into chunks of 256 rows that never cross a segment, the segment table travels
// BY VALUE in the kernel arguments with the running chunk count per segment, and a grid of at most 2048 workgroups
// strides over the chunk list.  A workgroup works inside one segment: kind, pose, basis, centre are wave-uniform (scalar
// loads from the kernel arguments).  Per chunk:
//   rows   one row per thread for the small fields (xyz, rotation, scaling, opacity: 44 B in, 44 B out);
//   sh     the chunk's [rows, K, 3] block is ONE contiguous run of the output: it moves element-wise and coalesced, as
//          16-byte vectors on the dense side whenever that side is 16-byte aligned (forward: the sh run; backward: the
//          features_rest gradient run), with one 16-byte load where the four source elements are contiguous in memory
//          (at dword alignment: the other side has a 12-byte gap per row) and dword loads for the vectors that hold a DC
//          coefficient or the end of a row; a run that is not 16-byte aligned (K = 1 at an odd row, say) goes element by
//          element.
// Backward recomputes the forward's intermediates from the raw parameters; the pose gradients are reduced per workgroup
// (wave shuffles, then LDS) and leave with one fp32 atomic add per value and chunk: their sum order is not fixed.
// No workspace, no host-to-device copy, no synchronisation.
#include "sc_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_GRID = 2048;                 // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int ROWS = BLOCK;                    // rows per chunk
constexpr int MAX_SEG = 16;                    // segments per launch: 16 x (136 + 48 + 4) B of kernel arguments in backward
constexpr int64_t MAX_CHUNKS = 0x7fffffff;
constexpr float NORM_EPS = 1e-12f;             // F.normalize's floor

struct Frame {                                 // what every segment of a call shares
    const float* obj_rots;
    const float* obj_trans;
    float flip_q[4];
    int K;
};

struct FwdArgs {
    sc_compose_segment s[MAX_SEG];
    uint32_t chunk_end[MAX_SEG];
    int n;
    Frame f;
    float *means, *quats, *scales, *opacities, *sh;
};

struct BwdArgs {
    sc_compose_segment s[MAX_SEG];
    sc_compose_grads g[MAX_SEG];
    uint32_t chunk_end[MAX_SEG];
    int n;
    Frame f;
    const float *g_means, *g_quats, *g_scales, *g_opacities, *g_sh;      // each nullable: zeros
    float *grad_obj_rots, *grad_obj_trans;                               // each nullable: not reduced
};

struct Quat { float w, x, y, z; };

// Hamilton product, real part first (general_utils.py:245-267)
__device__ __forceinline__ Quat qmul(const Quat a, const Quat b) {
    return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z,
            a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
            a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
// c = a (x) b, g = dL/dc: dL/da and dL/db
__device__ __forceinline__ Quat qmul_grad_a(const Quat g, const Quat b) {
    return {g.w * b.w + g.x * b.x + g.y * b.y + g.z * b.z,
            -g.w * b.x + g.x * b.w - g.y * b.z + g.z * b.y,
            -g.w * b.y + g.x * b.z + g.y * b.w - g.z * b.x,
            -g.w * b.z - g.x * b.y + g.y * b.x + g.z * b.w};
}
__device__ __forceinline__ Quat qmul_grad_b(const Quat g, const Quat a) {
    return {g.w * a.w + g.x * a.x + g.y * a.y + g.z * a.z,
            -g.w * a.x + g.x * a.w + g.y * a.z - g.z * a.y,
            -g.w * a.y - g.x * a.z + g.y * a.w + g.z * a.x,
            -g.w * a.z + g.x * a.y - g.y * a.x + g.z * a.w};
}
// F.normalize: q / max(|q|, 1e-12); returns the denominator
__device__ __forceinline__ float qnormalize(Quat& q) {
    const float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    const float d = n > NORM_EPS ? n : NORM_EPS;
    q.w /= d; q.x /= d; q.y /= d; q.z /= d;
    return d;
}
// its VJP: u the normalised value, d the denominator, n >= eps <=> d == n (clamp_min passes at equality)
__device__ __forceinline__ Quat qnormalize_grad(const Quat g, const Quat u, const float d, const bool floored) {
    if (floored) return {g.w / d, g.x / d, g.y / d, g.z / d};
    const float dot = g.w * u.w + g.x * u.x + g.y * u.y + g.z * u.z;
    return {(g.w - u.w * dot) / d, (g.x - u.x * dot) / d, (g.y - u.y * dot) / d, (g.z - u.z * dot) / d};
}
__device__ __forceinline__ bool qfloored(const float* r) {
    return !(sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]) >= NORM_EPS);
}

// general_utils.quaternion_to_matrix (general_utils.py:125-146): s = 2 / |q|^2, q not normalised first
__device__ __forceinline__ void qmatrix(const Quat q, float R[9]) {
    const float r = q.w, i = q.x, j = q.y, k = q.z;
    const float s = 2.0f / (r * r + i * i + j * j + k * k);
    R[0] = 1.0f - s * (j * j + k * k); R[1] = s * (i * j - k * r);        R[2] = s * (i * k + j * r);
    R[3] = s * (i * j + k * r);        R[4] = 1.0f - s * (i * i + k * k); R[5] = s * (j * k - i * r);
    R[6] = s * (i * k - j * r);        R[7] = s * (j * k + i * r);        R[8] = 1.0f - s * (i * i + j * j);
}
// R = I + s M(q): G = dL/dR -> dL/dq
__device__ __forceinline__ Quat qmatrix_grad(const Quat q, const float G[9]) {
    const float r = q.w, i = q.x, j = q.y, k = q.z;
    const float s = 2.0f / (r * r + i * i + j * j + k * k);
    const float gs = -G[0] * (j * j + k * k) + G[1] * (i * j - k * r) + G[2] * (i * k + j * r)
                     + G[3] * (i * j + k * r) - G[4] * (i * i + k * k) + G[5] * (j * k - i * r)
                     + G[6] * (i * k - j * r) + G[7] * (j * k + i * r) - G[8] * (i * i + j * j);
    const float t = -s * s * gs;                                       // ds/dq = -s^2 q
    Quat o;
    o.w = s * (-k * G[1] + j * G[2] + k * G[3] - i * G[5] - j * G[6] + i * G[7]) + t * r;
    o.x = s * (j * G[1] + k * G[2] + j * G[3] - 2.0f * i * G[4] - r * G[5] + k * G[6] + r * G[7] - 2.0f * i * G[8]) + t * i;
    o.y = s * (-2.0f * j * G[0] + i * G[1] + r * G[2] + i * G[3] + k * G[5] - r * G[6] + k * G[7] - 2.0f * j * G[8]) + t * j;
    o.z = s * (-2.0f * k * G[0] - r * G[1] + i * G[2] + r * G[3] - 2.0f * k * G[4] + j * G[5] + i * G[6] + j * G[7]) + t * k;
    return o;
}

// 16 bytes from an address that is only 4-byte aligned: one global_load_dwordx4 (gfx950 global memory takes a multi-dword
// access at dword alignment); the 16-byte STORES of this file go to 16-byte aligned addresses only
struct __attribute__((packed, aligned(4))) Float4u { float x, y, z, w; };
__device__ __forceinline__ float4 load4(const float* __restrict__ p) {
    const Float4u v = *reinterpret_cast<const Float4u*>(p);
    return make_float4(v.x, v.y, v.z, v.w);
}

// The vector form of the sh move: dst[v] (16-byte aligned) = four consecutive elements of a mapping with period `period`
// elements per row.  fast(row, col) is the source address when the four are contiguous in memory (else nullptr),
// slow(row, col) one element.  Four vectors per thread are loaded before the first is stored, so that a wave has 4 KB in
// flight, not 1; a lane without a contiguous source loads from `safe` (16 readable bytes, or nullptr: no load) and
// replaces the value, so the loads are not under divergent control.  (row, col) advance by 4 * BLOCK elements per vector:
// no division in the loop.
template <typename Fast, typename Slow>
__device__ __forceinline__ void move_vectors(float* __restrict__ dst, const int nvec, const int tid, const int period,
                                             const float* __restrict__ safe, Fast fast, Slow slow) {
    constexpr int U = 4;
    const int step_row = (4 * BLOCK) / period, step_col = (4 * BLOCK) - step_row * period;
    int row = (tid << 2) / period, col = (tid << 2) - row * period;
    for (int v0 = tid; v0 < nvec; v0 += U * BLOCK) {
        float4 o[U];
        int rr[U], cc[U];
        bool contiguous[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            rr[u] = row; cc[u] = col;
            const float* p = v0 + u * BLOCK < nvec ? fast(row, col) : nullptr;
            contiguous[u] = p != nullptr;
            if (p == nullptr) p = safe;
            o[u] = p != nullptr ? load4(p) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            row += step_row; col += step_col;
            if (col >= period) { col -= period; ++row; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int v = v0 + u * BLOCK;
            if (v >= nvec) break;
            if (!contiguous[u]) {                                       // a DC coefficient, or the end of a row, in it
                float e[4];
                int r = rr[u], c = cc[u];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    e[k] = slow(r, c);
                    if (++c == period) { c = 0; ++r; }
                }
                o[u] = make_float4(e[0], e[1], e[2], e[3]);
            }
            reinterpret_cast<float4*>(dst)[v] = o[u];
        }
    }
}

__device__ __forceinline__ float sigmoidf(const float x) { return 1.0f / (1.0f + expf(-x)); }

// DC coefficient c of a segment row: the IDFT sum of an actor (gaussian_model_actor.py:73), a copy otherwise
__device__ __forceinline__ float dc_value(const sc_compose_segment& s, const float* __restrict__ dc_row, const int c) {
    if (s.kind != SC_COMPOSE_ACTOR || s.fourier_dim == 1) return dc_row[c];
    float acc = s.basis[0] * dc_row[c];
    for (int f = 1; f < s.fourier_dim; ++f) acc += s.basis[f] * dc_row[3 * f + c];
    return acc;
}

__global__ void __launch_bounds__(BLOCK) compose_fwd_kernel(const FwdArgs a) {
    const uint32_t total = a.chunk_end[a.n - 1];
    const int tid = (int)threadIdx.x;
    const int K = a.f.K, W = 3 * K;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int e = sc_find_entry(a.chunk_end, a.n, c);
        const sc_compose_segment& s = a.s[e];
        const uint32_t first = e ? a.chunk_end[e - 1] : 0u;
        const int64_t r0 = (int64_t)(c - first) * ROWS;                 // first row of the chunk, in the segment
        const int64_t left = (s.end - s.start) - r0;
        const int nrows = left < ROWS ? (int)left : ROWS;               // 1..ROWS
        const int64_t row0 = s.start + r0;                              // ... in the frame
        // ---- the small fields: a row per thread ----
        if (tid < nrows) {
            const int64_t r = r0 + tid, i = row0 + tid;
            const float* x = s.xyz + 3 * r;
            const float* sc = s.scaling + 3 * r;
            const float* rt = s.rotation + 4 * r;
            float m0 = x[0], m1 = x[1], m2 = x[2];
            Quat q = {rt[0], rt[1], rt[2], rt[3]};
            qnormalize(q);
            float s0 = expf(sc[0]), s1 = expf(sc[1]), s2 = expf(sc[2]);
            if (s.kind == SC_COMPOSE_ACTOR) {
                if (s.flip != nullptr && s.flip[r]) {
                    m1 = -m1;
                    q = qmul({a.f.flip_q[0], a.f.flip_q[1], a.f.flip_q[2], a.f.flip_q[3]}, q);
                }
                const float* pr = a.f.obj_rots + 4 * (int64_t)s.pose_row;
                const float* pt = a.f.obj_trans + 3 * (int64_t)s.pose_row;
                const Quat p = {pr[0], pr[1], pr[2], pr[3]};
                float R[9];
                qmatrix(p, R);
                const float y0 = R[0] * m0 + R[1] * m1 + R[2] * m2 + pt[0];
                const float y1 = R[3] * m0 + R[4] * m1 + R[5] * m2 + pt[1];
                const float y2 = R[6] * m0 + R[7] * m1 + R[8] * m2 + pt[2];
                m0 = y0; m1 = y1; m2 = y2;
                q = qmul(p, q);
                qnormalize(q);
            } else if (s.kind == SC_COMPOSE_SKY) {
                const float rad = s.radius;
                s0 = s0 < rad ? s0 : (s0 != s0 ? s0 : rad);             // torch.clamp(max=): NaN propagates
                s1 = s1 < rad ? s1 : (s1 != s1 ? s1 : rad);
                s2 = s2 < rad ? s2 : (s2 != s2 ? s2 : rad);
                const float d0 = m0 - s.centre[0], d1 = m1 - s.centre[1], d2 = m2 - s.centre[2];
                const float ratio = sqrtf(d0 * d0 + d1 * d1 + d2 * d2) / (2.0f * rad);
                if (ratio < 1.0f) {
                    m0 = s.centre[0] + d0 / ratio;
                    m1 = s.centre[1] + d1 / ratio;
                    m2 = s.centre[2] + d2 / ratio;
                }
            }
            float* om = a.means + 3 * i;
            om[0] = m0; om[1] = m1; om[2] = m2;
            float* oq = a.quats + 4 * i;
            oq[0] = q.w; oq[1] = q.x; oq[2] = q.y; oq[3] = q.z;
            float* os = a.scales + 3 * i;
            os[0] = s0; os[1] = s1; os[2] = s2;
            a.opacities[i] = sigmoidf(s.opacity[r]);
        }
        // ---- sh: the chunk's run of nrows * W floats ----
        float* __restrict__ dst = a.sh + row0 * W;
        const float* __restrict__ rest = K > 1 ? s.features_rest + r0 * (W - 3) : nullptr;
        const float* __restrict__ dc = s.features_dc + r0 * 3 * s.fourier_dim;
        const int dcw = 3 * s.fourier_dim;
        const int n = nrows * W;
        auto at = [&](const int row, const int col) -> float {
            return col < 3 ? dc_value(s, dc + row * dcw, col) : rest[row * (W - 3) + col - 3];
        };
        auto elem = [&](const int j) -> float { return at(j / W, j % W); };
        if ((((uintptr_t)dst) & 15u) != 0) {
            for (int j = tid; j < n; j += BLOCK) dst[j] = elem(j);
            continue;
        }
        const int nvec = n >> 2;
        move_vectors(dst, nvec, tid, W, (K > 1 && nrows * (W - 3) >= 4) ? rest : nullptr,
                     [&](const int row, const int col) -> const float* {     // four elements of one features_rest row
                         return (col >= 3 && col + 3 < W) ? rest + row * (W - 3) + col - 3 : nullptr;
                     }, at);
        const int j = (nvec << 2) + tid;                                // the ragged tail: at most 3 elements
        if (j < n) dst[j] = elem(j);
    }
}

// sum over the workgroup; the result is valid in thread 0.  red: BLOCK / 64 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = sc_wave_sum(v);
    __syncthreads();
    if (sc_lane() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
    if (threadIdx.x == 0)
        for (int w = 0; w < BLOCK / SC_WAVE; ++w) t += red[w];
    return t;
}

__global__ void __launch_bounds__(BLOCK) compose_bwd_kernel(const BwdArgs a) {
    __shared__ float red[BLOCK / SC_WAVE];
    const uint32_t total = a.chunk_end[a.n - 1];
    const int tid = (int)threadIdx.x;
    const int K = a.f.K, W = 3 * K;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int e = sc_find_entry(a.chunk_end, a.n, c);
        const sc_compose_segment& s = a.s[e];
        const sc_compose_grads& g = a.g[e];
        const uint32_t first = e ? a.chunk_end[e - 1] : 0u;
        const int64_t r0 = (int64_t)(c - first) * ROWS;
        const int64_t left = (s.end - s.start) - r0;
        const int nrows = left < ROWS ? (int)left : ROWS;
        const int64_t row0 = s.start + r0;
        const bool actor = s.kind == SC_COMPOSE_ACTOR;
        Quat gp = {0.0f, 0.0f, 0.0f, 0.0f};                             // this row's share of the pose gradients
        float gt0 = 0.0f, gt1 = 0.0f, gt2 = 0.0f;
        if (tid < nrows) {
            const int64_t r = r0 + tid, i = row0 + tid;
            const float* x = s.xyz + 3 * r;
            const float* sc = s.scaling + 3 * r;
            const float* rt = s.rotation + 4 * r;
            float gm0 = 0.0f, gm1 = 0.0f, gm2 = 0.0f;
            if (a.g_means) { gm0 = a.g_means[3 * i]; gm1 = a.g_means[3 * i + 1]; gm2 = a.g_means[3 * i + 2]; }
            Quat gq = {0.0f, 0.0f, 0.0f, 0.0f};
            if (a.g_quats) gq = {a.g_quats[4 * i], a.g_quats[4 * i + 1], a.g_quats[4 * i + 2], a.g_quats[4 * i + 3]};
            float gs0 = 0.0f, gs1 = 0.0f, gs2 = 0.0f;
            if (a.g_scales) { gs0 = a.g_scales[3 * i]; gs1 = a.g_scales[3 * i + 1]; gs2 = a.g_scales[3 * i + 2]; }
            const float go = a.g_opacities ? a.g_opacities[i] : 0.0f;
            // scales, opacities
            const float e0 = expf(sc[0]), e1 = expf(sc[1]), e2 = expf(sc[2]);
            if (s.kind == SC_COMPOSE_SKY) {                             // torch.clamp(max=): passes iff exp <= radius
                const float rad = s.radius;
                if (!(e0 <= rad)) gs0 = 0.0f;
                if (!(e1 <= rad)) gs1 = 0.0f;
                if (!(e2 <= rad)) gs2 = 0.0f;
            }
            float* os = g.scaling + 3 * r;
            os[0] = gs0 * e0; os[1] = gs1 * e1; os[2] = gs2 * e2;
            const float sg = sigmoidf(s.opacity[r]);
            g.opacity[r] = go * (sg * (1.0f - sg));
            // means, quats
            Quat qn = {rt[0], rt[1], rt[2], rt[3]};
            const bool fl_n = qfloored(rt);
            const float dn = qnormalize(qn);
            float gx0 = gm0, gx1 = gm1, gx2 = gm2;
            Quat gqn = gq;                                              // dL/d normalize(rotation)
            if (actor) {
                const bool flip = s.flip != nullptr && s.flip[r];
                const Quat fq = {a.f.flip_q[0], a.f.flip_q[1], a.f.flip_q[2], a.f.flip_q[3]};
                const float x0 = x[0], x1 = flip ? -x[1] : x[1], x2 = x[2];
                const Quat ql = flip ? qmul(fq, qn) : qn;
                const float* pr = a.f.obj_rots + 4 * (int64_t)s.pose_row;
                const Quat p = {pr[0], pr[1], pr[2], pr[3]};
                float R[9];
                qmatrix(p, R);
                gx0 = R[0] * gm0 + R[3] * gm1 + R[6] * gm2;             // R^T g
                gx1 = R[1] * gm0 + R[4] * gm1 + R[7] * gm2;
                gx2 = R[2] * gm0 + R[5] * gm1 + R[8] * gm2;
                if (flip) gx1 = -gx1;
                Quat w = qmul(p, ql);
                const float wraw[4] = {w.w, w.x, w.y, w.z};
                const bool fl_w = qfloored(wraw);
                const float dw = qnormalize(w);
                const Quat gw = qnormalize_grad(gq, w, dw, fl_w);
                const Quat gql = qmul_grad_b(gw, p);
                gqn = flip ? qmul_grad_b(gql, fq) : gql;
                if (a.grad_obj_rots) {
                    const float G[9] = {gm0 * x0, gm0 * x1, gm0 * x2, gm1 * x0, gm1 * x1, gm1 * x2,
                                        gm2 * x0, gm2 * x1, gm2 * x2};
                    const Quat g1 = qmatrix_grad(p, G), g2 = qmul_grad_a(gw, ql);
                    gp = {g1.w + g2.w, g1.x + g2.x, g1.y + g2.y, g1.z + g2.z};
                }
                gt0 = gm0; gt1 = gm1; gt2 = gm2;
            } else if (s.kind == SC_COMPOSE_SKY) {
                const float rad = s.radius;
                const float d0 = x[0] - s.centre[0], d1 = x[1] - s.centre[1], d2 = x[2] - s.centre[2];
                const float dist = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
                const float ratio = dist / (2.0f * rad);
                if (ratio < 1.0f) {                                     // m = centre + d / ratio
                    const float u0 = d0 / dist, u1 = d1 / dist, u2 = d2 / dist;
                    const float dot = gm0 * u0 + gm1 * u1 + gm2 * u2;
                    gx0 = (gm0 - u0 * dot) / ratio;
                    gx1 = (gm1 - u1 * dot) / ratio;
                    gx2 = (gm2 - u2 * dot) / ratio;
                }
            }
            float* ox = g.xyz + 3 * r;
            ox[0] = gx0; ox[1] = gx1; ox[2] = gx2;
            const Quat gr = qnormalize_grad(gqn, qn, dn, fl_n);
            float* orot = g.rotation + 4 * r;
            orot[0] = gr.w; orot[1] = gr.x; orot[2] = gr.y; orot[3] = gr.z;
            // features_dc [n,F,3]
            const int Fd = s.fourier_dim;
            float* odc = g.features_dc + 3 * Fd * r;
            float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
            if (a.g_sh) { h0 = a.g_sh[i * W]; h1 = a.g_sh[i * W + 1]; h2 = a.g_sh[i * W + 2]; }
            if (actor && Fd > 1) {
                for (int f = 0; f < Fd; ++f) {
                    odc[3 * f] = s.basis[f] * h0; odc[3 * f + 1] = s.basis[f] * h1; odc[3 * f + 2] = s.basis[f] * h2;
                }
            } else {
                odc[0] = h0; odc[1] = h1; odc[2] = h2;
                for (int f = 3; f < 3 * Fd; ++f) odc[f] = 0.0f;
            }
        }
        // ---- pose gradients: reduced over the chunk, one atomic add per value ----
        if (actor && (a.grad_obj_rots || a.grad_obj_trans)) {
            if (a.grad_obj_rots) {
                float* o = a.grad_obj_rots + 4 * (int64_t)s.pose_row;
                const float t0 = block_sum(gp.w, red), t1 = block_sum(gp.x, red);
                const float t2 = block_sum(gp.y, red), t3 = block_sum(gp.z, red);
                if (tid == 0) { atomicAdd(o, t0); atomicAdd(o + 1, t1); atomicAdd(o + 2, t2); atomicAdd(o + 3, t3); }
            }
            if (a.grad_obj_trans) {
                float* o = a.grad_obj_trans + 3 * (int64_t)s.pose_row;
                const float t0 = block_sum(gt0, red), t1 = block_sum(gt1, red), t2 = block_sum(gt2, red);
                if (tid == 0) { atomicAdd(o, t0); atomicAdd(o + 1, t1); atomicAdd(o + 2, t2); }
            }
        }
        // ---- features_rest: the chunk's run of nrows * (W - 3) floats ----
        if (K == 1) continue;
        const int D = W - 3;
        float* __restrict__ dst = g.features_rest + r0 * D;
        const int n = nrows * D;
        const float* __restrict__ src = a.g_sh ? a.g_sh + row0 * W : nullptr;
        if (src == nullptr) {
            for (int j = tid; j < n; j += BLOCK) dst[j] = 0.0f;
            continue;
        }
        auto elem = [&](const int j) -> float {
            const int row = j / D;
            return src[j + 3 * (row + 1)];                              // row * W + (j - row * D) + 3
        };
        // (a chunk starts 256 rows into its tensor, so this is a gradient tensor that itself is not 16-byte aligned: never
        //  one of compose.py's fresh allocations, but the C ABI takes any fp32 pointer; tests/test_compose_gpu.py runs it)
        if ((((uintptr_t)dst) & 15u) != 0) {
            for (int j = tid; j < n; j += BLOCK) dst[j] = elem(j);
            continue;
        }
        const int nvec = n >> 2;
        move_vectors(dst, nvec, tid, D, src,
                     [&](const int row, const int col) -> const float* {     // four elements of one sh row
                         return col + 3 < D ? src + row * W + col + 3 : nullptr;
                     }, [&](const int row, const int col) -> float { return src[row * W + col + 3]; });
        const int j = (nvec << 2) + tid;
        if (j < n) dst[j] = elem(j);
    }
}

template <typename Args, typename Kernel>
int launch(const Args& a, Kernel kernel, hipStream_t stream) {
    const uint32_t total = a.chunk_end[a.n - 1];
    if (total == 0) return SC_OK;
    const unsigned grid = total < (uint32_t)MAX_GRID ? total : (uint32_t)MAX_GRID;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, stream, a);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

Frame frame_of(int K, const float* obj_rots, const float* obj_trans, const float* flip_q_host) {
    Frame f;
    f.obj_rots = obj_rots; f.obj_trans = obj_trans; f.K = K;
    for (int i = 0; i < 4; ++i) f.flip_q[i] = flip_q_host ? flip_q_host[i] : 0.0f;
    return f;
}

// cuts the (validated) table into launches of at most MAX_SEG non-empty segments
template <typename Args, typename Kernel, typename Fill>
int run(Args& a, Kernel kernel, const sc_compose_segment* seg, int n_segments, Fill fill, hipStream_t stream) {
    a.n = 0;
    int64_t chunks = 0;
    for (int i = 0; i < n_segments; ++i) {
        const int64_t c = (seg[i].end - seg[i].start + ROWS - 1) / ROWS;
        if (c == 0) continue;
        if (a.n == MAX_SEG || chunks + c > MAX_CHUNKS) {
            const int rc = launch(a, kernel, stream);
            if (rc) return rc;
            a.n = 0; chunks = 0;
        }
        chunks += c;
        a.s[a.n] = seg[i];
        fill(a, a.n, i);
        a.chunk_end[a.n] = (uint32_t)chunks;
        ++a.n;
    }
    return a.n ? launch(a, kernel, stream) : SC_OK;
}

}  // namespace

extern "C" int sc_compose_max_segments(void) { return MAX_SEG; }

// (arguments validated by capi.hip)
int sc_compose_fwd_run(const sc_compose_segment* segments_host, int n_segments, int K, const float* obj_rots,
                       const float* obj_trans, const float* flip_q_host, float* means, float* quats, float* scales,
                       float* opacities, float* sh, sc_stream_t stream) {
    FwdArgs a;
    a.f = frame_of(K, obj_rots, obj_trans, flip_q_host);
    a.means = means; a.quats = quats; a.scales = scales; a.opacities = opacities; a.sh = sh;
    return run(a, compose_fwd_kernel, segments_host, n_segments, [](FwdArgs&, int, int) {}, sc_s(stream));
}

int sc_compose_bwd_run(const sc_compose_segment* segments_host, const sc_compose_grads* grads_host, int n_segments, int K,
                       const float* obj_rots, const float* obj_trans, int A, const float* flip_q_host,
                       const float* g_means, const float* g_quats, const float* g_scales, const float* g_opacities,
                       const float* g_sh, float* grad_obj_rots, float* grad_obj_trans, sc_stream_t stream) {
    if (grad_obj_rots && A > 0) SC_HIP(hipMemsetAsync(grad_obj_rots, 0, sizeof(float) * 4 * (size_t)A, sc_s(stream)));
    if (grad_obj_trans && A > 0) SC_HIP(hipMemsetAsync(grad_obj_trans, 0, sizeof(float) * 3 * (size_t)A, sc_s(stream)));
    BwdArgs a;
    a.f = frame_of(K, obj_rots, obj_trans, flip_q_host);
    a.g_means = g_means; a.g_quats = g_quats; a.g_scales = g_scales; a.g_opacities = g_opacities; a.g_sh = g_sh;
    a.grad_obj_rots = grad_obj_rots; a.grad_obj_trans = grad_obj_trans;
    return run(a, compose_bwd_kernel, segments_host, n_segments,
               [grads_host](BwdArgs& b, int at, int i) { b.g[at] = grads_host[i]; }, sc_s(stream));
}
