// Densify and prune of any number of sub-models (train.py:292-299, street_gaussian_model.py:535-549; per sub-model
// gaussian_model.py:363-547): the reference's clone (cat), split (cat + mask) and prune (mask) as ONE selection and ONE
// gather of every parameter and Adam moment.
//
// Plan.  Every original row has four candidate output rows (slot 0 the original, 1 its clone, 2 / 3 its split children);
// whether a candidate exists and survives the prune tests depends on that row's data alone, so the reference's output
// order -- originals, clones, children 0, children 1, each in row order -- is an exclusive scan of the keep flags laid
// out [slot][row].  Three launches over the same chunk table as optim.hip (jobs by value in the kernel arguments, one
// chunk = one scan block of 256 rows, grid sized by chunks):
//   flags  one thread per row: the decisions, the children's xyz' / scaling', a 4-bit keep mask per row, the keep count
//          of each slot per block, the job's counters (integer atomics, one per block and counter)
//   scan   one workgroup per job: exclusive scan in place over the block counts [slot][block], n'
//   emit   one thread per row: rank inside the block by ballot, src_row / slot at block offset + rank
// No workgroup waits for another (no look-back, no flag): the passes are separate launches.  Integer sums only, so
// every output is the same from run to run.
// Apply.  A table of groups (parameter + both moments) with the same chunking by output elements: dst[r] =
// src[src_row[r]], coalesced on the destination; a source row is contiguous, so the lanes of one row read one segment.
#include "sc_common.h"

namespace {

constexpr int BLOCK = 256;                           // threads per workgroup = rows per scan block
constexpr int MAX_GRID = 2048;                       // 256 CUs x 8 workgroups, grid-stride beyond
constexpr int64_t MAX_CHUNKS = 0x7fffffff;
constexpr int64_t MAX_ROWS = (int64_t)1 << 29;       // 2 n output rows and 4 x blocks counts stay 32-bit

// ---- plan ---------------------------------------------------------------------------------------------------------------
constexpr int PLAN_MAX = 16;                         // jobs per launch: 16 x (176 + 20) B of kernel arguments
constexpr int SCAN_ITEMS = 8;                        // counts per thread and round of the scan kernel
constexpr float SPLIT_DIV = (float)(0.8 * 2);        // gaussian_model.py:473 with N = 2: the fp32 value torch divides by

struct PlanArgs {
    sc_densify_job j[PLAN_MAX];
    uint8_t* flags[PLAN_MAX];                        // [n] keep mask per row (bit = slot)
    int32_t* totals[PLAN_MAX];                       // [4][blocks]: keep counts, after the scan their exclusive offsets
    uint32_t chunk_end[PLAN_MAX];
    int n;
};

__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }   // torch.max
__device__ __forceinline__ float max3(const float* s) { return nan_max(nan_max(s[0], s[1]), s[2]); }

// general_utils.py:125-146 on the normalised quaternion
__device__ __forceinline__ void quat_matrix(const float* q, float* R) {
    const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float r = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
    R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - r * z);        R[2] = 2.0f * (x * z + r * y);
    R[3] = 2.0f * (x * y + r * z);        R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - r * x);
    R[6] = 2.0f * (x * z - r * y);        R[7] = 2.0f * (y * z + r * x);        R[8] = 1.0f - 2.0f * (x * x + y * y);
}

// out = p + R (noise * s)
__device__ __forceinline__ void sample_point(const float* p, const float* R, const float* noise, const float* s,
                                             float* out) {
    const float d0 = noise[0] * s[0], d1 = noise[1] * s[1], d2 = noise[2] * s[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = p[r] + (R[3 * r] * d0 + R[3 * r + 1] * d1 + R[3 * r + 2] * d2);
}

// the prune tests of one existing candidate (position p, activated scale s): bit 0 = pruned, bit 1 = big in world space
__device__ __forceinline__ int prune_bits(const sc_densify_job& J, int64_t i, int slot, const float* p, const float* s,
                                          const float* R, bool below, float max_r) {
    bool pruned = below, big = false;
    if (J.prune_big) {
        big = max3(s) > J.big_size;
        if (J.region == 1) {
            const float dx = p[0] - J.region_a[0], dy = p[1] - J.region_a[1], dz = p[2] - J.region_a[2];
            if (sqrtf(dx * dx + dy * dy + dz * dz) > J.region_b[0]) big = false;
        }
        pruned = pruned || big;
        if (J.region == 2) {
            const float* bn = J.box_noise + (((int64_t)slot * J.n + i) * 2) * 3;
            bool inside = true;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                float v[3];
                sample_point(p, R, bn + 3 * m, s, v);
#pragma unroll
                for (int r = 0; r < 3; ++r) inside = inside && v[r] >= J.region_a[r] && v[r] <= J.region_b[r];
            }
            pruned = pruned || !inside;
        }
    }
    if (slot == 0 && J.max_screen_size > 0.0f && max_r > J.max_screen_size) pruned = true;
    return (pruned ? 1 : 0) | (big ? 2 : 0);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

constexpr int N_SUMS = 9;      // keep counts of the four slots, then clone, split, below min opacity, big, pruned

__global__ void __launch_bounds__(BLOCK) densify_flags_kernel(const PlanArgs a) {
    __shared__ int acc[N_SUMS];
    const uint32_t total = a.chunk_end[a.n - 1];
    const int tid = (int)threadIdx.x;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int e = sc_find_entry(a.chunk_end, a.n, c);
        const uint32_t b = c - (e ? a.chunk_end[e - 1] : 0u);                   // block of the job
        const sc_densify_job& J = a.j[e];
        const int64_t n = J.n;
        const int64_t i = (int64_t)b * BLOCK + tid;
        int sums[N_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (tid < N_SUMS) acc[tid] = 0;
        if (i < n) {
            float p[3], sr[3], s[3], q[4], R[9];
#pragma unroll
            for (int k = 0; k < 3; ++k) { p[k] = J.xyz[3 * i + k]; sr[k] = J.scaling[3 * i + k]; s[k] = expf(sr[k]); }
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = J.rotation[4 * i + k];
            float g = J.grad_accum[2 * i + J.grad_col] / J.denom[i];
            if (g != g) g = 0.0f;
            const bool hot = g >= J.max_grad;
            const bool small = max3(s) <= J.dense_size;
            const bool clone = hot && small, split = hot && !small;
            const bool below = 1.0f / (1.0f + expf(-J.opacity[i])) < J.min_opacity;
            const bool need_R = split || (J.prune_big && J.region == 2);
            if (need_R) quat_matrix(q, R);
            int mask = 0;
            if (!split) {
                // slot 0, and slot 1 where the row is cloned: the clone is the same raw row with max_radii2D 0
                const int t0 = prune_bits(J, i, 0, p, s, R, below, J.max_radii[i]);
                mask |= (t0 & 1) ? 0 : 1;
                sums[6] += below; sums[7] += t0 >> 1; sums[8] += t0 & 1;
                if (clone) {
                    const int t1 = prune_bits(J, i, 1, p, s, R, below, 0.0f);
                    mask |= (t1 & 1) ? 0 : 2;
                    sums[6] += below; sums[7] += t1 >> 1; sums[8] += t1 & 1;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    float pc[3], sc[3], src[3];
                    sample_point(p, R, J.split_noise + ((int64_t)k * n + i) * 3, s, pc);
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        src[d] = logf(s[d] / SPLIT_DIV);
                        sc[d] = expf(src[d]);
                        J.child_xyz[((int64_t)k * n + i) * 3 + d] = pc[d];
                        J.child_scaling[((int64_t)k * n + i) * 3 + d] = src[d];
                    }
                    const int t = prune_bits(J, i, 2 + k, pc, sc, R, below, 0.0f);
                    mask |= (t & 1) ? 0 : (4 << k);
                    sums[6] += below; sums[7] += t >> 1; sums[8] += t & 1;
                }
            }
            a.flags[e][i] = (uint8_t)mask;
#pragma unroll
            for (int k = 0; k < 4; ++k) sums[k] = (mask >> k) & 1;
            sums[4] = clone; sums[5] = split;
        }
        __syncthreads();                                                        // acc is zero
#pragma unroll
        for (int k = 0; k < N_SUMS; ++k) {
            const int v = wave_sum_int(sums[k]);
            if (sc_lane() == 0 && v) atomicAdd(&acc[k], v);
        }
        __syncthreads();
        const int64_t nb = (n + BLOCK - 1) / BLOCK;
        if (tid < 4) a.totals[e][tid * nb + b] = acc[tid];
        else if (tid < N_SUMS && acc[tid]) atomicAdd(&J.counters[tid - 3], acc[tid]);   // counters[1..5]
        __syncthreads();                                                        // before the next chunk zeroes acc
    }
}

__global__ void __launch_bounds__(BLOCK) densify_scan_kernel(const PlanArgs a) {
    __shared__ int wsum[BLOCK / SC_WAVE];
    const int e = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6;
    const int64_t n = a.j[e].n;
    const int64_t m = 4 * ((n + BLOCK - 1) / BLOCK);
    int32_t* const t = a.totals[e];
    int carry = 0;
    for (int64_t base = 0; base < m; base += BLOCK * SCAN_ITEMS) {
        const int64_t i0 = base + (int64_t)tid * SCAN_ITEMS;
        int v[SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) { v[k] = i0 + k < m ? t[i0 + k] : 0; sum += v[k]; }
        const int incl = sc_wave_incl_scan(sum);
        if (sc_lane() == 63) wsum[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / SC_WAVE; ++w) { before += w < wave ? wsum[w] : 0; all += wsum[w]; }
        int excl = carry + before + incl - sum;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            if (i0 + k < m) t[i0 + k] = excl;
            excl += v[k];
        }
        carry += all;
        __syncthreads();                                                        // wsum is rewritten in the next round
    }
    if (tid == 0) { a.j[e].counters[0] = (int32_t)n; a.j[e].counters[6] = carry; }
}

__global__ void __launch_bounds__(BLOCK) densify_emit_kernel(const PlanArgs a) {
    __shared__ int wcnt[4][BLOCK / SC_WAVE];
    const uint32_t total = a.chunk_end[a.n - 1];
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int e = sc_find_entry(a.chunk_end, a.n, c);
        const uint32_t b = c - (e ? a.chunk_end[e - 1] : 0u);
        const int64_t n = a.j[e].n;
        const int64_t nb = (n + BLOCK - 1) / BLOCK;
        const int64_t i = (int64_t)b * BLOCK + tid;
        const int mask = i < n ? a.flags[e][i] : 0;
        int rank[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long votes = __ballot((mask >> k) & 1);
            rank[k] = __popcll(votes & sc_lanemask_lt());
            if (sc_lane() == 0) wcnt[k][wave] = __popcll(votes);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!((mask >> k) & 1)) continue;
            int64_t out = a.totals[e][k * nb + b] + rank[k];
            for (int w = 0; w < wave; ++w) out += wcnt[k][w];
            if (out < 2 * n) {                                                  // (holds by construction)
                a.j[e].src_row[out] = (int32_t)i;
                a.j[e].slot[out] = (uint8_t)k;
            }
        }
        __syncthreads();                                                        // before the next chunk rewrites wcnt
    }
}

int plan_launch(const PlanArgs& a, hipStream_t stream) {
    const uint32_t total = a.chunk_end[a.n - 1];
    const unsigned grid = total < (uint32_t)MAX_GRID ? total : (uint32_t)MAX_GRID;
    hipLaunchKernelGGL(densify_flags_kernel, dim3(grid), dim3(BLOCK), 0, stream, a);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(densify_scan_kernel, dim3((unsigned)a.n), dim3(BLOCK), 0, stream, a);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(densify_emit_kernel, dim3(grid), dim3(BLOCK), 0, stream, a);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

// workspace of one job: the keep masks, then the block counts, each 16-byte aligned
inline size_t job_flags_bytes(int64_t n) { return sc_align_up((size_t)n, 16); }
inline size_t job_totals_bytes(int64_t n) { return sc_align_up((size_t)(4 * ((n + BLOCK - 1) / BLOCK)) * 4, 16); }

bool job_sizes_ok(const sc_densify_job* jobs, int n_jobs) {
    if (n_jobs < 0 || (n_jobs > 0 && jobs == nullptr)) return false;
    for (int i = 0; i < n_jobs; ++i)
        if (jobs[i].n < 0 || jobs[i].n >= MAX_ROWS) return false;
    return true;
}

// ---- apply --------------------------------------------------------------------------------------------------------------
constexpr int APPLY_MAX = 32;                        // groups per launch: 32 x (96 + 4) B of kernel arguments
constexpr int APPLY_ITERS = 4;                       // 16-byte vectors per thread and chunk
constexpr int APPLY_CHUNK = BLOCK * 4 * APPLY_ITERS; // output elements per chunk

struct ApplyArgs {
    sc_densify_group g[APPLY_MAX];
    uint32_t chunk_end[APPLY_MAX];
    int n;
};

template <typename T> __device__ __forceinline__ T zero_of();
template <> __device__ __forceinline__ float zero_of<float>() { return 0.0f; }
template <> __device__ __forceinline__ float4 zero_of<float4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// One chunk of one group in units of T (float or float4): `w` units per row, `count` units in this chunk from `base`.
template <typename T>
__device__ __forceinline__ void apply_chunk(const sc_densify_group& G, const int64_t base, const int count,
                                            const uint32_t w, const int per_thread) {
    const T* __restrict__ sp = reinterpret_cast<const T*>(G.src_param);
    const T* __restrict__ sm = reinterpret_cast<const T*>(G.src_exp_avg);
    const T* __restrict__ sv = reinterpret_cast<const T*>(G.src_exp_avg_sq);
    const T* __restrict__ ch = reinterpret_cast<const T*>(G.child);
    T* __restrict__ dp = reinterpret_cast<T*>(G.dst_param);
    T* __restrict__ dm = reinterpret_cast<T*>(G.dst_exp_avg);
    T* __restrict__ dv = reinterpret_cast<T*>(G.dst_exp_avg_sq);
    const int64_t row0 = base / w;                                              // wave-uniform
    const uint32_t col0 = (uint32_t)(base - row0 * w);
    for (int j = 0; j < per_thread; ++j) {
        const int t = (int)threadIdx.x + j * BLOCK;
        if (t >= count) break;
        const uint32_t u = col0 + (uint32_t)t;
        const int64_t r = row0 + u / w;
        const uint32_t col = u % w;
        const int64_t src = G.src_row[r];
        const int sl = G.slot[r];
        if (src < 0 || src >= G.n) continue;                                    // (a plan never writes such a row)
        const int64_t from = src * w + col;
        const T* const pp = (ch != nullptr && sl >= 2) ? ch + ((int64_t)(sl - 2) * G.n + src) * w + col : sp + from;
        dp[base + t] = *pp;
        if (sm != nullptr) {
            T m = zero_of<T>(), v = zero_of<T>();
            if (sl == 0) { m = sm[from]; v = sv[from]; }
            dm[base + t] = m;
            dv[base + t] = v;
        }
    }
}

__global__ void __launch_bounds__(BLOCK) densify_apply_kernel(const ApplyArgs a) {
    const uint32_t total = a.chunk_end[a.n - 1];
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int e = sc_find_entry(a.chunk_end, a.n, c);
        const sc_densify_group& G = a.g[e];
        const int64_t base = (int64_t)(c - (e ? a.chunk_end[e - 1] : 0u)) * APPLY_CHUNK;   // first element
        const int64_t left = G.n_out * G.width - base;
        const int count = left < APPLY_CHUNK ? (int)left : APPLY_CHUNK;
        const uintptr_t bits = (uintptr_t)G.src_param | (uintptr_t)G.dst_param | (uintptr_t)G.src_exp_avg |
                               (uintptr_t)G.src_exp_avg_sq | (uintptr_t)G.dst_exp_avg | (uintptr_t)G.dst_exp_avg_sq |
                               (uintptr_t)G.child;
        if ((G.width & 3) == 0 && (bits & 15u) == 0)    // (base and count are then multiples of 4 as well)
            apply_chunk<float4>(G, base >> 2, count >> 2, (uint32_t)G.width >> 2, APPLY_ITERS);
        else
            apply_chunk<float>(G, base, count, (uint32_t)G.width, 4 * APPLY_ITERS);
    }
}

int apply_launch(const ApplyArgs& a, hipStream_t stream) {
    const uint32_t total = a.chunk_end[a.n - 1];
    const unsigned grid = total < (uint32_t)MAX_GRID ? total : (uint32_t)MAX_GRID;
    hipLaunchKernelGGL(densify_apply_kernel, dim3(grid), dim3(BLOCK), 0, stream, a);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

}  // namespace

extern "C" int sc_densify_scan_block(void) { return BLOCK; }
extern "C" int sc_densify_max_jobs(void) { return PLAN_MAX; }
extern "C" int sc_densify_max_groups(void) { return APPLY_MAX; }

extern "C" size_t sc_densify_plan_workspace_bytes(const sc_densify_job* jobs_host, int n_jobs) {
    if (!job_sizes_ok(jobs_host, n_jobs)) return 0;
    size_t bytes = 0;
    for (int i = 0; i < n_jobs; ++i)
        if (jobs_host[i].n > 0) bytes += job_flags_bytes(jobs_host[i].n) + job_totals_bytes(jobs_host[i].n);
    return bytes;
}

extern "C" int sc_densify_plan(const sc_densify_job* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes,
                               sc_stream_t stream) {
    if (n_jobs == 0) return SC_OK;
    if (!job_sizes_ok(jobs_host, n_jobs)) return SC_EINVAL;
    for (int i = 0; i < n_jobs; ++i) {
        const sc_densify_job& j = jobs_host[i];
        if (j.counters == nullptr) return SC_EINVAL;
        if (j.grad_col < 0 || j.grad_col > 1 || j.region < 0 || j.region > 2 || !(j.max_grad > 0.0f)) return SC_EINVAL;
        if (j.n == 0) continue;
        if (!j.xyz || !j.scaling || !j.rotation || !j.opacity || !j.grad_accum || !j.denom || !j.max_radii ||
            !j.split_noise || !j.src_row || !j.slot || !j.child_xyz || !j.child_scaling)
            return SC_EINVAL;
        if (j.prune_big && j.region == 2 && !j.box_noise) return SC_EINVAL;
    }
    const size_t need = sc_densify_plan_workspace_bytes(jobs_host, n_jobs);
    if (need == 0) return SC_OK;                                        // every job is empty
    if (workspace == nullptr || workspace_bytes < need) return SC_EWORKSPACE;
    if ((uintptr_t)workspace & 15u) return SC_EINVAL;
    PlanArgs a;
    a.n = 0;
    int64_t chunks = 0;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    for (int i = 0; i < n_jobs; ++i) {
        const int64_t n = jobs_host[i].n;
        if (n == 0) continue;
        const int64_t c = (n + BLOCK - 1) / BLOCK;
        if (a.n == PLAN_MAX || chunks + c > MAX_CHUNKS) {               // the piece is full: launch it, start the next
            const int rc = plan_launch(a, sc_s(stream));
            if (rc) return rc;
            a.n = 0; chunks = 0;
        }
        chunks += c;
        a.j[a.n] = jobs_host[i];
        a.flags[a.n] = ws;
        a.totals[a.n] = reinterpret_cast<int32_t*>(ws + job_flags_bytes(n));
        ws += job_flags_bytes(n) + job_totals_bytes(n);
        a.chunk_end[a.n] = (uint32_t)chunks;
        ++a.n;
    }
    return a.n ? plan_launch(a, sc_s(stream)) : SC_OK;
}

extern "C" int sc_densify_apply(const sc_densify_group* groups_host, int n_groups, sc_stream_t stream) {
    if (n_groups == 0) return SC_OK;
    if (n_groups < 0 || groups_host == nullptr) return SC_EINVAL;
    for (int i = 0; i < n_groups; ++i) {
        const sc_densify_group& g = groups_host[i];
        if (g.n < 0 || g.n >= MAX_ROWS || g.n_out < 0 || g.n_out > 2 * g.n || g.width < 0) return SC_EINVAL;
        const int moments = (g.src_exp_avg != nullptr) + (g.src_exp_avg_sq != nullptr) + (g.dst_exp_avg != nullptr) +
                            (g.dst_exp_avg_sq != nullptr);
        if (moments != 0 && moments != 4) return SC_EINVAL;
        if (g.n_out * g.width == 0) continue;
        if (!g.src_param || !g.dst_param || !g.src_row || !g.slot) return SC_EINVAL;
        if ((g.n_out * g.width + APPLY_CHUNK - 1) / APPLY_CHUNK > MAX_CHUNKS) return SC_EINVAL;
    }
    ApplyArgs a;
    a.n = 0;
    int64_t chunks = 0;
    for (int i = 0; i < n_groups; ++i) {
        const int64_t c = (groups_host[i].n_out * groups_host[i].width + APPLY_CHUNK - 1) / APPLY_CHUNK;
        if (c == 0) continue;
        if (a.n == APPLY_MAX || chunks + c > MAX_CHUNKS) {
            const int rc = apply_launch(a, sc_s(stream));
            if (rc) return rc;
            a.n = 0; chunks = 0;
        }
        chunks += c;
        a.g[a.n] = groups_host[i];
        a.chunk_end[a.n] = (uint32_t)chunks;
        ++a.n;
    }
    return a.n ? apply_launch(a, sc_s(stream)) : SC_OK;
}
