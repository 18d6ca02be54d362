// Scene initialisation on the GPU (include/street_crafter_amd.h, "scene initialisation"): what stands between the raw
// LiDAR sweeps and the first trainable Gaussians in the reference.
//   sc_voxel_downsample_*    open3d voxel_down_sample        street_gaussian/pointcloud_processor/base_processor.py:85
//   sc_radius_outlier_mask   open3d remove_radius_outlier    base_processor.py:86
//   sc_point_bounds_*        the min / max of get_Sphere_Norm   street_gaussian/datasets/base_readers.py:81-82
//   sc_gaussian_init         the arithmetic of create_from_pcd  models/gaussian_model.py:59-80, gaussian_model_actor.py:129-157
//
// Both open3d calls are RESTATED (open3d's source is not vendored: DESIGN.md section 4).  Points are float64 and every
// decision is taken in float64: a voxel index is one subtraction and one IEEE division, a squared distance is
// (dx*dx + dy*dy) + dz*dz with every operation rounded on its own.
//
// Both build on one pipeline: bounds -> host (the bit widths of the cell key come from the extents) -> key = ix | iy | iz
// packed into as few bits as the extents need -> the stable radix sort of radix_sort.hip over exactly those bits with the
// input index as value -> segment heads -> scan -> compacted segment starts.
// The down-sampler then walks each segment in sorted order, which is ascending input index because the sort is stable:
// the float64 sums are sequential in input order, as open3d's accumulator loop adds them, so the means are the same bits
// from run to run and equal to the restatement's.  Nothing is reassociated; a crowded voxel is a long walk of one lane.
// The radius filter keeps a table of the occupied cells; the three z neighbours of a column are adjacent keys, so a point
// searches nine columns and scans nine contiguous ranges, and stops as soon as its count exceeds nb_points.
#include "sc_common.h"
#include <float.h>
#include <math.h>

// Contraction is off for the whole file (see frame_viz.hip on why helper intrinsics are not enough).
#pragma clang fp contract(off)

namespace {

constexpr int PC_BLK = 256;
constexpr int PC_BOUNDS_BLOCKS = 1024;       // block partials of the bounds pass
constexpr int PC_ROW = 8;                    // values per partial: lo[3], hi[3], non-finite count, pad

template <typename T> struct PcLimits;
template <> struct PcLimits<float> { static __device__ float inf() { return __builtin_huge_valf(); } };
template <> struct PcLimits<double> { static __device__ double inf() { return __builtin_huge_val(); } };

// min / max by comparison: exact in any order.  v[0..2] lo, v[3..5] hi, v[6] the number of non-finite values met
template <typename T> __device__ __forceinline__ void pc_merge(T* v, const T* o) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v[a] = o[a] < v[a] ? o[a] : v[a];
        v[3 + a] = o[3 + a] > v[3 + a] ? o[3 + a] : v[3 + a];
    }
    v[6] = v[6] + o[6];
}

template <typename T> __device__ __forceinline__ void pc_block_reduce_store(T* v, T* __restrict__ out) {
    __shared__ T red[PC_BLK][7];
#pragma unroll
    for (int k = 0; k < 7; ++k) red[threadIdx.x][k] = v[k];
    __syncthreads();
    for (int d = PC_BLK / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) {
            T o[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) o[k] = red[threadIdx.x + d][k];
            pc_merge(v, o);
#pragma unroll
            for (int k = 0; k < 7; ++k) red[threadIdx.x][k] = v[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) out[k] = v[k];
        out[7] = (T)0;
    }
}

template <typename T>
__global__ __launch_bounds__(PC_BLK) void pc_bounds_kernel(const T* __restrict__ xyz, int64_t n, T* __restrict__ partial) {
    T v[7];
#pragma unroll
    for (int a = 0; a < 3; ++a) { v[a] = PcLimits<T>::inf(); v[3 + a] = -PcLimits<T>::inf(); }
    v[6] = (T)0;
    for (int64_t i = (int64_t)blockIdx.x * PC_BLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * PC_BLK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const T x = xyz[i * 3 + a];
            if (!(x - x == (T)0)) { v[6] = (T)1; continue; }          // NaN or +-inf
            v[a] = x < v[a] ? x : v[a];
            v[3 + a] = x > v[3 + a] ? x : v[3 + a];
        }
    }
    pc_block_reduce_store(v, partial + (size_t)blockIdx.x * PC_ROW);
}

template <typename T>
__global__ __launch_bounds__(PC_BLK) void pc_bounds_finish_kernel(const T* __restrict__ partial, int nb, T* __restrict__ out) {
    T v[7];
#pragma unroll
    for (int a = 0; a < 3; ++a) { v[a] = PcLimits<T>::inf(); v[3 + a] = -PcLimits<T>::inf(); }
    v[6] = (T)0;
    for (int b = threadIdx.x; b < nb; b += PC_BLK) pc_merge(v, partial + (size_t)b * PC_ROW);
    pc_block_reduce_store(v, out);
}

inline int pc_bounds_blocks(int64_t n) {
    const int64_t b = (n + PC_BLK - 1) / PC_BLK;
    return (int)(b < PC_BOUNDS_BLOCKS ? b : PC_BOUNDS_BLOCKS);
}
constexpr size_t PC_BOUNDS_WS = (size_t)(PC_BOUNDS_BLOCKS + 1) * PC_ROW * sizeof(double);

// bounds_host[6] = lo xyz, hi xyz.  The call waits for the stream.  SC_EINVAL when a coordinate is not finite.
template <typename T> int pc_bounds(const T* xyz, int64_t n, T* bounds_host, void* ws, hipStream_t s) {
    T* partial = (T*)ws;
    T* out = partial + (size_t)PC_BOUNDS_BLOCKS * PC_ROW;
    const int nb = pc_bounds_blocks(n);
    hipLaunchKernelGGL(pc_bounds_kernel<T>, dim3(nb), dim3(PC_BLK), 0, s, xyz, n, partial);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(pc_bounds_finish_kernel<T>, dim3(1), dim3(PC_BLK), 0, s, (const T*)partial, nb, out);
    SC_LAUNCH_CHECK();
    T h[PC_ROW];
    SC_HIP(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    if (h[6] != (T)0) return SC_EINVAL;
    for (int k = 0; k < 6; ++k) bounds_host[k] = h[k];
    return SC_OK;
}

// ---- cell keys -------------------------------------------------------------------------------------------------------
struct PcGrid {
    double origin[3];      // vmin of the restatement
    double edge;
    int shift_x, shift_y;  // key = ix << shift_x | iy << shift_y | iz
};

__global__ __launch_bounds__(PC_BLK) void pc_key_kernel(const double* __restrict__ xyz, int64_t n, PcGrid g,
                                                        unsigned long long* __restrict__ keys, int* __restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * PC_BLK + threadIdx.x;
    if (i >= n) return;
    unsigned long long q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double d = xyz[i * 3 + a] - g.origin[a];         // one subtraction,
        const double f = floor(d / g.edge);                    // one IEEE division
        q[a] = f > 0.0 ? (unsigned long long)f : 0ull;
    }
    keys[i] = (q[0] << g.shift_x) | (q[1] << g.shift_y) | q[2];
    ids[i] = (int)i;
}

// ---- segment heads -> compacted segment starts -----------------------------------------------------------------------
__device__ __forceinline__ bool pc_is_head(const unsigned long long* __restrict__ keys, int64_t i, int64_t n) {
    return i < n && (i == 0 || keys[i] != keys[i - 1]);
}

__global__ __launch_bounds__(PC_BLK) void pc_head_count_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                               unsigned* __restrict__ block_count) {
    __shared__ unsigned wsum[PC_BLK / 64];
    const int64_t i = (int64_t)blockIdx.x * PC_BLK + threadIdx.x;
    const unsigned long long b = __ballot(pc_is_head(keys, i, n));
    if (sc_lane() == 0) wsum[threadIdx.x >> 6] = (unsigned)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: exclusive scan of the block counts in place; the total to *total and n behind the last segment start
__global__ __launch_bounds__(PC_BLK) void pc_scan_blocks_kernel(unsigned* __restrict__ block_count, unsigned nb,
                                                                long long* __restrict__ total, int* __restrict__ seg_start,
                                                                int64_t n) {
    __shared__ unsigned wave_tot[4];
    __shared__ unsigned carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int lane = sc_lane(), wave = threadIdx.x >> 6;
    for (unsigned base = 0; base < nb; base += PC_BLK) {
        const unsigned i = base + threadIdx.x;
        const unsigned v = (i < nb) ? block_count[i] : 0u;
        const unsigned incl = (unsigned)sc_wave_incl_scan((int)v);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        unsigned pre = carry_s, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned s = wave_tot[w];
            if (w < wave) pre += s;
            tot += s;
        }
        if (i < nb) block_count[i] = pre + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) carry_s += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *total = (long long)carry_s;
        seg_start[carry_s] = (int)n;          // carry_s <= n: the table has n + 1 entries
    }
}

__global__ __launch_bounds__(PC_BLK) void pc_head_scatter_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                                 const unsigned* __restrict__ block_offset,
                                                                 int* __restrict__ seg_start,
                                                                 unsigned long long* __restrict__ seg_key /* nullable */) {
    __shared__ unsigned wsum[PC_BLK / 64];
    const int64_t i = (int64_t)blockIdx.x * PC_BLK + threadIdx.x;
    const bool head = pc_is_head(keys, i, n);
    const unsigned long long b = __ballot(head);
    const int wave = threadIdx.x >> 6;
    if (sc_lane() == 0) wsum[wave] = (unsigned)__popcll(b);
    __syncthreads();
    if (!head) return;
    unsigned pos = block_offset[blockIdx.x] + (unsigned)__popcll(b & sc_lanemask_lt());
    for (int w = 0; w < wave; ++w) pos += wsum[w];
    seg_start[pos] = (int)i;                  // pos < number of heads <= n
    if (seg_key) seg_key[pos] = keys[i];
}

// ---- voxel means: one lane per voxel, sequential float64 sums in sorted order = ascending input index ----------------
__global__ __launch_bounds__(PC_BLK) void pc_voxel_reduce_kernel(const double* __restrict__ xyz,
                                                                 const double* __restrict__ colors /* nullable */,
                                                                 const int* __restrict__ ids, const int* __restrict__ seg_start,
                                                                 const long long* __restrict__ m_dev, int64_t m_cap, int64_t n,
                                                                 double* __restrict__ out_points,
                                                                 double* __restrict__ out_colors /* nullable */,
                                                                 int* __restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * PC_BLK + threadIdx.x;
    const int64_t m = *m_dev < m_cap ? *m_dev : m_cap;
    if (s >= m) return;
    int64_t b = seg_start[s], e = seg_start[s + 1];
    b = b < 0 ? 0 : b;
    e = e > n ? n : e;
    double px = 0.0, py = 0.0, pz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
    int cnt = 0;
#pragma unroll 4
    for (int64_t j = b; j < e; ++j) {
        const int64_t id = ids[j];
        if (id < 0 || id >= n) continue;
        px += xyz[id * 3 + 0]; py += xyz[id * 3 + 1]; pz += xyz[id * 3 + 2];
        if (colors) { cr += colors[id * 3 + 0]; cg += colors[id * 3 + 1]; cb += colors[id * 3 + 2]; }
        ++cnt;
    }
    const double c = (double)cnt;
    out_points[s * 3 + 0] = px / c; out_points[s * 3 + 1] = py / c; out_points[s * 3 + 2] = pz / c;
    if (colors && out_colors) { out_colors[s * 3 + 0] = cr / c; out_colors[s * 3 + 1] = cg / c; out_colors[s * 3 + 2] = cb / c; }
    counts[s] = cnt;
}

// the longest segment (reported by the measuring tool; no part of the result).  *longest is zeroed before the launch
__global__ __launch_bounds__(PC_BLK) void pc_longest_segment_kernel(const int* __restrict__ seg_start,
                                                                    const long long* __restrict__ m_dev,
                                                                    int* __restrict__ longest) {
    __shared__ int red[PC_BLK];
    const long long m = *m_dev;
    int best = 0;
    for (long long s = (long long)blockIdx.x * PC_BLK + threadIdx.x; s < m; s += (long long)gridDim.x * PC_BLK)
        best = max(best, seg_start[s + 1] - seg_start[s]);
    red[threadIdx.x] = best;
    __syncthreads();
    for (int d = PC_BLK / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0] > 0) atomicMax(longest, red[0]);
}

// ---- radius filter ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_BLK) void pc_gather_kernel(const double* __restrict__ xyz, const int* __restrict__ ids,
                                                           int64_t n, double* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * PC_BLK + threadIdx.x;
    if (i >= n) return;
    int64_t src = ids[i];
    src = src < 0 ? 0 : (src >= n ? n - 1 : src);
#pragma unroll
    for (int a = 0; a < 3; ++a) sorted[i * 3 + a] = xyz[src * 3 + a];
}

struct PcCells {
    int bx, by, bz;        // key bits per axis
};

// true when more than nb points (self included) lie at d2 < r2
__device__ __forceinline__ bool pc_has_more_than(const double* __restrict__ sp, const unsigned long long* __restrict__ seg_key,
                                                 const int* __restrict__ seg_start, int U, int64_t n, PcCells c,
                                                 unsigned long long key, double px, double py, double pz, double r2, int nb) {
    const long long mx = (1ll << c.bx) - 1, my = (1ll << c.by) - 1, mz = (1ll << c.bz) - 1;
    const long long iz = (long long)(key & (unsigned long long)mz);
    const long long iy = (long long)((key >> c.bz) & (unsigned long long)my);
    const long long ix = (long long)(key >> (c.by + c.bz));
    const long long zlo = iz > 0 ? iz - 1 : 0, zhi = iz < mz ? iz + 1 : mz;
    int cnt = 0;
    for (long long x = ix - 1; x <= ix + 1; ++x) {
        if (x < 0 || x > mx) continue;
        for (long long y = iy - 1; y <= iy + 1; ++y) {
            if (y < 0 || y > my) continue;
            const unsigned long long col = ((unsigned long long)x << (c.by + c.bz)) | ((unsigned long long)y << c.bz);
            const unsigned long long klo = col | (unsigned long long)zlo, khi = col | (unsigned long long)zhi;
            int lo = 0, hi = U;                                   // first occupied cell with key >= klo
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (seg_key[mid] < klo) lo = mid + 1; else hi = mid;
            }
            int u = lo;
            while (u < U && seg_key[u] <= khi) ++u;               // at most three cells
            if (u == lo) continue;
            int64_t b = seg_start[lo], e = seg_start[u];          // u <= U: seg_start[U] = n
            b = b < 0 ? 0 : b;
            e = e > n ? n : e;
            for (int64_t j = b; j < e; ++j) {
                const double dx = px - sp[j * 3 + 0], dy = py - sp[j * 3 + 1], dz = pz - sp[j * 3 + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < r2 && ++cnt > nb) return true;
            }
        }
    }
    return false;
}

__global__ __launch_bounds__(PC_BLK) void pc_radius_count_kernel(const double* __restrict__ sp,
                                                                 const unsigned long long* __restrict__ keys,
                                                                 const int* __restrict__ ids,
                                                                 const unsigned long long* __restrict__ seg_key,
                                                                 const int* __restrict__ seg_start,
                                                                 const long long* __restrict__ u_dev, int64_t n, PcCells c,
                                                                 double r2, int nb, uint8_t* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * PC_BLK + threadIdx.x;
    if (i >= n) return;
    long long U = *u_dev;
    U = U < 0 ? 0 : (U > n ? n : U);
    const bool k = pc_has_more_than(sp, seg_key, seg_start, (int)U, n, c, keys[i], sp[i * 3 + 0], sp[i * 3 + 1],
                                    sp[i * 3 + 2], r2, nb);
    const int64_t dst = ids[i];
    if (dst >= 0 && dst < n) keep[dst] = k ? 1 : 0;
}

// ---- first Gaussians -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PC_BLK) void pc_gaussian_init_kernel(const float* __restrict__ rgb, const float* __restrict__ dist2,
                                                                  int64_t m, int F, int64_t n_rest_words, int64_t n_sem_words,
                                                                  float opacity, float* __restrict__ features_dc,
                                                                  float* __restrict__ features_rest, float* __restrict__ scaling,
                                                                  float* __restrict__ rotation, float* __restrict__ opacity_out,
                                                                  float* __restrict__ semantic, float* __restrict__ max_radii2d) {
    const int64_t i = (int64_t)blockIdx.x * PC_BLK + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * PC_BLK;
    if (i < m) {
        float* dc = features_dc + i * 3 * F;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) dc[ch] = (rgb[i * 3 + ch] - 0.5f) / 0.28209479177387814f;      // RGB2SH
        for (int k = 3; k < 3 * F; ++k) dc[k] = 0.f;
        const float d = dist2[i];
        const float s = logf(sqrtf(d < 1e-7f ? 1e-7f : d));          // clamp_min: a NaN stays a NaN
#pragma unroll
        for (int a = 0; a < 3; ++a) scaling[i * 3 + a] = s;
        rotation[i * 4 + 0] = 1.f; rotation[i * 4 + 1] = 0.f; rotation[i * 4 + 2] = 0.f; rotation[i * 4 + 3] = 0.f;
        opacity_out[i] = opacity;
        max_radii2d[i] = 0.f;
    }
    for (int64_t k = i; k < n_rest_words; k += stride) features_rest[k] = 0.f;
    for (int64_t k = i; k < n_sem_words; k += stride) semantic[k] = 0.f;
}

// ---- host side -------------------------------------------------------------------------------------------------------
struct PcLayout {
    size_t bounds, keys, tmp_keys, ids, tmp_ids, block_count, scalars, sort_ws, seg_key, sorted, total;
};
// scalars: [0] long long number of segments, [1] int longest segment
PcLayout pc_layout(int64_t n, bool radius) {
    PcLayout L;
    size_t o = 0;
    L.bounds = o; o += sc_align_up(PC_BOUNDS_WS, 256);
    L.keys = o; o += sc_align_up((size_t)n * 8, 256);
    L.tmp_keys = o; o += sc_align_up((size_t)n * 8 + 8, 256);      // after the sort: int seg_start[n + 1]
    L.ids = o; o += sc_align_up((size_t)n * 4, 256);
    L.tmp_ids = o; o += sc_align_up((size_t)n * 4, 256);
    L.block_count = o; o += sc_align_up((size_t)((n + PC_BLK - 1) / PC_BLK) * 4, 256);
    L.scalars = o; o += 256;
    L.sort_ws = o; o += sc_radix_sort_workspace_bytes(n);
    L.seg_key = o; o += radius ? sc_align_up((size_t)n * 8, 256) : 0;
    L.sorted = o; o += radius ? sc_align_up((size_t)n * 24, 256) : 0;
    L.total = o;
    return L;
}

int pc_bits(unsigned long long v) {
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

// keys of the cells of edge `edge` from `origin`, sorted over exactly the bits the extents need, and the compacted
// segment table.  bits[3] on return; SC_EINVAL when an axis needs more than max_axis_bits or the three more than 63.
int pc_sorted_cells(const double* xyz, int64_t n, const double* origin, const double* hi, double edge, int max_axis_bits,
                    unsigned char* ws, const PcLayout& L, bool with_keys, int bits[3], sc_stream_t stream) {
    for (int a = 0; a < 3; ++a) {
        const double q = floor((hi[a] - origin[a]) / edge);        // the kernel's expression on the largest coordinate
        if (!(q >= 0.0) || !(q < 4611686018427387904.0)) return SC_EINVAL;
        bits[a] = pc_bits((unsigned long long)q);
        if (bits[a] > max_axis_bits) return SC_EINVAL;
    }
    const int end_bit = bits[0] + bits[1] + bits[2];
    if (end_bit > 63) return SC_EINVAL;
    PcGrid g;
    for (int a = 0; a < 3; ++a) g.origin[a] = origin[a];
    g.edge = edge;
    g.shift_x = bits[1] + bits[2];
    g.shift_y = bits[2];
    hipStream_t s = sc_s(stream);
    unsigned long long* keys = (unsigned long long*)(ws + L.keys);
    int* ids = (int*)(ws + L.ids);
    const unsigned nb = (unsigned)((n + PC_BLK - 1) / PC_BLK);
    hipLaunchKernelGGL(pc_key_kernel, dim3(nb), dim3(PC_BLK), 0, s, xyz, n, g, keys, ids);
    SC_LAUNCH_CHECK();
    const int rc = sc_radix_sort_pairs_u64_i32((uint64_t*)keys, ids, (uint64_t*)(ws + L.tmp_keys), (int*)(ws + L.tmp_ids), n,
                                               end_bit, ws + L.sort_ws, sc_radix_sort_workspace_bytes(n), stream);
    if (rc != SC_OK) return rc;
    unsigned* block_count = (unsigned*)(ws + L.block_count);
    int* seg_start = (int*)(ws + L.tmp_keys);
    long long* total = (long long*)(ws + L.scalars);
    hipLaunchKernelGGL(pc_head_count_kernel, dim3(nb), dim3(PC_BLK), 0, s, (const unsigned long long*)keys, n, block_count);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(pc_scan_blocks_kernel, dim3(1), dim3(PC_BLK), 0, s, block_count, nb, total, seg_start, n);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(pc_head_scatter_kernel, dim3(nb), dim3(PC_BLK), 0, s, (const unsigned long long*)keys, n,
                       (const unsigned*)block_count, seg_start,
                       with_keys ? (unsigned long long*)(ws + L.seg_key) : (unsigned long long*)nullptr);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

bool pc_finite(double v) { return v - v == 0.0; }

}  // namespace

extern "C" size_t sc_point_bounds_workspace_bytes(void) { return PC_BOUNDS_WS; }

extern "C" int sc_point_bounds_f32(const float* xyz, int64_t n, float* bounds_host, void* workspace, size_t ws_bytes,
                                   sc_stream_t stream) {
    if (n <= 0 || n > 0x7fffffffLL || !xyz || !bounds_host || !workspace) return SC_EINVAL;
    if (ws_bytes < PC_BOUNDS_WS) return SC_EWORKSPACE;
    return pc_bounds<float>(xyz, n, bounds_host, workspace, sc_s(stream));
}

extern "C" int sc_point_bounds_f64(const double* xyz, int64_t n, double* bounds_host, void* workspace, size_t ws_bytes,
                                   sc_stream_t stream) {
    if (n <= 0 || n > 0x7fffffffLL || !xyz || !bounds_host || !workspace) return SC_EINVAL;
    if (ws_bytes < PC_BOUNDS_WS) return SC_EWORKSPACE;
    return pc_bounds<double>(xyz, n, bounds_host, workspace, sc_s(stream));
}

extern "C" size_t sc_voxel_downsample_workspace_bytes(int64_t n) {
    if (n <= 0) return 256;
    return pc_layout(n, false).total;
}

extern "C" int sc_voxel_downsample_plan(const double* xyz, int64_t n, double voxel_size, void* workspace, size_t ws_bytes,
                                        int64_t* m_host, int32_t* info_host, sc_stream_t stream) {
    if (n <= 0 || n > 0x7fffffffLL || !(voxel_size > 0.0) || !pc_finite(voxel_size)) return SC_EINVAL;
    if (!xyz || !workspace || !m_host) return SC_EINVAL;
    const PcLayout L = pc_layout(n, false);
    if (ws_bytes < L.total) return SC_EWORKSPACE;
    unsigned char* ws = (unsigned char*)workspace;
    hipStream_t s = sc_s(stream);
    double b[6];
    int rc = pc_bounds<double>(xyz, n, b, ws + L.bounds, s);
    if (rc != SC_OK) return rc;
    double vmin[3];
    const double half = 0.5 * voxel_size;
    for (int a = 0; a < 3; ++a) {
        vmin[a] = b[a] - half;
        if (!pc_finite(vmin[a])) return SC_EINVAL;
    }
    int bits[3];
    rc = pc_sorted_cells(xyz, n, vmin, b + 3, voxel_size, 63, ws, L, false, bits, stream);
    if (rc != SC_OK) return rc;
    long long* scalars = (long long*)(ws + L.scalars);
    SC_HIP(hipMemsetAsync(scalars + 1, 0, sizeof(long long), s));
    hipLaunchKernelGGL(pc_longest_segment_kernel, dim3(pc_bounds_blocks(n)), dim3(PC_BLK), 0, s, (const int*)(ws + L.tmp_keys),
                       (const long long*)scalars, (int*)(scalars + 1));
    SC_LAUNCH_CHECK();
    long long h[2] = {0, 0};
    SC_HIP(hipMemcpyAsync(h, scalars, sizeof(h), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *m_host = (int64_t)h[0];
    if (info_host) {
        info_host[0] = bits[0]; info_host[1] = bits[1]; info_host[2] = bits[2];
        info_host[3] = (int32_t)(h[1] & 0xffffffffll);
    }
    return SC_OK;
}

extern "C" int sc_voxel_downsample_reduce(const double* xyz, const double* colors, int64_t n, int64_t m,
                                          const void* workspace, size_t ws_bytes, double* points, double* colors_out,
                                          int32_t* counts, sc_stream_t stream) {
    if (n <= 0 || n > 0x7fffffffLL || m < 0 || m > n) return SC_EINVAL;
    if (m == 0) return SC_OK;
    if (!xyz || !workspace || !points || !counts || (colors && !colors_out)) return SC_EINVAL;
    const PcLayout L = pc_layout(n, false);
    if (ws_bytes < L.total) return SC_EWORKSPACE;
    const unsigned char* ws = (const unsigned char*)workspace;
    hipLaunchKernelGGL(pc_voxel_reduce_kernel, dim3((unsigned)((m + PC_BLK - 1) / PC_BLK)), dim3(PC_BLK), 0, sc_s(stream),
                       xyz, colors, (const int*)(ws + L.ids), (const int*)(ws + L.tmp_keys),
                       (const long long*)(ws + L.scalars), m, n, points, colors_out, counts);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" size_t sc_radius_outlier_workspace_bytes(int64_t m) {
    if (m <= 0) return 256;
    return pc_layout(m, true).total;
}

extern "C" int sc_radius_outlier_mask(const double* xyz, int64_t m, int nb_points, double radius, uint8_t* keep,
                                      void* workspace, size_t ws_bytes, int32_t* info_host, sc_stream_t stream) {
    if (m < 0 || m > 0x7fffffffLL || nb_points < 0 || !(radius > 0.0) || !pc_finite(radius)) return SC_EINVAL;
    if (m == 0) return SC_OK;
    if (!xyz || !keep || !workspace) return SC_EINVAL;
    const double r2 = radius * radius;
    if (!(r2 > 0.0) || !pc_finite(r2)) return SC_EINVAL;
    const PcLayout L = pc_layout(m, true);
    if (ws_bytes < L.total) return SC_EWORKSPACE;
    unsigned char* ws = (unsigned char*)workspace;
    hipStream_t s = sc_s(stream);
    double b[6];
    int rc = pc_bounds<double>(xyz, m, b, ws + L.bounds, s);
    if (rc != SC_OK) return rc;
    // Cells a hair wider than the radius: two points that the rounded d2 < r2 accepts differ by at most r (1 + 2^-51)
    // per axis, and their rounded cell coordinates (at most 26 bits) then differ by less than 1, so neighbours are
    // always in adjacent cells however the divisions round.
    const double edge = radius * (1.0 + 1.0 / 1048576.0);
    int bits[3];
    rc = pc_sorted_cells(xyz, m, b, b + 3, edge, 26, ws, L, true, bits, stream);
    if (rc != SC_OK) return rc;
    const unsigned nb = (unsigned)((m + PC_BLK - 1) / PC_BLK);
    double* sorted = (double*)(ws + L.sorted);
    hipLaunchKernelGGL(pc_gather_kernel, dim3(nb), dim3(PC_BLK), 0, s, xyz, (const int*)(ws + L.ids), m, sorted);
    SC_LAUNCH_CHECK();
    PcCells c;
    c.bx = bits[0]; c.by = bits[1]; c.bz = bits[2];
    hipLaunchKernelGGL(pc_radius_count_kernel, dim3(nb), dim3(PC_BLK), 0, s, (const double*)sorted,
                       (const unsigned long long*)(ws + L.keys), (const int*)(ws + L.ids),
                       (const unsigned long long*)(ws + L.seg_key), (const int*)(ws + L.tmp_keys),
                       (const long long*)(ws + L.scalars), m, c, r2, nb_points, keep);
    SC_LAUNCH_CHECK();
    if (info_host) { info_host[0] = bits[0]; info_host[1] = bits[1]; info_host[2] = bits[2]; }
    return SC_OK;
}

extern "C" int sc_gaussian_init(const float* rgb, const float* dist2, int64_t m, int fourier_dim, int n_rest, int num_classes,
                                float opacity, float* features_dc, float* features_rest, float* scaling, float* rotation,
                                float* opacity_out, float* semantic, float* max_radii2d, sc_stream_t stream) {
    if (m < 0 || m > 0x7fffffffLL || fourier_dim < 1 || n_rest < 0 || num_classes < 0) return SC_EINVAL;
    if (m == 0) return SC_OK;
    if (!rgb || !dist2 || !features_dc || !scaling || !rotation || !opacity_out || !max_radii2d) return SC_EINVAL;
    if ((n_rest > 0 && !features_rest) || (num_classes > 0 && !semantic)) return SC_EINVAL;
    hipLaunchKernelGGL(pc_gaussian_init_kernel, dim3((unsigned)((m + PC_BLK - 1) / PC_BLK)), dim3(PC_BLK), 0, sc_s(stream),
                       rgb, dist2, m, fourier_dim, m * n_rest * 3, m * num_classes, opacity, features_dc, features_rest,
                       scaling, rotation, opacity_out, semantic, max_radii2d);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
