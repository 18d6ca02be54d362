// The cameras' gradient of fully_fused_projection (gsplat's v_viewmats) and of the camera centres -R^T t, for gfx950.
//
// Per (camera c, Gaussian n) with radii > 0, with v_pc = dL/d(W m + t) and the symmetric vSc = dL/dSigma_c of
// proj_bwd_camera_core (Sigma_c = W Sigma W^T; the Jacobian's clamp limits depend on Ks alone):
//     v_t += v_pc          v_W += v_pc m^T + 2 vSc W Sigma
// One thread per Gaussian loops over the cameras as projection_bwd_kernel does.  The 12 sums of a camera are reduced
// without float atomics, so the result is the same bits from run to run: across the wave (sc_wave_sum), across the
// block's four waves through LDS in wave order, one partial row [12] per (camera, block) in the workspace, and a second
// kernel -- one block per camera -- that adds the rows in a fixed order in double.  Rows that take no part (n >= N,
// radii <= 0) contribute by SELECTION: their leaves are never multiplied into a sum.
//
// The per-Gaussian gradients of sc_projection_bwd_cam are written by projection_bwd_kernel itself (sc_projection_bwd), a
// launch of its own.  A kernel that produced them from the same recompute as the camera sums was built and gave other
// bits than sc_projection_bwd on most rows of v_quats / v_scales (a few ulps; up to 181 of 257 rows): these helpers are
// compiled with FMA contraction allowed, and which products the compiler fuses or packs depends on the code around them.
// Bit-equality with sc_projection_bwd -- a training run must not change when its cameras start to learn -- is only to
// be had from the same machine code, so the recompute is paid twice when both are asked for.
#include "projection_common.h"

namespace {

constexpr int CAM_BLOCK = 256;                  // threads of the per-Gaussian pass (as projection_bwd_kernel)
constexpr int CAM_WAVES = CAM_BLOCK / SC_WAVE;
constexpr int CAM_REDUCE = 1024;                // threads of the per-camera reduction
constexpr int CAM_REDUCE_WAVES = CAM_REDUCE / SC_WAVE;

__global__ __launch_bounds__(CAM_BLOCK) void projection_bwd_cam_kernel(
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ viewmats, const float* __restrict__ Ks, int C, int N, int width,
    int height, float eps2d, ProjOpt opt, const int32_t* __restrict__ radii, const float* __restrict__ conics,
    const float* __restrict__ comps, const float* __restrict__ v_means2d,
    const float* __restrict__ v_depths, const float* __restrict__ v_conics,
    const float* __restrict__ v_comps, float* __restrict__ partial /* [C][gridDim.x][12] */) {
    __shared__ float red[2][CAM_WAVES][12];
    const int n = blockIdx.x * CAM_BLOCK + threadIdx.x;
    const bool in = n < N;               // (no early return: every thread reaches every barrier)
    const int wave = (int)(threadIdx.x >> 6);
    ProjBwdPre pre = {};
    if (in) pre = proj_bwd_setup(means, quats, scales, n);

    for (int cam = 0; cam < C; ++cam) {
        const size_t o = (size_t)cam * N + (in ? n : 0);
        const bool live = in && radii[o] > 0;
        float s[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // v_W row-major [9], v_t [3]
        if (live) {
            const ProjBwdCam f = proj_bwd_recompute(pre, viewmats + cam * 16, Ks + cam * 9, width, height, eps2d, opt);
            const bool has_comp = v_comps && comps;
            float gm[3] = {0.f, 0.f, 0.f}, vS[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};      // (not used here)
            float v_pc[3], vSc[3][3];
            proj_bwd_camera_core(f, conics[o * 3 + 0], conics[o * 3 + 1], conics[o * 3 + 2], v_conics[o * 3 + 0],
                                 v_conics[o * 3 + 1], v_conics[o * 3 + 2], has_comp, has_comp ? comps[o] : 0.f,
                                 has_comp ? v_comps[o] : 0.f, v_means2d[o * 2 + 0], v_means2d[o * 2 + 1], v_depths[o], gm, vS,
                                 v_pc, vSc);
            // v_W = v_pc m^T + 2 (vSc W) Sigma
            const float m[3] = {pre.mx, pre.my, pre.mz};
            float Q[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Q[i][j] = vSc[i][0] * f.Wm[0][j] + vSc[i][1] * f.Wm[1][j] + vSc[i][2] * f.Wm[2][j];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    s[i * 3 + j] = v_pc[i] * m[j] + 2.f * (Q[i][0] * pre.S[0][j] + Q[i][1] * pre.S[1][j] + Q[i][2] * pre.S[2][j]);
                s[9 + i] = v_pc[i];
            }
        }
        // a wave without a live row adds exact zeros either way: it skips the shuffles (wave-uniform)
        if (__any(live)) {
#pragma unroll
            for (int k = 0; k < 12; ++k) s[k] = sc_wave_sum(s[k]);
        }
        float (*r)[12] = red[cam & 1];      // two buffers: one barrier per camera
        if (sc_lane() == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) r[wave][k] = s[k];
        }
        __syncthreads();
        if (threadIdx.x < 12) {
            float t = r[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < CAM_WAVES; ++w) t += r[w][threadIdx.x];
            partial[((size_t)cam * gridDim.x + blockIdx.x) * 12 + threadIdx.x] = t;
        }
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// One block per camera: thread t adds the partial rows t, t + 1024, ... in that order, the wave and then the block add
// the threads' sums in a fixed order, all in double; 16 floats out (bottom row +0).  nb == 0: 16 zeros.
__global__ __launch_bounds__(CAM_REDUCE) void projection_cam_reduce_kernel(const float* __restrict__ partial, int nb,
                                                                           float* __restrict__ v_viewmats) {
    __shared__ double red[CAM_REDUCE_WAVES][12];
    const int cam = blockIdx.x;
    const float4* rows = reinterpret_cast<const float4*>(partial + (size_t)cam * nb * 12);      // 48-B rows, 16-B aligned
    double a[12] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
    for (int b = (int)threadIdx.x; b < nb; b += CAM_REDUCE) {
        const float4 p0 = rows[(size_t)b * 3 + 0], p1 = rows[(size_t)b * 3 + 1], p2 = rows[(size_t)b * 3 + 2];
        a[0] += (double)p0.x; a[1] += (double)p0.y; a[2] += (double)p0.z; a[3] += (double)p0.w;
        a[4] += (double)p1.x; a[5] += (double)p1.y; a[6] += (double)p1.z; a[7] += (double)p1.w;
        a[8] += (double)p2.x; a[9] += (double)p2.y; a[10] += (double)p2.z; a[11] += (double)p2.w;
    }
    const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double t = wave_sum_f64(a[k]);
        if (sc_lane() == 0) red[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int row = (int)threadIdx.x >> 2, col = (int)threadIdx.x & 3;
        float out = 0.f;
        if (row < 3) {
            const int k = col < 3 ? row * 3 + col : 9 + row;        // [v_W | v_t]
            double t = red[0][k];
            for (int w = 1; w < CAM_REDUCE_WAVES; ++w) t += red[w][k];
            out = (float)t;
        }
        v_viewmats[(size_t)cam * 16 + threadIdx.x] = out;
    }
}

// VJP of c = -R^T t: v_t = -R v_c, v_R = -t v_c^T.  One thread per camera.
__global__ void camera_centers_bwd_kernel(const float* __restrict__ viewmats, const float* __restrict__ v_centers, int C,
                                          float* __restrict__ v_viewmats) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const float* V = viewmats + (size_t)c * 16;
    float* o = v_viewmats + (size_t)c * 16;
    const float g0 = v_centers[c * 3 + 0], g1 = v_centers[c * 3 + 1], g2 = v_centers[c * 3 + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t = V[i * 4 + 3];
        o[i * 4 + 0] = -(t * g0);
        o[i * 4 + 1] = -(t * g1);
        o[i * 4 + 2] = -(t * g2);
        o[i * 4 + 3] = -(V[i * 4 + 0] * g0 + V[i * 4 + 1] * g1 + V[i * 4 + 2] * g2);
    }
    o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 0.f;
}

}  // namespace

static inline int64_t cam_partial_bytes(int C, int N) {
    return (int64_t)C * ((N + (int64_t)CAM_BLOCK - 1) / CAM_BLOCK) * 12 * (int64_t)sizeof(float);
}

// the partial rows, then room for the per-Gaussian outputs a caller does not want (projection_bwd_kernel writes all three)
extern "C" int64_t sc_projection_bwd_cam_workspace_bytes(int C, int N) {
    if (C <= 0 || N <= 0) return 0;
    return cam_partial_bytes(C, N) + (int64_t)N * 10 * (int64_t)sizeof(float);
}

extern "C" int sc_projection_bwd_cam(const float* means, const float* quats, const float* scales,
                                     const float* viewmats, const float* Ks, int C, int N, int width,
                                     int height, float eps2d, const int32_t* radii, const float* conics,
                                     const float* compensations, const float* v_means2d,
                                     const float* v_depths, const float* v_conics,
                                     const float* v_compensations, float* v_means, float* v_quats,
                                     float* v_scales, float* v_viewmats, void* workspace, sc_stream_t stream) {
    if (C < 0 || N < 0 || width <= 0 || height <= 0) return SC_EINVAL;
    if (C > 0 && !v_viewmats) return SC_EINVAL;
    if (N > 0 && C > 0) {
        if (!means || !quats || !scales || !viewmats || !Ks || !radii || !conics || !v_means2d || !v_depths || !v_conics ||
            !workspace)
            return SC_EINVAL;
        if ((uintptr_t)workspace & 15) return SC_EINVAL;
    }
    const bool gauss = v_means || v_quats || v_scales;
    if (C == 0) {       // no camera: nothing to sum, and the rows anybody wants are zeros (as sc_projection_bwd writes them)
        if (v_means && N) SC_HIP(hipMemsetAsync(v_means, 0, (size_t)N * 3 * sizeof(float), sc_s(stream)));
        if (v_quats && N) SC_HIP(hipMemsetAsync(v_quats, 0, (size_t)N * 4 * sizeof(float), sc_s(stream)));
        if (v_scales && N) SC_HIP(hipMemsetAsync(v_scales, 0, (size_t)N * 3 * sizeof(float), sc_s(stream)));
        return SC_OK;
    }
    const int nb = (N + CAM_BLOCK - 1) / CAM_BLOCK;
    if (N > 0) {
        if (gauss) {
            // the same machine code as sc_projection_bwd: the same bits.  What the caller left null lands in the workspace.
            float* spare = reinterpret_cast<float*>(static_cast<char*>(workspace) + cam_partial_bytes(C, N));       // 16-B aligned
            const int rc = sc_projection_bwd(means, quats, scales, viewmats, Ks, C, N, width, height, eps2d, radii, conics,
                                             compensations, v_means2d, v_depths, v_conics, v_compensations,
                                             v_means ? v_means : spare + (size_t)N * 4, v_quats ? v_quats : spare,
                                             v_scales ? v_scales : spare + (size_t)N * 7, stream);
            if (rc != SC_OK) return rc;
        }
        hipLaunchKernelGGL(projection_bwd_cam_kernel, dim3(nb), dim3(CAM_BLOCK), 0, sc_s(stream), means, quats, scales,
                           viewmats, Ks, C, N, width, height, eps2d, sc_proj_opt(), radii, conics, compensations,
                           v_means2d, v_depths, v_conics, v_compensations, (float*)workspace);
        SC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(projection_cam_reduce_kernel, dim3(C), dim3(CAM_REDUCE), 0, sc_s(stream),
                       (const float*)workspace, nb, v_viewmats);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_camera_centers_bwd(const float* viewmats, const float* v_centers, int C, float* v_viewmats,
                                     sc_stream_t stream) {
    if (C < 0) return SC_EINVAL;
    if (C == 0) return SC_OK;
    if (!viewmats || !v_centers || !v_viewmats) return SC_EINVAL;
    hipLaunchKernelGGL(camera_centers_bwd_kernel, dim3((C + 63) / 64), dim3(64), 0, sc_s(stream), viewmats, v_centers, C,
                       v_viewmats);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
