// a1: fully_fused_projection forward / backward for gfx950.
// Replaces gsplat.rendering.fully_fused_projection as called at
// street_gaussian/models/street_gaussian_renderer.py:219-232 (semantics: SURVEY.md A.1).
//
// HBM-bound streaming kernel: 40 B in / 32 B out per Gaussian, one lane per (camera, gaussian).
// The forward feeds INTEGER decisions downstream (radii -> tile rectangles, depth bits -> sort
// key), so it is compiled without FMA contraction and mirrors oracle/gsplat_oracle.py's op
// order exactly: its outputs are bit-identical to the oracle's, not merely close.
#include "projection_common.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void projection_fwd_kernel(
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ viewmats, const float* __restrict__ Ks, int N, int width, int height,
    float eps2d, float near_plane, float far_plane, float radius_clip, ProjOpt opt,
    int32_t* __restrict__ radii, float* __restrict__ means2d, float* __restrict__ depths,
    float* __restrict__ conics, float* __restrict__ comps) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int cam = blockIdx.y;
    if (n >= N) return;
    const Cam c = load_cam(viewmats + cam * 16, Ks + cam * 9);
    const size_t o = (size_t)cam * N + n;

    const ProjOut p = project_one(c, means, quats, scales, n, width, height, eps2d, near_plane, far_plane,
                                  radius_clip, opt);
    radii[o] = p.rad_i;
    *reinterpret_cast<float2*>(means2d + o * 2) = make_float2(p.m2x, p.m2y);
    depths[o] = p.depth;
    conics[o * 3 + 0] = p.con0;
    conics[o * 3 + 1] = p.con1;
    conics[o * 3 + 2] = p.con2;
    if (comps) comps[o] = p.comp;
}

}  // namespace

#pragma clang fp contract(fast)

namespace {

// ---- backward -----------------------------------------------------------------------------
// Recomputes the forward intermediates per (camera, gaussian) and chains the VJPs of
// SURVEY.md A.1 steps 1-5 (radius / cull are non-differentiable).  One thread per Gaussian loops
// over the cameras itself: the mean's gradient and dL/dSigma are accumulated in registers across
// the cameras in which the Gaussian is visible (radii > 0), the chain to quats / scales runs once
// on the sum, and every output row is written exactly once -- no atomics for any C.
__global__ __launch_bounds__(256) void projection_bwd_kernel(
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ viewmats, const float* __restrict__ Ks, int C, int N, int width,
    int height, float eps2d, ProjOpt opt, const int32_t* __restrict__ radii, const float* __restrict__ conics,
    const float* __restrict__ comps, const float* __restrict__ v_means2d,
    const float* __restrict__ v_depths, const float* __restrict__ v_conics,
    const float* __restrict__ v_comps, float* __restrict__ v_means, float* __restrict__ v_quats,
    float* __restrict__ v_scales) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float gm[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f};
    const ProjBwdPre pre = proj_bwd_setup(means, quats, scales, n);
    float vS[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};  // dL/dSigma (world)

    bool seen = false;
    for (int cam = 0; cam < C; ++cam) {
        const size_t o = (size_t)cam * N + n;
        if (radii[o] <= 0) continue;
        seen = true;
        const ProjBwdCam f = proj_bwd_recompute(pre, viewmats + cam * 16, Ks + cam * 9, width, height, eps2d, opt);
        const bool has_comp = v_comps && comps;
        proj_bwd_camera(f, conics[o * 3 + 0], conics[o * 3 + 1], conics[o * 3 + 2], v_conics[o * 3 + 0],
                        v_conics[o * 3 + 1], v_conics[o * 3 + 2], has_comp, has_comp ? comps[o] : 0.f,
                        has_comp ? v_comps[o] : 0.f, v_means2d[o * 2 + 0], v_means2d[o * 2 + 1], v_depths[o], gm, vS);
    }
    // visible nowhere: exact zeros in every row, whatever the leaves hold (0 * a NaN or infinite M is NaN)
    if (seen) proj_bwd_finish(pre, vS, gq, gs);

    v_means[n * 3 + 0] = gm[0]; v_means[n * 3 + 1] = gm[1]; v_means[n * 3 + 2] = gm[2];
    *reinterpret_cast<float4*>(v_quats + (size_t)n * 4) = make_float4(gq[0], gq[1], gq[2], gq[3]);
    v_scales[n * 3 + 0] = gs[0]; v_scales[n * 3 + 1] = gs[1]; v_scales[n * 3 + 2] = gs[2];
}

}  // namespace

extern "C" int sc_projection_fwd(const float* means, const float* quats, const float* scales,
                                 const float* viewmats, const float* Ks, int C, int N, int width,
                                 int height, float eps2d, float near_plane, float far_plane,
                                 float radius_clip, int32_t* radii, float* means2d, float* depths,
                                 float* conics, float* compensations, sc_stream_t stream) {
    if (C < 0 || N < 0 || width <= 0 || height <= 0) return SC_EINVAL;
    if (C == 0 || N == 0) return SC_OK;
    if (!means || !quats || !scales || !viewmats || !Ks || !radii || !means2d || !depths || !conics)
        return SC_EINVAL;
    if (C > 65535) return SC_EINVAL;
    dim3 grid((N + 255) / 256, C);
    hipLaunchKernelGGL(projection_fwd_kernel, grid, dim3(256), 0, sc_s(stream), means, quats, scales,
                       viewmats, Ks, N, width, height, eps2d, near_plane, far_plane, radius_clip, sc_proj_opt(),
                       radii, means2d, depths, conics, compensations);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_projection_bwd(const float* means, const float* quats, const float* scales,
                                 const float* viewmats, const float* Ks, int C, int N, int width,
                                 int height, float eps2d, const int32_t* radii, const float* conics,
                                 const float* compensations, const float* v_means2d,
                                 const float* v_depths, const float* v_conics,
                                 const float* v_compensations, float* v_means, float* v_quats,
                                 float* v_scales, sc_stream_t stream) {
    if (C < 0 || N < 0 || width <= 0 || height <= 0) return SC_EINVAL;
    if (N == 0) return SC_OK;
    if (!means || !quats || !scales || !viewmats || !Ks || !radii || !conics || !v_means2d ||
        !v_depths || !v_conics || !v_means || !v_quats || !v_scales)
        return SC_EINVAL;
    hipLaunchKernelGGL(projection_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, sc_s(stream),
                       means, quats, scales, viewmats, Ks, C, N, width, height, eps2d, sc_proj_opt(), radii, conics,
                       compensations, v_means2d, v_depths, v_conics, v_compensations, v_means,
                       v_quats, v_scales);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
