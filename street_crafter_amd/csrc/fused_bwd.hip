// The backward of fused_fwd.hip's projection_sh_fwd_kernel: the VJP of
//
//   a1 fully_fused_projection + a2 opacities * compensations + a5 dirs = xyz - camera_center, masks = radii > 0
//   + a6 spherical_harmonics + a7 clamp_min(colors + 0.5, 0), cat(colors, depth)
//
// with respect to the five leaves (means, quats, scales, opacities, sh), in ONE kernel instead of projection_bwd +
// sh_bwd + the torch elementwise / reduction kernels autograd runs between them.  Camera tensors carry no gradient.
//
// One lane per Gaussian loops over the cameras itself, as projection_bwd_kernel does: every partial sum (mean, dL/dSigma,
// opacity, the SH coefficient rows) stays in registers across the cameras, each output row is written exactly once and
// overwritten -- no atomics, so the result is the same from run to run.  A (camera, Gaussian) the forward culled is
// skipped before any of its upstream values is read.  Per Gaussian at K = 4 and one camera: 92 B of leaves + 16 B of
// radii / conics + 40 B of upstream in, 92 B out.
//
// The arithmetic is the separate operators': proj_bwd_* (projection_common.h) and sh_basis_vjp / sh_dir_vjp
// (sh_common.h).  What is recomputed: the compensation (from det0 / det1 of the recomputed covariance), the direction
// and the SH colour that decides the clamp -- the last two by the forward's own device functions, so the decision is the
// forward's bit for bit.
#include "projection_common.h"
#include "sh_common.h"

namespace {

// VEC: rows of sh_coeffs / v_sh are a multiple of 16 B and 16-B aligned: read and written as float4 (sh_bwd_kernel).
template <int DEG, bool VEC>
__global__ __launch_bounds__(256) void projection_sh_bwd_kernel(
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ opacities, const float* __restrict__ coeffs, const float* __restrict__ viewmats,
    const float* __restrict__ Ks, const float* __restrict__ campos, int C, int N, int K, int width, int height,
    float eps2d, ProjOpt opt, int antialiased, const int32_t* __restrict__ radii, const float* __restrict__ conics,
    const float* __restrict__ v_means2d, const float* __restrict__ v_depths, const float* __restrict__ v_conics,
    const float* __restrict__ v_opac_out, const float* __restrict__ v_colors4, float* __restrict__ v_means,
    float* __restrict__ v_quats, float* __restrict__ v_scales, float* __restrict__ v_opacities,
    float* __restrict__ v_sh) {
    constexpr int NB = (DEG + 1) * (DEG + 1);
    constexpr int NV = (NB * 3 + 3) / 4;           // float4 chunks that hold the NB live coefficients
    constexpr int NF = VEC ? NV * 4 : NB * 3;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;

    const ProjBwdPre pre = proj_bwd_setup(means, quats, scales, n);
    const float op = opacities[n];
    const float* crow = coeffs + (size_t)n * K * 3;
    float cf[NF];                                  // this Gaussian's live coefficients, [k][3]
    if (VEC) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 q = reinterpret_cast<const float4*>(crow)[j];
            cf[4 * j] = q.x; cf[4 * j + 1] = q.y; cf[4 * j + 2] = q.z; cf[4 * j + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int f = 0; f < NB * 3; ++f) cf[f] = crow[f];
    }

    float gm[3] = {0.f, 0.f, 0.f}, gop = 0.f;
    float vS[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};  // dL/dSigma (world)
    float gsh[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) gsh[f] = 0.f;
    bool seen = false;

    for (int cam = 0; cam < C; ++cam) {
        const size_t o = (size_t)cam * N + n;
        if (radii[o] <= 0) continue;               // culled here: none of its upstream rows is read
        seen = true;
        const ProjBwdCam f = proj_bwd_recompute(pre, viewmats + cam * 16, Ks + cam * 9, width, height, eps2d, opt);
        const float4 vc4 = *reinterpret_cast<const float4*>(v_colors4 + o * 4);
        const float vdepth = v_depths ? vc4.w + v_depths[o] : vc4.w;

        // a2: opacity (* compensation, recomputed as the forward forms it: sqrt(max(0, det0 / det1)))
        const float vopo = v_opac_out[o];
        float comp = 0.f, vcomp = 0.f;
        if (antialiased) {
            comp = sqrtf(fmaxf(0.f, (f.a * f.cc - f.b * f.b) / f.det1));
            gop += vopo * comp;
            vcomp = vopo * op;
        } else {
            gop += vopo;
        }

        // a7 + a6 + a5: the clamp passes where the forward's colour + 0.5 >= 0 (torch's clamp_min backward)
        const float dx = pre.mx - campos[cam * 3 + 0];
        const float dy = pre.my - campos[cam * 3 + 1];
        const float dz = pre.mz - campos[cam * 3 + 2];
        float Y[NB];
        sh_basis<DEG>(dx, dy, dz, Y);
        float r, g, b;
        sh_dot<DEG>(Y, cf, r, g, b);
        const float vr = (r + 0.5f >= 0.f) ? vc4.x : 0.f;
        const float vg = (g + 0.5f >= 0.f) ? vc4.y : 0.f;
        const float vb = (b + 0.5f >= 0.f) ? vc4.z : 0.f;
        if (v_sh) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                gsh[k * 3 + 0] += Y[k] * vr; gsh[k * 3 + 1] += Y[k] * vg; gsh[k * 3 + 2] += Y[k] * vb;
            }
        }
        if (v_means && DEG >= 1) {
            float w[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) w[k] = vr * cf[k * 3 + 0] + vg * cf[k * 3 + 1] + vb * cf[k * 3 + 2];
            float vdx, vdy, vdz;
            sh_dir_vjp<DEG>(dx, dy, dz, w, vdx, vdy, vdz);
            gm[0] += vdx; gm[1] += vdy; gm[2] += vdz;        // dirs = means - centre
        }

        // a1
        proj_bwd_camera(f, conics[o * 3 + 0], conics[o * 3 + 1], conics[o * 3 + 2], v_conics[o * 3 + 0],
                        v_conics[o * 3 + 1], v_conics[o * 3 + 2], antialiased != 0, comp, vcomp,
                        v_means2d[o * 2 + 0], v_means2d[o * 2 + 1], vdepth, gm, vS);
    }

    float gq[4] = {0.f, 0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f};
    if (seen && (v_quats || v_scales)) proj_bwd_finish(pre, vS, gq, gs);   // visible nowhere: exact zeros in every row
    if (v_means) { v_means[n * 3 + 0] = gm[0]; v_means[n * 3 + 1] = gm[1]; v_means[n * 3 + 2] = gm[2]; }
    if (v_quats) *reinterpret_cast<float4*>(v_quats + (size_t)n * 4) = make_float4(gq[0], gq[1], gq[2], gq[3]);
    if (v_scales) { v_scales[n * 3 + 0] = gs[0]; v_scales[n * 3 + 1] = gs[1]; v_scales[n * 3 + 2] = gs[2]; }
    if (v_opacities) v_opacities[n] = gop;
    if (v_sh) {
        float* vrow = v_sh + (size_t)n * K * 3;
        if (VEC) {
#pragma unroll
            for (int j = 0; j < NV; ++j)
                reinterpret_cast<float4*>(vrow)[j] = make_float4(gsh[4 * j], gsh[4 * j + 1], gsh[4 * j + 2], gsh[4 * j + 3]);
            for (int j = NV; j < (K * 3) / 4; ++j) reinterpret_cast<float4*>(vrow)[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
#pragma unroll
            for (int f = 0; f < NB * 3; ++f) vrow[f] = gsh[f];
            for (int f = NB * 3; f < K * 3; ++f) vrow[f] = 0.f;
        }
    }
}

}  // namespace

extern "C" int sc_projection_sh_bwd(const float* means, const float* quats, const float* scales,
                                    const float* opacities, const float* sh_coeffs, const float* viewmats,
                                    const float* Ks, const float* camera_centers, int C, int N, int K,
                                    int sh_degree, int width, int height, float eps2d, int antialiased,
                                    const int32_t* radii, const float* conics, const float* v_means2d,
                                    const float* v_depths, const float* v_conics, const float* v_opacities_out,
                                    const float* v_colors4, float* v_means, float* v_quats, float* v_scales,
                                    float* v_opacities, float* v_sh, sc_stream_t stream) {
    if (C < 0 || N < 0 || width <= 0 || height <= 0) return SC_EINVAL;
    if (sh_degree < 0 || sh_degree > 4 || K < (sh_degree + 1) * (sh_degree + 1)) return SC_EINVAL;
    if (N == 0) return SC_OK;
    if (!means || !quats || !scales || !opacities || !sh_coeffs || !viewmats || !Ks || !camera_centers || !radii ||
        !conics || !v_means2d || !v_conics || !v_opacities_out || !v_colors4)
        return SC_EINVAL;
    if (!v_means && !v_quats && !v_scales && !v_opacities && !v_sh) return SC_OK;      // nothing asked for
    if (((uintptr_t)quats & 15) || ((uintptr_t)v_colors4 & 15) || ((uintptr_t)v_quats & 15)) return SC_EINVAL;
    const dim3 grid((N + 255) / 256), block(256);
    // float4 rows: K * 3 floats a multiple of 4 and both arrays 16-B aligned (torch allocations are)
    const bool vec = (K * 3) % 4 == 0 && ((uintptr_t)sh_coeffs % 16) == 0 && ((uintptr_t)v_sh % 16) == 0;
#define SC_LAUNCH_FUSED_BWD(D)                                                                                        \
    if (vec) hipLaunchKernelGGL((projection_sh_bwd_kernel<D, true>), grid, block, 0, sc_s(stream), means, quats,       \
                                scales, opacities, sh_coeffs, viewmats, Ks, camera_centers, C, N, K, width, height,   \
                                eps2d, sc_proj_opt(), antialiased, radii, conics, v_means2d, v_depths, v_conics,      \
                                v_opacities_out, v_colors4, v_means, v_quats, v_scales, v_opacities, v_sh);           \
    else hipLaunchKernelGGL((projection_sh_bwd_kernel<D, false>), grid, block, 0, sc_s(stream), means, quats, scales, \
                            opacities, sh_coeffs, viewmats, Ks, camera_centers, C, N, K, width, height, eps2d,        \
                            sc_proj_opt(), antialiased, radii, conics, v_means2d, v_depths, v_conics,                 \
                            v_opacities_out, v_colors4, v_means, v_quats, v_scales, v_opacities, v_sh)
    switch (sh_degree) {
        case 0: SC_LAUNCH_FUSED_BWD(0); break;
        case 1: SC_LAUNCH_FUSED_BWD(1); break;
        case 2: SC_LAUNCH_FUSED_BWD(2); break;
        case 3: SC_LAUNCH_FUSED_BWD(3); break;
        default: SC_LAUNCH_FUSED_BWD(4); break;
    }
#undef SC_LAUNCH_FUSED_BWD
    SC_LAUNCH_CHECK();
    return SC_OK;
}
