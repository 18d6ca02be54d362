// The per-(camera, Gaussian) projection arithmetic of SURVEY.md A.1, shared by projection_fwd_kernel
// (projection.hip) and the fused projection + SH kernel (fused_fwd.hip).  Compiled without FMA
// contraction, in oracle/gsplat_oracle.py's op order: bit-identical to the oracle wherever it is used.
// Below it the backward's per-Gaussian and per-camera VJP bodies, shared by projection.hip and fused_bwd.hip.
#pragma once
#include "sc_common.h"

#pragma clang fp contract(off)

struct ProjOpt { int clamp; float radius_floor; };
extern int g_sc_proj_clamp, g_sc_radius_floor;       // sc_set_option "proj_clamp" / "radius_floor" (capi.hip)

namespace {

__device__ __forceinline__ float dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

struct Cam {
    float W00, W01, W02, tx, W10, W11, W12, ty, W20, W21, W22, tz;
    float fx, fy, cx, cy;
};

__device__ __forceinline__ Cam load_cam(const float* __restrict__ V, const float* __restrict__ K) {
    Cam c;
    c.W00 = V[0]; c.W01 = V[1]; c.W02 = V[2];  c.tx = V[3];
    c.W10 = V[4]; c.W11 = V[5]; c.W12 = V[6];  c.ty = V[7];
    c.W20 = V[8]; c.W21 = V[9]; c.W22 = V[10]; c.tz = V[11];
    c.fx = K[0]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
    return c;
}

// The two constants of SURVEY A.1 that differ between upstream gsplat versions (the reference installs an unpinned fork,
// README.md:35), selectable at run time: sc_set_option("proj_clamp") 0 = x/z, y/z clamped to +-1.3 tan(fov/2) (v1.0-1.3,
// default), 1 = to [-(cx/fx + 0.3 tan), (W - cx)/fx + 0.3 tan] (v1.4+); sc_set_option("radius_floor") 0 = 0.01 (v1.x,
// default), 1 = 0.1 (the original Inria rasterizer).  oracle/gsplat_oracle.py takes the same two arguments.
static inline ProjOpt sc_proj_opt() { return ProjOpt{g_sc_proj_clamp, g_sc_radius_floor ? 0.1f : 0.01f}; }

struct ProjLim { float xp, xn, yp, yn; };       // tan-space limits: x/z in [-xn, xp], y/z in [-yn, yp]
__device__ __forceinline__ ProjLim proj_limits(const ProjOpt& opt, float fx, float fy, float cx, float cy, int width, int height) {
    const float tanx = 0.5f * (float)width / fx;
    const float tany = 0.5f * (float)height / fy;
    ProjLim l;
    if (opt.clamp == 0) {
        l.xp = l.xn = 1.3f * tanx;
        l.yp = l.yn = 1.3f * tany;
    } else {
        l.xp = ((float)width - cx) / fx + 0.3f * tanx;
        l.xn = cx / fx + 0.3f * tanx;
        l.yp = ((float)height - cy) / fy + 0.3f * tany;
        l.yn = cy / fy + 0.3f * tany;
    }
    return l;
}

struct ProjOut {
    int rad_i;
    float m2x, m2y, con0, con1, con2, comp, depth;
};

__device__ __forceinline__ ProjOut project_one(const Cam& c, const float* __restrict__ means,
                                               const float* __restrict__ quats,
                                               const float* __restrict__ scales, int n, int width, int height,
                                               float eps2d, float near_plane, float far_plane,
                                               float radius_clip, const ProjOpt& opt) {
    const float mx = means[n * 3 + 0], my = means[n * 3 + 1], mz = means[n * 3 + 2];
    const float x = dot3(c.W00, mx, c.W01, my, c.W02, mz) + c.tx;
    const float y = dot3(c.W10, mx, c.W11, my, c.W12, mz) + c.ty;
    const float z = dot3(c.W20, mx, c.W21, my, c.W22, mz) + c.tz;

    bool valid = !((z < near_plane) || (z > far_plane));
    int rad_i = 0;
    float m2x = 0.f, m2y = 0.f, con0 = 0.f, con1 = 0.f, con2 = 0.f, comp = 0.f, depth = 0.f;
    if (valid) {
        const float4 q = *reinterpret_cast<const float4*>(quats + (size_t)n * 4);
        float qw = q.x, qx = q.y, qy = q.z, qz = q.w;
        const float n2 = ((qx * qx + qy * qy) + qz * qz) + qw * qw;
        const float inv = 1.0f / sqrtf(n2);
        qw *= inv; qx *= inv; qy *= inv; qz *= inv;
        const float x2 = qx * qx, y2 = qy * qy, z2 = qz * qz;
        const float xy = qx * qy, xz = qx * qz, yz = qy * qz;
        const float wx = qw * qx, wy = qw * qy, wz = qw * qz;
        const float R00 = 1.0f - 2.0f * (y2 + z2), R01 = 2.0f * (xy - wz), R02 = 2.0f * (xz + wy);
        const float R10 = 2.0f * (xy + wz), R11 = 1.0f - 2.0f * (x2 + z2), R12 = 2.0f * (yz - wx);
        const float R20 = 2.0f * (xz - wy), R21 = 2.0f * (yz + wx), R22 = 1.0f - 2.0f * (x2 + y2);
        const float s0 = scales[n * 3 + 0], s1 = scales[n * 3 + 1], s2 = scales[n * 3 + 2];
        const float M00 = R00 * s0, M01 = R01 * s1, M02 = R02 * s2;
        const float M10 = R10 * s0, M11 = R11 * s1, M12 = R12 * s2;
        const float M20 = R20 * s0, M21 = R21 * s1, M22 = R22 * s2;
        const float S00 = dot3(M00, M00, M01, M01, M02, M02);
        const float S01 = dot3(M00, M10, M01, M11, M02, M12);
        const float S02 = dot3(M00, M20, M01, M21, M02, M22);
        const float S11 = dot3(M10, M10, M11, M11, M12, M12);
        const float S12 = dot3(M10, M20, M11, M21, M12, M22);
        const float S22 = dot3(M20, M20, M21, M21, M22, M22);
        // T = W * Sigma
        const float T00 = dot3(c.W00, S00, c.W01, S01, c.W02, S02);
        const float T01 = dot3(c.W00, S01, c.W01, S11, c.W02, S12);
        const float T02 = dot3(c.W00, S02, c.W01, S12, c.W02, S22);
        const float T10 = dot3(c.W10, S00, c.W11, S01, c.W12, S02);
        const float T11 = dot3(c.W10, S01, c.W11, S11, c.W12, S12);
        const float T12 = dot3(c.W10, S02, c.W11, S12, c.W12, S22);
        const float T20 = dot3(c.W20, S00, c.W21, S01, c.W22, S02);
        const float T21 = dot3(c.W20, S01, c.W21, S11, c.W22, S12);
        const float T22 = dot3(c.W20, S02, c.W21, S12, c.W22, S22);
        // Sigma_c = T * W^T
        const float c00 = dot3(T00, c.W00, T01, c.W01, T02, c.W02);
        const float c01 = dot3(T00, c.W10, T01, c.W11, T02, c.W12);
        const float c02 = dot3(T00, c.W20, T01, c.W21, T02, c.W22);
        const float c11 = dot3(T10, c.W10, T11, c.W11, T12, c.W12);
        const float c12 = dot3(T10, c.W20, T11, c.W21, T12, c.W22);
        const float c22 = dot3(T20, c.W20, T21, c.W21, T22, c.W22);

        const ProjLim lim = proj_limits(opt, c.fx, c.fy, c.cx, c.cy, width, height);
        const float rz = 1.0f / z;
        const float rz2 = rz * rz;
        const float tx = z * fminf(lim.xp, fmaxf(-lim.xn, x * rz));
        const float ty = z * fminf(lim.yp, fmaxf(-lim.yn, y * rz));
        const float ja = c.fx * rz;
        const float jb = ((-c.fx) * tx) * rz2;
        const float jc = c.fy * rz;
        const float jd = ((-c.fy) * ty) * rz2;
        const float u0 = ja * c00 + jb * c02;
        const float u1 = ja * c01 + jb * c12;
        const float u2 = ja * c02 + jb * c22;
        const float v1 = jc * c11 + jd * c12;
        const float v2 = jc * c12 + jd * c22;
        const float a = u0 * ja + u2 * jb;
        const float b = u1 * jc + u2 * jd;
        const float cc = v1 * jc + v2 * jd;
        m2x = (c.fx * x) * rz + c.cx;
        m2y = (c.fy * y) * rz + c.cy;

        const float det0 = a * cc - b * b;
        const float a1 = a + eps2d;
        const float c1 = cc + eps2d;
        const float det1 = a1 * c1 - b * b;
        comp = sqrtf(fmaxf(0.0f, det0 / det1));
        valid = det1 > 0.0f;  // false for NaN too
        con0 = c1 / det1;
        con1 = (-b) / det1;
        con2 = a1 / det1;
        const float bb = 0.5f * (a1 + c1);
        const float lam = bb + sqrtf(fmaxf(opt.radius_floor, bb * bb - det1));
        const float radius = ceilf(3.0f * sqrtf(lam));
        valid = valid && (radius > radius_clip);  // false for NaN
        const float Wf = (float)width, Hf = (float)height;
        valid = valid && !((m2x + radius <= 0.0f) || (m2x - radius >= Wf) ||
                           (m2y + radius <= 0.0f) || (m2y - radius >= Hf));
        rad_i = (int)fminf(radius, 2147483520.0f);
        depth = z;
    }
    if (!valid) {
        rad_i = 0; m2x = m2y = con0 = con1 = con2 = comp = depth = 0.f;
    }
    ProjOut r;
    r.rad_i = rad_i; r.m2x = m2x; r.m2y = m2y; r.con0 = con0; r.con1 = con1; r.con2 = con2;
    r.comp = comp; r.depth = depth;
    return r;
}

}  // namespace

#pragma clang fp contract(fast)

// ---- backward ---------------------------------------------------------------------------------
// The VJP of SURVEY.md A.1 steps 1-5 in three pieces, shared by projection_bwd_kernel (projection.hip) and the fused
// projection + SH backward (fused_bwd.hip): what depends on the Gaussian alone (proj_bwd_setup), the recomputed forward
// intermediates and the chain of one camera into the mean's gradient and dL/dSigma (proj_bwd_recompute / proj_bwd_camera),
// and the chain of the summed dL/dSigma to quats / scales (proj_bwd_finish).  FMA contraction allowed: these are gradients.
namespace {

struct ProjBwdPre {
    float mx, my, mz;
    float qw, qx, qy, qz, inv;      // normalised quaternion, 1 / |q|
    float sc[3], R[3][3], M[3][3], S[3][3];
};

__device__ __forceinline__ ProjBwdPre proj_bwd_setup(const float* __restrict__ means, const float* __restrict__ quats,
                                                     const float* __restrict__ scales, int n) {
    ProjBwdPre p;
    p.mx = means[n * 3 + 0]; p.my = means[n * 3 + 1]; p.mz = means[n * 3 + 2];
    const float4 q4 = *reinterpret_cast<const float4*>(quats + (size_t)n * 4);
    const float s0 = scales[n * 3 + 0], s1 = scales[n * 3 + 1], s2 = scales[n * 3 + 2];
    // normalised quaternion + rotation
    const float qn2 = q4.y * q4.y + q4.z * q4.z + q4.w * q4.w + q4.x * q4.x;
    const float inv = 1.0f / sqrtf(qn2);
    const float qw = q4.x * inv, qx = q4.y * inv, qy = q4.z * inv, qz = q4.w * inv;
    p.qw = qw; p.qx = qx; p.qy = qy; p.qz = qz; p.inv = inv;
    p.R[0][0] = 1.f - 2.f * (qy * qy + qz * qz); p.R[0][1] = 2.f * (qx * qy - qw * qz); p.R[0][2] = 2.f * (qx * qz + qw * qy);
    p.R[1][0] = 2.f * (qx * qy + qw * qz); p.R[1][1] = 1.f - 2.f * (qx * qx + qz * qz); p.R[1][2] = 2.f * (qy * qz - qw * qx);
    p.R[2][0] = 2.f * (qx * qz - qw * qy); p.R[2][1] = 2.f * (qy * qz + qw * qx); p.R[2][2] = 1.f - 2.f * (qx * qx + qy * qy);
    p.sc[0] = s0; p.sc[1] = s1; p.sc[2] = s2;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) p.M[i][j] = p.R[i][j] * p.sc[j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) p.S[i][j] = p.M[i][0] * p.M[j][0] + p.M[i][1] * p.M[j][1] + p.M[i][2] * p.M[j][2];
    return p;
}

// the forward intermediates of one (camera, Gaussian) the VJP needs
struct ProjBwdCam {
    float Wm[3][3], fx, fy, x, y, z, rz, rz2, tx, ty;
    bool clx, cly;
    float ja, jb, jc, jd, u0, u1, u2, w0, w1, w2;      // J = [[ja,0,jb],[0,jc,jd]]; (J Sc) rows (u0,u1,u2), (w0,w1,w2)
    float a, b, cc, a1, c1, det1;                      // cov2d = [[a,b],[b,cc]], blurred [[a1,b],[b,c1]]
};

__device__ __forceinline__ ProjBwdCam proj_bwd_recompute(const ProjBwdPre& p, const float* __restrict__ V,
                                                         const float* __restrict__ K, int width, int height,
                                                         float eps2d, const ProjOpt& opt) {
    ProjBwdCam f;
    f.Wm[0][0] = V[0]; f.Wm[0][1] = V[1]; f.Wm[0][2] = V[2];
    f.Wm[1][0] = V[4]; f.Wm[1][1] = V[5]; f.Wm[1][2] = V[6];
    f.Wm[2][0] = V[8]; f.Wm[2][1] = V[9]; f.Wm[2][2] = V[10];
    const float fx = K[0], fy = K[4];
    f.fx = fx; f.fy = fy;
    const float x = f.Wm[0][0] * p.mx + f.Wm[0][1] * p.my + f.Wm[0][2] * p.mz + V[3];
    const float y = f.Wm[1][0] * p.mx + f.Wm[1][1] * p.my + f.Wm[1][2] * p.mz + V[7];
    const float z = f.Wm[2][0] * p.mx + f.Wm[2][1] * p.my + f.Wm[2][2] * p.mz + V[11];
    f.x = x; f.y = y; f.z = z;
    // Sigma_c = W S W^T
    float T[3][3], Sc[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[i][j] = f.Wm[i][0] * p.S[0][j] + f.Wm[i][1] * p.S[1][j] + f.Wm[i][2] * p.S[2][j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Sc[i][j] = T[i][0] * f.Wm[j][0] + T[i][1] * f.Wm[j][1] + T[i][2] * f.Wm[j][2];

    const ProjLim lim = proj_limits(opt, fx, fy, K[2], K[5], width, height);
    const float rz = 1.f / z, rz2 = rz * rz;
    const float xr = x * rz, yr = y * rz;
    f.rz = rz; f.rz2 = rz2;
    f.clx = (xr < -lim.xn) || (xr > lim.xp);
    f.cly = (yr < -lim.yn) || (yr > lim.yp);
    const float tx = z * fminf(lim.xp, fmaxf(-lim.xn, xr));
    const float ty = z * fminf(lim.yp, fmaxf(-lim.yn, yr));
    f.tx = tx; f.ty = ty;
    const float ja = fx * rz, jb = -fx * tx * rz2, jc = fy * rz, jd = -fy * ty * rz2;
    f.ja = ja; f.jb = jb; f.jc = jc; f.jd = jd;
    // cov2d = J Sc J^T
    f.u0 = ja * Sc[0][0] + jb * Sc[2][0]; f.u1 = ja * Sc[0][1] + jb * Sc[2][1]; f.u2 = ja * Sc[0][2] + jb * Sc[2][2];
    f.w0 = jc * Sc[1][0] + jd * Sc[2][0]; f.w1 = jc * Sc[1][1] + jd * Sc[2][1]; f.w2 = jc * Sc[1][2] + jd * Sc[2][2];
    f.a = f.u0 * ja + f.u2 * jb; f.b = f.u1 * jc + f.u2 * jd; f.cc = f.w1 * jc + f.w2 * jd;
    f.a1 = f.a + eps2d; f.c1 = f.cc + eps2d;
    f.det1 = f.a1 * f.c1 - f.b * f.b;
    return f;
}

// One camera's (v_means2d, v_depth, v_conics, v_compensation) chained into gm += dL/dmean and vS += dL/dSigma (world).
// conic = the forward's conic of this (camera, Gaussian); has_comp: the compensation path is live (comp, vcomp given).
// Also hands out the two camera-space gradients everything else is chained from: v_pc = dL/d(W m + t) and the symmetric
// vSc_out = dL/dSigma_c (what the camera's own gradient needs, projection_cam.hip).
__device__ __forceinline__ void proj_bwd_camera_core(const ProjBwdCam& f, float i00, float i01, float i11, float g0, float g1h,
                                                     float g2, bool has_comp, float comp, float vcomp, float vm2x, float vm2y,
                                                     float vdepth, float gm[3], float vS[3][3], float v_pc[3],
                                                     float vSc_out[3][3]) {
    const float fx = f.fx, fy = f.fy, x = f.x, y = f.y, rz = f.rz, rz2 = f.rz2, tx = f.tx, ty = f.ty;
    const float ja = f.ja, jb = f.jb, jc = f.jc, jd = f.jd;
    const float a = f.a, b = f.b, cc = f.cc, a1 = f.a1, c1 = f.c1, det1 = f.det1;
    // ---- VJP: conics -> blurred cov2d.  conic = inv([[a1,b],[b,c1]]);  v_cov = -X^-1 V X^-1
    const float g1 = g1h * 0.5f;
    // P = Xinv * G
    const float p00 = i00 * g0 + i01 * g1, p01 = i00 * g1 + i01 * g2;
    const float p10 = i01 * g0 + i11 * g1, p11 = i01 * g1 + i11 * g2;
    float va = -(p00 * i00 + p01 * i01);
    float vb = -((p00 * i01 + p01 * i11) + (p10 * i00 + p11 * i01));  // grad wrt the single b
    float vc = -(p10 * i01 + p11 * i11);
    // ---- VJP: compensation = sqrt(max(0, det0/det1))
    if (has_comp) {
        if (comp > 0.f) {
            const float inv_det1 = 1.f / det1;
            const float one_m = 1.f - comp * comp;
            const float k = 0.5f * vcomp / comp * inv_det1;  // d comp / d ratio * (1/det1)
            // d ratio/da = (c - ratio*c1)/det1 ; d ratio/dc = (a - ratio*a1)/det1 ; d ratio/db = -2b(1-ratio)/det1
            const float ratio = comp * comp;
            va += k * (cc - ratio * c1);
            vc += k * (a - ratio * a1);
            vb += k * (-2.f * b * one_m);
        }
    }
    // ---- VJP: cov2d = J Sc J^T  ->  v_Sc = J^T Vc J ;  v_J = Vc J Sc^T + Vc^T J Sc
    const float h = 0.5f * vb;  // symmetric split of the b gradient
    // Vc = [[va,h],[h,vc]];  J rows: r0=(ja,0,jb) r1=(0,jc,jd)
    float vSc[3][3];
    {
        const float J0[3] = {ja, 0.f, jb}, J1[3] = {0.f, jc, jd};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                vSc[i][j] = J0[i] * (va * J0[j] + h * J1[j]) + J1[i] * (h * J0[j] + vc * J1[j]);
    }
    // v_J = 2 * Vc * J * Sc  (Sc symmetric)
    const float vJ00 = 2.f * (va * f.u0 + h * f.w0);
    const float vJ02 = 2.f * (va * f.u2 + h * f.w2);
    const float vJ11 = 2.f * (h * f.u1 + vc * f.w1);
    const float vJ12 = 2.f * (h * f.u2 + vc * f.w2);

    // ---- VJP: means2d & depth & J -> camera-space mean
    float vx = fx * rz * vm2x;
    float vy = fy * rz * vm2y;
    float vz = -(fx * x * vm2x + fy * y * vm2y) * rz2 + vdepth;
    // ja = fx/z ; jc = fy/z
    vz += -fx * rz2 * vJ00 - fy * rz2 * vJ11;
    // jb = -fx*tx/z^2 with tx = x (unclamped) or z*lim*sign (clamped)
    const float rz3 = rz2 * rz;
    if (!f.clx) {
        vx += -fx * rz2 * vJ02;
        vz += 2.f * fx * tx * rz3 * vJ02;
    } else {
        // tx = z*k  ->  jb = -fx*k/z  ->  d/dz = fx*k/z^2 = fx*tx/z^3
        vz += fx * tx * rz3 * vJ02;
    }
    if (!f.cly) {
        vy += -fy * rz2 * vJ12;
        vz += 2.f * fy * ty * rz3 * vJ12;
    } else {
        vz += fy * ty * rz3 * vJ12;
    }
    v_pc[0] = vx; v_pc[1] = vy; v_pc[2] = vz;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) vSc_out[i][j] = vSc[i][j];
    // camera -> world mean
    gm[0] += f.Wm[0][0] * vx + f.Wm[1][0] * vy + f.Wm[2][0] * vz;
    gm[1] += f.Wm[0][1] * vx + f.Wm[1][1] * vy + f.Wm[2][1] * vz;
    gm[2] += f.Wm[0][2] * vx + f.Wm[1][2] * vy + f.Wm[2][2] * vz;
    // Sc = W S W^T -> v_S += W^T vSc W
    float Q[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Q[i][j] = vSc[i][0] * f.Wm[0][j] + vSc[i][1] * f.Wm[1][j] + vSc[i][2] * f.Wm[2][j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) vS[i][j] += f.Wm[0][i] * Q[0][j] + f.Wm[1][i] * Q[1][j] + f.Wm[2][i] * Q[2][j];
}

__device__ __forceinline__ void proj_bwd_camera(const ProjBwdCam& f, float i00, float i01, float i11, float g0, float g1h,
                                                float g2, bool has_comp, float comp, float vcomp, float vm2x, float vm2y,
                                                float vdepth, float gm[3], float vS[3][3]) {
    float v_pc[3], vSc[3][3];
    proj_bwd_camera_core(f, i00, i01, i11, g0, g1h, g2, has_comp, comp, vcomp, vm2x, vm2y, vdepth, gm, vS, v_pc, vSc);
}

// ---- Sigma = M M^T -> v_M = (vS + vS^T) M ;  M = R diag(s);  rotation -> quaternion through its normalisation
__device__ __forceinline__ void proj_bwd_finish(const ProjBwdPre& p, const float vS[3][3], float gq[4], float gs[3]) {
    const float qw = p.qw, qx = p.qx, qy = p.qy, qz = p.qz, inv = p.inv;
    float vM[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            vM[i][j] = (vS[i][0] + vS[0][i]) * p.M[0][j] + (vS[i][1] + vS[1][i]) * p.M[1][j] + (vS[i][2] + vS[2][i]) * p.M[2][j];
    float vR[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gs[j] = p.R[0][j] * vM[0][j] + p.R[1][j] * vM[1][j] + p.R[2][j] * vM[2][j];
#pragma unroll
        for (int i = 0; i < 3; ++i) vR[i][j] = vM[i][j] * p.sc[j];
    }
    // rotation -> normalised quaternion (w,x,y,z)
    const float vqw = 2.f * (qx * (vR[2][1] - vR[1][2]) + qy * (vR[0][2] - vR[2][0]) + qz * (vR[1][0] - vR[0][1]));
    const float vqx = 2.f * (-2.f * qx * (vR[1][1] + vR[2][2]) + qy * (vR[1][0] + vR[0][1]) + qz * (vR[2][0] + vR[0][2]) + qw * (vR[2][1] - vR[1][2]));
    const float vqy = 2.f * (qx * (vR[1][0] + vR[0][1]) - 2.f * qy * (vR[0][0] + vR[2][2]) + qz * (vR[2][1] + vR[1][2]) + qw * (vR[0][2] - vR[2][0]));
    const float vqz = 2.f * (qx * (vR[2][0] + vR[0][2]) + qy * (vR[2][1] + vR[1][2]) - 2.f * qz * (vR[0][0] + vR[1][1]) + qw * (vR[1][0] - vR[0][1]));
    // through normalisation: v_q = (v_qn - (v_qn . qn) qn) / |q|
    const float dotp = vqw * qw + vqx * qx + vqy * qy + vqz * qz;
    gq[0] = (vqw - dotp * qw) * inv;
    gq[1] = (vqx - dotp * qx) * inv;
    gq[2] = (vqy - dotp * qy) * inv;
    gq[3] = (vqz - dotp * qz) * inv;
}

}  // namespace
