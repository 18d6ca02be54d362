// The per-point projection of the LiDAR condition render, shared by point_project_kernel (point_raster.hip: float32
// points handed in by the caller) and point_assemble_project_kernel (point_assemble.hip: points assembled from the
// resident float64 sweeps).  Both compile exactly this body, which is why the fused route's rows are bit-equal to
// sc_point_project run on the same float32 point.
#pragma once
#include "sc_common.h"

#pragma clang fp contract(off)

// radius modes (include/street_crafter_amd.h sc_point_project)
constexpr int SC_RMODE_CONST = 0, SC_RMODE_NDC = 1, SC_RMODE_KNN = 2, SC_RMODE_ARRAY = 3;

// The camera of one launch, by value in the kernel arguments.
struct ScPointCam {
    double fx, fy, cx, cy, focal_r, near_plane, far_plane, scale, half_min_hw;
    int radius_mode;
    float knn_scale_down;
};

// Row i of radii / means2d / depths / records [N][8] = (u, v, r^2, z | r, g, b, alpha) from the float32 point (px, py,
// pz), already widened to fp64.  The camera transform, u, v and r are evaluated in fp64 and rounded once to fp32.  LiDAR
// points sit tens of metres from the world origin: in fp32 the transform alone moves a disc centre by ~1e-4 px, the order
// of the band around a disc's edge inside which the contract's f64 coverage test and any fp32 test may disagree.  fp64
// leaves only the final rounding of u / v (half an ulp: <= 6e-5 px below 2048).  ~40 fp64 operations per point: not
// measurable next to the binning.  The knn radius rule stays in fp32, as the contract evaluates it
// (lidar_condition.knn_point_radii).
// listed == false (a point the visibility filter of the fused route drops): the whole row is zero, so that the tile
// binning sees a culled point (radius 0, means2d 0, depth 0) and nothing reads its record.
__device__ __forceinline__ void sc_point_project_row(
    int i, double px, double py, double pz, float c0, float c1, float c2, float a, const float* __restrict__ radius_in,
    const double* __restrict__ viewmat, const ScPointCam& cam, bool listed, int32_t* __restrict__ radii,
    float* __restrict__ means2d, float* __restrict__ depths, float4* __restrict__ records) {
    if (!listed) {
        radii[i] = 0;
        means2d[(int64_t)i * 2 + 0] = 0.f;
        means2d[(int64_t)i * 2 + 1] = 0.f;
        depths[i] = 0.f;
        records[(int64_t)i * 2 + 0] = make_float4(0.f, 0.f, 0.f, 0.f);
        records[(int64_t)i * 2 + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    // world -> camera: rows 0..2 of the [4,4] matrix (uniform loads: every lane reads the same 12 words)
    const double x = viewmat[0] * px + viewmat[1] * py + viewmat[2] * pz + viewmat[3];
    const double y = viewmat[4] * px + viewmat[5] * py + viewmat[6] * pz + viewmat[7];
    const double z = viewmat[8] * px + viewmat[9] * py + viewmat[10] * pz + viewmat[11];
    const double u = cam.fx * x / z + cam.cx;
    const double v = cam.fy * y / z + cam.cy;
    double world_r;
    if (cam.radius_mode == SC_RMODE_NDC) {
        world_r = cam.scale * z / cam.focal_r * cam.half_min_hw;         // render_utils.py:116-122
    } else if (cam.radius_mode == SC_RMODE_KNN) {                  // :123-127, radius_in = distCUDA2 of all points
        world_r = (double)fminf(sqrtf(fmaxf(radius_in[i], 1e-7f)) * cam.knn_scale_down, (float)cam.scale);
    } else if (cam.radius_mode == SC_RMODE_ARRAY) {                // the drop-in's per-point radius x scale_modifier
        world_r = (double)radius_in[i] * cam.scale;
    } else {
        world_r = cam.scale;
    }
    const double r = world_r * cam.focal_r / z;
    const float uf = (float)u, vf = (float)v, rf = (float)r;
    // culled: outside the open depth window (z > 0 as well, so that the depth bits of the sort key order like
    // floats), a non-finite centre or radius, or an alpha outside (0, 1] (the callers refuse those before launching)
    const bool keep = z > cam.near_plane && z < cam.far_plane && z > 0.0 && isfinite(uf) && isfinite(vf) &&
                      isfinite(rf) && rf >= 0.f && a > 0.f && a <= 1.f;
    // ceil(r), held below 2^30 so that it fits an int; tile_rect clamps the rectangle to the image anyway.  At least 1
    // for a kept point: tile_rect reads radius 0 as "culled", and a disc of r = 0 still covers the pixel whose centre it
    // sits on (0 <= 0); listed with radius 1, its r^2 = 0 decides per pixel.
    const int R = keep ? max((int)ceil(fmin(r, 1073741824.0)), 1) : 0;
    radii[i] = R;
    means2d[(int64_t)i * 2 + 0] = keep ? uf : 0.f;
    means2d[(int64_t)i * 2 + 1] = keep ? vf : 0.f;
    depths[i] = keep ? (float)z : 0.f;
    records[(int64_t)i * 2 + 0] = make_float4(uf, vf, (float)(r * r), (float)z);
    records[(int64_t)i * 2 + 1] = make_float4(c0, c1, c2, a);
}
