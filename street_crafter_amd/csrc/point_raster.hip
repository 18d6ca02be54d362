// LiDAR condition render: hard-disc point splatting for gfx950.
// Replaces diff_point_rasterization.PointRasterizer (forward) as called by
// data_processor/utils/render_utils.py:129-176.  The contract is street_crafter_amd/lidar_condition.py
// render_points: pinhole projection, open depth window, a hard disc of pixel radius r per point, front-to-back
// blending with a constant alpha per point and at most max_hit covering points per pixel.
//
// Data flow (street_crafter_amd/point_render.py):
//   point_project_kernel -> isect count / emit / radix sort (isect.hip, radix_sort.hip) -> sc_isect_offsets
//   -> point_raster_fwd_kernel
// The tile binning is the Gaussian path's, unchanged: point_project_kernel writes means2d / depths / radii in the
// layout isect_count / isect_emit read, with radii = max(ceil(r), 1).
//
// Why tile_rect (isect.hip) from means2d +- radii lists every tile that holds a covered pixel centre.  Let R =
// max(ceil(r), 1) >= r, m = the disc centre, x an integer pixel column it covers: |x + 0.5 - m| <= r <= R.
//   lower: x + 0.5 >= m - R.  x is an integer, so no multiple of 16 lies in (x, x + 0.5], hence
//          floor(x / 16) = floor((x + 0.5) / 16) >= floor((m - R) / 16) = the rectangle's first tile column.
//   upper: x / 16 < (x + 0.5) / 16 <= (m + R) / 16 <= ceil((m + R) / 16), and floor(x / 16) is an integer below
//          that bound, so it is < the rectangle's (exclusive) last tile column.
// Rows likewise.  tile_rect evaluates (m -+ R) / 16 as m / 16 -+ R / 16 in fp32 (both divisions exact, one rounding);
// the half-pixel slack above is far wider than that rounding for any on-screen coordinate.
#include "point_project.h"

#pragma clang fp contract(off)

namespace {

constexpr int PROJ_BLK = 256;

// One thread per point.  records[N][8] = (u, v, r^2, z | r, g, b, alpha): the 32 B the blend kernel stages.  The row
// itself is sc_point_project_row (point_project.h), shared with the fused assemble + project kernel.
__global__ __launch_bounds__(PROJ_BLK) void point_project_kernel(
    const float* __restrict__ points, const float* __restrict__ colors, const float* __restrict__ opacities,
    float occ, const float* __restrict__ radius_in, int N, const double* __restrict__ viewmat, ScPointCam cam,
    int32_t* __restrict__ radii, float* __restrict__ means2d, float* __restrict__ depths,
    float4* __restrict__ records) {
    const int i = blockIdx.x * PROJ_BLK + threadIdx.x;
    if (i >= N) return;
    const double px = points[(int64_t)i * 3 + 0], py = points[(int64_t)i * 3 + 1], pz = points[(int64_t)i * 3 + 2];
    const float a = opacities ? opacities[i] : occ;
    const float* c = colors + (int64_t)i * 3;
    sc_point_project_row(i, px, py, pz, c[0], c[1], c[2], a, radius_in, viewmat, cam, true, radii, means2d, depths,
                         records);
}

// One 64-lane wave per 16 x 16 tile (PPL = 4: 4 consecutive pixels of one row per lane, 16 rows x 4 lanes) or per
// 16 x 4 strip of it (PPL = 1: one pixel per lane, four waves per tile, sc_set_option "point_raster_waves").
// The strips exist for the launch's tail: aggregated LiDAR piles tens of thousands of records onto the near-field
// tiles, whose pixels are never all finished early (uncovered pixels walk the whole list), so the makespan is one
// wave's serial walk of the longest list.  Four waves share that walk; each gathers the whole list (L2 hits) and
// culls it against its own, 4x smaller rectangle.  DESIGN.md section 4 has the measurement.
// The tile's depth-sorted list is walked in batches of 64: every lane gathers one 32-B record, the records whose
// disc misses the tile's pixel rectangle are dropped, the rest are compacted into LDS and blended in list order.
// The next batch's records are in flight while the current one blends.  No atomics: deterministic.
constexpr int RB = 64;          // records per batch (one per lane)

template <int PPL>
__global__ __launch_bounds__(64) void point_raster_fwd_kernel(
    const float4* __restrict__ records, int N, int width, int height, int tile_width, int tile_height,
    const int32_t* __restrict__ isect_offsets, const int32_t* __restrict__ flatten_ids, int n_isects, int max_hit,
    const float* __restrict__ background, float* __restrict__ out_rgb, int64_t pix_stride, int64_t ch_stride,
    float* __restrict__ out_alpha, int64_t alpha_stride, float* __restrict__ out_depth) {
    __shared__ float4 geo_s[RB];      // u, v, r^2, z
    __shared__ float4 col_s[RB];      // r, g, b, alpha
    const int total_tiles = tile_width * tile_height;
    constexpr int ROWS = PPL == 4 ? 16 : 4;     // rows per wave
    constexpr int LPR = 16 / PPL;               // lanes per row
    const int tflat = blockIdx.x / (16 / ROWS), sub = blockIdx.x % (16 / ROWS);
    const int tyi = tflat / tile_width, txi = tflat - tyi * tile_width;
    const int lane = threadIdx.x;
    const int px0 = txi * 16 + PPL * (lane % LPR), py_i = tyi * 16 + sub * ROWS + lane / LPR;
    const float pyf = (float)py_i + 0.5f;

    // per pixel: transmittance, hits, colour and depth sums.  A finished pixel (outside the image, T == 0 or
    // max_hit hits) has done[k] set and is never touched again.
    float T[PPL], cr[PPL], cg[PPL], cb[PPL], dz[PPL];
    int hits[PPL];
    bool done[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        T[k] = 1.f; cr[k] = cg[k] = cb[k] = dz[k] = 0.f; hits[k] = 0;
        done[k] = !(px0 + k < width && py_i < height);
    }
    auto all_done = [&]() -> bool {
        bool d = true;
#pragma unroll
        for (int k = 0; k < PPL; ++k) d = d && done[k];
        return __all(d);
    };

    int range_start, range_end;
    {
        const int s = isect_offsets[tflat];
        const int e = (tflat + 1 < total_tiles) ? isect_offsets[tflat + 1] : n_isects;
        range_start = min(max(s, 0), n_isects);
        range_end = min(max(e, range_start), n_isects);
    }
    // the wave's pixel-centre rectangle (pixels inside the image only; a strip below the image's last row is empty,
    // ry1 < ry0, and culls every record)
    const float rx0 = (float)(txi * 16) + 0.5f, ry0 = (float)(tyi * 16 + sub * ROWS) + 0.5f;
    const float rx1 = (float)min(txi * 16 + 15, width - 1) + 0.5f;
    const float ry1 = (float)min(tyi * 16 + sub * ROWS + ROWS - 1, height - 1) + 0.5f;

    float4 g_geo = make_float4(0.f, 0.f, -1.f, 0.f), g_col = make_float4(0.f, 0.f, 0.f, 0.f);
    auto gather = [&](int idx) {
        g_geo = make_float4(0.f, 0.f, -1.f, 0.f);           // r^2 < 0: covers nothing
        if (idx < range_end) {
            const int g = flatten_ids[idx];
            if ((unsigned)g < (unsigned)N) {
                g_geo = records[(int64_t)g * 2];
                g_col = records[(int64_t)g * 2 + 1];
            }
        }
    };
    gather(range_start + lane);
    for (int base = range_start; base < range_end; base += RB) {
        if (all_done()) break;
        // ---- cull against the tile rectangle + compact.  The rectangle's nearest point to the centre is no nearer
        // than any pixel centre in it, coordinate by coordinate, and fp32 rounding is monotone: a record dropped here
        // covers no pixel of the tile under the per-pixel test below.
        const float ex = fmaxf(fmaxf(rx0 - g_geo.x, g_geo.x - rx1), 0.f);
        const float ey = fmaxf(fmaxf(ry0 - g_geo.y, g_geo.y - ry1), 0.f);
        const bool keep = ex * ex + ey * ey <= g_geo.z;
        const unsigned long long m = __ballot(keep);
        const int bsz = __popcll(m);
        __syncthreads();        // single-wave workgroup: the previous batch's LDS reads before these writes
        if (keep) {
            const int slot = __popcll(m & sc_lanemask_lt());
            geo_s[slot] = g_geo;
            col_s[slot] = g_col;
        }
        __syncthreads();
        gather(base + RB + lane);                          // next batch in flight during the blend
        for (int t = 0; t < bsz; ++t) {
            const float4 p = geo_s[t], c = col_s[t];       // broadcast reads
            const float dy = pyf - p.y;
            const float dy2 = dy * dy;
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                const float dx = ((float)(px0 + k) + 0.5f) - p.x;
                const bool cov = !done[k] && dx * dx + dy2 <= p.z;
                if (cov) {
                    const float w = T[k] * c.w;
                    cr[k] += w * c.x;
                    cg[k] += w * c.y;
                    cb[k] += w * c.z;
                    dz[k] += w * p.w;
                    T[k] = T[k] * (1.f - c.w);
                    hits[k] += 1;
                    done[k] = T[k] == 0.f || hits[k] >= max_hit;
                }
            }
            if ((t & 7) == 7 && all_done()) break;
        }
    }
    const float bg0 = background ? background[0] : 0.f, bg1 = background ? background[1] : 0.f,
                bg2 = background ? background[2] : 0.f;
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
        if (!(px0 + k < width && py_i < height)) continue;
        const int64_t pix = (int64_t)py_i * width + px0 + k;
        float* o = out_rgb + pix * pix_stride;
        o[0] = cr[k] + T[k] * bg0;
        o[ch_stride] = cg[k] + T[k] * bg1;
        o[2 * ch_stride] = cb[k] + T[k] * bg2;
        out_alpha[pix * alpha_stride] = 1.f - T[k];
        if (out_depth) out_depth[pix] = dz[k];
    }
}

}  // namespace

int g_sc_point_raster_waves = 4;    // sc_set_option "point_raster_waves": waves per 16 x 16 tile, 1 or 4

extern "C" int sc_point_project(const float* points, const float* colors, const float* opacities, float occ,
                                const float* radius_in, int N, const double* viewmat, double fx, double fy,
                                double cx, double cy, double focal_r, int width, int height, double near_plane,
                                double far_plane, int radius_mode, double scale, float knn_scale_down, int32_t* radii,
                                float* means2d, float* depths, float* records, sc_stream_t stream) {
    if (N < 0 || width <= 0 || height <= 0) return SC_EINVAL;
    if (radius_mode < SC_RMODE_CONST || radius_mode > SC_RMODE_ARRAY) return SC_EINVAL;
    if (!opacities && !(occ > 0.f && occ <= 1.f)) return SC_EINVAL;
    if ((radius_mode == SC_RMODE_KNN || radius_mode == SC_RMODE_ARRAY) && !radius_in) return SC_EINVAL;
    if (!(focal_r > 0.0) || !(scale >= 0.0)) return SC_EINVAL;
    if (N == 0) return SC_OK;
    if (!points || !colors || !viewmat || !radii || !means2d || !depths || !records) return SC_EINVAL;
    if (((uintptr_t)records & 15) != 0) return SC_EINVAL;        // written as float4
    const double half_min_hw = 0.5 * (double)(height <= width ? height : width);
    const ScPointCam cam = {fx, fy, cx, cy, focal_r, near_plane, far_plane, scale, half_min_hw, radius_mode,
                            knn_scale_down};
    hipLaunchKernelGGL(point_project_kernel, dim3((unsigned)((N + PROJ_BLK - 1) / PROJ_BLK)), dim3(PROJ_BLK), 0,
                       sc_s(stream), points, colors, opacities, occ, radius_in, N, viewmat, cam, radii, means2d,
                       depths, reinterpret_cast<float4*>(records));
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_point_rasterize_fwd(const float* records, int N, int width, int height, int tile_width,
                                      int tile_height, const int32_t* isect_offsets, const int32_t* flatten_ids,
                                      int64_t n_isects, int max_hit, const float* background, float* out_rgb,
                                      int64_t pix_stride, int64_t ch_stride, float* out_alpha, int64_t alpha_stride,
                                      float* out_depth, sc_stream_t stream) {
    if (N < 0 || width <= 0 || height <= 0 || max_hit < 1 || n_isects < 0 || n_isects > 0x7fffffff) return SC_EINVAL;
    if (tile_width != (width + 15) / 16 || tile_height != (height + 15) / 16) return SC_EINVAL;
    if (pix_stride < 1 || ch_stride < 1 || alpha_stride < 1) return SC_EINVAL;
    if (!records || !isect_offsets || !flatten_ids || !out_rgb || !out_alpha) return SC_EINVAL;
    if (((uintptr_t)records & 15) != 0) return SC_EINVAL;        // read as float4
    const unsigned tiles = (unsigned)(tile_width * tile_height);
    if (g_sc_point_raster_waves == 1)
        hipLaunchKernelGGL(point_raster_fwd_kernel<4>, dim3(tiles), dim3(64), 0, sc_s(stream),
                           reinterpret_cast<const float4*>(records), N, width, height, tile_width, tile_height,
                           isect_offsets, flatten_ids, (int)n_isects, max_hit, background, out_rgb, pix_stride,
                           ch_stride, out_alpha, alpha_stride, out_depth);
    else
        hipLaunchKernelGGL(point_raster_fwd_kernel<1>, dim3(4 * tiles), dim3(64), 0, sc_s(stream),
                           reinterpret_cast<const float4*>(records), N, width, height, tile_width, tile_height,
                           isect_offsets, flatten_ids, (int)n_isects, max_hit, background, out_rgb, pix_stride,
                           ch_stride, out_alpha, alpha_stride, out_depth);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
