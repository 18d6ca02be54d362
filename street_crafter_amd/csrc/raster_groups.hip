// Grouped rasterizer forward for gfx950: the composite image and one image per Gaussian group from ONE walk of the
// tile lists.  Replaces the three whole operator sequences of StreetGaussianRenderer.render_all
// (street_gaussian/models/street_gaussian_renderer.py:17-45: all non-sky models, ['background'], pc.obj_list) by one.
//
// Why the group images are bit-identical to their own renders: a group is a boolean-mask subset of the Gaussians, so its
// tile list is the subsequence of the full tile list (same depth keys, ties in Gaussian-index order, which the mask
// keeps); the blend is sequential per pixel; its arithmetic is pinned in raster_common.h and every variant compiles the one walk of
// raster_walk.h; and the tile-level cull is exact.  A set of (T, colour sums) that only ever sees its own group's records therefore goes through exactly the
// operations of a rasterizer that was handed the subset.
//
// Two kernels:
//   group_extents_kernel   per (camera, tile) and group: one past the last list position that holds the group.  Lets a
//                          tile stop waiting for a group that has no record left (most tiles hold no object record: without
//                          this they would walk their whole lists, and the early exit is what makes the forward fast).
//   raster_groups_kernel   one wave per 16x16 tile, four pixels per lane, the tile walk of raster_walk.h (ScStage,
//                          sc_cull_compact, sc_walk_batch): register-staged gathers one batch ahead, exact tile cull,
//                          compaction into LDS, blend.  Each pixel carries NG + 1 accumulator sets; a record is evaluated
//                          once (sc_pair_alpha) and blended into the composite set and into its own group's set
//                          (sc_blend_step).
// A finished set is marked in the SIGN of its transmittance (sc_blend_step, MARK_TSIGN); |T| is what it ends with.
// No dispatch list, work hint, packed records, planar output, backgrounds or tile masks.
// IDS (sc_rasterize_fwd_groups_ids, the training forward): every set also records, per pixel, the list position of the last
// record it blended -- what raster_groups_bwd.hip replays the list back from.  A record's position rides through the
// compaction in the fourth word of bck_s, which the forward-only instantiation leaves unused.
#include "raster_walk.h"

namespace {

constexpr int EXTENT_UNROLL = 8;          // list chunks of 64 in flight per wave of group_extents_kernel
constexpr int EXTENT_WAVES = 4;           // waves that share a tile's list in group_extents_kernel

// One block of EXTENT_WAVES waves per tile, walking the list from its END in steps of EXTENT_UNROLL * 64 records (all loads
// of a step are issued before the first is used: the walk is two dependent gathers per record); the waves take the steps
// in turn, each until it has seen every group or its steps are exhausted.  Every wave meets its positions in descending
// order, so the first record of a group it sees is the last one among ITS steps, and the maximum over the waves is the
// last one of the list.  (A list of 70 k records with no object record is 140 steps: the launch's tail.)
template <int NG>
__global__ __launch_bounds__(64 * EXTENT_WAVES) void group_extents_kernel(
    const int32_t* __restrict__ isect_offsets, const int32_t* __restrict__ flatten_ids, int n_isects,
    const uint8_t* __restrict__ group_ids, int N, int NS, int tiles_per_cam, int total_tiles,
    int32_t* __restrict__ group_end) {
    constexpr int STEP = 64 * EXTENT_UNROLL;
    __shared__ int end_s[EXTENT_WAVES][NG];
    const int tflat = blockIdx.x;                      // the grid is exactly total_tiles blocks
    const int lane = sc_lane(), wave = (int)(threadIdx.x >> 6);
    const int cam_base = (tflat / tiles_per_cam) * N;
    int range_start, range_end;
    sc_tile_range(isect_offsets, tflat, total_tiles, n_isects, range_start, range_end);
    int end_k[NG];
    bool found[NG];
#pragma unroll
    for (int k = 0; k < NG; ++k) { end_k[k] = range_start; found[k] = false; }
    for (int hi = range_end - wave * STEP; hi > range_start; hi -= STEP * EXTENT_WAVES) {
        int local[EXTENT_UNROLL], gid[EXTENT_UNROLL];
#pragma unroll
        for (int u = 0; u < EXTENT_UNROLL; ++u) {
            const int i = hi - 1 - u * 64 - lane;                   // lane 0 holds the LAST record of its chunk
            const int g = (i >= range_start) ? sc_safe_id(flatten_ids[i], NS) : -1;
            local[u] = (g >= 0) ? g - cam_base : -1;                // a dead entry belongs to no group
        }
#pragma unroll
        for (int u = 0; u < EXTENT_UNROLL; ++u)
            gid[u] = ((unsigned)local[u] < (unsigned)N) ? (int)group_ids[local[u]] : SC_GROUP_NONE;
        bool all_found = true;
#pragma unroll
        for (int k = 0; k < NG; ++k) {
#pragma unroll
            for (int u = 0; u < EXTENT_UNROLL; ++u) {
                const unsigned long long m = __ballot(gid[u] == k);
                if (!found[k] && m) {
                    found[k] = true;
                    end_k[k] = hi - u * 64 - (__ffsll((long long)m) - 1);      // position of the lowest set lane, plus one
                }
            }
            all_found = all_found && found[k];
        }
        if (all_found) break;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NG; ++k) end_s[wave][k] = end_k[k];
    }
    __syncthreads();
    if (threadIdx.x < NG) {
        int last = range_start;
#pragma unroll
        for (int w = 0; w < EXTENT_WAVES; ++w) last = max(last, end_s[w][threadIdx.x]);
        group_end[(int64_t)tflat * NG + threadIdx.x] = last;
    }
}

template <int CDIM, int NG, bool IDS>
__global__ __launch_bounds__(64) void raster_groups_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ colors,
    const float* __restrict__ opacities, const uint8_t* __restrict__ group_ids,
    const int32_t* __restrict__ group_end, int N, int NS, int width, int height, int tile_width, int tile_height,
    int total_tiles, const int32_t* __restrict__ isect_offsets, const int32_t* __restrict__ flatten_ids, int n_isects,
    float* __restrict__ render_colors, float* __restrict__ render_alphas, float* __restrict__ group_colors,
    float* __restrict__ group_alphas, int32_t* __restrict__ last_pos) {
    constexpr int B = SC_WALK_B;
    constexpr int NS_ = NG + 1;           // accumulator sets per pixel: 0 = composite, 1 + k = group k
    __shared__ float4 xyoa_s[B + 1];      // the compacted batch (sc_cull_compact); bck_s carries the record's group id
    __shared__ float4 bck_s[B + 1];       // and, with IDS, its list position
    __shared__ float4 col_s[B + 1];

    const int tflat = blockIdx.x;
    if (tflat >= total_tiles) return;
    const ScTileId tile = sc_tile_id(tflat, tile_width, tile_height);
    const int cam = tile.cam;
    const int lane = threadIdx.x;
    const ScLanePixels<1> px(tile, 0, lane, width, height);
    const bool (&inside)[4] = px.inside;
    const int64_t pix0 = px.pix0;
    sc_f2 pxp[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) pxp[p] = sc_f2{(float)(px.px0_i + 2 * p) + 0.5f, (float)(px.px0_i + 2 * p + 1) + 0.5f};

    int range_start, range_end;
    sc_tile_range(isect_offsets, tflat, total_tiles, n_isects, range_start, range_end);
    const int num_batches = (range_end - range_start + B - 1) / B;
    int gend[NG];                         // wave-uniform: no record of group k at or after this list position
#pragma unroll
    for (int k = 0; k < NG; ++k) gend[k] = min(max(group_end[(int64_t)tflat * NG + k], range_start), range_end);
    const ScRect rect = px.rect(tile, 0, width, height);

    // per-pixel state, in pixel PAIRS.  A finished set is marked in the sign of its T (MARK_TSIGN); a pixel outside the
    // image starts finished.
    sc_f2 T2[NS_][2];
    float acc[NS_][4][CDIM];
#pragma unroll
    for (int s = 0; s < NS_; ++s) {
#pragma unroll
        for (int p = 0; p < 2; ++p) T2[s][p] = sc_f2{inside[2 * p] ? 1.f : -1.f, inside[2 * p + 1] ? 1.f : -1.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int d = 0; d < CDIM; ++d) acc[s][k][d] = 0.f;
    }
    int lastp[IDS ? NS_ : 1][4];          // IDS: position of the last record set s blended into pixel k
#pragma unroll
    for (int s = 0; s < (IDS ? NS_ : 1); ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) lastp[s][k] = range_start - 1;
    // sign bit set <=> all four pixels of this lane have finished set s
    auto lane_bits = [&](int s) -> int {
        return __float_as_int(T2[s][0].x) & __float_as_int(T2[s][0].y) & __float_as_int(T2[s][1].x) &
               __float_as_int(T2[s][1].y);
    };
    bool gdone[NG];                       // wave-uniform, refreshed per batch: group k's sets are finished in this tile

    // register-staged pipeline: parameters of batch b, ids of batch b + 1; the record's group id is staged with it
    const ScSplatArrays in = {means2d, conics, colors, opacities};
    ScStage<CDIM> st;
    st.clear();
    int p_gid = SC_GROUP_NONE;
    auto load_gid = [&](int g) {
        const int local = g - cam * N;                  // group_ids is [N], shared by the cameras
        p_gid = ((unsigned)local < (unsigned)N) ? (int)group_ids[local] : SC_GROUP_NONE;
    };
    st.load(st.id_at(flatten_ids, range_start + lane, range_end, NS), in, load_gid);
    st.g_next = st.id_at(flatten_ids, range_start + B + lane, range_end, NS);

    for (int b = 0; b < num_batches; ++b) {
        const int batch_start = range_start + B * b;
        // ---- what is still open (wave-uniform) ------------------------------------------------------------------
        const bool cdone = __all(lane_bits(0) < 0);
        bool every = cdone;
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            gdone[k] = (batch_start >= gend[k]) || __all(lane_bits(1 + k) < 0);
            every = every && gdone[k];
        }
        if (every) break;
        // ---- cull + compact: a record whose composite AND own group's sets are finished everywhere can change nothing
        auto open = [&]() -> bool {
            bool o = !cdone;
#pragma unroll
            for (int k = 0; k < NG; ++k) o = o || (p_gid == k && !gdone[k]);
            return o;
        };
        const int bsz = sc_cull_compact<false>(st, rect, __int_as_float(p_gid), IDS ? __int_as_float(batch_start + lane) : 0.f,
                                               xyoa_s, bck_s, col_s, open);
        st.advance(in, flatten_ids, batch_start + 2 * B + lane, range_end, NS, load_gid);
        // ---- blend ---------------------------------------------------------------------------------------------
        if (bsz > 0) {
            // one record: a = (mx, my, log2 op, B2), bc = (A2, C2, group id, IDS: list position), c = colour
            auto blend = [&](const float4& a, const float4& bc, const float4& c) {
                const float dy = a.y - px.py;
                const float bdy = sc_row_b(a.w, dy), qdy = sc_row_q(bc.y, dy);    // shared by the lane's pixels
                const int gid = __builtin_amdgcn_readfirstlane(__float_as_int(bc.z));     // same record in every lane
                const int pos = __float_as_int(bc.w);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    // evaluated ONCE per record, blended into the composite set and into its own group's set
                    const ScPairAlpha pa = sc_pair_alpha(a.x, bc.x, a.z, bdy, qdy, pxp[p]);
                    auto step = [&](int s) {
                        sc_blend_step<MARK_TSIGN, CDIM, IDS>(pa.al, pa.v0, pa.v1, c, T2[s][p], pxp[p], acc[s][2 * p],
                                                             acc[s][2 * p + 1], pos, lastp[IDS ? s : 0][2 * p],
                                                             lastp[IDS ? s : 0][2 * p + 1]);
                    };
                    step(0);
                    // the record's own group: unrolled predication on a wave-uniform id (a uniform branch per group)
#pragma unroll
                    for (int k = 0; k < NG; ++k)
                        if (gid == k) step(1 + k);
                }
            };
            auto all_done = [&]() -> bool {
                int mbits = lane_bits(0);
#pragma unroll
                for (int k = 0; k < NG; ++k) mbits &= gdone[k] ? -1 : lane_bits(1 + k);
                return __all(mbits < 0);
            };
            sc_walk_batch(xyoa_s, bck_s, col_s, bsz, blend, all_done);
        }
    }

    // ---- every pixel inside the image is written, for every set ---------------------------------------------------
    const int64_t n_pix = (int64_t)(total_tiles / (tile_width * tile_height)) * height * width;     // pixels of one image set [C,H,W]
#pragma unroll
    for (int s = 0; s < NS_; ++s) {
        float* out_c = s == 0 ? render_colors : group_colors + (int64_t)(s - 1) * n_pix * CDIM;
        float* out_a = s == 0 ? render_alphas : group_alphas + (int64_t)(s - 1) * n_pix;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!inside[k]) continue;
            const float Tk = fabsf((k & 1) ? T2[s][k >> 1].y : T2[s][k >> 1].x);
            const int64_t pix = pix0 + k;
            out_a[pix] = 1.0f - Tk;
            if constexpr (IDS) last_pos[(int64_t)s * n_pix + pix] = lastp[s][k];
            sc_store_pixel<CDIM>(out_c, pix, acc[s][k]);
        }
    }
}

}  // namespace

extern "C" int sc_group_extents(const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                                const uint8_t* group_ids, int C, int N, int n_groups, int tile_width, int tile_height,
                                int32_t* group_end, sc_stream_t stream) {
    const int rc = sc_groups_check(C, N, n_groups, tile_width, tile_height, n_isects);
    if (rc) return rc < 0 ? rc : SC_OK;
    if (!isect_offsets || !group_end) return SC_EINVAL;
    if (n_isects > 0 && (!flatten_ids || !group_ids)) return SC_EINVAL;
    const int total_tiles = C * tile_width * tile_height;
    const dim3 grid(total_tiles), block(64 * EXTENT_WAVES);
#define SC_LAUNCH_EXTENTS(NG)                                                                                       \
    hipLaunchKernelGGL((group_extents_kernel<NG>), grid, block, 0, sc_s(stream), isect_offsets, flatten_ids,        \
                       (int)n_isects, group_ids, N, C * N, tile_width * tile_height, total_tiles, group_end)
    if (n_groups == 1) SC_LAUNCH_EXTENTS(1); else SC_LAUNCH_EXTENTS(2);
#undef SC_LAUNCH_EXTENTS
    SC_LAUNCH_CHECK();
    return SC_OK;
}

// both forward entries: the checks, then the kernel with or without the per-set last positions
template <bool IDS>
static int launch_fwd_groups(const float* means2d, const float* conics, const float* colors, const float* opacities,
                             const uint8_t* group_ids, const int32_t* group_end, int C, int N, int D, int n_groups,
                             int width, int height, int tile_size, int tile_width, int tile_height,
                             const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                             float* render_colors, float* render_alphas, float* group_colors, float* group_alphas,
                             int32_t* last_pos, sc_stream_t stream) {
    const int rc = sc_groups_check(C, N, n_groups, tile_width, tile_height, n_isects);
    if (rc < 0) return rc;
    if (D < 1 || width <= 0 || height <= 0 || tile_size < 1) return SC_EINVAL;
    if ((int64_t)tile_width * tile_size < width || (int64_t)tile_height * tile_size < height) return SC_EINVAL;
    if (tile_size != 16 || (D != 3 && D != 4)) return SC_EUNSUPPORTED;
    if (rc) return SC_OK;                 // C == 0: no pixel to write
    if (!isect_offsets || !group_end || !render_colors || !render_alphas || !group_colors || !group_alphas)
        return SC_EINVAL;
    if (IDS && !last_pos) return SC_EINVAL;
    if (n_isects > 0 && (!means2d || !conics || !colors || !opacities || !flatten_ids || !group_ids)) return SC_EINVAL;
    const int total_tiles = C * tile_width * tile_height;
#define SC_LAUNCH_GROUPS(CD, NG)                                                                                    \
    hipLaunchKernelGGL((raster_groups_kernel<CD, NG, IDS>), dim3(total_tiles), dim3(64), 0, sc_s(stream), means2d,  \
                       conics, colors, opacities, group_ids, group_end, N, C * N, width, height, tile_width,         \
                       tile_height, total_tiles, isect_offsets, flatten_ids, (int)n_isects, render_colors,           \
                       render_alphas, group_colors, group_alphas, last_pos)
    if (D == 4) { if (n_groups == 1) SC_LAUNCH_GROUPS(4, 1); else SC_LAUNCH_GROUPS(4, 2); }
    else { if (n_groups == 1) SC_LAUNCH_GROUPS(3, 1); else SC_LAUNCH_GROUPS(3, 2); }
#undef SC_LAUNCH_GROUPS
    SC_LAUNCH_CHECK();
    return SC_OK;
}

extern "C" int sc_rasterize_fwd_groups(const float* means2d, const float* conics, const float* colors,
                                       const float* opacities, const uint8_t* group_ids, const int32_t* group_end,
                                       int C, int N, int D, int n_groups, int width, int height, int tile_size,
                                       int tile_width, int tile_height, const int32_t* isect_offsets,
                                       const int32_t* flatten_ids, int64_t n_isects, float* render_colors,
                                       float* render_alphas, float* group_colors, float* group_alphas,
                                       sc_stream_t stream) {
    return launch_fwd_groups<false>(means2d, conics, colors, opacities, group_ids, group_end, C, N, D, n_groups, width,
                                    height, tile_size, tile_width, tile_height, isect_offsets, flatten_ids, n_isects,
                                    render_colors, render_alphas, group_colors, group_alphas, nullptr, stream);
}

extern "C" int sc_rasterize_fwd_groups_ids(const float* means2d, const float* conics, const float* colors,
                                           const float* opacities, const uint8_t* group_ids, const int32_t* group_end,
                                           int C, int N, int D, int n_groups, int width, int height, int tile_size,
                                           int tile_width, int tile_height, const int32_t* isect_offsets,
                                           const int32_t* flatten_ids, int64_t n_isects, float* render_colors,
                                           float* render_alphas, float* group_colors, float* group_alphas,
                                           int32_t* last_pos, sc_stream_t stream) {
    return launch_fwd_groups<true>(means2d, conics, colors, opacities, group_ids, group_end, C, N, D, n_groups, width,
                                   height, tile_size, tile_width, tile_height, isect_offsets, flatten_ids, n_isects,
                                   render_colors, render_alphas, group_colors, group_alphas, last_pos, stream);
}
