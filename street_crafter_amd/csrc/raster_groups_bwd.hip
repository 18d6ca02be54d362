// Grouped rasterizer backward for gfx950: the gradients of the composite image AND of the group images from ONE replay
// of the tile lists.  The reference gets the object accumulation loss (train.py:202-208: `render_object` under grad on
// four of every five iterations after densification) from a second whole operator sequence over pc.obj_list; here the
// object image is a second accumulator set of the same walk, forward (raster_groups.hip) and backward.
//
// The gradient is linear in the upstream images, so per record it is the sum of what rasterize_to_pixels' backward gives
// for the composite (on the full list) and for the record's own group (on the group's sub-list).  sigma and alpha are the
// same numbers in both: they are evaluated once, with the pinned arithmetic of raster_common.h, and the skip decision is
// the forward's.  Each set then runs the usual recurrence with its own transmittance (rebuilt from 1 - that set's stored
// alpha) and its own running dot product W (raster_bwd.hip, raster_bwd_item, on W); a record takes part in a set while
// its list position is <= the position the forward recorded for that set and pixel (last_pos).  The per-set v_alpha are
// summed and the chain to sigma, opacity, conic and mean runs once.  v_means2d_abs takes the COMPOSITE's term only: it is
// what rasterize_to_pixels(absgrad=True) on the full set attaches (the reference's object render has its own means2d and
// never reaches viewspace_points.absgrad).
//
// Shape: one 256-thread workgroup per 16x16 tile, one pixel per lane (three sets of state per pixel do not fit four
// pixels per lane).  Per round every wave stages 64 records back to front with the forward's exact tile cull and
// compacts them into its own LDS segment; the segments are then replayed in order.  Per record each wave reduces its 64
// pixels with the transposing butterfly (wave_transpose_sum16) into LDS; after a segment the four waves' partial sums of
// a record are added and ONE float atomic per (record, output value) leaves the tile, issued by 16 lanes per record side
// by side.  A row therefore receives one partial sum per tile list it is in, as from the wave-per-tile backward.
// The walk starts at the largest last_pos of the tile; a wave passes over records behind its own largest one, and a set
// whose upstream gradient is zero in a pixel is off there (its terms would all be products with zero), so a tile without
// object records, and the untouched group of the training form, cost the walk nothing.
// Safe against foreign last_pos / flatten_ids / isect_offsets: every last_pos is clamped into the tile's
// [range_start - 1, range_end), ids go through sc_safe_id, ranges through sc_tile_range.
#include "raster_walk.h"

namespace {

constexpr int BW_WAVES = 4;              // 256 threads: one pixel of the 16x16 tile per lane
constexpr int BW_SEG = 64;               // records a wave stages per round
constexpr int BW_RED_STRIDE = 16 * BW_WAVES + 16;     // floats per record in red_s (+16: records t, t + 1 on other banks)

template <int CDIM, int NG>
__global__ __launch_bounds__(64 * BW_WAVES) void raster_groups_bwd_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ colors,
    const float* __restrict__ opacities, const uint8_t* __restrict__ group_ids, int N, int NS, int width, int height,
    int tile_width, int tile_height, int total_tiles, const int32_t* __restrict__ isect_offsets,
    const int32_t* __restrict__ flatten_ids, int n_isects, const float* __restrict__ render_alphas,
    const float* __restrict__ group_alphas, const int32_t* __restrict__ last_pos,
    const float* __restrict__ v_render_colors, const float* __restrict__ v_render_alphas,
    const float* __restrict__ v_group_colors, const float* __restrict__ v_group_alphas,
    float* __restrict__ v_means2d_abs, float* __restrict__ v_means2d, float* __restrict__ v_conics,
    float* __restrict__ v_colors, float* __restrict__ v_opacities) {
    constexpr int NS_ = NG + 1;           // sets per pixel: 0 = composite, 1 + k = group k
    __shared__ float4 xyoa_s[BW_WAVES][BW_SEG];      // mx, my, log2(op), A2
    __shared__ float4 bck_s[BW_WAVES][BW_SEG];       // B2, C2, list position (int bits), flat id (int bits)
    __shared__ float4 col_s[BW_WAVES][BW_SEG];
    __shared__ int gid_s[BW_WAVES][BW_SEG];          // group id
    __shared__ float red_s[BW_SEG][BW_RED_STRIDE];   // per record of the segment: 16 sums of each wave
    __shared__ int cnt_s[BW_WAVES];
    __shared__ int hi_s[BW_WAVES];

    const int tflat = blockIdx.x;                    // the grid is exactly total_tiles blocks
    const ScTileId tile = sc_tile_id(tflat, tile_width, tile_height);
    const int cam = tile.cam, txi = tile.txi, tyi = tile.tyi;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int px_i = txi * 16 + (tid & 15), py_i = tyi * 16 + (tid >> 4);
    const float px = (float)px_i + 0.5f, py = (float)py_i + 0.5f;
    const bool inside = (px_i < width) && (py_i < height);
    const int64_t pix = inside ? ((int64_t)cam * height + py_i) * width + px_i : 0;
    const int64_t n_pix = (int64_t)(total_tiles / (tile_width * tile_height)) * height * width;    // pixels of one image set [C,H,W]

    int range_start, range_end;
    sc_tile_range(isect_offsets, tflat, total_tiles, n_isects, range_start, range_end);
    const int none = range_start - 1;                // the forward's "this set blended nothing in this pixel"

    // per set: transmittance, W = T_final v_alpha_upstream - (colour sums behind) . v_colour_upstream, upstream colour
    // gradient, last position.  A set is off in this pixel (position `none`) when both of its upstream pointers are null
    // or its upstream gradient is zero here.
    float T[NS_], W[NS_], vrc[NS_][CDIM];
    int lp[NS_];
    int wave_hi = none;
#pragma unroll
    for (int s = 0; s < NS_; ++s) {
        const float* vc = s == 0 ? v_render_colors : v_group_colors;
        const float* va = s == 0 ? v_render_alphas : v_group_alphas;
        const int64_t at = (int64_t)(s == 0 ? 0 : s - 1) * n_pix + pix;
        const bool on = inside && (vc != nullptr || va != nullptr);
        const float T_fin = on ? 1.0f - (s == 0 ? render_alphas : group_alphas)[at] : 1.0f;
        const float v_ra = (on && va) ? va[at] : 0.f;
        bool nonzero = v_ra != 0.f;
#pragma unroll
        for (int d = 0; d < CDIM; ++d) {
            vrc[s][d] = (on && vc) ? vc[at * CDIM + d] : 0.f;
            nonzero = nonzero || vrc[s][d] != 0.f;
        }
        lp[s] = (on && nonzero) ? min(max(last_pos[(int64_t)s * n_pix + pix], none), range_end - 1) : none;
        T[s] = T_fin;
        W[s] = T_fin * v_ra;
        wave_hi = max(wave_hi, lp[s]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wave_hi = max(wave_hi, __shfl_xor(wave_hi, o, 64));
    if (lane == 0) hi_s[wave] = wave_hi;
    __syncthreads();
    int tile_hi = hi_s[0];
#pragma unroll
    for (int w = 1; w < BW_WAVES; ++w) tile_hi = max(tile_hi, hi_s[w]);
    if (tile_hi < range_start) return;               // (the whole workgroup: tile_hi is the same in every thread)

    const ScRect rect = sc_tile_rect(tile, 0, 16, width, height);
    const float rx0 = rect.x0, rx1 = rect.x1, ry0 = rect.y0, ry1 = rect.y1;
    constexpr float LN2 = 0.6931471805599453f;

    // thread -> output value of the segment's reduction: tid & 15 names the sum as raster_bwd_item's lanes do
    // (sc_grad_owner; 9..10 are |mean| of the composite)
    const ScGradOwner out = sc_grad_owner<CDIM>(tid & 15, v_colors, v_conics, v_means2d, v_means2d_abs, v_opacities);

    for (int hi = tile_hi; hi >= range_start; hi -= BW_WAVES * BW_SEG) {
        // ---- stage: wave w takes positions hi - 64 w - lane (descending), culls and compacts into its segment ----------
        __syncthreads();
        {
            const int idx = hi - (wave * BW_SEG + lane);
            const int g = (idx >= range_start) ? sc_safe_id(flatten_ids[idx], NS) : -1;
            float2 xy = make_float2(0.f, 0.f);
            float ca = 0.f, cb = 0.f, cc = 0.f, op = 0.f;
            bool keep = false;
            if (g >= 0) {
                xy = *reinterpret_cast<const float2*>(means2d + (int64_t)g * 2);
                const float* cn = conics + (int64_t)g * 3;
                ca = cn[0]; cb = cn[1]; cc = cn[2];
                op = opacities[g];
                keep = !splat_misses_rect(ca, cb, cc, op, rx0 - xy.x, rx1 - xy.x, ry0 - xy.y, ry1 - xy.y);
            }
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const int slot = __popcll(m & sc_lanemask_lt());
                const ScSplat sp = sc_prescale(xy.x, xy.y, ca, cb, cc, op);
                const float* c = colors + (int64_t)g * CDIM;
                const int local = g - cam * N;                  // group_ids is [N], shared by the cameras
                xyoa_s[wave][slot] = make_float4(sp.mx, sp.my, sp.lop, sp.A2);
                bck_s[wave][slot] = make_float4(sp.B2, sp.C2, __int_as_float(idx), __int_as_float(g));
                col_s[wave][slot] = make_float4(c[0], c[1], c[2], CDIM > 3 ? c[3] : 0.f);
                gid_s[wave][slot] = ((unsigned)local < (unsigned)N) ? (int)group_ids[local] : SC_GROUP_NONE;
            }
            if (lane == 0) cnt_s[wave] = __popcll(m);
        }
        __syncthreads();
        // ---- replay the segments in order, each followed by its reduction -------------------------------------------
        for (int w = 0; w < BW_WAVES; ++w) {
            const int bsz = cnt_s[w];                           // the same in every thread of the workgroup
            if (bsz == 0) continue;
            for (int t = 0; t < bsz; ++t) {
                const float4 a = xyoa_s[w][t], bc = bck_s[w][t], c = col_s[w][t];
                const int pos = __builtin_amdgcn_readfirstlane(__float_as_int(bc.z));
                const int gid = __builtin_amdgcn_readfirstlane(gid_s[w][t]);
                float s16[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) s16[i] = 0.f;
                bool wave_any = false;
                if (pos <= wave_hi) {                           // (uniform) behind this wave's last record: nothing here
                    const float cl[4] = {c.x, c.y, c.z, c.w};
                    const float dx = a.x - px, dy = a.y - py;
                    // sigma and alpha once, in the forward's pinned arithmetic: the skip decision is the forward's
                    const float sg = sc_sigma2(a.w, sc_row_b(bc.x, dy), sc_row_q(bc.y, dy), dx);
                    const float araw = __builtin_amdgcn_exp2f(__fsub_rn(a.z, sg));      // op exp(-sigma)
                    const float al = fminf(SC_ALPHA_MAX, araw);
                    const bool valid = sc_valid(sg, al);
                    const float ra = __builtin_amdgcn_rcpf(1.0f - al);                  // 1 - alpha >= 1e-3
                    float v_alpha = 0.f, v_alpha0 = 0.f, sc[CDIM];
#pragma unroll
                    for (int d = 0; d < CDIM; ++d) sc[d] = 0.f;
                    bool any_part = false;
                    // the recurrence of one set: its own T, W and upstream gradient
                    auto set_step = [&](float& Ts, float& Ws, const float (&v)[CDIM], int lps, bool composite) {
                        const bool part = valid && pos <= lps;
                        const float Tn = Ts * ra;                                       // transmittance in front
                        const float fac = part ? al * Tn : 0.f;
                        float Q = cl[0] * v[0];                                         // sum_d c_d v_d of this record
#pragma unroll
                        for (int d = 1; d < CDIM; ++d) Q = __fmaf_rn(cl[d], v[d], Q);
#pragma unroll
                        for (int d = 0; d < CDIM; ++d) sc[d] = __fmaf_rn(fac, v[d], sc[d]);
                        const float va = part ? __fmaf_rn(ra, Ws, Tn * Q) : 0.f;        // W / (1 - alpha) + T Q
                        Ws = __fmaf_rn(-fac, Q, Ws);                                    // the record moves behind
                        Ts = part ? Tn : Ts;
                        v_alpha += va;
                        if (composite) v_alpha0 = va;
                        any_part = any_part || part;
                    };
                    set_step(T[0], W[0], vrc[0], lp[0], true);
                    // the record's own group: a uniform branch per group; an id >= NG is in the composite only
#pragma unroll
                    for (int k = 0; k < NG; ++k)
                        if (gid == k) set_step(T[1 + k], W[1 + k], vrc[1 + k], lp[1 + k], false);
                    wave_any = __any(any_part);
                    if (wave_any) {
                        // the chain behind v_alpha runs once; d alpha / d sigma = -alpha_raw while alpha is not clamped
                        const bool flow = araw <= SC_ALPHA_MAX;
                        const float vs = flow ? -araw * v_alpha : 0.f;
                        const float vs0 = flow ? -araw * v_alpha0 : 0.f;
                        // d sigma / d mean = (a dx + b dy, b dx + c dy) with a = 2 ln2 A2, b = ln2 B2, c = 2 ln2 C2
                        const float gx = __fmaf_rn(LN2 * 2.0f * a.w, dx, LN2 * bc.x * dy);
                        const float gy = __fmaf_rn(LN2 * bc.x, dx, LN2 * 2.0f * bc.y * dy);
#pragma unroll
                        for (int d = 0; d < CDIM; ++d) s16[d] = sc[d];
                        s16[4] = 0.5f * vs * dx * dx;           // d sigma / d conic = (dx^2 / 2, dx dy, dy^2 / 2)
                        s16[5] = vs * dx * dy;
                        s16[6] = 0.5f * vs * dy * dy;
                        s16[7] = vs * gx;
                        s16[8] = vs * gy;
                        s16[9] = fabsf(vs0) * fabsf(gx);        // absgrad: the composite's term alone
                        s16[10] = fabsf(vs0) * fabsf(gy);
                        s16[11] = -__builtin_amdgcn_exp2f(-a.z) * vs;      // d alpha / d op = alpha_raw / op
                    }
                }
                // (wave_any is uniform: every lane of the wave is in the butterfly)
                const float total = wave_any ? wave_transpose_sum16(s16, lane) : 0.f;
                if ((lane & 3) == 0) red_s[t][wave * 16 + (lane >> 2)] = total;        // lane 4 i owns sum i
            }
            __syncthreads();
            // ---- the four waves' sums of every record of the segment, one atomic per (record, value) -----------------
            for (int i = tid; i < bsz * 16; i += 64 * BW_WAVES) {
                const int t = i >> 4, vi = i & 15;                                      // vi == tid & 15
                float total = red_s[t][vi];
#pragma unroll
                for (int ww = 1; ww < BW_WAVES; ++ww) total += red_s[t][ww * 16 + vi];
                if (out.base && total != 0.f)
                    atomicAdd(out.base + (int64_t)__float_as_int(bck_s[w][t].w) * out.stride, total);
            }
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" int sc_rasterize_bwd_groups(const float* means2d, const float* conics, const float* colors,
                                       const float* opacities, const uint8_t* group_ids, int C, int N, int D,
                                       int n_groups, int width, int height, int tile_size, int tile_width,
                                       int tile_height, const int32_t* isect_offsets, const int32_t* flatten_ids,
                                       int64_t n_isects, const float* render_alphas, const float* group_alphas,
                                       const int32_t* last_pos, const float* v_render_colors,
                                       const float* v_render_alphas, const float* v_group_colors,
                                       const float* v_group_alphas, float* v_means2d_abs, float* v_means2d,
                                       float* v_conics, float* v_colors, float* v_opacities, sc_stream_t stream) {
    const int rc = sc_groups_check(C, N, n_groups, tile_width, tile_height, n_isects);
    if (rc < 0) return rc;
    if (D < 1 || width <= 0 || height <= 0 || tile_size < 1) return SC_EINVAL;
    if ((int64_t)tile_width * tile_size < width || (int64_t)tile_height * tile_size < height) return SC_EINVAL;
    if (tile_size != 16 || (D != 3 && D != 4)) return SC_EUNSUPPORTED;
    if (rc) return SC_OK;                 // C == 0: no gradient row
    if (!v_means2d || !v_conics || !v_colors || !v_opacities) return SC_EINVAL;
    if (n_isects == 0) return SC_OK;      // no record: the zero-filled gradients stand
    if (!v_render_colors && !v_render_alphas && !v_group_colors && !v_group_alphas) return SC_OK;     // every set is off
    if (!means2d || !conics || !colors || !opacities || !group_ids || !isect_offsets || !flatten_ids || !render_alphas ||
        !group_alphas || !last_pos)
        return SC_EINVAL;
    const int total_tiles = C * tile_width * tile_height;
#define SC_LAUNCH_GROUPS_BWD(CD, NG)                                                                                  \
    hipLaunchKernelGGL((raster_groups_bwd_kernel<CD, NG>), dim3(total_tiles), dim3(64 * BW_WAVES), 0, sc_s(stream),     \
                       means2d, conics, colors, opacities, group_ids, N, C * N, width, height, tile_width, tile_height, \
                       total_tiles, isect_offsets, flatten_ids, (int)n_isects, render_alphas, group_alphas, last_pos,   \
                       v_render_colors, v_render_alphas, v_group_colors, v_group_alphas, v_means2d_abs, v_means2d,      \
                       v_conics, v_colors, v_opacities)
    if (D == 4) { if (n_groups == 1) SC_LAUNCH_GROUPS_BWD(4, 1); else SC_LAUNCH_GROUPS_BWD(4, 2); }
    else { if (n_groups == 1) SC_LAUNCH_GROUPS_BWD(3, 1); else SC_LAUNCH_GROUPS_BWD(3, 2); }
#undef SC_LAUNCH_GROUPS_BWD
    SC_LAUNCH_CHECK();
    return SC_OK;
}
