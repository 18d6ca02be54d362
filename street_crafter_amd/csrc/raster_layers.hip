// Layered rasterizer forward for gfx950: the images of TWO independent layers of Gaussians -- a front layer (rows
// [0, n_front) of every camera) and a back layer (rows [n_front, N)) -- from ONE walk of the tile lists.  Replaces the
// second whole operator sequence of StreetGaussianRenderer.render_novel_view (street_gaussian_renderer.py:136-163: every
// sub-model but the sky, then render_sky over the sky Gaussians alone, then rgb + rgb_sky * (1 - acc)) by one projection,
// one isect_tiles and this kernel.
//
// The contract on the lists: they come from isect_tiles on LAYERED depth keys (street_crafter_amd/layers.py,
// layered_depths: the back rows' depths times a power of two larger than far / near, an exact and order-preserving lift
// that puts every visible back record behind every front record), so every tile's list is [front records by depth][back records by depth], and each
// part is that layer's own list.  The blend is sequential per pixel, its arithmetic is pinned in raster_common.h and the
// tile cull is exact: a set of (T, colour sums) that only ever sees its own layer's records goes through exactly the
// operations of a rasterizer that was handed that layer alone (the argument of raster_groups.hip).
//
// Per tile (one wave per 16x16 tile, four pixels per lane, the shape of raster_fwd.hip's wave kernel):
//   boundary  the first list position whose Gaussian is a back row, by a wave-wide 64-ary search (each lane probes one of
//             64 evenly spaced positions, one ballot per round: three rounds settle 2^18 records).  Its first probe is
//             issued beside the first front batch's gathers.  A dead entry (id outside [0, C*N)) counts as front.
//   phase 1   blends [start, boundary) until every pixel has terminated or the boundary is reached;
//   phase 2   blends [boundary, end) with a fresh accumulator set and its own termination vote (the skip-ahead: a front
//             layer that saturates after ten records does not walk the rest of its list to find the sky).
// The phases are sequential and the front images leave the registers before phase 2 starts (EPILOGUE 0: stored; frame
// epilogues: reduced to the clamped colour and 1 - acc and parked in 4 KB of LDS), so the blend loop carries ONE
// accumulator set, as the single-image kernel does.  On a list that is not layered the images are unspecified; every access stays in bounds
// (the search only ever probes inside the tile's clamped range, ids go through sc_safe_id).
// No backgrounds, tile masks, dispatch list, work hint, packed records or backward.
#include "raster_common.h"

namespace {

// one batch of the register-staged pipeline: the parameters of the record this lane stages, the id of the one after
struct LayerStage {
    float2 xy;
    float a, b, c, op;
    float4 col;
    bool live;
    int g_next;
};

template <int CDIM>
__device__ __forceinline__ void stage_load(LayerStage& st, int g, const float* __restrict__ means2d,
                                           const float* __restrict__ conics, const float* __restrict__ colors,
                                           const float* __restrict__ opacities) {
    st.live = g >= 0;
    if (!st.live) return;
    st.xy = *reinterpret_cast<const float2*>(means2d + (int64_t)g * 2);
    const float* cn = conics + (int64_t)g * 3;
    st.a = cn[0]; st.b = cn[1]; st.c = cn[2];
    st.op = opacities[g];
    const float* c = colors + (int64_t)g * CDIM;
    st.col = make_float4(c[0], c[1], c[2], CDIM > 3 ? c[3] : 0.f);
}

// Blends list positions [ps, pe) into (T2, acc), ND colour channels.  `st` holds the parameters of positions ps + lane
// and the ids of ps + 64 + lane (both already masked to the range).  The loop of raster_fwd.hip's raster_item (one
// record per lane per batch, whole tile): a finished pixel is marked by poisoning its x coordinate with +inf.
template <int CDIM, int ND>
__device__ __forceinline__ void blend_range(
    LayerStage& st, int ps, int pe, const float* __restrict__ means2d, const float* __restrict__ conics,
    const float* __restrict__ colors, const float* __restrict__ opacities, int NS,
    const int32_t* __restrict__ flatten_ids, float rx0, float rx1, float ry0, float ry1, float py, sc_f2 (&pxp)[2],
    sc_f2 (&T2)[2], float (&acc)[4][4], float4* xyoa_s, float4* bck_s, float4* col_s) {
    constexpr int B = 64;
    const int lane = threadIdx.x;
    const float INF = __builtin_huge_valf();
    const int num_batches = (pe - ps + B - 1) / B;
    auto all_done = [&]() -> bool {
        int m = min(min(__float_as_int(pxp[0].x), __float_as_int(pxp[0].y)),
                    min(__float_as_int(pxp[1].x), __float_as_int(pxp[1].y)));
        return __all(m == 0x7f800000);
    };
    for (int b = 0; b < num_batches; ++b) {
        if (all_done()) break;
        const int batch_start = ps + B * b;
        // ---- cull + compact (the workgroup is this wave) --------------------------------------------------------
        __syncthreads();   // single-wave workgroup: orders the previous batch's LDS reads vs these writes
        bool keep = false;
        if (st.live)
            keep = !splat_misses_rect(st.a, st.b, st.c, st.op, rx0 - st.xy.x, rx1 - st.xy.x, ry0 - st.xy.y,
                                      ry1 - st.xy.y);
        const unsigned long long m = __ballot(keep);
        const int bsz = __popcll(m);
        if (keep) {
            const int slot = __popcll(m & sc_lanemask_lt());
            const ScSplat sp = sc_prescale(st.xy.x, st.xy.y, st.a, st.b, st.c, st.op);
            xyoa_s[slot] = make_float4(sp.mx, sp.my, sp.lop, sp.B2);
            // (an exactly-zero A2 would turn the +inf of a finished pixel into NaN: raster_fwd.hip)
            bck_s[slot] = make_float4(sp.A2 == 0.f ? 1e-37f : sp.A2, sp.C2, 0.f, 0.f);
            col_s[slot] = st.col;
        }
        __syncthreads();
        // ---- next batch's parameters and the ids after that go in flight ------------------------------------------
        stage_load<CDIM>(st, st.g_next, means2d, conics, colors, opacities);
        {
            const int idx2 = batch_start + 2 * B + lane;
            st.g_next = (idx2 < pe) ? sc_safe_id(flatten_ids[idx2], NS) : -1;
        }
        // ---- blend ---------------------------------------------------------------------------------------------
        if (bsz > 0) {
            // one record: a = (mx, my, log2 op, B2), bc = (A2, C2, -, -), c = colour
            auto blend = [&](const float4& a, const float4& bc, const float4& c) {
                const float dy = a.y - py;
                const float bdy = sc_row_b(a.w, dy), qdy = sc_row_q(bc.y, dy);    // shared by the lane's pixels
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    // the pinned arithmetic of raster_common.h, two pixels per instruction
                    const sc_f2 dx = sc_f2{a.x, a.x} - pxp[p];
                    const sc_f2 tt = __builtin_elementwise_fma(sc_f2{bc.x, bc.x}, dx, sc_f2{bdy, bdy});
                    const sc_f2 sg = __builtin_elementwise_fma(tt, dx, sc_f2{qdy, qdy});
                    const sc_f2 e = sc_f2{a.z, a.z} - sg;
                    const sc_f2 al = sc_f2{fminf(SC_ALPHA_MAX, __builtin_amdgcn_exp2f(e.x)),
                                           fminf(SC_ALPHA_MAX, __builtin_amdgcn_exp2f(e.y))};
                    const bool v0 = sc_valid(sg.x, al.x), v1 = sc_valid(sg.y, al.y);
                    const sc_f2 nT = __builtin_elementwise_fma(-al, T2[p], T2[p]);
                    const bool t0 = v0 && (nT.x <= SC_T_EPS), t1 = v1 && (nT.y <= SC_T_EPS);
                    const bool b0 = v0 != t0, b1 = v1 != t1;                    // v && !t (t implies v)
                    const sc_f2 ae = sc_f2{b0 ? al.x : 0.f, b1 ? al.y : 0.f};   // one select drives vis AND T
                    const sc_f2 vis = ae * T2[p];
                    T2[p] = __builtin_elementwise_fma(-ae, T2[p], T2[p]);       // == nT when blending, else T
                    pxp[p] = sc_f2{t0 ? INF : pxp[p].x, t1 ? INF : pxp[p].y};
                    // adding c * 0 leaves the sums bit-identical to skipping (sums are never -0)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float vh = h ? vis.y : vis.x;
                        acc[2 * p + h][0] = __fmaf_rn(c.x, vh, acc[2 * p + h][0]);
                        acc[2 * p + h][1] = __fmaf_rn(c.y, vh, acc[2 * p + h][1]);
                        acc[2 * p + h][2] = __fmaf_rn(c.z, vh, acc[2 * p + h][2]);
                        if constexpr (ND > 3) acc[2 * p + h][3] = __fmaf_rn(c.w, vh, acc[2 * p + h][3]);
                    }
                }
            };
            // the next record is read from LDS while the current one blends; two register sets take turns
            float4 a0 = xyoa_s[0], b0 = bck_s[0], c0 = col_s[0], a1, b1, c1;
            int t = 0;
            for (;;) {
                a1 = xyoa_s[t + 1]; b1 = bck_s[t + 1]; c1 = col_s[t + 1];
                __builtin_amdgcn_sched_barrier(0);      // keeps the LDS reads above the blend (raster_fwd.hip)
                blend(a0, b0, c0);
                if (++t >= bsz) break;
                a0 = xyoa_s[t + 1]; b0 = bck_s[t + 1]; c0 = col_s[t + 1];
                __builtin_amdgcn_sched_barrier(0);
                blend(a1, b1, c1);
                if (all_done()) break;                  // the vote after every second record
                if (++t >= bsz) break;
            }
        }
    }
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// The frame's composite, front and back already clamped, keep = 1 - acc.
// Float frame: the torch expression of render_novel_view, `clamp(rgb + rgb_sky * (1 - acc), 0, 1)` -- a product and a sum,
// each rounded on its own (torch runs them as separate kernels), so contraction is switched off here.
__device__ __forceinline__ float composite_torch(float front, float back, float keep) {
#pragma clang fp contract(off)
    const float prod = back * keep;
    const float sum = front + prod;
    return clamp01(sum);
}
// uint8 frame: what sc_frame_composite_u8 computes (capi.hip).  Its product-and-sum pairs are compiled as fused
// multiply-adds (the compiler's default contraction), one rounding each; spelled out here so that the two agree on every
// pixel whatever a later compiler decides for this file.
__device__ __forceinline__ unsigned composite_u8(float front, float back, float keep, float bias) {
    const float v = clamp01(__fmaf_rn(back, keep, front));
    return (unsigned)(uint8_t)__fmaf_rn(v, 255.0f, bias);
}

// EPILOGUE 0: o0 front_colors [C,H,W,CDIM], o1 front_alphas [C,H,W,1], o2 back_colors [C,H,W,3], o3 back_alphas [C,H,W,1]
// EPILOGUE 1: o0 rgb [C,H,W,3], o1 acc [C,H,W,1], o2 depth [C,H,W,1] (CDIM == 4; nullable)
// EPILOGUE 2: o_u8 [C,H,W,3]; rounding 0 = truncate, 1 = +0.5 (sc_frame_composite_u8)
// The uint8 frame (the novel-view loop's form) asks for the single-image kernel's 5 waves per SIMD: it fits 96 VGPRs
// without scratch; the other epilogues take what the allocator gives them (DESIGN.md section 4 has the table).
template <int CDIM, int EPILOGUE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(EPILOGUE == 2 ? 5 : 4))) void raster_layers_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ colors,
    const float* __restrict__ opacities, int N, int NS, int n_front, int width, int height, int tile_width,
    int tile_height, int total_tiles, const int32_t* __restrict__ isect_offsets,
    const int32_t* __restrict__ flatten_ids, int n_isects, float* __restrict__ o0, float* __restrict__ o1,
    float* __restrict__ o2, float* __restrict__ o3, uint8_t* __restrict__ o_u8, int rounding,
    int32_t* __restrict__ layer_begin) {
    constexpr int B = 64;
    __shared__ float4 xyoa_s[B + 1];      // mx, my, log2 opacity, B2        (+1: the loop prefetches t + 1)
    __shared__ float4 bck_s[B + 1];       // A2, C2, -, -
    __shared__ float4 col_s[B + 1];       // colour channels
    // frame epilogues: the clamped front colour and 1 - acc of the lane's four pixels wait here while phase 2 runs (16
    // registers the blend loop would otherwise carry: one occupancy step)
    __shared__ float park_s[EPILOGUE ? 16 : 1][64];

    const int tflat = blockIdx.x;
    if (tflat >= total_tiles) return;
    const int tiles_per_cam = tile_width * tile_height;
    const int cam = tflat / tiles_per_cam;
    const int tile_id = tflat - cam * tiles_per_cam;
    const int tyi = tile_id / tile_width, txi = tile_id - tyi * tile_width;
    const int lane = threadIdx.x;
    // lane -> 4 consecutive pixels of one row of the tile
    const int px0_i = txi * 16 + 4 * (lane & 3), py_i = tyi * 16 + (lane >> 2);
    const float py = (float)py_i + 0.5f;
    const float INF = __builtin_huge_valf();
    bool inside[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) inside[k] = (px0_i + k < width) && (py_i < height);
    const int64_t pix0 = ((int64_t)cam * height + py_i) * width + px0_i;

    int range_start, range_end;
    sc_tile_range(isect_offsets, tflat, total_tiles, n_isects, range_start, range_end);

    // ---- the first front batch's ids and the search's first probes go in flight together ----------------------------
    LayerStage st;
    st.xy = make_float2(0.f, 0.f);
    st.a = st.b = st.c = st.op = 0.f;
    st.col = make_float4(0.f, 0.f, 0.f, 0.f);
    const int idx0 = range_start + lane, idx1 = idx0 + B;
    const int g0 = (idx0 < range_end) ? sc_safe_id(flatten_ids[idx0], NS) : -1;
    const int g1 = (idx1 < range_end) ? sc_safe_id(flatten_ids[idx1], NS) : -1;
    // Boundary search on [lo, hi]: no back record before lo, a back record (or the list's end) at hi.  A round cuts the
    // interval into 64 chunks of `step`; lane l probes the LAST position of chunk l, the first lane that sees a back
    // record names the chunk that holds the boundary.  Every probe lies in [lo, hi): inside the tile's clamped range.
    const int cam_base = cam * N;
    int lo = range_start, hi = range_end, step = 1, pos = 0, raw = 0;
    auto probe = [&]() {
        const int len = hi - lo;
        step = len <= 64 ? 1 : (len + 63) >> 6;
        const int64_t p64 = (int64_t)lo + (int64_t)(lane + 1) * step - 1;      // (past hi for the last lanes of a round)
        pos = p64 < hi ? (int)p64 : hi;
        raw = (pos < hi) ? flatten_ids[pos] : 0;
    };
    if (hi > lo) probe();
    stage_load<CDIM>(st, g0, means2d, conics, colors, opacities);
    while (hi > lo) {
        const int g = sc_safe_id(raw, NS);
        const bool back = (pos >= hi) || (g >= 0 && g - cam_base >= n_front);
        const unsigned long long m = __ballot(back);
        if (m == 0) { lo = hi; break; }
        const int j = __ffsll((long long)m) - 1;
        const int nlo = lo + j * step;
        hi = min(lo + (j + 1) * step - 1, hi);
        lo = nlo;
        if (hi > lo) probe();
    }
    const int lb = lo;                    // wave-uniform: the back layer's records are [lb, range_end)
    if (layer_begin && lane == 0) layer_begin[tflat] = lb;
    st.live = st.live && idx0 < lb;
    st.g_next = (idx1 < lb) ? g1 : -1;
    // the first back batch's ids, for the jump
    const int gb0 = (lb + lane < range_end) ? sc_safe_id(flatten_ids[lb + lane], NS) : -1;

    // the rectangle of pixel centres of this tile (only pixels inside the image count)
    const float rx0 = (float)(txi * 16) + 0.5f, ry0 = (float)(tyi * 16) + 0.5f;
    const float rx1 = (float)min(txi * 16 + 15, width - 1) + 0.5f;
    const float ry1 = (float)min(tyi * 16 + 15, height - 1) + 0.5f;

    sc_f2 pxp[2], T2[2];
    float acc[4][4];
    auto reset = [&](int px0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            pxp[p] = sc_f2{inside[2 * p] ? (float)(px0 + 2 * p) + 0.5f : INF,
                           inside[2 * p + 1] ? (float)(px0 + 2 * p + 1) + 0.5f : INF};
            T2[p] = sc_f2{1.f, 1.f};
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[k][d] = 0.f;
    };
    auto T_of = [&](int k) -> float { return (k & 1) ? T2[k >> 1].y : T2[k >> 1].x; };

    // ---- phase 1: the front layer -----------------------------------------------------------------------------------
    reset(px0_i);
    blend_range<CDIM, CDIM>(st, range_start, lb, means2d, conics, colors, opacities, NS, flatten_ids, rx0, rx1, ry0, ry1,
                            py, pxp, T2, acc, xyoa_s, bck_s, col_s);
    // the jump: the first back batch's parameters go in flight while the front images leave
    stage_load<CDIM>(st, gb0, means2d, conics, colors, opacities);
    st.g_next = (lb + B + lane < range_end) ? sc_safe_id(flatten_ids[lb + B + lane], NS) : -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float a_k = 1.0f - T_of(k);
        if (EPILOGUE == 0) {
            if (!inside[k]) continue;
            const int64_t pix = pix0 + k;
            o1[pix] = a_k;
            if (CDIM == 4) {
                *reinterpret_cast<float4*>(o0 + pix * 4) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
            } else {
#pragma unroll
                for (int d = 0; d < 3; ++d) o0[pix * 3 + d] = acc[k][d];
            }
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d) park_s[EPILOGUE ? k * 4 + d : 0][lane] = clamp01(acc[k][d]);
            park_s[EPILOGUE ? k * 4 + 3 : 0][lane] = __fsub_rn(1.0f, a_k);
            if (EPILOGUE == 1 && inside[k]) {
                o1[pix0 + k] = a_k;
                // expected depth as sc_rasterize_fwd_ed writes it: one IEEE divide
                if (CDIM == 4 && o2) o2[pix0 + k] = acc[k][3] / fmaxf(a_k, 1e-10f);
            }
        }
    }

    // ---- phase 2: the back layer ------------------------------------------------------------------------------------
    // (the pixel coordinates are derived again from a copy of the lane id the compiler cannot trace: it would otherwise
    //  carry four registers of them through phase 1's loop, and with them one occupancy step)
    int lane2 = lane;
    asm volatile("" : "+v"(lane2));
    reset(txi * 16 + 4 * (lane2 & 3));
    blend_range<CDIM, 3>(st, lb, range_end, means2d, conics, colors, opacities, NS, flatten_ids, rx0, rx1, ry0, ry1, py,
                         pxp, T2, acc, xyoa_s, bck_s, col_s);

    if (EPILOGUE == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!inside[k]) continue;
            const int64_t pix = pix0 + k;
            o3[pix] = 1.0f - T_of(k);
#pragma unroll
            for (int d = 0; d < 3; ++d) o2[pix * 3 + d] = acc[k][d];
        }
        return;
    }
    float fr[4][3], keep[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        keep[k] = park_s[EPILOGUE ? k * 4 + 3 : 0][lane];
#pragma unroll
        for (int d = 0; d < 3; ++d) fr[k][d] = park_s[EPILOGUE ? k * 4 + d : 0][lane];
    }
    // a lane's four pixels are 12 consecutive values; whole and aligned when the width is a multiple of 4
    const bool whole = inside[3] && (width & 3) == 0;
    if (EPILOGUE == 1) {
        float v[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int d = 0; d < 3; ++d) v[k][d] = composite_torch(fr[k][d], clamp01(acc[k][d]), keep[k]);
        float* dst = o0 + pix0 * 3;
        if (whole) {
            float4* d4 = reinterpret_cast<float4*>(dst);
            d4[0] = make_float4(v[0][0], v[0][1], v[0][2], v[1][0]);
            d4[1] = make_float4(v[1][1], v[1][2], v[2][0], v[2][1]);
            d4[2] = make_float4(v[2][2], v[3][0], v[3][1], v[3][2]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!inside[k]) continue;
#pragma unroll
                for (int d = 0; d < 3; ++d) dst[k * 3 + d] = v[k][d];
            }
        }
    } else {
        const float bias = rounding ? 0.5f : 0.0f;
        unsigned q[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int d = 0; d < 3; ++d) q[k][d] = composite_u8(fr[k][d], clamp01(acc[k][d]), keep[k], bias);
        uint8_t* dst = o_u8 + pix0 * 3;
        if (whole) {
            uint32_t* d1 = reinterpret_cast<uint32_t*>(dst);
            d1[0] = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[1][0] << 24);
            d1[1] = q[1][1] | (q[1][2] << 8) | (q[2][0] << 16) | (q[2][1] << 24);
            d1[2] = q[2][2] | (q[3][0] << 8) | (q[3][1] << 16) | (q[3][2] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!inside[k]) continue;
#pragma unroll
                for (int d = 0; d < 3; ++d) dst[k * 3 + d] = (uint8_t)q[k][d];
            }
        }
    }
}

}  // namespace

extern "C" int sc_rasterize_fwd_layers(const float* means2d, const float* conics, const float* colors,
                                       const float* opacities, int C, int N, int D, int n_front, int width, int height,
                                       int tile_size, int tile_width, int tile_height, const int32_t* isect_offsets,
                                       const int32_t* flatten_ids, int64_t n_isects, int epilogue, int rounding,
                                       float* out0, float* out1, float* out2, float* out3, uint8_t* out_u8,
                                       int32_t* layer_begin, sc_stream_t stream) {
    if (C < 0 || N < 0 || width <= 0 || height <= 0 || tile_width <= 0 || tile_height <= 0) return SC_EINVAL;
    if (D != 3 && D != 4) return SC_EINVAL;
    if (tile_size != 16) return SC_EINVAL;
    if (n_front < 0 || n_front > N) return SC_EINVAL;
    if (epilogue < 0 || epilogue > 2 || (rounding != 0 && rounding != 1)) return SC_EINVAL;
    // (the walk computes positions up to three batches past a list's end in 32 bits)
    if (n_isects < 0 || n_isects > 0x7fffffffLL - 256 || (int64_t)C * N > 0x7fffffffLL) return SC_EINVAL;
    if ((int64_t)C * tile_width * tile_height >= (1 << 29)) return SC_EINVAL;
    if ((int64_t)tile_width * 16 < width || (int64_t)tile_height * 16 < height) return SC_EINVAL;
    if (C == 0) return SC_OK;             // no pixel to write
    if (!isect_offsets) return SC_EINVAL;
    if (epilogue == 0 && (!out0 || !out1 || !out2 || !out3)) return SC_EINVAL;
    if (epilogue == 1 && (!out0 || !out1)) return SC_EINVAL;
    if (epilogue == 2 && !out_u8) return SC_EINVAL;
    if (n_isects > 0 && (!means2d || !conics || !colors || !opacities || !flatten_ids)) return SC_EINVAL;
    const int total_tiles = C * tile_width * tile_height;
#define SC_LAUNCH_LAYERS(CD, EP)                                                                                    \
    hipLaunchKernelGGL((raster_layers_kernel<CD, EP>), dim3(total_tiles), dim3(64), 0, sc_s(stream), means2d, conics, \
                       colors, opacities, N, C * N, n_front, width, height, tile_width, tile_height, total_tiles,   \
                       isect_offsets, flatten_ids, (int)n_isects, out0, out1, out2, out3, out_u8, rounding, layer_begin)
    if (D == 4) {
        if (epilogue == 0) SC_LAUNCH_LAYERS(4, 0); else if (epilogue == 1) SC_LAUNCH_LAYERS(4, 1); else SC_LAUNCH_LAYERS(4, 2);
    } else {
        if (epilogue == 0) SC_LAUNCH_LAYERS(3, 0); else if (epilogue == 1) SC_LAUNCH_LAYERS(3, 1); else SC_LAUNCH_LAYERS(3, 2);
    }
#undef SC_LAUNCH_LAYERS
    SC_LAUNCH_CHECK();
    return SC_OK;
}
