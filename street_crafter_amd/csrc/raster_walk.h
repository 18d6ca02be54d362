// The tile walk of the wave-per-tile rasterizers, one phase per helper: raster_fwd.hip (raster_item), raster_groups.hip
// and raster_layers.hip compile exactly these, which is why group and layer images are bit-identical to their own
// renders; the backward kernels (raster_bwd.hip, raster_groups_bwd.hip) take the tile geometry and the owner map.
// A tile is 16 x 16 pixels, one wave walks it (or its upper / lower half), a lane owns 4 (2) consecutive pixels of a row
// and keeps them in PAIRS (v_pk_add / v_pk_fma / v_pk_mul process two pixels per VALU op).  Per batch:
//   ScStage          the record this lane gathered for the batch, and the id of the one it gathers next
//   sc_cull_compact  exact tile cull, ballot compaction, prescaled records into LDS
//   ScStage::advance the next batch's parameters and the ids after that go in flight
//   sc_walk_batch    the compacted records, one after the other, through the caller's blend
//   sc_pair_alpha, sc_blend_step     the blend of one record into one pixel pair of one accumulator set
#pragma once
#include "raster_common.h"

// Records per batch: ONE per lane.  The walk's second bound, beside VALU issue, is the rate of its parameter gathers (4
// random sectors per list entry: with the blend loop compiled out S-1M's whole lists take 686 us, i.e. ~35 us per million
// entries walked), and a tile that stops after ~250 entries throws away what it staged beyond that
// point: on average half a batch plus the batch in flight.  Against two per lane (batches of 128): S-1M 142 -> 134 us, sky
// 107 -> 100, S-100k 135 -> 132, street scene unchanged; half-wave batches of 32 were measured too: +6 / +30 / +7 us on
// S-1M / street / S-100k (profiles/r03_raster_batch_ab.txt).  The LDS arrays are [SC_WALK_B + 1]: the walk reads t + 1.
constexpr int SC_WALK_B = 64;

// ---- tile geometry ---------------------------------------------------------------------------------------------------
struct ScTileId { int cam, txi, tyi; };
__device__ __forceinline__ ScTileId sc_tile_id(int tflat, int tile_width, int tile_height) {
    const int tiles_per_cam = tile_width * tile_height;
    ScTileId t;
    t.cam = tflat / tiles_per_cam;
    const int tile_id = tflat - t.cam * tiles_per_cam;
    t.tyi = tile_id / tile_width;
    t.txi = tile_id - t.tyi * tile_width;
    return t;
}
// the rectangle of pixel centres of rows [row0, row0 + rows) of a tile (only pixels inside the image count)
struct ScRect { float x0, x1, y0, y1; };
__device__ __forceinline__ ScRect sc_tile_rect(const ScTileId& t, int row0, int rows, int width, int height) {
    ScRect r;
    r.x0 = (float)(t.txi * 16) + 0.5f;
    r.y0 = (float)(t.tyi * 16 + row0) + 0.5f;
    r.x1 = (float)min(t.txi * 16 + 15, width - 1) + 0.5f;
    r.y1 = (float)min(t.tyi * 16 + row0 + rows - 1, height - 1) + 0.5f;
    return r;
}
// lane -> pixels.  NSUB 1: the wave covers the whole tile, 4 pixels per lane; 2: half `sub` (16 x 8), 2 pixels per lane.
template <int NSUB>
struct ScLanePixels {
    static constexpr int NP = NSUB == 1 ? 2 : 1;       // pixel PAIRS per lane
    static constexpr int PPL = 2 * NP;                 // pixels per lane
    static constexpr int LPR = 16 / PPL;               // lanes per row
    static constexpr int ROWS = 16 / NSUB;             // rows of the tile this wave covers
    int px0_i, py_i;                                   // the lane's first pixel
    float py;
    bool inside[PPL];                                  // (monotone along the lane's pixels)
    int64_t pix0;                                      // flat index of the first pixel in a [C, H, W] image
    __device__ __forceinline__ ScLanePixels(const ScTileId& t, int sub, int lane, int width, int height) {
        px0_i = t.txi * 16 + PPL * (lane % LPR);
        py_i = t.tyi * 16 + (sub * ROWS + lane / LPR);
        py = (float)py_i + 0.5f;
#pragma unroll
        for (int k = 0; k < PPL; ++k) inside[k] = (px0_i + k < width) && (py_i < height);
        pix0 = ((int64_t)t.cam * height + py_i) * width + px0_i;
    }
    __device__ __forceinline__ ScRect rect(const ScTileId& t, int sub, int width, int height) const {
        return sc_tile_rect(t, sub * ROWS, ROWS, width, height);
    }
    // x centres of pixel pair p counted from first pixel `px0`; a pixel outside the image gets `off` (+inf: finished)
    __device__ __forceinline__ sc_f2 x_pair(int p, int px0, float off) const {
        return sc_f2{inside[2 * p] ? (float)(px0 + 2 * p) + 0.5f : off,
                     inside[2 * p + 1] ? (float)(px0 + 2 * p + 1) + 0.5f : off};
    }
};

// ---- the register-staged record ----------------------------------------------------------------------------------------
// One batch of the pipeline: the parameters of the record this lane stages (position batch_start + lane) and the id of
// the one after (batch_start + 64 + lane).  PACKED: `means2d` points to one 48-B record per Gaussian, (x, y, conic a, b |
// conic c, opacity, colour 0, 1 | colour 2, 3, -, -), written by projection_sh_fwd_kernel for the fused forward: one
// gather line per splat instead of four.
struct ScSplatArrays { const float* means2d; const float* conics; const float* colors; const float* opacities; };
struct ScNoExtra { __device__ __forceinline__ void operator()(int) const {} };

template <int CDIM, bool PACKED = false>
struct ScStage {
    float2 xy;
    float a, b, c, op;
    float4 col;
    bool live;
    int g_next;
    __device__ __forceinline__ void clear() {
        xy = make_float2(0.f, 0.f);
        a = b = c = op = 0.f;
        col = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // the record of flat id g (< 0: none, the parameters keep their values); `extra(g)` gathers what else the caller stages
    template <class Extra = ScNoExtra>
    __device__ __forceinline__ void load(int g, const ScSplatArrays& in, Extra&& extra = Extra()) {
        live = g >= 0;
        if (!live) return;
        if (PACKED) {
            const float4* rec = reinterpret_cast<const float4*>(in.means2d) + (int64_t)g * 3;
            const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
            xy = make_float2(q0.x, q0.y);
            a = q0.z; b = q0.w; c = q1.x;
            op = q1.y;
            col = make_float4(q1.z, q1.w, q2.x, CDIM > 3 ? q2.y : 0.f);
            return;
        }
        xy = *reinterpret_cast<const float2*>(in.means2d + (int64_t)g * 2);
        const float* cn = in.conics + (int64_t)g * 3;
        a = cn[0]; b = cn[1]; c = cn[2];
        op = in.opacities[g];
        const float* cl = in.colors + (int64_t)g * CDIM;
        col = make_float4(cl[0], cl[1], cl[2], CDIM > 3 ? cl[3] : 0.f);
        extra(g);
    }
    // the id at list position idx if idx < end (flatten_ids come from the caller: sc_safe_id)
    static __device__ __forceinline__ int id_at(const int32_t* __restrict__ flatten_ids, int idx, int end, int n_splats) {
        return (idx < end) ? sc_safe_id(flatten_ids[idx], n_splats) : -1;
    }
    // next batch's parameters and the id after that (position idx2, two batches ahead, bounded by `end`) go in flight
    template <class Extra = ScNoExtra>
    __device__ __forceinline__ void advance(const ScSplatArrays& in, const int32_t* __restrict__ flatten_ids, int idx2,
                                            int end, int n_splats, Extra&& extra = Extra()) {
        load(g_next, in, extra);
        g_next = id_at(flatten_ids, idx2, end, n_splats);
    }
};

// ---- cull + compact ----------------------------------------------------------------------------------------------------
// Exact tile-level cull of the staged records (wave-level: the workgroup is this wave), ballot compaction, and the
// prescaled record into LDS: xyoa_s = (mx, my, log2 op, B2), bck_s = (A2, C2, w2, w3), col_s = colour.  mx, lop and A2 are
// broadcast to pixel PAIRS: they sit in even slots, the low half of a register pair, which is what v_pk_* can broadcast
// without a move.  w2 / w3 are the caller's (sorted index, group id, list position, as int bits); `open()` is a further
// reason to keep a live record (groups: its sets are not all finished).  Returns the number of records kept.
// GUARD_A2: an exactly-zero A2 is replaced by 1e-37f.  Needed exactly where a finished pixel is marked by +inf in x
// (sc_blend_step, MARK_X), and nowhere else: there dx = -inf and A2 == 0 would make 0 * inf = NaN of sigma2 instead of
// +inf; no finite pixel can see 1e-37 (1e-37 * dx^2 is absorbed by every other term).
__device__ __forceinline__ float sc_guard_a2(float A2) { return A2 == 0.f ? 1e-37f : A2; }
struct ScAlwaysOpen { __device__ __forceinline__ bool operator()() const { return true; } };
template <bool GUARD_A2, class Stage, class Open = ScAlwaysOpen>
__device__ __forceinline__ int sc_cull_compact(const Stage& st, const ScRect& r, float w2, float w3, float4* xyoa_s,
                                               float4* bck_s, float4* col_s, Open&& open = Open()) {
    __syncthreads();   // single-wave workgroup: orders the previous batch's LDS reads vs these writes
    bool keep = false;
    if (st.live)
        keep = open() && !splat_misses_rect(st.a, st.b, st.c, st.op, r.x0 - st.xy.x, r.x1 - st.xy.x, r.y0 - st.xy.y,
                                            r.y1 - st.xy.y);
    const unsigned long long m = __ballot(keep);
    if (keep) {
        const int slot = __popcll(m & sc_lanemask_lt());
        const ScSplat sp = sc_prescale(st.xy.x, st.xy.y, st.a, st.b, st.c, st.op);
        xyoa_s[slot] = make_float4(sp.mx, sp.my, sp.lop, sp.B2);
        bck_s[slot] = make_float4(GUARD_A2 ? sc_guard_a2(sp.A2) : sp.A2, sp.C2, w2, w3);
        col_s[slot] = st.col;
    }
    __syncthreads();
    return __popcll(m);
}

// ---- pair evaluation and blend step ------------------------------------------------------------------------------------
// The pinned arithmetic of raster_common.h (sc_sigma2, sc_alpha2, sc_valid), two pixels per instruction: sigma2, alpha
// and "this record blends" of the pixel pair with x centres px.  bdy, qdy: sc_row_b, sc_row_q of the lane's row.
struct ScPairAlpha { sc_f2 sg, al; bool v0, v1; };
__device__ __forceinline__ ScPairAlpha sc_pair_alpha(float mx, float A2, float lop, float bdy, float qdy, sc_f2 px) {
    ScPairAlpha r;
    const sc_f2 dx = sc_f2{mx, mx} - px;
    const sc_f2 tt = __builtin_elementwise_fma(sc_f2{A2, A2}, dx, sc_f2{bdy, bdy});
    r.sg = __builtin_elementwise_fma(tt, dx, sc_f2{qdy, qdy});
    const sc_f2 e = sc_f2{lop, lop} - r.sg;
    r.al = sc_f2{fminf(SC_ALPHA_MAX, __builtin_amdgcn_exp2f(e.x)), fminf(SC_ALPHA_MAX, __builtin_amdgcn_exp2f(e.y))};
    r.v0 = sc_valid(r.sg.x, r.al.x);
    r.v1 = sc_valid(r.sg.y, r.al.y);
    return r;
}

// One record (colour c) blended into one pixel pair of one accumulator set: transmittance T, colour sums ac0 / ac1 (ND
// channels).  Returns which of the two pixels the record blended into (what last_ids / last_pos record).  A pixel that
// terminates is marked finished and never blends again, with no per-pixel `done` flag in the loop:
//   MARK_X     +inf into its x centre: dx = -inf, sigma2 = +inf, alpha = exp2(-inf) = 0 < 1/255 (needs GUARD_A2 above);
//   MARK_TSIGN the sign of T (T > 1e-4 while a set is live): a set with T < 0 computes next_T < 0 <= SC_T_EPS, hence
//              "terminate again", an effective alpha of 0, and changes nothing; |T| is what it ends with.  For pixels that
//              carry several sets with their own ends.
// Nothing is skipped: adding c * 0 leaves the sums bit-identical to skipping (sums are never -0).
enum ScMark { MARK_X, MARK_TSIGN };
template <ScMark MARK, int ND, bool TRACK, int W>
__device__ __forceinline__ void sc_blend_step(const sc_f2 al, const bool v0, const bool v1, const float4& c, sc_f2& T,
                                              sc_f2& px, float (&ac0)[W], float (&ac1)[W], int idx, int& last0,
                                              int& last1) {
    const sc_f2 nT = __builtin_elementwise_fma(-al, T, T);
    const bool t0 = v0 && (nT.x <= SC_T_EPS), t1 = v1 && (nT.y <= SC_T_EPS);
    const bool b0 = v0 != t0, b1 = v1 != t1;                    // v && !t (t implies v): one mask xor
    const sc_f2 ae = sc_f2{b0 ? al.x : 0.f, b1 ? al.y : 0.f};   // one select drives vis AND T
    const sc_f2 vis = ae * T;
    T = __builtin_elementwise_fma(-ae, T, T);                   // == nT when blending, else T
    if (MARK == MARK_X) px = sc_f2{t0 ? __builtin_huge_valf() : px.x, t1 ? __builtin_huge_valf() : px.y};
    else T = sc_f2{t0 ? -fabsf(T.x) : T.x, t1 ? -fabsf(T.y) : T.y};
    ac0[0] = __fmaf_rn(c.x, vis.x, ac0[0]);
    ac0[1] = __fmaf_rn(c.y, vis.x, ac0[1]);
    ac0[2] = __fmaf_rn(c.z, vis.x, ac0[2]);
    if constexpr (ND > 3) ac0[3] = __fmaf_rn(c.w, vis.x, ac0[3]);
    ac1[0] = __fmaf_rn(c.x, vis.y, ac1[0]);
    ac1[1] = __fmaf_rn(c.y, vis.y, ac1[1]);
    ac1[2] = __fmaf_rn(c.z, vis.y, ac1[2]);
    if constexpr (ND > 3) ac1[3] = __fmaf_rn(c.w, vis.y, ac1[3]);
    if (TRACK) {
        last0 = b0 ? idx : last0;
        last1 = b1 ? idx : last1;
    }
}
// every pixel of every lane finished (MARK_X).  x centres are positive floats or +inf, so their bit patterns order like
// integers (integer min: no NaN canonicalisation ops)
template <int NP>
__device__ __forceinline__ bool sc_all_marked_x(const sc_f2 (&pxp)[NP]) {
    int m = min(__float_as_int(pxp[0].x), __float_as_int(pxp[0].y));
    if (NP > 1) m = min(m, min(__float_as_int(pxp[NP - 1].x), __float_as_int(pxp[NP - 1].y)));
    return __all(m == 0x7f800000);
}

// ---- the LDS walk ------------------------------------------------------------------------------------------------------
// blend(a, bc, c) on records [0, bsz) of the compacted batch, bsz > 0, until all_done().  Returns the records blended:
// t + 1 on a vote exit, bsz otherwise.
// The next record is read from LDS while the current one blends; two register sets take turns, so that no record is
// copied from "next" to "current" (4 v_mov_b64 of ~66 VALU ops per splat).
// The pin: the scheduler sinks the three LDS reads BELOW the blend of the current record (fewer live registers), which
// puts their latency in front of every iteration (ISA of round 2: ds_read x3 then s_waitcnt lgkmcnt(2) at the loop top).
// Pinning them above costs 10 VGPRs and gives -1 us on S-1M, -2..-6 us on the street scene
// (profiles/r03_raster_prefetch_ab.txt); with batches of 64 every single-image variant fits 86 VGPRs and the training
// forward gains 18 us from the pin (131 -> 113 us, profiles/r03_raster_batch_ab.txt).
// The vote is taken after every SECOND record: a record blended onto finished pixels changes nothing (sc_blend_step), and
// the vote is 3 VALU + 2 SALU ops and a branch.
template <class Blend, class Done>
__device__ __forceinline__ int sc_walk_batch(const float4* xyoa_s, const float4* bck_s, const float4* col_s, int bsz,
                                             Blend&& blend, Done&& all_done) {
    float4 a0 = xyoa_s[0], b0 = bck_s[0], c0 = col_s[0], a1, b1, c1;
    int t = 0, walked = 0;
    for (;;) {
        a1 = xyoa_s[t + 1]; b1 = bck_s[t + 1]; c1 = col_s[t + 1];
        __builtin_amdgcn_sched_barrier(0);
        blend(a0, b0, c0);
        if (++t >= bsz) break;
        a0 = xyoa_s[t + 1]; b0 = bck_s[t + 1]; c0 = col_s[t + 1];
        __builtin_amdgcn_sched_barrier(0);
        blend(a1, b1, c1);
        if (all_done()) { walked += t + 1 - bsz; break; }
        if (++t >= bsz) break;
    }
    return walked + bsz;
}

// ---- interleaved pixel store -------------------------------------------------------------------------------------------
// pixel `pix` of a [.., CDIM] image: one 16-B store for four channels, scalar stores for three
template <int CDIM, int W>
__device__ __forceinline__ void sc_store_pixel(float* __restrict__ out, int64_t pix, const float (&v)[W]) {
    if (CDIM == 4) {
        *reinterpret_cast<float4*>(out + pix * 4) = make_float4(v[0], v[1], v[2], v[W > 3 ? 3 : 0]);
    } else {
#pragma unroll
        for (int d = 0; d < CDIM; ++d) out[pix * CDIM + d] = v[d];
    }
}

// ---- backward: which reduced sum a lane owns ---------------------------------------------------------------------------
// Value index vi of wave_transpose_sum16's output: 0..3 colour channels, 4..6 conic, 7..8 mean, 9..10 |mean| (absgrad;
// nullable), 11 opacity.  The owner adds its total to base[flat id * stride]; base == nullptr: no atomic.
struct ScGradOwner { float* base = nullptr; int stride = 0; };
template <int CDIM>
__device__ __forceinline__ ScGradOwner sc_grad_owner(int vi, float* v_colors, float* v_conics, float* v_means2d,
                                                     float* v_means2d_abs, float* v_opacities) {
    ScGradOwner o;
    if (vi < CDIM) { o.base = v_colors + vi; o.stride = CDIM; }
    else if (vi >= 4 && vi <= 6) { o.base = v_conics + (vi - 4); o.stride = 3; }
    else if (vi == 7 || vi == 8) { o.base = v_means2d + (vi - 7); o.stride = 2; }
    else if ((vi == 9 || vi == 10) && v_means2d_abs) { o.base = v_means2d_abs + (vi - 9); o.stride = 2; }
    else if (vi == 11) { o.base = v_opacities; o.stride = 1; }
    return o;
}
