// Constants and the pinned pair arithmetic shared by the rasterizer kernels; the tile walk built
// on them is raster_walk.h.
#pragma once
#include "sc_common.h"

#define SC_ALPHA_MIN (1.0f / 255.0f)
#define SC_ALPHA_MAX 0.999f
#define SC_T_EPS 1e-4f
#define SC_MAX_CDIM 32
#define SC_LOG2E 1.4426950408889634f
#define SC_HALF_LOG2E 0.7213475204444817f

// The pair evaluation.  The blend loop is VALU-bound (rocprof: the VALU is busy ~80 % of the
// kernel), so the per-pixel work is folded as far as the algebra allows:
//     alpha = min(0.999, op * exp(-sigma)),  sigma = 0.5 (a dx^2 + c dy^2) + b dx dy
//           = min(0.999, exp2(log2(op) - sigma2)),
//     sigma2 = sigma * log2(e) = (A2 dx + B2 dy) dx + (C2 dy) dy,   A2 = a log2(e)/2, B2 = b log2(e),
//                                                                 C2 = c log2(e)/2
// A2/B2/C2/log2(op) are computed once per staged splat; (B2 dy) and (C2 dy) dy once per lane row.
// Every rounding point is pinned with explicit mul/fma intrinsics, so every forward variant and the
// backward replay compute bit-identical sigma2 / alpha / transmittance and always take the same
// skip / terminate decisions (no compiler-chosen contraction).  Relative to the literal formula
// alpha moves by ~2e-6 (relative); pixels stay within the 1e-4 bar of the parity tests.
// Degenerate and non-finite records follow the literal reading of the operator's semantics (the reference
// delegates to gsplat's rasterize_to_pixels and holds no kernel of its own), `if (sigma < 0 || alpha < 1/255) continue`
// with alpha = min(0.999, op * exp(-sigma)), IEEE comparisons and a min() that returns its other operand on NaN (fminf):
//   opacity <= 0 (-inf included): alpha <= 0, skipped.  log2 of a negative number is NaN, so sc_prescale maps a negative
//                 opacity to log2 = -inf, like 0;
//   NaN opacity, NaN sigma (a NaN conic entry or centre), opacity +inf: both comparisons are false and alpha is 0.999 --
//                 the record BLENDS at 0.999 into every pixel of the tiles that list it;
//   an infinite centre: inf - inf or 0 * inf in any order of evaluation; in this one, with b = 0, an infinite x gives
//                 sigma = +inf (skipped) and an infinite y gives 0 * inf = NaN (blends).  All kernels agree bit for bit.
// Nothing is filtered: keeping such rows out of the lists is the caller's business (tests/test_raster_edges_gpu.py).
struct ScSplat { float mx, my, A2, B2, C2, lop; };
typedef float sc_f2 __attribute__((ext_vector_type(2)));      // pixel pairs for the packed-fp32 VALU ops

__device__ __forceinline__ ScSplat sc_prescale(float mx, float my, float a, float b, float c, float op) {
    ScSplat s;
    s.mx = mx; s.my = my;
    s.A2 = __fmul_rn(a, SC_HALF_LOG2E);
    s.B2 = __fmul_rn(b, SC_LOG2E);
    s.C2 = __fmul_rn(c, SC_HALF_LOG2E);
    s.lop = op < 0.f ? -__builtin_huge_valf() : __log2f(op);
    return s;
}
// per-lane-row terms, shared by the pixels of one row
__device__ __forceinline__ float sc_row_b(float B2, float dy) { return __fmul_rn(B2, dy); }
__device__ __forceinline__ float sc_row_q(float C2, float dy) { return __fmul_rn(__fmul_rn(C2, dy), dy); }
__device__ __forceinline__ float sc_sigma2(float A2, float bdy, float q, float dx) {
    return __fmaf_rn(__fmaf_rn(A2, dx, bdy), dx, q);
}
__device__ __forceinline__ float sc_alpha2(float lop, float sigma2) {
    return fminf(SC_ALPHA_MAX, __builtin_amdgcn_exp2f(__fsub_rn(lop, sigma2)));
}
__device__ __forceinline__ bool sc_valid(float sigma2, float alpha) {
    return !(sigma2 < 0.f) && (alpha >= SC_ALPHA_MIN);
}
__device__ __forceinline__ float sc_next_T(float T, float alpha) { return __fmaf_rn(-alpha, T, T); }

// flatten_ids come from the caller (or, in diagnostic runs, from skipped passes): an out-of-range id
// must never become an out-of-bounds gather.  Returns -1 for ids outside [0, n_splats).
__device__ __forceinline__ int sc_safe_id(int g, int n_splats) {
    return ((unsigned)g < (unsigned)n_splats) ? g : -1;
}

// isect_offsets come from the caller too: a tile's [start, end) is clamped into [0, n_isects], so
// corrupt offsets (negative, past the end, decreasing) can shorten or empty a tile's list but never
// turn into an out-of-bounds read of flatten_ids.
__device__ __forceinline__ void sc_tile_range(const int32_t* __restrict__ isect_offsets, int tflat,
                                              int total_tiles, int n_isects, int& range_start, int& range_end) {
    const int s = isect_offsets[tflat];
    const int e = (tflat + 1 < total_tiles) ? isect_offsets[tflat + 1] : n_isects;
    range_start = min(max(s, 0), n_isects);
    range_end = min(max(e, range_start), n_isects);
}

// ---- exact tile-level cull, shared by forward and backward ------------------------------------
// Minimum of q(x,y) = 0.5*(A x^2 + C y^2) + B x y  over the rectangle [x0,x1] x [y0,y1]
// (coordinates relative to the splat centre).  q is a convex quadratic when the conic is
// positive definite; returns 0 if the centre is inside.
__device__ __forceinline__ float min_quad_on_rect(float A, float Bc, float Cc, float x0, float x1,
                                                  float y0, float y1) {
    if (x0 <= 0.f && x1 >= 0.f && y0 <= 0.f && y1 >= 0.f) return 0.f;
    float best = 3.0e38f;
    // vertical edges x = xe: minimise over y -> y* = -B xe / C clamped
    const float invC = 1.0f / Cc, invA = 1.0f / A;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float xe = e ? x1 : x0;
        float ys = fminf(fmaxf(-Bc * xe * invC, y0), y1);
        best = fminf(best, 0.5f * (A * xe * xe + Cc * ys * ys) + Bc * xe * ys);
        const float ye = e ? y1 : y0;
        float xs = fminf(fmaxf(-Bc * ye * invA, x0), x1);
        best = fminf(best, 0.5f * (A * xs * xs + Cc * ye * ye) + Bc * xs * ye);
    }
    return best;
}

// True only when NO pixel centre inside the rectangle can pass the blend loop's test
// (sigma >= 0 and op*exp(-sigma) >= 1/255, i.e. sigma <= ln(255 op)).  Conservative: the
// threshold is widened by an absolute margin plus a bound on the fp32 rounding error of both
// evaluations of the quadratic (2e-6 * the largest magnitude its terms reach on the rectangle);
// NaN inputs and non positive-definite conics are never dropped (every comparison is false).
__device__ __forceinline__ bool splat_misses_rect(float A, float Bc, float Cc, float op, float x0,
                                                  float x1, float y0, float y1) {
    const float L = __logf(255.0f * op);
    if (L + 1e-3f + 1e-3f * fabsf(L) < 0.f) return true;   // op*255 < 1: alpha < 1/255 everywhere
    const bool pd = (A > 0.f) && (Cc > 0.f) && (A * Cc - Bc * Bc > 0.f);
    if (!pd) return false;
    const float mx = fmaxf(fabsf(x0), fabsf(x1)), my = fmaxf(fabsf(y0), fabsf(y1));
    const float S = A * mx * mx + Cc * my * my + 2.0f * fabsf(Bc) * mx * my;
    const float tau = L + 1e-3f + 1e-3f * fabsf(L) + 2e-6f * S;
    return min_quad_on_rect(A, Bc, Cc, x0, x1, y0, y1) > tau;
}

// ---- the transposing wave reduction of the backward kernels (raster_bwd.hip, raster_groups_bwd.hip) ----------------
// lanes 0..31 get a(l) + a(l + 32), lanes 32..63 get b(l - 32) + b(l)
__device__ __forceinline__ float swap32_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// even rows get a(l) + a(l + 16), odd rows get b(l - 16) + b(l)   (row = 16 lanes)
__device__ __forceinline__ float swap16_add(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// 16 per-lane partial sums in, one register out: lane l holds the 64-lane total of v[l >> 2].
// Lane pairings per stage: l^32, l^16, l^15 (row_mirror), l^7 (row_half_mirror), l^2, l^1 - six
// independent masks, so every lane's contribution reaches the owner of each sum exactly once.
__device__ __forceinline__ float wave_transpose_sum16(const float (&v)[16], int lane) {
    float w[8], x[4], y[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = swap32_add(v[i], v[i + 8]);       // lane bit 5 picks +8
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = swap16_add(w[i], w[i + 4]);       // lane bit 4 picks +4
    const bool b3 = (lane & 8) != 0, b2 = (lane & 4) != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {                                         // lane bit 3 picks +2
        const float keep = b3 ? x[i + 2] : x[i], give = b3 ? x[i] : x[i + 2];
        y[i] = keep + dpp_move<0x140>(give);                              // row_mirror
    }
    const float keep = b2 ? y[1] : y[0], give = b2 ? y[0] : y[1];       // lane bit 2 picks +1
    float z = keep + dpp_move<0x141>(give);                               // row_half_mirror
    z += dpp_move<0x4E>(z);                                               // quad_perm [2,3,0,1]
    z += dpp_move<0xB1>(z);                                               // quad_perm [1,0,3,2]
    return z;
}

// ---- grouped rasterizer (raster_groups.hip, raster_groups_bwd.hip) -----------------------------------------------
#define SC_GROUP_NONE 255           // group id of a record that belongs to no group
// argument checks shared by the entry points of raster_groups.hip and raster_groups_bwd.hip; > 0: nothing to do, return SC_OK
static inline int sc_groups_check(int C, int N, int n_groups, int tile_width, int tile_height, int64_t n_isects) {
    if (n_groups < 1 || n_groups > 2) return SC_EINVAL;
    if (C < 0 || N < 0 || tile_width <= 0 || tile_height <= 0) return SC_EINVAL;
    if (n_isects < 0 || n_isects > 0x7fffffffLL) return SC_EINVAL;
    if ((int64_t)C * N > 0x7fffffffLL) return SC_EINVAL;
    if ((int64_t)C * tile_width * tile_height >= (1 << 29)) return SC_EINVAL;
    return C == 0 ? 1 : SC_OK;
}


extern int g_sc_raster_bwd_variant;  // sc_set_option "raster_bwd"
extern int g_sc_raster_bwd_split;    // sc_set_option "raster_bwd_split"
extern "C" int sc_tile_order_len(int total_tiles);     // raster_fwd.hip
int sc_tile_order_fwd_items(int total_tiles);          // raster_fwd.hip
extern int g_sc_raster_map;          // sc_set_option "raster_map"
extern int g_sc_raster_fwd_variant;  // see include/street_crafter_amd.h (sc_set_option "raster_fwd")
