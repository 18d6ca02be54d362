// Unit-test hook for the exact tile cull (raster_common.h: splat_misses_rect) and the lane-to-pixel map of the tile walk
// (raster_walk.h: ScLanePixels, sc_pair_alpha): one wave per record, through the helpers the rasterizers compile.
#include "raster_walk.h"

// What it covers: the walk as raster_item, raster_groups_kernel and raster_layers_kernel run it -- MARK_X / +inf x centres
// for pixels outside the image, and therefore the GUARD_A2 = true form of sc_cull_compact (sc_guard_a2 is applied here the
// way it is there).  An instantiation of the walk with GUARD_A2 = false is not what the probe evaluates.
// Bits: 16 * row + column of the rectangle, 256 for a whole tile; with NSUB 2 only the first 128 can be set (rows 0..7).
// Lanes own disjoint bits of a word; the LDS atomicOr merges them without a second pass.
namespace {

// rec = (a, b, c, op, mx, my); the wave plays tile t, half `sub`.  Returns the cull's verdict; every lane ORs the bits of
// the pixels the pair evaluation calls valid into bits_s (bit 16 * row + column of the rectangle).
template <int NSUB>
__device__ __forceinline__ int probe_tile(const float* rec, const ScTileId& t, int sub, int width, int height, int lane,
                                          unsigned* bits_s) {
    typedef ScLanePixels<NSUB> LP;
    const LP lp(t, sub, lane, width, height);
    const ScRect r = lp.rect(t, sub, width, height);
    const float a = rec[0], b = rec[1], c = rec[2], op = rec[3], mx = rec[4], my = rec[5];
    const bool miss = splat_misses_rect(a, b, c, op, r.x0 - mx, r.x1 - mx, r.y0 - my, r.y1 - my);
    const ScSplat sp = sc_prescale(mx, my, a, b, c, op);
    const float dy = sp.my - lp.py;
    const float bdy = sc_row_b(sp.B2, dy), qdy = sc_row_q(sp.C2, dy);
    const int row = lp.py_i - (t.tyi * 16 + sub * LP::ROWS), col0 = lp.px0_i - t.txi * 16;
#pragma unroll
    for (int p = 0; p < LP::NP; ++p) {
        const ScPairAlpha pa = sc_pair_alpha(sp.mx, sc_guard_a2(sp.A2), sp.lop, bdy, qdy,
                                             lp.x_pair(p, lp.px0_i, __builtin_huge_valf()));
        const int bit = row * 16 + col0 + 2 * p;
        if (pa.v0 && (unsigned)bit < 256u) atomicOr(&bits_s[bit >> 5], 1u << (bit & 31));
        if (pa.v1 && (unsigned)(bit + 1) < 256u) atomicOr(&bits_s[(bit + 1) >> 5], 1u << ((bit + 1) & 31));
    }
    return miss ? 1 : 0;
}

__global__ __launch_bounds__(64) void test_tile_cull_kernel(const float* __restrict__ records,
                                                            const int32_t* __restrict__ geometry,
                                                            int32_t* __restrict__ verdict, uint32_t* __restrict__ valid) {
    __shared__ unsigned bits_s[8];
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (lane < 8) bits_s[lane] = 0u;
    __syncthreads();
    const int32_t* g = geometry + i * 6;
    const int txi = g[0], tyi = g[1], sub = g[2], nsub = g[3], width = g[4], height = g[5];
    // the wave's first pixel must be a pixel of the image (all of this is wave-uniform)
    const bool ok = (nsub == 1 || nsub == 2) && sub >= 0 && sub < nsub && width > 0 && height > 0 && txi >= 0 && tyi >= 0 &&
                    (int64_t)txi * 16 < width && (int64_t)tyi * 16 + sub * (16 / nsub) < height;
    int v = -1;
    if (ok) {
        ScTileId t;
        t.cam = 0; t.txi = txi; t.tyi = tyi;
        v = nsub == 1 ? probe_tile<1>(records + i * 6, t, sub, width, height, lane, bits_s)
                      : probe_tile<2>(records + i * 6, t, sub, width, height, lane, bits_s);
    }
    __syncthreads();
    if (lane < 8) valid[i * 8 + lane] = bits_s[lane];
    if (lane == 0) verdict[i] = v;
}

}  // namespace

extern "C" int sc_test_tile_cull(const float* records, const int32_t* geometry, int n, int32_t* verdict, uint32_t* valid,
                                 sc_stream_t stream) {
    if (n < 0) return SC_EINVAL;
    if (n == 0) return SC_OK;
    if (!records || !geometry || !verdict || !valid) return SC_EINVAL;
    hipLaunchKernelGGL(test_tile_cull_kernel, dim3(n), dim3(64), 0, sc_s(stream), records, geometry, verdict, valid);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
