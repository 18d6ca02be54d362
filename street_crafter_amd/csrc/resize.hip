// Crop + separable resize of the novel-view training inputs (include/street_crafter_amd.h, sc_resize_*): what
// DiffusionRunner.preprocess_tensor (street_gaussian/utils/diffusion_utils.py:99-115) and the row slice of
// train.py:164-169 do to the render and its mask, as one gather per direction.  Three kernels, one launch each:
//
//   forward   a wave owns 64 adjacent output columns of one output row (one 256-byte store per channel); the four waves
//             of a workgroup own four adjacent rows, whose input rows overlap (L1).  Every lane walks its own x taps inside
//             the wave's y taps, straight from the strided input: the input is read about once and a tap's neighbours
//             sit in the same cache lines, so nothing is staged through LDS.  With the rasterizer's [H,W,4] layout the
//             channels of a tap are one 16-byte load.  Rows above row_begin are never computed.
//   mask      the same walk over bytes: an output is set iff any tap of the two tables is (zero-weight taps are not in
//             the tables, so this is `interpolated value != 0`).
//   backward  the transpose as a gather: a lane owns one INPUT element and walks the contiguous run of outputs that read
//             it (the transposed tables).  Every element of the gradient has one writer, inside the crop or not: no
//             memset, no atomics, a fixed sum order.
//
// The tap tables are device arrays (start[n], offset[n+1], weights), of any length per entry: the kernels loop over the
// counts.  Indices read through a table are clamped to the image, so a wrong table gives wrong numbers, not a fault.
#include "sc_common.h"

namespace {

constexpr int RS_ROWS = 4;                           // waves (rows) of a workgroup
constexpr int RS_THREADS = RS_ROWS * SC_WAVE;

struct Axis {                                        // one tap table: idx = start[n] | offset[n+1]
    const int32_t* idx;
    const float* w;
    int n;
};

struct Entry {
    int start, first, count;                         // first index of the entry, its first weight, its taps
};

__device__ __forceinline__ Entry entry_of(const Axis& t, int i) {
    Entry e;
    e.start = t.idx[i];
    e.first = t.idx[t.n + i];
    e.count = t.idx[t.n + i + 1] - e.first;
    return e;
}

struct FwdArgs {
    int64_t sb, sc, sh, sw;                          // element strides of x: batch, channel, row, column
    Axis ty, tx;
    int channels, in_h, in_w, h_out, w_out, row_begin, affine;
    float a, b;
};

// The wave's row (uniform across its lanes; said so to the compiler, which then keeps the y table in scalar registers).
__device__ __forceinline__ int wave_row() {
    return __builtin_amdgcn_readfirstlane((int)(blockIdx.y * RS_ROWS + (threadIdx.x >> 6)));
}

template <bool PACKED>
__global__ __launch_bounds__(RS_THREADS) void resize_fwd_kernel(const FwdArgs g, const float* __restrict__ x,
                                                                float* __restrict__ out) {
    const int ox = (int)blockIdx.x * SC_WAVE + sc_lane();
    const int r = wave_row(), rows = g.h_out - g.row_begin;
    if (r >= rows || ox >= g.w_out) return;
    const int z = (int)blockIdx.z;                   // PACKED: the batch index; else batch * channels + channel
    const Entry ey = entry_of(g.ty, r + g.row_begin), ex = entry_of(g.tx, ox);
    const int64_t plane = (int64_t)rows * g.w_out, at = (int64_t)r * g.w_out + ox;
    if (PACKED) {
        const float* __restrict__ img = x + z * g.sb;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int jy = 0; jy < ey.count; ++jy) {
            const float* __restrict__ row = img + (int64_t)min(ey.start + jy, g.in_h - 1) * g.sh;
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int jx = 0; jx < ex.count; ++jx) {
                const float4 v = *reinterpret_cast<const float4*>(row + (int64_t)min(ex.start + jx, g.in_w - 1) * 4);
                const float w = g.tx.w[ex.first + jx];
                s[0] = fmaf(w, v.x, s[0]);
                s[1] = fmaf(w, v.y, s[1]);
                s[2] = fmaf(w, v.z, s[2]);
                s[3] = fmaf(w, v.w, s[3]);
            }
            const float wy = g.ty.w[ey.first + jy];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fmaf(wy, s[c], acc[c]);
        }
        float* __restrict__ o = out + (int64_t)z * g.channels * plane + at;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < g.channels) o[c * plane] = g.affine ? fmaf(acc[c], g.a, g.b) : acc[c];
    } else {
        const int b = z / g.channels, c = z - b * g.channels;
        const float* __restrict__ img = x + b * g.sb + c * g.sc;
        float acc = 0.0f;
        for (int jy = 0; jy < ey.count; ++jy) {
            const float* __restrict__ row = img + (int64_t)min(ey.start + jy, g.in_h - 1) * g.sh;
            float s = 0.0f;
            for (int jx = 0; jx < ex.count; ++jx)
                s = fmaf(g.tx.w[ex.first + jx], row[(int64_t)min(ex.start + jx, g.in_w - 1) * g.sw], s);
            acc = fmaf(g.ty.w[ey.first + jy], s, acc);
        }
        out[(int64_t)z * plane + at] = g.affine ? fmaf(acc, g.a, g.b) : acc;
    }
}

__global__ __launch_bounds__(RS_THREADS) void resize_mask_kernel(const FwdArgs g, const uint8_t* __restrict__ x,
                                                                 uint8_t* __restrict__ out) {
    const int ox = (int)blockIdx.x * SC_WAVE + sc_lane();
    const int r = wave_row(), rows = g.h_out - g.row_begin;
    if (r >= rows || ox >= g.w_out) return;
    const int z = (int)blockIdx.z;
    const Entry ey = entry_of(g.ty, r + g.row_begin), ex = entry_of(g.tx, ox);
    const int b = z / g.channels, c = z - b * g.channels;
    const uint8_t* __restrict__ img = x + b * g.sb + c * g.sc;
    unsigned any = 0;
    for (int jy = 0; jy < ey.count; ++jy) {
        const uint8_t* __restrict__ row = img + (int64_t)min(ey.start + jy, g.in_h - 1) * g.sh;
        for (int jx = 0; jx < ex.count; ++jx) any |= row[(int64_t)min(ex.start + jx, g.in_w - 1) * g.sw];
    }
    out[((int64_t)z * rows + r) * g.w_out + ox] = any ? 1 : 0;
}

struct BwdArgs {
    Axis uy, ux;                                     // transposed tables: one entry per cropped input row / column
    int height, width, top, left, in_h, in_w, h_out, w_out, row_begin, affine;
    float a;
};

__global__ __launch_bounds__(RS_THREADS) void resize_bwd_kernel(const BwdArgs g, const float* __restrict__ grad_out,
                                                                float* __restrict__ grad_x) {
    const int xi = (int)blockIdx.x * SC_WAVE + sc_lane();
    const int yi = wave_row();
    if (yi >= g.height || xi >= g.width) return;
    const int z = (int)blockIdx.z;
    const int iy = yi - g.top, ix = xi - g.left;
    float res = 0.0f;
    if (iy >= 0 && iy < g.in_h && ix >= 0 && ix < g.in_w) {
        const Entry ey = entry_of(g.uy, iy), ex = entry_of(g.ux, ix);
        const int rows = g.h_out - g.row_begin;
        const float* __restrict__ gp = grad_out + (int64_t)z * rows * g.w_out;
        float acc = 0.0f;
        bool any = false;
        for (int jy = 0; jy < ey.count; ++jy) {
            const int oy = min(ey.start + jy, g.h_out - 1);
            if (oy < g.row_begin) continue;
            const float* __restrict__ row = gp + (int64_t)(oy - g.row_begin) * g.w_out;
            float s = 0.0f;
            for (int jx = 0; jx < ex.count; ++jx)
                s = fmaf(g.ux.w[ex.first + jx], row[min(ex.start + jx, g.w_out - 1)], s);
            acc = fmaf(g.uy.w[ey.first + jy], s, acc);
            any = ex.count > 0;
        }
        if (any) res = g.affine ? g.a * acc : acc;   // (no contributing output: +0 whatever the sign of a)
    }
    grad_x[((int64_t)z * g.height + yi) * g.width + xi] = res;
}

inline dim3 grid_of(int width, int rows, int planes) {
    return dim3((unsigned)((width + SC_WAVE - 1) / SC_WAVE), (unsigned)((rows + RS_ROWS - 1) / RS_ROWS), (unsigned)planes);
}

}  // namespace

// Arguments are checked by the callers in capi.hip.
int sc_resize_fwd_run(const float* x, const uint8_t* x_mask, const int64_t* strides, int batch, int channels, int in_h,
                      int in_w, const int32_t* ty_idx, const float* ty_w, const int32_t* tx_idx, const float* tx_w,
                      int h_out, int w_out, int row_begin, int flags, float a, float b, float* out, uint8_t* out_mask,
                      sc_stream_t stream) {
    FwdArgs g;
    g.sb = strides[0]; g.sc = strides[1]; g.sh = strides[2]; g.sw = strides[3];
    g.ty = Axis{ty_idx, ty_w, h_out};
    g.tx = Axis{tx_idx, tx_w, w_out};
    g.channels = channels; g.in_h = in_h; g.in_w = in_w; g.h_out = h_out; g.w_out = w_out; g.row_begin = row_begin;
    g.affine = (flags & SC_RESIZE_AFFINE) != 0;
    g.a = a; g.b = b;
    const int rows = h_out - row_begin;
    if (x_mask) {
        hipLaunchKernelGGL(resize_mask_kernel, grid_of(w_out, rows, batch * channels), dim3(RS_THREADS), 0, sc_s(stream), g,
                           x_mask, out_mask);
    } else if (flags & SC_RESIZE_PACKED4) {
        hipLaunchKernelGGL(resize_fwd_kernel<true>, grid_of(w_out, rows, batch), dim3(RS_THREADS), 0, sc_s(stream), g, x,
                           out);
    } else {
        hipLaunchKernelGGL(resize_fwd_kernel<false>, grid_of(w_out, rows, batch * channels), dim3(RS_THREADS), 0,
                           sc_s(stream), g, x, out);
    }
    SC_LAUNCH_CHECK();
    return SC_OK;
}

int sc_resize_bwd_run(const float* grad_out, int batch, int channels, int height, int width, int top, int left, int in_h,
                      int in_w, const int32_t* uy_idx, const float* uy_w, const int32_t* ux_idx, const float* ux_w,
                      int h_out, int w_out, int row_begin, int flags, float a, float* grad_x, sc_stream_t stream) {
    BwdArgs g;
    g.uy = Axis{uy_idx, uy_w, in_h};
    g.ux = Axis{ux_idx, ux_w, in_w};
    g.height = height; g.width = width; g.top = top; g.left = left; g.in_h = in_h; g.in_w = in_w;
    g.h_out = h_out; g.w_out = w_out; g.row_begin = row_begin;
    g.affine = (flags & SC_RESIZE_AFFINE) != 0;
    g.a = a;
    hipLaunchKernelGGL(resize_bwd_kernel, grid_of(width, height, batch * channels), dim3(RS_THREADS), 0, sc_s(stream), g,
                       grad_out, grad_x);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
