// Seamless bilinear sampling of a cube texture, forward and backward (include/street_crafter_amd.h, sc_cubemap_fwd/bwd):
// what the reference asks of nvdiffrast.torch.texture(boundary_mode='cube') at street_gaussian/models/sky_cubemap.py:102,
// 120,205, with the rest of SkyCubeMap.forward (sky_cubemap.py:92-127) fused around it: ray generation, the pixel mask,
// the sigmoid of the stored logits, the fill colour, the clamp and the [C,H,W] layout.
//
// One thread per sample.  A sample reads 4 taps of C floats; neighbouring pixels share taps through L2.  The backward
// adds w * g * act' to the four texels with fp32 atomicAdd (one global_atomic_add_f32 each, no compare-and-swap loop),
// after the wave has re-dealt its terms so that an instruction's lanes cover contiguous bytes (cube_wave_adds).
//
// Every product and sum below is a separately rounded fp32 operation (contraction off), so that the float32 replay in
// tests/cubemap_ref.py follows the same formula.
#include "sc_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CUBE_THREADS = 256;

// The face rule, once for the float direction and once for the integer tap centre below.  Faces +x -x +y -y +z -z; the
// major axis is z if |z| > max(|x|,|y|), else y if |y| > |x|, else x; (sc, tc) / ma are the OpenGL face coordinates.
template <typename T>
__device__ __forceinline__ int cube_face(T x, T y, T z, T& sc, T& tc, T& ma) {
    const T ax = x < T(0) ? -x : x, ay = y < T(0) ? -y : y, az = z < T(0) ? -z : z;
    if (az > (ax > ay ? ax : ay)) {
        ma = az;
        tc = -y;
        if (z > T(0)) { sc = x; return 4; }
        sc = -x;
        return 5;
    }
    if (ay > ax) {
        ma = ay;
        sc = x;
        if (y > T(0)) { tc = z; return 2; }
        tc = -z;
        return 3;
    }
    ma = ax;
    tc = -y;
    if (x > T(0)) { sc = -z; return 0; }
    sc = z;
    return 1;
}

// A tap that has left its face in ONE axis: the centre of that tap on the extended face plane, re-indexed with the face
// rule, in exact integers.  With ns = 2 ix + 1 - R, nt = 2 iy + 1 - R the centre is (ns, nt) / R in face coordinates; the
// point R * (x, y, z) is integral, its major axis has |.| = R + 1 and no tie is possible.  -> texel index in [0, 6 R R).
__device__ __forceinline__ int cube_edge_tap(int face, int ix, int iy, int R) {
    const int ns = 2 * ix + 1 - R, nt = 2 * iy + 1 - R;
    int x, y, z;
    switch (face) {
        case 0: x = R; y = -nt; z = -ns; break;
        case 1: x = -R; y = -nt; z = ns; break;
        case 2: x = ns; y = R; z = nt; break;
        case 3: x = ns; y = -R; z = -nt; break;
        case 4: x = ns; y = -nt; z = R; break;
        default: x = -ns; y = -nt; z = -R; break;
    }
    int sc, tc, ma;
    const int f2 = cube_face<int>(x, y, z, sc, tc, ma);
    // floor((s + 1) / 2 * R), s = sc / ma: (sc + ma) R / (2 ma), all positive; R <= 16384 keeps it inside int32
    const int x2 = min(((sc + ma) * R) / (2 * ma), R - 1);
    const int y2 = min(((tc + ma) * R) / (2 * ma), R - 1);
    return (f2 * R + y2) * R + x2;
}

// The four taps of a finite non-zero direction: texel indices and weights (a dropped corner tap has weight 0 and index 0).
__device__ __forceinline__ void cube_taps(float x, float y, float z, int R, int (&idx)[4], float (&w)[4]) {
    float sc, tc, ma;
    const int face = cube_face<float>(x, y, z, sc, tc, ma);
    const float s = sc / ma, t = tc / ma;
    const float half_r = 0.5f * (float)R;
    const float fu = (s + 1.0f) * half_r - 0.5f, fv = (t + 1.0f) * half_r - 0.5f;      // in [-0.5, R - 0.5]
    const float flu = floorf(fu), flv = floorf(fv);
    // (|s|, |t| <= 1 put the floors in [-1, R - 1]; the clamp keeps every index in bounds whatever the arithmetic did)
    const int ix0 = min(max((int)flu, -1), R - 1), iy0 = min(max((int)flv, -1), R - 1);
    const float fx = fu - flu, fy = fv - flv;
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
    float kept = 0.0f;
    bool dropped = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ix = ix0 + (k & 1), iy = iy0 + (k >> 1);
        const bool ox = ix < 0 || ix >= R, oy = iy < 0 || iy >= R;
        w[k] = wx[k & 1] * wy[k >> 1];
        if (ox && oy) {                         // a cube corner: no texel there
            w[k] = 0.0f;
            idx[k] = 0;
            dropped = true;
        } else {
            idx[k] = (ox || oy) ? cube_edge_tap(face, ix, iy, R) : (face * R + iy) * R + ix;
            kept += w[k];
        }
    }
    if (dropped) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = w[k] / kept;
    }
}

__device__ __forceinline__ float cube_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

struct CubeArgs {
    const float* tex;        // [6,R,R,C]
    const float* dirs;       // [n,3], or null: ray generation from m
    const float* perturb;    // [n,2] or null (0.5, 0.5)
    const uint8_t* mask;     // [n] or null
    const float* acc;        // [n] or null: masked = (1 - acc) > 1e-3
    int64_t n;
    int R, width, flags;
    float fill;
    float m[9];
};

// The backward's adds, shaped for the memory side.  Left as they fall, the 64 lanes of one atomic instruction hold one
// channel of 64 texels: 64 dwords 4 C bytes apart, a 64-byte request for every few lanes.  Instead the wave's 64 C
// (sample, channel) terms of a tap are dealt out again, sample-major: lane l of round j holds term j * 64 + l, so that the C
// channels of a texel sit in C adjacent lanes and neighbouring samples, whose taps are neighbouring texels, follow one
// another: an instruction covers about 64 / C texels of contiguous bytes.  Every lane of the wave takes part (a lane
// without a sample deals zeros); zero terms are not added.
template <int C>
__device__ __forceinline__ void cube_wave_adds(const int (&idx)[4], const float (&term)[4][C], float* __restrict__ grad_tex) {
    const int lane = sc_lane();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int e = j * SC_WAVE + lane, src = e / C, ch = e % C;
            const int texel = __shfl(idx[k], src, SC_WAVE);
            float v = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float t = __shfl(term[k][c], src, SC_WAVE);
                if (c == ch) v = t;
            }
            if (v != 0.0f) atomicAdd(&grad_tex[(int64_t)texel * C + ch], v);
        }
    }
}

template <int C, bool BWD>
__global__ __launch_bounds__(CUBE_THREADS) void cubemap_kernel(CubeArgs a, float* __restrict__ out,
                                                               const float* __restrict__ grad_out,
                                                               float* __restrict__ grad_tex) {
    const int64_t i = (int64_t)blockIdx.x * CUBE_THREADS + threadIdx.x;
    const bool inside = i < a.n;
    if (!BWD && !inside) return;                // (the backward keeps whole waves for cube_wave_adds)
    const bool planar = (a.flags & SC_CUBE_PLANAR) != 0;
    const int64_t o0 = planar ? i : i * C, os = planar ? a.n : 1;
    bool on = inside;
    if (on) {
        if (a.mask) on = a.mask[i] != 0;
        else if (a.acc) on = (1.0f - a.acc[i]) > 1e-3f;
    }
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (on) {
        if (a.dirs) {
            x = a.dirs[3 * i]; y = a.dirs[3 * i + 1]; z = a.dirs[3 * i + 2];
        } else {
            const float u = (float)(i % a.width) + (a.perturb ? a.perturb[2 * i] : 0.5f);
            const float v = (float)(i / a.width) + (a.perturb ? a.perturb[2 * i + 1] : 0.5f);
            x = (a.m[0] * u + a.m[1] * v) + a.m[2];
            y = (a.m[3] * u + a.m[4] * v) + a.m[5];
            z = (a.m[6] * u + a.m[7] * v) + a.m[8];
        }
    }
    const bool valid = on && isfinite(x) && isfinite(y) && isfinite(z) && !(x == 0.0f && y == 0.0f && z == 0.0f);
    const bool sig = (a.flags & SC_CUBE_SIGMOID) != 0, clamp01 = (a.flags & SC_CUBE_CLAMP) != 0;
    int idx[4] = {0, 0, 0, 0};
    float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float val[C], act[4][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        val[c] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) act[k][c] = 0.0f;
    }
    if (valid) {
        cube_taps(x, y, z, a.R, idx, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float t = a.tex[(int64_t)idx[k] * C + c];
                act[k][c] = sig ? cube_sigmoid(t) : t;
                val[c] = val[c] + w[k] * act[k][c];
            }
        }
    }
    if (!BWD) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float v = clamp01 ? fminf(fmaxf(val[c], 0.0f), 1.0f) : val[c];
            out[o0 + c * os] = valid ? v : (on ? 0.0f : a.fill);
        }
        return;
    }
    float term[4][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float g = valid ? grad_out[o0 + c * os] : 0.0f;
        if (clamp01 && !(val[c] >= 0.0f && val[c] <= 1.0f)) g = 0.0f;       // torch.clamp passes its gradient on [0, 1]
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = sig ? act[k][c] * (1.0f - act[k][c]) : 1.0f;
            term[k][c] = (valid && g != 0.0f && w[k] != 0.0f) ? (w[k] * g) * d : 0.0f;
        }
    }
    cube_wave_adds<C>(idx, term, grad_tex);
}

template <bool BWD>
int cubemap_launch(const CubeArgs& a, int C, float* out, const float* grad_out, float* grad_tex, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n + CUBE_THREADS - 1) / CUBE_THREADS)), block(CUBE_THREADS);
    switch (C) {
        case 1: hipLaunchKernelGGL((cubemap_kernel<1, BWD>), grid, block, 0, stream, a, out, grad_out, grad_tex); break;
        case 2: hipLaunchKernelGGL((cubemap_kernel<2, BWD>), grid, block, 0, stream, a, out, grad_out, grad_tex); break;
        case 3: hipLaunchKernelGGL((cubemap_kernel<3, BWD>), grid, block, 0, stream, a, out, grad_out, grad_tex); break;
        default: hipLaunchKernelGGL((cubemap_kernel<4, BWD>), grid, block, 0, stream, a, out, grad_out, grad_tex); break;
    }
    SC_LAUNCH_CHECK();
    return SC_OK;
}

}  // namespace

// Called by the validated entry points in capi.hip.
int sc_cubemap_run(const float* tex, int resolution, int channels, const float* dirs, const float* ray_matrix_host,
                   const float* perturb, const uint8_t* mask, const float* acc, int64_t n, int width, int flags, float fill,
                   float* out, const float* grad_out, float* grad_tex, sc_stream_t stream) {
    CubeArgs a;
    a.tex = tex; a.dirs = dirs; a.perturb = perturb; a.mask = mask; a.acc = acc;
    a.n = n; a.R = resolution; a.width = width > 0 ? width : 1; a.flags = flags; a.fill = fill;
    for (int k = 0; k < 9; ++k) a.m[k] = ray_matrix_host ? ray_matrix_host[k] : 0.0f;
    if (!grad_tex) return cubemap_launch<false>(a, channels, out, nullptr, nullptr, sc_s(stream));
    SC_HIP(hipMemsetAsync(grad_tex, 0, sizeof(float) * 6 * (size_t)resolution * resolution * channels, sc_s(stream)));
    if (n == 0) return SC_OK;
    return cubemap_launch<true>(a, channels, nullptr, grad_out, grad_tex, sc_s(stream));
}
