// LiDAR condition frame, assembled on the device: frame assembly + visibility filter + point projection in one launch.
// Replaces, per frame, the host work of data_processor/waymo_processor/waymo_render_lidar_pcd.py:207-267 and of
// WaymoPointCloudProcessor.render_condition (waymo_processor.py:199-226) in front of sc_point_project: the sweeps are
// resident on the device (street_crafter_amd/lidar_sequence.py: xyz float64 [M,3], rgb float32 [M,3], every track's
// frames contiguous in frame order), and a frame is a short table of segments (resident begin, count, output begin,
// pose slot) plus the actor poses and the camera, sent as one small block.
//
// One thread per assembled point i in [0, N):
//   segment s = the one whose output range holds i;  p = xyz[src_begin[s] + i - out_begin[s]]
//   w = p (no pose) or  w_r = P[r][0] x + P[r][1] y + P[r][2] z + P[r][3]       fp64, left to right, no contraction
//   filter (optional, lidar_condition.filter_visible in fp64):  cam = M [w,1],  pix = K cam,
//          kept iff cam_z > 1e-3, 0 <= pix_0 / pix_2 < W, 0 <= pix_1 / pix_2 < H;  a dropped point's row is all zero
//   q = (float)(w - origin)   (fp64 subtraction, as point_render.render_points_hip rounds host points)
//   row i = sc_point_project_row(q)  (point_project.h: the body of sc_point_project, bit for bit)
//   points_world [N,3] = (float)w  (optional: what distCUDA2 of the knn radius rule reads)
// Nothing is compacted: a dropped point keeps its row (radius 0), and the radix sort behind the tile binning is stable
// in the point index, so depth ties among kept points resolve as they do after the host's compaction.
//
// Segment search: upper bound over the output-begin column.  The first ASM_LDS_SEGS = 1024 entries of that column are
// copied into LDS (4 KiB) by every workgroup; the search reads entries beyond that capacity from the table in global
// memory (L2 hits: every lane of every wave probes the same few words).  A frame has 1 + (actors in view) segments,
// tens in practice.  sc_point_assemble_lds_segments() reports the capacity.
//
// Traffic per point: 24 B xyz + 12 B rgb read, 4 + 8 + 4 + 32 B written (+ 12 B points_world): streaming, one pass.
// ~60 fp64 operations per point with the filter.
#include "point_project.h"

#pragma clang fp contract(off)

namespace {

constexpr int ASM_BLK = 256;
constexpr int ASM_LDS_SEGS = 1024;

// words (8 B) of the frame block's header: include/street_crafter_amd.h sc_point_assemble_project
constexpr int HDR_VIEW = 0, HDR_ORIGIN = 16, HDR_FILT_M = 20, HDR_FILT_K = 32;
constexpr int HDR_WORDS = SC_POINT_FRAME_HEADER_WORDS;

__global__ __launch_bounds__(ASM_BLK) void point_assemble_project_kernel(
    const double* __restrict__ xyz, const float* __restrict__ rgb, int64_t n_resident,
    const double* __restrict__ hdr, const double* __restrict__ poses, const sc_point_segment* __restrict__ segs,
    int n_segments, int n_poses, int N, int filter, double width, double height, float occ,
    const float* __restrict__ radius_in, ScPointCam cam, int32_t* __restrict__ radii, float* __restrict__ means2d,
    float* __restrict__ depths, float4* __restrict__ records, float* __restrict__ points_world) {
    __shared__ int32_t begin_s[ASM_LDS_SEGS];
    const int n_lds = min(n_segments, ASM_LDS_SEGS);
    for (int t = threadIdx.x; t < n_lds; t += ASM_BLK) begin_s[t] = segs[t].out_begin;
    __syncthreads();
    const int i = blockIdx.x * ASM_BLK + threadIdx.x;
    if (i >= N) return;
    // first segment whose output begin lies beyond i; the one before it owns i.  Empty segments share their begin with
    // the next non-empty one, which is the last of the run and so the one found.  (The host entry has checked that the
    // ranges tile [0, N) in order: out_begin[0] == 0 <= i.)
    int lo = 0, hi = n_segments;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int b = mid < n_lds ? begin_s[mid] : segs[mid].out_begin;
        if (b > i) hi = mid; else lo = mid + 1;
    }
    const sc_point_segment seg = segs[max(lo - 1, 0)];
    const int64_t src = seg.src_begin + (int64_t)(i - seg.out_begin);
    // a table that is not the one the host entry checked must not read outside the resident arrays
    bool listed = src >= 0 && src < n_resident && seg.pose < n_poses;
    double wx = 0.0, wy = 0.0, wz = 0.0;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (listed) {
        const double x = xyz[src * 3 + 0], y = xyz[src * 3 + 1], z = xyz[src * 3 + 2];
        c0 = rgb[src * 3 + 0], c1 = rgb[src * 3 + 1], c2 = rgb[src * 3 + 2];
        wx = x, wy = y, wz = z;
        if (seg.pose >= 0) {
            const double* P = poses + (int64_t)seg.pose * 12;
            wx = P[0] * x + P[1] * y + P[2] * z + P[3];
            wy = P[4] * x + P[5] * y + P[6] * z + P[7];
            wz = P[8] * x + P[9] * y + P[10] * z + P[11];
        }
    }
    if (points_world) {
        points_world[(int64_t)i * 3 + 0] = (float)wx;
        points_world[(int64_t)i * 3 + 1] = (float)wy;
        points_world[(int64_t)i * 3 + 2] = (float)wz;
    }
    if (!radii) return;                                     // the world-points-only launch of the knn radius rule
    if (filter && listed) {
        const double* M = hdr + HDR_FILT_M;
        const double* K = hdr + HDR_FILT_K;
        const double mx = M[0] * wx + M[1] * wy + M[2] * wz + M[3];
        const double my = M[4] * wx + M[5] * wy + M[6] * wz + M[7];
        const double mz = M[8] * wx + M[9] * wy + M[10] * wz + M[11];
        const double p0 = K[0] * mx + K[1] * my + K[2] * mz;
        const double p1 = K[3] * mx + K[4] * my + K[5] * mz;
        const double p2 = K[6] * mx + K[7] * my + K[8] * mz;
        const double fu = p0 / p2, fv = p1 / p2;
        listed = mz > 1e-3 && fu >= 0.0 && fu < width && fv >= 0.0 && fv < height;
    }
    const double* O = hdr + HDR_ORIGIN;
    const double qx = (double)(float)(wx - O[0]), qy = (double)(float)(wy - O[1]), qz = (double)(float)(wz - O[2]);
    sc_point_project_row(i, qx, qy, qz, c0, c1, c2, occ, radius_in, hdr + HDR_VIEW, cam, listed, radii, means2d,
                         depths, records);
}

}  // namespace

extern "C" int sc_point_assemble_lds_segments(void) { return ASM_LDS_SEGS; }

extern "C" int sc_point_assemble_project(const double* xyz, const float* rgb, int64_t n_resident,
                                         const void* frame_host, const void* frame_dev, int n_segments, int n_poses,
                                         int N, int filter, float occ, const float* radius_in, double fx, double fy,
                                         double cx, double cy, double focal_r, int width, int height,
                                         double near_plane, double far_plane, int radius_mode, double scale,
                                         float knn_scale_down, int32_t* radii, float* means2d, float* depths,
                                         float* records, float* points_world, sc_stream_t stream) {
    if (N < 0 || n_segments < 0 || n_poses < 0 || n_resident < 0 || width <= 0 || height <= 0) return SC_EINVAL;
    if (radius_mode < SC_RMODE_CONST || radius_mode > SC_RMODE_KNN) return SC_EINVAL;
    if (!(occ > 0.f && occ <= 1.f)) return SC_EINVAL;
    if (radius_mode == SC_RMODE_KNN && !radius_in) return SC_EINVAL;
    if (!(focal_r > 0.0) || !(scale >= 0.0)) return SC_EINVAL;
    if (filter != 0 && filter != 1) return SC_EINVAL;
    if (!frame_host && n_segments > 0) return SC_EINVAL;
    // the segment table, on the host copy of the block: counts, the tiling of [0, N), pose slots, resident ranges
    const char* host = static_cast<const char*>(frame_host);
    const size_t seg_off = (size_t)8 * ((size_t)HDR_WORDS + (size_t)12 * (size_t)n_poses);
    const sc_point_segment* segs_h = reinterpret_cast<const sc_point_segment*>(host + seg_off);
    int64_t run = 0;
    for (int s = 0; s < n_segments; ++s) {
        const sc_point_segment& g = segs_h[s];
        if (g.count < 0 || (int64_t)g.out_begin != run) return SC_EINVAL;
        if (g.pose < -1 || g.pose >= n_poses) return SC_EINVAL;
        if (g.src_begin < 0 || g.src_begin > n_resident || (int64_t)g.count > n_resident - g.src_begin) return SC_EINVAL;
        run += g.count;
    }
    if (run != (int64_t)N) return SC_EINVAL;
    if (N == 0) return SC_OK;
    if (!xyz || !rgb || !frame_dev) return SC_EINVAL;
    if (((uintptr_t)frame_dev & 7) != 0) return SC_EINVAL;       // read as doubles / int64
    const bool project = radii || means2d || depths || records;
    if (project && (!radii || !means2d || !depths || !records)) return SC_EINVAL;
    if (!project && !points_world) return SC_EINVAL;
    if (((uintptr_t)records & 15) != 0) return SC_EINVAL;        // written as float4
    const double* hdr = static_cast<const double*>(frame_dev);
    const double* poses = hdr + HDR_WORDS;
    const sc_point_segment* segs = reinterpret_cast<const sc_point_segment*>(static_cast<const char*>(frame_dev) + seg_off);
    const double half_min_hw = 0.5 * (double)(height <= width ? height : width);
    const ScPointCam cam = {fx, fy, cx, cy, focal_r, near_plane, far_plane, scale, half_min_hw, radius_mode,
                            knn_scale_down};
    hipLaunchKernelGGL(point_assemble_project_kernel, dim3((unsigned)(((int64_t)N + ASM_BLK - 1) / ASM_BLK)),
                       dim3(ASM_BLK), 0, sc_s(stream), xyz, rgb, n_resident, hdr, poses, segs, n_segments, n_poses, N,
                       filter, (double)width, (double)height, occ, radius_in, cam, radii, means2d, depths,
                       reinterpret_cast<float4*>(records), points_world);
    SC_LAUNCH_CHECK();
    return SC_OK;
}
