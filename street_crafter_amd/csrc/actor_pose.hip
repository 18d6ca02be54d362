// The actor poses of a frame: ActorPose.get_tracking_rotation / get_tracking_translation of every visible actor
// (street_gaussian/models/actor_pose.py:83-144) in one launch, and the backward into the opt_trans / opt_rots tables in
// one launch behind one memset per table.  The formulas and their evaluation order are in include/street_crafter_amd.h.
//
// Tens of actors, a few hundred flops each: the kernel is a launch, not a throughput problem.  One thread per item, 64
// per workgroup; the item table travels BY VALUE in the kernel arguments (24 B x 128 items = 3 KB of HIP's 4 KB), as
// compose.hip's segment table does, so that a call copies nothing, stages nothing and waits for nothing: the host
// returns as soon as the launch is queued, whatever runs in front of it.  More than 128 items are more launches.
#include "sc_common.h"

// Every product, sum and quotient below is rounded on its own (frame_tail.hip: hipcc contracts a * b + c into an FMA by
// default, through __fmul_rn / __fadd_rn as well); tests/actor_pose_ref.py replays these operations one by one.
#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 64;
constexpr int MAX_ITEMS = 128;
constexpr float NORM_EPS = 1e-12f;             // F.normalize's floor
constexpr float SERIES_PHI = 1e-3f;            // at and below this angle the slerp takes its series
constexpr float SIXTH = 1.0f / 6.0f;

struct FwdArgs {
    sc_actor_pose_item it[MAX_ITEMS];
    int n;
    const float *input_trans, *input_rots, *opt_trans, *opt_rots;
    float *obj_rots, *obj_trans;               // row 0 = the launch's first item
};

struct BwdArgs {
    sc_actor_pose_item it[MAX_ITEMS];
    int n;
    const float *input_rots, *opt_rots;
    const float *g_obj_rots, *g_obj_trans;     // each nullable: zeros; row 0 = the launch's first item
    float *grad_opt_trans, *grad_opt_rots;     // each nullable: not computed
};

struct Quat { float w, x, y, z; };
struct Pose { float t[3]; Quat q; };

// Hamilton product, real part first; the four terms of a component are summed left to right
__device__ __forceinline__ Quat qmul(const Quat a, const Quat b) {
    return {((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z,
            ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y,
            ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x,
            ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w};
}

__device__ __forceinline__ Quat qnormalize(const Quat q) {
    const float n = sqrtf(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
    const float d = n > NORM_EPS ? n : NORM_EPS;
    return {q.w / d, q.x / d, q.y / d, q.z / d};
}

// the pose at one row of the tracklet tables (actor_pose.py:83-93)
__device__ __forceinline__ Pose plain_pose(const FwdArgs& a, const int64_t row, const bool delta) {
    Pose o;
    const float* t = a.input_trans + 3 * row;
    const float* r = a.input_rots + 4 * row;
    o.t[0] = t[0]; o.t[1] = t[1]; o.t[2] = t[2];
    o.q = {r[0], r[1], r[2], r[3]};
    if (delta) {
        const float* d = a.opt_trans + 3 * row;
        o.t[0] = o.t[0] + d[0]; o.t[1] = o.t[1] + d[1]; o.t[2] = o.t[2] + d[2];
        const float half = a.opt_rots[row] * 0.5f;
        const float c = cosf(half), s = sinf(half);
        const Quat q = o.q;
        o.q = {q.w * c - q.z * s, q.x * c + q.y * s, q.y * c - q.x * s, q.z * c + q.w * s};
    }
    return o;
}

__device__ __forceinline__ Quat slerp(const Quat p, const Quat n, const float alpha) {
    const Quat ph = qnormalize(p), nh = qnormalize(n);
    Quat r = qmul({ph.w, -ph.x, -ph.y, -ph.z}, nh);
    if (r.w < 0.0f) r = {-r.w, -r.x, -r.y, -r.z};
    const float sv = sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z);
    const float phi = atan2f(sv, r.w);
    float ew, f;
    if (phi <= SERIES_PHI) {
        const float p2 = phi * phi, a2 = alpha * alpha;
        ew = 1.0f - 0.5f * (a2 * p2);
        f = alpha * (1.0f + ((1.0f - a2) * p2) * SIXTH);
    } else {
        const float ap = alpha * phi;
        ew = cosf(ap);
        f = sinf(ap) / sv;
    }
    return qmul(ph, {ew, f * r.x, f * r.y, f * r.z});
}

__global__ void __launch_bounds__(BLOCK) actor_poses_fwd_kernel(const FwdArgs a) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= a.n) return;
    const sc_actor_pose_item it = a.it[i];
    const bool delta = (it.flags & SC_POSE_DELTA) != 0;
    Pose o;
    if (it.flags & SC_POSE_INTERP) {
        const Pose p = plain_pose(a, it.row_prev, delta), n = plain_pose(a, it.row_next, delta);
#pragma unroll
        for (int k = 0; k < 3; ++k) o.t[k] = it.alpha * n.t[k] + it.one_minus_alpha * p.t[k];
        o.q = slerp(p.q, n.q, it.alpha);
    } else {
        o = plain_pose(a, it.row, delta);
    }
    float* oq = a.obj_rots + 4 * (int64_t)i;
    oq[0] = o.q.w; oq[1] = o.q.x; oq[2] = o.q.y; oq[3] = o.q.z;
    float* ot = a.obj_trans + 3 * (int64_t)i;
    ot[0] = o.t[0]; ot[1] = o.t[1]; ot[2] = o.t[2];
}

// (the tables were zeroed in front of this launch; the rows of the SC_POSE_DELTA items are distinct: plain stores)
__global__ void __launch_bounds__(BLOCK) actor_poses_bwd_kernel(const BwdArgs a) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= a.n) return;
    const sc_actor_pose_item it = a.it[i];
    if (!(it.flags & SC_POSE_DELTA)) return;
    const int64_t row = it.row;
    if (a.grad_opt_trans && a.g_obj_trans) {
        const float* g = a.g_obj_trans + 3 * (int64_t)i;
        float* o = a.grad_opt_trans + 3 * row;
        o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
    }
    if (a.grad_opt_rots && a.g_obj_rots) {
        const float* g = a.g_obj_rots + 4 * (int64_t)i;
        const float* r = a.input_rots + 4 * row;
        const float half = a.opt_rots[row] * 0.5f;
        const float c = cosf(half), s = sinf(half);
        const float dc = -s * 0.5f, ds = c * 0.5f;
        const float kw = g[0] * (r[0] * dc - r[3] * ds);
        const float kx = g[1] * (r[1] * dc + r[2] * ds);
        const float ky = g[2] * (r[2] * dc - r[1] * ds);
        const float kz = g[3] * (r[3] * dc + r[0] * ds);
        a.grad_opt_rots[row] = ((kw + kx) + ky) + kz;
    }
}

template <typename Args, typename Kernel>
int launch(const Args& a, Kernel kernel, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, a);
    SC_LAUNCH_CHECK();
    return SC_OK;
}

}  // namespace

static_assert(sizeof(sc_actor_pose_item) == 24, "sc_actor_pose_item is 24 bytes");
static_assert(sizeof(FwdArgs) <= 4096 && sizeof(BwdArgs) <= 4096, "HIP passes at most 4 KB of kernel arguments");

extern "C" int sc_actor_poses_max_items(void) { return MAX_ITEMS; }

// (arguments validated by capi.hip)
int sc_actor_poses_fwd_run(const sc_actor_pose_item* items_host, int A, const float* input_trans, const float* input_rots,
                           const float* opt_trans, const float* opt_rots, float* obj_rots, float* obj_trans,
                           sc_stream_t stream) {
    FwdArgs a;
    a.input_trans = input_trans; a.input_rots = input_rots; a.opt_trans = opt_trans; a.opt_rots = opt_rots;
    for (int at = 0; at < A; at += MAX_ITEMS) {
        a.n = A - at < MAX_ITEMS ? A - at : MAX_ITEMS;
        for (int k = 0; k < a.n; ++k) a.it[k] = items_host[at + k];
        a.obj_rots = obj_rots + 4 * (int64_t)at;
        a.obj_trans = obj_trans + 3 * (int64_t)at;
        const int rc = launch(a, actor_poses_fwd_kernel, sc_s(stream));
        if (rc) return rc;
    }
    return SC_OK;
}

int sc_actor_poses_bwd_run(const sc_actor_pose_item* items_host, int A, int64_t rows, const float* input_rots,
                           const float* opt_rots, const float* g_obj_rots, const float* g_obj_trans, float* grad_opt_trans,
                           float* grad_opt_rots, sc_stream_t stream) {
    if (grad_opt_trans && rows > 0) SC_HIP(hipMemsetAsync(grad_opt_trans, 0, sizeof(float) * 3 * (size_t)rows, sc_s(stream)));
    if (grad_opt_rots && rows > 0) SC_HIP(hipMemsetAsync(grad_opt_rots, 0, sizeof(float) * (size_t)rows, sc_s(stream)));
    const bool trans = grad_opt_trans && g_obj_trans, rots = grad_opt_rots && g_obj_rots;
    if (!trans && !rots) return SC_OK;                                  // zeros are the whole answer
    BwdArgs a;
    a.input_rots = input_rots; a.opt_rots = opt_rots;
    a.grad_opt_trans = grad_opt_trans; a.grad_opt_rots = grad_opt_rots;
    for (int at = 0; at < A; at += MAX_ITEMS) {
        a.n = A - at < MAX_ITEMS ? A - at : MAX_ITEMS;
        bool any = false;
        for (int k = 0; k < a.n; ++k) {
            a.it[k] = items_host[at + k];
            any = any || (a.it[k].flags & SC_POSE_DELTA) != 0;
        }
        if (!any) continue;
        a.g_obj_rots = g_obj_rots ? g_obj_rots + 4 * (int64_t)at : nullptr;
        a.g_obj_trans = g_obj_trans ? g_obj_trans + 3 * (int64_t)at : nullptr;
        const int rc = launch(a, actor_poses_bwd_kernel, sc_s(stream));
        if (rc) return rc;
    }
    return SC_OK;
}
