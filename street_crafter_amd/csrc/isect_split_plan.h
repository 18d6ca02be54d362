// The RANGE PLAN of big_split_kernel (isect_bin.hip): how a super-tile bucket of n > cap records is cut into depth
// ranges that one sort workgroup takes.  The per-bin arithmetic lives here, __host__ __device__, so that the kernel and
// the host entries sc_isect_split_* (which the CPU tests drive against oracle/split_plan.py) run the SAME formulae.
//
//   1. bins    : bin_of(K) = min(SP_BINS - 1, (int)((double)(K - lo) * (SP_BINS / ((double)(hi - lo) + 1)))) over the
//                bucket's 60-bit keys; monotone in K.
//   2. groups  : a bin of more than light_max = cap / 4 records is HEAVY and a group of its own; consecutive light bins
//                share a group while their running total (over the light bins alone) stays inside one multiple of
//                target = 3/4 cap, so a light group holds < target + light_max = cap records.  Computed in parallel from
//                two prefix sums: gid = floor(light / target) + 2 H + heavy, made dense over the non-empty bins.
//                Alone this gives up to ~2 n / (light_max + 1) groups: a heavy bin of light_max + 1 records followed by
//                one light record opens two.
//   3. ranges  : serial greedy over the groups (sp_merge_groups): a group joins the open range when the sum stays
//                <= cap, else it opens the next.  A group of more than cap records (one bin that depth cannot cut) never
//                fits and nothing fits behind it: it is a range of its own, `heavy`, sorted by the exact quadratic path.
//
// THE BOUND (the one derivation; the kernel, seg_bound_for() and DESIGN.md refer to it).  Range r + 1 is opened by a
// group g that did not fit: count(r) + count(g) > cap, and count(r + 1) >= count(g).  So any two neighbouring ranges
// hold more than cap records together; pairing them (0,1), (2,3), ... gives floor(R / 2) * (cap + 1) <= n, i.e.
//                R <= sp_max_ranges(n, cap) = 2 * floor(n / (cap + 1)) + 1.
// Every range that is not heavy holds <= cap records.  Over the oversized buckets of a frame (at most nsb of them,
// sum of n_b <= N): sum_b R_b <= 2 * floor(N / (cap + 1)) + nsb.
#pragma once
#include <stdint.h>

constexpr int SP_BINS = 1024;                    // histogram bins of the split (== threads of big_split_kernel)

__host__ __device__ inline int sp_light_max(int cap) { return cap / 4; }
__host__ __device__ inline int sp_target(int cap) { return (cap * 3) / 4; }
__host__ __device__ inline int64_t sp_max_ranges(int64_t n, int cap) { return 2 * (n / ((int64_t)cap + 1)) + 1; }

__host__ __device__ inline double sp_bin_scale(unsigned long long lo, unsigned long long hi) {
    return (double)SP_BINS / ((double)(hi - lo) + 1.0);
}
__host__ __device__ inline int sp_bin_of(unsigned long long K, unsigned long long lo, double scale) {
    const int b = (int)((double)(K - lo) * scale);
    return b < SP_BINS - 1 ? b : SP_BINS - 1;
}

// sparse, monotone group id of a bin: `light` = records in the light bins before it, H = heavy bins before it
__host__ __device__ inline unsigned sp_group_id(unsigned light, unsigned H, bool heavy, int target) {
    return light / (unsigned)target + 2u * H + (heavy ? 1u : 0u);
}

// Step 3.  gcnt[g * gstride] = records of group g (G groups, in depth order) -> gmap[g * mstride] = its range, and per
// range its count and the exclusive prefix of the counts; returns R.  R <= sp_max_ranges(n, cap) (see THE BOUND), which
// the caller keeps <= max_ranges by bounding n; should it not, the surplus joins the LAST range, which then holds more
// than cap records and takes the exact path -- no table is ever indexed at or beyond max_ranges, no record is lost.
__host__ __device__ inline int sp_merge_groups(const unsigned* gcnt, int gstride, int G, int cap, int max_ranges,
                                               unsigned* gmap, int mstride, unsigned* rcnt, unsigned* rstart) {
    int r = -1;
    unsigned cur = 0, run = 0;
    for (int g = 0; g < G; ++g) {
        const unsigned c = gcnt[g * gstride];
        const bool fits = r >= 0 && cur + c <= (unsigned)cap;
        if (!fits && r + 1 < max_ranges) { ++r; rstart[r] = run; cur = 0; }
        cur += c; run += c;
        rcnt[r] = cur;
        gmap[g * mstride] = (unsigned)r;
    }
    return r + 1;
}
