"""Checker only: the RANGE PLAN of the tile-bucketed isect_tiles route for one oversized super-tile bucket, restated
in numpy -- steps 1-3 of the header comment of street_crafter_amd/csrc/isect_split_plan.h (big_split_kernel,
isect_bin.hip).  From the bucket's 60-bit keys (depth bits << 28 | flat id): lo / hi, the bin of every key with the
kernel's own arithmetic, the per-bin counts, heavy / light, the group id of every non-empty bin, the greedy merge of
the groups into ranges, R, the per-range counts and the `heavy` flag of each range.

Also here, shared by tests/test_isect_split_plan_cpu.py and the GPU cases of tests/test_gpu_parity.py: the COMB
histograms (teeth of a given size with light bins between them: the family on which the plan opens the most ranges
per record) and the frames that put such a histogram into one super-tile's bucket."""
import numpy as np

CAP = 3584            # records one sort workgroup takes (asserted against sc_isect_split_limits by the CPU tests)
BINS = 1024
ID_BITS = 28
LEVEL0_BITS = 0x41000000          # depth 8.0; level m = LEVEL0_BITS + LEVEL_STEP * m: depths in [8, 12)
LEVEL_STEP = 4096


def light_max(cap=CAP):
    return cap // 4


def target(cap=CAP):
    return (cap * 3) // 4


def max_ranges(n, cap=CAP):
    """f(n): the most ranges a bucket of n records is cut into (isect_split_plan.h, THE BOUND)."""
    return 2 * (int(n) // (cap + 1)) + 1


def key60(depth_bits, flat_ids):
    return (np.asarray(depth_bits).astype(np.uint64) << np.uint64(ID_BITS)) | np.asarray(flat_ids).astype(np.uint64)


def bin_of(keys, lo=None, hi=None):
    """(double)(K - lo) * (1024 / ((double)(hi - lo) + 1)), truncated, clamped to 1023."""
    keys = np.asarray(keys, dtype=np.uint64)
    lo = keys.min() if lo is None else np.uint64(lo)
    hi = keys.max() if hi is None else np.uint64(hi)
    scale = np.float64(BINS) / (np.float64(hi - lo) + np.float64(1.0))
    b = ((keys - lo).astype(np.float64) * scale).astype(np.int64)
    return np.minimum(b, BINS - 1)


def groups_from_counts(counts, cap=CAP):
    """Step 2.  -> (group_of_bin int64[BINS] (-1: empty bin), group_counts int64[G])."""
    counts = np.asarray(counts, dtype=np.int64)
    heavy = counts > light_max(cap)
    lc = np.where(heavy, 0, counts)
    light = np.cumsum(lc) - lc                      # records in the light bins before this one
    H = np.cumsum(heavy) - heavy                    # heavy bins before this one
    gid = light // target(cap) + 2 * H + heavy
    ne = np.flatnonzero(counts)
    first = np.ones(len(ne), dtype=bool)
    first[1:] = gid[ne][1:] != gid[ne][:-1]
    dense = np.cumsum(first) - 1
    group_of_bin = np.full(len(counts), -1, dtype=np.int64)
    group_of_bin[ne] = dense
    return group_of_bin, np.bincount(dense, weights=counts[ne]).astype(np.int64)


def merge_groups(group_counts, cap=CAP):
    """Step 3: a group joins the open range while the sum stays <= cap, else it opens the next.  -> range of each group."""
    out = np.empty(len(group_counts), dtype=np.int64)
    r, cur = -1, 0
    for g, c in enumerate(group_counts.tolist()):
        if r < 0 or cur + c > cap:
            r, cur = r + 1, 0
        cur += c
        out[g] = r
    return out


def plan_from_counts(counts, cap=CAP, merge=True):
    """-> dict(R, range_of_bin (-1: empty bin), range_counts, heavy (per range), G (groups before the merge)).
    merge=False: the groups themselves as ranges -- the plan as it was before the merge step existed."""
    counts = np.asarray(counts, dtype=np.int64)
    group_of_bin, gcnt = groups_from_counts(counts, cap)
    rng_of_group = merge_groups(gcnt, cap) if merge else np.arange(len(gcnt), dtype=np.int64)
    range_of_bin = np.where(group_of_bin >= 0, rng_of_group[np.maximum(group_of_bin, 0)], -1)
    R = int(rng_of_group[-1]) + 1 if len(gcnt) else 0
    range_counts = np.bincount(rng_of_group, weights=gcnt, minlength=R).astype(np.int64)
    return {"R": R, "range_of_bin": range_of_bin, "range_counts": range_counts, "heavy": range_counts > cap,
            "G": len(gcnt)}


def plan(keys, cap=CAP, merge=True):
    """The whole plan of one bucket from its keys; adds lo, hi, bins (of every key) and counts to plan_from_counts."""
    keys = np.asarray(keys, dtype=np.uint64)
    bins = bin_of(keys)
    counts = np.bincount(bins, minlength=BINS)
    out = plan_from_counts(counts, cap, merge)
    out.update(lo=int(keys.min()), hi=int(keys.max()), bins=bins, counts=counts)
    return out


# ---- comb histograms ---------------------------------------------------------------------------------------------
def comb_levels(teeth, gap_records=1, gap_bins=1):
    """Records per depth level (int64[BINS]): teeth[i] records at level i * (1 + gap_bins), gap_records at each of the
    gap_bins levels between two teeth, and one record at the last level (so that level == bin, see comb_frame)."""
    step = 1 + gap_bins
    assert (len(teeth) - 1) * step < BINS - 1
    lv = np.zeros(BINS, dtype=np.int64)
    for i, c in enumerate(teeth):
        lv[i * step] = c
        if i + 1 < len(teeth):
            lv[i * step + 1:(i + 1) * step] = gap_records
    lv[BINS - 1] = 1
    return lv


COMB_CASES = {            # name -> records per level of the bucket in super-tile 0
    "comb40": lambda: comb_levels([897] * 40),
    "comb129": lambda: comb_levels([897] * 129),
    "comb244": lambda: comb_levels([897] * 244),
    "comb_896_897": lambda: comb_levels([896, 897] * 50),
    "comb_heavy": lambda: comb_levels([3585] * 40),
}
SECOND_COMB = lambda: comb_levels([897] * 60)          # noqa: E731   ("two_combs": super-tile 4)


def _level_depths(levels):
    return (np.uint32(LEVEL0_BITS) + np.uint32(LEVEL_STEP) * np.asarray(levels).astype(np.uint32)).view(np.float32)


def in_super_tile(m2, r, sx=0, sy=0):
    """Which Gaussians (m2 f32[N,2], r i32[N] > 0) have a tile rectangle that reaches super-tile (sx, sy) -- tiles 2 sx ..
    2 sx + 1 in x, likewise in y -- of the 6x6 grid of 16 px tiles: float32, as gsplat_oracle.tile_rects."""
    ts, tr = np.float32(16.0), r.astype(np.float32) / np.float32(16.0)
    lo = [np.clip(np.floor(m2[:, k] / ts - tr), 0, 6) for k in (0, 1)]
    hi = [np.clip(np.ceil(m2[:, k] / ts + tr), 0, 6) for k in (0, 1)]
    return ((lo[0] < 2 * sx + 2) & (hi[0] > 2 * sx) & (lo[1] < 2 * sy + 2) & (hi[1] > 2 * sy)
            & (hi[0] > lo[0]) & (hi[1] > lo[1]))


def comb_frame(levels_st0, levels_st4=None, n_neighbours=3000, seed=0):
    """A 6x6-tile frame (16 px tiles, one camera) whose super-tile 0 holds the comb `levels_st0` (records per depth
    level): radius-1 Gaussians with centres in [8, 24]^2, one record each.  levels_st4: a second comb in super-tile 4
    (centres in [40, 56]^2).  n_neighbours ordinary Gaussians (radii 1-5) over [0, 96]^2 follow; their depths sit on
    levels ABOVE the teeth (below the last level), a few per level, so that they neither move a bucket's lo / hi nor
    fill a gap of the comb.  Comb Gaussians are shuffled, so flat ids carry no order.
    -> means2d f32[1,N,2], radii i32[1,N], depths f32[1,N], and the flat ids of the Gaussians of each comb."""
    rng = np.random.default_rng(seed)
    combs = [(levels_st0, 8.0)] + ([(levels_st4, 40.0)] if levels_st4 is not None else [])
    lv_all, xy_all, owner = [], [], []
    top = 0
    for k, (levels, origin) in enumerate(combs):
        lv = np.repeat(np.arange(BINS), levels)
        top = max(top, int(np.flatnonzero(levels[:-1]).max()))
        lv_all.append(lv)
        xy_all.append(rng.uniform(origin, origin + 16.0, size=(len(lv), 2)))
        owner.append(np.full(len(lv), k))
    lv_c, xy_c, owner = np.concatenate(lv_all), np.concatenate(xy_all), np.concatenate(owner)
    perm = rng.permutation(len(lv_c))
    lv_c, xy_c, owner = lv_c[perm], xy_c[perm], owner[perm]
    lv_n = rng.integers(top + 1, BINS - 1, size=n_neighbours)
    m2 = np.concatenate([xy_c, rng.uniform(0.0, 96.0, size=(n_neighbours, 2))]).astype(np.float32)
    r = np.concatenate([np.ones(len(lv_c), dtype=np.int32), rng.integers(1, 6, size=n_neighbours).astype(np.int32)])
    d = _level_depths(np.concatenate([lv_c, lv_n]))
    ids = [np.flatnonzero(owner == k) for k in range(len(combs))]
    return m2[None], r[None], d[None], ids


def bucket_keys(m2, r, d, sx=0, sy=0):
    """The 60-bit keys of the records of super-tile (sx, sy) of a frame (one record per Gaussian that reaches it)."""
    inside = np.flatnonzero(in_super_tile(m2[0], r[0], sx, sy))
    return key60(d[0].view(np.uint32)[inside], inside)


def limit_frame(n_bucket, n_neighbours=3000, seed=0):
    """As comb_frame, with uniform depths in [1, 50) and EXACTLY n_bucket records in super-tile 0's bucket: the radius-1
    Gaussians of [8, 24]^2 plus the neighbours whose rectangles reach it."""
    rng = np.random.default_rng(seed)
    m2_n = rng.uniform(0.0, 96.0, size=(n_neighbours, 2)).astype(np.float32)
    r_n = rng.integers(1, 6, size=n_neighbours).astype(np.int32)
    n_in = n_bucket - int(in_super_tile(m2_n, r_n).sum())
    m2 = np.concatenate([rng.uniform(8.0, 24.0, size=(n_in, 2)).astype(np.float32), m2_n])
    r = np.concatenate([np.ones(n_in, dtype=np.int32), r_n])
    d = rng.uniform(1.0, 50.0, size=len(r)).astype(np.float32)
    return m2[None], r[None], d[None]
