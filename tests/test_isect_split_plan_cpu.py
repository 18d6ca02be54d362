"""No-GPU checks of the RANGE PLAN by which the tile-bucketed isect_tiles route cuts an oversized super-tile bucket into
depth ranges (big_split_kernel, csrc/isect_bin.hip; the arithmetic is csrc/isect_split_plan.h, __host__ __device__).

The shipped arithmetic is driven through the host entries sc_isect_split_* and compared with the numpy restatement
oracle/split_plan.py; then the plan's invariants and its two bounds are asserted on every histogram:

  * R, the ranges of one bucket, fits the kernel's range tables for every bucket the split takes;
  * f(n_b) = 2 * floor(n_b / (cap + 1)) + 1 bounds R_b per bucket (any two neighbouring ranges hold more than cap
    records: the greedy merge opens a range only when the next group does not fit), and
    sum_b f(n_b) <= seg_bound_for(sum_b n_b, nsb) for any split of a frame's records over up to nsb oversized buckets,
    so no segment is ever left without a slot in the segment list.

COMBS (teeth of t records alternating with light bins) are the adversarial family: before the merge step existed a
tooth of cap / 4 + 1 records followed by one light record opened two ranges, ~2 n / 898 in all -- twice what the
tables and the segment list were sized for (test_the_groups_alone_cross_both_limits keeps that on record)."""
import ctypes

import numpy as np
import pytest

from oracle import split_plan as SP

NSB = 9               # super-tiles of the 6x6-tile frame of the GPU cases


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def limits(lib):
    out = (ctypes.c_int64 * 6)()
    assert lib.sc_isect_split_limits(ctypes.cast(out, ctypes.c_void_p)) == 0
    names = ("max_ranges", "max_bucket", "cap", "light_max", "target", "bins")
    return dict(zip(names, (int(v) for v in out)))


def _host_plan(lib, counts, cap):
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    rob = np.empty(len(c), dtype=np.int32)
    R = ctypes.c_int32(-1)
    assert lib.sc_isect_split_plan(c.ctypes.data, int(cap), rob.ctypes.data, ctypes.addressof(R)) == 0
    return int(R.value), rob


def _histograms(limits):
    """name -> bin counts (int64[1024], n in (cap, max_bucket]): the combs of the issue, combs around every threshold
    of the plan, the degenerate shapes and 3000 random sparse histograms."""
    cap, tgt, top = limits["cap"], limits["target"], limits["max_bucket"]
    out = {}
    for H in (18, 40, 129, 244):                                  # teeth of 897 + one record between them
        out[f"comb897x{H}"] = SP.comb_levels([897] * H)
    for t in (896, 897, 898, 1792, 1793, 3584, 3585):             # both sides of light_max, cap / 2, cap
        H = min(500, (top - 1) // (t + 1))
        out[f"teeth{t}"] = SP.comb_levels([t] * H)
        out[f"teeth{t}_few"] = SP.comb_levels([t] * 5)
    for t in (897, 3584, 3585):
        out[f"teeth{t}_gap0"] = SP.comb_levels([t] * min(1000, (top - 1) // t), gap_records=0, gap_bins=0)
        for gap_bins in (3, 4):                                   # light runs of ~target records between the teeth
            per = tgt // gap_bins
            H = min((SP.BINS - 2) // (1 + gap_bins), (top - 1) // (t + per * gap_bins))
            out[f"teeth{t}_gap{gap_bins}x{per}"] = SP.comb_levels([t] * H, gap_records=per, gap_bins=gap_bins)
    out["comb_896_897"] = SP.comb_levels([896, 897] * 50)
    out["all_light_flat"] = np.full(SP.BINS, top // SP.BINS, dtype=np.int64)
    for name, every in (("all_light_max", 1), ("all_light_max_sparse", 4)):     # bins of exactly light_max records
        c = np.zeros(SP.BINS, dtype=np.int64)
        c[: every * (top // limits["light_max"]): every] = limits["light_max"]
        out[name] = c
    k = (top - cap) // (cap + 1)                    # k + 1 teeth of cap records, one record between them: attains f(n)
    c = np.zeros(SP.BINS, dtype=np.int64)
    c[0:2 * k + 1:2], c[1:2 * k:2] = cap, 1
    out["attains_the_bound"] = c
    for n in (cap + 1, top):
        one = np.zeros(SP.BINS, dtype=np.int64)
        one[517] = n
        out[f"one_bin_{n}"] = one
    rng = np.random.default_rng(2024)
    for i in range(3000):
        n = int(rng.integers(cap + 1, top + 1))
        k = int(rng.integers(1, SP.BINS + 1)) if i % 3 else int(rng.integers(1, 40))     # non-empty bins
        where = rng.choice(SP.BINS, size=k, replace=False)
        # a few dominant bins + many small ones: heavy and light bins next to each other at every scale
        w = rng.random(k) ** float(rng.choice([1.0, 4.0, 16.0]))
        c = np.zeros(SP.BINS, dtype=np.int64)
        c[where] = rng.multinomial(n, w / w.sum())
        out[f"random{i}"] = c
    for name, c in out.items():
        assert cap < int(c.sum()) <= top, (name, int(c.sum()))
    return out


@pytest.fixture(scope="module")
def histograms(limits):
    return _histograms(limits)


@pytest.fixture(scope="module")
def plans(lib, limits, histograms):
    """name -> (n, R, range_of_bin) from the HOST ENTRY (the shipped arithmetic), computed once."""
    return {name: (int(c.sum()), *_host_plan(lib, c, limits["cap"])) for name, c in histograms.items()}


def test_limits_are_what_the_model_assumes(lib, limits):
    assert limits["cap"] == SP.CAP == lib.sc_isect_bin_bucket_capacity() and limits["bins"] == SP.BINS
    assert limits["light_max"] == SP.light_max() == 896 and limits["target"] == SP.target() == 2688
    assert limits["max_bucket"] > limits["cap"] and limits["max_ranges"] >= 1


def test_model_equals_the_host_entry(limits, histograms, plans):
    for name, c in histograms.items():
        n, R, rob = plans[name]
        m = SP.plan_from_counts(c, limits["cap"])
        assert R == m["R"], name
        np.testing.assert_array_equal(rob, m["range_of_bin"], err_msg=name)
        host_counts = np.bincount(rob[rob >= 0], weights=c[rob >= 0], minlength=R).astype(np.int64)
        np.testing.assert_array_equal(host_counts, m["range_counts"], err_msg=name)


def test_plan_invariants(limits, histograms, plans):
    cap = limits["cap"]
    for name, c in histograms.items():
        n, R, rob = plans[name]
        ne = np.flatnonzero(c)
        assert np.all(rob[c == 0] == -1), name
        ids = rob[ne]                              # ranges of the non-empty bins, in bin order
        assert ids[0] == 0 and ids[-1] == R - 1 and np.all((np.diff(ids) == 0) | (np.diff(ids) == 1)), name
        counts = np.bincount(ids, weights=c[ne], minlength=R).astype(np.int64)
        assert counts.sum() == n and np.all(counts > 0), name
        over = counts > cap                        # what the kernel flags `heavy`: the exact quadratic path
        bins_in = np.bincount(ids, minlength=R)
        assert np.all(bins_in[over] == 1), name    # ... is one bin that depth cannot cut, never a merge gone too far
        assert np.all(counts[~over] <= cap), name


def test_ranges_of_one_bucket_fit_the_range_tables(limits, plans):
    cap = limits["cap"]
    for name, (n, R, _) in plans.items():
        assert R <= SP.max_ranges(n, cap), (name, n, R)            # f(n_b)
        assert R <= limits["max_ranges"], (name, n, R)
    assert SP.max_ranges(limits["max_bucket"], cap) <= limits["max_ranges"]     # ... and for every n the split takes
    # the bound is attained (teeth of cap records + one record between them), so it cannot be tightened
    n, R, _ = plans["attains_the_bound"]
    assert R == SP.max_ranges(n, cap)


def test_segments_of_a_frame_fit_the_segment_list(lib, limits, plans):
    cap = limits["cap"]
    f = lambda n: SP.max_ranges(n, cap)            # noqa: E731
    seg_bound = lambda n, nsb: int(lib.sc_isect_split_seg_bound(int(n), int(nsb)))     # noqa: E731
    names = sorted(plans, key=lambda k: plans[k][1] / plans[k][0], reverse=True)       # most ranges per record first
    rng = np.random.default_rng(7)
    frames = [[k] for k in names]                                                      # 1 bucket
    for nb in (2, NSB):                                                                # 2 and nsb buckets at once
        frames += [names[i:i + nb] for i in range(0, 5 * nb, nb)]                      # the worst together
        frames += [list(rng.choice(names, size=nb)) for _ in range(400)]
    for frame in frames:
        n_frame = sum(plans[k][0] for k in frame)
        segs = sum(plans[k][1] for k in frame)
        bound = sum(f(plans[k][0]) for k in frame)
        # exact sizes (rec_capacity = the frame's records), and any larger prediction: the bound only grows
        assert segs <= bound <= seg_bound(n_frame, NSB) <= seg_bound(n_frame + n_frame // 8 + 4096, NSB), frame
    # f summed over ANY split of n records over up to nsb buckets: 2 * sum floor(n_b / (cap + 1)) + nsb
    for _ in range(2000):
        nb = int(rng.integers(1, NSB + 1))
        ns = rng.integers(cap + 1, limits["max_bucket"] + 1, size=nb)
        assert sum(f(int(n)) for n in ns) <= seg_bound(int(ns.sum()), NSB)
    assert seg_bound(0, NSB) >= 0 and lib.sc_isect_split_seg_bound(10, -1) < 0


def test_the_groups_alone_cross_both_limits(lib, limits):
    """What the merge step is for: the plan WITHOUT it (groups as ranges, oracle/split_plan.py merge=False -- the kernel
    as it was) on the combs.  36 k records already need more segments than the list has; from 116 k on the ranges
    outgrow the 256-entry tables."""
    rows = {}
    for H in (18, 40, 129, 244):
        c = SP.comb_levels([897] * H)
        old = SP.plan_from_counts(c, limits["cap"], merge=False)
        rows[H] = (int(c.sum()), old["R"], SP.plan_from_counts(c, limits["cap"])["R"])
        assert old["R"] == 2 * H
    assert rows[244][:2] == (219112, 488)
    assert rows[129][1] > limits["max_ranges"] and rows[244][1] > limits["max_ranges"]
    old_seg_bound = lambda n: 2 * n // (limits["cap"] // 2) + NSB + 8          # noqa: E731   (as it was)
    assert rows[40][1] > old_seg_bound(rows[40][0]) and rows[18][1] > old_seg_bound(rows[18][0])
    for n, _, R in rows.values():
        assert R <= SP.max_ranges(n, limits["cap"]) <= lib.sc_isect_split_seg_bound(n, NSB)


# ---- the frames of the GPU cases (tests/test_gpu_parity.py::test_isect_bin_comb_*) -----------------------------------
@pytest.mark.parametrize("case", sorted(SP.COMB_CASES) + ["two_combs"])
def test_fixture_levels_land_in_their_bins(lib, limits, case):
    """Level m of the fixture's depths lands in bin m for every flat id in use -- shipped bin_of and the model's -- so
    the bucket's histogram is the comb it claims to be, and its plan is the one the CPU tests above have judged."""
    levels = SP.COMB_CASES["comb40" if case == "two_combs" else case]()
    m2, r, d, ids = SP.comb_frame(levels, SP.SECOND_COMB() if case == "two_combs" else None)
    if case == "two_combs":                         # the second comb's bucket is one too
        k4 = SP.bucket_keys(m2, r, d, 1, 1)
        np.testing.assert_array_equal(np.bincount(SP.bin_of(k4), minlength=SP.BINS)[:119], SP.SECOND_COMB()[:119])
    keys = SP.bucket_keys(m2, r, d)
    lo, hi = int(keys.min()), int(keys.max())
    level = (keys >> np.uint64(SP.ID_BITS)).astype(np.int64) - SP.LEVEL0_BITS
    assert np.all(level % SP.LEVEL_STEP == 0)
    level //= SP.LEVEL_STEP
    assert level.min() == 0 and level.max() == SP.BINS - 1
    bins = np.empty(len(keys), dtype=np.int32)
    assert lib.sc_isect_split_bins(np.ascontiguousarray(keys).ctypes.data, len(keys), lo, hi, bins.ctypes.data) == 0
    np.testing.assert_array_equal(bins, level)
    np.testing.assert_array_equal(SP.bin_of(keys), level)
    # the comb is there: the teeth as built, the neighbours only above them, a few per level
    counts = np.bincount(level, minlength=SP.BINS)
    teeth = np.flatnonzero(levels[:-1])
    np.testing.assert_array_equal(counts[: teeth.max() + 1], levels[: teeth.max() + 1])
    assert counts[teeth.max() + 1:].max() <= 8 and counts.sum() == len(keys) > levels.sum()
    p = SP.plan(keys, limits["cap"])
    R, rob = _host_plan(lib, counts, limits["cap"])
    assert R == p["R"] <= SP.max_ranges(len(keys), limits["cap"])
    np.testing.assert_array_equal(rob, p["range_of_bin"])
    if case == "comb_heavy":
        assert int(p["heavy"].sum()) == 40          # every tooth takes the quadratic path


def test_limit_frame_has_exactly_the_records_it_claims(limits):
    from oracle import gsplat_oracle as O
    for n in (limits["cap"] + 1, 20000):
        m2, r, d = SP.limit_frame(n)
        x0, x1, y0, y1 = O.tile_rects(m2, r, 16, 6, 6)
        assert int(((x0 < 2) & (y0 < 2) & (x1 > x0) & (y1 > y0)).sum()) == n
