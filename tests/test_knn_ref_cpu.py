"""No-GPU checks of what test_knn_gpu.py stands on: the closed-form reference of tests/knn_ref.py against the brute-force
oracle and cKDTree, the properties of the large cloud that make it a test (clusters that straddle boxes of every level;
three simulated broken walks that it catches), and the oracle's rule for distances that are not finite."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as ref  # noqa: E402
from oracle import knn_oracle as KO  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the closed form is the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,pitch", [(5000, 8, 64.0), (4099, 37, 64.0), (20000, 64, 64.0),
                                       (4099, 37, 8.0), (20000, 40, 8.0)])
def test_ref_clustered_equals_the_oracle_bit_for_bit(n, m, pitch):
    pts, cl = ref.clustered(n, m, seed=1, pitch=pitch)
    assert pts.dtype == np.float32 and pts.shape == (n, 3) and np.bincount(cl).min() >= 4
    assert np.bincount(cl)[-1] == m + n % m                      # the remainder joins the last cluster
    np.testing.assert_array_equal(_bits(ref.ref_clustered(pts, cl)), _bits(KO.dist_cuda2(pts)))


def test_ref_clustered_agrees_with_ckdtree():
    pts, cl = ref.clustered(20000, 40, seed=2)
    np.testing.assert_allclose(ref.ref_clustered(pts, cl), ref.ckdtree_mean_dist2(pts), rtol=3e-5, atol=1e-9)


def test_ref_clustered_refuses_a_cluster_of_fewer_than_four():
    """A 3-point cluster's third neighbour lives in another cluster: the closed form does not hold and says so."""
    pts, cl = ref.clustered(403, 40, seed=4)
    with pytest.raises(ValueError):
        ref.clustered(403, 3, seed=4)
    cut = np.flatnonzero(cl == cl.max())[3:]                       # leave 3 members in the last cluster
    keep = np.setdiff1d(np.arange(403), cut)
    with pytest.raises(ValueError):
        ref.ref_clustered(pts[keep], cl[keep])
    # why: the oracle's answer for those three rows reaches into another cluster, more than the lattice gap away
    _, nearest = ref.separation(pts[keep], cl[keep])
    assert (KO.dist_cuda2(pts[keep])[cl[keep] == cl.max()] > nearest ** 2 / 3).all()


def test_curve_pos_is_a_permutation_and_follows_the_morton_order():
    pts = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], dtype=np.float32)
    # x is bit 0, y bit 1, z bit 2 of every triple; equal keys keep their input order
    np.testing.assert_array_equal(ref.curve_pos(pts), [0, 5, 2, 3, 4, 1])
    pts, _ = ref.clustered(4099, 37, seed=1)
    np.testing.assert_array_equal(np.sort(ref.curve_pos(pts)), np.arange(4099))
    with_nan = np.concatenate([pts, [[np.nan, 0, 0]], [[np.inf, 0, 0]]]).astype(np.float32)
    assert np.sort(ref.curve_pos(with_nan))[-1] == 4100


# ---- the large cloud of the GPU module --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    pts, cl = ref.clustered(**ref.LARGE)
    return dict(pts=pts, cl=cl, pos=ref.curve_pos(pts), want=ref.ref_clustered(pts, cl))


def test_large_cloud_fills_the_hierarchy_and_straddles_every_level(large):
    n = ref.LARGE["n"]
    assert -(-n // ref.LEVEL_POINTS[3]) == 3 and n % ref.LEVEL_POINTS[3] == 33      # 2^20 + 2^20 + (32 + 1) points
    assert np.bincount(large["cl"]).min() >= 4
    widest, nearest = ref.separation(large["pts"], large["cl"])
    assert nearest > widest, (nearest, widest)
    for level in (1, 2, 3):
        assert ref.straddlers(large["cl"], large["pos"], level) >= 100
    # beyond the next box on the curve, too: a walk that looks one box to either side would still lose neighbours
    for level in (1, 2):
        assert ref.straddlers(large["cl"], large["pos"], level, adjacent_counts=False) >= 100


@pytest.mark.parametrize("walk", ["own_top_box", "own_32768_box", "own_leaf_and_curve_neighbours"])
def test_large_cloud_catches_a_broken_walk(large, walk):
    """A walk that never leaves the point's own box of a level (or its leaf and the +-3 curve neighbours the kernel
    starts from) must come out different on at least 100 rows: a cloud on which it passes is not a test."""
    pos = large["pos"]
    if walk == "own_top_box":
        box = pos // ref.LEVEL_POINTS[3]
        allow = lambda i, j: box[i] == box[j]                                         # noqa: E731
    elif walk == "own_32768_box":
        box = pos // ref.LEVEL_POINTS[2]
        allow = lambda i, j: box[i] == box[j]                                         # noqa: E731
    else:
        leaf = pos // ref.LEVEL_POINTS[0]
        allow = lambda i, j: (leaf[i] == leaf[j]) | (np.abs(pos[i] - pos[j]) <= 3)    # noqa: E731
    broken = ref.ref_clustered(large["pts"], large["cl"], allow=allow)
    assert int((_bits(broken) != _bits(large["want"])).sum()) >= 100


# ---- the oracle on distances that are not finite ----------------------------------------------------------------------
def test_oracle_never_inserts_an_infinite_or_nan_distance():
    """simple-knn starts from FLT_MAX and inserts only d < best: a +inf or NaN distance is no candidate, and a row
    with fewer than three candidates keeps FLT_MAX terms as a cloud of fewer than 4 points does."""
    F = KO.FLT_MAX
    third = lambda *b: ((np.float32(b[0]) + np.float32(b[1])) + np.float32(b[2])) / np.float32(3.0)   # noqa: E731
    # overflow: three points 1e14 apart at +3e19, one at -3e19: d^2 between the groups is +inf in float32
    a = np.float32(3e19)
    s = np.float32(2.0 ** 47)
    pts = np.array([[a, 0, 0], [a + s, 0, 0], [a + 2 * s, 0, 0], [-a, 0, 0]], dtype=np.float32)
    with np.errstate(over="ignore"):
        got = KO.dist_cuda2(pts)
        s2 = s * s
        want = np.array([third(s2, 4 * s2, F), third(s2, s2, F), third(s2, 4 * s2, F), third(F, F, F)], dtype=np.float32)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert np.isfinite(got[:3]).all() and got[3] == np.inf
    # NaN and infinite rows: +inf for themselves, invisible to the others
    rng = np.random.default_rng(0)
    fin = rng.normal(size=(50, 3)).astype(np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.inf, 1]], dtype=np.float32)
    mixed = np.concatenate([fin[:20], bad[:2], fin[20:], bad[2:]])
    got = KO.dist_cuda2(mixed)
    is_bad = ~np.isfinite(mixed).all(axis=1)
    np.testing.assert_array_equal(_bits(got[~is_bad]), _bits(KO.dist_cuda2(fin)))
    assert (got[is_bad] == np.inf).all()
    # fewer than three finite candidates because the others are NaN rows
    few = np.concatenate([fin[:3], bad])
    np.testing.assert_array_equal(_bits(KO.dist_cuda2(few)[:3]), _bits(KO.dist_cuda2(fin[:3])))
