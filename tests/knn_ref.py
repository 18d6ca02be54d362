"""Reference for distCUDA2 (street_crafter_amd/csrc/knn.hip) at sizes the brute-force oracle cannot reach, in numpy.

oracle/knn_oracle.py compares every point with every other: O(n^2), 20 s at 32 769 points.  The kernel's hierarchy has
levels of 32 / 1024 / 32 768 / 1 048 576 points, so the sizes that matter lie beyond that.  clustered() builds a cloud
whose exact answer costs O(n m): tight clusters of m points on a lattice whose pitch is several cluster diameters, so a
point's three nearest others are always members of its own cluster and ref_clustered() finds them by brute force inside
the cluster, in float32 and in the oracle's operation order -- bit for bit what dist_cuda2 would give
(test_knn_ref_cpu.py checks that where dist_cuda2 is affordable).

The lattice is centred on 0 with an odd side, so a layer of cluster centres lies on each mid-plane of the bounding
box, where the top bits of the Morton code flip: the members of such a cluster land far apart on the curve, in
different boxes of every level.  A walk that prunes a box it must not prune loses their neighbours.  curve_pos()
restates the kernel's curve so that the tests can certify this of the cloud they use; it is never an expectation.
"""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)

# the large cloud of test_knn_gpu.py, certified by test_knn_ref_cpu.py: three top-level boxes (2^20, 2^20 and 33 points)
LARGE = dict(n=2 * 2 ** 20 + 33, m=40, seed=3, pitch=8.0)

LEVEL_POINTS = (32, 1024, 32768, 1 << 20)       # points per box of levels 0..3 of knn.hip's hierarchy


def clustered(n, m, seed, pitch=8.0):
    """-> points f32[n,3], cluster i64[n].  n // m clusters of m points, the remainder n % m in the last one; each
    point is its cluster's centre plus a jitter uniform in +-0.5 per axis.  Centres take distinct sites of a cubic
    lattice of odd side, centred on 0.  The rows are shuffled."""
    if m < 4 or n < m:
        raise ValueError(f"every cluster needs at least 4 points (n={n}, m={m})")
    rng = np.random.default_rng(seed)
    g = n // m
    side = 1
    while side ** 3 < g:
        side += 2
    sites = rng.permutation(side ** 3)[:g]
    ijk = np.stack(np.unravel_index(sites, (side, side, side)), axis=1)
    centres = (ijk - (side - 1) // 2).astype(np.float64) * pitch
    cluster = np.minimum(np.arange(n) // m, g - 1)
    pts = (centres[cluster] + rng.uniform(-0.5, 0.5, size=(n, 3))).astype(np.float32)
    order = rng.permutation(n)
    return np.ascontiguousarray(pts[order]), cluster[order]


def ref_clustered(points, cluster, allow=None, chunk=2048):
    """distCUDA2 of a clustered() cloud -> f32[n]: for every point the three smallest float32 distances
    (dx*dx + dy*dy) + dz*dz to the OTHER members of its cluster (self excluded by index), then ((b0 + b1) + b2) / 3.

    Exact only while every point's three nearest others are in its own cluster, which needs at least 4 members per
    cluster (ValueError otherwise) and clusters further apart than they are wide (separation()).

    `allow(i, j) -> bool`, given broadcastable arrays of row numbers, restricts the candidates j of point i: the tests
    use it to simulate a walk that fails to visit part of the cloud.  A missing candidate contributes FLT_MAX."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    n = p.shape[0]
    order = np.argsort(cluster, kind="stable")
    ids, counts = np.unique(np.asarray(cluster)[order], return_counts=True)
    if counts.min() < 4:
        raise ValueError(f"cluster {int(ids[counts.argmin()])} has {int(counts.min())} points: its neighbours are not its own")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    out = np.empty(n, dtype=np.float32)
    for size in np.unique(counts):
        first = starts[counts == size]
        for s in range(0, first.shape[0], chunk):
            rows = order[first[s:s + chunk, None] + np.arange(size)[None, :]]       # [G, size] row numbers
            q = p[rows]
            dx = q[:, :, None, 0] - q[:, None, :, 0]
            dy = q[:, :, None, 1] - q[:, None, :, 1]
            dz = q[:, :, None, 2] - q[:, None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            keep = ~np.eye(size, dtype=bool)[None]
            if allow is not None:
                keep = keep & allow(rows[:, :, None], rows[:, None, :])
            d2 = np.where(keep & (d2 < FLT_MAX), d2, FLT_MAX)
            best = np.partition(d2, 2, axis=2)[:, :, :3]
            best.sort(axis=2)
            with np.errstate(over="ignore"):
                out[rows] = ((best[..., 0] + best[..., 1]) + best[..., 2]) / np.float32(3.0)
    return out


def separation(points, cluster):
    """-> (widest, nearest): an upper bound on the distance between two members of one cluster and a lower bound on
    the distance between members of two clusters, from each cluster's centre (the middle of its bounding box) and
    radius.  ref_clustered is exact while nearest > widest."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, dtype=np.float64)
    order = np.argsort(cluster, kind="stable")
    _, first = np.unique(np.asarray(cluster)[order], return_index=True)
    lo = np.minimum.reduceat(p[order], first, axis=0)
    hi = np.maximum.reduceat(p[order], first, axis=0)
    radius = float(np.linalg.norm((hi - lo) / 2, axis=1).max())
    centre = (lo + hi) / 2
    if centre.shape[0] < 2:
        return 2 * radius, np.inf
    d, _ = cKDTree(centre).query(centre, k=2)
    return 2 * radius, float(d[:, 1].min()) - 2 * radius


def _spread10(x):
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    x = (x | (x << 2)) & 0x09249249
    return x


def curve_pos(points):
    """Position of every point on the kernel's Morton curve -> i64[n]: knn_morton_kernel in float32 (bounding box,
    q = uint(clamp((p - lo) / ext, 0, 1) * 1023) per axis, 30-bit interleave), then a stable sort of the keys.
    Point i is in box curve_pos(points)[i] // LEVEL_POINTS[k] of level k."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    n = p.shape[0]
    key = np.zeros(n, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(3):
            lo, hi = np.fmin.reduce(p[:, a]), np.fmax.reduce(p[:, a])       # fminf / fmaxf: a NaN is ignored
            ext = np.float32(hi - lo)
            r = (p[:, a] - lo) / ext if ext > 0 else np.zeros(n, dtype=np.float32)
            r = np.fmin(np.fmax(r, np.float32(0)), np.float32(1))           # NaN -> 0
            q = (r * np.float32(1023.0)).astype(np.uint32)
            key |= _spread10(q) << np.uint32(a)
    pos = np.empty(n, dtype=np.int64)
    pos[np.argsort(key, kind="stable")] = np.arange(n)
    return pos


def straddlers(cluster, pos, level, adjacent_counts=True):
    """How many clusters have members in different boxes of `level`; with adjacent_counts=False only clusters whose
    boxes are at least two apart, so that a walk which also looks at the next box on the curve would still miss."""
    box = pos // LEVEL_POINTS[level]
    order = np.argsort(cluster, kind="stable")
    _, first = np.unique(np.asarray(cluster)[order], return_index=True)
    span = np.maximum.reduceat(box[order], first) - np.minimum.reduceat(box[order], first)
    return int((span >= (1 if adjacent_counts else 2)).sum())


def ckdtree_mean_dist2(points, workers=16):
    """float64 mean squared distance to the 3 nearest other points, by scipy's exact k-NN."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, dtype=np.float64)
    d, _ = cKDTree(p).query(p, k=4, workers=workers)
    return (d[:, 1:] ** 2).mean(axis=1)
