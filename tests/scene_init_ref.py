"""The restatements street_crafter_amd/scene_init.py is judged against: numpy float64, never imported by the product.

open3d's source is not part of the reference, so these restate its two calls from their documented behaviour
(VoxelDownSample: hash map of voxel index -> accumulator, points added in input order; RemoveRadiusOutliers: nanoflann
radius search, strict `<` on squared distances, the query point counts).  test_scene_init_cpu.py pins the restatements
themselves: the voxel one against a literal dict loop, the radius one against scipy's cKDTree.
"""
from fractions import Fraction

import numpy as np

C0 = 0.28209479177387814


# ---- voxel down-sample ---------------------------------------------------------------------------------------------------
def voxel_index(xyz, v):
    """int64 [N,3]: floor((p - vmin) / v) with vmin = min_bound - 0.5 v; one subtraction and one division in float64."""
    xyz = np.asarray(xyz, dtype=np.float64)
    vmin = xyz.min(axis=0) - 0.5 * v
    return np.floor((xyz - vmin) / v).astype(np.int64)


def voxel_index_f32(xyz, v):
    """The same expressions evaluated in float32: what a float32 kernel would decide."""
    x = np.asarray(xyz, dtype=np.float64).astype(np.float32)
    v = np.float32(v)
    vmin = x.min(axis=0) - np.float32(0.5) * v
    return np.floor((x - vmin) / v).astype(np.int64)


def voxel_down_sample(xyz, colors, v):
    """(points f64[M,3], colors f64[M,3], counts i32[M]) in ascending (ix, iy, iz) order; the sums are sequential per
    voxel in input order (np.add.at is unbuffered and in order)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    colors = np.asarray(colors, dtype=np.float64)
    idx = voxel_index(xyz, v)
    uniq, inv = np.unique(idx, axis=0, return_inverse=True)         # rows sorted lexicographically
    inv = np.asarray(inv).reshape(-1)
    m = uniq.shape[0]
    sp, sc = np.zeros((m, 3)), np.zeros((m, 3))
    np.add.at(sp, inv, xyz)
    np.add.at(sc, inv, colors)
    counts = np.bincount(inv, minlength=m)
    return sp / counts[:, None].astype(np.float64), sc / counts[:, None].astype(np.float64), counts.astype(np.int32)


def voxel_down_sample_dict(xyz, colors, v):
    """open3d's algorithm, literally: one accumulator per voxel index in a dict, points added as the loop meets them."""
    xyz = np.asarray(xyz, dtype=np.float64)
    colors = np.asarray(colors, dtype=np.float64)
    vmin = xyz.min(axis=0) - 0.5 * v
    acc = {}
    for i in range(xyz.shape[0]):
        ref = (xyz[i] - vmin) / v
        key = (int(np.floor(ref[0])), int(np.floor(ref[1])), int(np.floor(ref[2])))
        a = acc.get(key)
        if a is None:
            a = acc[key] = [0, np.zeros(3), np.zeros(3)]
        a[0] += 1
        a[1] += xyz[i]
        a[2] += colors[i]
    keys = sorted(acc)
    pts = np.array([acc[k][1] / float(acc[k][0]) for k in keys])
    col = np.array([acc[k][2] / float(acc[k][0]) for k in keys])
    return pts, col, np.array([acc[k][0] for k in keys], dtype=np.int32)


# ---- radius outliers -------------------------------------------------------------------------------------------------------
def d2_unfused(a, b):
    """(dx dx + dy dy) + dz dz, every operation rounded (numpy never fuses)."""
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def radius_counts(xyz, radius, chunk=512):
    """int64 [M]: #{ j : d2(i, j) < r^2 }, i itself included; brute force."""
    xyz = np.asarray(xyz, dtype=np.float64)
    r2 = radius * radius
    out = np.empty(xyz.shape[0], dtype=np.int64)
    for s in range(0, xyz.shape[0], chunk):
        q = xyz[s:s + chunk]
        out[s:s + chunk] = (d2_unfused(q[:, None, :], xyz[None, :, :]) < r2).sum(axis=1)
    return out


def radius_outlier_mask(xyz, nb_points, radius):
    return radius_counts(xyz, radius) > nb_points


def min_relative_gap_to_r2(xyz, radius, chunk=512):
    """min over pairs of |d2 - r^2| / r^2: how far the cloud stays from the decision boundary."""
    xyz = np.asarray(xyz, dtype=np.float64)
    r2 = radius * radius
    best = np.inf
    for s in range(0, xyz.shape[0], chunk):
        q = xyz[s:s + chunk]
        best = min(best, float(np.abs(d2_unfused(q[:, None, :], xyz[None, :, :]) - r2).min()) / r2)
    return best


def _fma(a, b, c):
    """round(a b + c): exact in rationals, rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def d2_fused_variants(dx, dy, dz):
    """The two ways a contracting compiler evaluates (dx dx + dy dy) + dz dz."""
    return (_fma(dz, dz, _fma(dx, dx, dy * dy)), _fma(dz, dz, _fma(dy, dy, dx * dx)))


def adversarial_pairs(radius, want=8, seed=0, max_trials=4000):
    """[(dx, dy, dz, inside_unfused)]: offsets from the origin whose unfused d2 and BOTH fused evaluations fall on
    different sides of r^2.  dz is scanned over the doubles around sqrt(r^2 - dx^2 - dy^2)."""
    rng = np.random.default_rng(seed)
    r2 = radius * radius
    found = []
    for _ in range(max_trials):
        dx, dy = rng.uniform(0.1, 0.3, size=2) * radius * rng.choice([-1.0, 1.0], size=2)
        dz = float(np.sqrt(r2 - dx * dx - dy * dy))
        z = dz
        for _ in range(40):
            z = np.nextafter(z, 0.0)
        for _ in range(80):
            z = float(np.nextafter(z, np.inf))
            u = (dx * dx + dy * dy) + z * z
            if abs(u - r2) > 4 * np.spacing(r2):
                continue
            fused = d2_fused_variants(float(dx), float(dy), z)
            inside = u < r2
            if all((f < r2) != inside for f in fused):
                found.append((float(dx), float(dy), z, bool(inside)))
                break
        if len(found) >= want:
            break
    return found


# ---- first Gaussians -------------------------------------------------------------------------------------------------------
def init_scaling_f64(dist2_f32):
    """log(sqrt(max(dist2, 1e-7f))) in float64 on the float32 inputs."""
    d = np.maximum(np.asarray(dist2_f32, dtype=np.float32), np.float32(1e-7)).astype(np.float64)
    return np.log(np.sqrt(d))


def sphere_norm(xyz_f32, scale=1.0):
    """The bounding sphere of get_Sphere_Norm (street_gaussian/datasets/base_readers.py:79-91): centre = midpoint of the
    axis-aligned box, radius = half its diagonal times `scale`, in the dtype numpy gives float32 points."""
    pts = np.asarray(xyz_f32)
    hi, lo = pts.max(axis=0), pts.min(axis=0)
    half_diagonal = np.linalg.norm(hi - lo) / 2.0
    return (hi + lo) / 2, half_diagonal * scale


# ---- the clouds the tests share ------------------------------------------------------------------------------------------
RADIUS, NB_POINTS = 0.5, 10

# offsets (in lattice steps of 0.125) of nine points strictly inside r = 0.5 of a centre, and of six at exactly r
_STAR_NEAR = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]
_STAR_RIM = [(4, 0, 0), (-4, 0, 0), (0, 4, 0), (0, -4, 0), (0, 0, 4), (0, 0, -4)]


def radius_cloud(seed=0):
    """(xyz f64[M,3], tags): M close to 8000, every structure at least 2 away from the others.
    tags: name -> index array.  See test_scene_init_gpu.py for what each structure decides."""
    rng = np.random.default_rng(seed)
    parts, tags, at = [], {}, 0

    def add(name, pts):
        nonlocal at
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        parts.append(pts)
        tags[name] = np.concatenate([tags.get(name, np.zeros(0, dtype=np.int64)), np.arange(at, at + len(pts))])
        at += len(pts)

    # a uniform blob over 12^3 cells, all coordinates negative: counts on both sides of the threshold, neighbours in
    # every one of the 26 surrounding cells
    add("blob", rng.uniform(-9.0, -3.0, size=(5400, 3)))
    # clusters of exactly 10 and exactly 11 inside one radius
    for k in range(6):
        c = np.array([12.0 + 3.0 * k, -14.0, 5.0 - 3.0 * k])
        add("ten", c + rng.uniform(-0.1, 0.1, size=(10, 3)))
        add("eleven", c + np.array([0.0, 4.0, 0.0]) + rng.uniform(-0.1, 0.1, size=(11, 3)))
    # duplicates: d = 0
    add("dup10", np.tile([[5.25, 7.5, -2.125]], (10, 1)))
    add("dup12", np.tile([[-15.5, 9.0, 3.75]], (12, 1)))
    # a dyadic lattice block: many pairs at exactly d = r
    g = np.arange(12) * 0.125
    add("lattice", np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.array([8.0, 8.0, 8.0]))
    # stars: a centre with 9 points strictly inside and 6 at exactly r: the centre has 10 < r, 16 <= r
    for c in ([20.0, 0.0, 0.0], [-20.0, -3.0, 2.0], [0.0, -25.0, -7.5]):
        c = np.array(c)
        add("star_centre", c)
        add("star_near", c + 0.125 * np.array(_STAR_NEAR))
        add("star_rim", c + 0.125 * np.array(_STAR_RIM))
    # one crowded cell
    add("dense", np.array([3.0, -20.0, 11.0]) + rng.uniform(0.0, 0.3, size=(400, 3)))
    # an adversarial pair at the origin (dx, dy, dz exact): ten copies of the origin and the partner
    dx, dy, dz, _ = adversarial_pairs(RADIUS, want=1, seed=seed + 1)[0]
    add("adv_origin", np.zeros((10, 3)))
    add("adv_partner", [[dx, dy, dz]])
    # stragglers
    add("stragglers", rng.uniform(30.0, 60.0, size=(200, 3)) * rng.choice([-1.0, 1.0], size=(200, 3)))
    return np.concatenate(parts), tags


def lattice_sheet():
    """A 9 x 9 sheet of spacing 0.125 and the largest strict count in it: with nb_points = that count a strict filter
    keeps nothing, one that counts d = r keeps the middle."""
    g = np.arange(9) * 0.125
    xyz = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3) + np.array([-1.0, 2.0, 0.5])
    return xyz, int(radius_counts(xyz, RADIUS).max())


def voxel_cloud(kind, n=0, seed=0):
    """(xyz f64, colors f64, voxel_size) of the down-sampler's cases."""
    rng = np.random.default_rng([seed, n, len(kind)])
    if kind == "random":                    # a 1 m cube at 0.1: ~1000 voxels, so from a few hundred points voxels share
        xyz = rng.uniform(-0.5, 0.5, size=(n, 3)) * np.array([1.0, 1.0, 0.5]) + np.array([12.5, -7.25, 1.0])
        v = 0.1
    elif kind == "crowded":                 # 5000 points in one voxel (it starts at min - v / 2), 300 elsewhere
        xyz = np.concatenate([rng.uniform(0.0, 0.04, size=(5000, 3)), rng.uniform(0.5, 3.0, size=(300, 3))])
        xyz = xyz[rng.permutation(len(xyz))]
        v = 0.1
    elif kind == "alone":                   # a jittered lattice of spacing 0.25: every point in its own voxel
        g = np.arange(11) * 0.25
        xyz = np.stack(np.meshgrid(g, g, g[:5], indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.02, 0.02, size=(605, 3))
        xyz = xyz[rng.permutation(len(xyz))]
        v = 0.1
    elif kind == "dyadic":                  # v = 0.125; every (p - vmin) / v but the corner's is an exact integer
        v = 0.125
        base = np.array([-2.0, -1.5, -0.75])
        k = np.stack(np.meshgrid(np.arange(9), np.arange(7), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
        lat = base + 0.0625 + 0.125 * k
        xyz = np.concatenate([base[None], lat, lat[::3], lat[::5]])       # some voxels hold one point, some two or three
        xyz = xyz[rng.permutation(len(xyz))]
    elif kind == "offset":                  # world coordinates where float32 cannot hold the grid
        xyz = rng.uniform(0.0, 5.0, size=(3000, 3)) + np.array([3.0e4, -2.0e4, 50.0])
        v = 0.1
    else:
        raise KeyError(kind)
    return xyz, rng.uniform(0.0, 1.0, size=xyz.shape), v


def street_cloud(seed=0):
    """About 60 000 float64 points: a ground plane and two walls, each scanned several times with centimetre jitter,
    and 200 isolated stragglers."""
    rng = np.random.default_rng(seed)
    base_g = np.stack([rng.uniform(0.0, 30.0, 3000), rng.uniform(-3.0, 3.0, 3000), np.zeros(3000)], -1)
    base_l = np.stack([rng.uniform(0.0, 30.0, 1000), np.full(1000, 3.0), rng.uniform(0.0, 2.5, 1000)], -1)
    base_r = base_l * np.array([1.0, -1.0, 1.0])
    base = np.concatenate([base_g, base_l, base_r])
    sweeps = [base + rng.normal(scale=0.01, size=base.shape) for _ in range(12)]
    far = rng.uniform(10.0, 30.0, size=(200, 3)) * np.array([1.0, 1.0, 0.5]) + np.array([0.0, 10.0, 5.0])
    xyz = np.concatenate(sweeps + [far]) + np.array([1200.0, -350.0, 12.0])
    return xyz, rng.uniform(0.0, 1.0, size=xyz.shape)
