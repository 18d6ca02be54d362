"""Reference and exact frames for the LiDAR point render (csrc/point_raster.hip), numpy only, no GPU.

Written from the contract text of `sc_point_project` / `sc_point_rasterize_fwd` in include/street_crafter_amd.h, not from
the kernels.  tests/test_point_raster_ref_cpu.py judges this file on its own; tests/test_point_raster_walk_gpu.py and
tests/test_point_render_exact_gpu.py hold the kernels to it.

blend_f64          the contract's per-pixel walk in float64, with per-pixel hits and magnitude sums S
blend_f32_replay   the same walk in numpy float32, every product and sum rounded separately, in the kernel's order
                       w = T*a;  c += w*col;  dz += w*z;  T = T*(1-a);   then  c + T*bg  and  1 - T
                   (point_raster.hip is compiled with fp contract(off), so this is its arithmetic bit for bit)
project_f64        the header's expressions for sc_point_project in float64, left to right (knn radius rule in float32)
lists_from         the tile binning from its definition, sorted by (tile, fp32 depth bits, index)
assert_exact       the conditions under which every coverage decision is the same in fp32 and in float64, so that NO
                   pixel has to be left out of a verdict
walk_cases         hand-built records + lists for the blend kernel alone (40 x 24: 3 x 2 tiles, the right column 8 pixels
                   wide, the bottom row 8 rows high: strips 2 and 3 of the bottom tiles lie wholly below the image)
scene_runs         whole-pipeline scenes on the lattice: camera = axis permutation + integer translation, fx = fy = 64,
                   z in {2, 4, 8, 16}, u and v multiples of 1/8, r dyadic

The float64 bar.  For a pixel with h hits, S = sum of the magnitudes of the blended terms (T a |rgb| per hit, + T |bg|):
    |float32 walk - float64 walk| <= 2^-24 (3h + 4) S   for rgb and depth,      <= 2^-24 (2h + 2)   for alpha.
T_i (the transmittance before hit i) is a product of 2i rounded factors (1 - a and the product, each one rounding);
w = T a and w c add one rounding each: 2i + 2 <= 2h roundings on term i.  The h-term sum adds at most h - 1 more to
any term, the background term T bg and its addition 2: at most 3h + 1 first-order roundings of 2^-24 on any term, and
the second-order terms ((1 + 2^-24)^(3h+1) - 1 - (3h+1) 2^-24 < 2^-24 for h <= 1000) sit inside the + 4.  Alpha = 1 - T:
2h roundings on T <= 1, one for the subtraction, + 1 for the second order.
"""
import numpy as np

TILE = 16
EPS24 = 2.0 ** -24
W0, H0 = 40, 24
F32 = np.float32


def tiles_of(W, H):
    return -(-W // TILE), -(-H // TILE)


def tile_pixels(t, W, H):
    """-> (x0, x1, y0, y1), inclusive, the tile's pixels inside the image."""
    tw, _ = tiles_of(W, H)
    ty, tx = divmod(t, tw)
    return tx * TILE, min(tx * TILE + TILE, W) - 1, ty * TILE, min(ty * TILE + TILE, H) - 1


def list_range(offsets, n_isects, t):
    offsets = np.asarray(offsets).reshape(-1)
    return int(offsets[t]), int(offsets[t + 1]) if t + 1 < offsets.size else int(n_isects)


# ---- the walk -----------------------------------------------------------------------------------------------------------
def _walk(records, offsets, flatten_ids, n_isects, W, H, max_hit, bg, dt):
    rec = np.asarray(records, np.float32).reshape(-1, 8).astype(dt)        # the record's fp32 values, taken as exact
    ids = np.asarray(flatten_ids).reshape(-1)
    tw, th = tiles_of(W, H)
    assert np.asarray(offsets).size == tw * th
    T = np.ones((H, W), dt)
    c = np.zeros((H, W, 3), dt)
    d = np.zeros((H, W), dt)
    hits = np.zeros((H, W), np.int64)
    S_rgb = np.zeros((H, W, 3), np.float64)
    S_d = np.zeros((H, W), np.float64)
    one, half = dt(1), dt(0.5)
    for t in range(tw * th):
        s, e = list_range(offsets, n_isects, t)
        x0, x1, y0, y1 = tile_pixels(t, W, H)
        ys, xs = slice(y0, y1 + 1), slice(x0, x1 + 1)
        px = np.arange(x0, x1 + 1).astype(dt) + half
        py = np.arange(y0, y1 + 1).astype(dt) + half
        for i in range(s, e):
            u, v, r2, z, cr, cg, cb, a = rec[ids[i]]
            dx, dy = px - u, py - v
            live = ((dx * dx)[None, :] + (dy * dy)[:, None] <= r2) & (hits[ys, xs] < max_hit)
            if not live.any():
                continue
            w = T[ys, xs] * a
            for k, col in enumerate((cr, cg, cb)):
                term = w * col
                c[ys, xs, k] = np.where(live, c[ys, xs, k] + term, c[ys, xs, k])
                S_rgb[ys, xs, k] += np.where(live, np.abs(term.astype(np.float64)), 0.0)
            term = w * z
            d[ys, xs] = np.where(live, d[ys, xs] + term, d[ys, xs])
            S_d[ys, xs] += np.where(live, np.abs(term.astype(np.float64)), 0.0)
            T[ys, xs] = np.where(live, T[ys, xs] * (one - a), T[ys, xs])
            hits[ys, xs] += live
    b = np.zeros(3, dt) if bg is None else np.asarray(bg, np.float32).astype(dt)
    tb = T[..., None] * b
    return {"rgb": c + tb, "alpha": one - T, "depth": d, "hits": hits, "T": T,
            "S_rgb": S_rgb + np.abs(tb.astype(np.float64)), "S_depth": S_d}


def blend_f64(records, offsets, flatten_ids, n_isects, W, H, max_hit, bg=None):
    return _walk(records, offsets, flatten_ids, n_isects, W, H, max_hit, bg, np.float64)


def blend_f32_replay(records, offsets, flatten_ids, n_isects, W, H, max_hit, bg=None):
    return _walk(records, offsets, flatten_ids, n_isects, W, H, max_hit, bg, np.float32)


def judge(rgb, alpha, depth, ref64, what=""):
    """Asserts the float64 bars on every pixel (rgb [H,W,3], alpha [H,W], depth [H,W] or None); -> the largest
    |got - f64| / bar reached (pixels whose bar is 0 must be equal and count as 0)."""
    h = ref64["hits"].astype(np.float64)
    worst = 0.0
    pairs = [("rgb", rgb, ref64["rgb"], EPS24 * (3 * h + 4)[..., None] * ref64["S_rgb"]),
             ("alpha", alpha, ref64["alpha"], EPS24 * (2 * h + 2))]
    if depth is not None:
        pairs.append(("depth", depth, ref64["depth"], EPS24 * (3 * h + 4) * ref64["S_depth"]))
    for name, got, want, bar in pairs:
        err = np.abs(np.asarray(got, np.float64) - want)
        bad = err > bar
        assert not bad.any(), f"{what} {name}: {int(bad.sum())} pixels over the bar, first {np.argwhere(bad)[0]}, " \
                              f"err {err[bad].max():.3e}"
        pos = bar > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bar[pos]).max()))
    return worst


# ---- sc_point_project ---------------------------------------------------------------------------------------------------
def project_f64(points, colors, opacities, occ, radius_in, viewmat, fx, fy, cx, cy, focal_r, near, far, mode, scale,
                knn_scale_down, H, W):
    """-> dict keep, u, v, z, r, r2 (float64), R = radii (int64), a (float32).  `colors` is unused by the geometry and
    taken only to mirror the entry point."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    m = np.asarray(viewmat, np.float64).reshape(4, 4)
    n = p.shape[0]
    with np.errstate(all="ignore"):
        x = m[0, 0] * p[:, 0] + m[0, 1] * p[:, 1] + m[0, 2] * p[:, 2] + m[0, 3]
        y = m[1, 0] * p[:, 0] + m[1, 1] * p[:, 1] + m[1, 2] * p[:, 2] + m[1, 3]
        z = m[2, 0] * p[:, 0] + m[2, 1] * p[:, 1] + m[2, 2] * p[:, 2] + m[2, 3]
        u = fx * x / z + cx
        v = fy * y / z + cy
        if mode == 1:
            world_r = scale * z / focal_r * (0.5 * min(H, W))
        elif mode == 2:
            rin = np.asarray(radius_in, np.float32).reshape(-1)
            world_r = np.minimum(np.sqrt(np.maximum(rin, F32(1e-7))) * F32(knn_scale_down), F32(scale)).astype(np.float64)
        elif mode == 3:
            world_r = np.asarray(radius_in, np.float32).reshape(-1).astype(np.float64) * scale
        else:
            world_r = np.full(n, float(scale))
        r = world_r * focal_r / z
        a = np.full(n, occ, np.float32) if opacities is None else np.asarray(opacities, np.float32).reshape(-1)
        fin = np.isfinite(u.astype(np.float32)) & np.isfinite(v.astype(np.float32)) & np.isfinite(r.astype(np.float32))
        keep = (z > max(near, 0.0)) & (z < far) & fin & (r >= 0) & (a > 0) & (a <= 1)
        R = np.where(keep, np.maximum(np.ceil(np.minimum(np.where(keep, r, 0.0), 2.0 ** 30)), 1.0), 0.0).astype(np.int64)
    return {"keep": keep, "u": u, "v": v, "z": z, "r": r, "r2": r * r, "R": R, "a": a}


def records_from(proj, colors):
    """The fp32 records of the kept points' projection (every field rounded once from float64)."""
    with np.errstate(all="ignore"):
        return np.concatenate([np.stack([proj["u"], proj["v"], proj["r2"], proj["z"]], 1).astype(np.float32),
                               np.asarray(colors, np.float32).reshape(-1, 3), proj["a"][:, None]], 1)


# ---- tile binning -------------------------------------------------------------------------------------------------------
def point_tiles(u, v, R, W, H):
    """Tiles [x0, x1) x [y0, y1) that intersect the pixel rectangle of centre (u, v) and half-width R."""
    tw, th = tiles_of(W, H)
    x0 = int(min(max(np.floor((u - R) / TILE), 0), tw))
    x1 = int(min(max(np.ceil((u + R) / TILE), 0), tw))
    y0 = int(min(max(np.floor((v - R) / TILE), 0), th))
    y1 = int(min(max(np.ceil((v + R) / TILE), 0), th))
    return x0, x1, y0, y1


def lists_from(u, v, R, z, W, H):
    """u, v, z: the fp32 values the binning reads; R int radii (0 = not listed).  -> (offsets i32[th*tw], flatten_ids
    i32[I], I)."""
    tw, th = tiles_of(W, H)
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    zb = np.asarray(z, np.float32).view(np.uint32).astype(np.int64)
    ent = []
    for i in range(len(u)):
        if R[i] <= 0:
            continue
        x0, x1, y0, y1 = point_tiles(u[i], v[i], float(R[i]), W, H)
        ent += [(ty * tw + tx, int(zb[i]), i) for ty in range(y0, y1) for tx in range(x0, x1)]
    ent.sort()
    tiles = np.array([e[0] for e in ent], np.int64)
    offsets = np.searchsorted(tiles, np.arange(tw * th), side="left").astype(np.int32)
    return offsets, np.array([e[2] for e in ent], np.int32), len(ent)


def covered_tiles(u, v, r2, W, H):
    """Brute force: the tiles that hold a pixel centre with d^2 <= r^2 (float64)."""
    tw, _ = tiles_of(W, H)
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    cov = (xs - u) ** 2 + (ys - v) ** 2 <= r2
    yy, xx = np.nonzero(cov)
    return set((yy // TILE * tw + xx // TILE).tolist())


def cull_survivors(case, t, rows=None):
    """Per entry of tile t's list: does the record pass the cull against the pixel-centre rectangle of the tile (or of
    its rows `rows` = (first, last) relative to the tile), i.e. ex^2 + ey^2 <= r^2 with (ex, ey) the distance from the
    centre to that rectangle (float64, exact on these frames)."""
    W, H = case["W"], case["H"]
    x0, x1, y0, y1 = tile_pixels(t, W, H)
    if rows is not None:
        y0, y1 = y0 + rows[0], min(y0 + rows[1], y1)
    s, e = list_range(case["offsets"], case["n_isects"], t)
    rec = case["records"].astype(np.float64)[case["flatten_ids"][s:e]]
    if y1 < y0:
        return np.zeros(e - s, bool)
    ex = np.maximum(np.maximum(x0 + 0.5 - rec[:, 0], rec[:, 0] - (x1 + 0.5)), 0)
    ey = np.maximum(np.maximum(y0 + 0.5 - rec[:, 1], rec[:, 1] - (y1 + 0.5)), 0)
    return ex * ex + ey * ey <= rec[:, 2]


def edge_pixels(case):
    """Number of (list entry, pixel of its tile) pairs with d^2 == r^2 exactly."""
    n = 0
    for t in range(np.asarray(case["offsets"]).size):
        s, e = list_range(case["offsets"], case["n_isects"], t)
        x0, x1, y0, y1 = tile_pixels(t, case["W"], case["H"])
        xs, ys = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
        for g in case["flatten_ids"][s:e]:
            u, v, r2 = case["records"][g, :3].astype(np.float64)
            n += int(((xs - u) ** 2 + (ys - v) ** 2 == r2).sum())
    return n


# ---- exactness ----------------------------------------------------------------------------------------------------------
def assert_exact(case):
    """The conditions that make the verdict total; case: records f32 [N,8] (+ records64, the values they were meant to
    hold), offsets, flatten_ids, n_isects, W, H, max_hit, ties.
      1. u, v multiples of 1/8 within +-256; every field, r^2 above all, is exactly an fp32 number.
      2. for every (record, pixel of a tile that lists it): d^2 == r^2 exactly or |d^2 - r^2| >= 8 ulp_fp32(max(d^2, r^2)):
         the fp32 coverage test (d^2 carries at most one rounding) and the float64 one agree on every pair.
      3. every alpha is 1 or at most 1/2, and every pixel's transmittance, walked in float64, ends at exactly 0 or at
         >= 2^-100: T stays a normal fp32 number, no decision depends on the device's denormal mode.  (At most 100
         hits of alpha 1/2 imply this; the lists of 127 .. 200 whole-tile records reach it with smaller alphas, so the
         bound on T itself is what is asserted.)
      4. the fp32 depths within one tile list are pairwise different, except where `ties` is set: the hand-built ties
         case, and the pipeline scenes, whose z in {2, 4, 8, 16} must repeat in a list of 63 entries: there the order is
         (depth bits, index), which lists_from states and the stable radix sort yields."""
    rec = case["records"]
    name = case["name"]
    assert rec.dtype == np.float32
    listed = np.unique(case["flatten_ids"])
    r64 = case["records64"][listed]
    # 1. lattice centres; every field (r^2 above all) is the fp32 value it was meant to be
    with np.errstate(over="ignore"):
        assert np.array_equal(r64.astype(np.float32).astype(np.float64), r64), f"{name}: a field is not an fp32 number"
    assert np.array_equal(r64, rec[listed].astype(np.float64)), name
    uv = r64[:, :2]
    assert np.array_equal(uv * 8, np.round(uv * 8)) and np.abs(uv).max(initial=0) <= 256, f"{name}: centres off the lattice"
    # 2. d^2 == r^2 exactly, or 8 fp32 ulps apart, for every pixel of every listed tile
    for t in range(np.asarray(case["offsets"]).size):
        s, e = list_range(case["offsets"], case["n_isects"], t)
        x0, x1, y0, y1 = tile_pixels(t, case["W"], case["H"])
        xs, ys = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
        z = rec[case["flatten_ids"][s:e], 3]
        # 4. distinct fp32 depths within a list (the ties case: order by index, which the list states itself)
        if not case.get("ties"):
            assert np.unique(z.view(np.uint32)).size == z.size, f"{name}: tile {t} has equal depths"
        for g in np.unique(case["flatten_ids"][s:e]):
            u, v, r2 = rec[g, :3].astype(np.float64)
            d2 = (xs - u) ** 2 + (ys - v) ** 2
            gap = 8 * np.spacing(np.maximum(d2, r2).astype(np.float32)).astype(np.float64)
            ok = (d2 == r2) | (np.abs(d2 - r2) >= gap)
            assert ok.all(), f"{name}: record {g} tile {t}: a pixel within 8 ulp of the disc edge"
    # 3. alpha is 1 or at most 1/2, and T stays 0 or >= 2^-100 (normal in fp32): no denormal decides anything
    a = rec[listed, 7]
    assert ((a == 1) | ((a > 0) & (a <= 0.5))).all(), f"{name}: alpha"
    T = blend_f64(rec, case["offsets"], case["flatten_ids"], case["n_isects"], case["W"], case["H"],
                  case["max_hit"])["T"]
    assert ((T == 0) | (T >= 2.0 ** -100)).all(), f"{name}: transmittance below 2^-100"


# ---- hand-built cases for the blend kernel --------------------------------------------------------------------------------
def _col(i):
    return ((i % 16 + 1) / 16.0, ((i // 16) % 16 + 1) / 16.0, ((7 * i) % 16 + 1) / 16.0)


class _Build:
    def __init__(self, name, max_hit=1000, W=W0, H=H0, ties=False, seed=0):
        self.name, self.W, self.H, self.max_hit, self.ties = name, W, H, max_hit, ties
        self.rows, self.lists, self.k = [], {}, 0
        self.rng = np.random.default_rng(seed)

    def add(self, u, v, r2, rgb=None, a=0.5, z=None):
        if z is None:
            z = 2.0 + self.k / 64.0           # distinct, increasing, exact in fp32
        self.k += 1
        self.rows.append([u, v, r2, z, *(rgb if rgb is not None else _col(self.k)), a])
        return len(self.rows) - 1

    def centre(self, t):
        tw, _ = tiles_of(self.W, self.H)
        ty, tx = divmod(t, tw)
        return tx * TILE + 8.0, ty * TILE + 8.0

    def whole(self, t, a=0.5, rgb=None, z=None):
        """A disc that covers every pixel of tile t (r = 16 about the tile's centre: the far corner is at d^2 = 112.5)."""
        cx, cy = self.centre(t)
        return self.add(cx, cy, 256.0, rgb, a, z)

    def left(self, t, cols, a=0.5, rgb=None):
        """A disc that covers exactly the first `cols` columns of tile t, all 16 rows: r = 256, centred 256 to the left
        of the column border (the edge bends by 56.25 / 512 < 0.5 px over the tile's rows)."""
        cx, cy = self.centre(t)
        return self.add(cx - 8.0 + cols - 256.0, cy, 65536.0, rgb, a)

    def put(self, t, ids):
        self.lists.setdefault(t, []).extend(ids)

    def bin(self, i, R):
        x0, x1, y0, y1 = point_tiles(self.rows[i][0], self.rows[i][1], R, self.W, self.H)
        tw, _ = tiles_of(self.W, self.H)
        for ty in range(y0, y1):
            for tx in range(x0, x1):
                self.put(ty * tw + tx, [i])

    def finish(self, **meta):
        rows = np.array(self.rows, np.float64).reshape(-1, 8)
        n = rows.shape[0]
        new = self.rng.permutation(n)                     # record ids in no particular order: flatten_ids is a gather
        rec64 = np.zeros_like(rows)
        rec64[new] = rows
        tw, th = tiles_of(self.W, self.H)
        offsets, flat = [], []
        for t in range(tw * th):
            offsets.append(len(flat))
            flat += [int(new[i]) for i in self.lists.get(t, [])]
        with np.errstate(over="ignore"):
            rec32 = rec64.astype(np.float32)
        return dict(name=self.name, W=self.W, H=self.H, max_hit=self.max_hit, ties=self.ties, records=rec32,
                    records64=rec64, offsets=np.array(offsets, np.int32), flatten_ids=np.array(flat, np.int32),
                    n_isects=len(flat), **meta)


LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
CULL_PATTERNS = ((0, 1, 7), (8, 0, 9), (63, 64, 0), (64, 0, 1), (1, 63, 8), (9, 7, 64), (0, 0, 63))
CAPS = (1, 2, 7, 8, 9, 63, 64, 65, 100)
EDGE_R = (0.5, 1.0, 2.5, 5.0, 13.0)
# (u, v, r, the tiles whose pixel rectangle [floor((m - R) / 16), ceil((m + R) / 16)) holds, R = max(ceil(r), 1))
EDGE_DISCS = (
    (11.5, 8.5, 5.0, {0, 1}),        # touches (16.5, 8.5): the first column of the next tile
    (20.5, 8.5, 5.0, {0, 1}),        # touches (15.5, 8.5): the last column of the previous tile, its only pixel there
    (8.5, 11.5, 5.0, {0, 3}),        # touches (8.5, 16.5): the first row of the next tile row
    (8.5, 20.5, 5.0, {0, 3}),        # touches (8.5, 15.5): the last row of the previous tile row
    (11.5, 4.5, 13.0, {0, 1, 3, 4}), # (5, 12, 13): touches (16.5, 16.5), the only pixel it has in tile 4
    (2.5, 20.5, 13.0, {0, 3}),       # (13, 0): touches (15.5, 20.5), the last column of tile 3
    (16.0, 8.5, 0.5, {0, 1}),        # touches (15.5, 8.5) and (16.5, 8.5) and covers nothing else
    (15.5, 2.5, 1.0, {0, 1}),        # touches (16.5, 2.5), (14.5, 2.5), (15.5, 1.5), (15.5, 3.5)
    (15.0, 12.5, 2.5, {0, 1}),       # (1.5, 2, 2.5): touches (16.5, 14.5) and (16.5, 10.5)
    (24.5, 15.0, 2.5, {1, 4}),       # (2, 1.5, 2.5): touches (26.5, 16.5) and (22.5, 16.5) in the next tile row
    (44.5, 8.5, 5.0, {2}),           # centred right of the image: touches (39.5, 8.5), its only pixel in the image
    (20.5, 28.5, 5.0, {3, 4}),        # centred below the image: touches (20.5, 23.5), its only pixel in the image
    (28.5, 8.5, 5.0, {1, 2}),        # touches (28.5, 3.5): its only pixel in strip 0 (rows 0..3) of tile 1
    (36.5, 20.5, 0.0, {5}),          # r = 0 on a pixel centre: exactly that pixel
    (4.0, 20.5, 0.0, {3}),           # r = 0 off a centre: nothing
    (16.5, 16.5, 0.0, {0, 1, 3, 4}), # r = 0 on the first pixel of tile 4
)


def _alpha(rng, n, small=False):
    if small:
        return rng.choice([0.125, 0.25], n, p=[0.7, 0.3])
    return rng.choice([0.5, 0.25, 0.125, 0.375], n, p=[0.1, 0.2, 0.5, 0.2])


def _lengths():
    out = []
    for k, n in enumerate(LENGTHS):
        b = _Build(f"lengths_{n}", seed=100 + n)
        t = k % 6
        b.put(t, [b.whole(t, a) for a in _alpha(b.rng, n)])
        if n == 0:
            b.whole(t, 0.5)                   # a record no list names (the entry refuses an empty record array)
        out.append(b.finish(tile=t, n=n))
    return out


def _cull():
    out = []
    for k, pat in enumerate(CULL_PATTERNS):
        t = (0, 5, 1, 3, 4, 2, 0)[k]
        b = _Build("cull_" + "_".join(map(str, pat)), seed=200 + k)
        x0, x1, y0, y1 = tile_pixels(t, W0, H0)
        ids = []
        for nb in pat:
            surv = np.zeros(64, bool)
            surv[b.rng.choice(64, nb, replace=False)] = True
            for j in range(64):
                kind = b.rng.random()
                if surv[j]:
                    if kind < 0.7:
                        ids.append(b.whole(t, float(_alpha(b.rng, 1, small=True)[0])))
                    elif kind < 0.9:      # a 3 x 3 block about one pixel: survives in one or two strips only
                        ids.append(b.add(b.rng.integers(x0, x1 + 1) + 0.5, b.rng.integers(y0, y1 + 1) + 0.5, 2.25, a=0.125))
                    else:                 # inside the rectangle, between four pixel centres: survives, covers nothing
                        ids.append(b.add(float(b.rng.integers(x0 + 1, x1 + 1)), float(b.rng.integers(y0 + 1, y1 + 1)),
                                         0.0625, a=0.5))
                else:
                    if kind < 0.5:        # the corner gap: each coordinate within r of the rectangle, the corner is not
                        sx, sy = b.rng.integers(0, 2, 2)
                        ids.append(b.add(x1 + 1.25 if sx else x0 - 0.25, y1 + 1.25 if sy else y0 - 0.25, 1.0, a=1.0))
                    else:                 # nowhere near
                        cx, cy = b.centre(t)
                        ids.append(b.add(cx + 40.0 * (1 if b.rng.random() < 0.5 else -1), cy + 40.0, 1.0, a=1.0))
        b.put(t, ids)
        out.append(b.finish(tile=t, survivors=pat))
    return out


def _caps():
    out = []
    for cap in CAPS:
        for half in (False, True):
            b = _Build(f"cap_{cap}" + ("_left8" if half else ""), max_hit=cap, seed=300 + cap)
            t = 1 if half else 0
            ids = [b.left(t, 8, 0.125) for _ in range(64)] if half else []       # one alpha throughout: (7/8)^hits
            ids += [b.whole(t, 0.125) for _ in range(130)]
            b.put(t, ids)
            out.append(b.finish(tile=t, cap=cap, half=half))
    return out


RED, GREEN, BLUE = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)


def _opaque():
    out = []
    for k, t in ((7, 0), (8, 1), (9, 3)):
        # k - 1 opaque bands of 1 .. k - 1 columns (every one reaches all 16 rows, so it survives in every strip), the
        # k-th opaque record covers the tile; whatever follows must not show
        b = _Build(f"opaque_finish_after_{k}", seed=400 + k)
        ids = [b.left(t, j, 1.0, (j / 16.0, 0.0, 0.0)) for j in range(1, k)] + [b.whole(t, 1.0, GREEN)]
        ids += [b.whole(t, 0.5, BLUE) for _ in range(20)]
        b.put(t, ids)
        out.append(b.finish(tile=t, finish=k))
    b = _Build("opaque_finish_at_batch_end", seed=410)
    ids = [b.left(4, 1 + j % 15, 0.125, (0.5, j / 64.0, 0.0)) for j in range(63)] + [b.whole(4, 1.0, GREEN)]
    ids += [b.whole(4, 0.5, BLUE) for _ in range(66)]
    b.put(4, ids)
    out.append(b.finish(tile=4, finish=64))
    # sixteen opaque 4 x 4 blocks (r = 2.5 about a pixel corner covers exactly the 16 pixels around it), then the rest
    b = _Build("opaque_blocks", seed=420)
    ids = [b.add(2.0 + 4 * i, 2.0 + 4 * j, 6.25, ((1 + i) / 4.0, (1 + j) / 4.0, 0.0), 1.0) for j in range(4) for i in range(4)]
    ids += [b.whole(0, 0.5, BLUE) for _ in range(10)]
    b.put(0, ids)
    out.append(b.finish(tile=0, finish=None))
    return out


def _edge_r2(r, shift):
    r2 = np.float32(r * r)
    return float(r2 + np.float32(shift * 8) * np.spacing(r2)) if r > 0 else 0.0


def _edges():
    out = []
    for shift, tag in ((0, "exact"), (-1, "8ulp_down"), (1, "8ulp_up")):
        b = _Build(f"edge_{tag}", seed=500)
        for u, v, r, _ in EDGE_DISCS:
            b.bin(b.add(u, v, _edge_r2(r, shift), a=0.5), max(np.ceil(r), 1.0))
        out.append(b.finish(shift=shift))
    return out


def _partial():
    b = _Build("partial_tiles", seed=600)
    for t in (2, 3, 4, 5):
        b.put(t, [b.whole(t, 0.25) for _ in range(3)])
    for u, v, r in ((45.0, 30.0, 13.0), (-3.0, 20.0, 5.0), (44.5, 8.5, 5.0), (20.5, 28.5, 5.0), (41.0, 12.0, 2.5),
                    (30.0, 25.5, 2.5), (43.0, 27.0, 6.5), (-8.0, 30.0, 13.0)):
        b.bin(b.add(u, v, r * r, a=0.5), np.ceil(r))
    for t in (2, 5):
        b.put(t, [b.whole(t, 0.125)])
    return [b.finish()]


def _ties():
    b = _Build("ties", ties=True, seed=700)
    b.put(1, [b.whole(1, a, z=4.0) for a in (0.5, 0.25, 0.5, 0.125, 1.0, 0.5)])
    b.put(5, [b.whole(5, 0.5, z=8.0) for _ in range(70)])
    return [b.finish()]


_WALK = None


def walk_cases():
    """Every hand-built case, generated once."""
    global _WALK
    if _WALK is None:
        _WALK = _lengths() + _cull() + _caps() + _opaque() + _edges() + _partial() + _ties()
    return _WALK


# ---- whole-pipeline scenes ----------------------------------------------------------------------------------------------
W2C = np.array([[0.0, -1.0, 0.0, 1.0], [0.0, 0.0, -1.0, -2.0], [1.0, 0.0, 0.0, 3.0], [0.0, 0.0, 0.0, 1.0]])
FOCAL = 64.0
HALF = 0.5                                   # the drop-in's scale_modifier


def world_points(u, v, z, W, H):
    """Camera-space lattice points (u, v multiples of 1/8, z a power of two) -> world, float32, exactly."""
    cam = np.stack([(u - W / 2) * z / FOCAL, (v - H / 2) * z / FOCAL, z], 1)
    p = (cam - W2C[:3, 3]) @ W2C[:3, :3]
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return p.astype(np.float32)


def _run(name, u, v, z, rgb, W=W0, H=H0, *, kind, a=None, occ=0.5, r=None, scale=None, near=1.0, far=100.0, max_hit=100,
         bg=None, **meta):
    """kind "hip": render_points_hip (radius mode 0, one occ); kind "dropin": PointRasterizer (per-point opacities and
    radius, scale_modifier 1/2)."""
    u, v, z = (np.asarray(x, np.float64) for x in (u, v, z))
    run = dict(name=f"{name}_{kind}", kind=kind, W=W, H=H, points=world_points(u, v, z, W, H),
               colors=np.asarray(rgb, np.float32).reshape(-1, 3), near=near, far=far, max_hit=max_hit, bg=bg,
               ties=True, **meta)
    if kind == "hip":
        run.update(mode=0, scale=float(scale), occ=occ, opacities=None, radius_in=None)
    else:
        rin = np.asarray(r, np.float64) * z / (HALF * FOCAL)
        assert np.array_equal(rin.astype(np.float32).astype(np.float64), rin)
        run.update(mode=3, scale=HALF, occ=1.0, opacities=np.asarray(a, np.float32), radius_in=rin.astype(np.float32))
    return run


Z_OF_R = {5.0: 2.0, 2.5: 4.0, 1.0: 8.0, 0.5: 16.0, 13.0: 2.0, 0.0: 4.0}


def scene_runs():
    runs = []
    bg = np.array([0.25, 0.5, 0.75], np.float32)
    # -- the edge set across tile borders; through the constant-scale entry one run per scale that yields its radii
    E = np.array([(u, v, r) for u, v, r, _ in EDGE_DISCS])
    z = np.array([Z_OF_R[r] for r in E[:, 2]])
    rgb = np.array([_col(i) for i in range(len(E))])
    tiles = [t for *_, t in EDGE_DISCS]
    rng = np.random.default_rng(11)
    runs.append(_run("edge", E[:, 0], E[:, 1], z, rgb, kind="dropin", a=rng.choice([1.0, 0.5, 0.25, 0.125], len(E)),
                     r=E[:, 2], bg=bg, expect_tiles=tiles))
    for scale, rs in ((5 / 32, (5.0, 2.5)), (1 / 8, (1.0, 0.5)), (13 / 32, (13.0,)), (0.0, (0.0,))):
        m = np.isin(E[:, 2], rs)
        runs.append(_run(f"edge_scale_{scale:g}", E[m, 0], E[m, 1], z[m], rgb[m], kind="hip", scale=scale,
                         expect_tiles=[t for t, k in zip(tiles, m) if k], expect_r=E[m, 2]))
    # -- lists of exactly 63, 64 and 65 entries: small discs whose rectangle stays inside one tile
    rng = np.random.default_rng(12)
    us, vs, zs = [], [], []
    for t, n in ((0, 63), (1, 64), (3, 65)):
        tx, ty = t % 3, t // 3
        us.append(tx * 16 + rng.integers(4 * 8, 12 * 8 + 1, n) / 8.0)
        vs.append(ty * 16 + rng.integers(4 * 8, 12 * 8 + 1, n) / 8.0)
        zs.append(rng.choice([2.0, 4.0, 8.0, 16.0], n))
    us, vs, zs = map(np.concatenate, (us, vs, zs))
    rgb = np.array([_col(i) for i in range(len(us))])
    runs.append(_run("lists_63_64_65", us, vs, zs, rgb, kind="hip", scale=1 / 8, occ=0.25, expect_lists={0: 63, 1: 64, 3: 65}))
    runs.append(_run("lists_63_64_65", us, vs, zs, rgb, kind="dropin", a=rng.choice([1.0, 0.5, 0.25, 0.125], len(us),
                                                                                  p=[0.05, 0.15, 0.3, 0.5]),
                     r=8.0 / zs, bg=bg, expect_lists={0: 63, 1: 64, 3: 65}))
    # -- discs far larger than the image: r = 2^20, and r = 2^31 (ceil(r) is held at 2^30); every tile lists them
    for W, H in ((W0, H0), (64, 48)):
        u = np.array([W / 2 + 3.0, 5.0, W - 2.5])
        v = np.array([H / 2, 7.5, 3.0])
        z = np.array([2.0, 4.0, 8.0])
        rgb = np.array([_col(i) for i in range(3)])
        runs.append(_run(f"big_disc_{W}x{H}", u, v, z, rgb, W, H, kind="dropin", a=[0.5, 0.25, 1.0],
                         r=[2.0 ** 20, 2.0 ** 31, 2.0 ** 31], all_tiles=3, bg=bg))
        runs.append(_run(f"big_disc_2p20_{W}x{H}", u, v, z, rgb, W, H, kind="hip", scale=2.0 ** 15, all_tiles=3))
        runs.append(_run(f"big_disc_2p31_{W}x{H}", u, v, z, rgb, W, H, kind="hip", scale=2.0 ** 26, all_tiles=3))
    # -- the open depth window: z == near and z == far are culled, one fp32 step inside they are kept
    u = np.array([6.0, 14.5, 23.0, 33.5])
    v = np.array([6.5, 12.0, 17.5, 9.0])
    z = np.array([2.0, 4.0, 8.0, 16.0])
    rgb = np.array([_col(i) for i in range(4)])
    below2, above16 = float(np.nextafter(F32(2), F32(0))), float(np.nextafter(F32(16), F32(32)))
    runs.append(_run("window_at_the_planes", u, v, z, rgb, kind="hip", scale=1 / 2, near=2.0, far=16.0, bg=bg,
                     expect_keep=[False, True, True, False]))
    runs.append(_run("window_one_step_inside", u, v, z, rgb, kind="hip", scale=1 / 2, near=below2, far=above16, bg=bg,
                     expect_keep=[True, True, True, True]))
    # -- nothing kept: the background, without a launch of the blend kernel, in both layouts
    runs.append(_run("nothing_kept", u, v, z, rgb, kind="hip", scale=1 / 2, near=16.0, far=100.0, bg=bg,
                     expect_keep=[False] * 4))
    runs.append(_run("nothing_kept", u, v, z, rgb, kind="dropin", a=[0.5] * 4, r=[4.0] * 4, near=32.0, far=100.0, bg=bg,
                     expect_keep=[False] * 4))
    return runs


def reference_render(run):
    """project_f64 -> records -> lists_from -> both walks, for one run.  The result also passes as a `case` to
    assert_exact."""
    W, H = run["W"], run["H"]
    proj = project_f64(run["points"], run["colors"], run["opacities"], run["occ"], run["radius_in"], W2C, FOCAL, FOCAL,
                       W / 2, H / 2, FOCAL, run["near"], run["far"], run["mode"], run["scale"], 1.0, H, W)
    rec64 = np.concatenate([np.stack([proj["u"], proj["v"], proj["r2"], proj["z"]], 1),
                            run["colors"].astype(np.float64), proj["a"].astype(np.float64)[:, None]], 1)
    rec = records_from(proj, run["colors"])
    offsets, flat, n = lists_from(rec[:, 0], rec[:, 1], proj["R"], rec[:, 3], W, H)
    case = dict(name=run["name"], W=W, H=H, max_hit=run["max_hit"], ties=run["ties"], records=rec, records64=rec64,
                offsets=offsets, flatten_ids=flat, n_isects=n, proj=proj)
    args = (rec, offsets, flat, n, W, H, run["max_hit"], run["bg"])
    case["f64"], case["f32"] = blend_f64(*args), blend_f32_replay(*args)
    return case
