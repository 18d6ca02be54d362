"""Records for the tile-cull probe and their float64 reference -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_tile_cull_cpu.py (the generator's conditions, the reference's own consistency, a float32 emulation
of the cull) and tests/test_tile_cull_gpu.py (sc_test_tile_cull: the real splat_misses_rect / sc_pair_alpha on the device).
A record is one Gaussian (conic a, b, c, opacity, centre) against one rectangle of pixel centres: a whole 16 x 16 tile, a
partial tile at the frame's edge, or the upper / lower half of a tile.  Nothing in this file touches a GPU.

The reference takes the record's float32 values (exact in float64) and gives, per pixel centre of the rectangle,
    q      = (a dx^2 + c dy^2) / 2 + b dx dy
    S      = (|a| dx^2 + |c| dy^2) / 2 + |b dx dy|              (blend_f64's term magnitude)
    valid  = q >= 0 and min(0.999, op exp(-q)) >= 1 / 255
    near   = the decision is inside blend_f64's window:  |q| <= k 2^-24 S  or  |ln(255 op) - q| <= k 2^-24 S + 4 2^-24
and per record the continuous minimum of q over the rectangle (stationary points of its four edges, 0 when the centre of a
positive definite conic is inside) and the cull's own magnitude bound S_rect = a X^2 + c Y^2 + 2 |b| X Y with X, Y the
largest |dx|, |dy| of the rectangle (csrc/raster_common.h).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

ALPHA_MIN = 1.0 / 255.0
ALPHA_MAX = 0.999
EPS24 = 2.0 ** -24
K_ROUND = 8.0
LN255 = float(np.log(255.0))

FAMILIES = {"covariance": 7001, "raw": 7002}       # name -> seed
N_RECORDS = 100_000
KIND_WHOLE, KIND_PARTIAL, KIND_HALF = 0, 1, 2
EPS_LADDER = np.array([1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7])
PD_REL = 1e-6                                       # "positive definite by a relative 1e-6": a c - b^2 > PD_REL a c
COMPLETE_FACTOR = 2.0                               # the completeness margin is this times the documented one


# ---- geometry -------------------------------------------------------------------------------------------------------------
def rectangle(geo):
    """geo i32[n, 6] = (txi, tyi, sub, NSUB, width, height) -> x0, y0 (first pixel centre), ncols, nrows of the rectangle
    of in-image pixels the wave covers.  Written from the definition, not from the kernel's code."""
    geo = np.asarray(geo, np.int64)
    txi, tyi, sub, nsub, w, h = (geo[:, i] for i in range(6))
    rows = 16 // nsub
    px0 = txi * 16
    py0 = tyi * 16 + sub * rows
    ncols = np.minimum(16, w - px0)
    nrows = np.minimum(rows, h - py0)
    assert (ncols >= 1).all() and (nrows >= 1).all()
    return px0 + 0.5, py0 + 0.5, ncols, nrows


def lane_bit(nsub, lane, k):
    """Bit of the probe's mask that pixel k of `lane` owns: NSUB 1 -> 4 pixels per lane, 4 lanes per row; NSUB 2 -> 2
    pixels per lane, 8 lanes per row.  Bit = 16 * row + column of the rectangle."""
    ppl = 4 if nsub == 1 else 2
    lpr = 16 // ppl
    return 16 * (lane // lpr) + ppl * (lane % lpr) + k


# ---- float64 reference ----------------------------------------------------------------------------------------------------
def _lattice(rec, x0, y0, ncols, nrows):
    rec = np.asarray(rec, np.float64)
    a, b, c, op, mx, my = (rec[:, i][:, None, None] for i in range(6))
    j = np.arange(16, dtype=np.float64)
    dx = (np.asarray(x0, np.float64)[:, None, None] + j[None, None, :]) - mx
    dy = (np.asarray(y0, np.float64)[:, None, None] + j[None, :, None]) - my
    inside = (j[None, None, :] < np.asarray(ncols)[:, None, None]) & (j[None, :, None] < np.asarray(nrows)[:, None, None])
    t_a, t_c, t_b = 0.5 * a * dx * dx, 0.5 * c * dy * dy, b * dx * dy
    return t_a + t_c + t_b, np.abs(t_a) + np.abs(t_c) + np.abs(t_b), inside, op


def classify(rec, x0, y0, ncols, nrows):
    """-> dict of per-pixel bool [n, 256] (bit 16 * row + column) `inside`, `cv` (certainly valid), `ci` (certainly
    invalid), and per record `qmin` (lattice minimum of q), `S_pix` (largest S over the pixels)."""
    q, S, inside, op = _lattice(rec, x0, y0, ncols, nrows)
    with np.errstate(all="ignore"):
        lnr = np.log(op) + LN255 - q                     # ln(raw alpha * 255), in log form: no underflow
        valid = (q >= 0.0) & (np.minimum(np.log(ALPHA_MAX) + LN255, lnr) >= 0.0)
        es = K_ROUND * EPS24 * S
        near = ((es > 0.0) & (np.abs(q) <= es)) | (np.abs(lnr) <= es + 4.0 * EPS24)
    n = q.shape[0]
    cv = (valid & ~near & inside).reshape(n, 256)
    ci = (~valid & ~near & inside).reshape(n, 256)
    return dict(inside=inside.reshape(n, 256), cv=cv, ci=ci,
                qmin=np.where(inside, q, np.inf).min(axis=(1, 2)), S_pix=np.where(inside, S, 0.0).max(axis=(1, 2)))


def continuous_min(rec, x0, y0, ncols, nrows):
    """Minimum of q over the rectangle [x0, x0 + ncols - 1] x [y0, y0 + nrows - 1] in float64: every edge at its ends and
    at its clamped stationary point; 0 where the conic is positive semi-definite and the centre lies inside.  (A quadratic
    that is not convex takes its minimum over a rectangle on the boundary, so this holds for indefinite conics too.)"""
    rec = np.asarray(rec, np.float64)
    a, b, c, mx, my = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 4], rec[:, 5]
    xl, xh = np.asarray(x0, np.float64) - mx, np.asarray(x0, np.float64) + (np.asarray(ncols) - 1) - mx
    yl, yh = np.asarray(y0, np.float64) - my, np.asarray(y0, np.float64) + (np.asarray(nrows) - 1) - my

    def q(x, y):
        return 0.5 * (a * x * x + c * y * y) + b * x * y

    best = np.full(rec.shape[0], np.inf)
    with np.errstate(all="ignore"):
        for xe in (xl, xh):
            ys = np.clip(np.where(c > 0, -b * xe / np.where(c > 0, c, 1.0), yl), yl, yh)
            for y in (ys, yl, yh):
                best = np.minimum(best, q(xe, y))
        for ye in (yl, yh):
            xs = np.clip(np.where(a > 0, -b * ye / np.where(a > 0, a, 1.0), xl), xl, xh)
            for x in (xs, xl, xh):
                best = np.minimum(best, q(x, ye))
    psd = (a >= 0) & (c >= 0) & (a * c - b * b >= 0)
    centre_in = (xl <= 0) & (xh >= 0) & (yl <= 0) & (yh >= 0)
    return np.where(psd & centre_in, 0.0, best)


def s_rect(rec, x0, y0, ncols, nrows):
    rec = np.asarray(rec, np.float64)
    a, b, c, mx, my = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 4], rec[:, 5]
    X = np.maximum(np.abs(x0 - mx), np.abs(x0 + (ncols - 1) - mx))
    Y = np.maximum(np.abs(y0 - my), np.abs(y0 + (nrows - 1) - my))
    return a * X * X + c * Y * Y + 2.0 * np.abs(b) * X * Y


def complete_class(rec, cmin, S_rect):
    """Records the cull MUST drop: conic positive definite by a relative PD_REL and the continuous minimum above
    L + COMPLETE_FACTOR (1e-3 + 1e-3 |L| + 2e-6 S_rect), L = ln(255 op).  S here is the CULL's S_rect, the one its
    documented margin is written with (csrc/raster_common.h), not blend_f64's per-pixel S: S_rect is at least twice the
    largest per-pixel S, so this class is the narrower of the two readings of "twice the documented margin"."""
    rec = np.asarray(rec, np.float64)
    a, b, c, op = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    L = np.log(255.0 * op)
    pd = (a > 0) & (c > 0) & (a * c - b * b > PD_REL * a * c)
    return pd & (cmin > L + COMPLETE_FACTOR * (1e-3 + 1e-3 * np.abs(L) + 2e-6 * S_rect))


# ---- numpy float32 emulation of splat_misses_rect (csrc/raster_common.h) ---------------------------------------------------
def emulate_cull_f32(rec, x0, y0, ncols, nrows):
    """The cull's verdict with every operation rounded to float32, in the order the source writes them (the compiler may
    contract a * b + c into one rounding; this does not).  True = "misses"."""
    f = np.float32
    rec = np.asarray(rec, f)
    A, B, C, op, mx, my = (rec[:, i] for i in range(6))
    x0f = np.asarray(x0, f)
    y0f = np.asarray(y0, f)
    x1f = (np.asarray(x0, np.float64) + (np.asarray(ncols) - 1)).astype(f)
    y1f = (np.asarray(y0, np.float64) + (np.asarray(nrows) - 1)).astype(f)
    xl, xh, yl, yh = x0f - mx, x1f - mx, y0f - my, y1f - my
    with np.errstate(all="ignore"):
        L = np.log(f(255.0) * op).astype(f)
        base = L + f(1e-3) + f(1e-3) * np.abs(L)
        early = base < 0
        pd = (A > 0) & (C > 0) & (A * C - B * B > 0)
        X, Y = np.maximum(np.abs(xl), np.abs(xh)), np.maximum(np.abs(yl), np.abs(yh))
        S = A * X * X + C * Y * Y + f(2.0) * np.abs(B) * X * Y
        tau = base + f(2e-6) * S
        centre_in = (xl <= 0) & (xh >= 0) & (yl <= 0) & (yh >= 0)
        best = np.full(A.shape, f(3.0e38))
        invC, invA = f(1.0) / C, f(1.0) / A
        for e in range(2):
            xe = xh if e else xl
            ys = np.minimum(np.maximum(-B * xe * invC, yl), yh)
            best = np.fmin(best, f(0.5) * (A * xe * xe + C * ys * ys) + B * xe * ys)
            ye = yh if e else yl
            xs = np.minimum(np.maximum(-B * ye * invA, xl), xh)
            best = np.fmin(best, f(0.5) * (A * xs * xs + C * ye * ye) + B * xs * ye)
        best = np.where(centre_in, f(0.0), best)
        return early | (pd & (best > tau))


# ---- records ----------------------------------------------------------------------------------------------------------------
def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _draw_geometry(rng, n):
    kind = rng.choice([KIND_WHOLE, KIND_PARTIAL, KIND_HALF], size=n, p=[0.3, 0.35, 0.35])
    txi, tyi = rng.integers(0, 8, n), rng.integers(0, 8, n)
    pw, ph = rng.integers(1, 17, n), rng.integers(1, 17, n)
    sub = np.where(kind == KIND_HALF, rng.integers(0, 2, n), 0)
    nsub = np.where(kind == KIND_HALF, 2, 1)
    # whole: the frame goes on beyond the tile; partial: the frame ends pw x ph pixels into it; half: every other half
    # is cut by the frame's edge as well (in x, and in y within the half)
    half_cut = (kind == KIND_HALF) & (rng.random(n) < 0.5)
    cut_x = (kind == KIND_PARTIAL) | half_cut
    width = np.where(cut_x, txi * 16 + pw, (txi + 1 + rng.integers(0, 3, n)) * 16)
    ph_half = sub * 8 + 1 + (ph - 1) % 8
    height = np.where(kind == KIND_PARTIAL, tyi * 16 + ph,
                      np.where(half_cut, tyi * 16 + ph_half, (tyi + 1 + rng.integers(0, 3, n)) * 16))
    geo = np.stack([txi, tyi, sub, nsub, width, height], axis=1).astype(np.int32)
    return geo, kind


def _draw_conics(rng, family, n):
    if family == "covariance":
        s1, s2 = _log_uniform(rng, 0.01, 800.0, n), _log_uniform(rng, 0.01, 800.0, n)
        th = rng.uniform(0, np.pi, n)
        co, si = np.cos(th), np.sin(th)
        cxx = co * co * s1 * s1 + si * si * s2 * s2 + 0.3
        cyy = si * si * s1 * s1 + co * co * s2 * s2 + 0.3
        cxy = co * si * (s1 * s1 - s2 * s2)
        det = cxx * cyy - cxy * cxy
        return cyy / det, -cxy / det, cxx / det
    A, C = _log_uniform(rng, 1e-6, 1e3, n), _log_uniform(rng, 1e-6, 1e3, n)
    rho = (1.0 - _log_uniform(rng, 1e-7, 1.0, n)) * rng.choice([-1.0, 1.0], n)
    return A, rho * np.sqrt(A * C), C


# record classes and their shares of a family: opacity aimed at the threshold of the lattice minimum (centre anywhere /
# centre along the conic's major axis, where q stays small while its terms grow: the ill-conditioned records), opacity
# drawn freely (centre far away: the plainly missing records / centre anywhere: records with many valid pixels)
CLASSES = (("aimed", 0.24), ("aimed_axis", 0.36), ("free_far", 0.35), ("free_any", 0.05))


DISTANCE = {"aimed": (0.3, 3000.0), "aimed_axis": (25.0, 300.0), "free_far": (30.0, 3000.0), "free_any": (0.3, 3000.0)}


def _draw(rng, family, cls, n):
    geo, kind = _draw_geometry(rng, n)
    x0, y0, ncols, nrows = rectangle(geo)
    a, b, c = _draw_conics(rng, family, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    d = _log_uniform(rng, *DISTANCE[cls], n)
    ox, oy = d * np.cos(phi), d * np.sin(phi)
    if cls == "aimed_axis":
        # unit vector of the conic's smallest eigenvalue (the Gaussian's long axis), and a small step across it
        lam = 0.5 * (a + c) - np.sqrt(0.25 * (a - c) ** 2 + b * b)
        ux, uy = np.where(np.abs(b) > 0, b, 1.0), np.where(np.abs(b) > 0, lam - a, 0.0)
        flip = (np.abs(b) == 0) & (c < a)
        ux, uy = np.where(flip, 0.0, ux), np.where(flip, 1.0, uy)
        nrm = np.hypot(ux, uy)
        ux, uy = ux / nrm, uy / nrm
        t = _log_uniform(rng, 0.01, 3.0, n) * rng.choice([-1.0, 1.0], n)
        # most of them: the distance at which the axis term alone is of the order of ln(255 op) (redrawn when out of range)
        with np.errstate(all="ignore"):
            dq = np.sqrt(2.0 * _log_uniform(rng, 1.5, 5.3, n) / lam)
        d = np.where((rng.random(n) < 0.8) & (lam > 0) & (dq >= 25.0) & (dq <= 300.0), dq, d)
        ox, oy = d * ux - t * uy, d * uy + t * ux
        d = np.hypot(ox, oy)
    in_range = np.ones(n, bool)
    if cls == "aimed":
        # the distance along the drawn direction at which q reaches a target of the order of ln(255 op), 0.02 .. 5.5: an
        # opacity aimed at a q far below that is within rounding of 1 / 255 whatever eps is
        ex, ey = ox / d, oy / d
        kappa = 0.5 * (a * ex * ex + c * ey * ey) + b * ex * ey
        with np.errstate(all="ignore"):
            d2 = np.sqrt(_log_uniform(rng, 0.02, 5.5, n) / kappa)
        in_range = (kappa > 0) & (d2 >= 0.3) & (d2 <= 3000.0)
        d2 = np.where(in_range, d2, 1.0)
        ox, oy = ex * d2, ey * d2
    # offsets count from the rectangle's middle, or (aimed: 70 %) from the corner that faces the centre: then that corner
    # pixel, or a neighbour of it, is the lattice minimum and its q is the target
    corner = (cls == "aimed") & (rng.random(n) < 0.7)
    hx, hy = 0.5 * (ncols - 1), 0.5 * (nrows - 1)
    mx = x0 + hx + np.where(corner, np.sign(ox) * hx, 0.0) + ox
    my = y0 + hy + np.where(corner, np.sign(oy) * hy, 0.0) + oy
    rec = np.stack([a, b, c, np.ones(n), mx, my], axis=1).astype(np.float32)
    is_free = cls.startswith("free")
    free = np.full(n, is_free)
    if is_free:
        op = _log_uniform(rng, 0.5 / 255.0, 1.0, n)
    else:
        # aimed at the float64 lattice minimum of the float32 record
        q, _, inside, _ = _lattice(rec, x0, y0, ncols, nrows)
        qmin = np.where(inside, q, np.inf).min(axis=(1, 2))
        # (along the axis the terms of q reach 1e3 .. 1e5 and the near window 5e-4 .. 5e-2: the coarse rungs weigh more)
        wts = np.where(EPS_LADDER >= 1e-3, 4.0, 1.0) if cls == "aimed_axis" else np.ones(EPS_LADDER.size)
        wts = np.concatenate([wts, wts, [1.0]])
        eps = rng.choice(np.concatenate([EPS_LADDER, -EPS_LADDER, [0.0]]), n, p=wts / wts.sum())
        with np.errstate(all="ignore"):
            op = np.clip(np.exp(qmin * (1.0 + eps)) / 255.0, 0.0, 2.0)
    op32 = op.astype(np.float32)
    ok = in_range & np.isfinite(op) & (op32 >= np.float32(1e-30)) & (op32 <= np.float32(1.0))
    rec[:, 3] = op32
    return rec[ok], geo[ok], kind[ok], free[ok]


@lru_cache(maxsize=None)
def family(name, n=N_RECORDS):
    """-> dict: rec f32[n, 6] = (a, b, c, op, mx, my), geo i32[n, 6], kind i8[n], free bool[n]; seeded, shuffled."""
    rng = np.random.default_rng(FAMILIES[name])
    parts = []
    for ci, (cls, share) in enumerate(CLASSES):
        want = n - sum(p[0].shape[0] for p in parts) if ci == len(CLASSES) - 1 else int(round(share * n))
        have = 0
        while have < want:
            p = _draw(rng, name, cls, max(2 * want, 1000))
            p = tuple(x[:want - have] for x in p)
            parts.append(p)
            have += p[0].shape[0]
    order = rng.permutation(n)
    rec, geo, kind, free = (np.concatenate([p[i] for p in parts])[order] for i in range(4))
    for arr in (rec, geo, kind, free):
        arr.setflags(write=False)
    return dict(rec=rec, geo=geo, kind=kind, free=free)


@lru_cache(maxsize=None)
def reference(name, n=N_RECORDS, chunk=10_000):
    """The float64 reference of family `name`, computed once: packed masks u32[n, 8] `inside`, `cv`, `ci`; counts n_cv,
    n_near (in-image pixels); qmin, cmin, S_pix, S_rect; `must_drop` (complete_class)."""
    fam = family(name, n)
    x0, y0, ncols, nrows = rectangle(fam["geo"])
    out = {k: [] for k in ("inside", "cv", "ci", "n_cv", "n_near", "qmin", "S_pix")}
    for s in range(0, n, chunk):
        sl = slice(s, s + chunk)
        c = classify(fam["rec"][sl], x0[sl], y0[sl], ncols[sl], nrows[sl])
        for k in ("inside", "cv", "ci"):
            out[k].append(pack_bits(c[k]))
        out["n_cv"].append(c["cv"].sum(axis=1))
        out["n_near"].append((c["inside"] & ~c["cv"] & ~c["ci"]).sum(axis=1))
        out["qmin"].append(c["qmin"])
        out["S_pix"].append(c["S_pix"])
    ref = {k: np.concatenate(v) for k, v in out.items()}
    ref["cmin"] = continuous_min(fam["rec"], x0, y0, ncols, nrows)
    ref["S_rect"] = s_rect(fam["rec"], x0, y0, ncols, nrows)
    ref["must_drop"] = complete_class(fam["rec"], ref["cmin"], ref["S_rect"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def pack_bits(b):
    """bool [n, 256] -> u32 [n, 8], bit i of the row in word i >> 5 at position i & 31"""
    return np.packbits(np.ascontiguousarray(b), axis=1, bitorder="little").view("<u4")
