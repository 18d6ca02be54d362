"""Closed-form float64 backward of rasterize_to_pixels with per-row error scales -- TEST INFRASTRUCTURE ONLY.

Why it exists: the backward comparisons that use max|a - b| / max|b| over a whole gradient tensor say nothing
about the many rows that are small next to the tensor's largest entry.  This file evaluates SURVEY A.6 per tile
in plain numpy (independent of autograd; `oracle/gsplat_torch.py` is the cross-check) and returns, next to every
gradient row G, two scales that bound what ANY float32 evaluation of the same sums can be off by:

  S  the sum over pixels of the magnitudes of the row's terms, no cancellation allowed.  Per (splat g, pixel p):
         M_gp = sum_d (|c_gd| T_before + S_abs_after_d / (1 - alpha)) |v_rc_pd|
                + T_final / (1 - alpha) (|v_ra_p| + |bg| . |v_rc_p|),       S_abs_after = sum_{k>g} |c_k| vis_k
     and the outer factors in absolute value: exp(-sigma) M (opacity), alpha_raw M (dx^2/2, |dx dy|, dy^2/2) (conic),
     alpha_raw M (|a dx| + |b dy|, |b dx| + |c dy|) (mean, and absgrad), vis |v_rc| (colour), T_final |v_rc|
     (background).  An evaluation in another order, with FMA, with the running-dot-product form of the
     wave-per-tile kernel (W = T_final (v_a - bg.v) - sum_k vis_k Q_k), adds the same terms: its rounding
     error is a small multiple of 2^-24 S.
  A  the same sum with every pixel's terms multiplied by 0.5 / T_final_p.  Every gsplat-shaped backward rebuilds
     the transmittance behind the last splat from the STORED float32 render_alphas: T_final = 1 - alpha_stored.
     Half an ulp of a float32 next to 1 is 2^-25, i.e. a relative error 2^-25 / T_final on every term of that
     pixel (T_final > 1e-4 always, so at most 2^-25 * 1e4).  2^-24 A is that error, summed with no cancellation.

The bar a float32 backward is judged by is, row by row,   |x - G| <= 2^-24 (K S + A),   exactly 0 where S == 0.

`dtype=np.float32` replays the same formulas in float32 with transmittances rebuilt from the float32
render_alphas: the noise floor of the computation itself, from which the tests take K (no kernel involved).

Decisions as in oracle/gsplat_oracle.py: `sigma < 0` or `alpha < 1/255` skips the pair, the walk stops before the
splat that would take T to <= 1e-4, alpha is clamped at 0.999 and a clamped alpha passes no gradient on to sigma
and the opacity.  A masked tile contributes nothing (its pixels show the background: they count in
v_backgrounds).  Entries of flatten_ids outside [0, C N) are skipped.

The sums over channels are taken first (Q_gp = sum_d c_gd v_rc_pd, one matrix product per tile), so every
intermediate is [G splats, P pixels] whatever D is.
"""
from __future__ import annotations

import numpy as np

from oracle import gsplat_oracle as O

ALPHA_MIN = 1.0 / 255.0
ALPHA_MAX = 0.999
T_EPS = 1e-4
EPS24 = 2.0 ** -24
OUTPUTS = ("means2d", "conics", "colors", "opacities", "absgrad", "backgrounds")


def _suffix_sum(x):
    """R[g] = sum_{k > g} x[k] along axis 0 (built from the far end: no subtraction of nearly equal sums)."""
    r = np.zeros_like(x)
    if x.shape[0] > 1:
        r[:-1] = np.cumsum(x[:0:-1], axis=0, dtype=x.dtype)[::-1]
    return r


def _tiles(C, H, W, ts, offs, I, masks):
    th, tw = offs.shape[1], offs.shape[2]
    flat = offs.reshape(-1)
    for c in range(C):
        for ty in range(th):
            for tx in range(tw):
                t = (c * th + ty) * tw + tx
                y0, x0 = ty * ts, tx * ts
                y1, x1 = min(y0 + ts, H), min(x0 + ts, W)
                if y1 <= y0 or x1 <= x0:
                    continue
                s = int(flat[t])
                e = int(flat[t + 1]) if t + 1 < flat.shape[0] else I
                s = min(max(s, 0), I)
                e = min(max(e, s), I)
                masked = masks is not None and not bool(masks[c, ty, tx])
                yield c, y0, y1, x0, x1, s, e, masked


def _blend(dt, m2, cn, op, g, y0, y1, x0, x1):
    """The forward of one tile in `dt`: everything the backward needs, [G splats, P pixels]."""
    hh, ww = y1 - y0, x1 - x0
    P = hh * ww
    G = g.shape[0]
    px = np.broadcast_to((np.arange(x0, x1, dtype=dt) + dt(0.5))[None, :], (hh, ww)).reshape(-1)
    py = np.broadcast_to((np.arange(y0, y1, dtype=dt) + dt(0.5))[:, None], (hh, ww)).reshape(-1)
    with np.errstate(all="ignore"):
        dx = m2[g, 0][:, None] - px[None]
        dy = m2[g, 1][:, None] - py[None]
        ca, cb, cc = cn[g, 0][:, None], cn[g, 1][:, None], cn[g, 2][:, None]
        sig = dt(0.5) * (ca * dx * dx + cc * dy * dy) + cb * dx * dy
        ex = np.exp(-sig)
        araw = op[g][:, None] * ex
        a = np.minimum(araw, dt(ALPHA_MAX))
        ok = ~((sig < 0) | (a < dt(ALPHA_MIN))) & np.isfinite(a)
    ae = np.where(ok, a, dt(0))
    om = dt(1) - ae
    Ta = np.cumprod(om, axis=0, dtype=dt)
    Tb = np.concatenate([np.ones((1, P), dt), Ta[:-1]], axis=0)
    term = ok & (Ta <= dt(T_EPS))
    first = np.where(term.any(0), term.argmax(0), G)
    live = ok & (np.arange(G)[:, None] < first[None])
    Tfin = np.prod(np.where(live, om, dt(1)), axis=0, dtype=dt)
    ex = np.where(live, ex, dt(0))
    araw = np.where(live, araw, dt(0))
    return dict(dx=dx, dy=dy, ca=ca, cb=cb, cc=cc, ex=ex, araw=araw, ae=ae, live=live, Tb=Tb, Tfin=Tfin)


def _as(a, dt, shape):
    return np.asarray(a).astype(dt).reshape(shape)


def unstable_bwd(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets,
                 flatten_ids, masks=None, unstable_rel=2e-5, return_stats=False):
    """bool[C,H,W]: the numpy oracle's `unstable` flag (an alpha, sigma or transmittance within its window of a hard
    threshold of the FORWARD) or some live alpha_raw within `unstable_rel` (relative) of the clamp at 0.999: there the
    forward is continuous but the gradient through that pair switches on or off.  Tests give these pixels zero
    upstream gradient.  return_stats: also {"live": live (splat, pixel) pairs, "clamped": those with a clamped alpha}."""
    C, N = np.asarray(opacities).shape
    H, W = int(image_height), int(image_width)
    offs = np.asarray(isect_offsets, dtype=np.int64)
    fids = np.asarray(flatten_ids, dtype=np.int64).reshape(-1)
    D = np.asarray(colors).shape[-1]
    m2, cn = _as(means2d, np.float32, (-1, 2)), _as(conics, np.float32, (-1, 3))
    co, op = _as(colors, np.float32, (-1, D)), _as(opacities, np.float32, (-1,))
    shp = (C, N)
    bad = (fids < 0) | (fids >= C * N)
    if bad.any():      # a stand-in per camera, far outside every frame with opacity 0: skipped, and near no threshold
        fids = np.where(bad, N, (fids // N) * (N + 1) + fids % N)

        def grown(a, row):
            a = a.reshape((C, N) + a.shape[1:])
            return np.concatenate([a, np.broadcast_to(np.asarray(row, np.float32), (C, 1) + a.shape[2:])], axis=1)

        m2, cn = grown(m2, [-1e6, -1e6]).reshape(-1, 2), grown(cn, [1.0, 0.0, 1.0]).reshape(-1, 3)
        co, op = grown(co, np.zeros(D)).reshape(-1, D), grown(op, 0.0).reshape(-1)
        shp = (C, N + 1)
    un = O.rasterize_to_pixels(m2.reshape(*shp, 2), cn.reshape(*shp, 3), co.reshape(*shp, D), op.reshape(shp), W, H,
                               tile_size, offs, fids, masks=masks, return_unstable=True, unstable_rel=unstable_rel)[3]
    un = un.copy()
    m2d, cnd, opd = m2.astype(np.float64), cn.astype(np.float64), op.astype(np.float64)
    n_live = n_clamped = 0
    for c, y0, y1, x0, x1, s, e, masked in _tiles(C, H, W, tile_size, offs, fids.shape[0], masks):
        if masked or e <= s:
            continue
        b = _blend(np.float64, m2d, cnd, opd, fids[s:e], y0, y1, x0, x1)
        near = b["live"] & (np.abs(b["araw"] - ALPHA_MAX) <= unstable_rel * ALPHA_MAX)
        un[c, y0:y1, x0:x1] |= near.any(0).reshape(y1 - y0, x1 - x0)
        n_live += int(b["live"].sum())
        n_clamped += int((b["live"] & (b["araw"] > ALPHA_MAX)).sum())
    if return_stats:
        return un, {"live": n_live, "clamped": n_clamped}
    return un


def rasterize_bwd(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets,
                  flatten_ids, v_render_colors, v_render_alphas, backgrounds=None, masks=None, dtype=np.float64,
                  _skip_every=None, stored_means2d=False):
    """Inputs as rasterize_to_pixels ([C,N,*], isect_offsets i32[C,th,tw], flatten_ids i32[I]) plus the upstream
    gradients v_render_colors [C,H,W,D], v_render_alphas [C,H,W,1] (or [C,H,W]).
    -> {"G": gradients, "S": term magnitudes, "A": stored-alpha magnitudes} (float64), each a dict with
       means2d [C,N,2], conics [C,N,3], colors [C,N,D], opacities [C,N], absgrad [C,N,2] (S and A of absgrad ARE
       those of means2d) and backgrounds [C,D] (None without backgrounds); "render_alphas" [C,H,W] as computed here.
    dtype: np.float64 = the reference; np.float32 = the noise-floor replay (see the module text).
    `_skip_every` (for the reference's own mutation tests): the gradient contributions of the first entry of every
    `_skip_every`-entry batch of each tile's list are dropped, as a staging loop that loses a slot would.
    stored_means2d (for callers whose reference is a float64 CHAIN that ends in this operator, oracle/param_grad_f64.py;
    the operator-level tests hand both sides the same float32 means2d and leave it off): A of means2d / absgrad also
    carries the rounding of the float32 means2d the backward reads.  mean2d = f x / z + c is four roundings downstream
    of the camera-space mean (the dot product, the divide, the multiply, the add), each at most 2^-24 of a magnitude that
    is at most |mean2d| for a principal point inside the frame, so dx = mean_x - pixel_x inherits |d dx| <= 4 2^-24 |mean_x|
    whatever |dx| is, and v_mean = -alpha_raw v_alpha (a dx + b dy, b dx + c dy) is linear in it:
    4 alpha_raw M (|a| |mean_x| + |b| |mean_y|, |b| |mean_x| + |c| |mean_y|) per pair, no cancellation.  A row fed by one
    pixel next to its own centre has S ~ |dx| -> 0 and nothing but this term.  A["absgrad"] IS A["means2d"] (one array, as
    S["absgrad"] is S["means2d"]), so it carries the term as well: the absolute gradient sums |alpha_raw v_alpha (a dx + b dy)|
    over the same pairs and inherits the same rounding of dx, pair by pair."""
    dt = np.dtype(dtype).type
    replay = dt is np.float32
    opacities = np.asarray(opacities)
    C, N = opacities.shape
    D = np.asarray(colors).shape[-1]
    H, W = int(image_height), int(image_width)
    m2, cn = _as(means2d, dt, (-1, 2)), _as(conics, dt, (-1, 3))
    co, op = _as(colors, dt, (-1, D)), _as(opacities, dt, (-1,))
    v_rc = _as(v_render_colors, dt, (C, H, W, D))
    v_ra = _as(v_render_alphas, dt, (C, H, W))
    bg = None if backgrounds is None else _as(backgrounds, dt, (C, D))
    offs = np.asarray(isect_offsets, dtype=np.int64)
    fids = np.asarray(flatten_ids, dtype=np.int64).reshape(-1)
    masks = None if masks is None else np.asarray(masks)
    shp = {"means2d": (C * N, 2), "conics": (C * N, 3), "colors": (C * N, D), "opacities": (C * N,)}
    Gd = {k: np.zeros(s, np.float64) for k, s in shp.items()}
    Sd = {k: np.zeros(s, np.float64) for k, s in shp.items()}
    Ad = {k: np.zeros(s, np.float64) for k, s in shp.items()}
    Gabs = np.zeros((C * N, 2), np.float64)
    Gb, Sb, Ab = (np.zeros((C, D), np.float64) for _ in range(3))
    r_alpha = np.zeros((C, H, W), np.float64)

    def rows(*cols):
        return np.stack([x.sum(1) for x in cols], -1)

    for c, y0, y1, x0, x1, s, e, masked in _tiles(C, H, W, tile_size, offs, fids.shape[0], masks):
        P = (y1 - y0) * (x1 - x0)
        vrc = v_rc[c, y0:y1, x0:x1].reshape(P, D)
        vra = v_ra[c, y0:y1, x0:x1].reshape(P)
        avrc = np.abs(vrc)
        g = fids[s:e]
        keep = (g >= 0) & (g < C * N)
        pos = np.arange(g.shape[0])[keep]
        g = g[keep]
        if masked or g.shape[0] == 0:        # the pixels show the background, T_final = 1
            if bg is not None:
                Gb[c] += vrc.sum(0, dtype=np.float64)
                Sb[c] += avrc.sum(0, dtype=np.float64)
                Ab[c] += 0.5 * avrc.sum(0, dtype=np.float64)
            continue
        b = _blend(dt, m2, cn, op, g, y0, y1, x0, x1)
        dx, dy, ca, cb, cc, ex, araw, ae, live, Tb, Tfin = (b[k] for k in ("dx", "dy", "ca", "cb", "cc", "ex", "araw", "ae",
                                                                           "live", "Tb", "Tfin"))
        if replay:      # what a backward reads: T_final = 1 - render_alphas, both float32; every T_before scales with it
            Tf2 = np.float32(1) - (np.float32(1) - Tfin)
            Tb = Tb * (Tf2 / Tfin)[None]
            Tfin = Tf2
        r_alpha[c, y0:y1, x0:x1] = (dt(1) - Tfin).reshape(y1 - y0, x1 - x0)
        vis = np.where(live, ae * Tb, dt(0))
        cg = co[g]
        ra = dt(1) / (dt(1) - ae)
        Q = cg @ vrc.T                                   # [G,P]  sum_d c_gd v_rc_pd
        Qa = np.abs(cg) @ avrc.T
        tail, tail_a = vra, np.abs(vra)
        if bg is not None:
            tail = tail - vrc @ bg[c]
            tail_a = tail_a + avrc @ np.abs(bg[c])
        va = Tb * Q - ra * _suffix_sum(vis * Q) + (Tfin * tail)[None] * ra
        M = Tb * Qa + ra * _suffix_sum(vis * Qa) + (Tfin * tail_a)[None] * ra
        flow = live & (araw <= dt(ALPHA_MAX))            # a clamped alpha passes nothing on
        va = np.where(flow, va, dt(0))
        M = np.where(flow, M, dt(0))
        w = (dt(0.5) / Tfin)[None]
        vs = -araw * va
        Ms = araw * M
        gx, gy = vs * (ca * dx + cb * dy), vs * (cb * dx + cc * dy)
        fc = (dt(0.5) * dx * dx, np.abs(dx * dy), dt(0.5) * dy * dy)
        fm = (np.abs(ca * dx) + np.abs(cb * dy), np.abs(cb * dx) + np.abs(cc * dy))
        out = {
            "colors": (vis @ vrc, vis @ avrc, (vis * w) @ avrc),
            "opacities": ((ex * va).sum(1), (ex * M).sum(1), (ex * M * w).sum(1)),
            "conics": (rows(dt(0.5) * vs * dx * dx, vs * dx * dy, dt(0.5) * vs * dy * dy),
                       rows(*(Ms * f for f in fc)), rows(*(Ms * w * f for f in fc))),
            "means2d": (rows(gx, gy), rows(*(Ms * f for f in fm)), rows(*(Ms * w * f for f in fm))),
        }
        if stored_means2d:
            mx, my = np.abs(m2[g, 0])[:, None], np.abs(m2[g, 1])[:, None]
            g_, s_, a_ = out["means2d"]
            out["means2d"] = (g_, s_, a_ + dt(4) * rows(Ms * (np.abs(ca) * mx + np.abs(cb) * my),
                                                          Ms * (np.abs(cb) * mx + np.abs(cc) * my)))
        ab = rows(np.abs(gx), np.abs(gy))
        if _skip_every:
            lost = (pos % int(_skip_every)) == 0
            ab = np.where(lost[:, None], 0.0, ab)
            out = {k: tuple(np.where(lost.reshape((-1,) + (1,) * (x.ndim - 1)), 0.0, x) for x in v) for k, v in out.items()}
        for k, (g_, s_, a_) in out.items():
            np.add.at(Gd[k], g, g_)
            np.add.at(Sd[k], g, s_)
            np.add.at(Ad[k], g, a_)
        np.add.at(Gabs, g, ab)
        if bg is not None:
            Gb[c] += (Tfin[:, None] * vrc).sum(0, dtype=np.float64)
            Sb[c] += (Tfin[:, None] * avrc).sum(0, dtype=np.float64)
            Ab[c] += 0.5 * avrc.sum(0, dtype=np.float64)

    def shaped(d):
        o = {k: v.reshape((C, N) + v.shape[1:]) for k, v in d.items()}
        o["absgrad"] = o["means2d"]
        o["backgrounds"] = None
        return o

    G_, S_, A_ = shaped(Gd), shaped(Sd), shaped(Ad)
    G_["absgrad"] = Gabs.reshape(C, N, 2)
    if bg is not None:
        G_["backgrounds"], S_["backgrounds"], A_["backgrounds"] = Gb, Sb, Ab
    return {"G": G_, "S": S_, "A": A_, "render_alphas": r_alpha}


def row_ratio(x, ref, name):
    """-> (ratio, off): ratio = (|x - G| - 2^-24 A)+ / (2^-24 S) for every entry of output `name` with S > 0 (0
    elsewhere); off = the largest |x| over the entries with S == 0, which must be exactly 0.  The per-row bar
    |x - G| <= 2^-24 (K S + A) is `ratio.max() <= K and off == 0`."""
    G, S, A = ref["G"][name], ref["S"][name], ref["A"][name]
    x = np.asarray(x, np.float64).reshape(G.shape)
    err = np.abs(x - G)
    nz = S > 0
    ratio = np.zeros_like(G)
    ratio[nz] = np.maximum(err[nz] - EPS24 * A[nz], 0.0) / (EPS24 * S[nz])
    ratio[~np.isfinite(x)] = np.inf
    off = float(np.abs(x[~nz]).max()) if (~nz).any() else 0.0
    return ratio, (off if np.isfinite(off) else np.inf)
