"""Hand-built frames for the tile walk of the rasterizers -- TEST INFRASTRUCTURE ONLY.

A frame is 136 x 100 pixels: 9 x 7 tiles of 16 x 16, the last column 8 pixels wide, the last row 4 pixels high.  Every
tile is one case with its own records and its own list: `isect_offsets` and `flatten_ids` are written down, not sorted,
and a record is listed by its own tile only.  Three frames:

    "finite"      contour cases (the 1/255 contour around exactly one pixel of a tile, a partial tile, a half tile) and
                  list cases (lengths and cull patterns around the batch of 64, saturation at chosen positions); the
                  frame's last tile has 128 entries and ends at n_isects
    "finite129"   degenerate but finite records, in front of and behind the records that finish their tile; 129 entries
                  in the last tile
    "nonfinite"   NaN / +-inf in one conic entry, the opacity or the mean of one record per tile

The float64 reference here walks a tile's list for all its pixels at once (blend_f64.walk does one pixel at a time;
tests/test_raster_edges_cpu.py holds the two against each other) and reports, per pixel, the smallest distance of any
decision from its threshold: |ln(255 op exp(-sigma))| for valid / not valid, |T' / 1e-4 - 1| for terminate, |sigma| / S for
the sign of sigma (S = 0: sigma is exactly 0 in every arithmetic).  The finite frames keep every decision >= 1e-4 away, so
no pixel of them is "unstable" (2e-5) and none may be left out of a comparison.

Non-finite values follow the literal formula, `if sigma < 0 or alpha < 1/255: skip` with alpha = fmin(0.999, op
exp(-sigma)): a NaN sigma or alpha fails both comparisons and the record blends at 0.999 (csrc/raster_common.h).  One
exception: an infinite centre, where the literal sum is inf - inf or 0 * inf for some pixels and the outcome depends on
the order of evaluation.  There the reference evaluates in the kernels' order, ((a/2 dx + b dy) dx) + (c/2 dy) dy: with
b = 0 an infinite x is skipped (sigma = +inf) and an infinite y blends (0 * inf = NaN).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

W, H, TILE = 136, 100, 16
TW, TH = 9, 7
ALPHA_MIN, ALPHA_MAX, T_EPS = 1.0 / 255.0, 0.999, 1e-4
MARGIN = 1e-4
F32 = np.float32
NAN, INF = float("nan"), float("inf")


def _conic_of_cov(s1, s2, theta):
    """conic (a, b, c) of the Gaussian with standard deviations s1 along angle theta and s2 across it"""
    co, si = np.cos(theta), np.sin(theta)
    cxx = co * co * s1 * s1 + si * si * s2 * s2
    cyy = si * si * s1 * s1 + co * co * s2 * s2
    cxy = co * si * (s1 * s1 - s2 * s2)
    det = cxx * cyy - cxy * cxy
    return cyy / det, -cxy / det, cxx / det


def indefinite_by_rounding():
    """Two float32 conics with a c < b^2 in exact arithmetic whose determinant test `a * c - b * b > 0` passes when the
    compiler contracts it into one fused multiply-add: fma(a, c, -fl(b b)) for the first, fma(-b, b, fl(a c)) for the
    second.  (With two separately rounded products no indefinite conic passes: rounding is monotone.)"""
    rng = np.random.default_rng(99)
    a = rng.uniform(0.02, 0.04, 200_000).astype(F32).astype(np.float64)
    c = rng.uniform(0.02, 0.04, 200_000).astype(F32).astype(np.float64)
    ac = a * c
    b0 = np.sqrt(ac).astype(F32)
    out = []
    for form in (0, 1):
        for b in (b0.astype(np.float64), np.nextafter(b0, F32(1)).astype(np.float64)):
            bb = b * b
            ok = (bb > ac) & ((bb.astype(F32).astype(np.float64) < ac) if form == 0 else (ac.astype(F32).astype(np.float64) > bb))
            if ok.any():
                i = int(np.argmax(ok))
                out.append((float(a[i]), float(b[i]), float(c[i])))
                break
    assert len(out) == 2, out
    return out


class _Frame:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rec = []          # (mx, my, a, b, c, op)
        self.lists = {}        # (tx, ty) -> [record index]
        self.names = {}        # (tx, ty) -> case name
        self.expect = {}       # (tx, ty) -> dict of expectations the CPU test checks on the float64 reference
        self.free = [(tx, ty) for ty in range(TH - 1) for tx in range(TW - 1)]       # whole tiles not yet used

    def add(self, mx, my, a, b, c, op):
        self.rec.append((mx, my, a, b, c, op))
        return len(self.rec) - 1

    def mid(self, t):
        return t[0] * 16 + 8.0, t[1] * 16 + 8.0

    # a record that covers the tile almost uniformly (q <= 1e-3 over it): alpha is op (1.0: the clamp, 0.999) everywhere.
    # Its centre is a pixel CORNER, so that no pixel centre has sigma within 1e-6 of 0 (the numpy oracle's window).
    def cover(self, t, op, jitter=True):
        x, y = self.mid(t)
        j = self.rng.integers(-1, 2, 2) if jitter else (0, 0)
        return self.add(x + j[0], y + j[1], 1e-5, 0.0, 1e-5, op)

    def K(self, t):            # kept, faint: a list of these never saturates (0.988^193 = 0.1)
        return self.cover(t, self.rng.uniform(0.008, 0.012))

    def Wl(self, t):           # wall: two of them finish every pixel (T = 1e-3, then 1e-6 <= 1e-4)
        return self.cover(t, 1.0, jitter=False)

    def C(self, t):            # culled: a sharp record 60 pixels away from the tile's middle
        x, y = self.mid(t)
        phi = self.rng.uniform(0, 2 * np.pi)
        return self.add(x + 60 * np.cos(phi), y + 60 * np.sin(phi), 1.0, 0.0, 1.0, 0.5)

    def tile(self, name, pattern_or_ids, t=None, **expect):
        """pattern: string of K / W / C, or a list of record indices / letters"""
        if t is None:
            t = self.free.pop(0)
        ids = []
        for p in pattern_or_ids:
            ids.append({"K": self.K, "W": self.Wl, "C": self.C}[p](t) if isinstance(p, str) else p)
        assert t not in self.lists
        self.lists[t], self.names[t], self.expect[t] = ids, name, expect
        return t

    def finish(self):
        n = len(self.rec)
        rec = np.array(self.rec, np.float64)
        offs = np.zeros((1, TH, TW), np.int32)
        fids = []
        for ty in range(TH):
            for tx in range(TW):
                offs[0, ty, tx] = len(fids)
                fids += self.lists.get((tx, ty), [])
        rng = np.random.default_rng(4242)
        colors = rng.uniform(0.05, 1.0, (1, n, 4)).astype(F32)
        colors[..., 3] = rng.uniform(1.0, 20.0, (1, n)).astype(F32)
        with np.errstate(all="ignore"):
            return dict(means2d=rec[None, :, 0:2].astype(F32), conics=rec[None, :, 2:5].astype(F32),
                        opacities=rec[None, :, 5].astype(F32), colors=colors, isect_offsets=offs,
                        flatten_ids=np.array(fids, np.int32), width=W, height=H, tile_size=TILE,
                        names=dict(self.names), expect=dict(self.expect), lists=dict(self.lists))


def _contour_cases(f):
    """One record whose 1/255 contour holds exactly one pixel, behind it a faint cover.  Isotropic: conic 12 I, opacity
    0.5 (L = ln 127.5 = 4.85): a pixel 0.57 away has q = 1.9, its neighbours (1.4, 0.4) away q = 12.7.  Needle: long axis
    (s 30) across the diagonal that points into the tile, s 0.4 along it, centre (0.6, 0.6) outside the corner."""
    corners = {"tl": (0, 0, -1, -1), "tr": (15, 0, 1, -1), "bl": (0, 15, -1, 1), "br": (15, 15, 1, 1)}
    for kind in ("round", "needle"):
        for cn, (cx, cy, sx, sy) in corners.items():
            t = f.free.pop(0)
            px, py = t[0] * 16 + cx + 0.5, t[1] * 16 + cy + 0.5
            if kind == "round":
                r = f.add(px + 0.4 * sx, py + 0.4 * sy, 12.0, 0.0, 12.0, 0.5)
            else:
                a, b, c = _conic_of_cov(30.0, 0.4, np.arctan2(sx, -sy))
                r = f.add(px + 0.6 * sx, py + 0.6 * sy, a, b, c, 0.5)
            f.tile(f"contour-{kind}-{cn}", [r, "K"], t, only=[(cx, cy)], rec=r)
    # an edge midpoint: the centre 0.4 outside the middle of the top edge / of the left edge
    t = f.free.pop(0)
    r = f.add(t[0] * 16 + 7.5, t[1] * 16 + 0.1, 12.0, 0.0, 12.0, 0.5)
    f.tile("contour-edge-top", [r, "K"], t, only=[(7, 0)], rec=r)
    t = f.free.pop(0)
    r = f.add(t[0] * 16 + 0.1, t[1] * 16 + 8.5, 12.0, 0.0, 12.0, 0.5)
    f.tile("contour-edge-left", [r, "K"], t, only=[(0, 8)], rec=r)
    # the last in-image pixel of a partial tile: the centre sits on the frame's edge, half a pixel from the last pixel
    # inside and from the first one outside, which would have been valid (q = 1.5) had it existed
    t = (TW - 1, 2)
    r = f.add(float(W), t[1] * 16 + 5.5, 12.0, 0.0, 12.0, 0.5)
    f.tile("contour-partial-x", [r, "K"], t, only=[(7, 5)], rec=r)
    t = (3, TH - 1)
    r = f.add(t[0] * 16 + 9.5, float(H), 12.0, 0.0, 12.0, 0.5)
    f.tile("contour-partial-y", [r, "K"], t, only=[(9, 3)], rec=r)
    t = (TW - 1, 3)
    a, b, c = _conic_of_cov(30.0, 0.4, np.pi / 2)          # long axis along y, outside the frame's right edge
    r = f.add(float(W) + 0.1, t[1] * 16 + 20.0, a, b, c, 0.5)
    f.tile("contour-needle-partial-x", [r, "K"], t, rec=r, column=7)
    # valid only in the lower half tile (rows 8..15): centre below the tile
    t = f.free.pop(0)
    r = f.add(t[0] * 16 + 8.0, t[1] * 16 + 17.0, 0.5, 0.0, 0.5, 0.5)
    f.tile("contour-lower-half", [r, "K"], t, rec=r, rows=(8, 16))
    # the centre exactly on the rectangle's border (the first pixel centre's column / the last one's row)
    t = f.free.pop(0)
    r = f.add(t[0] * 16 + 0.5, t[1] * 16 + 6.2, 3.0, 0.0, 3.0, 0.5)
    f.tile("contour-centre-on-border-x", [r, "K"], t, rec=r)
    t = f.free.pop(0)
    r = f.add(t[0] * 16 + 11.3, t[1] * 16 + 15.5, 3.0, 1.0, 3.0, 0.5)
    f.tile("contour-centre-on-border-y", [r, "K"], t, rec=r)
    # 255 op just above / below 1: a record 0.02 off a pixel centre, blended there only / nowhere
    for nm, op in (("above", (1.0 + 1e-3) / 255.0), ("below", (1.0 - 1e-3) / 255.0)):
        t = f.free.pop(0)
        r = f.add(t[0] * 16 + 5.52, t[1] * 16 + 9.5, 0.01, 0.0, 0.01, op)
        f.tile(f"contour-op-{nm}-1/255", [r, "K"], t, rec=r, only=[(5, 9)] if nm == "above" else [])


def _list_cases(f, last_len):
    for n in (0, 1, 2, 63, 64, 65, 127, 129, 192, 193):
        f.tile(f"len-{n}", "K" * n, never_saturates=True)
    f.tile("len-128-mid", "K" * 128, never_saturates=True)
    # what compaction keeps of a batch
    f.tile("keep-none", "C" * 64 + "KKK")
    f.tile("keep-lane0", "K" + "C" * 63 + "K")
    f.tile("keep-lane63", "C" * 63 + "K" + "K")
    f.tile("keep-two", "K" + "C" * 62 + "K")
    f.tile("keep-63-first-culled", "C" + "K" * 63)
    f.tile("keep-63-last-culled", "K" * 63 + "C" + "K")
    f.tile("keep-every-other", "KC" * 64 + "K")
    f.tile("culled-batch-between", "K" * 64 + "C" * 64 + "K" * 64)
    # saturation: the second wall crosses T = 1e-4 and is not blended; last_ids stays at the wall before it
    f.tile("sat-second-record", "WW" + "K" * 5, last=0)
    f.tile("sat-even-kept", "KWW" + "K" * 5, last=1)
    f.tile("sat-odd-kept", "KKWW" + "K" * 5, last=2)
    f.tile("sat-odd-kept-even-listed", "CKCKWCWK", last=4)
    f.tile("sat-last-of-batch", "K" * 62 + "WW" + "K" * 70, last=62)
    f.tile("sat-first-of-second-batch", "K" * 63 + "WW" + "K" * 70, last=63)
    f.tile("sat-behind-culled-batch", "C" * 64 + "KWW" + "K" * 3, last=65)
    f.tile("sat-then-long-tail", "WW" + "K" * 191, last=0)
    # the frame's last tile (8 x 4 pixels): its list ends at n_isects
    f.tile(f"last-tile-{last_len}", "K" * last_len, (TW - 1, TH - 1), never_saturates=True)


DEGENERATE = {          # name -> (a, b, c, op); the centre sits (0.25, 0.1) off the tile's middle: no pixel has |dx| = |dy|
    "a-zero": (0.0, 0.0, 0.02, 0.5),
    "a-zero-c-zero": (0.0, 0.01, 0.0, 0.5),
    "c-zero-b-set": (0.02, 0.01, 0.0, 0.5),
    "a-denormal": (1e-40, 0.0, 0.02, 0.5),
    "c-denormal-b-denormal": (0.02, 1e-41, 1e-39, 0.5),
    "a-negative": (-0.02, 0.0, 0.02, 0.5),
    "c-negative": (0.02, 0.0, -0.03, 0.5),
    "b-large": (0.02, 0.05, 0.02, 0.5),
    "op-zero": (0.02, 0.0, 0.02, 0.0),
    "op-negative": (0.02, 0.0, 0.02, -0.5),
    "op-one": (0.02, 0.0, 0.02, 1.0),
    "op-above-one": (0.02, 0.0, 0.02, 1.7),
}


def _degenerate_cases(f):
    kinds = dict(DEGENERATE)
    for i, (a, b, c) in enumerate(indefinite_by_rounding()):
        kinds[f"indefinite-by-rounding-{i}"] = (a, b, c, 0.5)
    for name, (a, b, c, op) in kinds.items():
        for where in ("before", "after"):
            t = f.free.pop(0)
            x, y = f.mid(t)
            if name.startswith("indefinite"):
                # q vanishes on a line of slope about -1 through the centre: from (-3.25, -2.9) off the tile's first
                # pixel it misses the tile, and q grows like a PD ridge across the tile's corner
                x, y = t[0] * 16 - 3.5, t[1] * 16 - 3.0
            r = f.add(x + 0.25, y + 0.1, a, b, c, op)
            # after: two records pass between votes (raster_walk.h), so the walls are records 1 and 2 and the degenerate
            # record, the fourth, is blended onto pixels that all finished at the third
            f.tile(f"deg-{name}-{where}", [r, "W", "W", "K"] if where == "before" else ["K", "W", "W", r, "K"], t, rec=r)


NONFINITE = {           # name -> (field, value); fields: 0 mx, 1 my, 2 a, 3 b, 4 c, 5 op
    "a-nan": (2, NAN), "b-nan": (3, NAN), "c-nan": (4, NAN), "a-inf": (2, INF), "c-inf": (4, INF), "a-ninf": (2, -INF),
    "b-inf": (3, INF), "b-ninf": (3, -INF), "op-nan": (5, NAN), "op-inf": (5, INF), "op-ninf": (5, -INF),
    "mx-nan": (0, NAN), "my-nan": (1, NAN), "mx-inf": (0, INF), "mx-ninf": (0, -INF), "my-inf": (1, INF),
}


def _nonfinite_cases(f):
    """One non-finite value in one record per tile, at three places of a list: in front of faint records, behind them, and
    behind the walls that finish the tile.  Every other tile holds plain
    faint records: it must not change at all against the same frame without the non-finite records."""
    for name, (field, val) in NONFINITE.items():
        for where, pat in (("front", lambda r: [r, "K", "K"]), ("behind", lambda r: ["K", "K", "K", r, "K"]),
                           ("finished", lambda r: ["K", "W", "W", r, "K"])):
            if not f.free:
                break
            t = f.free.pop(0)
            x, y = f.mid(t)
            v = [x + 0.25, y + 0.1, 0.02, 0.0, 0.03, 0.5]
            v[field] = val
            r = f.add(*v)
            f.tile(f"nonfinite-{name}-{where}", pat(r), t, rec=r)


@lru_cache(maxsize=None)
def frame(kind):
    """-> dict: means2d f32[1, N, 2], conics f32[1, N, 3], opacities f32[1, N], colors f32[1, N, 4], isect_offsets
    i32[1, 7, 9], flatten_ids i32[I], width, height, tile_size, names / expect / lists per tile (tx, ty)."""
    if kind == "finite":
        f = _Frame(11)
        _contour_cases(f)
        _list_cases(f, 128)
    elif kind == "finite129":
        f = _Frame(13)
        _degenerate_cases(f)
        f.tile("last-tile-129", "K" * 129, (TW - 1, TH - 1), never_saturates=True)
    elif kind == "nonfinite":
        f = _Frame(12)
        _nonfinite_cases(f)
    else:
        raise KeyError(kind)
    for t in [(x, y) for y in range(TH) for x in range(TW)]:
        if t not in f.lists:
            f.tile("plain", "KKK", t)
    return f.finish()


def without_records(p, drop):
    """The frame with the records `drop` (indices) taken out of every list (the arrays keep them: ids stay the same)."""
    q = dict(p)
    fids = p["flatten_ids"]
    keep = ~np.isin(fids, np.asarray(list(drop)))
    offs = p["isect_offsets"].reshape(-1)
    new_offs = np.concatenate([[0], np.cumsum(keep)])[offs].astype(np.int32)
    q["isect_offsets"] = new_offs.reshape(p["isect_offsets"].shape)
    q["flatten_ids"] = fids[keep]
    return q


# ---- float64 reference: one tile's list for all its pixels ---------------------------------------------------------------
def reference(p, D=4, background=None):
    """-> dict: colors f64[H, W, D], alphas f64[H, W], last i32[H, W] (position in flatten_ids of the last record blended,
    0 if none: what last_ids holds), margin f64[H, W] (smallest distance of a decision from its threshold), n_blended."""
    m2 = p["means2d"][0].astype(np.float64)
    cn = p["conics"][0].astype(np.float64)
    op = p["opacities"][0].astype(np.float64)
    col = p["colors"][0, :, :D].astype(np.float64)
    offs = p["isect_offsets"].reshape(-1)
    fids = p["flatten_ids"]
    out_c = np.zeros((H, W, D))
    out_a = np.zeros((H, W))
    out_l = np.zeros((H, W), np.int32)
    out_m = np.full((H, W), np.inf)
    out_n = np.zeros((H, W), np.int32)
    for ti in range(TW * TH):
        tx, ty = ti % TW, ti // TW
        s, e = int(offs[ti]), int(offs[ti + 1]) if ti + 1 < offs.size else fids.size
        xs = np.arange(tx * 16, min(tx * 16 + 16, W))
        ys = np.arange(ty * 16, min(ty * 16 + 16, H))
        px, py = np.meshgrid(xs + 0.5, ys + 0.5)
        T = np.ones(px.shape)
        acc = np.zeros(px.shape + (D,))
        done = np.zeros(px.shape, bool)
        last = np.zeros(px.shape, np.int32)
        margin = np.full(px.shape, np.inf)
        nb = np.zeros(px.shape, np.int32)
        for k in range(s, e):
            g = fids[k]
            with np.errstate(all="ignore"):
                dx, dy = m2[g, 0] - px, m2[g, 1] - py
                t_a, t_c, t_b = 0.5 * cn[g, 0] * dx * dx, 0.5 * cn[g, 2] * dy * dy, cn[g, 1] * dx * dy
                sigma = t_a + t_c + t_b
                if np.isinf(m2[g]).any():                         # an infinite centre: see the module text
                    sigma = (0.5 * cn[g, 0] * dx + cn[g, 1] * dy) * dx + (0.5 * cn[g, 2] * dy) * dy
                S = np.abs(t_a) + np.abs(t_c) + np.abs(t_b)
                raw = op[g] * np.exp(-sigma)
                alpha = np.fmin(ALPHA_MAX, raw)
                valid = ~(sigma < 0) & ~(alpha < ALPHA_MIN)
                # distances from the thresholds, for finite records (a non-finite one has no threshold to be near to)
                m_sig = np.where(S > 0, np.abs(sigma) / np.where(S > 0, S, 1.0), np.inf)
                m_al = np.where(raw > 0, np.abs(np.log(np.where(raw > 0, raw, 1.0) / ALPHA_MIN)), np.inf)
                m_al = np.where(sigma < 0, np.inf, m_al)          # (skipped by its sign whatever alpha is)
                m = np.where(np.isfinite(sigma) & np.isfinite(raw), np.minimum(m_sig, m_al), np.inf)
                Tn = T * (1.0 - alpha)
                m_T = np.abs(Tn / T_EPS - 1.0)
            live = ~done
            margin = np.where(live, np.minimum(margin, m), margin)
            v = live & valid
            margin = np.where(v, np.minimum(margin, m_T), margin)
            term = v & (Tn <= T_EPS)
            b = v & ~term
            acc = np.where(b[..., None], acc + col[g] * (alpha * T)[..., None], acc)
            T = np.where(b, Tn, T)
            last = np.where(b, k, last)
            nb += b
            done |= term
        if background is not None:
            acc = acc + T[..., None] * np.asarray(background, np.float64)
        sl = (slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
        out_c[sl], out_a[sl], out_l[sl], out_m[sl], out_n[sl] = acc, 1.0 - T, last, margin, nb
    return dict(colors=out_c, alphas=out_a, last=out_l, margin=out_m, n_blended=out_n)


# ---- a hand-written dispatch list ------------------------------------------------------------------------------------------
def dispatch_list(split, total_tiles=TW * TH):
    """The rasterizer's dispatch-list buffer (include/street_crafter_amd.h, sc_tile_order_len) with the tiles `split`
    walked as two half-tile items and every other tile whole: the forward's list (tile << 2 | kind, padded with -1),
    the whole-tile list, "second list present" = 1, view slot 0.  At most total_tiles / 8 + 8 tiles can be split."""
    split = sorted(set(int(t) for t in split))
    n_fwd = total_tiles + total_tiles // 8 + 8
    assert len(split) <= n_fwd - total_tiles and all(0 <= t < total_tiles for t in split)
    items = [t << 2 | k for t in split for k in (1, 2)] + [t << 2 for t in range(total_tiles) if t not in split]
    fwd = np.full(n_fwd, -1, np.int32)
    fwd[:len(items)] = items
    whole = np.array([t << 2 for t in split] + [t << 2 for t in range(total_tiles) if t not in split], np.int32)
    return np.concatenate([fwd, whole, np.array([1, 0], np.int32)])


def split_sets(per_list=TW * TH // 8 + 8):
    """Every tile that is 16 rows high, dealt into lists of at most `per_list` tiles: each is split in one of them."""
    full = [ty * TW + tx for ty in range(TH - 1) for tx in range(TW)]
    return [full[i:i + per_list] for i in range(0, len(full), per_list)]
