"""Float64 forward of rasterize_to_pixels with a per-pixel error scale -- TEST INFRASTRUCTURE ONLY.

Why it exists: the forward comparisons of tests/test_gpu_parity.py hold the HIP image against the float32 oracle at a flat
1e-4 (1e-3 on a depth channel) and leave out the pixels the oracle flags.  A float32 blend is 50 to 600 times closer to the
truth than that, on every pixel (tests/test_raster_fwd_ref_cpu.py prints the figures), so a wrong constant, a lost faint
record or a shifted pixel centre passes.  This file evaluates SURVEY A.5 per tile in float64 from the SAME float32 inputs
(vectorised; `oracle/blend_f64.walk` is the sequential, per-pixel cross-check) and returns, next to the truth G
(render_colors [C,H,W,D] with backgrounds and masked tiles as the operator has them, render_alphas, last_ids), a scale E
for every pixel and channel and for alpha that bounds, to first order, what ANY float32 evaluation of the same blend can
be off by.  The bar is, pixel by pixel and channel by channel,

    |x - G| <= 2^-24 K E,       x exactly G (the background, or 0) where E == 0,       last_ids exactly equal.

The scale (all in units of 2^-24, magnitudes summed with no cancellation; k runs over the records the pixel blends,
front to back, vis_k = alpha_k T_k, T_k the transmittance in front of k):

  ea_k    relative error of the raw alpha op exp(-sigma): sigma = (a dx^2 + c dy^2)/2 + b dx dy is a sum of terms of
          magnitude S_k = (|a| dx^2 + |c| dy^2)/2 + |b dx dy|, rounded k_round = 8 times (blend_f64's bound), so
          |d sigma| <= k_round S_k, which IS the relative error of exp(-sigma); + 4 for the product and exp; and for the
          kernels' pre-scaled form alpha = exp2(log2(op) - sigma2) (csrc/raster_common.h) one rounding of log2(op), a full
          ulp of v_log_f32, and one of the difference: |d log2 alpha| <= 2 |log2 op| + |log2 raw|, i.e. 2 |ln op| + |ln raw|
          relative to alpha.  A clearly clamped alpha is the constant 0.999f, 0.25 away from 0.999.
  terr_k  relative error of T_k: sum over the records j in front of k of alpha_j ea_j / (1 - alpha_j) + 2 (the error of
          the factor 1 - alpha_j, its rounding and the product's).
  colour  E_d = sum_k |c_kd| vis_k (ea_k + terr_k + 1)            the error of every term, + 1 for the product alpha T
                + sum_k P_kd,   P_kd = sum_{j <= k} |c_jd| vis_j    one rounding per accumulation step, bounded by the
                                                                    magnitude of the partial sum it rounds
                + |bg_d| T_final (terr_final + 1) + (|bg_d| T_final + P_last,d)      the background term and its addition
  alpha   E_a = T_final terr_final + 1/2: 1 - T is exact for T >= 1/2 and otherwise rounds a value below 1, half an ulp
          of which is at most 2^-25.
  A pixel that blends nothing has E = 0: 0 + 1 * bg is exact.
  Depth-normalising epilogue (channel D-1 divided by max(alpha, 1e-10)): q = c / a to first order,
  E_q = E_c / a + |c| E_a / a^2 + |q| (the divide's own rounding); `depth_normalised`.

K = 4 K_REF.  K_REF is the largest ratio |replay - G| / (2^-24 E) two float32 replays of the blend in numpy reach over
all pixels, channels and cases of oracle/raster_bwd_cases.py (no kernel involved): the literal order of
oracle/gsplat_oracle.py and the pinned order of csrc/raster_common.h (`replay_pinned`).  The factor 4 stands for the
hardware's 1-ulp exp2 / log2 where numpy rounds correctly and for true FMA.  tests/test_raster_fwd_ref_cpu.py measures
K_REF again and fails if the constant below is less than the largest replay or more than twice it.

No pixel is left out.  A pixel whose natural float64 path meets a NEAR decision in blend_f64's sense (`sigma < 0`,
`alpha < 1/255`, `T (1 - alpha) <= 1e-4` closer to the threshold than the bound of the tested quantity; the clamp at
0.999 is continuous) is flagged by the same windows, vectorised; for those `blend_f64.outcomes(log_form=True)` enumerates
the blend under every combination of the near decisions and the pixel passes iff colour, alpha and last_ids TOGETHER
are within the bar of ONE outcome, judged by that outcome's own scale.  Per case the pixels with more than one outcome
must stay under raster_bwd_cases.UNSTABLE_CAP and none may reach `max_outcomes`.

Measured on the 31 cases (tests/test_raster_fwd_ref_cpu.py prints every figure):
  replays  largest ratio 0.974 (clamp-D3, alpha, both orders: the half ulp of the stored alpha against E_a just above
           1/2); alpha 0.10 (deep_soft) .. 0.97, colours 0.09 (deep_soft) .. 0.79 (edge-finite-D4bg); the pinned and the
           literal order are within 0.05 of each other everywhere.  max |float32 - G| over a case is 1.4e-7 .. 2.8e-6: the
           flat 1e-4 is 35 to 700 times that.
  near     pixels judged against several outcomes: 0 in 26 cases, 0.007 % (two_cameras, half_tiles), 0.008 % (clamp),
           0.052 % (deep_hard: every list saturates); none truncated; no replay needed another outcome than the natural one.
  faults   on ragged-D3, share of the pixels past K: pixel centres off by 1e-4 px 11.4 % (largest change on the oracle's
           stable pixels 8.8e-5: the flat bar passes it), opacities x (1 - 2^-16) 77 %, sigma x (1 + 2^-16) 51 %, the
           faintest live record of every pixel dropped 100 %.
"""
from __future__ import annotations

import numpy as np

from oracle import blend_f64 as B
from oracle import raster_bwd_f64 as RB

ALPHA_MIN, ALPHA_MAX, T_EPS, EPS24 = B.ALPHA_MIN, B.ALPHA_MAX, B.T_EPS, B.EPS24
K_ROUND = 8.0
MAX_OUTCOMES = 64
K_REF = 0.98           # measured: 0.974, the largest ratio of the two float32 replays over all pixels of all cases (clamp-D3)
K = 4.0 * K_REF
FAULTS = ("centre", "opacity", "sigma", "drop_faintest")
_F = np.float32


def _as(a, dt, shape):
    return np.asarray(a).astype(dt).reshape(shape)


def _tile_blend(m2, cn, op, g, y0, y1, x0, x1, fault=None, drop=None):
    """The float64 blend of one tile, [G records, P pixels], with the error terms of the module text."""
    hh, ww = y1 - y0, x1 - x0
    P, G = hh * ww, g.shape[0]
    off = 1e-4 if fault == "centre" else 0.0
    px = np.broadcast_to((np.arange(x0, x1, dtype=np.float64) + 0.5 + off)[None, :], (hh, ww)).reshape(-1)
    py = np.broadcast_to((np.arange(y0, y1, dtype=np.float64) + 0.5 + off)[:, None], (hh, ww)).reshape(-1)
    dx = m2[g, 0][:, None] - px[None]
    dy = m2[g, 1][:, None] - py[None]
    t_a, t_c, t_b = 0.5 * cn[g, 0][:, None] * dx * dx, 0.5 * cn[g, 2][:, None] * dy * dy, cn[g, 1][:, None] * dx * dy
    sig = t_a + t_c + t_b
    S = np.abs(t_a) + np.abs(t_c) + np.abs(t_b)
    o = op[g][:, None]
    if fault == "sigma":
        sig = sig * (1.0 + 2.0 ** -16)
    if fault == "opacity":
        o = o * (1.0 - 2.0 ** -16)
    with np.errstate(all="ignore"):
        raw = o * np.exp(-sig)
        a = np.minimum(raw, ALPHA_MAX)
        ok = (sig >= 0) & (a >= ALPHA_MIN)
        if drop is not None:
            ok &= ~drop
        logt = np.where((o > 0) & (raw > 0), 2.0 * np.abs(np.log(np.where(o > 0, o, 1.0)))
                        + np.abs(np.log(np.where(raw > 0, raw, 1.0))), 0.0)
        lograt = np.where(raw > 0, np.abs(np.log(np.where(raw > 0, raw, 1.0) / ALPHA_MIN)), np.inf)
    ea = K_ROUND * S + 4.0 + logt
    ea_eff = np.where(raw > ALPHA_MAX * (1.0 + 2.0 * EPS24 * ea), 0.25, ea)
    ae = np.where(ok, a, 0.0)
    om = 1.0 - ae
    Ta = np.cumprod(om, axis=0)
    Tb = np.concatenate([np.ones((1, P)), Ta[:-1]], axis=0)
    term = ok & (Ta <= T_EPS)
    first = np.where(term.any(0), term.argmax(0), G)
    kk = np.arange(G)[:, None]
    live = ok & (kk < first[None])
    tterm = np.where(ok, ae * ea_eff / np.maximum(om, 1e-3) + 2.0, 0.0)
    terr_a = np.cumsum(tterm, axis=0)
    terr_b = terr_a - tterm
    ar = np.arange(P)
    fi = np.minimum(first, G - 1)
    sat = first < G
    Tfin = np.where(sat, Tb[fi, ar], Ta[-1])
    terr_fin = np.where(sat, terr_b[fi, ar], terr_a[-1])
    vis = np.where(live, ae * Tb, 0.0)
    # the windows of blend_f64.walk, on the records the natural path looks at (up to the one that terminates it)
    considered = kk <= first[None]
    es = K_ROUND * EPS24 * S
    slack = 1.0 + 1e-9           # (the vectorised flag must be a superset of the walk's: its sums round differently)
    near_v = ((es > 0) & (np.abs(sig) <= es * slack)) | (lograt <= (EPS24 * ea + 2e-7) * slack)
    near_t = ok & (np.abs(Ta / T_EPS - 1.0) <= (EPS24 * terr_a + 2e-7) * slack)
    near = ((near_v | near_t) & considered).any(0)
    return dict(vis=vis, live=live, Tfin=Tfin, terr_fin=terr_fin, terr_b=terr_b, ea_eff=ea_eff, near=near, sat=sat)


def rasterize_fwd(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                  backgrounds=None, masks=None, fault=None, enumerate_near=True, max_outcomes=MAX_OUTCOMES):
    """Inputs as rasterize_to_pixels ([C,N,*] float32, isect_offsets i32[C,th,tw], flatten_ids i32[I]).
    -> dict: colors f64[C,H,W,D], alphas f64[C,H,W], last_ids i32[C,H,W] (the truth G); E_colors, E_alphas (the scales, in
       units of 2^-24); near bool[C,H,W] (a near decision on the natural path); blended, saturated bool[C,H,W]; alts = one
       entry per near pixel with more than one outcome: (c, y, x, colors [n,D], alphas [n], last [n], E_colors [n,D],
       E_alphas [n]), the natural outcome first; truncated = pixels whose enumeration reached `max_outcomes`.
    fault (the reference's own sensitivity tests; tests/test_raster_fwd_ref_cpu.py): "centre" pixel centres off by 1e-4 px,
    "opacity" opacities times 1 - 2^-16, "sigma" sigma times 1 + 2^-16, "drop_faintest" the live record of smallest
    alpha T of every pixel is skipped."""
    opacities = np.asarray(opacities)
    C, N = opacities.shape
    D = np.asarray(colors).shape[-1]
    H, W = int(image_height), int(image_width)
    m2, cn = _as(means2d, np.float64, (-1, 2)), _as(conics, np.float64, (-1, 3))
    co, op = _as(colors, np.float64, (-1, D)), _as(opacities, np.float64, (-1,))
    bg = None if backgrounds is None else _as(backgrounds, np.float64, (C, D))
    offs = np.asarray(isect_offsets, dtype=np.int64)
    fids = np.asarray(flatten_ids, dtype=np.int64).reshape(-1)
    masks = None if masks is None else np.asarray(masks)
    out_c, E_c = np.zeros((C, H, W, D)), np.zeros((C, H, W, D))
    out_a, E_a = np.zeros((C, H, W)), np.zeros((C, H, W))
    out_l = np.zeros((C, H, W), np.int32)
    near, blended, saturated = (np.zeros((C, H, W), bool) for _ in range(3))
    alts, truncated = [], 0
    for c, y0, y1, x0, x1, s, e, masked in RB._tiles(C, H, W, tile_size, offs, fids.shape[0], masks):
        hh, ww = y1 - y0, x1 - x0
        sl = (c, slice(y0, y1), slice(x0, x1))
        g = fids[s:e]
        keep = (g >= 0) & (g < C * N)
        pos = (s + np.arange(g.shape[0]))[keep]
        g = g[keep]
        if masked or g.shape[0] == 0:
            if bg is not None:
                out_c[sl] = bg[c]
            continue
        b = _tile_blend(m2, cn, op, g, y0, y1, x0, x1, fault)
        if fault == "drop_faintest":
            vis, live = b["vis"], b["live"]
            kmin = np.where(live, vis, np.inf).argmin(0)
            drop = (np.arange(g.shape[0])[:, None] == kmin[None]) & live.any(0)[None]
            b = _tile_blend(m2, cn, op, g, y0, y1, x0, x1, None, drop)
        vis, live, Tfin, terr_fin = b["vis"], b["live"], b["Tfin"], b["terr_fin"]
        cg = co[g]
        acg = np.abs(cg)
        col = vis.T @ cg
        cnt = np.cumsum(live, axis=0)
        nlive = cnt[-1]
        some = nlive > 0
        steps_from = np.where(live, nlive[None] - cnt + 1, 0)
        pabs = vis.T @ acg
        E = (vis * (b["ea_eff"] + b["terr_b"] + 1.0 + steps_from)).T @ acg
        if bg is not None:
            col = col + Tfin[:, None] * bg[c][None]
            abg = np.abs(bg[c])[None]
            E = E + some[:, None] * (abg * Tfin[:, None] * (terr_fin[:, None] + 1.0) + abg * Tfin[:, None] + pabs)
        idx_last = np.where(live, np.arange(g.shape[0])[:, None], -1).max(0)
        out_c[sl], E_c[sl] = col.reshape(hh, ww, D), E.reshape(hh, ww, D)
        out_a[sl] = (1.0 - Tfin).reshape(hh, ww)
        E_a[sl] = np.where(some, Tfin * terr_fin + 0.5, 0.0).reshape(hh, ww)
        out_l[sl] = np.where(some, pos[np.maximum(idx_last, 0)], 0).reshape(hh, ww)
        near[sl], blended[sl], saturated[sl] = b["near"].reshape(hh, ww), some.reshape(hh, ww), b["sat"].reshape(hh, ww)
        if enumerate_near and fault is None:
            for p in np.nonzero(b["near"])[0]:
                y, x = y0 + int(p) // ww, x0 + int(p) % ww
                outs = B.outcomes(x + 0.5, y + 0.5, g, m2, cn, co, op, None if bg is None else bg[c], K_ROUND, max_outcomes,
                                  log_form=True)
                truncated += len(outs) >= max_outcomes
                if len(outs) > 1:
                    alts.append((c, y, x, np.stack([o.color for o in outs]), np.array([o.alpha for o in outs]),
                                 np.array([pos[o.last] if o.last >= 0 else 0 for o in outs], np.int32),
                                 np.stack([o.scale for o in outs]), np.array([o.alpha_scale for o in outs])))
    return dict(colors=out_c, alphas=out_a, last_ids=out_l, E_colors=E_c, E_alphas=E_a, near=near, blended=blended,
                saturated=saturated, alts=alts, truncated=int(truncated))


def depth_normalised(colors, alphas, E_colors, E_alphas):
    """The truth and the scale behind the depth-normalising epilogue: the last channel becomes c / max(alpha, 1e-10), its
    scale E_c / a + |c| E_a / a^2 + |q|.  Where nothing blends (E == 0) the expected value is the float32 quotient the kernel
    forms, bit for bit: float32(c) / 1e-10f."""
    colors, E_colors = np.array(colors, np.float64), np.array(E_colors, np.float64)
    alphas, E_alphas = np.asarray(alphas, np.float64), np.asarray(E_alphas, np.float64)
    c = colors[..., -1]
    a = np.maximum(alphas, 1e-10)
    q = c / a
    blend = E_alphas > 0
    with np.errstate(all="ignore"):
        exact = (c.astype(np.float32) / np.maximum(alphas.astype(np.float32), _F(1e-10))).astype(np.float64)
    colors[..., -1] = np.where(blend, q, exact)
    E_colors[..., -1] = np.where(blend, E_colors[..., -1] / a + np.abs(c) * E_alphas / (a * a) + np.abs(q), 0.0)
    return colors, E_colors


def _ratios(x_c, x_a, G_c, G_a, E_c, E_a):
    """-> (colour ratio, alpha ratio), the channel maximum of |x - G| / (2^-24 E); inf where E == 0 and x != G, or x is
    not finite."""
    def one(x, G, E):
        err = np.abs(x - G)
        with np.errstate(all="ignore"):
            r = np.where(E > 0, err / (EPS24 * np.where(E > 0, E, 1.0)), np.where(err == 0, 0.0, np.inf))
        return np.where(np.isfinite(x), r, np.inf)
    return one(x_c, G_c, E_c).max(-1), one(x_a, G_a, E_a)


def judge(ref, colors, alphas, last_ids=None, depth_normalise=False):
    """Every pixel of a float32 image against the reference `ref` (rasterize_fwd's dict).
    -> dict: colors, alphas = the largest ratio of each output; ratio f64[C,H,W] = the pixel's ratio (the larger of the two;
       inf: not exact where E == 0, not finite, or last_ids differ); alt = pixels that pass by an outcome other than the
       natural one.  A near pixel with several outcomes gets the smallest ratio over them, each outcome judged WHOLE (colour,
       alpha and last_ids) by its own scale.  The bar is `ratio.max() <= K`."""
    G_c, G_a, E_c, E_a = ref["colors"], ref["alphas"], ref["E_colors"], ref["E_alphas"]
    x_c = np.asarray(colors, np.float64).reshape(G_c.shape)
    x_a = np.asarray(alphas, np.float64).reshape(G_a.shape)
    x_l = None if last_ids is None else np.asarray(last_ids).reshape(G_a.shape)
    if depth_normalise:
        G_c, E_c = depth_normalised(G_c, G_a, E_c, E_a)
    r_c, r_a = _ratios(x_c, x_a, G_c, G_a, E_c, E_a)
    if x_l is not None:
        r_c = np.where(x_l == ref["last_ids"], r_c, np.inf)
    n_alt = 0
    for (c, y, x, oc, oa, ol, oEc, oEa) in ref["alts"]:
        if depth_normalise:
            oc, oEc = depth_normalised(oc, oa, oEc, oEa)
        rc, ra = _ratios(x_c[c, y, x][None], x_a[c, y, x][None], oc, oa, oEc, oEa)
        if x_l is not None:
            rc = np.where(ol == x_l[c, y, x], rc, np.inf)
        best = int(np.argmin(np.maximum(rc, ra)))
        n_alt += best != 0
        r_c[c, y, x], r_a[c, y, x] = rc[best], ra[best]
    return dict(colors=float(r_c.max()), alphas=float(r_a.max()), ratio=np.maximum(r_c, r_a), alt=n_alt)


# ---- the cases: those of oracle/raster_bwd_cases.py ----------------------------------------------------------------------------
def case_ids():
    """The backward module's cases but `one_hot-D4`, which differs from `ragged-D4` in its upstream gradient only."""
    from oracle import raster_bwd_cases as RC
    return [c for c in RC.CASE_IDS if c != "one_hot-D4"]


def case_args(p):
    """(positional, keyword) arguments of rasterize_fwd / replay_pinned / gsplat_oracle.rasterize_to_pixels for a case dict."""
    return ((p["means2d"], p["conics"], p["colors"], p["opacities"], p["width"], p["height"], p["tile_size"],
             p["isect_offsets"], p["flatten_ids"]), dict(backgrounds=p["backgrounds"], masks=p["masks"]))


def reference(p, **kw):
    a, k = case_args(p)
    return rasterize_fwd(*a, **k, **kw)


_CASE_REFS = {}


def case_reference(case_id, p=None):
    """(inputs, reference) of a case of oracle/raster_bwd_cases.py: computed once per process and shared by the test
    modules that judge a forward on it; nobody writes to either.  `p`: the case's inputs where the caller has made them
    already (make_case runs the float32 oracle for its own purposes: seconds at 32 channels)."""
    if case_id not in _CASE_REFS:
        if p is None:
            from oracle import raster_bwd_cases as RC
            p = RC.make_case(case_id)
        assert p["case"] == case_id
        _CASE_REFS[case_id] = (p, reference(p))
    return _CASE_REFS[case_id]


def replays(p):
    """{"literal": ..., "pinned": ...}: (colors, alphas, last_ids) of the two float32 replays K_REF is measured on."""
    from oracle import gsplat_oracle as O
    a, k = case_args(p)
    return {"literal": O.rasterize_to_pixels(*a, **k), "pinned": replay_pinned(*a, **k)}


def near_share(ref):
    """Share of a case's pixels that are judged against more than one outcome (the cap is on this)."""
    return len(ref["alts"]) / ref["near"].size


# ---- the float32 replay in the kernels' pinned order (csrc/raster_common.h), per tile --------------------------------------
def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def replay_pinned(means2d, conics, colors, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                  backgrounds=None, masks=None):
    """blend_f64.blend_pixel_pinned_fp32 for all pixels of a tile at once: pre-scaled conic, sigma2 by two FMAs,
    alpha = min(0.999f, exp2(log2(op) - sigma2)), T' = fma(-alpha, T, T), colour += c (alpha T) by FMA; FMA emulated through
    float64, exp2 / log2 numpy's.  -> render_colors f32[C,H,W,D], render_alphas f32[C,H,W], last_ids i32[C,H,W]."""
    opacities = np.asarray(opacities)
    C, N = opacities.shape
    D = np.asarray(colors).shape[-1]
    H, W = int(image_height), int(image_width)
    m2, cn = _as(means2d, _F, (-1, 2)), _as(conics, _F, (-1, 3))
    co, op = _as(colors, _F, (-1, D)), _as(opacities, _F, (-1,))
    bg = None if backgrounds is None else _as(backgrounds, _F, (C, D))
    offs = np.asarray(isect_offsets, dtype=np.int64)
    fids = np.asarray(flatten_ids, dtype=np.int64).reshape(-1)
    masks = None if masks is None else np.asarray(masks)
    out_c = np.zeros((C, H, W, D), _F)
    out_a = np.zeros((C, H, W), _F)
    out_l = np.zeros((C, H, W), np.int32)
    with np.errstate(all="ignore"):
        A2 = cn[:, 0] * _F(0.7213475204444817)
        B2 = cn[:, 1] * _F(1.4426950408889634)
        C2 = cn[:, 2] * _F(0.7213475204444817)
        lop = np.where(op < 0, _F(-np.inf), np.log2(np.where(op < 0, _F(1), op))).astype(_F)
    for c, y0, y1, x0, x1, s, e, masked in RB._tiles(C, H, W, tile_size, offs, fids.shape[0], masks):
        hh, ww = y1 - y0, x1 - x0
        P = hh * ww
        sl = (c, slice(y0, y1), slice(x0, x1))
        g = fids[s:e]
        keep = (g >= 0) & (g < C * N)
        pos = (s + np.arange(g.shape[0]))[keep]
        g = g[keep]
        if masked or g.shape[0] == 0:
            if bg is not None:
                out_c[sl] = bg[c]
            continue
        px = np.broadcast_to((np.arange(x0, x1, dtype=_F) + _F(0.5))[None, :], (hh, ww)).reshape(-1)
        py = np.broadcast_to((np.arange(y0, y1, dtype=_F) + _F(0.5))[:, None], (hh, ww)).reshape(-1)
        with np.errstate(all="ignore"):
            dx = m2[g, 0][:, None] - px[None]
            dy = m2[g, 1][:, None] - py[None]
            bdy = B2[g][:, None] * dy
            q = (C2[g][:, None] * dy) * dy
            sg = _fma32(_fma32(A2[g][:, None], dx, bdy), dx, q)
            al = np.minimum(_F(0.999), np.exp2(lop[g][:, None] - sg).astype(_F))
        valid = ~(sg < 0) & (al >= _F(1.0 / 255.0))
        T = np.ones(P, _F)
        acc = np.zeros((P, D), _F)
        last = np.zeros(P, np.int32)
        done = np.zeros(P, bool)
        for k in np.nonzero(valid.any(1))[0]:
            v = valid[k] & ~done
            if not v.any():
                if done.all():
                    break
                continue
            nT = _fma32(-al[k], T, T)
            t = v & (nT <= _F(1e-4))
            b = v & ~t
            vis = np.where(b, al[k] * T, _F(0))
            acc = _fma32(co[g[k]][None, :], vis[:, None], acc)
            T = np.where(b, nT, T)
            last = np.where(b, pos[k], last).astype(np.int32)
            done |= t
        if bg is not None:
            acc = acc + T[:, None] * bg[c][None]
        out_c[sl], out_a[sl], out_l[sl] = acc.reshape(hh, ww, D), (_F(1) - T).reshape(hh, ww), last.reshape(hh, ww)
    return out_c, out_a, out_l
