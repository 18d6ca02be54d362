"""Closed-form float64 backward of spherical_harmonics with per-row error scales -- TEST INFRASTRUCTURE ONLY.

The 25 real SH basis functions of degrees 0..4 (the constants and recurrences of `oracle/gsplat_torch.py::sh_basis`)
are expanded ONCE into a table of monomials (coefficient, ex, ey, ez) of the unit direction u = d / |d| by a few
lines of polynomial arithmetic.  From the table, without autograd:

  Y_k(u)          = sum_m c_m x^ex y^ey z^ez                       dY_k/du_j = sum_m c_m e_j u^(e - 1_j)
  v_coeffs[k, ch] = Y_k v_colors[ch]                                (0 for k beyond the degree, 0 on masked-off rows)
  v_u[j]          = sum_k dY_k/du_j  sum_ch coeffs[k, ch] v_colors[ch]
  v_dirs          = (I - u u^T) v_u / |d|                           (the normalisation; 0 at degree 0)

and, next to every entry G, the scale S a float32 evaluation of the same sums is judged by (the project's sense, see
oracle/raster_bwd_f64.py): the same sums with |c_m|, |u|, |v_colors|, |coeffs| -- no cancellation allowed -- and the
projector (I - u u^T) / |d| taken as (I + |u| |u|^T) / |d|.  The bar is  |x - G| <= 2^-24 K S,  exactly 0 where S == 0
(masked-off rows, bases beyond the degree, v_dirs at degree 0).  A masked-off row is never evaluated (gsplat does not
either), so its direction may be anything, the zero vector included.
"""
from __future__ import annotations

import numpy as np

EPS24 = 2.0 ** -24


def _mul(a, b):
    out = {}
    for ea, ca in a.items():
        for eb, cb in b.items():
            e = (ea[0] + eb[0], ea[1] + eb[1], ea[2] + eb[2])
            out[e] = out.get(e, 0.0) + ca * cb
    return out


def _add(a, b, sb=1.0):
    out = dict(a)
    for e, c in b.items():
        out[e] = out.get(e, 0.0) + sb * c
    return out


def _scl(a, s):
    return {e: s * c for e, c in a.items()}


def _table():
    x, y, z = {(1, 0, 0): 1.0}, {(0, 1, 0): 1.0}, {(0, 0, 1): 1.0}
    one = {(0, 0, 0): 1.0}
    Y = [_scl(one, 0.2820947917738781)]
    c1 = 0.48860251190292
    Y += [_scl(y, -c1), _scl(z, c1), _scl(x, -c1)]
    z2 = _mul(z, z)
    fTmp0B = _scl(z, -1.092548430592079)
    fC1 = _add(_mul(x, x), _mul(y, y), -1.0)
    fS1 = _scl(_mul(x, y), 2.0)
    pSH6 = _add(_scl(z2, 0.9461746957575601), one, -0.3153915652525201)
    Y += [_scl(fS1, 0.5462742152960395), _mul(fTmp0B, y), pSH6, _mul(fTmp0B, x), _scl(fC1, 0.5462742152960395)]
    fTmp0C = _add(_scl(z2, -2.285228997322329), one, 0.4570457994644658)
    fTmp1B = _scl(z, 1.445305721320277)
    fC2 = _add(_mul(x, fC1), _mul(y, fS1), -1.0)
    fS2 = _add(_mul(x, fS1), _mul(y, fC1))
    pSH12 = _mul(z, _add(_scl(z2, 1.865881662950577), one, -1.119528997770346))
    Y += [_scl(fS2, -0.5900435899266435), _mul(fTmp1B, fS1), _mul(fTmp0C, y), pSH12, _mul(fTmp0C, x),
          _mul(fTmp1B, fC1), _scl(fC2, -0.5900435899266435)]
    fTmp0D = _mul(z, _add(_scl(z2, -4.683325804901025), one, 2.007139630671868))
    fTmp1C = _add(_scl(z2, 3.31161143515146), one, -0.47308734787878)
    fTmp2B = _scl(z, -1.770130769779931)
    fC3 = _add(_mul(x, fC2), _mul(y, fS2), -1.0)
    fS3 = _add(_mul(x, fS2), _mul(y, fC2))
    pSH20 = _add(_scl(_mul(z, pSH12), 1.984313483298443), pSH6, -1.006230589874905)
    Y += [_scl(fS3, 0.6258357354491763), _mul(fTmp2B, fS2), _mul(fTmp1C, fS1), _mul(fTmp0D, y), pSH20,
          _mul(fTmp0D, x), _mul(fTmp1C, fC1), _mul(fTmp2B, fC2), _scl(fC3, 0.6258357354491763)]
    return tuple(tuple((c, e[0], e[1], e[2]) for e, c in sorted(p.items()) if c != 0.0) for p in Y)


TABLE = _table()        # TABLE[k] = ((coefficient, ex, ey, ez), ...): Y_k(u) = sum coefficient x^ex y^ey z^ez


def basis(degree, u, absolute=False):
    """u [M,3] (unit vectors, float64) -> (Y [M,K], dY [M,K,3]) from the monomial table, K = (degree + 1)^2.
    absolute: every coefficient and every component of u by its magnitude (the scales: aY >= |Y|, adY >= |dY|)."""
    u = np.asarray(u, np.float64)
    if absolute:
        u = np.abs(u)
    M, K = u.shape[0], (degree + 1) ** 2
    pw = [[np.ones(M)] for _ in range(3)]
    for j in range(3):
        for _ in range(4):
            pw[j].append(pw[j][-1] * u[:, j])
    Y, dY = np.zeros((M, K)), np.zeros((M, K, 3))
    for k in range(K):
        for c, ex, ey, ez in TABLE[k]:
            c = abs(c) if absolute else c
            e = (ex, ey, ez)
            Y[:, k] += c * pw[0][ex] * pw[1][ey] * pw[2][ez]
            for j in range(3):
                if e[j]:
                    f = [pw[i][e[i] - (i == j)] for i in range(3)]
                    dY[:, k, j] += c * e[j] * f[0] * f[1] * f[2]
    return Y, dY


def sh_bwd(degree, dirs, coeffs, v_colors, masks=None):
    """dirs [...,3], coeffs [...,Kt,3] (Kt >= (degree+1)^2), v_colors [...,3], masks bool[...] | None
    -> {"G": {"coeffs", "dirs"}, "S": {...}, "A": {...}} (float64, shaped like the inputs; A is zero: the SH backward
    rebuilds nothing from a stored float32)."""
    dirs = np.asarray(dirs, np.float64)
    coeffs = np.asarray(coeffs, np.float64)
    lead, Kt = dirs.shape[:-1], coeffs.shape[-2]
    K = (degree + 1) ** 2
    d, c, v = dirs.reshape(-1, 3), coeffs.reshape(-1, Kt, 3), np.asarray(v_colors, np.float64).reshape(-1, 3)
    live = np.ones(d.shape[0], bool) if masks is None else np.asarray(masks, bool).reshape(-1)
    Gc, Sc = np.zeros_like(c), np.zeros_like(c)
    Gd, Sd = np.zeros_like(d), np.zeros_like(d)
    if live.any():
        dl, cl, vl = d[live], c[live][:, :K], v[live]
        n = np.sqrt((dl * dl).sum(-1, keepdims=True))
        assert (n > 0).all(), "a live row needs a direction"
        u = dl / n
        au = np.abs(u)
        Y, dY = basis(degree, u)
        aY, adY = basis(degree, u, absolute=True)
        g = np.zeros((dl.shape[0], Kt, 3))
        s = np.zeros((dl.shape[0], Kt, 3))
        g[:, :K] = Y[:, :, None] * vl[:, None, :]
        s[:, :K] = aY[:, :, None] * np.abs(vl)[:, None, :]
        Gc[live], Sc[live] = g, s
        t = (cl * vl[:, None, :]).sum(-1)
        ta = (np.abs(cl) * np.abs(vl)[:, None, :]).sum(-1)
        vu = (dY * t[:, :, None]).sum(1)
        su = (adY * ta[:, :, None]).sum(1)
        Gd[live] = (vu - u * (u * vu).sum(-1, keepdims=True)) / n
        Sd[live] = (su + au * (au * su).sum(-1, keepdims=True)) / n
    shp = {"coeffs": lead + (Kt, 3), "dirs": lead + (3,)}
    G = {"coeffs": Gc.reshape(shp["coeffs"]), "dirs": Gd.reshape(shp["dirs"])}
    S = {"coeffs": Sc.reshape(shp["coeffs"]), "dirs": Sd.reshape(shp["dirs"])}
    return {"G": G, "S": S, "A": {k: np.zeros(s_) for k, s_ in shp.items()}}


# ---------------------------------------------------------------------------------------------
# the inputs of the per-row SH-backward tests (shared by the CPU module, which judges the replay, and the GPU module)
# ---------------------------------------------------------------------------------------------
# rows every input of 16 rows or more starts with: the poles, the axes, the coordinate planes (one component exactly 0).
# (M = 1 has no room for them; 255, 257, 2000 and [2, 1000] all carry them, under every mask kind but "all_false".)
SPECIAL_DIRS = ((0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0), (0.6, 0.8, 0), (0, -0.28, 0.96), (0.8, 0, -0.6), (1e-3, 0, 1), (0, 1, 1e-3))
# The row lengths of tests/test_gpu_parity.py::test_sh_backward_vs_autograd (odd lengths: the scalar-row kernel; n x 16 B:
# the float4-row kernel) crossed with the degrees 0-4, as far as a row can hold the degree's (degree + 1)^2 bases: 26 pairs.
K_TOTALS = (3, 6, 11, 18, 27, 4, 16, 28)
DEG_K_TOTAL = tuple((deg, kt) for deg in range(5) for kt in K_TOTALS if kt >= (deg + 1) ** 2)
SHAPES = ((1,), (255,), (257,), (2000,), (2, 1000))
MASK_KINDS = ("none", "all_false", "random")


def make_inputs(degree, k_total, shape, mask_kind, seed=0):
    """float32 dirs [*shape,3] with |d| log-uniform over 1e-3..1e3, coeffs [*shape,k_total,3], v_colors [*shape,3] and
    masks bool[*shape] | None.  Masked-off rows include rows whose direction is the ZERO vector."""
    assert mask_kind in MASK_KINDS and k_total >= (degree + 1) ** 2
    rng = np.random.default_rng(1000 * seed + 31 * degree + k_total + 7 * int(np.prod(shape)))
    M = int(np.prod(shape))
    d = rng.normal(size=(M, 3))
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    if M >= 16:
        d[:len(SPECIAL_DIRS)] = SPECIAL_DIRS
    d *= np.exp(rng.uniform(np.log(1e-3), np.log(1e3), size=(M, 1)))
    masks = {"none": None, "all_false": np.zeros(M, bool), "random": rng.random(M) > 0.2}[mask_kind]
    if masks is not None:
        if M >= 16 and mask_kind == "random":              # the special rows stay live; "all_false" keeps every row off
            masks[:len(SPECIAL_DIRS)] = True
            masks[len(SPECIAL_DIRS) + 2] = False
        d[~masks & (np.arange(M) % 3 != 0)] = 0.0          # two in three of the masked-off rows have no direction at all
    return dict(degree=degree, dirs=d.astype(np.float32).reshape(shape + (3,)),
                coeffs=rng.normal(size=shape + (k_total, 3)).astype(np.float32),
                v_colors=rng.normal(size=shape + (3,)).astype(np.float32),
                masks=None if masks is None else masks.reshape(shape))


def reference(p):
    return sh_bwd(p["degree"], p["dirs"], p["coeffs"], p["v_colors"], p["masks"])


def replay(p):
    """The torch oracle's float32 autograd on the same inputs (no kernel): the noise floor K_sh is taken from.  The
    oracle multiplies by the mask, which needs a finite colour to multiply, so masked-off rows are handed a unit direction
    (their gradients are zero either way)."""
    import torch
    from oracle import gsplat_torch as OT
    d = p["dirs"].copy()
    if p["masks"] is not None:
        d[~p["masks"]] = (0.0, 0.0, 1.0)
    dt = torch.from_numpy(d).requires_grad_(True)
    ct = torch.from_numpy(p["coeffs"]).requires_grad_(True)
    m = None if p["masks"] is None else torch.from_numpy(p["masks"])
    (OT.spherical_harmonics(p["degree"], dt, ct, masks=m) * torch.from_numpy(p["v_colors"])).sum().backward()
    return {"coeffs": ct.grad.numpy().astype(np.float64),
            "dirs": np.zeros(d.shape) if dt.grad is None else dt.grad.numpy().astype(np.float64)}


def all_inputs():
    """Every input of the GPU module: each (degree, k_total) at [2000] with random masks, and each shape x mask kind at
    degree 3 / 16 bases (float4 rows) and degree 4 / 27 bases (scalar rows)."""
    out = {}
    for deg, kt in DEG_K_TOTAL:
        out[(deg, kt, (2000,), "random")] = make_inputs(deg, kt, (2000,), "random")
    for deg, kt in ((3, 16), (4, 27)):
        for shape in SHAPES:
            for mk in MASK_KINDS:
                out.setdefault((deg, kt, shape, mk), make_inputs(deg, kt, shape, mk))
    return out


# The replay is float32, not exact: below 1 would mean S overstates.  A degree-4 basis function is a handful of monomials of
# four factors after the normalisation, a dozen-odd roundings against a scale that allows no cancellation; the replay reaches
# 8.5, and twice that would mean the closed form and the oracle no longer evaluate the same sums.
K_REF_BAND = (1.0, 17.0)


def k_ref(inputs=None, verbose=False):
    """The largest per-row ratio |replay - G| / (2^-24 S) over `inputs` (default: all_inputs()); asserts the replay is
    exactly 0 wherever S == 0."""
    from oracle import raster_bwd_f64 as RB
    worst = 0.0
    for key, p in (inputs or all_inputs()).items():
        ref, rep = reference(p), replay(p)
        for name in ("coeffs", "dirs"):
            r, off = RB.row_ratio(rep[name], ref, name)
            assert off == 0.0, (key, name, off)
            if verbose:
                print(f"[sh replay] {key} {name}: {float(r.max()) if r.size else 0.0:.2f}")
            worst = max(worst, float(r.max()) if r.size else 0.0)
    return worst
