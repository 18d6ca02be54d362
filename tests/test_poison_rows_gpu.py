"""Non-finite and overflowing Gaussians stay row-local: the recipes of oracle/poison_cases.py through the kernels.

culled class   a grafted row the oracle culls is indistinguishable from the twin scene's benign culled row: every forward
               output bit-identical, its own gradients exactly +0 (bytes), every other row judged against reference(twin).
visible class  projection and intersection bit-exact with the numpy oracle, pixels inside the float64 per-pixel bar of
               oracle/raster_fwd_f64.py; its own gradient may be non-finite, no other row's.

THE TRACE, made by reading before the first run.  Every integer used as an index, count or loop bound, and where it comes
from.  "row" = one recipe row; n, cam, tile, list positions are launch indices or integers read from integer tensors.

kernel / code                          integer                         comes from                                     safe because
project_one (projection_common.h)      rad_i                           (int)fminf(radius, 2147483520.f)               clamped before the cast, so NaN (fminf gives the clamp) and +inf cannot reach
                                                                                                                      it unclamped; the cast runs inside `if (z passes the planes)`, and a row
                                                                                                                      that is not valid at the end (det1 > 0 and radius > clip are false for
                                                                                                                      NaN) gets rad_i = 0 and all-zero outputs; a row outside the planes keeps
                                                                                                                      the initial rad_i = 0 and never reaches the cast
                                       n, cam                          blockIdx / threadIdx                           n < N checked
  culled recipes: z NaN passes !(z < near || z > far) on purpose and falls at det1 > 0 (every NaN mean / scale / quat makes
  det1 NaN: 0 * inf and inf - inf included); +-inf z, 3e38 x, near_below, far_above fall at the planes or at m2x -+ radius.
  visible recipes: bb * bb = inf -> radius = inf -> 2147483520; det1 = inf -> bb * bb - det1 = NaN -> fmaxf gives the floor ->
  radius = ceil(3 sqrt(bb)) = 1.3e10 -> 2147483520; conic c1 / inf = 0; det0 / det1 = NaN or 0 -> compensation 0.
proj_bwd_* / projection_bwd_kernel     n, cam, o = cam * N + n         launch index, loop over C                      no float becomes an index; rows with radii <= 0 are skipped BEFORE any
                                                                                                                      upstream value is read.  FOUND BY READING: proj_bwd_finish ran for rows
                                                                                                                      seen in no camera and formed 0 * M with M NaN / inf -> NaN in v_quats /
                                                                                                                      v_scales of a culled row.  Fixed (`seen`, as fused_bwd.hip already had).
tile_rect (isect.hip:16,              x0, x1, y0, y1                  (int)fmaxf(fminf(floor / ceil(..), tiles), 0)  clamp-then-cast: NaN -> fminf gives `tiles`, +-inf and 1.3e8 tiles clamp;
  isect_bin.hip:62-72, the same code)                                                                                 radius <= 0 returns the empty rectangle first; x0 <= x1, y0 <= y1
  isect_count / emit (isect.hip:47,97) cnt, pre_s, local / w           (y1 - y0) * (x1 - x0) of the above             0 <= cnt <= tiles; w > 0 where a slot exists
  bin_count (isect_bin.hip:199)        d[y * w + x], ch[...]           the same rectangle, `cnt <= 0 -> continue`     inside the (tiles + 1)^2 grid
  bin_scatter (isect_bin.hip:578)      cb[k], pay                      the same rectangle, tiles_per_gauss > 0        16-bit fields hold [0, tiles]
  depth bins (isect_bin.hip:~926)      c = (int)((K - lo) * s1)        integer keys (depth BITS of listed rows)       K in [lo, hi] -> p < NC, clamped to NC - 1; listed rows have finite
                                                                                                                      positive depths (near <= z <= far), culled rows are never listed
raster_walk.h cull and walk            g, idx, range_start / end       flatten_ids via sc_safe_id, isect_offsets      integers from integer tensors, clamped; splat_misses_rect never drops a
                                                                       via sc_tile_range                              conic that is not positive definite (conic 0: kept), A2 == 0 is guarded
record pack / unpack (fused_fwd.hip)   o                               launch index                                   floats are copied, never indexed with
sh.hip, fused_fwd.hip (SH part)        i                               launch index                                   a masked / culled row is written 0 without reading dirs or coeffs
fused_bwd.hip                          n, cam, o                       launch index                                   culled (cam, row): skipped before any upstream read; `seen` guards finish
raster_bwd.hip                         g, pixel and list positions     flatten_ids, isect_offsets, last_ids           as the forward walk; a culled row is in no list, so no atomic names it
rendering.py glue                      --                              opac * comps, dirs = means - centre            backward: 0 * NaN = NaN reaches sc_projection_bwd as v_compensation of a
                                                                                                                      culled row and is never read there; v_dirs of a masked row is written 0

An output the reference never reads: meta["opacities"] of a culled row is opacity * compensation = NaN * 0 = NaN where the
recipe holds a NaN opacity (the torch product and the fused kernel agree; no list names the row).  Compared everywhere else.
"""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_param_grad_rows_gpu as TP                      # noqa: E402  (routes, the caller's sequences, K)
from guard_arena import GuardedAlloc, guarded_adapter      # noqa: E402
from oracle import gsplat_oracle as O                      # noqa: E402  (checker only)
from oracle import param_grad_f64 as PG                    # noqa: E402
from oracle import poison_cases as PC                      # noqa: E402
from oracle import raster_bwd_cases as RC                  # noqa: E402
from oracle import raster_fwd_f64 as RF                    # noqa: E402
from street_crafter_amd.scenes import make_camera          # noqa: E402

DEV = "cuda"
W, H, TS, TW, TH = 160, 96, 16, 10, 6
_t, _np = TP._t, TP._np


@pytest.fixture(scope="module")
def ops():
    from street_crafter_amd import _lib
    _lib.load()
    import gsplat.rendering as R
    return R


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what=""):
    a, b = _np(a) if isinstance(a, torch.Tensor) else a, _np(b) if isinstance(b, torch.Tensor) else b
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(_u32(a), _u32(b), err_msg=what)


def _zero_bytes(t):
    return not bool(t.contiguous().view(torch.uint8).any())


@contextlib.contextmanager
def _setting(setter, value):
    prev = setter(value)
    try:
        yield
    finally:
        setter(prev)


@contextlib.contextmanager
def _option(key, value):
    from street_crafter_amd import _lib
    prev = _lib.set_option(key, value)
    try:
        yield
    finally:
        _lib.set_option(key, prev)


@functools.lru_cache(maxsize=None)
def _grafted(case_id, cls):
    """(recipes, slots, poisoned, twin) -- shared, nobody writes to them."""
    case = PG.make_case(case_id)
    cams = case["cameras"]
    cat = PC.catalogue(cams[0])
    pick = PC.gradient_judged(cat) if cls == "judged" else [r for r in cat if r.cls == cls and (len(cams) == 1 or not r.home)]
    slots = PC.slots_for(case["means"].shape[0], len(pick))
    p, t = PC.graft(case, pick, slots)
    return pick, slots, p, t


@functools.lru_cache(maxsize=None)
def _twin_reference(case_id):
    return PG.reference(_grafted(case_id, "culled")[3])


# =============================================================================================
# projection
# =============================================================================================
def _proj_cams():
    return dict(plain=PG.make_case("plain")["cameras"][0], yawed=PG.make_case("two_cameras")["cameras"][1],
                identity=make_camera(W, H, 180.0, 180.0))


@pytest.mark.parametrize("fast", [True, False], ids=["compiled", "ctypes"])
def test_projection_bit_exact_on_every_recipe(ops, fast):
    """All recipes x three cameras x with / without compensations x the four proj_clamp / radius_floor pairs, uint32 views.
    Subnormal conics, overflowing intermediates, 0 * inf under the exact-identity camera."""
    from street_crafter_amd import _lib
    cams = _proj_cams()
    cat = PC.catalogue(cams["plain"]) + PC.planes(cams["identity"], "@identity")
    L = PC.rows(cat * 6, 1)                                  # 294 rows: more than one block
    means, quats, scales = (_t(L[k]) for k in ("means", "quats", "scales"))
    V = torch.stack([c.viewmat for c in cams.values()]).to(DEV)
    K = torch.stack([c.K for c in cams.values()]).to(DEV)
    cam0 = cams["plain"]
    # one pair of planes for the whole call: the @identity plane rows sit at the identity camera's own planes only then
    assert all((c.znear, c.zfar) == (cam0.znear, cam0.zfar) for c in cams.values())
    n_sub = 0
    prev = _lib.set_projection_variant()
    try:
        for clamp in O.PROJ_CLAMPS:
            for floor in O.RADIUS_FLOORS:
                _lib.set_projection_variant(clamp, floor)
                exp = [O.fully_fused_projection(L["means"], L["quats"], L["scales"], c.viewmat.numpy(), c.K.numpy(), W, H,
                                                near_plane=cam0.znear, far_plane=cam0.zfar, proj_clamp=clamp, radius_floor=floor)
                       for c in cams.values()]
                for comp in (True, False):
                    with TP._routes(fast=fast, native=fast), torch.no_grad():
                        got = ops.fully_fused_projection(means, None, quats, scales, V, K, W, H, packed=False,
                                                         near_plane=cam0.znear, far_plane=cam0.zfar, calc_compensations=comp)
                    torch.cuda.synchronize()
                    assert (got[4] is None) == (not comp)
                    for i, what in enumerate(("radii", "means2d", "depths", "conics", "compensations")):
                        if got[i] is not None:
                            _same(got[i], np.stack([e[i] for e in exp]), f"{clamp} {floor} comp={comp} {what}")
                con = np.stack([e[3] for e in exp])
                n_sub += int(((con != 0) & (np.abs(con) < 2.0 ** -126)).sum())
    finally:
        _lib.set_projection_variant(*prev)
    assert n_sub > 0                                         # subnormal conics were among what was compared


# =============================================================================================
# tile intersection
# =============================================================================================
def _isect(ops, m2, radii, depths, C):
    tpg, ids, fids = ops.isect_tiles(_t(m2), torch.from_numpy(radii).to(DEV), _t(depths), TS, TW, TH, packed=False, n_cameras=C)
    offs = ops.isect_offset_encode(ids, C, TW, TH)
    torch.cuda.synchronize()
    fids = fids.plain() if hasattr(fids, "plain") else fids
    return _np(tpg), _np(ids), _np(fids), _np(offs)


def _isect_oracle(m2, radii, depths, C):
    tpg, ids, fids = O.isect_tiles(m2, radii, depths, TS, TW, TH, n_cameras=C)
    return tpg, ids, fids, O.isect_offset_encode(ids, C, TW, TH)


def _two_clamped_only():
    """A frame whose only visible rows are two clamped-radius splats at the SAME depth (10.0: the tie goes to the index),
    among culled recipes."""
    cam = PG.make_case("plain")["cameras"][0]
    cat = PC.catalogue(cam)
    rows = [r for r in cat if r.cls == "culled"]
    a, b = PC.by_name(cat, "iso_det1_p8", "iso_bb2_m8")
    rows = rows[:5] + [a] + rows[5:] + [b] + rows[:3]
    L = PC.rows(rows * 11, 1)                                # 286 rows; only the first copy's two splats are kept
    radii, m2, d, _, _ = PC.project(L, cam, W, H)
    keep = np.zeros(radii.shape, bool)
    keep[[5, len(rows) - 4]] = True
    radii = np.where(keep, radii, 0).astype(np.int32)
    assert (radii[keep] == PC.RADIUS_CLAMP).all() and d[5] == d[len(rows) - 4] == np.float32(10.0)
    return m2[None], radii[None], d[None], (5, len(rows) - 4)


@pytest.mark.parametrize("mode", ["radix", "bin"])
def test_tile_intersection_on_poisoned_scenes(ops, mode):
    from street_crafter_amd import isect
    with _setting(isect.set_isect_mode, mode), TP._routes():
        for case_id in ("plain", "two_cameras"):
            _, slots, p, t = _grafted(case_id, "culled")
            C = len(p["cameras"])
            got = _isect(ops, p["means2d"], p["radii"], p["depths"], C)
            for g, e, e2 in zip(got, _isect_oracle(p["means2d"], p["radii"], p["depths"], C),
                                _isect_oracle(t["means2d"], t["radii"], t["depths"], C)):
                _same(g, e.astype(g.dtype), f"{mode} {case_id} culled")
                _same(g, e2.astype(g.dtype), f"{mode} {case_id} twin")
            assert (got[0][:, slots] == 0).all()
        _, slots, p, _ = _grafted("plain", "visible")
        got = _isect(ops, p["means2d"], p["radii"], p["depths"], 1)
        for g, e in zip(got, _isect_oracle(p["means2d"], p["radii"], p["depths"], 1)):
            _same(g, e.astype(g.dtype), f"{mode} visible")
        assert (got[0][0, slots] > 0).all() and (got[0][0] == TW * TH).sum() >= 20
        m2, radii, d, (ia, ib) = _two_clamped_only()
        got = _isect(ops, m2, radii, d, 1)
        for g, e in zip(got, _isect_oracle(m2, radii, d, 1)):
            _same(g, e.astype(g.dtype), f"{mode} two clamped")
        np.testing.assert_array_equal(got[2].reshape(TW * TH, 2), np.tile([ia, ib], (TW * TH, 1)))
        np.testing.assert_array_equal(got[3].reshape(-1), 2 * np.arange(TW * TH))


def test_tile_intersection_ctypes_route_inside_guard_zones(ops):
    from street_crafter_amd import _lib
    _, slots, p, _ = _grafted("plain", "visible")
    _, _, pc, _ = _grafted("plain", "culled")
    res = {}
    prev = _lib.set_fast_binding(False)
    try:
        for fill in (0xA5, 0x3F):
            for tag, q in (("visible", p), ("culled", pc)):
                alloc = GuardedAlloc(fill, fill)
                with guarded_adapter(alloc), torch.no_grad():
                    m2, r, d = alloc.guard(_t(q["means2d"])), alloc.guard(torch.from_numpy(q["radii"]).to(DEV)), alloc.guard(_t(q["depths"]))
                    tpg, ids, fids = ops.isect_tiles(m2, r, d, TS, TW, TH, packed=False, n_cameras=1)
                    offs = ops.isect_offset_encode(ids, 1, TW, TH)
                    torch.cuda.synchronize()
                    fids = fids.plain() if hasattr(fids, "plain") else fids
                    res[fill, tag] = [_np(x).copy() for x in (tpg, ids, fids, offs)]
                assert alloc.broken_guards() == [], (fill, tag, alloc.broken_guards())
                _same(m2, q["means2d"]), _same(r, q["radii"]), _same(d, q["depths"])
    finally:
        _lib.set_fast_binding(prev)
    for tag, q in (("visible", p), ("culled", pc)):
        for a, b, e in zip(res[0xA5, tag], res[0x3F, tag], _isect_oracle(q["means2d"], q["radii"], q["depths"], 1)):
            _same(a, b, tag)
            _same(a, e.astype(a.dtype), tag)


# =============================================================================================
# forward, culled class: poisoned == twin, bit for bit, no pixel left out
# =============================================================================================
META_KEYS = ("radii", "means2d", "depths", "conics", "opacities", "colors", "tiles_per_gauss", "isect_ids", "flatten_ids",
             "isect_offsets")


def _rasterization(ops, p, render_mode, rasterize_mode, grad=False, absgrad=False):
    L = {k: _t(p[k]).requires_grad_(grad) for k in PG.LEAVES}
    V, K, ctr = TP._cameras(p)
    cam = p["cameras"][0]
    rc, ra, meta = ops.rasterization(L["means"], L["quats"], L["scales"], L["opacities"].reshape(-1), L["sh"], V, K, W, H,
                                     near_plane=cam.znear, far_plane=cam.zfar, sh_degree=p["sh_degree"], render_mode=render_mode,
                                     rasterize_mode=rasterize_mode, camera_centers_=ctr, absgrad=absgrad)
    return L, rc, ra, meta


def _compare_frames(tag, p_out, t_out, nan_opacity_slots):
    (_, rc_p, ra_p, m_p), (_, rc_t, ra_t, m_t) = p_out, t_out
    assert m_p["fused"] == m_t["fused"]
    assert torch.equal(rc_p.detach().contiguous().view(torch.int32), rc_t.detach().contiguous().view(torch.int32)), tag
    assert torch.equal(ra_p.detach().contiguous().view(torch.int32), ra_t.detach().contiguous().view(torch.int32)), tag
    assert bool(torch.isfinite(rc_p).all()) and float(ra_p.sum()) > 0, tag
    for key in META_KEYS:
        a, b = m_p[key], m_t[key]
        a, b = (x.plain() if hasattr(x, "plain") else x for x in (a, b))
        a, b = _np(a), _np(b)
        if key == "opacities":          # the one output nothing reads: NaN * 0 on a culled row that holds a NaN opacity
            assert np.isnan(a[:, nan_opacity_slots]).all(), tag
            a, b = np.delete(a, nan_opacity_slots, axis=1), np.delete(b, nan_opacity_slots, axis=1)
        _same(a, b, f"{tag} meta[{key}]")


@pytest.mark.parametrize("rasterize_mode", ["antialiased", "classic"])
@pytest.mark.parametrize("case_id", ["plain", "two_cameras"])
def test_forward_with_culled_rows_equals_the_twin_bit_for_bit(ops, case_id, rasterize_mode):
    from street_crafter_amd import rendering
    pick, slots, p, t = _grafted(case_id, "culled")
    nan_op = [s for r, s in zip(pick, slots) if "opacities" in r.fields]
    assert len(nan_op) == 2
    n = 0
    with TP._routes():
        for render_mode in ("RGB", "RGB+ED", "D"):
            for fused in (False, True):
                for packed in ((True, False) if fused else (True,)):
                    for planar in (True, False):
                        with _setting(rendering.set_fused_rasterization, fused), _setting(rendering.set_packed_records, packed), \
                                _setting(rendering.set_planar_output, planar), torch.no_grad():
                            outs = [_rasterization(ops, q, render_mode, rasterize_mode) for q in (p, t)]
                            torch.cuda.synchronize()
                        if fused and render_mode == "RGB+ED":
                            assert outs[0][3]["fused"]
                        _compare_frames(f"{case_id} {rasterize_mode} {render_mode} fused={fused} packed={packed} planar={planar}",
                                        outs[0], outs[1], nan_op)
                        n += 1
        # the training routes' forwards: the composition and the fused per-Gaussian node, under grad
        for fused_train in (False, True):
            with _setting(rendering.set_fused_training, fused_train):
                outs = [_rasterization(ops, q, "RGB+ED", rasterize_mode, grad=True, absgrad=True) for q in (p, t)]
                torch.cuda.synchronize()
            assert outs[0][3]["fused"] == fused_train
            _compare_frames(f"{case_id} {rasterize_mode} train fused={fused_train}", outs[0], outs[1], nan_op)
    assert n == 18


def test_grouped_and_layered_entries_with_culled_rows_equal_the_twin(ops):
    """The grouped and the layered rasterizer on the oracle's arrays of the poisoned scene -- the rows nothing lists hold
    NaN opacities among them -- against the twin's: every image bit-identical.  The grafted rows are spread over the
    groups (ids 0, 1 and "no group") and over both layers."""
    from street_crafter_amd import groups, layers
    pick, slots, p, t = _grafted("plain", "culled")
    N = p["means"].shape[0]
    gid = (np.arange(N) % 3).astype(np.uint8)
    gid[gid == 2] = 255
    assert {int(g) for g in gid[slots]} == {0, 1, 255} and min(slots) < 1200 < max(slots)
    assert np.isnan(p["opacities2d"][:, slots]).any() and np.isfinite(t["opacities2d"]).all()
    outs = []
    for q in (p, t):
        a = [_t(q[k]) for k in ("means2d", "conics", "colors", "opacities2d")]
        with torch.no_grad():
            g = groups.rasterize_to_pixels_grouped(*a, W, H, TS, torch.from_numpy(q["isect_offsets"]).to(DEV),
                                                   torch.from_numpy(q["flatten_ids"]).to(DEV), torch.from_numpy(gid).to(DEV), 2)
            lifted = _np(layers.layered_depths(_t(q["depths"]), 1200))
            _, ids, fids = O.isect_tiles(q["means2d"], q["radii"], lifted, TS, TW, TH, n_cameras=1)
            offs = O.isect_offset_encode(ids, 1, TW, TH)
            lay = layers.rasterize_to_pixels_layered(*a, W, H, TS, torch.from_numpy(offs).to(DEV), torch.from_numpy(fids).to(DEV), 1200)
            torch.cuda.synchronize()
        outs.append(list(g) + list(lay))
    assert len(outs[0]) == 8
    for i, (a, b) in enumerate(zip(*outs)):
        assert bool(torch.isfinite(a).all()) and float(a.abs().sum()) > 0, i
        _same(a.contiguous(), b.contiguous(), f"grouped / layered output {i}")


# =============================================================================================
# forward, visible class: per pixel against float64
# =============================================================================================
@pytest.mark.parametrize("rasterize_mode", ["antialiased", "classic"])
def test_forward_with_visible_rows_per_pixel_against_float64(ops, rasterize_mode):
    """Among them what no other test holds: conics of exactly 0 (classic: they blend at their opacity into every pixel) and
    twenty splats that cover every tile."""
    from street_crafter_amd import rendering
    _, slots, p, _ = _grafted("plain", "visible")
    op = p["opacities2d"] if rasterize_mode == "antialiased" else np.broadcast_to(p["opacities"][None, :, 0], p["radii"].shape)
    ref = RF.rasterize_fwd(p["means2d"], p["conics"], p["colors"], np.ascontiguousarray(op), W, H, TS, p["isect_offsets"],
                           p["flatten_ids"])
    assert RF.near_share(ref) < RC.UNSTABLE_CAP and ref["truncated"] == 0
    assert ((p["conics"][0, slots] == 0).all(-1)).sum() == 4
    for fused in (False, True):
        with TP._routes(), _setting(rendering.set_fused_rasterization, fused), torch.no_grad():
            _, rc, ra, meta = _rasterization(ops, p, "RGB+D", rasterize_mode)
            torch.cuda.synchronize()
        assert meta["fused"] == fused
        TP._check_lists(p, meta["radii"], meta["isect_offsets"], meta["flatten_ids"])
        _same(meta["conics"], p["conics"]), _same(meta["means2d"], p["means2d"])
        _same(meta["opacities"], np.ascontiguousarray(op, np.float32)), _same(meta["colors"], p["colors"])
        j = RF.judge(ref, _np(rc.contiguous()), _np(ra))
        print(f"[hip] visible rows {rasterize_mode} fused={fused}: colours {j['colors']:.2f} alphas {j['alphas']:.2f}, bar {RF.K:.2f}; "
              f"{j['alt']} pixels by another outcome")
        assert j["ratio"].max() <= RF.K, (rasterize_mode, fused, j["colors"], j["alphas"])


# =============================================================================================
# backward
# =============================================================================================
def _step(ops, p, route):
    """-> (leaves, viewspace points) after backward of param_grad_f64's loss."""
    from street_crafter_amd import rendering
    if route == "operators":
        return TP._step_operators(ops, p)
    if route == "rasterization":
        return TP._step_rasterization(ops, p)
    with _setting(rendering.set_fused_training, True):
        L, rc, ra, meta = _rasterization(ops, p, "RGB+ED", "antialiased" if p["antialiasing"] else "classic", grad=True, absgrad=True)
        assert meta["fused"]
        TP._check_lists(p, meta["radii"], meta["isect_offsets"], meta["flatten_ids"])
        meta["means2d"].retain_grad()
        TP._loss(p, rc[..., :3], ra[..., 0], rc[..., 3]).backward()
        torch.cuda.synchronize()
        return L, meta["means2d"]


def _grads(L, vp):
    g = {k: L[k].grad for k in PG.LEAVES}
    g["means2d"], g["absgrad"] = vp.grad, vp.absgrad
    assert all(v is not None for v in g.values())
    return g


def _row(g, k, rows):
    return g[k][:, rows] if k in ("means2d", "absgrad") else g[k][rows]


BWD_RUNS = [(c, r, v, n, s) for c, r in (("plain", "operators"), ("plain", "fused_train"), ("two_cameras", "rasterization"),
                                         ("two_cameras", "fused_train"))
            for v, n, s in ((0, True, 1), (1, True, 1), (1, False, 1), (1, True, 0), (0, False, 0))]


@pytest.mark.parametrize("case_id,route,raster_bwd,native,bwd_split", BWD_RUNS,
                         ids=[f"{c}-{r}-bwd{v}-{'compiled' if n else 'python'}-split{s}" for c, r, v, n, s in BWD_RUNS])
def test_backward_with_culled_rows(ops, case_id, route, raster_bwd, native, bwd_split):
    """Grafted rows: exactly +0 on all five leaves, in viewspace_points.grad and .absgrad (bytes: -0 and NaN both fail).
    Every other row: param_grad_f64's bar against reference(twin) with the module's own K; where the twin's backward is the
    same from run to run, bit-equal to the twin's."""
    _, K = TP.build_refs()
    _, slots, p, t = _grafted(case_id, "culled")
    ref = _twin_reference(case_id)
    others = np.setdiff1d(np.arange(p["means"].shape[0]), slots)
    with TP._routes(native=native, raster_bwd=raster_bwd), _option("raster_bwd_split", bwd_split):
        gp = _grads(*_step(ops, p, route))
        gt1 = _grads(*_step(ops, t, route))
        gt2 = _grads(*_step(ops, t, route))
    for k, g in gp.items():
        assert _zero_bytes(_row(gp, k, slots)), (k, _np(_row(gp, k, slots)))
        assert bool(torch.isfinite(g).all()), k
    got = {k: _np(gp[k]).astype(np.float64) for k in PG.JUDGED}
    worst = PG.worst_ratios(got, ref)
    print(f"[hip] poisoned {case_id} {route}: " + ", ".join(f"{k} {r:.1f}" for k, (r, _) in worst.items()) + f"; bar {K:.1f}")
    for k, (r, off) in worst.items():
        assert off == 0.0 and r <= K, (k, r, off, K)
    ab = _np(gp["absgrad"]).astype(np.float64)
    assert (ab[ref["S"]["means2d"] == 0] == 0).all() and (ab + 1e-6 * ab.max() >= np.abs(got["means2d"])).all()
    repeatable = [k for k in gp if torch.equal(gt1[k], gt2[k])]
    print(f"[hip] twin backward repeats bit for bit on: {repeatable}")
    for k in repeatable:
        _same(_row(gp, k, others), _row(gt1, k, others), k)


@functools.lru_cache(maxsize=None)
def _judged_reference():
    _, slots, p, _ = _grafted("plain", "judged")
    ref = PG.reference(p)
    keep = np.setdiff1d(np.arange(p["means"].shape[0]), slots)
    return keep, {q: {k: (v[:, keep] if k == "means2d" else v[keep]) for k, v in ref[q].items()} for q in ("G", "S", "A")}


VIS_RUNS = [(r, v, n, s) for r in ("operators", "fused_train") for v, n, s in ((0, True, 1), (1, True, 1), (1, False, 1), (1, True, 0), (0, False, 0))]


@pytest.mark.parametrize("route,raster_bwd,native,bwd_split", VIS_RUNS,
                         ids=[f"{r}-bwd{v}-{'compiled' if n else 'python'}-split{s}" for r, v, n, s in VIS_RUNS])
def test_backward_with_visible_rows_per_row_against_float64(ops, route, raster_bwd, native, bwd_split):
    """The twelve visible recipes the float64 chain can judge (oracle/poison_cases.py::gradient_judged: eight needles listed
    in every tile among them) grafted into `plain`: every row that is NOT grafted within param_grad_f64's bar of
    reference(poisoned) with the module's own K, and finite.  The grafted rows' own gradients are not judged."""
    _, K = TP.build_refs()
    _, slots, p, _ = _grafted("plain", "judged")
    keep, ref = _judged_reference()
    assert float(p["unstable"].mean()) < RC.UNSTABLE_CAP and (p["radii"][0, slots] == PC.RADIUS_CLAMP).sum() == 8
    with TP._routes(native=native, raster_bwd=raster_bwd), _option("raster_bwd_split", bwd_split):
        g = _grads(*_step(ops, p, route))
    got = {k: _np(_row(g, k, keep)).astype(np.float64) for k in PG.JUDGED}
    assert all(np.isfinite(v).all() for v in got.values()) and bool(torch.isfinite(_row(g, "absgrad", keep)).all())
    worst = PG.worst_ratios(got, ref)
    print(f"[hip] visible rows grafted, {route}: " + ", ".join(f"{k} {r:.1f}" for k, (r, _) in worst.items()) + f"; bar {K:.1f}")
    for k, (r, off) in worst.items():
        assert off == 0.0 and r <= K, (k, r, off, K)


@pytest.mark.parametrize("route", ["operators", "fused_train"])
def test_backward_with_visible_rows_stays_finite_elsewhere(ops, route):
    """All 24 visible recipes, the twelve included on which the float64 chain is no reference (the catalogue's docstring
    says why): a visible recipe's own gradient may be non-finite (1 / det1 of an infinite det1); no other row's is."""
    _, slots, p, _ = _grafted("plain", "visible")
    others = np.setdiff1d(np.arange(p["means"].shape[0]), slots)
    for raster_bwd in (0, 1):
        with TP._routes(raster_bwd=raster_bwd):
            g = _grads(*_step(ops, p, route))
        for k in g:
            assert bool(torch.isfinite(_row(g, k, others)).all()), (route, raster_bwd, k)
        assert float(g["means"][others].abs().sum()) > 0


def test_projection_and_sh_backward_never_read_a_culled_rows_upstream(ops):
    """sc_projection_bwd and the SH backward called directly: NaN in all upstream tensors at the culled (camera, row) pairs
    gives exactly 0 there and the same bits everywhere else as zeros in their place."""
    cams = _proj_cams()
    cat = [r for r in PC.camera_free() if r.cls == "culled"]        # culled under every camera
    case = PG.make_case("plain")
    n = 600
    L = {k: case[k][:n].copy() for k in ("means", "quats", "scales")}
    slots = PC.slots_for(n, 8)[:5] + [100, 101, 300] + list(range(400, 400 + len(cat) - 8))
    for r, s in zip(cat, slots):
        for k in L:
            L[k][s] = np.asarray(r.fields[k], np.float32)
    V = torch.stack([c.viewmat for c in cams.values()]).to(DEV)
    K = torch.stack([c.K for c in cams.values()]).to(DEV)
    rng = np.random.default_rng(3)
    ups = [rng.normal(size=s).astype(np.float32) for s in ((3, n, 2), (3, n), (3, n, 3), (3, n))]
    for fast in (True, False):
        res = []
        for fill in (np.nan, 0.0):
            leaves = [_t(L[k]).requires_grad_(True) for k in ("means", "quats", "scales")]
            with TP._routes(fast=fast, native=fast):
                radii, m2, d, con, comp = ops.fully_fused_projection(leaves[0], None, leaves[1], leaves[2], V, K, W, H, near_plane=0.001,
                                                                     far_plane=1000.0, calc_compensations=True)
                dead = radii <= 0
                assert bool(dead[:, slots].all()) and bool((~dead).any())
                v = []
                for u in ups:
                    u = _t(u)
                    u[dead] = fill
                    v.append(u)
                torch.autograd.backward([m2, d, con, comp], v)
                torch.cuda.synchronize()
            res.append([x.grad for x in leaves])
        nowhere = _np(dead.all(0))
        for a, b in zip(*res):
            assert _zero_bytes(a[torch.from_numpy(nowhere).to(DEV)])
            _same(a, b, f"projection backward fast={fast}")
        assert bool(torch.isfinite(torch.cat([x.reshape(-1) for x in res[0]])).all())
        # SH backward under masks = radii > 0, NaN directions and coefficients on the masked rows
        dirs = torch.randn(3, n, 3, device=DEV)
        sh = torch.randn(3, n, 9, 3, device=DEV)
        res = []
        for fill in (np.nan, 0.0):
            dd, cc = dirs.clone(), sh.clone()
            dd[dead], cc[dead] = np.nan, np.nan
            dd.requires_grad_(True), cc.requires_grad_(True)
            u = torch.ones(3, n, 3, device=DEV)
            u[dead] = fill
            with TP._routes(fast=fast, native=fast):
                out = ops.spherical_harmonics(2, dd, cc, masks=~dead)
                assert _zero_bytes(out[dead])
                out.backward(u)
                torch.cuda.synchronize()
            res.append((dd.grad, cc.grad))
        for a, b in zip(*res):
            assert _zero_bytes(a[dead])
            _same(a, b, f"sh backward fast={fast}")


# =============================================================================================
# training tail
# =============================================================================================
def test_adam_and_densification_statistics_keep_culled_rows_out(ops):
    """One fused Adam step, one step of the densification statistics and one densify call whose thresholds select nothing,
    on the poisoned scene's and on the twin's own backward: grafted rows keep their bytes -- gradient and state are zero --,
    every statistics column stays zero for them, nothing is cloned, split or pruned and the row counts are equal.
    Row-locality of the three kernels bit for bit: the rasterizer backward's atomics make no two backward runs equal (the
    gradients themselves are judged per row in the tests above), so the twin is stepped a second time on the POISONED run's
    gradients and viewspace points; every row that is not grafted must then come out bit-identical to the poisoned scene's,
    parameters, both moments and all statistics columns."""
    from street_crafter_amd import optim
    from street_crafter_amd import densify as D
    from street_crafter_amd.densify_stats import DensificationStats
    _, slots, p, t = _grafted("plain", "culled")
    N = p["means"].shape[0]
    others = np.setdiff1d(np.arange(N), slots)
    after, stats, counts, first = [], [], [], None
    with TP._routes():
        for q, own in ((p, True), (t, True), (t, False)):
            if own:
                L, vp = _step(ops, q, "fused_train")
                first = first or (L, vp)
            else:
                L = {k: _t(q[k]).requires_grad_(True) for k in PG.LEAVES}
                for k in PG.LEAVES:
                    L[k].grad = first[0][k].grad.clone()
                vp = first[1]
            before = {k: L[k].detach().clone() for k in PG.LEAVES}
            opt = optim.Adam([{"params": [L[k]], "name": k} for k in PG.LEAVES], lr=1e-2)
            opt.step()
            torch.cuda.synchronize()
            state = {k: opt.state[L[k]] for k in PG.LEAVES}
            for k in PG.LEAVES:
                a, b = L[k].detach()[slots], before[k][slots]
                assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), k
                assert _zero_bytes(state[k]["exp_avg"][slots]) and _zero_bytes(state[k]["exp_avg_sq"][slots]), k
            after.append({**{k: L[k].detach() for k in PG.LEAVES},
                          **{k + "/m": state[k]["exp_avg"] for k in PG.LEAVES}, **{k + "/v": state[k]["exp_avg_sq"] for k in PG.LEAVES}})
            st = DensificationStats({"all": (0, N)}, device=DEV)
            radii = torch.from_numpy(q["radii"][0]).to(DEV)
            out = dict(radii=radii.float() / max(W, H), visibility_filter=radii > 0, viewspace_points=vp)
            st.accumulate_from_render_fused(out, W, H)
            torch.cuda.synchronize()
            cols = dict(accum=st.xyz_gradient_accum["all"], denom=st.denom["all"], max_radii=st.max_radii2D["all"])
            for k, v in cols.items():
                assert _zero_bytes(v[slots]), k
                assert bool(torch.isfinite(v).all()), k
            stats.append({k: v.clone() for k, v in cols.items()})
            # one densify call whose thresholds select nothing (no gradient reaches max_grad, sigmoid(opacity) >= 0 > -1):
            # the NaN and infinite scales / opacities of the grafted rows meet every comparison of the plan kernel
            res = D.densify_and_prune_many([D.DensifyJob(
                optimizer=opt, xyz_gradient_accum=cols["accum"], denom=cols["denom"], max_radii2D=cols["max_radii"],
                max_grad=1e30, extent=1.0, min_opacity=-1.0, xyz="means", scaling="scales", rotation="quats",
                opacity="opacities", passengers=("sh",))])[0]
            torch.cuda.synchronize()
            counts.append((res.n_out, dict(res.scalar_dict)))
            assert res.n_out == N and torch.equal(res.src_row.cpu(), torch.arange(N, dtype=torch.int32)), res.scalar_dict
            assert all(res.scalar_dict[k] == 0 for k in ("points_clone", "points_split", "points_pruned")), res.scalar_dict
            for k in PG.LEAVES:
                a, b = res.params[k].detach()[slots], L[k].detach()[slots]
                assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), k
    for k in after[0]:
        _same(after[0][k][others], after[2][k][others], k)
    for k in stats[0]:
        _same(stats[0][k][others], stats[2][k][others], k)
    assert float(stats[0]["denom"].sum()) > 0
    assert counts[0] == counts[1] == counts[2], counts
