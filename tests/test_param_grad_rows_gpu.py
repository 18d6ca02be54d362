"""What the optimiser receives, judged PER GRADIENT ROW against float64 references:

E  the training step end to end -- `render_gaussians(mode="train")`, and for two cameras the operator sequence and
   `rasterization()` -- against oracle/param_grad_f64.py: every leaf gradient and viewspace_points.grad within
       |hip - G| <= 2^-24 (K S + A),   exactly 0 where S == 0,   .grad is None exactly for frozen leaves,
   on the tile lists the numpy oracle built (asserted bit-equal to the operators').  K = 4 K_ref, K_ref the largest ratio
   the float32 replay of the torch oracle chain (CPU, no kernel) reaches over all rows, leaves and cases; the 4 is the
   project's margin for v_exp_f32 / v_rcp_f32, FMA contraction and atomics in arbitrary order.  These runs hand the
   operators the cameras' stored centres; one more lets `rasterization()` derive them from the view matrices, judges the
   derived centres against float64 and the gradients against the case rebuilt on them.
C  spherical_harmonics backward against the closed form of oracle/sh_bwd_f64.py: |hip - G| <= 2^-24 K_sh S per entry,
   exact zeros for masked-off rows (a zero direction among them), bases beyond the degree and v_dirs at degree 0.
D  sc_projection_bwd with three cameras against the sum over cameras of the single-camera float64 autograd, under the
   per-row conditioning bars of test_gpu_parity.py::test_projection_backward_one_output_at_a_time.

tests/test_param_grad_ref_cpu.py judges the references on their own (and shows which wrong results the per-row bars
catch that max|a - b| / max|b| lets pass).
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gsplat_torch as OT              # noqa: E402  (checker only)
from oracle import param_grad_f64 as PG            # noqa: E402
from oracle import raster_bwd_cases as RC          # noqa: E402
from oracle import raster_bwd_f64 as RB            # noqa: E402
from oracle import sh_bwd_f64 as SH                # noqa: E402
from street_crafter_amd.scenes import Scene, make_camera, make_scene   # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from street_crafter_amd import _lib
    _lib.load()
    import gsplat.rendering as R
    return R


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


class _routes:
    """ctypes table or compiled binding layer, Python or compiled autograd functions, and the rasterizer's backward."""

    def __init__(self, fast=True, native=True, raster_bwd=None):
        self.want = (fast, native, raster_bwd)

    def __enter__(self):
        from street_crafter_amd import _lib, rendering
        fast, native, raster_bwd = self.want
        self.undo = []          # one entry per setting actually changed: whatever fails below, the session gets them back
        try:
            prev = _lib.set_fast_binding(fast)
            self.undo.append(lambda: _lib.set_fast_binding(prev))
            prev_native = rendering.set_native_autograd(native)
            self.undo.append(lambda: rendering.set_native_autograd(prev_native))
            if raster_bwd is not None:
                prev_bwd = _lib.set_option("raster_bwd", raster_bwd)
                self.undo.append(lambda: _lib.set_option("raster_bwd", prev_bwd))
            assert (_lib.fast() is not None) == fast
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        while self.undo:
            self.undo.pop()()
        return False


# =============================================================================================
# E  the training step end to end
# =============================================================================================
@functools.lru_cache(maxsize=None)
def build_refs():
    """{case: (inputs, float64 reference)} and K: ONE number for the module (and for tests/test_call_history_gpu.py, which
    holds the training steps of its call histories to the same bar: built once per process)."""
    table, k_ref = {}, 0.0
    for cid in PG.CASE_IDS:
        p = PG.make_case(cid)
        ref = PG.reference(p)
        rep = PG.worst_ratios(PG.chain(p, torch.float32)["G"], ref)
        assert all(off == 0.0 for _, off in rep.values()), (cid, rep)
        print(f"[replay] {cid}: K_ref " + ", ".join(f"{k} {r:.1f}" for k, (r, _) in rep.items())
              + f"; left out {100 * p['unstable'].mean():.3f} %")
        k_ref = max(k_ref, max(r for r, _ in rep.values()))
        table[cid] = (p, ref)
    print(f"[replay] K_ref over {len(table)} cases: {k_ref:.1f}; K = {4 * k_ref:.1f}")
    assert PG.K_REF_BAND[0] < k_ref < PG.K_REF_BAND[1]
    return table, 4.0 * k_ref


@pytest.fixture(scope="module")
def refs():
    return build_refs()


def _leaves(p):
    return {k: _t(p[k]).requires_grad_(k not in p["frozen"]) for k in PG.LEAVES}


def _loss(p, rgb, acc, depth):
    """rgb [C,H,W,3], acc [C,H,W], depth [C,H,W] under the case's weights."""
    return (rgb * _t(p["w_rgb"])).sum() + (acc * _t(p["w_acc"])).sum() + (depth * _t(p["w_depth"])).sum()


def _check_lists(p, radii, offs, fids):
    fids = fids.plain() if hasattr(fids, "plain") else fids
    np.testing.assert_array_equal(_np(radii), p["radii"])
    np.testing.assert_array_equal(_np(offs), p["isect_offsets"])
    np.testing.assert_array_equal(_np(fids), p["flatten_ids"])


def _step_caller(ops, p):
    """harness/caller.py's train step (one camera)."""
    from harness.caller import render_gaussians
    L = _leaves(p)
    sc = Scene(L["means"], L["quats"], L["scales"], L["opacities"], L["sh"], p["sh_degree"])
    out = render_gaussians(sc, p["cameras"][0].to(DEV), mode="train", antialiasing=p["antialiasing"], return_intermediates=True)
    _check_lists(p, out["_radii"], out["_isect_offsets"], out["_flatten_ids"])
    _loss(p, out["rgb"].permute(1, 2, 0)[None], out["acc"], out["depth"]).backward()
    torch.cuda.synchronize()
    return L, out["viewspace_points"]


def _cameras(p):
    cams = p["cameras"]
    return (torch.stack([c.viewmat for c in cams]).to(DEV), torch.stack([c.K for c in cams]).to(DEV),
            torch.stack([c.camera_center for c in cams]).to(DEV))


def _forward_operators(ops, p):
    """The caller's sequence spelt out for C cameras, up to the loss -> (leaves, viewspace points, loss)."""
    L = _leaves(p)
    V, K, ctr = _cameras(p)
    C, W, H, ts = V.shape[0], p["width"], p["height"], p["tile_size"]
    cam = p["cameras"][0]
    radii, m2, d, con, comp = ops.fully_fused_projection(L["means"], None, L["quats"], L["scales"], V, K, W, H, packed=False,
                                                         near_plane=cam.znear, far_plane=cam.zfar,
                                                         calc_compensations=p["antialiasing"])
    op = L["opacities"][None, :, 0].expand(C, -1)
    if comp is not None:
        op = op * comp
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    _, ids, fids = ops.isect_tiles(m2, radii, d, ts, tw, th, packed=False, n_cameras=C)
    offs = ops.isect_offset_encode(ids, C, tw, th)
    _check_lists(p, radii, offs, fids)
    dirs = L["means"][None] - ctr[:, None, :]
    cols = ops.spherical_harmonics(p["sh_degree"], dirs, L["sh"][None].expand(C, -1, -1, -1), masks=radii > 0)
    cols = torch.clamp_min(cols + 0.5, 0.0)
    m2.retain_grad()
    cols = torch.cat((cols, d[..., None]), dim=-1)
    rc, ra = ops.rasterize_to_pixels(m2, con, cols, op.contiguous(), W, H, ts, offs, fids, backgrounds=None, packed=False, absgrad=True)
    return L, m2, _loss(p, rc[..., :3], ra[..., 0], rc[..., 3] / ra[..., 0].clamp(min=1e-10))


def _step_operators(ops, p):
    L, m2, loss = _forward_operators(ops, p)
    loss.backward()
    torch.cuda.synchronize()
    return L, m2


def _forward_rasterization(ops, p, own_centers=False):
    """gsplat's one-call API in training mode on the same inputs (RGB+ED: it divides the depth channel itself), up to the
    loss -> (leaves, viewspace points, loss).
    own_centers: without `camera_centers_`, so that it derives the camera positions from the view matrices itself."""
    L = _leaves(p)
    V, K, ctr = _cameras(p)
    cam = p["cameras"][0]
    rc, ra, meta = ops.rasterization(L["means"], L["quats"], L["scales"], L["opacities"].reshape(-1), L["sh"], V, K, p["width"],
                                     p["height"], near_plane=cam.znear, far_plane=cam.zfar, sh_degree=p["sh_degree"],
                                     render_mode="RGB+ED", absgrad=True,
                                     rasterize_mode="antialiased" if p["antialiasing"] else "classic",
                                     camera_centers_=None if own_centers else ctr)
    assert not meta["fused"]
    _check_lists(p, meta["radii"], meta["isect_offsets"], meta["flatten_ids"])
    meta["means2d"].retain_grad()
    return L, meta["means2d"], _loss(p, rc[..., :3], ra[..., 0], rc[..., 3])


def _step_rasterization(ops, p, own_centers=False):
    L, vp, loss = _forward_rasterization(ops, p, own_centers)
    loss.backward()
    torch.cuda.synchronize()
    return L, vp


def _judge_step(tag, p, ref, K, L, vp):
    got = {}
    for k in PG.LEAVES:
        assert (L[k].grad is None) == (k in p["frozen"]), (tag, k)
        if L[k].grad is not None:
            got[k] = _np(L[k].grad).astype(np.float64)
    assert vp.grad is not None and hasattr(vp, "absgrad")
    got["means2d"] = _np(vp.grad).astype(np.float64)
    worst = PG.worst_ratios(got, ref, list(got))
    print(f"[hip] {tag}: " + ", ".join(f"{k} {r:.1f}" + (f" (|x| {off:.1e} where S = 0)" if off else "") for k, (r, off) in worst.items())
          + f"; bar {K:.1f}")
    for k, (r, off) in worst.items():
        assert np.isfinite(got[k]).all(), (tag, k)
        assert off == 0.0, (tag, k, off)
        assert r <= K, (tag, k, r, K)
    # absgrad rides on the same rows (its own per-row bar: tests/test_raster_bwd_rows_gpu.py)
    ab = _np(vp.absgrad).astype(np.float64)
    assert (ab[ref["S"]["means2d"] == 0] == 0).all() and (ab + 1e-6 * ab.max() >= np.abs(got["means2d"])).all(), tag
    assert float(p["unstable"].mean()) < RC.UNSTABLE_CAP and (ref["S"]["means"] > 0).any(), tag


STEPS = {"caller": _step_caller, "operators": _step_operators, "rasterization": _step_rasterization}
# (case, route, raster_bwd, compiled autograd functions)
RUNS = ([(c, "caller", None, True) for c in PG.CASE_IDS if c != "two_cameras"]
        + [("two_cameras", "operators", None, True), ("two_cameras", "rasterization", None, True)]
        + [("plain", "caller", v, n) for v in (0, 1) for n in (True, False)]
        + [("two_cameras", r, v, n) for r in ("operators", "rasterization") for v in (0, 1) for n in (True, False)])


@pytest.mark.parametrize("case_id,route,raster_bwd,native", RUNS,
                         ids=[f"{c}-{r}-bwd{'default' if v is None else v}-{'compiled' if n else 'python'}" for c, r, v, n in RUNS])
def test_train_step_rows_against_the_float64_chain(ops, refs, case_id, route, raster_bwd, native):
    table, K = refs
    p, ref = table[case_id]
    assert len(p["cameras"]) == (2 if case_id == "two_cameras" else 1)
    with _routes(native=native, raster_bwd=raster_bwd):
        L, vp = STEPS[route](ops, p)
    _judge_step(f"{case_id} {route} raster_bwd={raster_bwd} compiled_autograd={native}", p, ref, K, L, vp)


def test_train_step_rows_through_the_ctypes_table(ops, refs):
    table, K = refs
    for case_id, route in (("plain", "caller"), ("two_cameras", "operators")):
        p, ref = table[case_id]
        with _routes(fast=False, native=False):
            L, vp = STEPS[route](ops, p)
        _judge_step(f"{case_id} {route} ctypes", p, ref, K, L, vp)


def test_train_step_rows_with_the_camera_centres_rasterization_derives(ops, refs):
    """`rasterization()` WITHOUT `camera_centers_` -- what a gsplat caller writes -- takes the camera positions from
    `camera_centers(viewmats)`, the rigid inverse -R^T t evaluated in float32 on the device, not from the cameras' stored
    float64-rounded `camera_center` the runs above pass in.  Two things are judged:
      the centres themselves: each component is three products and two sums, at most three roundings deep, so
        |c_hip - c_f64| <= 4 x 2^-24 sum_i |R_ij| |t_i|   (first-order bound 3, the fourth for the second-order terms);
      the gradients: the derived centres are a FACT of this forward like its tile lists, so the case is rebuilt on them
        (colours, unstable pixels, float64 chain, S and A) and held to the same bar with the same K.  The conditions every
        case meets are re-asserted for the rebuilt one (tests/test_param_grad_ref_cpu.py checks them for the stored centres)."""
    table, K = refs
    p0, ref0 = table["two_cameras"]
    V = torch.stack([c.viewmat for c in p0["cameras"]])
    from street_crafter_amd.rendering import camera_centers
    ctr = _np(camera_centers(V.to(DEV)))
    R, t = V.double().numpy()[:, :3, :3], V.double().numpy()[:, :3, 3]
    exact = -np.einsum("cij,ci->cj", R, t)
    bound = 4 * 2.0 ** -24 * np.einsum("cij,ci->cj", np.abs(R), np.abs(t))
    stored = np.stack([c.camera_center.numpy() for c in p0["cameras"]])
    print(f"[hip] camera centres: |hip - f64| / bound {(np.abs(ctr - exact)[bound > 0] / bound[bound > 0]).max():.3f}; "
          f"{int((ctr != stored).sum())} of {ctr.size} components differ from the stored float32 ones")
    assert (np.abs(ctr - exact) <= bound).all(), (ctr, exact)
    if (ctr == stored).all():
        p, ref = p0, ref0
    else:
        p = PG.make_case("two_cameras", centers=ctr)
        ref = PG.reference(p)
        vis = p["radii"] > 0
        np.testing.assert_array_equal(ref["radii"] > 0, vis)
        assert np.abs(p["colors_pre_clamp"][vis]).min() > PG.CLAMP_WINDOW
    with _routes():
        L, vp = _step_rasterization(ops, p, own_centers=True)
    _judge_step("two_cameras rasterization, centres derived from viewmats", p, ref, K, L, vp)


# =============================================================================================
# C  spherical_harmonics backward per row
# =============================================================================================
@pytest.fixture(scope="module")
def k_sh():
    worst = SH.k_ref()
    print(f"[sh replay] K_ref over {len(SH.all_inputs())} inputs: {worst:.2f}; K_sh = {4 * worst:.1f}")
    assert SH.K_REF_BAND[0] < worst < SH.K_REF_BAND[1]
    return 4.0 * worst


def _sh_hip(ops, p, dirs_grad=True, strided_v=False):
    d = _t(p["dirs"]).requires_grad_(dirs_grad)
    c = _t(p["coeffs"]).requires_grad_(True)
    m = None if p["masks"] is None else torch.from_numpy(p["masks"]).to(DEV)
    v = _t(p["v_colors"])
    if strided_v:            # the upstream gradient as a view of a wider tensor: the operator must not read it as dense
        wide = torch.full(v.shape[:-1] + (5,), 1e9, device=DEV)
        wide[..., 1:4] = v
        v = wide[..., 1:4]
        assert not v.is_contiguous()
    out = ops.spherical_harmonics(p["degree"], d, c, masks=m)
    out.backward(v)
    torch.cuda.synchronize()
    return {"coeffs": _np(c.grad), "dirs": None if d.grad is None else _np(d.grad)}


def _judge_sh(tag, got, p, K):
    ref = SH.reference(p)
    line = []
    for name in ("coeffs", "dirs"):
        if got[name] is None:
            continue
        assert np.isfinite(got[name]).all(), (tag, name)             # no NaN anywhere, the zero directions included
        r, off = RB.row_ratio(got[name], ref, name)
        worst = float(r.max()) if r.size else 0.0
        line.append(f"{name} {worst:.2f}")
        assert off == 0.0, (tag, name, off)
        assert worst <= K, (tag, name, worst, K)
    print(f"[hip sh] {tag}: " + ", ".join(line) + f"; bar {K:.1f}")
    Kd = (p["degree"] + 1) ** 2
    assert (got["coeffs"][..., Kd:, :] == 0).all()
    if p["masks"] is not None:
        assert (got["coeffs"][~p["masks"]] == 0).all() and (got["dirs"] is None or (got["dirs"][~p["masks"]] == 0).all())
    if p["degree"] == 0 and got["dirs"] is not None:
        assert (got["dirs"] == 0).all()


@pytest.mark.parametrize("fast", [True, False], ids=["compiled", "ctypes"])
@pytest.mark.parametrize("deg,k_total", SH.DEG_K_TOTAL)
def test_sh_backward_rows_every_degree_and_row_length(ops, k_sh, deg, k_total, fast):
    p = SH.make_inputs(deg, k_total, (2000,), "random")
    dead = ~p["masks"]
    assert (np.abs(p["dirs"][dead]).sum(-1) == 0).any() and (np.abs(p["dirs"][dead]).sum(-1) > 0).any()
    n = np.sqrt((p["dirs"].astype(np.float64) ** 2).sum(-1))[p["masks"]]
    assert n.min() < 1e-2 and n.max() > 1e2                          # |d| far from 1, both ways
    with _routes(fast=fast, native=fast):
        got = _sh_hip(ops, p)
    _judge_sh(f"deg {deg} K {k_total} {'compiled' if fast else 'ctypes'}", got, p, k_sh)


@pytest.mark.parametrize("mask_kind", SH.MASK_KINDS)
@pytest.mark.parametrize("shape", SH.SHAPES, ids=[str(s) for s in SH.SHAPES])
def test_sh_backward_rows_shapes_and_masks(ops, k_sh, shape, mask_kind):
    for deg, kt in ((3, 16), (4, 27)):
        p = SH.make_inputs(deg, kt, shape, mask_kind)
        for fast in (True, False):
            with _routes(fast=fast, native=fast):
                got = _sh_hip(ops, p)
            assert got["dirs"].shape == p["dirs"].shape and got["coeffs"].shape == p["coeffs"].shape
            _judge_sh(f"deg {deg} K {kt} {shape} masks {mask_kind} {'compiled' if fast else 'ctypes'}", got, p, k_sh)
            if mask_kind == "all_false":
                assert not got["coeffs"].any() and not got["dirs"].any()


@pytest.mark.parametrize("fast", [True, False], ids=["compiled", "ctypes"])
def test_sh_backward_rows_without_v_dirs_and_with_a_strided_upstream(ops, k_sh, fast):
    for deg, kt in ((2, 11), (4, 28)):
        p = SH.make_inputs(deg, kt, (2, 1000), "random")
        with _routes(fast=fast, native=fast):
            no_dirs = _sh_hip(ops, p, dirs_grad=False)
            strided = _sh_hip(ops, p, strided_v=True)
            plain = _sh_hip(ops, p)
        assert no_dirs["dirs"] is None
        _judge_sh(f"deg {deg} K {kt} dirs frozen", no_dirs, p, k_sh)
        _judge_sh(f"deg {deg} K {kt} strided v_colors", strided, p, k_sh)
        np.testing.assert_array_equal(no_dirs["coeffs"], plain["coeffs"])
        np.testing.assert_array_equal(strided["coeffs"], plain["coeffs"])
        np.testing.assert_array_equal(strided["dirs"], plain["dirs"])


# =============================================================================================
# D  projection backward with several cameras
# =============================================================================================
PROJ_W, PROJ_H = 320, 200
PROJ_GROUPS = ("means2d_x", "means2d_y", "depths", "conic_a", "conic_b", "conic_c", "compensation")
BLOCKS = ((0, 3, "means"), (3, 7, "quats"), (7, 10, "scales"))


def _proj_cameras():
    cams = [make_camera(PROJ_W, PROJ_H, 350.0, 350.0, yaw=0.1),
            make_camera(PROJ_W, PROJ_H, 300.0, 330.0, yaw=-0.25, shift=(0.5, 0.1, -0.3)),
            make_camera(PROJ_W, PROJ_H, 420.0, 400.0, yaw=0.35, shift=(-0.4, -0.2, 0.6))]
    cams[1].K = cams[1].K.clone()
    cams[1].K[0, 2], cams[1].K[1, 2] = 0.42 * PROJ_W, 0.55 * PROJ_H          # principal point off centre
    return cams


def _proj_scene(n):
    if n == 1:
        g = torch.Generator().manual_seed(2)
        q = torch.randn(1, 4, generator=g)
        return torch.tensor([[0.1, 0.05, 5.0]]), (q / q.norm()).contiguous(), torch.tensor([[0.2, 0.05, 0.4]])
    sc = make_scene(n, seed=13, x_span=0.8, y_span=0.5, z_range=(1.0, 40.0), scale_range=(0.002, 0.5))      # needles included
    return sc.means, sc.quats, sc.scales


@pytest.fixture(scope="module")
def proj_refs():
    """{N: per-camera float64 autograd [7][C] x [N,10] with a unit upstream on one output, and the conditioning of every
    row from the reference's own forward}."""
    out = {}
    cams = _proj_cameras()
    for n in (403, 1):
        means, quats, scales = _proj_scene(n)
        per = [[None] * len(cams) for _ in PROJ_GROUPS]
        vis, kappa, kappa0, kcomp = (np.zeros((len(cams), n)) for _ in range(4))
        for c, cam in enumerate(cams):
            for gi in range(len(PROJ_GROUPS)):
                ref = [t.clone().double().requires_grad_(True) for t in (means, quats, scales)]
                radii, m2, dep, con, comp = OT.fully_fused_projection(ref[0], ref[1], ref[2], cam.viewmat.double(), cam.K.double(),
                                                                      PROJ_W, PROJ_H, near_plane=0.001, far_plane=1000.0)
                (m2[:, 0], m2[:, 1], dep, con[:, 0], con[:, 1], con[:, 2], comp)[gi].sum().backward()
                per[gi][c] = np.concatenate([r.grad.numpy() if r.grad is not None else np.zeros(tuple(r.shape)) for r in ref], axis=1)
            v = radii.numpy() > 0
            cn, cp = con.detach().numpy(), comp.detach().numpy()
            with np.errstate(all="ignore"):
                di = cn[:, 0] * cn[:, 2] - cn[:, 1] ** 2                     # 1 / det1
                a1, c1, bb = cn[:, 2] / di, cn[:, 0] / di, -cn[:, 1] / di
                det0 = np.maximum((a1 - 0.3) * (c1 - 0.3) - bb * bb, 1e-300)
                vis[c] = v
                kappa[c] = np.where(v, (cn[:, 0] + cn[:, 2]) ** 2 / di, 0.0)
                kappa0[c] = np.where(v, (a1 + c1 - 0.6) ** 2 / det0, 0.0)
                kcomp[c] = np.where(v, 1.0 / np.maximum(1.0 - cp ** 2, 1e-12), 0.0)
        out[n] = dict(inputs=(means, quats, scales), per=per, vis=vis.astype(bool), kappa=kappa.max(0),
                      kappa0=np.maximum(kappa, kappa0).max(0), kcomp=kcomp.max(0))
    return out


def _proj_tol(gi, r):
    """The per-row tolerances of test_projection_backward_one_output_at_a_time, the conditioning taken as the largest over
    the cameras in which the row is visible."""
    if gi < 3:
        return np.full(r["kappa"].shape, 2e-5)
    if gi < 6:
        return 1e-4 + 2e-6 * r["kappa"]
    return 1e-4 + 2e-6 * r["kappa0"] + 2e-6 * r["kcomp"]


def _proj_hip(ops, r, calc_comp, weights):
    """weights: [7] x ([C,N] | None) upstream gradient per output -> ([N,10] gradients, radii > 0)."""
    cams = _proj_cameras()
    V, K = torch.stack([c.viewmat for c in cams]).to(DEV), torch.stack([c.K for c in cams]).to(DEV)
    leaves = [t.clone().to(DEV).requires_grad_(True) for t in r["inputs"]]
    radii, m2, d, con, comp = ops.fully_fused_projection(leaves[0], None, leaves[1], leaves[2], V, K, PROJ_W, PROJ_H,
                                                         near_plane=0.001, far_plane=1000.0, calc_compensations=calc_comp)
    assert (comp is None) == (not calc_comp)
    outs = (m2[..., 0], m2[..., 1], d, con[..., 0], con[..., 1], con[..., 2], comp)
    loss = sum((o * _t(w)).sum() for o, w in zip(outs, weights) if w is not None and o is not None)
    loss.backward()
    torch.cuda.synchronize()
    return np.concatenate([_np(t.grad) for t in leaves], axis=1).astype(np.float64), _np(radii) > 0


@pytest.mark.parametrize("fast", [True, False], ids=["compiled", "ctypes"])
@pytest.mark.parametrize("calc_comp", [True, False], ids=["comp", "nocomp"])
@pytest.mark.parametrize("n", [403, 1])
def test_projection_backward_three_cameras_one_output_at_a_time(ops, proj_refs, n, calc_comp, fast):
    r = proj_refs[n]
    vis = r["vis"]
    C = vis.shape[0]
    if n == 403:
        assert all((vis[c] & ~vis[(c + 1) % C]).any() for c in range(C)) and (~vis.any(0)).sum() > 10 and (vis.sum(0) >= 2).sum() > 50
    else:
        assert vis.sum() >= 2
    seen = vis.any(0)
    worst = {}
    for gi, name in enumerate(PROJ_GROUPS):
        if gi == 6 and not calc_comp:
            continue                    # without compensations the output does not exist: its upstream is None in every run here
        weights = [np.ones((C, n), np.float32) if k == gi else None for k in range(7)]
        with _routes(fast=fast, native=fast):
            got, vis_hip = _proj_hip(ops, r, calc_comp, weights)
        np.testing.assert_array_equal(vis_hip, vis)
        assert np.isfinite(got).all(), name
        assert (got[~seen] == 0).all(), name                          # visible in no camera: exactly zero
        ref = sum(r["per"][gi])
        tol = _proj_tol(gi, r)
        for lo, hi, blk in BLOCKS:
            scale = sum(np.abs(pc[:, lo:hi]).max(axis=1) for pc in r["per"][gi])       # no cancellation between cameras
            live = seen & (scale > 1e-12 * max(1e-300, scale.max()))
            if not live.any():                                        # e.g. depth does not depend on quats / scales
                assert np.abs(got[:, lo:hi]).max() <= 1e-6 * max(1.0, np.abs(got).max()), (name, blk)
                continue
            rel = np.abs(got[live, lo:hi] - ref[live, lo:hi]).max(axis=1) / scale[live]
            if gi == 6:
                assert np.abs(got[:, lo:hi] - ref[:, lo:hi]).max() <= 1e-3 * scale.max(), (name, blk, "absolute")
            ratio = rel / tol[live]
            worst[(name, blk)] = float(ratio.max())
            assert ratio.max() < 1.0, (name, blk, float(rel.max()), float(r["kappa"][live][ratio.argmax()]))
    print(f"N {n} comp {calc_comp} {'compiled' if fast else 'ctypes'}: worst error / tolerance:", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("fast", [True, False], ids=["compiled", "ctypes"])
@pytest.mark.parametrize("calc_comp", [True, False], ids=["comp", "nocomp"])
def test_projection_backward_three_cameras_random_weights_on_all_outputs(ops, proj_refs, calc_comp, fast):
    """The gradient is linear in the upstream: under weights w the error of a row is at most
    sum_outputs tol_output sum_cameras |w| (largest entry of that camera's unit-upstream block) -- the bars of the test
    above, added up."""
    n = 403
    r = proj_refs[n]
    vis = r["vis"]
    C = vis.shape[0]
    rng = np.random.default_rng(17)
    weights = [rng.normal(size=(C, n)).astype(np.float32) for _ in range(7)]
    if not calc_comp:
        weights[6] = None
    with _routes(fast=fast, native=fast):
        got, vis_hip = _proj_hip(ops, r, calc_comp, weights)
    np.testing.assert_array_equal(vis_hip, vis)
    seen = vis.any(0)
    assert np.isfinite(got).all() and (got[~seen] == 0).all()
    ref = sum(w[c].astype(np.float64)[:, None] * r["per"][gi][c] for gi, w in enumerate(weights) if w is not None for c in range(C))
    worst = {}
    for lo, hi, blk in BLOCKS:
        bound = sum(_proj_tol(gi, r) * sum(np.abs(w[c].astype(np.float64)) * np.abs(r["per"][gi][c][:, lo:hi]).max(axis=1) for c in range(C))
                    for gi, w in enumerate(weights) if w is not None)
        err = np.abs(got[seen, lo:hi] - ref[seen, lo:hi]).max(axis=1)
        assert (bound[seen] > 0).all()
        worst[blk] = float((err / bound[seen]).max())
        assert worst[blk] < 1.0, (blk, worst[blk])
    print(f"random weights, comp {calc_comp} {'compiled' if fast else 'ctypes'}: worst error / bound:", {k: round(v, 3) for k, v in worst.items()})
