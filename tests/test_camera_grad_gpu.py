"""Camera gradients on the device: sc_projection_bwd_cam / sc_camera_centers_bwd and the routes into them, judged per
entry against tests/camera_grad_ref.py (float64 autograd with the view matrix as a leaf).

  operator   `fully_fused_projection` with `viewmats.requires_grad`: |v_viewmats - G| <= 2^-24 K S, 0 where S == 0,
             bottom row +0, over the sizes around the wave / block / reduction boundaries, C in {1, 3}, centred and
             off-centre principal points, both Jacobian clamp variants, with and without compensations; through the
             compiled binding layer and the ctypes table.
  entry      null per-Gaussian outputs, bit-equality with sc_projection_bwd, repeatability, exact zeros, poisoned culled
             rows, guard zones, no host wait.
  chain      `rasterization()` with cameras under grad, with and without `camera_centers_`, against the float64 chain; the
             same call's leaf gradients bit-equal to the call without camera grad; the composition by hand bit-equal.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import camera_grad_ref as CR                       # noqa: E402
from guard_arena import Arena                      # noqa: E402
from oracle import param_grad_f64 as PG            # noqa: E402
from oracle import poison_cases as PZ              # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from street_crafter_amd import _lib
    _lib.load()
    if _lib.fast() is None:
        pytest.fail("compiled binding layer not loaded")
    import gsplat.rendering as R
    return R


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import _lib
    return _lib.load()


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int32)


@contextlib.contextmanager
def _routes(fast=True, native=True, proj_clamp="symmetric"):
    from street_crafter_amd import _lib, rendering
    prev_fast = _lib.set_fast_binding(fast)
    prev_native = rendering.set_native_autograd(native)
    prev_clamp = _lib.set_projection_variant(proj_clamp=proj_clamp)[0]
    try:
        assert (_lib.fast() is not None) == fast
        yield
    finally:
        _lib.set_projection_variant(proj_clamp=prev_clamp)
        rendering.set_native_autograd(prev_native)
        _lib.set_fast_binding(prev_fast)


def _upstream(inp, cams):
    u = inp["u"]
    pick = lambda k: _t(u[k][cams])
    v_m2 = torch.stack([pick(0), pick(1)], dim=-1).contiguous()
    v_con = torch.stack([pick(3), pick(4), pick(5)], dim=-1).contiguous()
    return v_m2, pick(2), v_con, (pick(6) if u[6] is not None else None)


def _assert_bottom_row_plus_zero(v):
    assert bool((_bits(v[:, 3, :]) == 0).all()), "bottom row of v_viewmats is not +0"


# =============================================================================================
# the operator against the bar
# =============================================================================================
CAM_SETS = {"all3": [0, 1, 2], "second": [1], "first": [0]}
OPERATOR_RUNS = ([(n, cs) for n in CR.OPERATOR_CASES if not n.startswith("clamped") for cs in ("all3", "second")]
                 + [("n513", "first"), ("clamped_symmetric", "first"), ("clamped_asymmetric", "first")])


def _operator_grad(ops, inp, cams, leaves_grad):
    """`fully_fused_projection` under the case's upstream -> (viewmats.grad, leaves)."""
    L = [_t(inp[k]).requires_grad_(leaves_grad) for k in ("means", "quats", "scales")]
    V, K = _t(inp["V"][cams]).requires_grad_(True), _t(inp["K"][cams])
    radii, m2, d, con, comp = ops.fully_fused_projection(L[0], None, L[1], L[2], V, K, inp["width"], inp["height"],
                                                         eps2d=inp["eps2d"], near_plane=inp["near"], far_plane=inp["far"],
                                                         calc_compensations=inp["comp"])
    np.testing.assert_array_equal(_np(radii), inp["radii"][cams])
    assert m2._sc_viewmats.grad_fn is None and not m2._sc_viewmats.requires_grad        # no graph kept alive through means2d
    v_m2, v_d, v_con, v_comp = _upstream(inp, cams)
    outs, ups = [m2, d, con], [v_m2, v_d, v_con]
    if inp["comp"]:
        outs.append(comp)
        ups.append(v_comp)
    torch.autograd.backward(outs, ups)
    torch.cuda.synchronize()
    return V.grad, L


@pytest.mark.parametrize("fast", [True, False], ids=["compiled", "ctypes"])
@pytest.mark.parametrize("name,cam_set", OPERATOR_RUNS, ids=[f"{n}-{c}" for n, c in OPERATOR_RUNS])
def test_operator_viewmats_grad_against_the_float64_bar(ops, name, cam_set, fast):
    inp, ref, K = CR.operator_inputs(name), CR.operator_reference(name), CR.operator_k()
    cams = CAM_SETS[cam_set]
    assert (inp["radii"][cams] > 0).any()
    with _routes(fast=fast, native=fast, proj_clamp=inp["proj_clamp"]):
        got, L = _operator_grad(ops, inp, cams, leaves_grad=(len(name) % 2 == 0))
    assert got is not None and got.shape == (len(cams), 4, 4), "viewmats.grad is missing"
    _assert_bottom_row_plus_zero(got)
    ratio, off = CR.worst_ratio(_np(got), ref["G"][cams], ref["S"][cams])
    print(f"[hip] {name} {cam_set} {'compiled' if fast else 'ctypes'}: worst ratio {ratio:.2f}; bar {K:.1f} (replay {ref['k_ref']:.2f})")
    assert off == 0.0 and ratio <= K, (name, cam_set, ratio, K, off)
    if name.startswith("clamped"):
        assert PG.clamp_limit_margin(PG.make_case("clamped"))[1] > 50         # the scene does reach beyond the clamp limit


# =============================================================================================
# the entry itself
# =============================================================================================
class _Call:
    """One set of device buffers for sc_projection_bwd / sc_projection_bwd_cam of an operator case."""

    def __init__(self, lib, inp, cams, leaves=None, nan_upstream_rows=None):
        self.lib, self.inp = lib, inp
        src = inp if leaves is None else leaves
        self.means, self.quats, self.scales = (_t(src[k]) for k in ("means", "quats", "scales"))
        self.V, self.K = _t(inp["V"][cams]), _t(inp["K"][cams])
        self.C, self.N = len(cams), self.means.shape[0]
        C, N = self.C, self.N
        self.radii = torch.empty((C, N), dtype=torch.int32, device=DEV)
        self.conics = torch.empty((C, N, 3), device=DEV)
        self.comps = torch.empty((C, N), device=DEV) if inp["comp"] else None
        m2, d = torch.empty((C, N, 2), device=DEV), torch.empty((C, N), device=DEV)
        rc = lib.sc_projection_fwd(_p(self.means), _p(self.quats), _p(self.scales), _p(self.V), _p(self.K), C, N, inp["width"],
                                   inp["height"], inp["eps2d"], inp["near"], inp["far"], 0.0, _p(self.radii), _p(m2), _p(d),
                                   _p(self.conics), _p(self.comps), _st())
        assert rc == 0, rc
        self.up = list(_upstream(inp, cams))
        if nan_upstream_rows is not None:
            for t in self.up:
                if t is not None:
                    t[:, nan_upstream_rows] = float("nan")

    def _args(self):
        i = self.inp
        v_m2, v_d, v_con, v_comp = self.up
        return (_p(self.means), _p(self.quats), _p(self.scales), _p(self.V), _p(self.K), self.C, self.N, i["width"], i["height"],
                i["eps2d"], _p(self.radii), _p(self.conics), _p(self.comps), _p(v_m2), _p(v_d), _p(v_con),
                _p(v_comp if self.comps is not None else None))

    def plain(self):
        out = [torch.full((self.N, k), float("nan"), device=DEV) for k in (3, 4, 3)]
        rc = self.lib.sc_projection_bwd(*self._args(), *(_p(o) for o in out), _st())
        assert rc == 0, rc
        return out

    def cam(self, want=(True, True, True)):
        out = [torch.full((self.N, k), float("nan"), device=DEV) if w else None for k, w in zip((3, 4, 3), want)]
        vV = torch.full((self.C, 4, 4), float("nan"), device=DEV)
        nbytes = self.lib.sc_projection_bwd_cam_workspace_bytes(self.C, self.N)
        assert nbytes == self.C * ((self.N + 255) // 256) * 48 + 40 * self.N
        ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=DEV)          # NaN bit patterns
        rc = self.lib.sc_projection_bwd_cam(*self._args(), *(_p(o) for o in out), _p(vV), _p(ws), _st())
        assert rc == 0, rc
        torch.cuda.synchronize()
        return out, vV


@pytest.mark.parametrize("name", ["n257", "n513_nocomp", "n65", "clamped_asymmetric"])
def test_null_outputs_and_bit_equality_with_projection_bwd(lib, name):
    inp = CR.operator_inputs(name)
    cams = [0] if name.startswith("clamped") else [0, 1, 2]
    with _routes(proj_clamp=inp["proj_clamp"]):
        call = _Call(lib, inp, cams)
        np.testing.assert_array_equal(_np(call.radii), inp["radii"][cams])
        want = call.plain()
        full, vV = call.cam()
        none, vV_none = call.cam((False, False, False))
        only_means, vV_means = call.cam((True, False, False))
        only_qs, vV_qs = call.cam((False, True, True))
    for a, b, what in zip(want, full, ("v_means", "v_quats", "v_scales")):
        assert torch.equal(_bits(a), _bits(b)), f"{what} differs from sc_projection_bwd's"
    assert torch.isfinite(vV).all() and none == [None, None, None]
    for other in (vV_none, vV_means, vV_qs):
        assert torch.equal(_bits(vV), _bits(other)), "v_viewmats depends on which per-Gaussian outputs were asked for"
    assert torch.equal(_bits(only_means[0]), _bits(want[0])) and only_means[1] is None and only_means[2] is None
    assert torch.equal(_bits(only_qs[1]), _bits(want[1])) and torch.equal(_bits(only_qs[2]), _bits(want[2]))
    ref = CR.operator_reference(name)
    ratio, off = CR.worst_ratio(_np(vV), ref["G"][cams], ref["S"][cams])
    assert off == 0.0 and ratio <= CR.operator_k(), (ratio, off)


def test_repeatable_and_exact_zeros(lib):
    from street_crafter_amd.scenes import make_camera
    inp = CR.operator_inputs(f"n{CR.BIG_N}")
    call = _Call(lib, inp, [0, 1, 2])
    (_, a), (_, b) = call.cam(), call.cam((False, False, False))
    (_, c) = call.cam()
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c)) and bool((a[:, :3] != 0).all())
    _assert_bottom_row_plus_zero(a)
    # a camera that sees nothing (it looks the other way) between two that do
    small = dict(CR.operator_inputs("n513"))
    away = make_camera(CR.W0, CR.H0, 350.0, 350.0, yaw=math.pi)
    small["V"] = np.stack([small["V"][0], away.viewmat.numpy(), small["V"][2]])
    small["K"] = np.stack([small["K"][0], away.K.numpy(), small["K"][2]])
    call = _Call(lib, small, [0, 1, 2])
    assert not bool((call.radii[1] > 0).any()) and bool((call.radii[0] > 0).any())
    _, vV = call.cam()
    assert bool((_bits(vV[1]) == 0).all()) and bool((vV[0, :3] != 0).all()) and bool((vV[2, :3] != 0).all())
    # every row culled: behind all three cameras
    behind = dict(CR.operator_inputs("n513"))
    behind["means"] = behind["means"] * np.float32([1.0, 1.0, -1.0]) - np.float32([0.0, 0.0, 5.0])
    call = _Call(lib, behind, [0, 1, 2])
    assert not bool((call.radii > 0).any())
    out, vV = call.cam()
    assert bool((_bits(vV) == 0).all()) and all(bool((_bits(o) == 0).all()) for o in out)
    # N == 0: the cameras' rows are still written
    for C in (1, 3):
        vV = torch.full((C, 4, 4), float("nan"), device=DEV)
        assert lib.sc_projection_bwd_cam_workspace_bytes(C, 0) == 0
        rc = lib.sc_projection_bwd_cam(None, None, None, _p(call.V), _p(call.K), C, 0, CR.W0, CR.H0, 0.3, None, None, None, None,
                                       None, None, None, None, None, None, _p(vV), None, _st())
        torch.cuda.synchronize()
        assert rc == 0 and bool((_bits(vV) == 0).all())


def test_poisoned_culled_rows_leave_no_trace(lib):
    """Rows with NaN / inf leaves that the projection culls (oracle/poison_cases.py's `culled` recipes that hold under
    every camera), their upstream rows NaN as well: v_viewmats and every other row's gradients are the benign twin's bits."""
    inp = CR.operator_inputs("n513")
    cams = [0, 1, 2]
    recipes = [r for r in PZ.camera_free() if r.cls == "culled"]
    slots = [0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256, 257, 300, 383, 384, 511, 512][:len(recipes)]
    assert len(slots) == len(recipes) >= 19
    rows = PZ.rows(recipes, 1)
    poisoned = {k: inp[k].copy() for k in ("means", "quats", "scales")}
    twin = {k: inp[k].copy() for k in ("means", "quats", "scales")}
    for i, s in enumerate(slots):
        for k in poisoned:
            poisoned[k][s] = rows[k][i]
        twin["means"][s], twin["quats"][s], twin["scales"][s] = PZ.TWIN_MEAN, PZ.UNIT, PZ.SCALE
    for c in cams:       # the oracle classes every recipe (and the twin row) as culled under these cameras
        cam = CR.operator_cameras()[c]
        cam.znear, cam.zfar = inp["near"], inp["far"]
        assert set(PZ.classes(recipes, cam, inp["width"], inp["height"]).values()) == {"culled"}
    a = _Call(lib, inp, cams, leaves=poisoned, nan_upstream_rows=slots)
    b = _Call(lib, inp, cams, leaves=twin)
    assert not bool((a.radii[:, slots] > 0).any()) and not bool((b.radii[:, slots] > 0).any())
    assert torch.equal(a.radii, b.radii) and bool((a.radii > 0).any(1).all())
    (ga, va), (gb, vb) = a.cam(), b.cam()
    assert torch.isfinite(va).all() and torch.equal(_bits(va), _bits(vb))
    _, va_none = a.cam((False, False, False))
    assert torch.equal(_bits(va_none), _bits(vb))
    for x, y in zip(ga, gb):
        assert torch.equal(_bits(x), _bits(y)) and bool((_bits(x[slots]) == 0).all())


@pytest.mark.parametrize("name", ["n1", "n257", "n513_nocomp"])
def test_guard_zones_around_every_buffer(lib, name):
    """Both entries with every buffer cut from one arena, the workspace at exactly the size the library asks for, under two
    fills: no guard byte changes, no input changes, and the outputs are the same bits under both fills."""
    inp = CR.operator_inputs(name)
    cams = [0, 1, 2]
    call = _Call(lib, inp, cams)
    C, N = call.C, call.N
    v_m2, v_d, v_con, v_comp = call.up
    ins = dict(means=call.means, quats=call.quats, scales=call.scales, V=call.V, K=call.K, radii=call.radii, conics=call.conics,
               v_m2=v_m2, v_d=v_d, v_con=v_con, v_centers=_t(np.random.default_rng(3).normal(size=(C, 3))))
    if call.comps is not None:
        ins.update(comps=call.comps, v_comp=v_comp)
    outs = dict(v_means=12 * N, v_quats=16 * N, v_scales=12 * N, v_viewmats=64 * C, v_quats_alone=16 * N, v_viewmats_2=64 * C,
                v_viewmats_centres=64 * C, workspace=lib.sc_projection_bwd_cam_workspace_bytes(C, N))
    partial_words = C * ((N + 255) // 256) * 12
    res = {}
    for fill in (0xA5, 0x3F):
        sizes = {k: v.numel() * v.element_size() for k, v in ins.items()}
        sizes.update(outs)
        ar = Arena(sizes, DEV, fill=fill)
        for k, v in ins.items():
            ar.view(k).copy_(v.contiguous().view(torch.uint8).reshape(-1))
        comp = (ar.ptr("comps"), ar.ptr("v_comp")) if call.comps is not None else (None, None)
        # all three per-Gaussian outputs, then v_quats alone (the other two land in the workspace's spare rows)
        for want in ((ar.ptr("v_means"), ar.ptr("v_quats"), ar.ptr("v_scales"), ar.ptr("v_viewmats")),
                     (None, ar.ptr("v_quats_alone"), None, ar.ptr("v_viewmats_2"))):
            rc = lib.sc_projection_bwd_cam(ar.ptr("means"), ar.ptr("quats"), ar.ptr("scales"), ar.ptr("V"), ar.ptr("K"), C, N,
                                           inp["width"], inp["height"], inp["eps2d"], ar.ptr("radii"), ar.ptr("conics"), comp[0],
                                           ar.ptr("v_m2"), ar.ptr("v_d"), ar.ptr("v_con"), comp[1], *want, ar.ptr("workspace"), _st())
            assert rc == 0, rc
        rc = lib.sc_camera_centers_bwd(ar.ptr("V"), ar.ptr("v_centers"), C, ar.ptr("v_viewmats_centres"), _st())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert ar.broken_guards() == [], (fill, ar.broken_guards(), ar.span)
        for k, v in ins.items():
            assert torch.equal(ar.view(k), v.contiguous().view(torch.uint8).reshape(-1)), f"input {k} was written"
        res[fill] = {k: ar.view(k, torch.int32).clone() for k in outs}
        res[fill]["workspace"] = res[fill]["workspace"][:partial_words]      # every partial row is written before it is read
    for k in outs:
        assert torch.equal(res[0xA5][k], res[0x3F][k]), f"{k} differs between the fills"
    assert torch.equal(res[0xA5]["v_quats"], res[0xA5]["v_quats_alone"]) and torch.equal(res[0xA5]["v_viewmats"], res[0xA5]["v_viewmats_2"])
    _, vV = call.cam()
    assert torch.equal(res[0xA5]["v_viewmats"].view(C, 4, 4), _bits(vV))


def test_camera_centers_backward(ops):
    """VJP of c = -R^T t against float64: v_t = -R v_c (three products deep), v_R = -t v_c^T (one product); bottom row +0;
    no graph without grad."""
    from street_crafter_amd.rendering import camera_centers
    rng = np.random.default_rng(11)
    for C in (1, 3, 65):
        V64 = np.tile(np.eye(4), (C, 1, 1))
        q, _ = np.linalg.qr(rng.normal(size=(C, 3, 3)))
        V64[:, :3, :3], V64[:, :3, 3] = q, rng.normal(size=(C, 3)) * 5
        V = _t(V64).requires_grad_(True)
        g = _t(rng.normal(size=(C, 3)))
        ctr = camera_centers(V)
        assert ctr.requires_grad
        ctr.backward(g)
        torch.cuda.synchronize()
        Vf, gf = _np(V).astype(np.float64), _np(g).astype(np.float64)
        want = np.zeros((C, 4, 4))
        want[:, :3, :3] = -Vf[:, :3, 3, None] * gf[:, None, :]
        want[:, :3, 3] = -np.einsum("cij,cj->ci", Vf[:, :3, :3], gf)
        mag = np.zeros((C, 4, 4))
        mag[:, :3, :3] = np.abs(want[:, :3, :3])
        mag[:, :3, 3] = np.einsum("cij,cj->ci", np.abs(Vf[:, :3, :3]), np.abs(gf))
        assert (np.abs(_np(V.grad) - want) <= 4 * 2.0 ** -24 * mag).all()
        _assert_bottom_row_plus_zero(V.grad)
        with torch.no_grad():
            assert camera_centers(V).grad_fn is None
        plain = camera_centers(V.detach())
        assert plain.grad_fn is None and torch.equal(plain, ctr.detach())


def test_no_host_wait(ops):
    """Projection forward + the camera backward and camera_centers + its backward are enqueued behind 200 passes over
    256 MB and return while that work is still running (tests/test_actor_pose_gpu.py's check)."""
    from street_crafter_amd.rendering import camera_centers
    inp = CR.operator_inputs("n513")
    cams = [0, 1, 2]

    dev = [_t(inp[k]) for k in ("means", "quats", "scales")] + [_t(inp["V"][cams]), _t(inp["K"][cams])]

    def step():
        L = [t.detach().requires_grad_(True) for t in dev[:3]]
        V, K = dev[3].detach().requires_grad_(True), dev[4]
        radii, m2, d, con, comp = ops.fully_fused_projection(L[0], None, L[1], L[2], V, K, inp["width"], inp["height"],
                                                             near_plane=inp["near"], far_plane=inp["far"], calc_compensations=True)
        ctr = camera_centers(V)
        torch.autograd.backward([m2, d, con, comp, ctr], [*ups, g_ctr])
        return V, L

    ups = list(_upstream(inp, cams))
    g_ctr = torch.ones(3, 3, device=DEV)
    step()                                                              # warm-up: everything loaded
    big = torch.ones(64 * 1024 * 1024, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        front = torch.cuda.Event()
        for _ in range(200):
            big.mul_(1.0001)
        front.record()
        V, L = step()
        pending = not front.query()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert pending, "the work in front had finished when forward + backward returned: something in them waited for the GPU"
    assert torch.isfinite(V.grad).all() and all(torch.isfinite(x.grad).all() for x in L)


def test_argument_checks_on_the_device_side(lib):
    v = torch.zeros(1, 4, 4, device=DEV)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    big = [_p(ws)] * 5
    # a workspace that is not 16-byte aligned is refused before any launch
    assert lib.sc_projection_bwd_cam(*big, 1, 1, 8, 8, 0.3, *([_p(ws)] * 2), None, *([_p(ws)] * 3), None, None, None, None, _p(v),
                                     _p(ws) + 4, _st()) == -1


# =============================================================================================
# the whole chain
# =============================================================================================
def _leaves(p, grad=True):
    return {k: _t(p[k]).requires_grad_(grad and k not in p["frozen"]) for k in PG.LEAVES}


def _loss(p, rgb, acc, depth):
    return (rgb * _t(p["w_rgb"])).sum() + (acc * _t(p["w_acc"])).sum() + (depth * _t(p["w_depth"])).sum()


def _cameras(p, grad):
    cams = p["cameras"]
    return (torch.stack([c.viewmat for c in cams]).to(DEV).requires_grad_(grad), torch.stack([c.K for c in cams]).to(DEV),
            torch.stack([c.camera_center for c in cams]).to(DEV))


def _check_lists(p, radii, offs, fids):
    fids = fids.plain() if hasattr(fids, "plain") else fids
    np.testing.assert_array_equal(_np(radii), p["radii"])
    np.testing.assert_array_equal(_np(offs), p["isect_offsets"])
    np.testing.assert_array_equal(_np(fids), p["flatten_ids"])


def _step_rasterization(ops, p, cam_grad, own_centers, boundary_upstream=None):
    """boundary_upstream: instead of the loss, given gradients on the rasterizer's four inputs (everything below them is
    free of atomics, so the leaves' gradients are the same bits from run to run)."""
    L = _leaves(p)
    V, K, ctr = _cameras(p, cam_grad)
    cam = p["cameras"][0]
    rc, ra, meta = ops.rasterization(L["means"], L["quats"], L["scales"], L["opacities"].reshape(-1), L["sh"], V, K, p["width"],
                                     p["height"], near_plane=cam.znear, far_plane=cam.zfar, sh_degree=p["sh_degree"],
                                     render_mode="RGB+ED", absgrad=True,
                                     rasterize_mode="antialiased" if p["antialiasing"] else "classic",
                                     camera_centers_=None if own_centers else ctr)
    assert not meta["fused"]
    _check_lists(p, meta["radii"], meta["isect_offsets"], meta["flatten_ids"])
    if boundary_upstream is None:
        _loss(p, rc[..., :3], ra[..., 0], rc[..., 3]).backward()
    else:
        outs = [meta[k] for k in ("means2d", "conics", "colors", "opacities")]
        torch.autograd.backward(outs, [u.reshape(o.shape) for u, o in zip(boundary_upstream, outs)])
    torch.cuda.synchronize()
    return L, V


def _step_by_hand(ops, p, own_centers, boundary_upstream=None):
    """projection, camera_centers, spherical_harmonics, rasterizer: the composition spelt out."""
    from street_crafter_amd.rendering import camera_centers
    L = _leaves(p)
    V, K, ctr = _cameras(p, True)
    C, W, H, ts = V.shape[0], p["width"], p["height"], p["tile_size"]
    cam = p["cameras"][0]
    radii, m2, d, con, comp = ops.fully_fused_projection(L["means"], None, L["quats"], L["scales"], V, K, W, H, packed=False,
                                                         near_plane=cam.znear, far_plane=cam.zfar,
                                                         calc_compensations=p["antialiasing"])
    op = L["opacities"].reshape(1, -1).expand(C, -1)
    if comp is not None:
        op = op * comp
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    _, ids, fids = ops.isect_tiles(m2, radii, d, ts, tw, th, packed=False, n_cameras=C)
    offs = ops.isect_offset_encode(ids, C, tw, th)
    _check_lists(p, radii, offs, fids)
    campos = camera_centers(V) if own_centers else ctr
    dirs = L["means"][None] - campos[:, None, :]
    cols = ops.spherical_harmonics(p["sh_degree"], dirs, L["sh"][None].expand(C, -1, -1, -1), masks=radii > 0)
    cols = torch.cat([torch.clamp_min(cols + 0.5, 0.0), d[..., None]], dim=-1)
    if boundary_upstream is not None:
        outs = [m2, con, cols, op]
        torch.autograd.backward(outs, [u.reshape(o.shape) for u, o in zip(boundary_upstream, outs)])
        torch.cuda.synchronize()
        return L, V
    rc, ra = ops.rasterize_to_pixels(m2, con, cols.contiguous(), op.contiguous(), W, H, ts, offs, fids, backgrounds=None,
                                     packed=False, absgrad=True)
    rc = torch.cat([rc[..., :-1], rc[..., -1:] / ra.clamp(min=1e-10)], dim=-1)
    _loss(p, rc[..., :3], ra[..., 0], rc[..., 3]).backward()
    torch.cuda.synchronize()
    return L, V


@pytest.mark.parametrize("own_centers", [False, True], ids=["camera_centers_", "derived"])
@pytest.mark.parametrize("case_id", CR.CHAIN_CASES)
def test_rasterization_delivers_viewmats_grad(ops, case_id, own_centers):
    """`rasterization()` with `viewmats.requires_grad`, per entry against the float64 chain.  Without `camera_centers_`
    the centres are camera_centers(viewmats), -R^T t in float32, within 4 x 2^-24 sum|R||t| of the stored ones
    (tests/test_param_grad_rows_gpu.py): the tile lists do not depend on them and the clamp decisions of the colours are
    more than PG.CLAMP_WINDOW away from flipping, so the facts of the case hold for both.
    The leaves' gradients of the same call are the bits of the call without camera grad wherever a call's gradients are
    the same bits twice in a row at all: the same kernels on the same inputs (sc_projection_bwd_cam's per-Gaussian rows
    ARE sc_projection_bwd's), accumulated by autograd in the same order.  From the loss they are not -- the rasterizer's
    backward accumulates with float atomics in arbitrary order, two identical calls without camera grad already differ --
    so the equality is asserted from given upstream gradients on the rasterizer's inputs, below which nothing is atomic, and
    from the loss only if the call without camera grad repeats itself."""
    r, K = CR.chain_reference(case_id), CR.chain_k()
    p = r["p"]
    mode = "derived" if own_centers else "constant"
    vis = p["radii"] > 0
    assert np.abs(p["colors_pre_clamp"][vis]).min() > PG.CLAMP_WINDOW
    with _routes():
        L, V = _step_rasterization(ops, p, True, own_centers)
        L0, V0 = _step_rasterization(ops, p, False, own_centers)
    assert V.grad is not None and V0.grad is None, "viewmats.grad is missing"
    _assert_bottom_row_plus_zero(V.grad)
    ratio, off = CR.worst_ratio(_np(V.grad), r["G"][mode], r["S"][mode], r["A"][mode])
    print(f"[hip] {case_id} {mode}: worst ratio {ratio:.2f}; bar {K:.1f} (replay {r['k_ref']:.2f})")
    assert off == 0.0 and ratio <= K, (case_id, mode, ratio, K, off)
    if case_id in CR.CENTRE_DETACHED_CAUGHT:      # the direction path shows through the bar: the other mode's reference is out of reach
        other = "constant" if own_centers else "derived"
        assert CR.worst_ratio(_np(V.grad), r["G"][other], r["S"][other], r["A"][other])[0] > K
    C, N = p["radii"].shape
    g = torch.Generator(device=DEV).manual_seed(7)
    ups = [torch.randn((C, N, k), device=DEV, generator=g) for k in (2, 3, 4, 1)]
    with _routes():
        L0b, _ = _step_rasterization(ops, p, False, own_centers)
        Lu, Vu = _step_rasterization(ops, p, True, own_centers, ups)
        Lu0, _ = _step_rasterization(ops, p, False, own_centers, ups)
    assert Vu.grad is not None and torch.isfinite(Vu.grad).all()
    repeats = all(L0[k].grad is None or torch.equal(_bits(L0[k].grad), _bits(L0b[k].grad)) for k in PG.LEAVES)
    print(f"[hip] {case_id} {mode}: two calls without camera grad give {'the same' if repeats else 'different'} leaf gradients from the loss")
    for k in PG.LEAVES:
        assert (L[k].grad is None) == (L0[k].grad is None) == (k in p["frozen"])
        if L[k].grad is not None:
            assert torch.equal(_bits(Lu[k].grad), _bits(Lu0[k].grad)), f"{k}.grad changes when the cameras require grad"
            if repeats:
                assert torch.equal(_bits(L[k].grad), _bits(L0[k].grad)), f"{k}.grad changes when the cameras require grad"


@pytest.mark.parametrize("own_centers", [False, True], ids=["camera_centers_", "derived"])
def test_composition_by_hand_gives_the_same_bits(ops, own_centers):
    """projection, camera_centers, spherical_harmonics, rasterizer by hand against `rasterization()`: the same bits in
    viewmats.grad and in every leaf from given upstream gradients on the rasterizer's inputs (its backward adds with float
    atomics: from the loss no call repeats itself bit for bit), and within the float64 bar from the loss."""
    r, K = CR.chain_reference("two_cameras"), CR.chain_k()
    p = r["p"]
    mode = "derived" if own_centers else "constant"
    C, N = p["radii"].shape
    g = torch.Generator(device=DEV).manual_seed(9)
    ups = [torch.randn((C, N, k), device=DEV, generator=g) for k in (2, 3, 4, 1)]
    for native in (True, False):
        with _routes(native=native):
            L, V = _step_rasterization(ops, p, True, own_centers, ups)
            Lh, Vh = _step_by_hand(ops, p, own_centers, ups)
            _, Vl = _step_by_hand(ops, p, own_centers)
        assert torch.equal(_bits(V.grad), _bits(Vh.grad)) and bool((V.grad[:, :3] != 0).all())
        for k in PG.LEAVES:
            assert torch.equal(_bits(L[k].grad), _bits(Lh[k].grad)), k
        ratio, off = CR.worst_ratio(_np(Vl.grad), r["G"][mode], r["S"][mode], r["A"][mode])
        assert off == 0.0 and ratio <= K, (mode, native, ratio, K, off)


def test_camera_centers_given_under_grad_get_their_gradient(ops):
    """A `camera_centers_` that itself requires grad receives dL/dcentre from autograd through dirs; judged against the
    float64 chain's centre gradient through the identity derived = constant + centre_vjp (both within their bars)."""
    r = CR.chain_reference("plain")
    p = r["p"]
    L = _leaves(p)
    V, K, ctr = _cameras(p, True)
    ctr.requires_grad_(True)
    cam = p["cameras"][0]
    with _routes():
        rc, ra, meta = ops.rasterization(L["means"], L["quats"], L["scales"], L["opacities"].reshape(-1), L["sh"], V, K,
                                         p["width"], p["height"], near_plane=cam.znear, far_plane=cam.zfar,
                                         sh_degree=p["sh_degree"], render_mode="RGB+ED", rasterize_mode="antialiased",
                                         camera_centers_=ctr)
        _loss(p, rc[..., :3], ra[..., 0], rc[..., 3]).backward()
    torch.cuda.synchronize()
    assert ctr.grad is not None and torch.isfinite(ctr.grad).all() and bool((ctr.grad != 0).all())
    both = V.grad.double().cpu()[:, :3, :] + torch.stack([CR.centre_vjp(V.detach().double().cpu()[c], ctr.grad.double().cpu()[c])
                                                          for c in range(V.shape[0])])
    ratio, off = CR.worst_ratio(both.numpy(), r["G"]["derived"], r["S"]["derived"], r["A"]["derived"])
    assert off == 0.0 and ratio <= CR.chain_k(), (ratio, off)
