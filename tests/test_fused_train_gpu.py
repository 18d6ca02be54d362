"""Training through `rasterization()` with the per-Gaussian part as ONE forward and ONE backward kernel
(rendering.set_fused_training / SC_FUSED_TRAIN, csrc/fused_bwd.hip), judged like the composition it replaces:

1  end to end, every case of oracle/param_grad_f64.py: every leaf gradient and meta["means2d"].grad per row against the
   float64 chain, |hip - G| <= 2^-24 (K S + A), exactly 0 where S == 0, K = 4 K_ref of the float32 replay (the bar and
   the K of tests/test_param_grad_rows_gpu.py), on the tile lists the numpy oracle built;
2  the forward is the composition's bit for bit;
3  the new autograd node alone, under fixed upstream gradients, against the float64 per-Gaussian Jacobians
   (PG.carry): |hip - G| <= 2^-24 K_A S, K_A = 4 x what the float32 torch replay of the same sub-chain reaches; and
   what must hold bit for bit: run-to-run, frozen leaves, a prefix of the Gaussians on its own, padded SH rows, NaN in
   the upstream rows of culled (camera, Gaussian) pairs;
4  which calls take the route.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import param_grad_f64 as PG            # noqa: E402  (checker only)
from oracle import raster_bwd_cases as RC          # noqa: E402
from oracle import raster_bwd_f64 as RB            # noqa: E402

DEV = "cuda"
NODE_CASES = ("plain", "two_cameras")


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
    """ctypes table or compiled binding layer, Python or compiled autograd functions, and the fused training switch."""

    def __init__(self, fast=True, native=True, fused=True):
        self.want = (fast, native, fused)

    def __enter__(self):
        from street_crafter_amd import _lib, rendering
        fast, native, fused = self.want
        self.undo = []          # one entry per setting actually changed: whatever fails below, the session gets them back
        try:
            prev = _lib.set_fast_binding(fast)
            self.undo.append(lambda: _lib.set_fast_binding(prev))
            prev_native = rendering.set_native_autograd(native)
            self.undo.append(lambda: rendering.set_native_autograd(prev_native))
            prev_fused = rendering.set_fused_training(fused)
            self.undo.append(lambda: rendering.set_fused_training(prev_fused))
            assert (_lib.fast() is not None) == fast
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        while self.undo:
            self.undo.pop()()
        return False


@pytest.fixture(scope="module")
def refs():
    """{case: (inputs, float64 reference)} and K: ONE number for the module, as in tests/test_param_grad_rows_gpu.py."""
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


def _leaves(p, frozen=None):
    frozen = p["frozen"] if frozen is None else frozen
    return {k: _t(p[k]).requires_grad_(k not in frozen) for k in PG.LEAVES}


def _loss(p, rgb, acc, depth):
    """rgb [C,H,W,3], acc [C,H,W], depth [C,H,W] under the case's weights."""
    return (rgb * _t(p["w_rgb"])).sum() + (acc * _t(p["w_acc"])).sum() + (depth * _t(p["w_depth"])).sum()


def _check_lists(p, radii, offs, fids):
    fids = fids.plain() if hasattr(fids, "plain") else fids
    np.testing.assert_array_equal(_np(radii), p["radii"])
    np.testing.assert_array_equal(_np(offs), p["isect_offsets"])
    np.testing.assert_array_equal(_np(fids), p["flatten_ids"])


def _cameras(p):
    cams = p["cameras"]
    return (torch.stack([c.viewmat for c in cams]).to(DEV), torch.stack([c.K for c in cams]).to(DEV),
            torch.stack([c.camera_center for c in cams]).to(DEV))


def _rasterization(ops, p, L, V=None, absgrad=True):
    V0, K, ctr = _cameras(p)
    cam = p["cameras"][0]
    return ops.rasterization(L["means"], L["quats"], L["scales"], L["opacities"].reshape(-1), L["sh"], V0 if V is None else V, K,
                             p["width"], p["height"], near_plane=cam.znear, far_plane=cam.zfar, sh_degree=p["sh_degree"],
                             render_mode="RGB+ED", absgrad=absgrad,
                             rasterize_mode="antialiased" if p["antialiasing"] else "classic", camera_centers_=ctr)


def _step_fused(ops, p):
    """gsplat's one-call API in training mode with the switch on (the caller holds it): RGB+ED, absgrad."""
    L = _leaves(p)
    rc, ra, meta = _rasterization(ops, p, L)
    assert meta["fused"] is True and type(meta) is dict
    _check_lists(p, meta["radii"], meta["isect_offsets"], meta["flatten_ids"])
    meta["means2d"].retain_grad()
    _loss(p, rc[..., :3], ra[..., 0], rc[..., 3]).backward()
    torch.cuda.synchronize()
    return L, meta["means2d"]


def _judge_step(tag, p, ref, K, L, vp):
    got = {}
    for k in PG.LEAVES:
        assert (L[k].grad is None) == (k in p["frozen"]), (tag, k)
        if L[k].grad is not None:
            got[k] = _np(L[k].grad).astype(np.float64)
    assert vp.grad is not None and hasattr(vp, "absgrad")
    got["means2d"] = _np(vp.grad).astype(np.float64)
    worst = PG.worst_ratios(got, ref, list(got))
    print(f"[hip fused] {tag}: " + ", ".join(f"{k} {r:.1f}" + (f" (|x| {off:.1e} where S = 0)" if off else "") for k, (r, off) in worst.items())
          + f"; bar {K:.1f}")
    for k, (r, off) in worst.items():
        assert np.isfinite(got[k]).all(), (tag, k)
        assert off == 0.0, (tag, k, off)
        assert r <= K, (tag, k, r, K)
    # absgrad rides on the same rows (its own per-row bar: tests/test_raster_bwd_rows_gpu.py)
    ab = _np(vp.absgrad).astype(np.float64)
    assert (ab[ref["S"]["means2d"] == 0] == 0).all() and (ab + 1e-6 * ab.max() >= np.abs(got["means2d"])).all(), tag
    assert float(p["unstable"].mean()) < RC.UNSTABLE_CAP and (ref["S"]["means"] > 0).any(), tag


# =============================================================================================
# 1  end to end
# =============================================================================================
@pytest.mark.parametrize("case_id", PG.CASE_IDS)
def test_fused_train_step_rows_against_the_float64_chain(ops, refs, case_id):
    table, K = refs
    p, ref = table[case_id]
    with _routes():
        L, vp = _step_fused(ops, p)
    _judge_step(f"{case_id} compiled", p, ref, K, L, vp)


def test_fused_train_step_rows_through_the_ctypes_table(ops, refs):
    table, K = refs
    for case_id in ("plain", "two_cameras"):
        p, ref = table[case_id]
        with _routes(fast=False, native=False):
            L, vp = _step_fused(ops, p)
        _judge_step(f"{case_id} ctypes", p, ref, K, L, vp)


# =============================================================================================
# 2  the forward is the composition's
# =============================================================================================
@pytest.mark.parametrize("case_id", ("plain", "classic", "two_cameras"))
def test_fused_train_forward_is_bit_identical_to_the_composition(ops, refs, case_id):
    p, _ = refs[0][case_id]
    out = {}
    for fused in (False, True):
        with _routes(fused=fused):
            rc, ra, meta = _rasterization(ops, p, _leaves(p))
        assert meta["fused"] is fused and rc.requires_grad
        out[fused] = dict(render_colors=rc, render_alphas=ra, **{k: meta[k] for k in ("radii", "means2d", "depths", "conics",
                                                                                      "opacities", "colors")})
    for k, a in out[False].items():
        b = out[True][k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        np.testing.assert_array_equal(_np(a).view(np.uint32 if a.dtype == torch.float32 else np.int32),
                                      _np(b).view(np.uint32 if b.dtype == torch.float32 else np.int32), err_msg=k)


def test_fused_train_meta_has_every_key_of_the_compositions(ops, refs):
    p, _ = refs[0]["plain"]
    keys = {}
    for fused in (False, True):
        with _routes(fused=fused):
            keys[fused] = set(_rasterization(ops, p, _leaves(p))[2])
    assert keys[True] == keys[False]


# =============================================================================================
# 3  the new node alone
# =============================================================================================
NODE_OUT = ("means2d", "conics", "opacities", "colors")          # the node's four differentiable outputs the chain uses


def _upstream(p, seed=77):
    """Fixed upstream gradients of the node's outputs, float32 values, zero on culled (camera, Gaussian) rows."""
    rng = np.random.default_rng(seed)
    C, N = p["radii"].shape
    vis = p["radii"] > 0
    X = dict(means2d=rng.normal(size=(C, N, 2)), conics=rng.normal(size=(C, N, 3)), opacities=rng.normal(size=(C, N)),
             colors=rng.normal(size=(C, N, 4)))
    X["colors"][..., 3] *= 0.1
    return {k: (v * vis.reshape(C, N, *([1] * (v.ndim - 2)))).astype(np.float32) for k, v in X.items()}


def _node(p, X, frozen=(), n=None, pad_k=None, ctypes_table=False, depth_apart=False):
    """torch.autograd.grad of _ProjectionSh's outputs under the upstream X -> {leaf: float32 numpy | None}.
    depth_apart: the depth's upstream arrives on the `depths` output instead of colour channel 3."""
    from street_crafter_amd.rendering import _ProjectionSh
    n = p["means"].shape[0] if n is None else n
    L = {k: _t(p[k][:n]).requires_grad_(k not in frozen) for k in PG.LEAVES}
    sh = L["sh"]
    if pad_k is not None:
        sh = torch.cat([_t(p["sh"][:n]), torch.full((n, pad_k - p["sh"].shape[1], 3), 0.25, device=DEV)], dim=1).requires_grad_("sh" not in frozen)
        L["sh"] = sh
    V, K, ctr = _cameras(p)
    cam = p["cameras"][0]
    with _routes(fast=not ctypes_table, native=not ctypes_table):
        radii, m2, d, con, op, col = _ProjectionSh.apply(L["means"], L["quats"], L["scales"], L["opacities"].reshape(-1), sh, V, K, ctr,
                                                         p["sh_degree"], p["width"], p["height"], PG.EPS2D, cam.znear, cam.zfar, 0.0,
                                                         p["antialiasing"])
        np.testing.assert_array_equal(_np(radii), p["radii"][:, :n])
        src = [k for k in PG.LEAVES if k not in frozen]
        outs, ups = [m2, con, op, col], [_t(X[k][:, :n]) for k in NODE_OUT]
        if depth_apart:
            outs.append(d)
            ups.append(ups[3][..., 3].clone())
            ups[3][..., 3] = 0.0
        g = torch.autograd.grad(outs, [L[k] for k in src], grad_outputs=ups)
        torch.cuda.synchronize()
    out = {k: None for k in PG.LEAVES}
    out.update({k: _np(x) for k, x in zip(src, g)})
    return out


@pytest.fixture(scope="module")
def node_refs(refs):
    """{case: (p, X, {"G", "S", "A" = 0} over the leaves)} and K_A: 4 x the worst ratio of the float32 torch replay of the
    SAME sub-chain (PG._camera_ops on the CPU) under the SAME upstream."""
    table, worst = {}, 0.0
    for cid in NODE_CASES:
        p, ref = refs[0][cid]
        X = _upstream(p)
        X64 = {k: v.astype(np.float64) for k, v in X.items()}
        G = PG.carry(p, X64, ref["jac"], absolute=False)
        S = PG.carry(p, {k: np.abs(v) for k, v in X64.items()}, ref["jac"])
        nref = {"G": G, "S": S, "A": {k: np.zeros_like(v) for k, v in S.items()}}
        L = PG._leaves(p, torch.float32)
        per = [PG._camera_ops(p, c, L, torch.float32) for c in range(len(p["cameras"]))]
        outs = [torch.stack([q[k] for q in per]) for k in NODE_OUT]
        g = torch.autograd.grad(outs, [L[k] for k in PG.LEAVES], grad_outputs=[torch.from_numpy(X[k]) for k in NODE_OUT],
                                allow_unused=True)
        rep = {k: (np.zeros(tuple(L[k].shape)) if x is None else x.double().numpy()) for k, x in zip(PG.LEAVES, g)}
        r = PG.worst_ratios(rep, nref, PG.LEAVES)
        assert all(off == 0.0 for _, off in r.values()), (cid, r)
        print(f"[node replay] {cid}: " + ", ".join(f"{k} {v:.1f}" for k, (v, _) in r.items()))
        worst = max(worst, max(v for v, _ in r.values()))
        table[cid] = (p, X, nref)
    print(f"[node replay] worst ratio {worst:.1f}; K_A = {4 * worst:.1f}")
    return table, 4.0 * worst


@pytest.mark.parametrize("case_id", NODE_CASES)
@pytest.mark.parametrize("ctypes_table", [False, True], ids=["compiled", "ctypes"])
def test_node_rows_against_the_float64_jacobians(node_refs, case_id, ctypes_table):
    table, K_A = node_refs
    p, X, nref = table[case_id]
    got = _node(p, X, ctypes_table=ctypes_table)
    worst = PG.worst_ratios({k: got[k].astype(np.float64) for k in PG.LEAVES}, nref, PG.LEAVES)
    print(f"[hip node] {case_id}: " + ", ".join(f"{k} {r:.1f}" for k, (r, _) in worst.items()) + f"; bar K_A {K_A:.1f}")
    for k, (r, off) in worst.items():
        assert np.isfinite(got[k]).all(), k
        assert off == 0.0, (k, off)
        assert r <= K_A, (k, r, K_A)
    nowhere = ~(p["radii"] > 0).any(0)
    assert nowhere.sum() > 10 and (p["radii"] > 0).any(0).sum() > 100
    for k in PG.LEAVES:
        assert (got[k][nowhere] == 0).all(), k


def _same(a, b, msg):
    for k in PG.LEAVES:
        assert (a[k] is None) == (b[k] is None), (msg, k)
        if a[k] is not None:
            np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=f"{msg}: {k}")


@pytest.mark.parametrize("case_id", NODE_CASES)
def test_node_is_deterministic_and_rows_do_not_depend_on_the_launch(node_refs, case_id):
    p, X, _ = node_refs[0][case_id]
    full = _node(p, X)
    _same(full, _node(p, X), "second run")
    part = _node(p, X, frozen=("quats", "sh"))
    assert part["quats"] is None and part["sh"] is None
    for k in ("means", "scales", "opacities"):
        np.testing.assert_array_equal(part[k].view(np.uint32), full[k].view(np.uint32), err_msg=f"quats, sh frozen: {k}")
    _same(full, _node(p, X, depth_apart=True), "depth upstream on the depths output")
    for n in (1, 257):                                   # one lane of one block; one lane into the second block
        sub = _node(p, X, n=n)
        for k in PG.LEAVES:
            assert sub[k].shape[0] == n
            np.testing.assert_array_equal(sub[k].view(np.uint32), full[k][:n].view(np.uint32), err_msg=f"first {n}: {k}")


@pytest.mark.parametrize("case_id", NODE_CASES)
def test_node_never_reads_the_upstream_rows_of_culled_pairs(node_refs, case_id):
    p, X, _ = node_refs[0][case_id]
    culled = ~(p["radii"] > 0)
    assert culled.any() and (~culled).any()
    Xn = {k: v.copy() for k, v in X.items()}
    for v in Xn.values():
        v[culled] = np.nan
    got = _node(p, Xn)
    _same(_node(p, X), got, "NaN in culled upstream rows")
    nowhere = culled.all(0)
    for k in PG.LEAVES:
        assert np.isfinite(got[k]).all() and (got[k][nowhere] == 0).all(), k


def test_node_with_sh_rows_padded_to_16_bases(refs):
    p, _ = refs[0]["ragged"]
    assert p["sh_degree"] == 1 and p["sh"].shape[1] == 4
    X = _upstream(p, seed=78)
    own, padded = _node(p, X), _node(p, X, pad_k=16)
    assert padded["sh"].shape == (p["sh"].shape[0], 16, 3)
    np.testing.assert_array_equal(padded["sh"][:, :4].view(np.uint32), own["sh"].view(np.uint32))
    assert (padded["sh"][:, 4:] == 0).all() and np.abs(own["sh"]).max() > 0
    for k in ("means", "quats", "scales", "opacities"):
        np.testing.assert_array_equal(padded[k].view(np.uint32), own[k].view(np.uint32), err_msg=k)


# =============================================================================================
# 4  which calls take the route
# =============================================================================================
def test_route_is_taken_only_under_grad_with_fixed_cameras(ops, refs):
    from street_crafter_amd.rendering import _FusedMeta
    p, _ = refs[0]["plain"]
    with _routes():
        with torch.no_grad():
            meta = _rasterization(ops, p, _leaves(p))[2]
        assert type(meta) is _FusedMeta and meta["fused"] is True          # today's forward-only fused path
        rc, _, meta = _rasterization(ops, p, _leaves(p, frozen=PG.LEAVES))
        assert type(meta) is _FusedMeta and not rc.requires_grad
        V = _cameras(p)[0].clone().requires_grad_(True)
        rc, _, meta = _rasterization(ops, p, _leaves(p), V=V)
        assert meta["fused"] is False and rc.requires_grad                  # cameras under grad: the composition
        rc, _, meta = _rasterization(ops, p, _leaves(p))
        assert meta["fused"] is True and type(meta) is dict and rc.requires_grad
    rc, _, meta = _rasterization(ops, p, _leaves(p))                        # the switch is off by default
    assert meta["fused"] is False


def test_route_refuses_cpu_tensors(ops, refs):
    p, _ = refs[0]["plain"]
    L = {k: torch.from_numpy(p[k]).requires_grad_(True) for k in PG.LEAVES}
    V, K, ctr = (t.cpu() for t in _cameras(p))
    with _routes():
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.rasterization(L["means"], L["quats"], L["scales"], L["opacities"].reshape(-1), L["sh"], V, K, p["width"], p["height"],
                              sh_degree=p["sh_degree"], render_mode="RGB+ED", rasterize_mode="antialiased", camera_centers_=ctr)
