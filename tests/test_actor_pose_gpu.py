"""GPU checks of the actor poses (street_crafter_amd.actor_pose, sc_actor_poses_fwd / _bwd) against
tests/actor_pose_ref.py: translations bit for bit against the float32 replay, rotations against float64 within derived
bars, the backward's tables in full, the chain into compose_frame, guard zones around every buffer, and no host wait.

One table for the whole module: cams=2, frames=5, max_obj=M; A in {0, 1, 63, 64, 65, max_items, max_items + 1}: one lane,
the wave boundary, and the boundary between two launches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import actor_pose_ref as ref  # noqa: E402
from guard_arena import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAMS, FRAMES, M = 2, 5, 130
MAX_ITEMS = 128
SIZES = [0, 1, 63, 64, 65, MAX_ITEMS, MAX_ITEMS + 1]


class World:
    """The table, its flat float32 arrays, the operator's objects and the torch restatement: built once, never changed."""

    def __init__(self):
        from street_crafter_amd import _lib, actor_pose
        self.lib, self.AP = _lib.load(), actor_pose
        assert self.lib.sc_actor_poses_max_items() == MAX_ITEMS
        self.tr, self.ts, ot, th = ref.make_table(CAMS, FRAMES, M, seed=11)
        self.tab = ref.flat(self.tr, ot, th)
        self.table = actor_pose.TrackTable(self.tr, self.ts, device=DEV)
        self.opt_trans = torch.from_numpy(ot).to(DEV)
        self.opt_rots = torch.from_numpy(th).to(DEV)
        self.torch_mod = ref.TorchActorPose(self.tr, self.ts, self.opt_trans, self.opt_rots, DEV)
        g = np.random.default_rng(5)
        self.ids = [int(i) for i in g.permutation(M)]          # the plan's order is not the table's
        self.g_rots = g.standard_normal((M, 4)).astype(np.float32)
        self.g_trans = g.standard_normal((M, 3)).astype(np.float32)

    def stamp(self, cam, f, alpha):
        pre, nxt = self.ts[cam][f - 1], self.ts[cam][f + 1]
        return pre if alpha == 0.0 else (nxt if alpha == 1.0 else pre + alpha * (nxt - pre))


@pytest.fixture(scope="module")
def W():
    return World()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", SIZES)
def test_plain_poses(W, A):
    """Translations: one add, bit-equal to the replay.  Rotations, per component against float64 on the fp32 inputs:
    |err| <= 2^-21 (|a1| + |a2|) -- two products and one sum at 2^-24 each, cosf / sinf at <= 2 ulp = 2^-22."""
    for kw in (dict(), dict(is_novel_view=True)):
        plan = W.table.plan(W.ids[:A], 1, 2, W.ts[1][2], **kw)
        with torch.no_grad():
            rots, trans = W.AP.actor_poses(W.table, plan, W.opt_trans, W.opt_rots)
        assert rots.shape == (A, 4) and trans.shape == (A, 3) and rots.dtype == trans.dtype == torch.float32
        assert rots.device == trans.device == torch.device(DEV) and not rots.requires_grad
        if A == 0:
            continue
        items = ref.items_of(plan)
        q32, t32 = ref.poses(items, W.tab, np.float32)
        q64, _ = ref.poses(items, W.tab, np.float64)
        assert np.array_equal(_bits(trans.cpu().numpy()), _bits(t32)), kw
        bar = 2.0 ** -21 * ref.plain_rot_bar(W.tab, items)
        ratio = (np.abs(rots.cpu().numpy().astype(np.float64) - q64) / bar).max()
        print(f"actor_pose plain rotations A={A} {kw}: kernel at {ratio:.3f} of the bar "
              f"(CPU replay {(np.abs(q32.astype(np.float64) - q64) / bar).max():.3f})")
        assert ratio <= 1.0, (A, kw, ratio)
        if kw:
            assert np.array_equal(_bits(rots.cpu().numpy()), _bits(W.tab["input_rots"][[it[0] for it in items]]))   # a copy


def test_torch_on_the_device_meets_the_plain_bar(W):
    """The 2 ulp of cosf / sinf are an assumption about the device's library: torch's own cos / sin on the same device go
    through the same check (were torch over the bar, the bar would be twice torch's ratio: DESIGN section 4)."""
    ids = W.ids[:MAX_ITEMS + 1]
    items = ref.items_of(W.table.plan(ids, 1, 2, W.ts[1][2]))
    q64, _ = ref.poses(items, W.tab, np.float64)
    with torch.no_grad():
        rows = torch.tensor(ids, device=DEV)
        got = ref.torch_quaternion_raw_multiply_theta(W.torch_mod.input_rots[1, 2, rows], W.opt_rots[1, 2, rows, 0])
    ratio = (np.abs(got.cpu().numpy().astype(np.float64) - q64) / (2.0 ** -21 * ref.plain_rot_bar(W.tab, items))).max()
    print(f"actor_pose plain rotations: torch on the device at {ratio:.3f} of the bar")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("A", SIZES[1:])
def test_interpolated_poses(W, A):
    """Validation frame 2 of camera 0 between frames 1 and 3 (where the slerp pairs of the CPU test sit, the degenerate
    ones included; without the deltas they arrive as they are).  Translations: two products and one sum, bit-equal to
    the replay.  Rotations against float64, sign compared: 4 x the worst error of the float32 replay on the same cases
    (device atan2f / sinf / cosf at 2 ulp against libm's 1, and another operation order)."""
    ids = list(range(A))                                                    # objects 0 .. 61 hold the pairs
    cases = []
    for alpha in ref.ALPHAS:
        for kw in (dict(is_novel_view=True), dict()):
            plan = W.table.plan(ids, 0, 2, W.stamp(0, 2, alpha), is_val=True, **kw)
            assert plan.interp and all(it.flags & ref.INTERP for it in plan.items[:A])
            assert abs(plan.items[0].alpha - alpha) <= 1e-6 and (alpha not in (0.0, 1.0) or plan.items[0].alpha == alpha)
            items = ref.items_of(plan)
            q32, t32 = ref.poses(items, W.tab, np.float32)
            q64, _ = ref.poses(items, W.tab, np.float64)
            cases.append((alpha, kw, plan, q32, t32, q64))
    replay = max(np.abs(q32.astype(np.float64) - q64).max() for _, _, _, q32, _, q64 in cases)     # on the CPU: the reference
    assert replay > 0
    worst = 0.0
    for alpha, kw, plan, q32, t32, q64 in cases:
        with torch.no_grad():
            rots, trans = W.AP.actor_poses(W.table, plan, W.opt_trans, W.opt_rots)
        got = rots.cpu().numpy()
        assert np.all(np.isfinite(got))
        assert np.array_equal(_bits(trans.cpu().numpy()), _bits(t32)), (alpha, kw)
        err = np.abs(got.astype(np.float64) - q64).max()
        worst = max(worst, err / replay)
        assert err <= 4.0 * replay, (A, alpha, kw, err, replay)
    print(f"actor_pose slerp A={A}: worst kernel error / worst replay error = {worst:.3f} (bar 4; replay "
          f"{replay / 2 ** -24:.2f} x 2^-24)")


def test_interpolation_happens_per_item(W):
    """One neighbour of object 5 is not valid: it takes the plain pose while the others interpolate."""
    tr = W.tr.copy()
    tr[0, 3, 5, 7] = 0.0
    table = W.AP.TrackTable(tr, W.ts, device=DEV)
    plan = table.plan([4, 5, 6], 0, 2, W.stamp(0, 2, 0.25), is_val=True)
    assert [it.flags for it in plan.items[:3]] == [3, 1, 3]
    with torch.no_grad():
        rots, trans = W.AP.actor_poses(table, plan, W.opt_trans, W.opt_rots)
    q32, t32 = ref.poses(ref.items_of(plan), W.tab, np.float32)
    assert np.array_equal(_bits(trans.cpu().numpy()), _bits(t32))
    # (which of the two poses a row took is a difference of order 1; the bars proper are the tests above)
    assert np.abs(rots.cpu().numpy() - q32).max() <= 1e-5


# ---- backward ----------------------------------------------------------------------------------------------------------------
def _bwd_direct(W, plan, g_rots, g_trans, want_trans=True, want_rots=True):
    """sc_actor_poses_bwd over NaN-filled tables -> (grad_opt_trans [rows,3], grad_opt_rots [rows]) numpy, or None"""
    rows = W.table.rows
    gt = torch.full((rows, 3), float("nan"), device=DEV) if want_trans else None
    gr = torch.full((rows,), float("nan"), device=DEV) if want_rots else None
    p = lambda t: None if t is None else t.data_ptr()
    rc = W.lib.sc_actor_poses_bwd(plan.items, plan.A, rows, W.table.input_rots.data_ptr(), W.opt_rots.data_ptr(), p(g_rots),
                                  p(g_trans), p(gt), p(gr), _stream())
    assert rc == 0, rc
    return (None if gt is None else gt.cpu().numpy()), (None if gr is None else gr.cpu().numpy())


@pytest.mark.parametrize("A", SIZES[1:])
def test_backward_tables(W, A):
    plan = W.table.plan(W.ids[:A], 1, 2, W.ts[1][2])
    items = ref.items_of(plan)
    rows = np.array([it[0] for it in items])
    g_rots, g_trans = torch.from_numpy(W.g_rots[:A]).to(DEV), torch.from_numpy(W.g_trans[:A]).to(DEV)
    gt, gr = _bwd_direct(W, plan, g_rots, g_trans)
    # translations: the upstream rows, bit for bit; every other row of both tables exactly zero (over NaN)
    assert np.array_equal(_bits(gt[rows]), _bits(W.g_trans[:A]))
    other = np.ones(W.table.rows, dtype=bool)
    other[rows] = False
    assert np.array_equal(_bits(gt[other]), np.zeros((other.sum(), 3), dtype=np.uint32))
    assert np.array_equal(_bits(gr[other]), np.zeros(other.sum(), dtype=np.uint32))
    # rotations: the forward's bar through four products, plus their sum
    _, want, mag = ref.backward64(items, W.tab, W.g_rots[:A], None, W.table.rows)
    bar = 2.0 ** -20 * 0.5 * mag[rows]
    ratio = (np.abs(gr[rows].astype(np.float64) - want[rows]) / bar).max()
    print(f"actor_pose grad_opt_rots A={A}: kernel at {ratio:.3f} of the bar")
    assert np.all(np.isfinite(gr)) and ratio <= 1.0, (A, ratio)
    # run to run
    gt2, gr2 = _bwd_direct(W, plan, g_rots, g_trans)
    assert np.array_equal(_bits(gt), _bits(gt2)) and np.array_equal(_bits(gr), _bits(gr2))
    # a null upstream gradient is zeros; a null table is not computed and the other is the same bits
    gt0, gr0 = _bwd_direct(W, plan, None, g_trans)
    assert np.array_equal(_bits(gt0), _bits(gt)) and np.array_equal(_bits(gr0), np.zeros_like(_bits(gr)))
    gt0, gr0 = _bwd_direct(W, plan, g_rots, None)
    assert np.array_equal(_bits(gr0), _bits(gr)) and np.array_equal(_bits(gt0), np.zeros_like(_bits(gt)))
    gt0, gr0 = _bwd_direct(W, plan, g_rots, g_trans, want_trans=False)
    assert gt0 is None and np.array_equal(_bits(gr0), _bits(gr))
    gt0, gr0 = _bwd_direct(W, plan, g_rots, g_trans, want_rots=False)
    assert gr0 is None and np.array_equal(_bits(gt0), _bits(gt))
    # a plan without deltas: zeros
    flat_plan = W.table.plan(W.ids[:A], 1, 2, W.ts[1][2], is_novel_view=True)
    gt0, gr0 = _bwd_direct(W, flat_plan, g_rots, g_trans)
    assert not gt0.any() and not gr0.any() and np.array_equal(_bits(gt0), np.zeros_like(_bits(gt)))
    # the operator's autograd route hands back the same tables
    ot, orr = W.opt_trans.clone().requires_grad_(True), W.opt_rots.clone().requires_grad_(True)
    rots, trans = W.AP.actor_poses(W.table, plan, ot, orr)
    assert rots.requires_grad and trans.requires_grad
    torch.autograd.backward([rots, trans], [g_rots, g_trans])
    assert ot.grad.shape == ot.shape and orr.grad.shape == orr.shape
    assert np.array_equal(_bits(ot.grad.cpu().numpy().reshape(-1, 3)), _bits(gt))
    assert np.array_equal(_bits(orr.grad.cpu().numpy().reshape(-1)), _bits(gr))


def test_one_sided_gradients_and_refusals(W):
    plan = W.table.plan(W.ids[:3], 1, 2, W.ts[1][2])
    ot = W.opt_trans.clone().requires_grad_(True)
    rots, trans = W.AP.actor_poses(W.table, plan, ot, W.opt_rots)
    (rots.sum() + trans.sum()).backward()
    assert float(ot.grad.sum()) == 9.0 and W.opt_rots.grad is None
    orr = W.opt_rots.clone().requires_grad_(True)
    rots, trans = W.AP.actor_poses(W.table, plan, W.opt_trans, orr)
    rots.sum().backward()                                                    # trans unused: its gradient is None
    assert torch.isfinite(orr.grad).all() and int((orr.grad != 0).sum()) == 3
    # nothing requires grad, or no_grad: no graph
    for ctx, args in ((torch.enable_grad(), (W.opt_trans, W.opt_rots)), (torch.no_grad(), (ot, orr))):
        with ctx:
            rots, trans = W.AP.actor_poses(W.table, plan, *args)
        assert rots.grad_fn is None and trans.grad_fn is None and not rots.requires_grad and not trans.requires_grad
    # interpolated rows carry no gradient
    val = W.table.plan([0, 1], 0, 2, W.stamp(0, 2, 0.5), is_val=True)
    with pytest.raises(NotImplementedError):
        W.AP.actor_poses(W.table, val, ot, orr)
    rc = W.lib.sc_actor_poses_bwd(val.items, val.A, W.table.rows, W.table.input_rots.data_ptr(), W.opt_rots.data_ptr(), None, None,
                                  None, None, _stream())
    assert rc == -3
    with pytest.raises(RuntimeError, match="no CPU path"):
        W.AP.actor_poses(W.table, plan, W.opt_trans.cpu(), W.opt_rots)


# ---- the chain into compose_frame ------------------------------------------------------------------------------------------
def test_chain_into_compose_frame(W):
    from street_crafter_amd import compose
    g = torch.Generator(device=DEV).manual_seed(3)
    rnd = lambda *s: torch.randn(s, device=DEV, generator=g)

    def models():
        gg = torch.Generator(device=DEV).manual_seed(4)
        r = lambda *s: torch.randn(s, device=DEV, generator=gg).requires_grad_(True)
        return [compose.FrameModel(name=f"obj_{k}", kind=compose.ACTOR, xyz=r(3, 3), scaling=r(3, 3), rotation=r(3, 4),
                                   opacity=r(3, 1), features_dc=r(3, 1, 3), features_rest=r(3, 1, 3)) for k in range(2)]
    ids = [7, 3]
    plan = W.table.plan(ids, 1, 2, W.ts[1][2])
    rows = [it.row for it in plan.items[:2]]
    ot, orr = W.opt_trans.clone().requires_grad_(True), W.opt_rots.clone().requires_grad_(True)
    rots, trans = W.AP.actor_poses(W.table, plan, ot, orr)
    outs = compose.compose_frame(models(), rots, trans, 0)[:5]
    sum(o.sum() for o in outs).backward()
    # compose's own pose gradients, from the same poses as leaves
    lr, lt = rots.detach().clone().requires_grad_(True), trans.detach().clone().requires_grad_(True)
    sum(o.sum() for o in compose.compose_frame(models(), lr, lt, 0)[:5]).backward()
    got_t, got_r = ot.grad.reshape(-1, 3), orr.grad.reshape(-1)
    assert torch.equal(got_t[rows].view(torch.int32), lt.grad.view(torch.int32))
    items = ref.items_of(plan)
    _, want, mag = ref.backward64(items, W.tab, lr.grad.cpu().numpy(), None, W.table.rows)
    err = np.abs(got_r.cpu().numpy().astype(np.float64) - want)
    assert torch.isfinite(got_r).all() and np.all(err[rows] <= 2.0 ** -20 * 0.5 * mag[rows]) and np.all(mag[rows] > 0)
    other = torch.ones(W.table.rows, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert not got_t[other].any() and not got_r[other].any()
    with torch.no_grad():
        rots, trans = W.AP.actor_poses(W.table, plan, ot, orr)
        outs = compose.compose_frame(models(), rots, trans, 0)[:5]
    assert rots.grad_fn is None and trans.grad_fn is None and all(o.grad_fn is None for o in outs)


# ---- guard zones -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [65, MAX_ITEMS + 1])
def test_guard_zones_around_every_buffer(W, A):
    """Both entries with every buffer cut from one arena, under two fills: no guard byte changes, no input changes, and
    the outputs are the same bits under both fills (an element left unwritten would keep its fill)."""
    plans = {"plain": W.table.plan(W.ids[:A], 1, 2, W.ts[1][2]),
             "interp": W.table.plan(list(range(A)), 0, 2, W.stamp(0, 2, 0.25), is_val=True)}
    ins = dict(input_trans=W.tab["input_trans"], input_rots=W.tab["input_rots"], opt_trans=W.tab["opt_trans"],
               opt_rots=W.tab["opt_rots"], g_rots=W.g_rots[:A], g_trans=W.g_trans[:A])
    outs = dict(obj_rots=16 * A, obj_trans=12 * A, grad_opt_trans=12 * W.table.rows, grad_opt_rots=4 * W.table.rows)
    res = {}
    for fill in (0xA5, 0x3F):
        sizes = {k: v.nbytes for k, v in ins.items()}
        sizes.update(outs)
        for name, plan in plans.items():
            ar = Arena(sizes, DEV, fill=fill)
            for k, v in ins.items():
                ar.view(k).copy_(torch.from_numpy(np.ascontiguousarray(v)).view(torch.uint8).reshape(-1))
            rc = W.lib.sc_actor_poses_fwd(plan.items, A, W.table.rows, ar.ptr("input_trans"), ar.ptr("input_rots"),
                                          ar.ptr("opt_trans"), ar.ptr("opt_rots"), ar.ptr("obj_rots"), ar.ptr("obj_trans"),
                                          _stream())
            assert rc == 0, rc
            written = ["obj_rots", "obj_trans"]
            if name == "plain":
                rc = W.lib.sc_actor_poses_bwd(plan.items, A, W.table.rows, ar.ptr("input_rots"), ar.ptr("opt_rots"),
                                              ar.ptr("g_rots"), ar.ptr("g_trans"), ar.ptr("grad_opt_trans"),
                                              ar.ptr("grad_opt_rots"), _stream())
                assert rc == 0, rc
                written += ["grad_opt_trans", "grad_opt_rots"]
            torch.cuda.synchronize()
            assert ar.broken_guards() == [], (fill, name, ar.broken_guards(), ar.span)
            for k, v in ins.items():
                assert np.array_equal(ar.view(k).cpu().numpy(), np.ascontiguousarray(v).view(np.uint8).reshape(-1)), f"input {k} was written"
            res[fill, name] = {k: ar.view(k, torch.int32).clone() for k in written}
    for name in plans:
        for k, v in res[0xA5, name].items():
            assert torch.equal(v, res[0x3F, name][k]), f"{name}: {k} differs between the fills"
    q32, t32 = ref.poses(ref.items_of(plans["plain"]), W.tab, np.float32)
    assert np.array_equal(res[0xA5, "plain"]["obj_trans"].cpu().numpy().view(np.uint32).reshape(A, 3), _bits(t32))


# ---- no host wait ------------------------------------------------------------------------------------------------------------
def test_no_host_wait(W):
    """Forward and backward are enqueued behind 200 passes over 256 MB (12.8 ms at the memory's 8 TB/s, more in practice)
    and return while that work is still running: the event recorded behind it has not completed.  Under
    set_sync_debug_mode("error") torch's own waits would raise as well."""
    plan = W.table.plan(W.ids[:32], 1, 2, W.ts[1][2])
    val = W.table.plan(list(range(32)), 0, 2, W.stamp(0, 2, 0.25), is_val=True)
    ot, orr = W.opt_trans.clone().requires_grad_(True), W.opt_rots.clone().requires_grad_(True)
    g_rots, g_trans = torch.from_numpy(W.g_rots[:32]).to(DEV), torch.from_numpy(W.g_trans[:32]).to(DEV)
    torch.autograd.backward(W.AP.actor_poses(W.table, plan, ot, orr), [g_rots, g_trans])      # warm-up: everything loaded
    ot.grad = orr.grad = None
    big = torch.ones(64 * 1024 * 1024, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        front = torch.cuda.Event()
        for _ in range(200):
            big.mul_(1.0001)
        front.record()
        rots, trans = W.AP.actor_poses(W.table, plan, ot, orr)
        torch.autograd.backward([rots, trans], [g_rots, g_trans])
        with torch.no_grad():
            vr, vt = W.AP.actor_poses(W.table, val, ot, orr)
        pending = not front.query()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert pending, "the work in front had finished when forward + backward returned: something in them waited for the GPU"
    assert torch.isfinite(ot.grad).all() and torch.isfinite(orr.grad).all() and torch.isfinite(vr).all() and torch.isfinite(vt).all()
