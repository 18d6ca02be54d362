"""No-GPU checks of the actor poses: TrackTable.plan against hand-written tables, the float64 slerp of
tests/actor_pose_ref.py against scipy's, the float32 replay against the float64 truth, the argument checks of
sc_actor_poses_fwd / sc_actor_poses_bwd, and the Python refusals in their order."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import actor_pose_ref as ref  # noqa: E402

from street_crafter_amd import actor_pose  # noqa: E402
from street_crafter_amd.actor_pose import DELTA, INTERP, TrackTable  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


# ---- plan ---------------------------------------------------------------------------------------------------------------
CAMS, FRAMES, OBJ = 2, 5, 4
TS = [[10.0, 10.1, 10.25, 10.3, 10.4], [20.0, 20.1, 20.1, 20.1, 20.4]]


def _table(valid=None):
    tr = np.zeros((CAMS, FRAMES, OBJ, 8), dtype=np.float32)
    tr[..., 3] = 1.0
    tr[..., 7] = 1.0 if valid is None else valid
    return TrackTable(tr, TS, device="cpu")


def _row(cam, f, i):
    return (cam * FRAMES + f) * OBJ + i


def _items(plan):
    return [(it.row, it.row_prev, it.row_next, it.flags) for it in plan.items[:plan.A]]


def test_table_keeps_mask_and_timestamps_on_the_host():
    t = _table()
    assert isinstance(t.valid, np.ndarray) and t.valid.dtype == np.int32 and t.valid.shape == (CAMS, FRAMES, OBJ)
    assert t.camera_timestamps is TS and t.rows == CAMS * FRAMES * OBJ
    assert t.input_trans.shape == (CAMS, FRAMES, OBJ, 3) and t.input_rots.shape == (CAMS, FRAMES, OBJ, 4)
    assert t.input_trans.dtype == t.input_rots.dtype == torch.float32
    assert t.input_trans.is_contiguous() and t.input_rots.is_contiguous()
    with pytest.raises(ValueError, match="max_obj, 8"):
        TrackTable(np.zeros((2, 3, 4, 7)), TS, device="cpu")


def test_plan_rows_and_flags_against_a_hand_written_table():
    t = _table()
    p = t.plan([2, 0, 3], 1, 3, 20.1)
    assert p.A == 3 and p.rows == 40 and p.delta and not p.interp and p.ids == (2, 0, 3)
    assert _items(p) == [(_row(1, 3, i),) * 3 + (DELTA,) for i in (2, 0, 3)]
    assert all(it.alpha == 0.0 and it.one_minus_alpha == 1.0 for it in p.items[:3])
    # DELTA against is_novel_view (the reference's is_lidar_pose) and opt_track
    p = t.plan([1], 0, 2, 10.2, is_novel_view=True)
    assert _items(p) == [(_row(0, 2, 1),) * 3 + (0,)] and not p.delta
    p = t.plan([1], 0, 2, 10.2, opt_track=False)
    assert _items(p) == [(_row(0, 2, 1),) * 3 + (0,)] and not p.delta
    p = t.plan([1], 0, 2, 10.2, opt_track=False, is_val=True)            # no interpolation without opt_track
    assert _items(p) == [(_row(0, 2, 1),) * 3 + (0,)] and not p.interp
    # an empty list
    p = t.plan([], 0, 2, 10.2)
    assert p.A == 0 and not p.delta and not p.interp


def test_plan_validity_refusal():
    valid = np.ones((CAMS, FRAMES, OBJ), dtype=np.float32)
    valid[1, 3, 2] = 0.0
    t = _table(valid)
    with pytest.raises(ValueError, match="Invalid object 2"):
        t.plan([0, 2], 1, 3, 20.1)
    assert t.plan([0, 1, 3], 1, 3, 20.1).A == 3
    valid[1, 3, 2] = 2.0                                 # the reference asserts == 1
    with pytest.raises(ValueError, match="Invalid object"):
        _table(valid).plan([2], 1, 3, 20.1)
    with pytest.raises(ValueError, match="outside"):
        t.plan([OBJ], 1, 3, 20.1)
    with pytest.raises(ValueError, match="outside"):
        t.plan([0], CAMS, 3, 20.1)
    with pytest.raises(ValueError, match="outside"):
        t.plan([0], 0, FRAMES, 20.1)


def test_plan_interp_needs_all_four_conditions():
    t = _table()
    full = [(_row(0, 2, 1), _row(0, 1, 1), _row(0, 3, 1), DELTA | INTERP)]
    p = t.plan([1], 0, 2, 10.2, is_val=True)
    assert _items(p) == full and p.interp and p.delta
    p = t.plan([1], 0, 2, 10.2, is_val=True, is_novel_view=True)          # interpolated, without the deltas
    assert _items(p) == [full[0][:3] + (INTERP,)] and p.interp and not p.delta
    here = [(_row(0, 2, 1),) * 3 + (DELTA,)]
    assert _items(t.plan([1], 0, 2, 10.2, is_val=False)) == here                            # not a validation frame
    assert _items(t.plan([1], 0, 2, 10.2, is_val=True, opt_track=False)) == [here[0][:3] + (0,)]   # no opt_track
    assert _items(t.plan([1], 0, 0, 10.0, is_val=True)) == [(_row(0, 0, 1),) * 3 + (DELTA,)]       # the first frame
    assert _items(t.plan([1], 0, FRAMES - 1, 10.4, is_val=True)) == [(_row(0, FRAMES - 1, 1),) * 3 + (DELTA,)]   # the last
    for f in (1, 3):                                                                       # a neighbour that is not valid
        valid = np.ones((CAMS, FRAMES, OBJ), dtype=np.float32)
        valid[0, f, 1] = 0.0
        p = _table(valid).plan([1, 0], 0, 2, 10.2, is_val=True)
        assert _items(p) == [here[0], (_row(0, 2, 0), _row(0, 1, 0), _row(0, 3, 0), DELTA | INTERP)] and p.interp


def test_plan_alpha_is_the_fp32_of_the_float64_quotient():
    t = _table()
    for stamp in (10.1, 10.2, 10.25, 10.3, 10.17, 9.9):
        it = t.plan([0], 0, 2, stamp, is_val=True).items[0]
        alpha = (stamp - TS[0][1]) / (TS[0][3] - TS[0][1])
        assert it.alpha == np.float32(alpha) and it.one_minus_alpha == np.float32(1.0 - alpha)
        assert it.flags == DELTA | INTERP                                   # also outside [0, 1]: the reference extrapolates
    with pytest.raises(ValueError, match="same timestamp"):
        t.plan([0], 1, 2, 20.1, is_val=True)             # frames 1 and 3 of camera 1
    assert t.plan([0], 1, 2, 20.1, is_val=False).A == 1  # ... which only an interpolated item looks at


def test_plan_refuses_duplicates():
    with pytest.raises(ValueError, match="twice"):
        _table().plan([1, 2, 1], 0, 2, 10.2)


# ---- the float64 slerp against scipy ---------------------------------------------------------------------------------------
def _scipy_slerp(p, n, alpha):
    from scipy.spatial.transform import Rotation, Slerp
    out = np.zeros((len(p), 4))
    for k in range(len(p)):
        xyzw = np.stack((p[k], n[k]))[:, [1, 2, 3, 0]].astype(np.float64)
        q = Slerp([0.0, 1.0], Rotation.from_quat(xyzw))([alpha]).as_quat()[0]
        out[k] = q[[3, 0, 1, 2]]
    return out


def _fold(a, b):
    """a with the sign of each row chosen to match b"""
    return a * np.where((a * b).sum(-1, keepdims=True) < 0, -1.0, 1.0)


def test_float64_slerp_agrees_with_scipy_and_the_replay_with_it():
    P, N, what = ref.slerp_pairs()
    assert {"random", "equal", "opposite", "near", "unnormalised"} == set(what)
    worst64 = worst32 = 0.0
    for alpha in ref.ALPHAS:
        a32 = np.full(len(P), alpha, dtype=np.float32)
        truth = ref.slerp(P.astype(np.float64), N.astype(np.float64), a32.astype(np.float64))
        assert np.all(np.isfinite(truth))
        np.testing.assert_allclose(np.linalg.norm(truth, axis=-1), 1.0, rtol=0, atol=1e-15)
        ph = ref.normalize(P.astype(np.float64))
        assert np.all((truth * ph).sum(-1) > 0)                          # the sign follows p
        sp = _scipy_slerp(P, N, float(a32[0]))
        worst64 = max(worst64, np.abs(_fold(sp, truth) - truth).max())
        replay = ref.slerp(P, N, a32)
        assert replay.dtype == np.float32 and np.all(np.isfinite(replay))
        worst32 = max(worst32, np.abs(replay.astype(np.float64) - truth).max())   # the sign is compared, not folded
    print(f"actor_pose slerp: float64 vs scipy {worst64:.3g}; float32 replay vs float64 {worst32 / 2 ** -24:.2f} x 2^-24")
    # scipy: double arithmetic on another route (rotation vectors), a few ulp of 1
    assert worst64 <= 2e-15
    # the replay: some twenty fp32 operations deep on values <= 1: well under 16 ulp of 1, and far above 0 (it IS fp32)
    assert 0.0 < worst32 <= 16 * 2.0 ** -24
    # p == n returns normalize(p) at every alpha, in both precisions
    eq = [k for k, w in enumerate(what) if w == "equal"]
    for alpha in ref.ALPHAS:
        a32 = np.full(len(eq), alpha, dtype=np.float32)
        got = ref.slerp(P[eq], P[eq], a32)
        assert np.abs(got - ref.normalize(P[eq])).max() <= 2.0 ** -22
    # zero quaternions: the floor keeps everything finite
    z = np.zeros((1, 4), dtype=np.float32)
    assert np.all(np.isfinite(ref.slerp(z, z, np.float32([0.5])))) and np.all(np.isfinite(ref.slerp(z.astype(np.float64), z.astype(np.float64), np.array([0.5]))))


def test_replay_of_the_plain_path_sits_inside_the_bar_with_cpu_libm():
    tr, ts, ot, th = ref.make_table(2, 5, 130, seed=3)
    tab = ref.flat(tr, ot, th)
    t = TrackTable(tr, ts, device="cpu")
    items = ref.items_of(t.plan(range(130), 1, 2, ts[1][2]))
    q64, t64 = ref.poses(items, tab, np.float64)
    q32, t32 = ref.poses(items, tab, np.float32)
    bar = 2.0 ** -21 * ref.plain_rot_bar(tab, items)
    ratio = (np.abs(q32.astype(np.float64) - q64) / bar).max()
    print(f"actor_pose plain rotations: CPU replay at {ratio:.2f} of the bar")
    assert 0.0 < ratio <= 1.0
    rows = [it[0] for it in items]
    assert np.array_equal(t32, tab["input_trans"][rows] + tab["opt_trans"][rows])      # one add
    assert {0.0, np.float32(np.pi), np.float32(-np.pi)} <= set(tab["opt_rots"][rows].tolist())
    # float64 closed form of the backward against a central difference of the float64 forward
    g = np.random.default_rng(0).standard_normal((len(items), 4)).astype(np.float32)
    _, gr, mag = ref.backward64(items, tab, g, None, len(tab["opt_rots"]))
    h = 1e-6
    up, dn = dict(tab), dict(tab)
    up["opt_rots"] = tab["opt_rots"].astype(np.float64) + h
    dn["opt_rots"] = tab["opt_rots"].astype(np.float64) - h
    fd = ((ref.poses(items, up, np.float64)[0] - ref.poses(items, dn, np.float64)[0]) / (2 * h) * g).sum(-1)
    assert np.abs(fd - gr[rows]).max() <= 1e-8 * mag[rows].max() and np.all(mag[rows] > 0)


def test_torch_restatement_equals_the_truth():
    tr, ts, ot, th = ref.make_table(2, 5, 50, seed=1)
    tab = ref.flat(tr, ot, th)
    t = TrackTable(tr, ts, device="cpu")
    mod = ref.TorchActorPose(tr, ts, torch.from_numpy(ot), torch.from_numpy(th), "cpu")
    for kw, stamp in ((dict(), ts[0][2]), (dict(is_val=True), 0.3 * ts[0][1] + 0.7 * ts[0][3]), (dict(is_novel_view=True), ts[0][2])):
        ids = list(range(50))
        q64, t64 = ref.poses(ref.items_of(t.plan(ids, 0, 2, stamp, **kw)), tab, np.float64)
        q, tt = mod.poses(ids, 0, 2, stamp, **kw)
        assert q.shape == (50, 4) and tt.shape == (50, 3)
        assert np.abs(q.double().numpy() - q64).max() <= 1e-5 and np.abs(tt.double().numpy() - t64).max() <= 1e-4, kw
    valid = tr.copy()
    valid[0, 2, 7, 7] = 0.0
    with pytest.raises(AssertionError, match="Invalid object"):
        ref.TorchActorPose(valid, ts, torch.from_numpy(ot), torch.from_numpy(th), "cpu").poses([7], 0, 2, ts[0][2])


# ---- argument checks ---------------------------------------------------------------------------------------------------
FAKE = 0x1000                                          # never dereferenced: every call below returns before a launch


def _tab(rows, **over):
    seg = (actor_pose.PoseItem * max(len(rows), 1))()
    for k, (row, flags) in enumerate(rows):
        seg[k].row = seg[k].row_prev = seg[k].row_next = row
        seg[k].flags, seg[k].alpha, seg[k].one_minus_alpha = flags, 0.25, 0.75
    for key, v in over.items():
        setattr(seg[0], key, v)
    return seg


def test_argument_checks_without_gpu(lib):
    assert ctypes.sizeof(actor_pose.PoseItem) == 24
    n_max = lib.sc_actor_poses_max_items()
    assert n_max == 128 and 24 * n_max + 64 <= 4096                         # the table fits HIP's 4 KB of arguments
    fwd = lambda tab, A, rows=40, it=FAKE, ir=FAKE, ot=FAKE, orr=FAKE, oq=FAKE, otr=FAKE: \
        lib.sc_actor_poses_fwd(tab, A, rows, it, ir, ot, orr, oq, otr, None)
    assert fwd(None, 0) == 0 and fwd(None, 0, rows=0) == 0                  # A == 0: nothing launched
    assert fwd(None, 0, it=None, ir=None, oq=None, otr=None) == 0           # ... and no pointer is looked at
    assert fwd(None, -1) == -1 and fwd(_tab([(0, 0)]), 1, rows=-1) == -1    # negative counts
    assert fwd(None, 1) == -1                                               # a null table
    assert fwd(_tab([(40, 0)]), 1) == -1 and fwd(_tab([(-1, 0)]), 1) == -1  # a row outside [0, rows)
    assert fwd(_tab([(0, 0)]), 1, rows=0) == -1
    assert fwd(_tab([(3, 0), (40, DELTA)]), 2) == -1                        # ... in a later item
    for key in ("row_prev", "row_next"):
        assert fwd(_tab([(3, INTERP)], **{key: 40}), 1) == -1 and fwd(_tab([(3, INTERP)], **{key: -1}), 1) == -1
    assert fwd(_tab([(3, 4)]), 1) == -1 and fwd(_tab([(3, -1)]), 1) == -1   # unknown flag bits
    assert fwd(_tab([(3, DELTA)]), 1, ot=None) == -1 and fwd(_tab([(3, DELTA)]), 1, orr=None) == -1
    assert fwd(_tab([(3, DELTA | INTERP)]), 1, ot=None) == -1
    assert fwd(_tab([(3, 0)]), 1, it=None) == -1 and fwd(_tab([(3, 0)]), 1, ir=None) == -1
    assert fwd(_tab([(3, 0)]), 1, oq=None) == -1 and fwd(_tab([(3, 0)]), 1, otr=None) == -1   # a null output

    bwd = lambda tab, A, rows=40, ir=FAKE, orr=FAKE, gq=FAKE, gt=FAKE, dt=FAKE, dr=FAKE: \
        lib.sc_actor_poses_bwd(tab, A, rows, ir, orr, gq, gt, dt, dr, None)
    assert bwd(None, 0) == 0 and bwd(None, 0, ir=None, orr=None, dt=None, dr=None) == 0
    assert bwd(None, -1) == -1 and bwd(_tab([(0, 0)]), 1, rows=-1) == -1 and bwd(None, 1) == -1
    assert bwd(_tab([(40, DELTA)]), 1) == -1 and bwd(_tab([(-1, DELTA)]), 1) == -1
    assert bwd(_tab([(3, 8)]), 1) == -1
    assert bwd(_tab([(3, INTERP)]), 1) == -3 and bwd(_tab([(3, DELTA), (4, DELTA | INTERP)]), 2) == -3   # SC_EUNSUPPORTED
    assert bwd(_tab([(3, INTERP)], row_next=40), 1) == -1                   # ... after the table is found sound
    assert bwd(_tab([(3, DELTA)]), 1, ir=None) == -1 and bwd(_tab([(3, DELTA)]), 1, orr=None) == -1
    assert bwd(_tab([(3, DELTA), (5, DELTA), (3, DELTA)]), 3) == -1         # two DELTA items naming one row
    assert bwd(_tab([(3, DELTA), (5, DELTA), (5, DELTA)]), 3) == -1
    assert lib.sc_error_string(-3) == b"street_crafter_amd: unsupported configuration"


# ---- the Python refusals ---------------------------------------------------------------------------------------------------
def test_actor_poses_refuses_in_python_and_in_order():
    t = _table()
    shape = (CAMS, FRAMES, OBJ)
    ot, orr = torch.zeros(shape + (3,)), torch.zeros(shape + (1,))
    plan = t.plan([0, 1], 0, 2, 10.2)
    other = TrackTable(np.zeros((1, 2, 3, 8), dtype=np.float32), [[0.0, 1.0]], device="cpu")
    with pytest.raises(ValueError, match="rows"):
        actor_pose.actor_poses(other, plan, ot, orr)
    with pytest.raises(ValueError, match="opt_trans must be a float32"):
        actor_pose.actor_poses(t, plan, None, orr)
    with pytest.raises(ValueError, match="opt_rots must be a float32"):
        actor_pose.actor_poses(t, plan, ot, orr.double())
    with pytest.raises(ValueError, match=r"opt_trans must be \(2, 5, 4, 3\)"):
        actor_pose.actor_poses(t, plan, ot[..., :2], orr)
    with pytest.raises(ValueError, match=r"opt_rots must be \(2, 5, 4, 1\)"):
        actor_pose.actor_poses(t, plan, ot, orr[..., 0])
    with pytest.raises(ValueError, match="contiguous"):
        actor_pose.actor_poses(t, plan, torch.zeros((CAMS, FRAMES, 3, OBJ)).transpose(2, 3), orr)
    # a gradient through an interpolated row: refused before the device is looked at, and only when a gradient is asked
    val = t.plan([0, 1], 0, 2, 10.2, is_val=True)
    with pytest.raises(NotImplementedError, match="interpolated"):
        actor_pose.actor_poses(t, val, ot.clone().requires_grad_(True), orr)
    with pytest.raises(NotImplementedError, match="interpolated"):
        actor_pose.actor_poses(t, val, ot, orr.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="float32"):                         # ... and after the tensors are found sound
        actor_pose.actor_poses(t, val, ot.clone().requires_grad_(True), orr.double())
    for args in ((ot.clone().requires_grad_(True), orr), (ot, orr)):
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="no CPU path"):           # past the gradient rule: the device rule
                actor_pose.actor_poses(t, val, *args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        actor_pose.actor_poses(t, val, ot, orr)
    with pytest.raises(RuntimeError, match="no CPU path"):
        actor_pose.actor_poses(t, plan, ot.clone().requires_grad_(True), orr)
    # a plan without deltas does not look at opt_*
    with pytest.raises(RuntimeError, match="no CPU path"):
        actor_pose.actor_poses(t, t.plan([0], 0, 2, 10.2, is_novel_view=True), None, "nonsense")
