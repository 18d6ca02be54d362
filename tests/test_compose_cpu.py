"""No-GPU checks of the frame composition: plan_frame's ranges, the argument checks of sc_compose_fwd / sc_compose_bwd, the
float64 reference of tests/compose_ref.py against scene_io.compose_scene and against its own autograd, the recorded K_REF,
the exclusion cap of the GPU cases, and mutations of the fp32 replay against the bar the GPU test applies."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_ref as ref  # noqa: E402

from street_crafter_amd import compose, scene_io  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cases():
    return ref.build_cases()


@pytest.fixture(scope="module")
def graded(cases):
    """per case: (G by float64 autograd, S and the hand-written backward's values)"""
    out = []
    for case in cases:
        V, S = ref.track(case)
        out.append((ref.run(case, torch.float64), V, S))
    return out


# ---- ranges ---------------------------------------------------------------------------------------------------------
def _records():
    z = lambda *s: torch.zeros(s)
    mk = lambda name, kind, n, **kw: compose.FrameModel(name=name, kind=kind, xyz=z(n, 3), scaling=z(n, 3), rotation=z(n, 4),
                                                        opacity=z(n, 1), features_dc=z(n, 1, 3), features_rest=z(n, 15, 3),
                                                        **kw)
    # listed out of order on purpose: the sky first, the background in the middle
    return [mk("sky", compose.SKY, 7), mk("obj_001", compose.ACTOR, 5, start_frame=0, end_frame=10),
            mk("background", compose.STATIC, 11), mk("obj_002", compose.ACTOR, 3, start_frame=20, end_frame=30),
            mk("obj_003", compose.ACTOR, 2, start_frame=0, end_frame=99)]


def test_plan_frame_ranges_against_a_hand_written_table():
    models = _records()
    rows = {"obj_001": 0, "obj_002": 1, "obj_003": 2}
    plan = compose.plan_frame(models, rows, frame=5)
    assert plan.order == ["background", "obj_001", "obj_003", "sky"]              # obj_002 is outside its frame range
    assert plan.ranges == {"background": [0, 11], "obj_001": [11, 16], "obj_003": [16, 18], "sky": [18, 25]}
    assert [s["pose_row"] for s in plan.segments] == [-1, 0, 2, -1] and plan.n == 25
    assert list(plan.ranges) == plan.order                                          # the sky last
    plan = compose.plan_frame(models, rows, frame=25)
    assert plan.ranges == {"background": [0, 11], "obj_002": [11, 14], "obj_003": [14, 16], "sky": [16, 23]}
    # background absent
    plan = compose.plan_frame([m for m in models if m.name != "background"], rows, frame=5)
    assert plan.ranges == {"obj_001": [0, 5], "obj_003": [5, 7], "sky": [7, 14]}
    # an actor without a pose row is not visible
    plan = compose.plan_frame(models, {"obj_003": 0}, frame=5)
    assert plan.ranges == {"background": [0, 11], "obj_003": [11, 13], "sky": [13, 20]}
    # include lists as render_object / render_background use them
    plan = compose.plan_frame(models, rows, frame=5, include=["obj_001", "obj_002", "obj_003"])
    assert plan.ranges == {"obj_001": [0, 5], "obj_003": [5, 7]}
    plan = compose.plan_frame(models, rows, frame=5, include=["background"])
    assert plan.ranges == {"background": [0, 11]} and plan.segments[0]["kind"] == compose.STATIC
    plan = compose.plan_frame(models, rows, frame=5, include=[])
    assert plan.ranges == {} and plan.n == 0
    # without a table the actors inside their frame range take rows 0, 1, ... in list order
    plan = compose.plan_frame(models, None, frame=25)
    assert plan.order == ["background", "obj_002", "obj_003", "sky"] and [s["pose_row"] for s in plan.segments] == [-1, 0, 1, -1]
    assert compose.plan_frame(models, {}, frame=5).order == ["background", "sky"]
    with pytest.raises(ValueError):
        compose.plan_frame(models + [models[0]], rows)


def test_compose_frame_refuses_bad_inputs_in_python():
    models = _records()
    rots, trans = torch.zeros(3, 4), torch.zeros(3, 3)
    bad = _records()
    bad[2].xyz = bad[2].xyz.double()
    with pytest.raises(ValueError, match="float32"):
        compose.compose_frame(bad, rots, trans, 5)
    bad = _records()
    bad[2].features_rest = torch.zeros(11, 3, 15).transpose(1, 2)
    with pytest.raises(ValueError, match="contiguous"):
        compose.compose_frame(bad, rots, trans, 5)
    bad = _records()
    bad[0].features_rest = torch.zeros(7, 8, 3)
    with pytest.raises(ValueError, match="different K"):
        compose.compose_frame(bad, rots, trans, 5)
    with pytest.raises(ValueError, match="obj_rots"):
        compose.compose_frame(models, rots[:, :3].contiguous(), trans, 5)
    with pytest.raises(ValueError, match="pose row"):
        compose.compose_frame(models, rots[:1], trans[:1], 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compose.compose_frame(models, rots, trans, 5)


# ---- argument checks --------------------------------------------------------------------------------------------------
def _table(n, **over):
    from street_crafter_amd import _lib
    seg = (_lib.ComposeSegment * max(n, 1))()
    fake = 0x1000                                      # never dereferenced: every call below returns before a launch
    at = 0
    for k in range(n):
        s = seg[k]
        s.start, s.end = at, at + 4
        at += 4
        s.xyz = s.scaling = s.rotation = s.opacity = s.features_dc = s.features_rest = fake
        s.kind, s.pose_row, s.fourier_dim = 0, 0, 1
    for key, v in over.items():
        setattr(seg[0], key, v)
    return seg


def test_argument_checks_without_gpu(lib):
    from street_crafter_amd import _lib
    fake = 0x1000
    out5 = (fake,) * 5
    fwd = lambda seg, n, N, K=16, rots=fake, trans=fake, A=2, fq=None, outs=out5: \
        lib.sc_compose_fwd(seg, n, N, K, rots, trans, A, fq, *outs, None)
    assert lib.sc_compose_max_segments() == ref.MAX_SEGMENTS
    assert ctypes.sizeof(_lib.ComposeSegment) == 136 and ctypes.sizeof(_lib.ComposeGrads) == 48
    assert fwd(None, 0, 0) == 0                                                    # N == 0: nothing launched
    assert fwd(_table(1, end=0), 1, 0) == 0                                        # an empty segment is legal
    assert fwd(_table(1, end=0, xyz=None), 1, 0) == 0                              # ... and its pointers are not looked at
    assert fwd(None, -1, 0) == -1 and fwd(None, 0, -1) == -1                       # negative counts
    assert fwd(_table(1), 1, 4, A=-1) == -1
    assert fwd(None, 1, 4) == -1                                                   # a null table
    assert fwd(_table(1, start=5), 1, 4) == -1                                     # start > end
    assert fwd(_table(1, start=1), 1, 4) == -1                                     # does not start at 0
    assert fwd(_table(2), 2, 9) == -1 and fwd(_table(2), 2, 7) == -1               # does not end at N
    two = _table(2)
    two[1].start = 3                                                               # overlap
    assert fwd(two, 2, 8) == -1
    two = _table(2)
    two[0].start, two[0].end, two[1].start, two[1].end = 4, 8, 0, 4               # out of order
    assert fwd(two, 2, 8) == -1
    for key in ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest"):
        assert fwd(_table(1, **{key: None}), 1, 4) == -1, key                      # a null pointer in a non-empty segment
    assert fwd(_table(1), 1, 4, K=0) == -1                                         # K < 1
    assert fwd(_table(1, fourier_dim=0), 1, 4) == -1 and fwd(_table(1, fourier_dim=9), 1, 4) == -1
    assert fwd(_table(1, kind=3), 1, 4) == -1 and fwd(_table(1, kind=-1), 1, 4) == -1
    assert fwd(_table(1, kind=1, pose_row=2), 1, 4) == -1 and fwd(_table(1, kind=1, pose_row=-1), 1, 4) == -1
    assert fwd(_table(1, kind=1), 1, 4, rots=None) == -1 and fwd(_table(1, kind=1), 1, 4, trans=None) == -1
    assert fwd(_table(1, kind=1, flip=fake), 1, 4) == -1                           # a flip mask without flip_q
    for k in range(5):
        assert fwd(_table(1), 1, 4, outs=out5[:k] + (None,) + out5[k + 1:]) == -1  # a null output
    # backward: the same table checks, and the gradient table
    grads = (_lib.ComposeGrads * 1)()
    for f, _ in _lib.ComposeGrads._fields_:
        setattr(grads[0], f, fake)
    bwd = lambda seg, g, n, N, K=16, A=2: lib.sc_compose_bwd(seg, g, n, N, K, fake, fake, A, None, None, None, None, None,
                                                             None, None, None, None)
    assert bwd(None, None, 0, 0) == 0
    assert bwd(_table(1, end=0), grads, 1, 0) == 0
    assert bwd(_table(1), None, 1, 4) == -1 and bwd(None, grads, 1, 4) == -1
    assert bwd(_table(1), grads, 1, 5) == -1 and bwd(_table(1), grads, 1, 4, K=0) == -1
    assert bwd(_table(1, kind=1, pose_row=2), grads, 1, 4) == -1 and bwd(_table(1, fourier_dim=9), grads, 1, 4) == -1
    for f, _ in _lib.ComposeGrads._fields_:
        g = (_lib.ComposeGrads * 1)()
        for f2, _ in _lib.ComposeGrads._fields_:
            setattr(g[0], f2, None if f2 == f else fake)
        assert bwd(_table(1), g, 1, 4) == -1, f


# ---- the reference ----------------------------------------------------------------------------------------------------
def test_reference_forward_equals_compose_scene():
    """on what scene_io.compose_scene supports: background + posed actors with Fourier colours, no flip, no sky"""
    case = ref.build_cases()[0]
    models = [m for m in case["models"] if m["kind"] != ref.SKY]
    sub = dict(case, models=models, flip={}, N=sum(m["n"] for m in models))
    G = ref.run(sub, torch.float64, ups=None)
    subs, poses, row = {}, {}, 0
    for m in models:
        subs[m["name"]] = scene_io.SubModel(name=m["name"], **{k: m[k] for k in ref.PARAMS}, start_frame=m["start_frame"],
                                            end_frame=m["end_frame"], fourier_scale=m["fourier_scale"])
        if m["kind"] == ref.ACTOR:
            poses[m["name"]] = (case["obj_rots"][row], case["obj_trans"][row])
            row += 1
    cs = scene_io.compose_scene(subs, poses, frame=case["frame"])
    assert cs.graph_gaussian_range == {m["name"]: tuple(case["ranges"][m["name"]]) for m in models}
    got = dict(means=cs.scene.means, quats=cs.scene.quats, scales=cs.scene.scales, opacities=cs.scene.opacities,
               sh=cs.scene.sh)
    for k in ref.OUTPUTS:
        a, b = got[k].double().numpy(), G[k]
        assert a.shape == b.shape, k
        assert np.abs(a - b).max() <= 1e-5 * max(1.0, np.abs(b).max()), (k, np.abs(a - b).max())


def test_hand_written_backward_equals_autograd(cases, graded):
    """the tracked forward and backward carry the same values as float64 autograd: S is the S of the right formula"""
    for case, (G, V, S) in zip(cases, graded):
        assert set(V) == set(G) == set(S), set(V) ^ set(G)
        for key in G:
            assert V[key].shape == G[key].shape == S[key].shape, (case["name"], key)
            assert np.all(S[key] >= 0) and np.all(np.isfinite(S[key])), (case["name"], key)
            err = np.abs(V[key] - G[key])
            assert np.all(err <= 1e-12 * S[key] + 1e-300 * (S[key] == 0)) and np.all(err[S[key] == 0] == 0), \
                (case["name"], key, float(err.max()))


def test_exclusions_stay_inside_the_cap(cases):
    seen = 0
    for case in cases:
        assert case["excluded_rows"] <= 0.01 * case["N"], (case["name"], case["excluded_rows"], case["N"])
        seen += case["excluded_rows"]
    assert seen > 0                     # the rows at the radius exist


def test_k_ref_is_the_recorded_one(cases, graded):
    top = 0.0
    for case, (G, V, S) in zip(cases, graded):
        r, key = ref.worst(ref.run(case, torch.float32), G, S)
        print(f"compose K_ref  {case['name']:22s} {r:8.3f}  at {key}")
        top = max(top, r)
    print(f"compose K_ref = {top:.3f} (recorded {ref.K_REF})")
    # the record IS the measurement (1 %: what another libm's exp may move it by); the GPU bar is 4 times the record
    assert abs(top - ref.K_REF) <= 0.01 * ref.K_REF


@pytest.mark.parametrize("mut", ref.MUTATIONS)
def test_mutations_of_the_fp32_replay_exceed_the_bar(cases, graded, mut):
    """flip on the wrong axis; R built as if obj_rot were normalised (s = 2 instead of 2 / |q|^2); the clamp's gradient
    passed above the radius; the basis shifted by one.  norm_rot_first (obj_rot normalised, then the 2 / |q|^2 matrix) is
    the SAME function -- quaternion_to_matrix is invariant to the scale of q -- so it is measured and must stay inside."""
    K = 4.0 * ref.K_REF
    top = 0.0
    for case, (G, V, S) in zip(cases, graded):
        r, key = ref.worst(ref.run(case, torch.float32, mut=mut), G, S)
        top = max(top, r / K)
    print(f"compose mutation {mut:16s} worst error / bar = {top:.3g}")
    if mut == "norm_rot_first":
        assert top <= 1.0
    else:
        assert top > 1000.0
