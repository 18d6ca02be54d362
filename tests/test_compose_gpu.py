"""GPU checks of the frame composition (csrc/compose.hip through street_crafter_amd/compose.py, both binding routes)
against the float64 reference of tests/compose_ref.py on the same fp32 inputs.

The bar, every element of every output and gradient, no exclusions:  |hip - G| <= 2^-24 K S,  K = 4 K_REF (K_REF: what
the fp32 torch restatement reaches, tests/test_compose_cpu.py), S the sum of the magnitudes of the element's terms, and
exactly G where S = 0 (the pure copies, the gradients nothing reaches).  Sky rows within DECISION_MARGIN of ratio == 1 or
exp(scaling) == radius carry no upstream gradient for that field (at most 1 % of a case, checked on the CPU).
The cases are compose_ref.build_cases(): see its docstring for the sizes, K, F, flips, sky rows and the zero rotations.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_BAR = 4.0 * ref.K_REF
CASES = ref.build_cases()
_GRADED = {}


def graded(case):
    """(G, S) of a case with all its upstream gradients, computed once"""
    if case["name"] not in _GRADED:
        _GRADED[case["name"]] = (ref.run(case, torch.float64), ref.track(case)[1])
    return _GRADED[case["name"]]


@pytest.fixture(scope="module")
def cp():
    from street_crafter_amd import _lib, compose
    _lib.load()
    assert _lib.load().sc_compose_max_segments() == ref.MAX_SEGMENTS
    return compose


@pytest.fixture(params=[True, False], ids=["compiled", "ctypes"])
def route(request):
    from street_crafter_amd import _lib
    prev = _lib.set_fast_binding(request.param)
    yield request.param
    _lib.set_fast_binding(prev)


def hip(cp, case, ups=True, pose_grad=True, include=None, actor_rows=None):
    """compose_frame on the device -> (dict with compose_ref.run's keys as float64 numpy, ranges)"""
    ups = case["ups"] if ups is True else ups
    models = ref.frame_models(case, DEV, requires_grad=ups is not None)
    rots = case["obj_rots"].to(DEV).requires_grad_(ups is not None and pose_grad)
    trans = case["obj_trans"].to(DEV).requires_grad_(ups is not None and pose_grad)
    flip = {k: v.to(DEV) for k, v in case["flip"].items()}
    if actor_rows is None:
        actor_rows = {m.name: i for i, m in enumerate(m for m in models if m.kind == cp.ACTOR)}
    *outs, ranges = cp.compose_frame(models, rots, trans, case["frame"], flip=flip, flip_q=case["flip_q"],
                                     actor_rows=actor_rows, include=include)
    res = {}
    for k, t in zip(ref.OUTPUTS, outs):
        assert t.is_contiguous() and t.dtype == torch.float32, k
        res[k] = t.detach().cpu().double().numpy()
    if ups is not None:
        live = [(t, ups[k].to(DEV)) for k, t in zip(ref.OUTPUTS, outs) if ups.get(k) is not None]
        torch.autograd.backward([t for t, _ in live], [g for _, g in live])
        for m in models:
            if include is not None and m.name not in include:
                continue
            for k in ref.PARAMS:
                g = getattr(m, k).grad
                assert g is not None, (m.name, k)
                res[f"g/{m.name}/{k}"] = g.cpu().double().numpy()
        res["pose_grads"] = (rots.grad, trans.grad)
        if pose_grad:
            res["g/obj_rots"], res["g/obj_trans"] = rots.grad.cpu().double().numpy(), trans.grad.cpu().double().numpy()
    return res, ranges


def assert_within(got, G, S, keys, what):
    for key in keys:
        assert got[key].shape == G[key].shape, (what, key, got[key].shape, G[key].shape)
        r, _ = ref.worst(got, G, S, [key])
        assert r <= K_BAR, f"{what}: {key}: worst |hip - G| / (2^-24 S) = {r:.3g} > K = {K_BAR}"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_forward_and_backward_are_within_the_bar(cp, route, case):
    if case["name"] == "max_segments_plus_1":       # empty segments take no slot: count the ones that do
        assert sum(1 for m in case["models"] if m["n"] > 0) > ref.MAX_SEGMENTS
    G, S = graded(case)
    got, ranges = hip(cp, case)
    assert ranges == case["ranges"]
    assert_within(got, G, S, list(G), case["name"])
    # the pure copies, bit for bit (S = 0 there already demands it; said once more in the open)
    for m in case["models"]:
        a, b = case["ranges"][m["name"]]
        np.testing.assert_array_equal(got["sh"][a:b, 1:], m["features_rest"].double().numpy())
        if m["kind"] != ref.ACTOR:
            np.testing.assert_array_equal(got["sh"][a:b, 0], m["features_dc"][:, 0].double().numpy())
        if m["kind"] == ref.STATIC:
            np.testing.assert_array_equal(got["means"][a:b], m["xyz"].double().numpy())


@pytest.mark.parametrize("absent", ref.OUTPUTS)
def test_each_upstream_gradient_absent_in_turn(cp, route, absent):
    case = CASES[0]
    ups = {k: (None if k == absent else v) for k, v in case["ups"].items()}
    G, S = ref.run(case, torch.float64, ups=ups), ref.track(case, ups=ups)[1]
    got, _ = hip(cp, case, ups=ups)
    assert_within(got, G, S, list(G), f"without {absent}")


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=lambda c: c["name"])
def test_poses_without_grad_leave_the_parameter_gradients_unchanged(cp, route, case):
    on, _ = hip(cp, case)
    off, _ = hip(cp, case, pose_grad=False)
    assert off["pose_grads"] == (None, None)
    assert on["pose_grads"][0] is not None and on["pose_grads"][1] is not None
    for key in on:
        if key.startswith("g/") and not key.startswith("g/obj_"):
            np.testing.assert_array_equal(on[key].view(np.uint64), off[key].view(np.uint64), err_msg=key)


def test_range_slices_equal_the_single_model_composes(cp, route):
    case = CASES[0]
    whole, ranges = hip(cp, case, ups=None)
    rows = {m["name"]: i for i, m in enumerate(m for m in case["models"] if m["kind"] == ref.ACTOR)}
    for m in case["models"]:
        if m["n"] == 0:
            continue
        one, r1 = hip(cp, case, ups=None, include=[m["name"]], actor_rows=rows)
        assert r1 == {m["name"]: [0, m["n"]]}
        a, b = ranges[m["name"]]
        for k in ref.OUTPUTS:
            np.testing.assert_array_equal(whole[k][a:b].view(np.uint64), one[k].view(np.uint64), err_msg=f"{m['name']} {k}")


def test_outputs_feed_rasterization_like_detached_copies(cp):
    """layout and contiguity are what the operators expect: the image from compose_frame's own outputs equals, bit for
    bit, the image from copies of the same values made element by element"""
    from street_crafter_amd import rendering
    from street_crafter_amd.scenes import make_camera
    case = CASES[0]
    models = ref.frame_models(case, DEV)
    flip = {k: v.to(DEV) for k, v in case["flip"].items()}
    means, quats, scales, opac, sh, _ = cp.compose_frame(models, case["obj_rots"].to(DEV), case["obj_trans"].to(DEV),
                                                         case["frame"], flip=flip)
    cam = make_camera(160, 96, 120.0, 120.0).to(DEV)
    render = lambda m, q, s, o, c: rendering.rasterization(
        m, q, s, o, c, cam.viewmat[None], cam.K[None], cam.width, cam.height, near_plane=cam.znear, far_plane=cam.zfar,
        sh_degree=3, render_mode="RGB+ED", rasterize_mode="antialiased")[:2]
    img, alpha = render(means, quats, scales, opac.squeeze(-1), sh)
    copy = lambda t: torch.from_numpy(t.detach().cpu().numpy().copy()).to(DEV)
    img2, alpha2 = render(copy(means), copy(quats), copy(scales), copy(opac).squeeze(-1), copy(sh))
    assert float(alpha.max()) > 0.5                      # something is in view
    assert torch.equal(img, img2) and torch.equal(alpha, alpha2)


def test_backward_into_a_misaligned_features_rest_gradient(cp):
    """compose_frame's gradient tensors are fresh allocations, so its features_rest gradient runs always start 16-byte
    aligned; a caller of the C ABI may hand over any fp32 pointer.  One static segment whose features_rest gradient
    starts 4 bytes into a buffer takes the element-by-element path: the same bits, nothing written outside."""
    import ctypes
    from street_crafter_amd import _ctypes_binding as cb
    from street_crafter_amd import _lib
    n, K = 70, 16
    gen = torch.Generator(device=DEV).manual_seed(3)
    rnd = lambda *shape: torch.randn(shape, device=DEV, generator=gen)
    raws = [[rnd(n, 3)], [rnd(n, 3)], [rnd(n, 4)], [rnd(n, 1)], [rnd(n, 1, 3)], [rnd(n, K - 1, 3)]]
    table = cb._compose_table(*raws, [torch.empty(0, dtype=torch.uint8, device=DEV)], [0, n], [cp.STATIC], [0],
                              [1.0] + [0.0] * 11)
    g_sh = rnd(n, K, 3)
    outs = [torch.empty_like(t[0]) for t in raws[:5]]
    buf = torch.full((n * (K - 1) * 3 + 2,), -7.0, device=DEV)
    grads = (_lib.ComposeGrads * 1)()
    grads[0].xyz, grads[0].scaling, grads[0].rotation, grads[0].opacity, grads[0].features_dc = (t.data_ptr() for t in outs)
    grads[0].features_rest = buf.data_ptr() + 4
    assert (buf.data_ptr() + 4) % 16 != 0
    rc = _lib.load().sc_compose_bwd(table, grads, 1, n, K, None, None, 0, None, None, None, None, None, g_sh.data_ptr(),
                                    None, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert torch.equal(buf[1:-1].view(n, K - 1, 3), g_sh[:, 1:])
    assert float(buf[0]) == -7.0 and float(buf[-1]) == -7.0
    assert torch.equal(outs[4], g_sh[:, :1]) and not outs[0].any() and not outs[2].any()
