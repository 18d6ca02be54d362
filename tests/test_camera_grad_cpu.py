"""tests/camera_grad_ref.py judged on its own (CPU, float64), and the argument checks of the two new entries that need no
device.  The references are shared with tests/test_camera_grad_gpu.py (built once per process)."""
import numpy as np
import pytest
import torch

import camera_grad_ref as CR
from oracle import gsplat_torch as OT

SMALL = ("n1", "n65", "n257", "n513_nocomp", "clamped_symmetric", "clamped_asymmetric")


def _loss_and_leaves(inp, c, V=None):
    """The operator-level float64 loss of camera c: sum_k sum_n u_k out_k over the rows the float32 forward keeps."""
    m, q, s = (torch.from_numpy(inp[k]).double() for k in ("means", "quats", "scales"))
    m.requires_grad_(True)
    V = torch.from_numpy(inp["V"][c]).double().requires_grad_(True) if V is None else V
    _, m2, d, con, comp = OT.fully_fused_projection(m, q, s, V, torch.from_numpy(inp["K"][c]).double(), inp["width"], inp["height"],
                                                    eps2d=inp["eps2d"], near_plane=inp["near"], far_plane=inp["far"],
                                                    proj_clamp=inp["proj_clamp"])
    vis = torch.from_numpy(inp["radii"][c] > 0).double()
    outs = (m2[:, 0], m2[:, 1], d, con[:, 0], con[:, 1], con[:, 2], comp)
    loss = sum((o * vis * torch.from_numpy(u[c]).double()).sum() for o, u in zip(outs, inp["u"]) if u is not None)
    return loss, m, V


@pytest.mark.parametrize("name", SMALL)
def test_rows_sum_to_autograd_and_the_means_identity(name):
    inp, ref = CR.operator_inputs(name), CR.operator_reference(name)
    assert (ref["S"] > 0).all() and ref["T"].shape[1:] == (inp["means"].shape[0], 3, 4)
    assert not ref["T"][inp["radii"] <= 0].any()
    for c in range(inp["V"].shape[0]):
        loss, m, V = _loss_and_leaves(inp, c)
        loss.backward()
        G = V.grad[:3].numpy()
        assert not V.grad[3].any()
        scale = np.abs(ref["T"][c]).sum(0)
        assert (np.abs(ref["T"][c].sum(0) - G) <= 1e-12 * scale).all() and (np.abs(ref["G"][c] - G) <= 1e-12 * scale).all()
        # the mean enters through W m + t alone: sum_n v_means_n = W^T v_t
        W = inp["V"][c].astype(np.float64)[:3, :3]
        lhs, rhs = m.grad.sum(0).numpy(), W.T @ G[:, 3]
        assert (np.abs(lhs - rhs) <= 1e-12 * (np.abs(W.T) @ scale[:, 3])).all()


@pytest.mark.parametrize("name", ["n65", "clamped_asymmetric"])
def test_central_differences_on_all_twelve_entries(name):
    """(f(V + h e) - f(V - h e)) / 2h with h = 1e-6: truncation h^2 f''' / 6 and cancellation 2^-53 sum|terms| / h, both far
    below 1e-5 of S, the sum of the entry's |contributions|."""
    inp, ref = CR.operator_inputs(name), CR.operator_reference(name)
    h = 1e-6
    for c in range(inp["V"].shape[0]):
        for i in range(3):
            for j in range(4):
                vals = []
                for sgn in (1.0, -1.0):
                    V = torch.from_numpy(inp["V"][c]).double()
                    V[i, j] += sgn * h
                    with torch.no_grad():
                        vals.append(float(_loss_and_leaves(inp, c, V)[0]))
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - ref["G"][c, i, j]) <= 1e-5 * ref["S"][c, i, j], (c, i, j, fd, ref["G"][c, i, j])


def test_operator_replay_band_and_wrong_variants():
    K = CR.operator_k()
    ks = {n: CR.operator_reference(n)["k_ref"] for n in CR.OPERATOR_CASES}
    print("[replay] operator K_ref " + ", ".join(f"{n} {k:.2f}" for n, k in ks.items()) + f"; K = {K:.1f}")
    assert K == 4 * max(ks.values())
    for name in CR.OPERATOR_CASES:
        ref = CR.operator_reference(name)
        assert CR.worst_ratio(ref["G"], ref["G"], ref["S"]) == (0.0, 0.0)
        for kind in ("cov_dropped", "w_transposed"):
            ratio, _ = CR.worst_ratio(CR.mutate_operator(name, kind), ref["G"], ref["S"])
            assert ratio > 10 * K, (name, kind, ratio, K)
        full = np.zeros(ref["G"].shape[:1] + (4, 4))
        full[:, :3] = ref["G"]
        assert CR.worst_ratio(full, ref["G"], ref["S"]) == (0.0, 0.0)           # the [C,4,4] form is read as its top block


def test_centre_vjp_is_autograd_of_minus_rt_t():
    g = torch.Generator().manual_seed(0)
    V = torch.randn(4, 4, generator=g, dtype=torch.float64).requires_grad_(True)
    u = torch.randn(3, generator=g, dtype=torch.float64)
    (-(V[:3, :3].T @ V[:3, 3]) * u).sum().backward()
    assert torch.allclose(V.grad[:3], CR.centre_vjp(V.detach(), u), rtol=0, atol=1e-14) and not V.grad[3].any()


@pytest.mark.parametrize("case_id", CR.CHAIN_CASES)
def test_chain_reference_carriage_replay_and_wrong_variants(case_id):
    """Autograd through the chain with the cameras as leaves equals the signed carriage of the boundary gradients through
    the per-row Jacobians (the route S and A take); the float32 replay stays inside the band; a transposed v_W is out of
    reach of the bar on every case, a detached centre on the cases of CENTRE_DETACHED_CAUGHT (the figures of the other two
    are in camera_grad_ref's docstring: nothing to see at SH degree 0, 0.92 x 2^-24 A on `classic`)."""
    r, K = CR.chain_reference(case_id), CR.chain_k()
    C = len(r["p"]["cameras"])
    for mode in ("constant", "derived"):
        G, S, A = r["G"][mode], r["S"][mode], r["A"][mode]
        assert G.shape == S.shape == A.shape == (C, 3, 4) and (S > 0).all() and (A > 0).all()
        assert (np.abs(r["carried"][mode] - G) <= 1e-10 * S).all()
        ratio, off = CR.worst_ratio(r["replay"][mode], G, S, A)
        print(f"[replay] {case_id} {mode}: ratio {ratio:.3f}, |err| / (2^-24 S) {(np.abs(r['replay'][mode] - G) / (CR.EPS24 * S)).max():.3f}, "
              f"/ (2^-24 A) {(np.abs(r['replay'][mode] - G) / (CR.EPS24 * A)).max():.4f}; K {K:.2f}")
        assert off == 0.0 and ratio <= r["k_ref"] <= K / 4 + 1e-12
        wrong = G.copy()
        wrong[:, :, :3] = np.swapaxes(wrong[:, :, :3], 1, 2)
        assert CR.worst_ratio(wrong, G, S, A)[0] > max(10 * K, 100.0)
    detached = CR.worst_ratio(r["G"]["constant"], r["G"]["derived"], r["S"]["derived"], r["A"]["derived"])[0]
    print(f"[mutation] {case_id}: centre detached -> ratio {detached:.1f}")
    if case_id in CR.CENTRE_DETACHED_CAUGHT:
        assert detached > max(10 * K, 100.0)
    if r["p"]["sh_degree"] == 0:
        assert np.array_equal(r["G"]["constant"], r["G"]["derived"])


def test_argument_checks_without_a_device():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    lib = _lib.load()
    assert lib.sc_projection_bwd_cam_workspace_bytes(3, 257) == 3 * 2 * 48 + 257 * 40
    assert lib.sc_projection_bwd_cam_workspace_bytes(1, 256) == 48 + 256 * 40 and lib.sc_projection_bwd_cam_workspace_bytes(1, 1) == 88
    assert lib.sc_projection_bwd_cam_workspace_bytes(65535, 2 ** 31 - 1) == 65535 * 8388608 * 48 + (2 ** 31 - 1) * 40
    for C, N in ((-1, 5), (5, -1), (0, 5), (5, 0)):
        assert lib.sc_projection_bwd_cam_workspace_bytes(C, N) == 0
    F = 4096                                   # a pointer nothing dereferences: every call below returns before a launch

    def call(C=1, N=1, w=8, h=8, inputs=F, v_viewmats=F, ws=F, v_means=F):
        return lib.sc_projection_bwd_cam(inputs, inputs, inputs, inputs, inputs, C, N, w, h, 0.3, inputs, inputs, None, inputs,
                                         inputs, inputs, None, v_means, None, None, v_viewmats, ws, None)

    assert call(C=-1) == -1 and call(N=-1) == -1 and call(w=0) == -1 and call(h=0) == -1
    assert call(v_viewmats=None) == -1                       # required whenever there is a camera
    assert call(inputs=None) == -1 and call(ws=None) == -1
    assert call(ws=F + 4) == -1                              # 16-byte alignment of the partial rows
    assert call(C=0, N=0, inputs=None, v_viewmats=None, ws=None, v_means=None) == 0
    assert lib.sc_camera_centers_bwd(None, None, -1, None, None) == -1
    assert lib.sc_camera_centers_bwd(None, None, 0, None, None) == 0
    assert lib.sc_camera_centers_bwd(F, F, 1, None, None) == -1 and lib.sc_camera_centers_bwd(None, F, 1, F, None) == -1


def test_python_routes_without_a_device():
    """The operators have no CPU path; what is new refuses the same way."""
    from street_crafter_amd import rendering as R
    V = torch.eye(4)[None].requires_grad_(True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        R.camera_centers(V)
