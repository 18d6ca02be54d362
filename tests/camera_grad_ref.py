"""The cameras' gradient (gsplat's v_viewmats) in float64 with per-entry error scales -- TEST INFRASTRUCTURE ONLY.

float64 autograd through oracle/gsplat_torch.py with the view matrix as a LEAF is the reference; nothing under oracle/ is
changed.  A Gaussian's projection depends on the view matrix row-independently, so the per-row Jacobians come from ONE
backward call per projection output: the oracle is vmapped over the rows with a view matrix of each row's own
(`row_jacobians`), and d out_k[n] / d V lands in row n of that leaf's gradient.  Entries are the [3,4] block [W | t] of a
view matrix; the bottom row never enters the projection and its gradient must be exactly +0.

OPERATOR level (`operator_reference`): upstream u_k [C,N] on the 7 projection outputs (means2d x, y; depth; conic a, b, c;
compensation), the radii of the float32 forward as a fact (a row with radii <= 0 takes no part, whatever float64 says):
    T[c,n]  = sum_k u_k[c,n] d out_k[n] / d V_c          the per-row contributions
    G[c]    = sum_n T[c,n]                               the float64 gradient
    S[c,e]  = sum_n sum_k |d out_k[n] / d V_e| |u_k|     no cancellation, neither between outputs nor between rows
    bar       |x - G| <= 2^-24 K S,  exactly 0 where S == 0.
CHAIN level (`chain_reference`): oracle/param_grad_f64.py's chain with the cameras as leaves.  The cameras of the case
are replaced by stand-ins whose view matrix and centre are float64 leaves (`leaf_cameras`: `.to(dtype)` of a tensor of
that dtype is the tensor itself, so param_grad_f64 builds its graph on them), and ONE PG.reference() call yields the
leaves' reference, dL/dV with the centre a constant and dL/dcentre; with the centre derived from the view matrix,
c = -R^T t, the gradient is the sum of the first and the VJP of the second (`centre_vjp`).  S and A are PG.reference's
boundary scales carried through the absolute per-row Jacobians with respect to V, the direction path included where the
centre is derived, and summed over n -- param_grad_f64.carry for the cameras:
    bar       |x - G| <= 2^-24 (K S + A),  exactly 0 where S == 0.

K = 4 K_ref at either level, K_ref the largest ratio |x32 - G| / (2^-24 S) (chain: (|x32 - G| - 2^-24 A)+) a float32
torch replay of the same computation reaches over all entries of all cases of that level (CPU, no kernel); the 4 is the
project's margin for FMA contraction, v_rcp_f32 and another summation order (oracle/param_grad_f64.py).  K_ref is not a
rounding count.  The sum over n adds little: a float32 sum of N terms errs by some 2^-24 log2(N) sum|T| at most and S is
sum|T| without the cancellation between outputs (the 262401-row case replays at 0.13).  What K_ref measures is the
conditioning of one row's float32 Jacobian -- the conic is the inverse of a 2x2 covariance that the needles of the operator
scenes (scales from 0.002 to 0.5) make nearly singular -- which S, a sum of |Jacobian| |upstream|, does not see.
Measured on the CPU (x86-64, torch 2.x), operator level: between 0.12 (the clamped scene) and 9.3 (n513) over
OPERATOR_CASES, 4.9 for the single row of n1.  Chain level: 0 on all five CHAIN_CASES in both centre modes -- the replay's
error is at most 0.2 x 2^-24 S and 0.002 x 2^-24 A (row errors of either sign add up over some 2000 rows while S and A add
magnitudes, and A, the stored-alpha term, is 70 to 430 times S here), so it never leaves the A part of the bar, K = 0 and
the chain-level bar is |x - G| <= 2^-24 A.  That bar is wide next to the direction path: with the centre wrongly detached
the gradient moves by 2.4 (plain, clamped), 54 (two_cameras) but only 0.92 (classic) times 2^-24 A, and by nothing at SH
degree 0.  Bands (a replay outside means the cases or the reference changed character, not noise -- one K per level
loosens every case's bar):
"""
from __future__ import annotations

import functools
import types

import numpy as np
import torch

from oracle import gsplat_oracle as O
from oracle import gsplat_torch as OT
from oracle import param_grad_f64 as PG

EPS24 = 2.0 ** -24
K_REF_BAND_OPERATOR = (1.0, 25.0)
K_REF_BAND_CHAIN = (0.0, 4.0)              # lower end included
CHAIN_CASES = ("plain", "classic", "deg0", "clamped", "two_cameras")
MUTATIONS = ("cov_dropped", "w_transposed", "centre_detached")
CENTRE_DETACHED_CAUGHT = ("plain", "clamped", "two_cameras")     # where the chain-level bar tells the two centre modes apart
W0, H0 = 320, 200                                # the operator cases' frame
BIG_N = 256 * 1025 + 1                           # more partial rows per camera than the reduction kernel has threads (1024)
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, BIG_N)


# ---- per-row Jacobians ------------------------------------------------------------------------------------------------------
def row_jacobians(means, quats, scales, V, K, width, height, dtype=torch.float64, **kw):
    """[7] x [N,3,4]: d (means2d x, y, depth, conic a, b, c, compensation)[n] / d V[:3,:4], torch tensors of `dtype`.
    kw: eps2d, near_plane, far_plane, proj_clamp of oracle/gsplat_torch.py::fully_fused_projection."""
    m, q, s = (torch.as_tensor(a).to(dtype) for a in (means, quats, scales))
    V, K = torch.as_tensor(V).to(dtype), torch.as_tensor(K).to(dtype)
    N = m.shape[0]
    Vr = V[None].expand(N, 4, 4).clone().requires_grad_(True)

    def one(mm, qq, ss, Vn):
        _, m2, d, con, comp = OT.fully_fused_projection(mm[None], qq[None], ss[None], Vn, K, width, height, **kw)
        return m2[0], d[0], con[0], comp[0]

    m2, d, con, comp = torch.func.vmap(one)(m, q, s, Vr)
    outs = (m2[:, 0], m2[:, 1], d, con[:, 0], con[:, 1], con[:, 2], comp)
    return [torch.autograd.grad(o.sum(), Vr, retain_graph=True)[0][:, :3, :].detach() for o in outs]


# ---- operator level ---------------------------------------------------------------------------------------------------------
def operator_cameras():
    """Three cameras of one frame size; the second has its principal point off centre."""
    from street_crafter_amd.scenes import make_camera
    cams = [make_camera(W0, H0, 350.0, 350.0, yaw=0.1),
            make_camera(W0, H0, 300.0, 330.0, yaw=-0.25, shift=(0.5, 0.1, -0.3)),
            make_camera(W0, H0, 420.0, 400.0, yaw=0.35, shift=(-0.4, -0.2, 0.6))]
    cams[1].K = cams[1].K.clone()
    cams[1].K[0, 2], cams[1].K[1, 2] = 0.42 * W0, 0.55 * H0
    return cams


# name -> (N | "clamped", proj_clamp, compensations).  The cases with a number run with all three cameras and with the
# second one alone (C = 1, principal point off centre); "centred" with the first alone.
OPERATOR_CASES = {f"n{n}": (n, "symmetric", True) for n in SIZES}
OPERATOR_CASES.update({"n513_nocomp": (513, "symmetric", False), "n257_nocomp": (257, "symmetric", False),
                       "clamped_symmetric": ("clamped", "symmetric", True), "clamped_asymmetric": ("clamped", "asymmetric", True)})


@functools.lru_cache(maxsize=None)
def operator_inputs(name):
    """float32 numpy: means, quats, scales, V [C,4,4], K [C,3,3], radii [C,N] (numpy oracle = the kernels' forward, bit for
    bit), upstream u [7][C,N] (None for the compensation without it), frame and planes."""
    from street_crafter_amd.scenes import make_scene
    n, proj_clamp, comp = OPERATOR_CASES[name]
    if n == "clamped":       # param_grad_f64's scene with Gaussians beyond the Jacobian clamp limit, under its own camera
        p = PG.make_case("clamped")
        means, quats, scales = p["means"], p["quats"], p["scales"]
        cams, width, height = p["cameras"], p["width"], p["height"]
    else:
        if n == 1:
            means, quats, scales = (np.array(a, np.float32) for a in ([[0.1, 0.05, 5.0]], [[0.8, 0.2, -0.4, 0.4]], [[0.2, 0.05, 0.4]]))
        else:
            sc = make_scene(n, seed=13 + (n % 97), x_span=0.8, y_span=0.5, z_range=(1.0, 40.0), scale_range=(0.002, 0.5))
            means, quats, scales = sc.means.numpy(), sc.quats.numpy(), sc.scales.numpy()
        cams, width, height = operator_cameras(), W0, H0
    V = np.stack([c.viewmat.numpy() for c in cams])
    K = np.stack([c.K.numpy() for c in cams])
    near, far = 0.001, 1000.0
    radii = np.stack([O.fully_fused_projection(means, quats, scales, V[c], K[c], width, height, near_plane=near, far_plane=far,
                                               calc_compensations=True, proj_clamp=proj_clamp)[0] for c in range(len(cams))])
    rng = np.random.default_rng(100 + len(name) + int(means.shape[0]) % 1000)
    u = [rng.normal(size=radii.shape).astype(np.float32) for _ in range(7)]
    if not comp:
        u[6] = None
    return dict(name=name, means=means, quats=quats, scales=scales, V=V, K=K, radii=radii, u=u, width=width, height=height,
                near=near, far=far, eps2d=0.3, proj_clamp=proj_clamp, comp=comp)


def operator_gradient(inp, dtype):
    """(T [C,N,3,4], |T| summed without cancellation between outputs [C,N,3,4]) in `dtype`, rows with radii <= 0 exactly 0."""
    C = inp["V"].shape[0]
    Ts, Ss = [], []
    for c in range(C):
        J = row_jacobians(inp["means"], inp["quats"], inp["scales"], inp["V"][c], inp["K"][c], inp["width"], inp["height"], dtype,
                          eps2d=inp["eps2d"], near_plane=inp["near"], far_plane=inp["far"], proj_clamp=inp["proj_clamp"])
        vis = torch.from_numpy(inp["radii"][c] > 0)
        T = torch.zeros_like(J[0])
        S = torch.zeros_like(J[0])
        for k, Jk in enumerate(J):
            if inp["u"][k] is None:
                continue
            uk = torch.from_numpy(inp["u"][k][c]).to(dtype)[:, None, None]
            T = T + uk * Jk
            S = S + uk.abs() * Jk.abs()
        zero = torch.zeros((), dtype=dtype)
        Ts.append(torch.where(vis[:, None, None], T, zero))
        Ss.append(torch.where(vis[:, None, None], S, zero))
    return torch.stack(Ts), torch.stack(Ss)


@functools.lru_cache(maxsize=None)
def operator_reference(name):
    """{"G" [C,3,4], "S" [C,3,4], "T" [C,N,3,4], "k_ref": the float32 replay's worst ratio} (float64 numpy)."""
    inp = operator_inputs(name)
    T, S = operator_gradient(inp, torch.float64)
    # a row the float32 forward keeps must be one the float64 oracle keeps: its Jacobian is what is summed
    G, Ssum = T.sum(1).numpy(), S.sum(1).numpy()
    T32, _ = operator_gradient(inp, torch.float32)
    G32 = T32.sum(1).double().numpy()
    return dict(G=G, S=Ssum, T=T.numpy(), k_ref=worst_ratio(G32, G, Ssum)[0])


def worst_ratio(x, G, S, A=None):
    """(largest (|x - G| - 2^-24 A)+ / (2^-24 S) over the entries with S > 0, largest |x| where S == 0); x [...,3,4] or the
    full [...,4,4] (whose bottom row is then held to exactly +0 by the caller)."""
    x = np.asarray(x, np.float64)[..., :3, :]
    err = np.abs(x - G)
    if A is not None:
        err = np.maximum(err - EPS24 * A, 0.0)
    nz = S > 0
    ratio = float((err[nz] / (EPS24 * S[nz])).max()) if nz.any() else 0.0
    if not np.isfinite(x).all():
        ratio = np.inf
    off = float(np.abs(x[~nz]).max()) if (~nz).any() else 0.0
    return ratio, off


@functools.lru_cache(maxsize=None)
def operator_k():
    """K of the operator level: 4 x the replay's worst ratio over every case."""
    k_ref = max(operator_reference(name)["k_ref"] for name in OPERATOR_CASES)
    assert K_REF_BAND_OPERATOR[0] < k_ref < K_REF_BAND_OPERATOR[1], k_ref
    return 4.0 * k_ref


def mutate_operator(name, kind):
    """A deliberately wrong operator-level result (float64 [C,3,4]) for the reference's own tests."""
    inp, ref = operator_inputs(name), operator_reference(name)
    if kind == "w_transposed":
        G = ref["G"].copy()
        G[:, :, :3] = np.swapaxes(G[:, :, :3], 1, 2)
        return G
    assert kind == "cov_dropped"
    # the mean enters through p_c = W m + t alone, so v_pc[n] = T[n][:, 3] and the term left is v_pc m^T
    v_pc = ref["T"][..., 3]
    G = np.zeros_like(ref["G"])
    G[:, :, 3] = v_pc.sum(1)
    G[:, :, :3] = np.einsum("cni,nj->cij", v_pc, inp["means"].astype(np.float64))
    return G


# ---- chain level ------------------------------------------------------------------------------------------------------------
def centre_vjp(V, g):
    """VJP of c = -R^T t: [3,4] block [-t g^T | -R g], in the dtype of the arguments (torch)."""
    R, t = V[:3, :3], V[:3, 3]
    return torch.cat([-(t[:, None] * g[None, :]), -(R @ g)[:, None]], dim=1)


def leaf_cameras(p, dtype):
    """(the case with stand-in cameras, their view matrices [C] and centres [C]: leaves of `dtype`)."""
    Vs = [c.viewmat.to(dtype).clone().requires_grad_(True) for c in p["cameras"]]
    ctrs = [c.camera_center.to(dtype).clone().requires_grad_(True) for c in p["cameras"]]
    cams = [types.SimpleNamespace(viewmat=V, K=c.K, camera_center=ctr, znear=c.znear, zfar=c.zfar, width=c.width, height=c.height)
            for c, V, ctr in zip(p["cameras"], Vs, ctrs)]
    return dict(p, cameras=cams), Vs, ctrs


def _camera_grads(Vs, ctrs):
    const = torch.stack([V.grad[:3, :] for V in Vs])
    assert all(not V.grad[3].any() for V in Vs)
    # (SH degree 0: the colours do not depend on the direction and the centre has no gradient at all)
    derived = torch.stack([V.grad[:3, :] + centre_vjp(V.detach(), torch.zeros_like(ctr) if ctr.grad is None else ctr.grad)
                           for V, ctr in zip(Vs, ctrs)])
    return {"constant": const.double().numpy(), "derived": derived.double().numpy()}


def chain_replay(p):
    """The float32 replay of the chain: {"constant" | "derived": dL/dV [C,3,4]} (float64 numpy of float32 values)."""
    p32, Vs, ctrs = leaf_cameras(p, torch.float32)
    PG.chain(p32, torch.float32)
    return _camera_grads(Vs, ctrs)


def carry_cameras(p, X, jac, jac_v, derived, absolute=True):
    """param_grad_f64.carry for the cameras: the operator-boundary rows X carried through the per-row Jacobians with respect
    to V (jac_v[c]: row_jacobians, numpy) and, where the centre is derived from V, through the colours' direction Jacobians
    of jac[c] (PG.jacobians) and d dir / d V = -d centre / d V; summed over n -> [C,3,4]."""
    f = np.abs if absolute else (lambda a: a)
    opac = p["opacities"].astype(np.float64).reshape(-1)
    out = []
    for c, (j, jv) in enumerate(zip(jac, jac_v)):
        rows = [X["means2d"][c, :, 0], X["means2d"][c, :, 1], X["colors"][c, :, 3], X["conics"][c, :, 0], X["conics"][c, :, 1],
                X["conics"][c, :, 2]]
        if p["antialiasing"]:
            rows.append(X["opacities"][c] * f(opac))
        vis = p["radii"][c] > 0
        acc = np.zeros((3, 4))
        for r, J in zip(rows, jv):
            acc += (f(J) * np.where(vis, r, 0.0)[:, None, None]).sum(0)
        if derived:
            V = p["cameras"][c].viewmat.detach().double().numpy()
            R, t = V[:3, :3], V[:3, 3]
            live = j["live"] & j["vis"][:, None]
            xc = np.where(live, X["colors"][c, :, :3], 0.0)
            for ch in range(3):
                d = j["dirs"][ch]                                                    # [N,3] d colour_ch / d dir
                Jd = np.concatenate([t[None, :, None] * d[:, None, :], (d @ R.T)[:, :, None]], axis=2)      # [N,3,4]
                acc += (f(Jd) * xc[:, ch, None, None]).sum(0)
        out.append(acc)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def chain_reference(case_id):
    """{"p": the case, "ref": PG.reference of it (the leaves' G, S, A), "G" | "S" | "A": {"constant" | "derived": [C,3,4]},
    "k_ref": the float32 replay's worst ratio over both centre modes, "carried": the signed carriage of the boundary
    gradients (must equal G: the reference's own test)}."""
    p = PG.make_case(case_id)
    p64, Vs, ctrs = leaf_cameras(p, torch.float64)
    ref = PG.reference(p64)                      # its chain's backward() leaves dL/dV and dL/dcentre on the leaves
    G = _camera_grads(Vs, ctrs)
    jac_v = []
    for cam in p["cameras"]:
        J = row_jacobians(p["means"], p["quats"], p["scales"], cam.viewmat, cam.K, p["width"], p["height"], torch.float64,
                          eps2d=PG.EPS2D, near_plane=cam.znear, far_plane=cam.zfar)
        jac_v.append([x.numpy() for x in J])
    rb = ref["boundary"]
    S, A, carried = {}, {}, {}
    for mode in ("constant", "derived"):
        S[mode] = carry_cameras(p, rb["S"], ref["jac"], jac_v, mode == "derived")
        A[mode] = carry_cameras(p, rb["A"], ref["jac"], jac_v, mode == "derived")
        carried[mode] = carry_cameras(p, rb["G"], ref["jac"], jac_v, mode == "derived", absolute=False)
    rep = chain_replay(p)
    k_ref = 0.0
    for mode in ("constant", "derived"):
        r, off = worst_ratio(rep[mode], G[mode], S[mode], A[mode])
        assert off == 0.0, (case_id, mode, off)
        k_ref = max(k_ref, r)
    return dict(p=p, ref=ref, G=G, S=S, A=A, k_ref=k_ref, carried=carried, replay=rep)


@functools.lru_cache(maxsize=None)
def chain_k():
    """K of the chain level: 4 x the replay's worst ratio over CHAIN_CASES and both centre modes."""
    k_ref = max(chain_reference(c)["k_ref"] for c in CHAIN_CASES)
    assert K_REF_BAND_CHAIN[0] <= k_ref < K_REF_BAND_CHAIN[1], k_ref
    return 4.0 * k_ref
