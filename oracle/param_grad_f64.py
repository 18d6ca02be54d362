"""The training step's parameter gradients in float64 with per-row error scales -- TEST INFRASTRUCTURE ONLY.

What the optimiser receives (means, quats, scales, opacities, sh through `harness/caller.py::render_gaussians(mode=
"train")` / `rasterization()`) is judged here as ONE chain: projection -> opacity * compensation -> SH colours of
dirs = means - camera centre under masks = radii > 0 -> clamp_min(colours + 0.5, 0) -> depth as the extra colour
channel -> rasterize -> loss = sum(w_rgb rgb) + sum(w_acc acc) + sum(w_depth depth), depth = channel 3 / acc.

`make_case(case_id)`    float32 leaves, camera(s), loss weights, and the FACTS of the float32 forward from the numpy
                        oracle (oracle/gsplat_oracle.py): radii, isect_offsets, flatten_ids, the operator-boundary
                        tensors and the unstable-pixel mask (RB.unstable_bwd).  The kernels are bit-exact with that
                        oracle on the integers, so the GPU test asserts the lists and judges the same ones.  The weights
                        are zero on the unstable pixels, and w_depth also where acc < 0.05 (the division by a small alpha
                        is the caller's torch arithmetic, not a kernel's).
`chain(p, dtype)`       the caller's train sequence restated over oracle/gsplat_torch.py with the fixed lists and masks,
                        one single-camera oracle call per camera; torch.float64 = the reference, torch.float32 = the
                        noise-floor replay (no kernel involved) the tests take K from; `mutate` = one deliberately wrong
                        variant of the glue (for the reference's own tests).
`reference(p)`          per leaf the gradient G (float64 autograd), v_means2d (-> viewspace_points.grad), and the two row
                        scales S and A of the bar   |x - G| <= 2^-24 (K S + A),  exactly 0 where S == 0.

S and A: those of RB.rasterize_bwd at the operator boundary (the upstream v_render_colors / v_render_alphas read from
the float64 chain), carried to the leaves through the ABSOLUTE VALUE of the per-Gaussian Jacobians.  The Gaussians are
independent, so the projection's Jacobians come from seven float64 backward calls per camera with a unit upstream on
one output at a time (means2d x, y; depth; three conic entries; compensation) and the colours' from three.  Per
projection output: means2d and conics take their own scales, depth takes the scale of the depth colour channel, the
compensation takes S_opacities |opacity|; the direction path into means is sum_ch |d colour_ch / d dir| S_colors[ch]
over the channels the clamp leaves live; opacities: S_opacities |comp|; sh: |Y_k| (monomial table, oracle/sh_bwd_f64.py)
times S_colors.  `carry(..., absolute=False)` runs the SAME code with signed Jacobians on G: it must give autograd's
total, which is how tests/test_param_grad_ref_cpu.py checks the carriage.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np
import torch

from oracle import gsplat_oracle as O
from oracle import gsplat_torch as OT
from oracle import raster_bwd_f64 as RB
from oracle import sh_bwd_f64 as SH

LEAVES = ("means", "quats", "scales", "opacities", "sh")
JUDGED = LEAVES + ("means2d",)
TILE = 16
EPS2D = 0.3
ACC_MIN = 0.05
CLAMP_WINDOW = 1e-5
# The replay's K_ref is not a rounding count: it is the conditioning of the float32 forward the backward starts from.  An
# alpha moves by |a dx + b dy| |d mean2d| (relative) when its mean2d is rounded; |a dx| <= 3 / sigma_px at the 3-sigma
# cut, sigma_px >= sqrt(eps2d) = 0.55 px, |d mean2d| <= a few 2^-24 x 160 px: some hundreds of 2^-24 on the worst row of
# a frame this size.  Below 1 the replay would be exact (it is float32).  The upper limit is about twice what the replay
# reaches on the committed cases (725 or 803, always a quats row: torch's float32 summation order differs between hosts):
# K = 4 K_ref is ONE number for all rows of all cases, so a new or drifting case that doubles it loosens every other case's
# bar and is ill-conditioned, not noisy.
K_REF_BAND = (1.0, 1500.0)
MUTATIONS = ("comp_detached", "depth_detached", "dir_detached", "conic_b_halved", "clamp_ignored")

_PLAIN_CAM = dict(width=160, height=96, fx=180.0, fy=180.0, yaw=0.1)
_PLAIN_SCENE = dict(n=2500, seed=2, z_range=(1.0, 30.0), scale_range=(0.02, 0.3))
# case -> scene (make_scene keywords | "street" | "side": plus Gaussians beyond the Jacobian clamp), sh_degree, cameras,
# antialiasing, leaves that do not require grad
CASES = {
    "plain": dict(scene=_PLAIN_SCENE, sh_degree=2, cams=(_PLAIN_CAM,)),
    "ragged": dict(scene=dict(n=2200, seed=6, z_range=(1.0, 30.0), scale_range=(0.02, 0.3)), sh_degree=1,
                   cams=(dict(width=150, height=90, fx=170.0, fy=175.0, yaw=-0.05),)),
    "deg0": dict(scene=dict(n=2000, seed=7, z_range=(1.0, 30.0), scale_range=(0.02, 0.3)), sh_degree=0, cams=(_PLAIN_CAM,)),
    "deg3": dict(scene=dict(n=2000, seed=8, z_range=(1.0, 30.0), scale_range=(0.02, 0.3)), sh_degree=3, cams=(_PLAIN_CAM,)),
    "classic": dict(scene=_PLAIN_SCENE, sh_degree=2, cams=(_PLAIN_CAM,), antialiasing=False),
    "clamped": dict(scene=dict(n=1800, seed=9, z_range=(1.0, 30.0), scale_range=(0.02, 0.3)), side=(300, 10), sh_degree=1,
                    cams=(dict(width=160, height=96, fx=180.0, fy=180.0, yaw=0.0),)),
    "street": dict(scene="street", sh_degree=1, cams=(dict(width=160, height=100, fx=170.0, fy=170.0, yaw=0.0),)),
    "two_cameras": dict(scene=dict(n=2500, seed=11, x_span=0.9, y_span=0.5, z_range=(1.0, 30.0), scale_range=(0.02, 0.3)),
                        sh_degree=2,
                        cams=(dict(width=160, height=96, fx=180.0, fy=180.0, yaw=0.1),
                              dict(width=160, height=96, fx=150.0, fy=165.0, yaw=-0.25, shift=(0.5, 0.1, -0.3),
                                   principal=(0.42, 0.55)))),
    "frozen": dict(scene=_PLAIN_SCENE, sh_degree=2, cams=(_PLAIN_CAM,), frozen=("quats", "sh")),
}
CASE_IDS = tuple(CASES)


def _scene(spec):
    from street_crafter_amd.scenes import Scene, make_scene, make_street_scene
    deg = spec["sh_degree"]
    if spec["scene"] == "street":
        return make_street_scene(1500, seed=1, sh_degree=deg)[0]
    sc = make_scene(sh_degree=deg, **spec["scene"])
    if "side" in spec:
        # wide Gaussians beyond the clamp limit of x/z (and a third of them of y/z too) that still reach the frame: their
        # EWA Jacobian is evaluated AT the limit (tools/make_golden.py::projection_bwd_case does the same for the operator)
        n, seed = spec["side"]
        cam = spec["cams"][0]
        ex = make_scene(n, sh_degree=deg, seed=seed, z_range=(2.0, 20.0), scale_range=(0.2, 1.0))
        g = torch.Generator().manual_seed(seed)
        m = ex.means.clone()
        limx, limy = 1.3 * 0.5 * cam["width"] / cam["fx"], 1.3 * 0.5 * cam["height"] / cam["fy"]
        side = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        m[:, 0] = m[:, 2] * side * (limx + 0.02 + 0.2 * torch.rand(n, generator=g))
        m[::3, 1] = m[::3, 2] * (limy + 0.02 + 0.1 * torch.rand(m[::3].shape[0], generator=g))
        ex.opacities.mul_(0.5)
        sc = Scene(*(torch.cat([a, b]).contiguous() for a, b in ((sc.means, m), (sc.quats, ex.quats), (sc.scales, ex.scales),
                                                                  (sc.opacities, ex.opacities), (sc.sh, ex.sh))), deg)
    return sc


def _camera(c):
    from street_crafter_amd.scenes import make_camera
    cam = make_camera(c["width"], c["height"], c["fx"], c["fy"], yaw=c.get("yaw", 0.0), shift=c.get("shift", (0.0, 0.0, 0.0)))
    if "principal" in c:
        K = cam.K.clone()
        K[0, 2], K[1, 2] = c["principal"][0] * c["width"], c["principal"][1] * c["height"]
        cam.K = K
    return cam


def _build_case(case_id, centers=None, leaves=None):
    spec = CASES[case_id]
    sc = _scene(spec)
    cams = [_camera(c) for c in spec["cams"]]
    if centers is not None:
        for cam, ctr in zip(cams, np.asarray(centers, np.float32).reshape(len(cams), 3)):
            cam.camera_center = torch.from_numpy(ctr.copy())
    W, H = cams[0].width, cams[0].height
    aa = spec.get("antialiasing", True)
    deg = spec["sh_degree"]
    own = dict(means=sc.means.numpy(), quats=sc.quats.numpy(), scales=sc.scales.numpy(), opacities=sc.opacities.numpy(),
               sh=sc.sh.numpy())
    if leaves is not None:      # the case on other leaves of the same shapes (oracle/poison_cases.py grafts rows into it)
        assert set(leaves) == set(own) and all(leaves[k].shape == own[k].shape and leaves[k].dtype == np.float32 for k in own)
    leaves = own if leaves is None else {k: np.ascontiguousarray(leaves[k]) for k in LEAVES}
    per = []
    for cam in cams:
        radii, m2, d, con, comp = O.fully_fused_projection(leaves["means"], leaves["quats"], leaves["scales"], cam.viewmat.numpy(),
                                                           cam.K.numpy(), W, H, eps2d=EPS2D, near_plane=cam.znear,
                                                           far_plane=cam.zfar, calc_compensations=aa)
        op = leaves["opacities"].reshape(-1)
        if aa:
            op = op * comp
        dirs = leaves["means"] - cam.camera_center.numpy()[None]
        col = O.spherical_harmonics(deg, dirs, leaves["sh"], masks=radii > 0)
        pre = col + np.float32(0.5)
        col4 = np.concatenate([np.maximum(pre, np.float32(0.0)), d[:, None]], axis=-1)
        per.append((radii, m2, d, con, comp, op.astype(np.float32), col4.astype(np.float32), pre))
    radii, m2, d, con, comp, op, col4, pre = (np.stack(x) for x in zip(*per))
    C = len(cams)
    tw, th = math.ceil(W / TILE), math.ceil(H / TILE)
    _, ids, fids = O.isect_tiles(m2, radii, d, TILE, tw, th, n_cameras=C)
    offs = O.isect_offset_encode(ids, C, tw, th)
    un = RB.unstable_bwd(m2, con, col4, op, W, H, TILE, offs, fids)
    acc = O.rasterize_to_pixels(m2, con, col4, op, W, H, TILE, offs, fids)[1][..., 0]
    rng = np.random.default_rng(5000 + CASE_IDS.index(case_id))
    w_rgb = rng.normal(size=(C, H, W, 3)).astype(np.float32)
    w_acc = rng.normal(size=(C, H, W)).astype(np.float32)
    w_depth = (0.1 * rng.normal(size=(C, H, W))).astype(np.float32)
    w_rgb[un] = 0.0
    w_acc[un] = 0.0
    w_depth[un | (acc < ACC_MIN)] = 0.0
    return dict(case=case_id, **leaves, sh_degree=deg, antialiasing=aa, frozen=tuple(spec.get("frozen", ())), cameras=cams,
                width=W, height=H, tile_size=TILE, radii=radii, means2d=m2, depths=d, conics=con, compensations=comp,
                opacities2d=op, colors=col4, colors_pre_clamp=pre, isect_offsets=offs, flatten_ids=fids, unstable=un,
                w_rgb=w_rgb, w_acc=w_acc, w_depth=w_depth)


_make_case = lru_cache(maxsize=None)(_build_case)


def make_case(case_id, centers=None):
    """centers (optional float32 [C,3]): the camera positions the float32 forward used where they are not the cameras' own
    `camera_center` -- `rasterization()` without `camera_centers_` derives them from the view matrices in float32.  Like
    the tile lists they are then a FACT of that forward: the colours, the unstable pixels and the whole chain are rebuilt
    on them, and how far they may be from -R^T t is the caller's to judge."""
    if centers is None:
        return dict(_make_case(case_id))
    return _build_case(case_id, centers)


def with_leaves(case_id, leaves):
    """The case rebuilt on other float32 leaves of the same shapes: cameras and the random part of the loss weights are the
    case's own, every fact of the float32 forward (radii, lists, colours, unstable pixels) is recomputed."""
    return _build_case(case_id, None, leaves)


def _half_grad(x):
    """x by value, half of its gradient."""
    return 0.5 * x + 0.5 * x.detach()


def _camera_ops(p, c, L, dtype, mutate=None):
    """One camera of the chain up to the rasterizer's inputs -> dict of [N,*] tensors (graph attached to the leaves L)."""
    cam = p["cameras"][c]
    V, K, ctr = cam.viewmat.to(dtype), cam.K.to(dtype), cam.camera_center.to(dtype)
    radii, m2, d, con, comp = OT.fully_fused_projection(L["means"], L["quats"], L["scales"], V, K, p["width"], p["height"],
                                                        eps2d=EPS2D, near_plane=cam.znear, far_plane=cam.zfar)
    vis = torch.from_numpy(p["radii"][c] > 0)
    op = L["opacities"][:, 0]
    if p["antialiasing"]:
        op = op * (comp.detach() if mutate == "comp_detached" else comp)
    dirs = L["means"] - ctr
    if mutate == "dir_detached":
        dirs = dirs.detach()
    # (a culled row's colour is never evaluated by the operator: the oracle multiplies by the mask, which needs a finite
    #  value to multiply -- every direction here is non-zero)
    pre = OT.spherical_harmonics(p["sh_degree"], dirs, L["sh"], masks=vis) + 0.5
    col = torch.clamp_min(pre, 0.0)
    if mutate == "clamp_ignored":
        col = pre + (col - pre).detach()
    if mutate == "conic_b_halved":
        con = torch.stack([con[:, 0], _half_grad(con[:, 1]), con[:, 2]], dim=-1)
    dd = d.detach() if mutate == "depth_detached" else d
    return dict(radii=radii, means2d=m2, depths=d, conics=con, comp=comp, opacities=op, pre=pre,
                colors=torch.cat([col, dd[:, None]], dim=-1))


def _leaves(p, dtype):
    return {k: torch.from_numpy(p[k]).to(dtype).requires_grad_(True) for k in LEAVES}


def chain(p, dtype=torch.float64, mutate=None, keep=False):
    """-> {"G": {leaf: gradient, "means2d": v_means2d [C,N,2]}} (float64 numpy); keep: also "boundary" (the rasterizer's
    inputs and the upstream gradients of its outputs, float64 numpy), "radii" [C,N] and "acc" [C,H,W] of THIS chain."""
    assert mutate is None or mutate in MUTATIONS, mutate
    L = _leaves(p, dtype)
    C = len(p["cameras"])
    per = [_camera_ops(p, c, L, dtype, mutate) for c in range(C)]
    m2, con, col, op = (torch.stack([q[k] for q in per]) for k in ("means2d", "conics", "colors", "opacities"))
    m2.retain_grad()
    rc, ra = OT.rasterize_to_pixels(m2, con, col, op, p["width"], p["height"], p["tile_size"],
                                    torch.from_numpy(p["isect_offsets"]), torch.from_numpy(p["flatten_ids"]))
    rc.retain_grad()
    ra.retain_grad()
    w = {k: torch.from_numpy(p[k]).to(dtype) for k in ("w_rgb", "w_acc", "w_depth")}
    depth = rc[..., 3] / ra[..., 0].clamp(min=1e-10)
    ((rc[..., :3] * w["w_rgb"]).sum() + (ra[..., 0] * w["w_acc"]).sum() + (depth * w["w_depth"]).sum()).backward()
    G = {k: (np.zeros(tuple(L[k].shape)) if L[k].grad is None else L[k].grad.double().numpy()) for k in LEAVES}
    G["means2d"] = m2.grad.double().numpy()
    out = {"G": G}
    if keep:
        out["boundary"] = dict(means2d=m2.detach().double().numpy(), conics=con.detach().double().numpy(),
                               colors=col.detach().double().numpy(), opacities=op.detach().double().numpy(),
                               v_render_colors=rc.grad.double().numpy(), v_render_alphas=ra.grad.double().numpy())
        out["radii"] = np.stack([q["radii"].numpy() for q in per])
        out["acc"] = ra.detach().double().numpy()[..., 0]
    return out


def jacobians(p, c):
    """Camera c in float64: {"proj": [7] x [N,10] d output / d (means 3, quats 4, scales 3), outputs in the order means2d
    x, y, depth, conic a, b, c, compensation; "dirs": [3] x [N,3] d (colour_ch before the clamp) / d dir; "live": bool[N,3]
    the channels the clamp passes; "comp" [N]; "vis" bool[N]; "u" [N,3] the unit directions} -- numpy."""
    L = _leaves(p, torch.float64)
    q = _camera_ops(p, c, L, torch.float64)
    outs = (q["means2d"][:, 0], q["means2d"][:, 1], q["depths"], q["conics"][:, 0], q["conics"][:, 1], q["conics"][:, 2], q["comp"])
    src = (L["means"], L["quats"], L["scales"])
    proj = []
    for o in outs:
        g = torch.autograd.grad(o.sum(), src, retain_graph=True, allow_unused=True)
        proj.append(np.concatenate([np.zeros(tuple(s.shape)) if x is None else x.numpy() for x, s in zip(g, src)], axis=1))
    # the colours' dependence on the direction alone (the mean enters the projection separately)
    ctr = p["cameras"][c].camera_center.double()
    dirs = (L["means"].detach() - ctr).requires_grad_(True)
    vis = torch.from_numpy(p["radii"][c] > 0)
    pre = OT.spherical_harmonics(p["sh_degree"], dirs, L["sh"].detach(), masks=vis) + 0.5
    dj = []
    for ch in range(3):
        if p["sh_degree"] == 0:
            dj.append(np.zeros((dirs.shape[0], 3)))
        else:
            dj.append(torch.autograd.grad(pre[:, ch].sum(), dirs, retain_graph=True)[0].numpy())
    dn = dirs.detach().numpy()
    return dict(proj=proj, dirs=dj, live=(pre.detach().numpy() > 0), comp=q["comp"].detach().numpy(), vis=vis.numpy(),
                u=dn / np.sqrt((dn * dn).sum(-1, keepdims=True)))


def carry(p, X, jac, absolute=True, paths=None):
    """The operator-boundary rows X = {means2d [C,N,2], conics [C,N,3], colors [C,N,4], opacities [C,N]} carried to the
    leaves through the per-Gaussian Jacobians `jac` (one jacobians() per camera), summed over the cameras.
    absolute=True: |Jacobian| -- X are scales (S or A); False: signed -- X are gradients and the result is the chain rule.
    paths (optional dict): filled with every path's contribution to `means` by name."""
    f = np.abs if absolute else (lambda a: a)
    N = p["means"].shape[0]
    K = (p["sh_degree"] + 1) ** 2
    out = dict(means=np.zeros((N, 3)), quats=np.zeros((N, 4)), scales=np.zeros((N, 3)), opacities=np.zeros((N, 1)),
               sh=np.zeros((N, K, 3)))
    opac = p["opacities"].astype(np.float64).reshape(-1)
    for c, j in enumerate(jac):
        rows = [X["means2d"][c, :, 0], X["means2d"][c, :, 1], X["colors"][c, :, 3], X["conics"][c, :, 0], X["conics"][c, :, 1],
                X["conics"][c, :, 2]]
        names = ["means2d", "means2d", "depth", "conics", "conics", "conics"]
        if p["antialiasing"]:
            rows.append(X["opacities"][c] * f(opac))
            names.append("compensation")
        for r, J, name in zip(rows, j["proj"], names):
            t = f(J) * r[:, None]
            out["means"] += t[:, :3]
            out["quats"] += t[:, 3:7]
            out["scales"] += t[:, 7:]
            if paths is not None:
                paths[name] = paths.get(name, 0.0) + t[:, :3]
        live = j["live"] & j["vis"][:, None]
        xc = np.where(live, X["colors"][c, :, :3], 0.0)
        t = sum(f(j["dirs"][ch]) * xc[:, ch:ch + 1] for ch in range(3))
        out["means"] += t
        if paths is not None:
            paths["direction"] = paths.get("direction", 0.0) + t
        out["opacities"][:, 0] += X["opacities"][c] * (f(j["comp"]) if p["antialiasing"] else j["vis"].astype(np.float64))
        Y = SH.basis(p["sh_degree"], j["u"], absolute=absolute)[0]
        out["sh"] += Y[:, :, None] * xc[:, None, :]
    return out


def reference(p):
    """-> {"G", "S", "A"}: dicts over JUDGED (the five leaves and "means2d" = v_means2d [C,N,2]), float64 numpy; plus
    "radii" / "acc" of the float64 chain, "boundary" = RB.rasterize_bwd's own result and "jac" (the tests of the
    reference itself read them)."""
    ch = chain(p, torch.float64, keep=True)
    b = ch["boundary"]
    rb = RB.rasterize_bwd(b["means2d"], b["conics"], b["colors"], b["opacities"], p["width"], p["height"], p["tile_size"],
                          p["isect_offsets"], p["flatten_ids"], b["v_render_colors"], b["v_render_alphas"], stored_means2d=True)
    jac = [jacobians(p, c) for c in range(len(p["cameras"]))]
    S = carry(p, rb["S"], jac)
    A = carry(p, rb["A"], jac)
    S["means2d"], A["means2d"] = rb["S"]["means2d"], rb["A"]["means2d"]
    return {"G": ch["G"], "S": S, "A": A, "radii": ch["radii"], "acc": ch["acc"], "boundary": rb, "jac": jac}


def worst_ratios(x, ref, names=JUDGED):
    """{name: (largest per-row ratio (|x - G| - 2^-24 A)+ / (2^-24 S), largest |x| where S == 0)}."""
    out = {}
    for k in names:
        r, off = RB.row_ratio(x[k], ref, k)
        out[k] = (float(r.max()) if r.size else 0.0, off)
    return out


def clamp_limit_margin(p):
    """Smallest relative distance of any visible Gaussian's x/z, y/z (float64) from the Jacobian clamp limit, and the number
    of visible Gaussians beyond it."""
    best, beyond = np.inf, 0
    for c, cam in enumerate(p["cameras"]):
        V, K = cam.viewmat.double().numpy(), cam.K.double().numpy()
        x = p["means"].astype(np.float64) @ V[:3, :3].T + V[:3, 3]
        vis = p["radii"][c] > 0
        lim = (1.3 * 0.5 * p["width"] / K[0, 0], 1.3 * 0.5 * p["height"] / K[1, 1])
        t = np.stack([np.abs(x[vis, 0] / x[vis, 2]) / lim[0], np.abs(x[vis, 1] / x[vis, 2]) / lim[1]], -1)
        best = min(best, float(np.abs(t - 1.0).min()))
        beyond += int((t > 1.0).any(-1).sum())
    return best, beyond
