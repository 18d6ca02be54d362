"""GPU checks of the cube-map sampler (csrc/cubemap.hip through street_crafter_amd/cubemap.py and the nvdiffrast shim)
against the float64 reference of tests/cubemap_ref.py on the same fp32 inputs.

Forward, every sample, no exclusions:   |hip - f64| <= 2^-24 (k R L + 8 V),  L = max - min and V = max |value| of the
activated texture, k = 4 * K_FWD_REPLAY: four times what a float32 numpy replay of the same formula reaches.
Backward, every texel-channel:          |hip - f64| <= 2^-24 (n S + k_b (S + R A)),  n contributing samples, S the sum of
|terms|, A the sum of |g act'| over them, k_b = 4 * K_BWD_REPLAY; exactly 0 where no sample reaches.  Samples whose taps
the two precisions may place differently (cubemap_ref.excluded) get zero upstream gradient, at most 0.5 % of a case.

sky_color generates its directions in the kernel in fp32 from the fp32 matrix M: d_j = (M_j0 u + M_j1 v) + M_j2, each
component within e_j = 3 * 2^-24 (|M_j0 u| + |M_j1 v| + |M_j2|) of the exact value.  A face coordinate s = sc / ma then
moves by at most 2 max(e) / ma, the texel coordinate by R / 2 of that, and the sample, piecewise bilinear with slope at most
2 L per texel in each axis (L per texel inside a face; up to 1 / 0.75^2 < 2 times that where a corner tap is dropped and
the weights are renormalised), by at most 4 R L max(e) / ma over the two axes.  That term is added to the forward bar per
pixel, and its weight form A * 4 R max(e / ma) to the backward bar.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubemap_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = ref.EPS
K_FWD, K_BWD = 4.0 * ref.K_FWD_REPLAY, 4.0 * ref.K_BWD_REPLAY
H, W = 61, 37


@pytest.fixture(scope="module")
def cm():
    from street_crafter_amd import _lib, cubemap
    _lib.load()
    return cubemap


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(a).to(DEV, dtype)


def _hip(cm, tex, dirs, activation, g=None):
    """-> (out, grad_tex) as float64 numpy; grad_tex None without g."""
    t = _dev(tex).requires_grad_(g is not None)
    out = cm.texture_cube(t, _dev(dirs), activation)
    if g is not None:
        out.backward(_dev(g))
    return out.detach().cpu().numpy().astype(np.float64), None if g is None else t.grad.cpu().numpy().astype(np.float64)


def _bwd_bar(b, R, extra=0.0):
    return EPS * (b["n"] * b["S"] + K_BWD * (b["S"] + R * b["A"])) + extra * b["A"]


@pytest.mark.parametrize("C", ref.CHANNELS)
@pytest.mark.parametrize("R", ref.RESOLUTIONS)
def test_forward_is_within_the_bar_of_float64_everywhere(cm, R, C):
    tex = ref.texture(R, C)
    dirs = np.concatenate([ref.random_dirs(R), ref.adversarial_dirs(R), ref.invalid_dirs()])
    n_bad = len(ref.invalid_dirs())
    for activation in (None, "sigmoid"):
        tex_act = ref.activate(tex, activation)
        want = ref.sample(tex, dirs, activation)
        got, _ = _hip(cm, tex, dirs, activation)
        err = np.abs(got - want)
        print(f"R={R} C={C} {activation}: k reached {ref.forward_ratio(err[:-n_bad], tex_act, R):.3f} of {K_FWD:.2f}")
        assert (err <= ref.forward_bar(tex_act, R, K_FWD)).all()
        assert (got[-n_bad:] == 0).all() and not np.signbit(got[-n_bad:]).any()          # zero, NaN and Inf rows: exactly 0


@pytest.mark.parametrize("C", ref.CHANNELS)
@pytest.mark.parametrize("R", ref.RESOLUTIONS)
def test_backward_is_within_the_bar_per_texel_channel(cm, R, C):
    tex, dirs = ref.texture(R, C), ref.random_dirs(R)
    tp = ref.taps(dirs, R)
    out = ref.excluded(tp, R)
    assert out.mean() <= 0.005
    g = ref.upstream(len(dirs), C)
    g[out] = 0
    for activation in (None, "sigmoid"):
        b = ref.backward(tex, dirs, g, activation, tp=tp)
        _, grad = _hip(cm, tex, dirs, activation, g)
        grad = grad.reshape(-1, C)
        err, bar = np.abs(grad - b["grad"]), _bwd_bar(b, R)
        live = b["n"] > 0
        den = EPS * (b["S"] + R * b["A"])
        kb = ((err[live] - EPS * (b["n"] * b["S"])[live]) / den[live]).max()
        print(f"R={R} C={C} {activation}: k_b reached {kb:.3f} of {K_BWD:.2f}, excluded {out.mean():.5f}")
        assert (err <= bar).all()
        assert (grad[~live] == 0).all()


@pytest.mark.parametrize("R", ref.RESOLUTIONS)
def test_backward_on_the_adversarial_set_conserves_the_gradient_and_stays_in_the_footprint(cm, R):
    C = 3
    tex = ref.texture(R, C)
    dirs = np.concatenate([ref.adversarial_dirs(R), ref.invalid_dirs()])
    g = ref.upstream(len(dirs), C)
    _, grad = _hip(cm, tex, dirs, None, g)
    grad = grad.reshape(-1, C)
    tp = ref.taps(dirs, R)
    gv = g[tp["valid"]].astype(np.float64)
    n = int(tp["valid"].sum())
    assert (np.abs(grad.sum(axis=0) - gv.sum(axis=0)) <= n * EPS * np.abs(gv).sum(axis=0)).all()
    allowed = np.zeros(6 * R * R, bool)
    nb = ref.neighbourhood(tp, R)
    allowed[nb[nb >= 0]] = True
    assert (grad[~allowed] == 0).all()
    # per sample, on a texture-sized scratch of its own: nothing outside that sample's one-texel neighbourhood
    for i in np.random.default_rng(R).choice(np.flatnonzero(tp["valid"]), 24, replace=False):
        gi = np.zeros_like(g)
        gi[i] = 1.0
        _, one = _hip(cm, tex, dirs, None, gi)
        one = one.reshape(-1, C)
        ok = np.zeros(6 * R * R, bool)
        ok[nb[i][nb[i] >= 0]] = True
        assert (one[~ok] == 0).all() and abs(one[:, 0].sum() - 1.0) <= 8 * EPS


def _camera(seed=0):
    rng = np.random.default_rng(seed)
    K = np.array([[30.0, 0.0, W / 2 + 0.3], [0.0, 31.0, H / 2 - 0.2], [0.0, 0.0, 1.0]])      # wide: rays reach several faces
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    T = np.array([250.0, -30.0, 1200.0])
    return K, Q * np.sign(np.linalg.det(Q)), T


def _sky_reference(cm, K, Rm, perturb):
    """float64 directions from the fp32 matrix and the fp32 pixel positions the kernel forms -> (dirs [H*W,3], e / ma)."""
    M = cm.ray_matrix(K, Rm).astype(np.float32).astype(np.float64)
    px = np.tile(np.arange(W, dtype=np.float32), H)
    py = np.repeat(np.arange(H, dtype=np.float32), W)
    p = np.full((H * W, 2), 0.5, np.float32) if perturb is None else perturb.reshape(-1, 2)
    u, v = (px + p[:, 0]).astype(np.float64), (py + p[:, 1]).astype(np.float64)
    uv1 = np.stack([u, v, np.ones_like(u)], axis=1)
    d = uv1 @ M.T
    e = 3 * EPS * (np.abs(uv1)[:, None, :] * np.abs(M)[None, :, :]).sum(axis=2).max(axis=1)
    return d, e / np.abs(d).max(axis=1)


def _acc_map(seed):
    """fp32 [1,H,W] in [0,1] with a band of values at and around 1 - 1e-3, where (1 - acc) > 1e-3 flips."""
    rng = np.random.default_rng(seed)
    acc = rng.uniform(0, 1, (1, H, W)).astype(np.float32)
    acc[0, :, ::3] = 1.0
    edge = np.float32(1.0) - np.float32(1e-3)
    band = [edge, np.float32(0.999)]
    for start in (edge, np.float32(0.999)):
        lo = hi = start
        for _ in range(6):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(2))
            band += [lo, hi]
    flat = acc.reshape(-1)
    flat[: 8 * len(band)] = np.tile(np.array(band, np.float32), 8)
    return acc


_MASKS = ("none", "all_false", "all_true", "checker", "acc", "acc_band")


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("kind", _MASKS)
@pytest.mark.parametrize("R", [3, 16])
def test_sky_color_masks_fill_layout_and_gradient(cm, R, kind, white):
    K, Rm, T = _camera(R)
    tex = ref.texture(R, 3)
    rng = np.random.default_rng(R + len(kind))
    perturb = None if kind in ("all_true", "acc") else rng.uniform(0, 1, (H, W, 2)).astype(np.float32)
    kw, mask = {}, np.ones((H, W), bool)
    if kind in ("all_false", "all_true", "checker"):
        mask = {"all_false": np.zeros((H, W), bool), "all_true": np.ones((H, W), bool),
                "checker": (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(bool)}[kind]
        kw["sky_mask"] = _dev(mask)
    elif kind.startswith("acc"):
        acc = _acc_map(R) if kind == "acc_band" else np.random.default_rng(1).uniform(0.99, 1, (1, H, W)).astype(np.float32)
        kw["acc"] = _dev(acc)
        mask = ((1 - kw["acc"][0]) > 1e-3).cpu().numpy()              # torch's fp32 expression, sky_cubemap.py:88
        assert 0 < mask.sum() < mask.size
    if perturb is not None:
        kw["perturb"] = _dev(perturb)
    cube = _dev(tex).requires_grad_(True)
    out = cm.sky_color(cube, K, torch.tensor(Rm), T, H, W, white_background=white, **kw)
    assert out.shape == (3, H, W) and out.is_contiguous()
    got = out.detach().cpu().numpy().astype(np.float64).reshape(3, -1).T
    fill = 1.0 if white else 0.0
    # the mask decision, bit for bit: a sigmoid of logits in [-3, 3) is never 0 or 1
    assert np.array_equal((got != fill).all(axis=1), mask.reshape(-1))
    assert (got[~mask.reshape(-1)] == fill).all()
    dirs, e_rel = _sky_reference(cm, K, Rm, perturb)
    tex_act = ref.activate(tex, "sigmoid")
    L = float(tex_act.max() - tex_act.min())
    tp = ref.taps(dirs, R)
    want = ref.sample(tex, dirs, "sigmoid", tp=tp)
    m = mask.reshape(-1)
    bar = ref.forward_bar(tex_act, R, K_FWD) + 4 * R * L * e_rel
    assert (np.abs(got - want)[m] <= bar[m, None]).all()
    # backward: only masked pixels contribute, and to cube_map only
    g = ref.upstream(H * W, 3, seed=R)
    g[ref.excluded(tp, R)] = 0
    out.backward(_dev(np.ascontiguousarray(g.T.reshape(3, H, W))))
    grad = cube.grad.cpu().numpy().astype(np.float64).reshape(-1, 3)
    gm = g * m[:, None]
    b = ref.backward(tex, dirs, gm, "sigmoid", tp=tp)
    assert (np.abs(grad - b["grad"]) <= _bwd_bar(b, R, extra=4 * R * float(e_rel.max()))).all()
    assert (grad[b["n"] == 0] == 0).all()
    if kind == "all_false":
        assert (grad == 0).all()


def test_the_shim_runs_the_three_reference_call_shapes(cm):
    import nvdiffrast.torch as dr
    R, r = 8, 6
    tex = _dev(ref.texture(R, 3)).requires_grad_(True)
    rays = _dev(ref.random_dirs(R)[: H * W].reshape(H, W, 3))
    # sky_cubemap.py:102: the whole image
    a = dr.texture(tex[None, ...].sigmoid(), rays[None, ...], filter_mode="linear", boundary_mode="cube")
    assert a.shape == (1, H, W, 3) and torch.equal(a[0], cm.texture_cube(tex.detach().sigmoid(), rays))
    # :120: the masked rays as [1,1,N,3]
    sel = rays[torch.arange(H * W, device=DEV).reshape(H, W) % 3 == 0]
    bb = dr.texture(tex[None, ...].sigmoid(), sel[None, None, ...], filter_mode="linear", boundary_mode="cube")
    assert bb.shape == (1, 1, sel.shape[0], 3) and torch.equal(bb[0, 0], cm.texture_cube(tex.detach().sigmoid(), sel))
    # :205: the latlong grid of cubemap_to_latlong, [1,r,2r,3]
    gy, gx = torch.meshgrid(torch.linspace(0.0 + 1.0 / r, 1.0 - 1.0 / r, r, device=DEV),
                            torch.linspace(-1.0 + 1.0 / (2 * r), 1.0 - 1.0 / (2 * r), 2 * r, device=DEV), indexing="ij")
    refl = torch.stack((torch.sin(gy * np.pi) * torch.sin(gx * np.pi), torch.cos(gy * np.pi),
                        -torch.sin(gy * np.pi) * torch.cos(gx * np.pi)), dim=-1)
    c = dr.texture(tex[None, ...], refl[None, ...].contiguous(), filter_mode="linear", boundary_mode="cube")
    assert c.shape == (1, r, 2 * r, 3) and torch.equal(c[0], cm.texture_cube(tex.detach(), refl))
    want = ref.sample(tex.detach().cpu().numpy(), refl.reshape(-1, 3).cpu().numpy())
    assert np.abs(c[0].detach().cpu().numpy().reshape(-1, 3) - want).max() <= ref.forward_bar(tex.detach().cpu().numpy(), R, K_FWD)
    # a batch of directions against a texture batch of 1, 'auto' filtering; the gradient reaches the parameter
    d = dr.texture(tex[None, ...], torch.stack([rays, -rays]), boundary_mode="cube")
    assert d.shape == (2, H, W, 3) and torch.equal(d[1], cm.texture_cube(tex.detach(), -rays))
    a.sum().backward()
    direct = tex.detach().clone().requires_grad_(True)
    cm.texture_cube(direct, rays, "sigmoid").sum().backward()
    assert torch.allclose(tex.grad, direct.grad, rtol=1e-4, atol=1e-5)          # torch's sigmoid against the fused one


def test_the_ctypes_route_equals_the_compiled_binding_route(cm):
    from street_crafter_amd import _lib
    R, C = 8, 3
    tex, dirs = ref.texture(R, C), np.concatenate([ref.random_dirs(R)[:1024], ref.adversarial_dirs(R), ref.invalid_dirs()])
    g = ref.upstream(len(dirs), C)
    K, Rm, T = _camera(1)
    acc = _dev(_acc_map(2))

    def run():
        o, gr = _hip(cm, tex, dirs, "sigmoid", g)
        sky = cm.sky_color(_dev(tex), K, Rm, T, H, W, acc=acc, white_background=True).cpu().numpy()
        return o, gr, sky

    assert _lib.binding() is _lib.fast()
    fast = run()
    prev = _lib.set_fast_binding(False)
    try:
        assert _lib.fast() is None
        slow = run()
    finally:
        _lib.set_fast_binding(prev)
    assert np.array_equal(fast[0], slow[0]) and np.array_equal(fast[2], slow[2])
    b = ref.backward(tex, dirs, g, "sigmoid")
    assert (np.abs(fast[1] - slow[1]).reshape(-1, C) <= 2 * EPS * b["n"] * b["S"]).all()      # the order of the atomic adds


def test_a_checkpoint_cube_map_loads_and_renders(cm, tmp_path):
    from street_crafter_amd import scene_io
    from street_crafter_amd.scenes import make_scene
    cube = torch.from_numpy(ref.texture(4, 3))
    path = str(tmp_path / "it.pth")
    scene_io.save_checkpoint(path, [scene_io.scene_to_submodel(make_scene(16, seed=1), "background")],
                             extra={"sky_cubemap": {"params": {"sky_cube_map": cube}}})
    got = scene_io.load_sky_cubemap(path)
    assert torch.equal(got, cube)
    K, Rm, T = _camera(2)
    img = cm.sky_color(got.to(DEV), K, Rm, T, H, W, white_background=False)
    assert img.shape == (3, H, W) and bool(((img > 0) & (img < 1)).all())
    five = cm.texture_cube(got.to(DEV)[None], torch.ones(2, 5, 3, device=DEV))          # [1,6,R,R,C] and [...,3]
    assert five.shape == (2, 5, 3)
