"""No-GPU checks of the cube-map sampler: the float64 reference of tests/cubemap_ref.py against the properties the
definition promises, the float32 replay constants the GPU bars are built from, the ray matrix, the `nvdiffrast` shim's
import and refusals, the C ABI's argument checks and the checkpoint reader.

The product exposes no edge table to Python (csrc/cubemap.hip re-projects the tap centre in exact integers), so there is
no table to compare with the re-projection here; test_cubemap_gpu.py compares the kernel's taps with it instead."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubemap_ref as ref  # noqa: E402


def _centres(R):
    """Directions of every texel centre: [6,R,R,3], index order (face, y, x)."""
    c = (2.0 * (np.arange(R) + 0.5) / R - 1.0)
    t, s = np.meshgrid(c, c, indexing="ij")
    out = np.empty((6, R, R, 3))
    for f in range(6):
        x, y, z = ref.face_to_dir(np.full(s.shape, f), s, t)
        out[f] = np.stack([x, y, z], axis=-1)
    return out


def _tex64(R, C, seed=0):
    return np.random.default_rng(seed + R).uniform(-3, 3, (6, R, R, C))


@pytest.mark.parametrize("R", [2, 3, 8])
def test_every_texel_centre_samples_exactly_that_texel(R):
    tex = _tex64(R, 2)
    for scale in (1.0, 3.7):
        dirs = _centres(R).reshape(-1, 3) * scale
        tp = ref.taps(dirs, R)
        # (for R = 3 a centre is no float64 number: the texel gets all of the weight but a few 2^-53)
        top = tp["w"].argmax(axis=1)
        assert np.array_equal(tp["idx"][np.arange(len(dirs)), top], np.arange(6 * R * R))
        assert (tp["w"].max(axis=1) >= 1.0 - 8 * 2.0 ** -53 * R).all()
        got = ref.sample(tex, dirs, tp=tp)
        if R != 3:
            assert np.array_equal(got, tex.reshape(-1, 2))
        assert np.abs(got - tex.reshape(-1, 2)).max() <= 6.0 * 16 * 2.0 ** -53 * R


@pytest.mark.parametrize("R", [2, 3, 8])
def test_constant_map_is_constant_and_weights_sum_to_one(R):
    dirs = np.concatenate([ref.corner_dirs(), ref.edge_dirs(), ref.adversarial_dirs(R), ref.random_dirs(R)]).astype(np.float64)
    tp = ref.taps(dirs, R)
    assert tp["valid"].all()
    assert np.abs(tp["w"].sum(axis=1) - 1.0).max() < 1e-15
    assert (tp["w"] >= 0).all() and ((tp["idx"] >= 0) | (tp["w"] == 0)).all()
    tex = np.full((6, R, R, 3), 0.625)
    assert np.abs(ref.sample(tex, dirs, tp=tp) - 0.625).max() < 1e-15
    # the 8 corners drop one tap and keep three, each from another face
    tc = ref.taps(ref.corner_dirs().astype(np.float64), R)
    assert ((tc["idx"] < 0).sum(axis=1) == 1).all()
    for row in tc["idx"]:
        assert len({int(i) // (R * R) for i in row if i >= 0}) == 3
    # the 12 edge midpoints weigh the two faces equally
    te = ref.taps(ref.edge_dirs().astype(np.float64), R)
    for idx, w in zip(te["idx"], te["w"]):
        by_face = {}
        for i, ww in zip(idx, w):
            by_face[int(i) // (R * R)] = by_face.get(int(i) // (R * R), 0.0) + ww
        assert sorted(by_face.values()) == [0.5, 0.5]


@pytest.mark.parametrize("R", [2, 3, 8])
def test_value_is_continuous_across_face_edges_and_texel_boundaries(R):
    """Stepping 1e-9 across every face edge (j = 0, R) and every texel boundary changes the sample by < 1e-7 * range."""
    tex = _tex64(R, 3, seed=4)
    rng_ = float(tex.max() - tex.min())
    b = 2.0 * np.arange(R + 1) / R - 1.0
    half = 2.0 * (np.arange(2 * R + 1)) / (2 * R) - 1.0          # boundaries and centres of the other axis
    other = np.concatenate([half, half[1:-1] + 1e-9, half[1:-1] - 1e-9, np.random.default_rng(R).uniform(-1, 1, 16)])
    worst = 0.0
    for f in range(6):
        s, t = (a.ravel() for a in np.meshgrid(b, other, indexing="ij"))
        for swap in (False, True):
            lo = ref.face_to_dir(np.full(s.size, f), *((t, s - 1e-9) if swap else (s - 1e-9, t)))
            hi = ref.face_to_dir(np.full(s.size, f), *((t, s + 1e-9) if swap else (s + 1e-9, t)))
            a = ref.sample(tex, np.stack(lo, axis=1))
            c = ref.sample(tex, np.stack(hi, axis=1))
            worst = max(worst, float(np.abs(a - c).max()))
    assert worst < 1e-7 * rng_, worst / rng_


def _rotations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            Q = np.zeros((3, 3))
            for r in range(3):
                Q[r, perm[r]] = signs[r]
            if np.linalg.det(Q) > 0:
                out.append(Q)
    return out


@pytest.mark.parametrize("R", [2, 3, 8])
def test_the_24_rotations_of_the_cube_commute_with_sampling(R):
    rots = _rotations()
    assert len(rots) == 24
    tex = _tex64(R, 2, seed=9)
    dirs = np.concatenate([ref.random_dirs(R)[:512], ref.adversarial_dirs(R)]).astype(np.float64)
    want = ref.sample(tex, dirs)
    centres = _centres(R).reshape(-1, 3)
    for Q in rots:
        # the rotated texture: its texel with centre c holds the original texel with centre Q^T c
        src = ref.taps(centres @ Q, R)                       # rows of (centres @ Q) are Q^T c
        assert (src["w"].max(axis=1) >= 1.0 - 8 * 2.0 ** -53 * R).all()
        texel = src["idx"][np.arange(len(centres)), src["w"].argmax(axis=1)]
        assert sorted(texel.tolist()) == list(range(6 * R * R))
        rotated = tex.reshape(-1, 2)[texel].reshape(tex.shape)
        got = ref.sample(rotated, dirs @ Q.T)
        assert np.abs(got - want).max() < 1e-12


def test_the_replay_constants_are_what_a_fresh_float32_replay_reaches():
    k, kb = ref.replay_constants()
    assert 0.75 * ref.K_FWD_REPLAY <= k <= ref.K_FWD_REPLAY, k
    assert 0.75 * ref.K_BWD_REPLAY <= kb <= ref.K_BWD_REPLAY, kb


def test_the_exclusion_of_the_backward_test_stays_under_its_cap():
    for R in ref.RESOLUTIONS:
        share = ref.excluded(ref.taps(ref.random_dirs(R), R), R).mean()
        assert share <= 0.005, (R, share)


def test_ray_matrix_gives_the_ray_direction_of_the_camera_model():
    """M (u, v, 1) with M = R^T K^-1 against the direction the reference's ray generation forms in float64: the pixel's
    camera-space point K^-1 p, moved to the world as R^T (p_cam - T), minus the camera origin -R^T T."""
    from street_crafter_amd.cubemap import ray_matrix
    rng = np.random.default_rng(3)
    K = np.array([[1234.5, 0.0, 801.25], [0.0, 1240.75, 530.5], [0.0, 0.0, 1.0]])
    Rm, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    T = np.array([312.5, -48.0, 1907.0])
    M = ray_matrix(torch.tensor(K), Rm)
    uv1 = np.concatenate([rng.uniform(0, 1600, (64, 2)), np.ones((64, 1))], axis=1)
    cam = uv1 @ np.linalg.inv(K).T
    world = (cam - T) @ Rm
    origin = -(Rm.T @ T)
    want = world - origin
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    got = uv1 @ M.T
    got /= np.linalg.norm(got, axis=1, keepdims=True)
    assert np.abs(got - want).max() < 1e-11
    with pytest.raises(ValueError):
        ray_matrix(np.eye(4), np.eye(3))


def test_nvdiffrast_imports_and_refuses_what_it_does_not_implement():
    import nvdiffrast.torch as dr
    tex, uv = torch.zeros(1, 6, 4, 4, 3), torch.zeros(1, 2, 2, 3)
    with pytest.raises(NotImplementedError, match="latlong_to_cubemap"):
        dr.texture(torch.zeros(1, 4, 8, 3), torch.zeros(1, 2, 2, 2), filter_mode="linear")        # the 2-D wrap case
    with pytest.raises(NotImplementedError, match="filter_mode"):
        dr.texture(tex, uv, filter_mode="nearest", boundary_mode="cube")
    for kw in (dict(uv_da=uv), dict(mip_level_bias=uv), dict(mip=[tex]), dict(max_mip_level=2)):
        with pytest.raises(NotImplementedError, match="mip"):
            dr.texture(tex, uv, boundary_mode="cube", **kw)
    with pytest.raises(ValueError, match="HIP device"):
        dr.texture(tex, uv, filter_mode="linear", boundary_mode="cube")
    with pytest.raises(ValueError, match=r"\[B,6,R,R,C\]"):
        dr.texture(tex[0], uv, boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="rasterize"):
        dr.rasterize(None, None, None, None)


def test_cubemap_operators_refuse_cpu_tensors_and_bad_shapes():
    from street_crafter_amd.cubemap import sky_color, texture_cube
    with pytest.raises(ValueError, match="HIP device"):
        texture_cube(torch.zeros(6, 4, 4, 3), torch.zeros(5, 3))
    with pytest.raises(ValueError, match="HIP device"):
        sky_color(torch.zeros(6, 4, 4, 3), np.eye(3), np.eye(3), np.zeros(3), 4, 4, white_background=False)
    with pytest.raises(TypeError):
        texture_cube(np.zeros((6, 4, 4, 3)), torch.zeros(5, 3))
    # shape and dtype checks come after the device check, so they are exercised on the meta of fake device tensors
    dev = torch.device("meta")

    class _Fake(torch.Tensor):
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=dev).as_subclass(_Fake)

    for bad in (fake(6, 1, 1, 3), fake(6, 4, 5, 3), fake(5, 4, 4, 3), fake(6, 4, 4, 5), fake(2, 6, 4, 4, 3),
                fake(6, 4, 4, 3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            texture_cube(bad, fake(5, 3))
    with pytest.raises(ValueError):
        texture_cube(fake(6, 4, 4, 3), fake(5, 2))
    with pytest.raises(ValueError):
        texture_cube(fake(6, 4, 4, 3), fake(5, 3), activation="tanh")
    with pytest.raises(NotImplementedError, match="dirs"):
        texture_cube(fake(6, 4, 4, 3), fake(5, 3).requires_grad_(True))
    with pytest.raises(ValueError, match="3 channels"):
        sky_color(fake(6, 4, 4, 4), np.eye(3), np.eye(3), np.zeros(3), 4, 4, white_background=False)
    with pytest.raises(ValueError, match="sky_mask"):
        sky_color(fake(6, 4, 4, 3), np.eye(3), np.eye(3), np.zeros(3), 4, 4, sky_mask=fake(4, 5, dtype=torch.bool),
                  white_background=False)
    with pytest.raises(ValueError, match="acc"):
        sky_color(fake(6, 4, 4, 3), np.eye(3), np.eye(3), np.zeros(3), 4, 4, acc=fake(4, 4), white_background=True)
    with pytest.raises(ValueError, match="perturb"):
        sky_color(fake(6, 4, 4, 3), np.eye(3), np.eye(3), np.zeros(3), 4, 4, perturb=fake(4, 4, 3), white_background=True)


def test_cubemap_abi_refuses_bad_arguments_before_any_launch():
    from street_crafter_amd import _lib, build
    build.build()
    lib = _lib.load()
    m = (ctypes.c_float * 9)(*np.eye(3).ravel())
    one = 1                                                     # any non-null pointer value: nothing is dereferenced

    def fwd(tex=one, R=8, C=3, dirs=one, ray=None, perturb=None, mask=None, acc=None, n=16, width=0, flags=0, out=one):
        return lib.sc_cubemap_fwd(tex, R, C, dirs, ray, perturb, mask, acc, n, width, flags, 0.0, out, None)

    def bwd(tex=one, R=8, C=3, dirs=one, ray=None, n=16, flags=0, g=one, gt=one):
        return lib.sc_cubemap_bwd(tex, R, C, dirs, ray, None, None, None, n, 4, flags, 0.0, g, gt, None)

    assert fwd(n=0) == 0 and fwd(n=0, dirs=None, ray=m, width=4) == 0
    for kw in (dict(R=1), dict(R=16385), dict(C=0), dict(C=5), dict(n=-1), dict(n=1 << 38), dict(flags=8), dict(tex=None),
               dict(out=None), dict(dirs=None), dict(ray=m), dict(perturb=one), dict(mask=one, acc=one),
               dict(dirs=None, ray=m, width=0), dict(dirs=None, ray=m, width=5)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(R=1), dict(gt=None), dict(g=None), dict(flags=16), dict(dirs=None)):
        assert bwd(**kw) == -1, kw
    from street_crafter_amd import _ctypes_binding
    assert callable(_ctypes_binding.cubemap_fwd) and callable(_lib.fast().cubemap_bwd)


def test_load_sky_cubemap_round_trips_a_written_checkpoint(tmp_path):
    from street_crafter_amd import scene_io
    from street_crafter_amd.scenes import make_scene
    cube = torch.randn(6, 4, 4, 3)
    bg = scene_io.scene_to_submodel(make_scene(32, seed=1), "background")
    with_sky, without = str(tmp_path / "a.pth"), str(tmp_path / "b.pth")
    scene_io.save_checkpoint(with_sky, [bg], extra={"sky_cubemap": {"params": {"sky_cube_map": cube}}, "iter": 7})
    scene_io.save_checkpoint(without, [bg])
    got = scene_io.load_sky_cubemap(with_sky)
    assert got.dtype == torch.float32 and torch.equal(got, cube)
    assert scene_io.load_sky_cubemap(without) is None
    assert set(scene_io.load_checkpoint(with_sky)) == {"background"}          # load_checkpoint is as it was
