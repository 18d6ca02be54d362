"""No-GPU checks of the layered novel-view frame (street_crafter_amd/layers.py, csrc/raster_layers.hip): the depth lift
is exact and orders the layers, lifted keys make every tile list of the numpy oracle a front run followed by a back run
(each that layer's own list), and the operator, the frame function and the C entry refuse bad arguments."""
import math

import numpy as np
import pytest
import torch

TWO64 = 2.0 ** 64


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


# ---- the lift -----------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("near,far", [(0.001, 1000.0), (0.01, 1e10)])
def test_lift_is_exact_and_puts_the_back_layer_behind(near, far):
    from street_crafter_amd.layers import layered_depths
    g = torch.Generator().manual_seed(7)
    C, N, n_front = 2, 400, 300
    # log-uniform in [near, far], with both planes themselves and some exact ties in each layer
    d = torch.exp(math.log(near) + (math.log(far) - math.log(near)) * torch.rand(C, N, generator=g, dtype=torch.float64))
    d = d.to(torch.float32).clamp(near, far)
    d[:, 0], d[:, 1], d[:, n_front], d[:, n_front + 1] = far, near, near, far
    d[:, 10:14] = d[:, 10:11]
    d[:, n_front + 10:n_front + 14] = d[:, n_front + 10:n_front + 11]
    keys = layered_depths(d, n_front)
    assert keys.dtype == torch.float32 and keys.shape == d.shape and keys.data_ptr() != d.data_ptr()
    assert torch.equal(_bits(keys[:, :n_front]), _bits(d[:, :n_front]))                      # front rows: bit for bit
    back = keys[:, n_front:]
    assert torch.isfinite(back).all() and (back > 0).all()
    assert torch.equal(back.double(), d[:, n_front:].double() * TWO64)                      # exactly * 2^64 ...
    assert torch.equal(_bits(back / TWO64), _bits(d[:, n_front:]))                           # ... and back again
    # order and ties inside the back layer: the stable order of the lifted keys is the stable order of the depths
    for c in range(C):
        assert torch.equal(torch.sort(back[c], stable=True).indices, torch.sort(d[c, n_front:], stable=True).indices)
        assert torch.equal(back[c, 10:14], back[c, 10:11].expand(4))
    assert (back.min(dim=1).values > keys[:, :n_front].max(dim=1).values).all()
    # as isect_tiles sees them: the key is the float's bit pattern
    assert (_bits(back).min() > _bits(keys[:, :n_front]).max())


def test_lift_edge_cases_and_argument_checks():
    from street_crafter_amd.layers import layered_depths
    d = torch.rand(1, 5) + 1.0
    assert torch.equal(layered_depths(d, 5), d) and torch.equal(layered_depths(d, 0), d * TWO64)
    assert torch.equal(layered_depths(d, 2, lift=4.0)[:, 2:], d[:, 2:] * 4.0)
    for bad in (dict(n_front=6), dict(n_front=-1), dict(n_front=2, lift=3.0), dict(n_front=2, lift=1.0)):
        with pytest.raises(ValueError):
            layered_depths(d, **bad)
    with pytest.raises(ValueError):
        layered_depths(d.double(), 2)
    with pytest.raises(ValueError):
        layered_depths(d[0], 2)


def test_smallest_lift_is_the_least_power_of_two_that_separates_the_planes():
    from street_crafter_amd.layers import smallest_lift
    assert smallest_lift(0.001, 1000.0) == 2.0 ** 20 and smallest_lift(0.01, 1e10) == 2.0 ** 40
    assert smallest_lift(1.0, 1.0) == 2.0 and smallest_lift(0.5, 1.0) == 4.0 and smallest_lift(1.0, 1024.0) == 2048.0
    for near, far in ((0.001, 1000.0), (0.01, 1e10), (0.3, 77.0)):
        lift = smallest_lift(near, far)
        assert near * lift > far and not near * (lift / 2) > far
    for bad in ((0.0, 1.0), (2.0, 1.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            smallest_lift(*bad)


# ---- the lists, through the numpy oracle ---------------------------------------------------------------------------
W, H, TILE, FOCAL = 64, 48, 16, 60.0
TW, TH = 4, 3


def _oracle_scene(n_front=300, n_back=40, seed=3):
    rng = np.random.default_rng(seed)
    n = n_front + n_back
    z = np.concatenate([rng.uniform(4.0, 20.0, n_front), rng.uniform(1.0, 8.0, n_back)])     # back NEARER than much of the front
    z[5:9] = z[5]                                                                             # ties inside the front layer
    z[n_front + 2:n_front + 6] = z[n_front + 2]                                               # ... inside the back layer
    z[n_front + 7] = z[20]                                                                    # ... and across the layers
    x = rng.uniform(-1, 1, n) * (W / 2.0 / FOCAL) * z
    y = rng.uniform(-1, 1, n) * (H / 2.0 / FOCAL) * z
    means = np.stack([x, y, z], -1).astype(np.float32)
    scales = np.exp(rng.uniform(math.log(0.05), math.log(0.5), (n, 3))).astype(np.float32)
    quats = rng.standard_normal((n, 4)).astype(np.float32)
    quats /= np.linalg.norm(quats, axis=-1, keepdims=True)
    return means, quats, scales


def _lists(radii, means2d, keys):
    """-> per tile, the list of Gaussian rows in list order."""
    from oracle import gsplat_oracle as O
    _, ids, fids = O.isect_tiles(means2d[None], radii[None], keys[None], TILE, TW, TH)
    offs = O.isect_offset_encode(ids, 1, TW, TH).reshape(-1)
    ends = np.append(offs[1:], len(fids))
    return [fids[s:e].tolist() for s, e in zip(offs, ends)]


def test_lifted_keys_layer_every_tile_list_of_the_oracle():
    from oracle import gsplat_oracle as O
    from street_crafter_amd.layers import layered_depths
    n_front, n_back = 300, 40
    means, quats, scales = _oracle_scene(n_front, n_back)
    K = np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1]], np.float32)
    radii, means2d, depths, _, _ = O.fully_fused_projection(means, quats, scales, np.eye(4, dtype=np.float32), K, W, H,
                                                           near_plane=0.001, far_plane=1000.0)
    assert (radii[:n_front] > 0).sum() > 200 and (radii[n_front:] > 0).sum() > 20
    keys = layered_depths(torch.from_numpy(depths)[None], n_front)[0].numpy()
    full = _lists(radii, means2d, keys)
    own_front = _lists(radii[:n_front], means2d[:n_front], depths[:n_front])
    own_back = _lists(radii[n_front:], means2d[n_front:], depths[n_front:])
    both = 0
    for t in range(TW * TH):
        rows = np.asarray(full[t], dtype=np.int64)
        is_back = rows >= n_front
        k = int(np.argmax(is_back)) if is_back.any() else len(rows)
        assert not is_back[:k].any() and is_back[k:].all(), f"tile {t}: not a front run followed by a back run"
        assert rows[:k].tolist() == own_front[t], f"tile {t}: the front run is not the front layer's own list"
        assert (rows[k:] - n_front).tolist() == own_back[t], f"tile {t}: the back run is not the back layer's own list"
        both += bool(0 < k < len(rows))
    assert both >= TW * TH // 2                    # the property is exercised: most tiles hold both layers
    # ... and it is the lift that does it: on the true depths at least one tile interleaves
    plain = _lists(radii, means2d, depths)
    interleaved = 0
    for rows in plain:
        is_back = np.asarray(rows) >= n_front
        k = int(np.argmax(is_back)) if is_back.any() else len(rows)
        interleaved += bool((~is_back[k:]).any())
    assert interleaved >= 1


# ---- argument checks -------------------------------------------------------------------------------------------------
def _operator_args(N=6, C=1, D=4, Wd=32, Hd=16):
    return dict(means2d=torch.zeros(C, N, 2), conics=torch.zeros(C, N, 3), colors=torch.zeros(C, N, D),
                opacities=torch.zeros(C, N), image_width=Wd, image_height=Hd, tile_size=16,
                isect_offsets=torch.zeros(C, 1, 2, dtype=torch.int32), flatten_ids=torch.zeros(0, dtype=torch.int32),
                n_front=4)


def test_operator_checks_come_in_order_on_cpu_tensors():
    from street_crafter_amd.layers import rasterize_to_pixels_layered as op
    # 1. dtypes / shapes / sizes: ValueError or NotImplementedError, although the tensors are CPU tensors
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), conics=torch.zeros(1, 6, 2)))
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), means2d=torch.zeros(1, 6, 2, dtype=torch.float64)))
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), flatten_ids=torch.zeros(0, dtype=torch.int64)))
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), isect_offsets=torch.zeros(1, 1, 2, dtype=torch.int64)))
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), image_width=33))                # two tile columns do not cover 33 pixels
    for bad in (-1, 7):
        with pytest.raises(ValueError):
            op(**dict(_operator_args(), n_front=bad))
    with pytest.raises(NotImplementedError):
        op(**dict(_operator_args(), tile_size=8, isect_offsets=torch.zeros(1, 2, 4, dtype=torch.int32)))
    with pytest.raises(NotImplementedError):
        op(**_operator_args(D=5))
    # 2. forward only: an input that requires grad is refused (before the device check), not detached silently
    for name in ("means2d", "conics", "colors", "opacities"):
        args = _operator_args()
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError):
            op(**args)
        with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
            op(**args)
    # 3. well-formed CPU tensors: there is no CPU path
    for n_front in (0, 4, 6):
        with pytest.raises(RuntimeError, match="HIP device"):
            op(**dict(_operator_args(), n_front=n_front))


def test_novel_view_frame_refuses_planes_the_lift_cannot_separate():
    from street_crafter_amd.layers import novel_view_frame
    n = 4
    args = (torch.zeros(n, 3), torch.zeros(n, 4), torch.zeros(n, 3), torch.zeros(n), torch.zeros(n, 4, 3), torch.eye(4),
            torch.eye(3), 32, 16, 2)
    with pytest.raises(ValueError, match="near_plane"):
        novel_view_frame(*args, near_plane=1e-30, far_plane=1e10, sh_degree=1)          # 1e-30 * 2^64 < 1e10
    with pytest.raises(ValueError, match="near_plane"):
        novel_view_frame(*args, near_plane=0.01, far_plane=1e20, sh_degree=1)           # 1e20 * 2^64 overflows float32
    with pytest.raises(ValueError, match="lift"):
        novel_view_frame(*args, near_plane=0.001, far_plane=1000.0, sh_degree=1, lift=2.0 ** 10)     # too small for these planes
    with pytest.raises(ValueError, match="lift"):
        novel_view_frame(*args, near_plane=0.001, far_plane=1000.0, sh_degree=1, lift=3.0)
    with pytest.raises(ValueError, match="lift"):
        novel_view_frame(*args, near_plane=0.001, far_plane=1000.0, sh_degree=1, lift=2.0 ** 65)     # 2^64 is the largest
    # inference only: a scene that requires grad is refused, not rendered detached
    grad_args = (args[0].clone().requires_grad_(True),) + args[1:]
    with pytest.raises(NotImplementedError):
        novel_view_frame(*grad_args, near_plane=0.001, far_plane=1000.0, sh_degree=1)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        novel_view_frame(*grad_args, near_plane=0.001, far_plane=1000.0, sh_degree=1)
    with pytest.raises(ValueError):
        novel_view_frame(*args, near_plane=0.01, far_plane=1e10, sh_degree=1, output="png")
    with pytest.raises(ValueError):
        novel_view_frame(*args, near_plane=0.01, far_plane=1e10, sh_degree=1, output="u8", rounding="nearest")
    # planes that qualify: on to the tensors, which are CPU tensors
    for near, far in ((0.001, 1000.0), (0.01, 1e10)):
        with pytest.raises(RuntimeError, match="HIP device"):
            novel_view_frame(*args, near_plane=near, far_plane=far, sh_degree=1)


def _entry(lib, N=8, D=4, n_front=4, tile=16, width=64, height=48, tw=4, th=3, C=1, n_isects=0, epilogue=0, rounding=0,
           outs=(None, None, None, None), u8=None, offsets=None):
    return lib.sc_rasterize_fwd_layers(None, None, None, None, C, N, D, n_front, width, height, tile, tw, th, offsets,
                                       None, n_isects, epilogue, rounding, *outs, u8, None, None)


def test_c_entry_rejects_bad_arguments_before_any_launch(lib):
    # nothing here touches a device: the pointers are null or host addresses that are never dereferenced
    host = torch.zeros(64, dtype=torch.float32)
    p = host.data_ptr()
    full = dict(outs=(p, p, p, p), offsets=p)
    assert _entry(lib, n_front=9, **full) == -1 and _entry(lib, n_front=-1, **full) == -1       # n_front outside [0, N]
    assert _entry(lib, **dict(full, offsets=None)) == -1                                       # a null pointer
    assert _entry(lib, **dict(full, outs=(p, p, None, p))) == -1
    assert _entry(lib, epilogue=1, outs=(p, None, None, None), offsets=p) == -1
    assert _entry(lib, epilogue=2, offsets=p) == -1                                            # no uint8 frame to write
    assert _entry(lib, D=5, **full) == -1 and _entry(lib, D=2, **full) == -1                    # D not 3 or 4
    assert _entry(lib, tile=8, tw=8, th=6, **full) == -1                                       # tile size not 16
    assert _entry(lib, epilogue=3, **full) == -1 and _entry(lib, epilogue=-1, **full) == -1
    assert _entry(lib, epilogue=2, rounding=2, u8=p, offsets=p) == -1
    assert _entry(lib, width=65, **full) == -1 and _entry(lib, height=49, **full) == -1         # a grid smaller than the image
    assert _entry(lib, width=0, **full) == -1 and _entry(lib, tw=0, **full) == -1 and _entry(lib, N=-1, **full) == -1
    assert _entry(lib, n_isects=-1, **full) == -1 and _entry(lib, n_isects=2 ** 31, **full) == -1
    # no camera: nothing to write and nothing launched -- but the arguments are still checked
    assert _entry(lib, C=0) == 0 and _entry(lib, C=0, n_front=8) == 0 and _entry(lib, C=0, n_front=9) == -1


def test_binding_routes_offer_the_same_host_function():
    import inspect
    import os
    import re
    from street_crafter_amd import _ctypes_binding, _lib
    params = list(inspect.signature(_ctypes_binding.rasterize_fwd_layers).parameters)
    src = open(os.path.join(os.path.dirname(_ctypes_binding.__file__), "csrc", "binding.cpp")).read()
    m = re.search(r"py::tuple rasterize_fwd_layers\((.*?)\)\s*\{", src, flags=re.S)
    assert m and 'm.def("rasterize_fwd_layers", &rasterize_fwd_layers)' in src
    assert [re.split(r"[\s&*]+", p.strip())[-1] for p in m.group(1).split(",")] == params
    assert "sc_rasterize_fwd_layers" in _lib.SIGNATURES
