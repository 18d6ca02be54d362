"""No-GPU checks of the grouped rasterizer's boundary: the two C entry points reject bad arguments before any launch,
the Python operator's three classes of checks come in their stated order, and `render_all(grouped=False)` builds its
subsets in order."""
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


def _raster(lib, n_groups=2, tile=16, D=4, width=64, height=48, tw=4, th=3, C=1, n_isects=0):
    return lib.sc_rasterize_fwd_groups(None, None, None, None, None, None, C, 8, D, n_groups, width, height, tile, tw,
                                       th, None, None, n_isects, None, None, None, None, None)


def _extents(lib, n_groups=2, tw=4, th=3, C=1, n_isects=0):
    return lib.sc_group_extents(None, None, n_isects, None, C, 8, n_groups, tw, th, None, None)


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    # nothing here touches a device: every pointer is null
    for bad in (0, 3, -1):
        assert _raster(lib, n_groups=bad) == -1 and _extents(lib, n_groups=bad) == -1
    assert _raster(lib, tile=8, tw=8, th=6) == -3                   # tile size other than 16
    assert _raster(lib, D=5) == -3 and _raster(lib, D=2) == -3      # channels other than 3 or 4
    assert _raster(lib, width=65) == -1 and _raster(lib, height=49) == -1       # a grid smaller than the image
    assert _raster(lib, tile=8) == -1                               # ... which comes before the tile size
    assert _raster(lib, width=0) == -1 and _raster(lib, height=-4) == -1 and _raster(lib, D=0) == -1
    assert _raster(lib, tw=0) == -1 and _extents(lib, th=0) == -1 and _extents(lib, C=-1) == -1
    assert _raster(lib, n_isects=-1) == -1 and _extents(lib, n_isects=2 ** 31) == -1
    assert _raster(lib) == -1 and _extents(lib) == -1               # valid sizes, null required pointers
    # no camera: an image set of 0 pixels, nothing to write and nothing launched
    assert _raster(lib, C=0) == 0 and _extents(lib, C=0) == 0
    assert _raster(lib, C=0, n_groups=3) == -1 and _raster(lib, C=0, tile=8, tw=8, th=6) == -3


def _operator_args(N=6, C=1, D=4, W=32, H=16):
    return dict(means2d=torch.zeros(C, N, 2), conics=torch.zeros(C, N, 3), colors=torch.zeros(C, N, D),
                opacities=torch.zeros(C, N), image_width=W, image_height=H, tile_size=16,
                isect_offsets=torch.zeros(C, 1, 2, dtype=torch.int32), flatten_ids=torch.zeros(0, dtype=torch.int32),
                group_ids=torch.zeros(N, dtype=torch.uint8))


def test_operator_checks_come_in_order_on_cpu_tensors():
    from street_crafter_amd.groups import rasterize_to_pixels_grouped as op
    # 1. shapes / dtypes / sizes: ValueError or NotImplementedError, although the tensors are CPU tensors
    for bad in (torch.zeros(6, dtype=torch.int32), torch.zeros(6, 1, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            op(**dict(_operator_args(), group_ids=bad))
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), conics=torch.zeros(1, 6, 2)))
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), flatten_ids=torch.zeros(0, dtype=torch.int64)))
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), image_width=33))                # two tile columns do not cover 33 pixels
    with pytest.raises(ValueError):
        op(**_operator_args(), n_groups=0)
    with pytest.raises(NotImplementedError):
        op(**_operator_args(), n_groups=3)
    with pytest.raises(NotImplementedError):
        op(**dict(_operator_args(), tile_size=8, isect_offsets=torch.zeros(1, 2, 4, dtype=torch.int32)))
    with pytest.raises(NotImplementedError):
        op(**_operator_args(D=5))
    # ... and they come before the grad check
    with pytest.raises(ValueError):
        op(**dict(_operator_args(), means2d=torch.zeros(1, 6, 2, requires_grad=True), group_ids=torch.zeros(6, 1, dtype=torch.uint8)))
    # 2. forward only: an input that requires grad is refused (before the device check), not detached silently
    for name in ("means2d", "conics", "colors", "opacities"):
        args = _operator_args()
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError):
            op(**args)
        with torch.no_grad(), pytest.raises(RuntimeError):          # nothing to record: on to the device check
            op(**args)
    # 3. well-formed CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        op(**_operator_args())
    with pytest.raises(RuntimeError, match="HIP device"):
        op(**_operator_args(D=3), n_groups=1)


def test_binding_routes_offer_the_same_host_function():
    import inspect
    import os
    import re
    from street_crafter_amd import _ctypes_binding
    params = list(inspect.signature(_ctypes_binding.rasterize_fwd_groups).parameters)
    src = open(os.path.join(os.path.dirname(_ctypes_binding.__file__), "csrc", "binding.cpp")).read()
    m = re.search(r"py::tuple rasterize_fwd_groups\((.*?)\)\s*\{", src, flags=re.S)
    assert m and 'm.def("rasterize_fwd_groups", &rasterize_fwd_groups)' in src
    assert [re.split(r"[\s&*]+", p.strip())[-1] for p in m.group(1).split(",")] == params


def test_render_all_subsets_keep_order_and_handle_an_empty_one():
    from harness.caller import scene_subset
    from street_crafter_amd.scenes import make_scene_portable
    scene = make_scene_portable(50)
    gids = (torch.arange(50) % 3 == 1).to(torch.uint8)              # 0,1,0,0,1,0,...: no id 2
    for k in (0, 1):
        sub = scene_subset(scene, gids == k)
        rows = torch.nonzero(gids == k)[:, 0]
        assert sub.n == rows.numel() and sub.sh_degree == scene.sh_degree
        for name in ("means", "quats", "scales", "opacities", "sh"):
            assert torch.equal(getattr(sub, name), getattr(scene, name)[rows]), name      # ascending rows: order kept
    empty = scene_subset(scene, gids == 2)
    assert empty.n == 0 and empty.means.shape == (0, 3) and empty.sh.shape[1:] == scene.sh.shape[1:]
    assert empty.opacities.shape == (0, 1) and empty.quats.shape == (0, 4)


def test_render_all_answers_an_empty_scene_with_zero_images():
    # both spellings return zeros without reaching an operator (the reference's answer for len(xyz) == 0)
    from harness.caller import render_all, scene_subset
    from street_crafter_amd.scenes import make_camera, make_scene_portable
    scene = make_scene_portable(4)
    empty = scene_subset(scene, torch.zeros(4, dtype=torch.bool))
    cam = make_camera(32, 16, 40.0, 40.0)
    for grouped in (False, True):
        out = render_all(empty, cam, torch.zeros(0, dtype=torch.uint8), grouped=grouped)
        assert set(out) == {"rgb", "acc", "depth", "rgb_background", "acc_background", "rgb_object", "acc_object"}
        for k, v in out.items():
            assert v.shape == ((3 if k.startswith("rgb") else 1), 16, 32) and not v.any(), k
