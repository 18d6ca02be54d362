"""No-GPU checks of the grouped rasterizer's training boundary: the two new C entry points reject bad arguments before
any launch (every pointer null, or a host address that is never read), both binding routes offer the two new host
functions with the same parameters, and `rasterize_to_pixels_grouped_train` runs the forward-only operator's checks in
their order, without the grad refusal."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


def _fwd(lib, n_groups=2, tile=16, D=4, width=64, height=48, tw=4, th=3, C=1, n_isects=0):
    return lib.sc_rasterize_fwd_groups_ids(None, None, None, None, None, None, C, 8, D, n_groups, width, height, tile, tw,
                                           th, None, None, n_isects, None, None, None, None, None, None)


def _bwd(lib, n_groups=2, tile=16, D=4, width=64, height=48, tw=4, th=3, C=1, n_isects=0, inputs=None, upstream=None,
         outputs=None):
    i, u, o = inputs, upstream, outputs
    return lib.sc_rasterize_bwd_groups(i, i, i, i, i, C, 8, D, n_groups, width, height, tile, tw, th, i, i, n_isects, i, i,
                                       i, u, None, None, None, None, o, o, o, o, None)


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    for f in (_fwd, _bwd):                                          # nothing here touches a device: every pointer is null
        for bad in (0, 3, -1):
            assert f(lib, n_groups=bad) == -1
        assert f(lib, tile=8, tw=8, th=6) == -3                     # tile size other than 16
        assert f(lib, D=5) == -3 and f(lib, D=2) == -3              # channels other than 3 or 4
        assert f(lib, width=65) == -1 and f(lib, height=49) == -1   # a grid smaller than the image
        assert f(lib, tile=8) == -1                                 # ... which comes before the tile size
        assert f(lib, width=0) == -1 and f(lib, height=-4) == -1 and f(lib, D=0) == -1
        assert f(lib, tw=0) == -1 and f(lib, th=0) == -1 and f(lib, C=-1) == -1
        assert f(lib, n_isects=-1) == -1 and f(lib, n_isects=2 ** 31) == -1
        assert f(lib) == -1 and f(lib, n_isects=5) == -1            # valid sizes, null required pointers
        # no camera: nothing to write and nothing launched
        assert f(lib, C=0) == 0
        assert f(lib, C=0, n_groups=3) == -1 and f(lib, C=0, tile=8, tw=8, th=6) == -3


def test_backward_entry_has_nothing_to_do_without_records_or_upstream_gradients(lib):
    """With the four gradient outputs present: no record, or no upstream gradient at all, is 0 with nothing launched (the
    inputs are still null); an upstream gradient with records and null inputs is rejected.  The addresses are a host
    buffer's: a launch would have to read them, and none happens."""
    host = ctypes.addressof((ctypes.c_float * 16)())
    assert _bwd(lib, outputs=host) == 0                                             # n_isects == 0
    assert _bwd(lib, outputs=host, upstream=host) == 0
    assert _bwd(lib, outputs=host, n_isects=5) == 0                                 # every upstream pointer null
    assert _bwd(lib, outputs=host, n_isects=5, upstream=host) == -1                 # work to do, null inputs
    assert _bwd(lib, outputs=None, n_isects=5, upstream=host, inputs=host) == -1    # null gradient outputs
    assert _bwd(lib, outputs=host, n_isects=5, D=5) == -3                           # (the size checks still come first)


def test_binding_routes_offer_the_same_host_functions():
    import inspect
    import os
    import re
    from street_crafter_amd import _ctypes_binding
    src = open(os.path.join(os.path.dirname(_ctypes_binding.__file__), "csrc", "binding.cpp")).read()
    for name in ("rasterize_fwd_groups_ids", "rasterize_bwd_groups"):
        params = list(inspect.signature(getattr(_ctypes_binding, name)).parameters)
        m = re.search(r"py::tuple %s\((.*?)\)\s*\{" % name, src, flags=re.S)
        assert m and f'm.def("{name}", &{name})' in src
        assert [re.split(r"[\s&*]+", p.strip())[-1] for p in m.group(1).split(",")] == params, name
    # the forward takes exactly what the forward-only host function takes
    assert (list(inspect.signature(_ctypes_binding.rasterize_fwd_groups_ids).parameters)
            == list(inspect.signature(_ctypes_binding.rasterize_fwd_groups).parameters))


def _operator_args(N=6, C=1, D=4, W=32, H=16):
    return dict(means2d=torch.zeros(C, N, 2), conics=torch.zeros(C, N, 3), colors=torch.zeros(C, N, D),
                opacities=torch.zeros(C, N), image_width=W, image_height=H, tile_size=16,
                isect_offsets=torch.zeros(C, 1, 2, dtype=torch.int32), flatten_ids=torch.zeros(0, dtype=torch.int32),
                group_ids=torch.zeros(N, dtype=torch.uint8))


def test_operator_checks_come_in_order_on_cpu_tensors():
    from street_crafter_amd.groups import rasterize_to_pixels_grouped_train as op
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
    with pytest.raises(ValueError):                                 # ... also when an input requires grad
        op(**dict(_operator_args(), means2d=torch.zeros(1, 6, 2, requires_grad=True), group_ids=torch.zeros(6, 1, dtype=torch.uint8)))
    # 2. no grad refusal: an input that requires grad goes on to the device check, with grad enabled or not
    for name in ("means2d", "conics", "colors", "opacities"):
        args = _operator_args()
        args[name] = args[name].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="HIP device"):
            op(**args, absgrad=True)
        with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
            op(**args)
    # 3. well-formed CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        op(**_operator_args())
    with pytest.raises(RuntimeError, match="HIP device"):
        op(**_operator_args(D=3), n_groups=1)
