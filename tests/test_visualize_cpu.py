"""No-GPU checks of the visualizer frames (street_crafter_amd/visualize.py, csrc/frame_viz.hip): the numpy reference on
hand cases, every public function's ValueErrors, and the C ABI's argument checks through the loaded library."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visualize_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


# ---- the reference itself ----------------------------------------------------------------------------------------------
def test_reference_cast_wraps_like_x86():
    t = np.array([-30.7, -300.2, 256.5, 1e10, np.nan, np.inf, -np.inf, 0.0, 0.999, 255.999, 255.0, -0.5, -1.0, -256.0,
                  2.0 ** 31, -2.0 ** 31, 2147483904.0, 3e38, -3e38], dtype=np.float32)
    want = [226, 212, 0, 0, 0, 0, 0, 0, 0, 255, 255, 0, 255, 0, 0, 0, 0, 0, 0]
    assert R.q(t).tolist() == want


def test_reference_range_and_colour_map_on_hand_cases():
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    v = np.array([[0.0, 2.0, np.nan], [6.0, -1.0, 4.0]], dtype=np.float32)
    mi, ma = R.value_range(v)
    assert (mi, ma) == (np.float32(2.0), np.float32(6.0)) and mi.dtype == np.float32
    got = R.colorize(v, ramp)[..., 0]
    # 0 and NaN -> 255 * (0 - 2) / 4 = -127.5 -> trunc -127 -> 129; -1 -> -191.25 -> 65; 6 -> 255 * (4 / (4 + 1e-8f)) = 255
    assert got.tolist() == [[129, 0, 129], [255, 65, 127]]
    # inf -> FLT_MAX is the maximum; -inf -> -FLT_MAX lands at 255 * (-1) -> 1
    w = np.array([[1.0, np.inf, -np.inf]], dtype=np.float32)
    mi, ma = R.value_range(w)
    assert mi == np.float32(1.0) and ma == np.finfo(np.float32).max
    assert R.colorize(w, ramp)[..., 0].tolist() == [[0, 255, 1]]
    # no positive value: mi = 0; a constant map: denominator 1e-8f, every pixel 0
    assert R.value_range(np.array([[0.0, -3.0]], dtype=np.float32)) == (np.float32(0), np.float32(0))
    assert R.colorize(np.full((2, 2), 7.5, np.float32), ramp)[..., 0].tolist() == [[0, 0], [0, 0]]
    # a denormal is positive
    tiny = np.float32(1e-45)
    assert R.value_range(np.array([[tiny, 1.0]], dtype=np.float32))[0] == tiny and tiny > 0
    # a caller's range: below mi wraps, above ma wraps (1 + 1e-8f is 1 in float32, so the quotients are -1, 0, 1, 3)
    got = R.colorize(np.array([[1.0, 2.0, 3.0, 5.0]], dtype=np.float32), ramp, minmax=(2.0, 3.0))[..., 0]
    assert got.tolist() == [[(-255) & 255, 0, 255, (3 * 255) & 255]]


def test_reference_diff_and_grey():
    rgb = np.array([[[0.5, 1.0]], [[0.25, 0.0]], [[0.0, 0.0]]], dtype=np.float32)       # [3,1,2]
    gt = np.zeros_like(rgb)
    assert R.diff_map(rgb, gt).tolist() == [[0.3125, 1.0]]
    assert R.diff_map(rgb, gt, np.array([[True, False]])).tolist() == [[0.3125, 0.0]]
    nan = rgb.copy()
    nan[0, 0, 1] = np.nan
    assert R.diff_map(nan, gt, np.array([[True, False]])).tolist() == [[0.3125, 0.0]]      # where() hides it
    a = np.array([[0.0, 1.0, 1.0 - 2.0 ** -24, 0.5, 1.004]], dtype=np.float32)
    assert R.gray(a)[..., 0].tolist() == [[0, 255, 254, 127, 0]]


# ---- ValueErrors of the public functions ------------------------------------------------------------------------------------
def test_public_functions_refuse_bad_arguments_on_the_host():
    from street_crafter_amd import visualize as V
    x = torch.zeros(4, 6)
    lut = torch.zeros(256, 3, dtype=torch.uint8)
    img = torch.zeros(3, 4, 6)
    for call in (lambda: V.value_range(x), lambda: V.diff_range(img, img), lambda: V.colorize(x, lut),
                 lambda: V.colorize_diff(img, img, lut), lambda: V.gray_u8(x),
                 lambda: V.novel_view_frames({"rgb": img, "acc": x[None], "depth": x[None]}, lut),
                 lambda: V.trajectory_frames({"rgb": img, "rgb_background": img, "rgb_object": img, "acc_object": x[None],
                                              "depth": x[None]}, img, None, lut, lut)):
        with pytest.raises(ValueError, match="HIP device"):            # no CPU path
            call()
    # shapes and dtypes
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        V.value_range(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match=r"\[3,4,6\]"):
        V._image(torch.zeros(3, 4, 5), "gt", (4, 6))            # (the second image of a pair must match the first)
    with pytest.raises(ValueError):
        V.value_range(torch.zeros(4, 6, dtype=torch.float64))
    with pytest.raises(ValueError):
        V.value_range([[1.0]])
    with pytest.raises(ValueError):
        V.gray_u8(torch.zeros(4, 6, dtype=torch.float16))
    with pytest.raises(ValueError):
        V.diff_range(torch.zeros(4, 4, 6), img)
    with pytest.raises(ValueError):
        V.novel_view_frames({"rgb": img, "acc": x[None]}, lut)
    with pytest.raises(ValueError, match="rounding"):
        V.novel_view_frames({"rgb": img, "acc": x[None], "depth": x[None]}, lut, rounding="nearest")
    with pytest.raises(ValueError):
        V.trajectory_frames({"rgb": img}, img, None, lut, lut)


def test_argument_helpers_judge_luts_outs_masks_and_ranges():
    """The checks behind every public function, on CPU tensors (their device is an argument)."""
    from street_crafter_amd import visualize as V
    cpu = torch.device("cpu")
    good = torch.zeros(256, 3, dtype=torch.uint8)
    assert V._lut(good, "lut", cpu) is good
    for bad in (torch.zeros(256, 3), torch.zeros(255, 3, dtype=torch.uint8), torch.zeros(3, 256, dtype=torch.uint8).t(),
                torch.zeros(256, 4, dtype=torch.uint8)[:, :3], None, good.to("meta")):
        with pytest.raises(ValueError, match="lut"):
            V._lut(bad, "lut", cpu)
    assert V._out(None, (4, 6, 3), cpu).shape == (4, 6, 3)
    slot = torch.zeros(4, 6, 3, dtype=torch.uint8)
    assert V._out(slot, (4, 6, 3), cpu) is slot
    for bad in (torch.zeros(4, 6, 1, dtype=torch.uint8), torch.zeros(4, 6, 3), torch.zeros(4, 6, 4, dtype=torch.uint8)[..., :3],
                slot.to("meta")):
        with pytest.raises(ValueError, match="out"):
            V._out(bad, (4, 6, 3), cpu)
    assert V._mask(None, (4, 6), cpu) is None
    assert V._mask(torch.ones(1, 4, 6, dtype=torch.bool), (4, 6), cpu).dtype == torch.uint8
    for bad in (torch.ones(4, 6), torch.ones(4, 5, dtype=torch.bool), torch.ones(4, 6, dtype=torch.bool, device="meta")):
        with pytest.raises(ValueError, match="mask"):
            V._mask(bad, (4, 6), cpu)
    assert V._range4(None, cpu) is None
    assert V._range4((1.5, 3), cpu).tolist() == [1.5, 3.0, 1.5, 3.0]
    assert V._range4(torch.tensor([2.0, 4.0]), cpu).tolist() == [2.0, 4.0, 2.0, 4.0]
    for bad in ((1.0,), "ab", torch.zeros(3), torch.zeros(2, dtype=torch.float64), torch.zeros(2, device="meta")):
        with pytest.raises(ValueError, match="minmax"):
            V._range4(bad, cpu)
    with pytest.raises(ValueError, match="out"):
        V._slots({"colour": slot}, ("rgb", "acc", "depth"))


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------
def test_entry_points_validate_before_any_launch(lib):
    ws_bytes = lib.sc_frame_viz_workspace_bytes()
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    P = 4096                        # stands in for a device address: nothing here is dereferenced or launched
    EINVAL, EWORKSPACE = -1, -2

    def rng(depth=P, ds=1, rgb=None, rp=1, rc=1, gt=None, gp=1, gc=1, mask=None, n=100, ws=P, wsb=ws_bytes):
        return lib.sc_frame_viz_range(depth, ds, rgb, rp, rc, gt, gp, gc, mask, n, ws, wsb, None)

    assert rng(n=-1) == EINVAL and rng(n=2 ** 31) == EINVAL
    assert rng(ds=-1) == EINVAL
    assert rng(rgb=P, gt=P, rp=-1) == EINVAL and rng(rgb=P, gt=P, gc=-4) == EINVAL
    assert rng(rgb=P) == EINVAL and rng(gt=P) == EINVAL               # a diff source given only in part
    assert rng(mask=P) == EINVAL                                      # a mask without its images
    assert rng(depth=None) == EINVAL                                  # no map
    assert rng(ws=None) == EINVAL
    assert rng(wsb=ws_bytes - 1) == EWORKSPACE and rng(depth=None, rgb=P, gt=P, wsb=0) == EWORKSPACE
    assert rng(n=0) == 0 and rng(n=0, ws=None, wsb=0) == 0

    def fin(ws=P, wsb=ws_bytes, n=100, maps=3, out=P):
        return lib.sc_frame_viz_range_finish(ws, wsb, n, maps, out, None)

    assert fin(n=-1) == EINVAL and fin(n=2 ** 31) == EINVAL and fin(maps=0) == EINVAL and fin(maps=4) == EINVAL
    assert fin(ws=None) == EINVAL and fin(out=None) == EINVAL
    assert fin(wsb=16) == EWORKSPACE
    assert fin(n=0) == 0

    def u8(depth=None, ds=1, rgb=None, rp=1, rc=1, gt=None, gp=1, gc=1, mask=None, acc=None, acc_obj=None, n=100,
           dlut=None, flut=None, r4=None, ws=None, wsb=0, o_depth=None, o_diff=None, o_acc=None, o_obj=None):
        return lib.sc_frame_viz_u8(depth, ds, rgb, rp, rc, gt, gp, gc, mask, acc, acc_obj, n, dlut, flut, r4, ws, wsb,
                                   o_depth, o_diff, o_acc, o_obj, None)

    assert u8(depth=P, dlut=P, r4=P) == EINVAL                                        # no output requested
    assert u8(depth=P, dlut=P, r4=P, o_depth=P, n=-1) == EINVAL
    assert u8(depth=P, dlut=P, r4=P, o_depth=P, n=2 ** 31) == EINVAL
    assert u8(depth=P, ds=-1, dlut=P, r4=P, o_depth=P) == EINVAL
    assert u8(depth=P, r4=P, o_depth=P) == EINVAL                                     # a colour output without its lut
    assert u8(dlut=P, r4=P, o_depth=P) == EINVAL                                      # ... without its source
    assert u8(rgb=P, gt=P, r4=P, o_diff=P) == EINVAL
    assert u8(rgb=P, flut=P, r4=P, o_diff=P) == EINVAL                                # a diff source given only in part
    assert u8(o_acc=P) == EINVAL and u8(o_obj=P, acc=P) == EINVAL                     # a grey output without its source
    assert u8(depth=P, dlut=P, o_depth=P) == EINVAL                                   # neither range4 nor workspace
    assert u8(depth=P, dlut=P, o_depth=P, ws=P, wsb=ws_bytes - 1) == EWORKSPACE
    assert u8(rgb=P, gt=P, flut=P, o_diff=P, ws=P, wsb=0) == EWORKSPACE
    assert u8(depth=P, dlut=P, r4=P, o_depth=P, n=0) == 0
    assert u8(acc=P, o_acc=P, n=0) == 0 and u8(depth=P, dlut=P, o_depth=P, ws=P, wsb=ws_bytes, n=0) == 0


def test_header_ctypes_table_and_documents_name_the_same_entries(lib):
    from street_crafter_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ("sc_frame_viz_workspace_bytes", "sc_frame_viz_range", "sc_frame_viz_range_finish", "sc_frame_viz_u8")
    header = open(os.path.join(root, "include", "street_crafter_amd.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES and n + "(" in header and hasattr(lib, n)
    assert "frame_viz.hip" in build.SOURCES
    assert _lib.SIGNATURES["sc_frame_viz_workspace_bytes"][0] is ctypes.c_size_t
    # the new entries are called through the ctypes table only: neither binding layer grows
    from street_crafter_amd import _ctypes_binding
    assert not [n for n in dir(_ctypes_binding) if "viz" in n]
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "visualize" in open(os.path.join(root, doc)).read(), doc
