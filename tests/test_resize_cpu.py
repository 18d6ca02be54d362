"""No-GPU checks of street_crafter_amd/resize.py's host side: the reference's crop arithmetic, the tap tables against
torch's own float64 interpolate, their transpose, the argument checks of the C entries and the refusals of CPU tensors.

One finding is pinned here.  ATen's antialias rule leaves, for some ratios, a tap whose weight is zero in exact arithmetic
but 1e-16 or so in float64 (30 -> 18: 7.9e-17).  tap_table keeps such a residue tap, as float64 ATen does: a mask pixel
whose only set taps are residue taps is True in both.  float32 arithmetic may call the same weight zero, so those pixels
are the ones no implementation can be held to (tests/test_resize_gpu.py counts them)."""
import ctypes
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rz():
    from street_crafter_amd import resize
    return resize


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


def test_crop_box_is_the_references_arithmetic(rz):
    assert rz.crop_box(1066, 1600, 576, 1024) == (166, 1066, 0, 1600)
    assert rz.crop_box(1280, 1920, 576, 1024) == (200, 1280, 0, 1920)
    assert rz.crop_box(30, 64, 18, 32) == (0, 30, 5, 58)
    assert rz.crop_box(29, 50, 18, 32) == (1, 29, 0, 50)
    assert rz.crop_box(45, 80, 18, 32) == (0, 45, 0, 80)
    for bad in ((0, 5, 18, 32), (5, -1, 18, 32), (5, 5, 0, 32), (5.0, 5, 18, 32), (True, 5, 18, 32)):
        with pytest.raises(ValueError):
            rz.crop_box(*bad)
    with pytest.raises(ValueError, match="leaves nothing"):
        rz.crop_box(1000, 1, 1, 2000)


def _along_width(x, n_out, antialias):
    """x [R, n_in] float64 resized along its last axis by torch (two identical rows, height 2 -> 2)."""
    return ref.interpolate64(np.repeat(x[:, None, :], 2, axis=1), (2, n_out), antialias)[:, 0]


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("n_in,n_out", ref.PAIRS)
def test_tap_table_is_torchs_float64_interpolate(rz, n_in, n_out, antialias):
    t = rz.tap_table(n_in, n_out, antialias)
    assert (t.n_in, t.n_out, t.antialias) == (n_in, n_out, antialias)
    assert t.start.dtype == np.int32 and t.offset.dtype == np.int32 and t.weight.dtype == np.float32
    assert t.offset[0] == 0 and len(t.weight) == len(t.weight64) == t.offset[-1] and (t.counts() >= 1).all()
    assert (t.start >= 0).all() and (t.start + t.counts() <= n_in).all()
    assert np.array_equal(t.weight, t.weight64.astype(np.float32)) and (t.weight64 > 0).all()
    x = np.random.default_rng(n_in + n_out).uniform(-1.0, 1.0, (4, n_in))
    err = np.abs(x @ ref.dense(t).T - _along_width(x, n_out, antialias)).max()
    print(f"{n_in}->{n_out} antialias={antialias}: max taps {t.counts().max()}, |table - torch| {err:.2e}")
    assert err <= 1e-14
    # the fp32 weights of every output sum to 1
    sums = np.add.reduceat(t.weight.astype(np.float64), t.offset[:-1])
    assert np.abs(sums - 1.0).max() <= 2.0 ** -22
    if n_in == n_out:
        assert (t.counts() == 1).all() and np.array_equal(t.start, np.arange(n_in)) and (t.weight == 1.0).all()
    if n_in <= 100:
        # exactly the taps float64 ATen gives a non-zero weight: one-hot inputs show them
        assert np.array_equal(_along_width(np.eye(n_in), n_out, antialias).T != 0, ref.dense(t) != 0)


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("n_in,n_out", ref.PAIRS + [(28, 18), (30, 18), (53, 32), (7, 50), (50, 7)])
def test_transposed_table_lists_every_pair_once(rz, n_in, n_out, antialias):
    t = rz.tap_table(n_in, n_out, antialias)
    fwd = [(i, int(t.start[i]) + j, t.weight[t.offset[i] + j]) for i in range(n_out) for j in range(t.counts()[i])]
    bwd = [(int(t.t_start[k]) + j, k, t.t_weight[t.t_offset[k] + j]) for k in range(n_in) for j in range(t.t_counts()[k])]
    assert t.t_start.dtype == np.int32 and t.t_offset.dtype == np.int32 and t.t_weight.dtype == np.float32
    assert len(bwd) == len(fwd) == t.offset[-1] == t.t_offset[-1]
    assert sorted(bwd) == sorted(fwd) and len(set(p[:2] for p in bwd)) == len(bwd)
    assert all(0 <= o < n_out for o, _k, _w in bwd)
    assert np.array_equal(ref.dense_transposed(t), ref.dense(t, use64=False))
    if antialias or n_out >= n_in:
        assert (t.t_counts() >= 1).all()          # (plain bilinear downsampling skips inputs: their gradient is 0)


def test_residue_taps_of_the_gpu_cases(rz):
    """Among the tables the GPU tests use, only 30 -> 18 with antialias has a weight below 2^-20, and it is a rounding
    residue (below 2^-40), kept because float64 ATen keeps it."""
    found = {}
    for shape in ref.SHAPES:
        t, b, l, r = rz.crop_box(shape[-2], shape[-1], *ref.TARGET)
        for n_in, n_out in ((b - t, ref.TARGET[0]), (r - l, ref.TARGET[1])):
            for antialias in (True, False):
                w = rz.tap_table(n_in, n_out, antialias).weight64
                if w.min() < 2.0 ** -20:
                    found[(n_in, n_out, antialias)] = float(w.min())
    assert list(found) == [(30, 18, True)] and 0 < found[(30, 18, True)] < ref.RESIDUE
    assert rz.tap_table(30, 18, True).weight.min() > 0          # (and it survives the rounding to fp32)


def test_tap_table_arguments_and_sharing(rz):
    for bad in ((0, 5), (5, 0), (-3, 5), (5.0, 5), ("5", 5), (1 << 17, 5)):
        with pytest.raises(ValueError):
            rz.tap_table(*bad)
    a = rz.tap_table(29, 18)
    assert a is rz.tap_table(29, 18, True) and a is not rz.tap_table(29, 18, False)
    with pytest.raises(ValueError):
        a.weight[0] = 0.0                                      # shared between calls: read-only
    one = rz.tap_table(5, 1)                                   # any ratio, no tap cap
    assert one.counts().tolist() == [5] and rz.tap_table(1000, 3).counts().max() > 600
    up = rz.tap_table(1, 9)
    assert (up.counts() == 1).all() and (up.start == 0).all() and up.t_counts().tolist() == [9]


def test_device_tables_are_cached_and_bounded(rz):
    dev = torch.device("cpu")                                  # (the cache only moves arrays: any device shows its policy)
    rz._device_tables.clear()
    first = rz._device_table(29, 18, True, dev)
    assert rz._device_table(29, 18, True, dev) is first and rz._device_table(29, 18, False, dev) is not first
    t = rz.tap_table(29, 18, True)
    assert first.idx.dtype == torch.int32 and first.w.dtype == torch.float32
    assert np.array_equal(first.idx.numpy(), np.concatenate([t.start, t.offset]))
    assert np.array_equal(first.w.numpy(), t.weight) and np.array_equal(first.t_w.numpy(), t.t_weight)
    assert np.array_equal(first.t_idx.numpy(), np.concatenate([t.t_start, t.t_offset]))
    for n in range(40, 40 + 2 * rz._CACHE_ENTRIES):
        rz._device_table(n, 18, True, dev)
    assert len(rz._device_tables) == rz._CACHE_ENTRIES
    assert (29, 18, True, "cpu", None) not in rz._device_tables   # the oldest entries went
    rz._device_tables.clear()


def test_the_rasterizers_layout_is_recognised(rz):
    """The 16-byte form is taken for the [1,H,W,4] render seen as [3,H,W] (also cropped, also batched), and only where
    every pixel's 16 bytes lie inside the storage."""
    base = torch.zeros(1, 29, 50, 4)
    view = base[0, :, :, :3].permute(2, 0, 1)
    assert rz._packed4(view[None]) and rz._strides4(view[None]) == [0, 1, 200, 4]
    assert rz._packed4(view[None][:, :, 1:, 5:45])                                    # a crop keeps the layout
    assert rz._packed4(torch.zeros(2, 29, 50, 4)[..., :3].permute(0, 3, 1, 2))
    assert rz._packed4(torch.zeros(1, 29, 50, 4).permute(0, 3, 1, 2))                 # all four channels
    assert not rz._packed4(torch.zeros(1, 3, 29, 50))
    assert not rz._packed4(torch.zeros(1, 29, 50, 3).permute(0, 3, 1, 2))
    assert not rz._packed4(torch.zeros(29 * 50 * 4 + 1)[1:].view(1, 29, 50, 4)[..., :3].permute(0, 3, 1, 2))   # not aligned
    short = torch.zeros(29 * 50 * 4 - 1).as_strided((1, 3, 29, 50), (0, 1, 200, 4))
    assert not rz._packed4(short)                                                      # the last pixel has 12 bytes only
    assert rz._strides4(torch.zeros(2, 3, 29, 50)) == [4350, 1450, 50, 1]


def test_public_functions_refuse_cpu_tensors_and_non_tensors(rz):
    x, m = torch.zeros(3, 29, 50), torch.zeros(1, 29, 50, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="HIP device"):
        rz.resize(x, (18, 32))
    with pytest.raises(RuntimeError, match="HIP device"):
        rz.resize(m, (18, 32))
    with pytest.raises(RuntimeError, match="HIP device"):
        rz.preprocess_tensor(x, 18, 32)
    with pytest.raises(RuntimeError, match="HIP device"):
        rz.novel_view_inputs(x, m, 18, 32)
    with pytest.raises(TypeError):
        rz.resize(np.zeros((3, 29, 50), np.float32), (18, 32))
    with pytest.raises(TypeError):
        rz.novel_view_inputs(x.numpy(), None, 18, 32)


def test_c_entries_check_their_arguments_without_a_gpu(lib):
    """Rejected before any launch: nothing here touches a device (the pointers are made-up addresses)."""
    st = (ctypes.c_int64 * 4)(4500, 1500, 50, 1)
    p = 4096                                                   # "a pointer": never dereferenced by a refused call

    def fwd(x=p, strides=st, B=1, C=3, ih=28, iw=50, ho=18, wo=32, rb=0, flags=0, out=p, ty=p):
        return lib.sc_resize_fwd(x, strides, B, C, ih, iw, ty, p, p, p, ho, wo, rb, flags, 1.0, 0.0, out, None)

    def mask(x=p, strides=st, B=1, C=1, ih=28, iw=50, ho=18, wo=32, rb=0, out=p):
        return lib.sc_resize_mask_fwd(x, strides, B, C, ih, iw, p, p, ho, wo, rb, out, None)

    def bwd(g=p, B=1, C=3, H=29, W=50, top=1, left=0, ih=28, iw=50, ho=18, wo=32, rb=0, flags=0, gx=p):
        return lib.sc_resize_bwd(g, B, C, H, W, top, left, ih, iw, p, p, p, p, ho, wo, rb, flags, 1.0, gx, None)

    for call in (fwd, mask):
        for bad in (dict(x=None), dict(out=None), dict(strides=None), dict(B=0), dict(C=0), dict(B=300, C=300), dict(ih=0),
                    dict(iw=-1), dict(ho=0), dict(wo=0), dict(rb=-1), dict(rb=18), dict(ih=(1 << 16) + 1),
                    dict(strides=(ctypes.c_int64 * 4)(4500, -1500, 50, 1))):
            assert call(**bad) == -1, (call.__name__, bad)
    assert fwd(ty=None) == -1 and fwd(flags=4) == -1
    # the 16-byte form only on the layout it is for: channel stride 1, pixel stride 4, at most 4 channels, aligned
    packed = (ctypes.c_int64 * 4)(8000, 1, 200, 4)
    assert fwd(flags=2) == -1
    assert fwd(flags=2, strides=packed, C=5) == -1
    assert fwd(flags=2, strides=packed, x=4100) == -1
    assert fwd(flags=2, strides=(ctypes.c_int64 * 4)(8000, 1, 202, 4)) == -1
    for bad in (dict(g=None), dict(gx=None), dict(B=0), dict(H=0), dict(W=0), dict(top=-1), dict(left=-1), dict(top=2),
                dict(left=1), dict(ih=30), dict(iw=51), dict(rb=18), dict(flags=2), dict(ho=0)):
        assert bwd(**bad) == -1, bad


def test_both_binding_layers_have_the_entries_and_refuse_cpu_tensors(lib):
    from street_crafter_amd import _ctypes_binding, _lib
    fast = _lib.fast()
    assert fast is not None
    for name in ("resize_fwd", "resize_mask_fwd", "resize_bwd"):
        assert callable(getattr(fast, name)) and callable(getattr(_ctypes_binding, name))
    i, f = torch.zeros(5, dtype=torch.int32), torch.zeros(4)
    with pytest.raises(RuntimeError, match="HIP device"):
        fast.resize_fwd(torch.zeros(1, 3, 4, 4), [48, 16, 4, 1], 1, 3, 4, 4, i, f, i, f, 2, 2, 0, 0, 1.0, 0.0, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        fast.resize_mask_fwd(torch.zeros(1, 1, 4, 4, dtype=torch.bool), [16, 16, 4, 1], 1, 1, 4, 4, i, i, 2, 2, 0, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        fast.resize_bwd(torch.zeros(1, 3, 2, 2), 1, 3, 4, 4, 0, 0, 4, 4, i, f, i, f, 2, 2, 0, 0, 1.0, 0)


def test_nothing_imports_the_module_by_default():
    """Opt-in: no other product module names it."""
    pat = re.compile(r"^\s*(from\s+\.resize\s+import|from\s+\.\s+import\s+.*\bresize\b|"
                     r"(import|from)\s+street_crafter_amd\.resize\b|from\s+street_crafter_amd\s+import\s+.*\bresize\b)", re.M)
    for pkg in ("street_crafter_amd", "gsplat", "simple_knn", "nvdiffrast", "diff_point_rasterization"):
        for path in glob.glob(os.path.join(ROOT, pkg, "**", "*.py"), recursive=True):
            if os.path.basename(path) == "resize.py":
                continue
            assert not pat.search(open(path).read()), path
