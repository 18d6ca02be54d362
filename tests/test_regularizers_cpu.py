"""No-GPU checks of the regularizers (csrc/regularizers.hip, street_crafter_amd/regularizers.py):
- float64 references of the LiDAR depth loss and the sky / object accumulation losses, written with the reference's
  own torch expressions (train.py:194-220), reproduce those expressions run in fp32 on the CPU;
- k = int(0.95 * n), which the device forms as a truncated double product, equals (19 n) // 20 for every n up to 3e6;
- the C ABI refuses every bad argument before touching a device;
- the Python operators refuse CPU tensors, other dtypes, mismatched shapes and keep outside (0, 1]."""
import ctypes

import numpy as np
import pytest
import torch


# ---- float64 references (the reference's expressions) -----------------------------------------------------------
def lidar_depth_f64(depth, lidar_depth, mask=None, keep=0.95):
    """train.py:213-218 with the error formed in fp32, as the reference forms it, then selected and averaged in float64.
    -> (value, sorted kept errors (fp32 values, float64 tensor), n, k)."""
    if mask is None:
        mask = torch.ones_like(lidar_depth, dtype=torch.bool)
    depth_mask = torch.logical_and(lidar_depth > 0., mask)
    e = torch.abs(depth.float()[depth_mask] - lidar_depth.float()[depth_mask]).double()
    n = e.size(0)
    k = int(keep * n)
    sel, _ = torch.topk(e, k, largest=False)
    return sel.mean(), torch.sort(e)[0], n, k


def lidar_depth_torch(depth, lidar_depth, mask, keep=0.95):
    """train.py:213-218 verbatim (the dtype of its inputs)."""
    depth_mask = torch.logical_and((lidar_depth > 0.), mask)
    depth_error = torch.abs((depth[depth_mask] - lidar_depth[depth_mask]))
    depth_error, _ = torch.topk(depth_error, int(keep * depth_error.size(0)), largest=False)
    return depth_error.mean()


def sky_torch(acc, sky_mask):
    """train.py:194-196 verbatim."""
    acc = torch.clamp(acc, min=1e-6, max=1. - 1e-6)
    return torch.where(sky_mask, -torch.log(1 - acc), -(acc * torch.log(acc) + (1. - acc) * torch.log(1. - acc))).mean()


def obj_torch(acc_obj, obj_bound):
    """train.py:205-206 verbatim."""
    acc_obj = torch.clamp(acc_obj, min=1e-6, max=1. - 1e-6)
    return torch.where(obj_bound, -(acc_obj * torch.log(acc_obj) + (1. - acc_obj) * torch.log(1. - acc_obj)),
                       -torch.log(1. - acc_obj)).mean()


def acc_f64(acc, mask, mode):
    """The accumulation losses in float64, clamped at the reference's fp32 bounds (mode 0 sky, 1 object)."""
    lo, hi = float(np.float32(1e-6)), float(np.float32(1. - 1e-6))
    a = torch.clamp(acc.double(), min=lo, max=hi)
    lg = -torch.log(1 - a)
    ent = -(a * torch.log(a) + (1. - a) * torch.log(1. - a))
    return (torch.where(mask, lg, ent) if mode == 0 else torch.where(mask, ent, lg)).mean()


def _depth_case(H, W, density, seed):
    g = torch.Generator().manual_seed(seed)
    depth = 1 + 50 * torch.rand(1, H, W, generator=g)
    lidar = depth + torch.randn(1, H, W, generator=g)
    lidar[torch.rand(1, H, W, generator=g) > density] = 0.0
    mask = torch.rand(1, H, W, generator=g) > 0.1
    return depth, lidar, mask


@pytest.mark.parametrize("H,W,density", [(7, 13, 0.3), (37, 53, 0.05), (37, 53, 1.0), (64, 64, 0.3)])
def test_depth_reference_matches_train_py(H, W, density):
    depth, lidar, mask = _depth_case(H, W, density, seed=H * W)
    v64, srt, n, k = lidar_depth_f64(depth, lidar, mask)
    v32 = lidar_depth_torch(depth, lidar, mask)
    assert k >= 1
    assert abs(float(v32) - float(v64)) <= 1e-6 * abs(float(v64)) + 1e-7
    # the k smallest of the sorted errors are exactly what topk keeps
    assert float(srt[:k].mean()) == pytest.approx(float(v64), rel=1e-15)
    # and their gradients agree on which pixels are selected (no ties here)
    d = depth.clone().requires_grad_(True)
    lidar_depth_torch(d, lidar, mask).backward()
    assert int((d.grad != 0).sum()) == k


def test_depth_reference_empty_selection_is_nan():
    depth = torch.ones(1, 3, 3)
    lidar = torch.zeros(1, 3, 3)
    mask = torch.ones(1, 3, 3, dtype=torch.bool)
    assert torch.isnan(lidar_depth_torch(depth, lidar, mask))       # n = 0
    lidar[0, 1, 1] = 2.0
    assert torch.isnan(lidar_depth_torch(depth, lidar, mask))       # n = 1: k = int(0.95) = 0
    assert torch.isnan(lidar_depth_f64(depth, lidar, mask)[0])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Cm", [1, 3])
def test_acc_reference_matches_train_py(mode, Cm):
    g = torch.Generator().manual_seed(7 + Cm + mode)
    acc = torch.rand(1, 29, 41, generator=g)
    acc[0, 0, :5] = torch.tensor([0.0, 1.0, 1e-6, 1. - 1e-6, 1e-9])
    mask = torch.rand(Cm, 29, 41, generator=g) > 0.5
    ref = (sky_torch if mode == 0 else obj_torch)(acc, mask)
    v64 = acc_f64(acc, mask, mode)
    assert abs(float(ref) - float(v64)) <= 2e-6 * abs(float(v64))


def test_keep_count_for_every_n():
    """k = int(0.95 * n): the device's (long long)(keep * (double)n) is numpy's truncated float64 product; both equal
    (19 n) // 20 for every n in [0, 3e6]."""
    n = np.arange(3_000_001, dtype=np.int64)
    dev = (0.95 * n.astype(np.float64)).astype(np.int64)
    np.testing.assert_array_equal(dev, (19 * n) // 20)
    step = 997                                      # Python's own int(0.95 * n) on a sample plus the ends
    for i in list(range(0, 3_000_001, step)) + list(range(2_999_000, 3_000_001)):
        assert int(0.95 * i) == dev[i], i


# ---- C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


FAKE = 0x10000      # a non-null pointer that is never dereferenced: every call below is refused on the host


def _st(n, vals=None):
    v = vals if vals is not None else [8, 1] * (n // 2) + ([1] if n % 2 else [])
    return (ctypes.c_int64 * n)(*v)


def _dfwd(lib, H=8, W=8, keep=0.95, ptr=FAKE, value=FAKE, ws=FAKE, ws_bytes=1 << 20, st=None, strides=True):
    return lib.sc_depth_trim_fwd(ptr, ptr, None, _st(6, st) if strides else None, H, W, keep, value, None, None, ws,
                                 ws_bytes, None)


def _dbwd(lib, H=8, W=8, ptr=FAKE, g=FAKE, ws=FAKE, ws_bytes=1 << 20, gd=FAKE, gl=None, st=None):
    return lib.sc_depth_trim_bwd(ptr, ptr, None, _st(6, st), H, W, g, ws, ws_bytes, gd, gl, None)


def _afwd(lib, Cm=1, H=8, W=8, mode=0, ptr=FAKE, mask=FAKE, value=FAKE, ws=FAKE, ws_bytes=1 << 20, st=None):
    return lib.sc_acc_reg_fwd(ptr, mask, _st(5, st), Cm, H, W, mode, value, ws, ws_bytes, None)


def _abwd(lib, Cm=1, H=8, W=8, mode=0, ptr=FAKE, mask=FAKE, g=FAKE, ga=FAKE, st=None):
    return lib.sc_acc_reg_bwd(ptr, mask, _st(5, st), Cm, H, W, mode, g, ga, None)


def test_depth_trim_abi_refuses_bad_arguments(lib):
    assert lib.sc_depth_trim_workspace_bytes(8, 8) > 8 * 8 * 4
    for bad in ((0, 8), (8, 0), (-1, 8), (8, -3), (1 << 16, 1 << 15)):
        assert lib.sc_depth_trim_workspace_bytes(*bad) == 0
    for kw in (dict(H=0), dict(W=0), dict(H=-1), dict(W=-7), dict(H=1 << 16, W=1 << 15)):
        assert _dfwd(lib, **kw) == -1, kw
        assert _dbwd(lib, **kw) == -1, kw
    for keep in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert _dfwd(lib, keep=keep) == -1, keep
    assert _dfwd(lib, keep=1.0, ws_bytes=8) == -2                    # keep = 1 is allowed: refused for the workspace
    assert _dfwd(lib, ptr=None) == -1
    assert _dfwd(lib, value=None) == -1
    assert _dfwd(lib, ws=None) == -1
    assert _dfwd(lib, strides=False) == -1
    assert _dfwd(lib, st=[8, 1, 8, -1, 8, 1]) == -1
    assert _dbwd(lib, ptr=None) == -1
    assert _dbwd(lib, g=None) == -1
    assert _dbwd(lib, ws=None) == -1
    assert _dbwd(lib, gd=None, gl=None) == -1                        # no gradient asked for
    assert _dbwd(lib, st=[-8, 1, 8, 1, 8, 1]) == -1
    # a workspace too small
    need = lib.sc_depth_trim_workspace_bytes(8, 8)
    assert _dfwd(lib, ws_bytes=need - 1) == -2
    assert _dbwd(lib, ws_bytes=need - 1) == -2


def test_acc_reg_abi_refuses_bad_arguments(lib):
    assert lib.sc_acc_reg_workspace_bytes(8, 8) > 0
    for bad in ((0, 8), (8, 0), (-2, 8)):
        assert lib.sc_acc_reg_workspace_bytes(*bad) == 0
    for kw in (dict(H=0), dict(W=0), dict(H=-4), dict(Cm=0), dict(Cm=-1), dict(mode=2), dict(mode=-1),
               dict(ptr=None), dict(mask=None), dict(st=[8, 1, 64, 8, -1])):
        assert _afwd(lib, **kw) == -1, kw
        assert _abwd(lib, **kw) == -1, kw
    assert _afwd(lib, value=None) == -1
    assert _afwd(lib, ws=None) == -1
    assert _abwd(lib, g=None) == -1
    assert _abwd(lib, ga=None) == -1
    assert _afwd(lib, ws_bytes=0) == -2


def test_library_exports_the_regularizers(lib):
    from street_crafter_amd import _lib
    for name in ("sc_depth_trim_workspace_bytes", "sc_depth_trim_fwd", "sc_depth_trim_bwd",
                 "sc_acc_reg_workspace_bytes", "sc_acc_reg_fwd", "sc_acc_reg_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


# ---- Python refusals -------------------------------------------------------------------------------------------
def _pretend_hip(monkeypatch):
    """Lets CPU tensors past the device check, so that the checks behind it (dtype, shapes, keep) are reached here
    without a GPU; every call in these tests is refused before anything is launched."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))


def _ops():
    from street_crafter_amd import regularizers as R
    return R


def test_regularizers_refuse_cpu_tensors():
    R = _ops()
    d, m = torch.rand(1, 8, 8), torch.ones(1, 8, 8, dtype=torch.bool)
    for fn in (lambda: R.lidar_depth_loss(d, d, m), lambda: R.lidar_depth_forward(d, d), lambda: R.sky_loss(d, m),
               lambda: R.obj_acc_loss(d, m)):
        with pytest.raises(ValueError, match="HIP device"):
            fn()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_regularizers_refuse_other_dtypes(monkeypatch, dtype):
    R = _ops()
    _pretend_hip(monkeypatch)
    d, m = torch.rand(1, 8, 8).to(dtype), torch.ones(1, 8, 8, dtype=torch.bool)
    f = torch.rand(1, 8, 8)
    for fn in (lambda: R.lidar_depth_loss(d, f, m), lambda: R.lidar_depth_loss(f, d, m), lambda: R.sky_loss(d, m),
               lambda: R.obj_acc_loss(d, m)):
        with pytest.raises(ValueError, match="float32"):
            fn()
    with pytest.raises(ValueError, match="bool"):
        R.sky_loss(f, m.float())
    with pytest.raises(ValueError, match="bool"):
        R.lidar_depth_loss(f, f, m.to(torch.uint8))


def test_regularizers_refuse_shapes_and_keep(monkeypatch):
    R = _ops()
    _pretend_hip(monkeypatch)
    d, m = torch.rand(1, 8, 9), torch.ones(1, 8, 9, dtype=torch.bool)
    with pytest.raises(ValueError, match="mismatch"):
        R.lidar_depth_loss(d, torch.rand(1, 9, 8), m)
    with pytest.raises(ValueError, match="does not match"):
        R.lidar_depth_loss(d, d, torch.ones(1, 8, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="does not match"):
        R.lidar_depth_loss(d, d, torch.ones(2, 8, 9, dtype=torch.bool))     # the depth mask is [1,H,W]
    with pytest.raises(ValueError, match="does not match"):
        R.sky_loss(d, torch.ones(3, 9, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="does not match"):
        R.obj_acc_loss(d, torch.ones(8, 9, dtype=torch.bool))
    for bad in (torch.rand(8, 9), torch.rand(2, 8, 9), torch.rand(1, 1, 8, 9), torch.rand(1, 0, 9)):
        with pytest.raises(ValueError):
            R.lidar_depth_loss(bad, bad)
        with pytest.raises(ValueError):
            R.sky_loss(bad, m)
    for keep in (0.0, -0.1, 1.5, float("nan"), float("inf"), "0.9", True):
        with pytest.raises(ValueError, match="keep"):
            R.lidar_depth_loss(d, d, m, keep=keep)
    # keep = 1.0 and a multi-channel accumulation mask pass the checks
    from street_crafter_amd import regularizers
    assert regularizers._check_depth(d, d, m, 1.0, "t")[:2] == (8, 9)
    assert regularizers._check_acc(d, torch.ones(3, 8, 9, dtype=torch.bool), "t")[:3] == (3, 8, 9)
