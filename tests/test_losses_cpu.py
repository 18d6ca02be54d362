"""No-GPU checks of the fused photometric loss (csrc/losses.hip, street_crafter_amd/losses.py):
- a float64 restatement of the reference's ssim / l1_loss (loss_utils.py:21-37, 95-131) reproduces the reference's own
  float64 values and autograd gradients stored in tests/golden/losses_ref.npz;
- the C ABI refuses every bad argument with SC_EINVAL before touching a device;
- the Python operators refuse CPU tensors, other dtypes, other windows, mismatched shapes and the 3-D
  size_average=False call."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "losses_ref.npz")

# loss_utils.gaussian(11, 1.5) in fp32; the reference's window is their fp32 outer product
_G32 = torch.tensor([float.fromhex(h) for h in (
    "0x1.0d956cp-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.106560p-2",
    "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d956cp-10")], dtype=torch.float32)


def ssim_f64(x, y, mask=None, size_average=True):
    """The reference's ssim formula, restated in float64 on the CPU (x, y: [C,H,W] or [B,C,H,W]; mask [1,H,W])."""
    x, y = x.double(), y.double()
    C = x.shape[-3]
    w = torch.outer(_G32, _G32).double().expand(C, 1, 11, 11)
    if mask is not None:
        x, y = torch.where(mask, x, torch.zeros_like(x)), torch.where(mask, y, torch.zeros_like(y))
    f = (lambda t: F.conv2d(t, w, padding=5, groups=C))
    mu1, mu2 = f(x), f(y)
    s1, s2, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return m.mean() if size_average else m.flatten(1).mean(1)


def l1_f64(x, y, mask=None):
    """The reference's l1_loss in float64: mean |x - y| over the (pixel, channel) entries the [1,H,W] mask keeps."""
    d = (x.double() - y.double()).abs()
    if mask is not None:
        d = d[mask.expand_as(d)]
    return d.mean()


def train_loss_f64(x, y, mask=None):
    return 0.8 * l1_f64(x, y, mask) + 0.2 * (1.0 - ssim_f64(x, y, mask))


def _case(d, name):
    base = name[:-2] if name.endswith("_m") else name
    x, y = torch.from_numpy(d[f"{base}_img1"]), torch.from_numpy(d[f"{base}_img2"])
    m = torch.from_numpy(d[f"{name}_mask"]) if f"{name}_mask" in d.files else None
    return x, y, m


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name", ["rand", "rand_m", "smooth", "smooth_m"])
def test_restatement_matches_reference_f64(gold, name):
    x, y, m = _case(gold, name)
    gi = 1 if f"{name}_grad1_f64" in gold.files else 2
    a, b = x.double().requires_grad_(True), y.double().requires_grad_(True)
    s, l = ssim_f64(a, b, m), l1_f64(a, b, m)
    (0.8 * l + 0.2 * (1.0 - s)).backward()
    assert abs(s.item() - gold[f"{name}_ssim_f64"]) <= 1e-12
    assert abs(l.item() - gold[f"{name}_l1_f64"]) <= 1e-12
    g = (a if gi == 1 else b).grad.numpy()
    np.testing.assert_allclose(g, gold[f"{name}_grad{gi}_f64"], rtol=0, atol=1e-12)


def test_restatement_matches_reference_batch_and_crop(gold):
    x, y = (torch.from_numpy(gold[k]).double().requires_grad_(True) for k in ("batch_img1", "batch_img2"))
    s = ssim_f64(x, y, size_average=False)
    s.sum().backward()
    np.testing.assert_allclose(s.detach().numpy(), gold["batch_ssim_f64"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(x.grad.numpy(), gold["batch_grad1_f64"], rtol=0, atol=1e-12)

    up = int(gold["crop_upper"])
    rc = torch.from_numpy(gold["crop_img1"]).double().requires_grad_(True)
    gt = torch.from_numpy(gold["crop_img2"]).double()
    m = torch.from_numpy(gold["crop_mask"])
    view = (lambda t: t[0, ..., :3].permute(2, 0, 1)[:, up:, :])
    s, l = ssim_f64(view(rc), view(gt), m), l1_f64(view(rc), view(gt), m)
    (0.8 * l + 0.2 * (1.0 - s)).backward()
    assert abs(s.item() - gold["crop_ssim_f64"]) <= 1e-12 and abs(l.item() - gold["crop_l1_f64"]) <= 1e-12
    np.testing.assert_allclose(rc.grad.numpy(), gold["crop_grad1_f64"], rtol=0, atol=1e-12)


def test_fixture_is_small_and_holds_data_only(gold):
    assert os.path.getsize(GOLD) < 1 << 20
    assert all(gold[k].dtype.kind in "fbi" for k in gold.files)


# ---- C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


FAKE = 0x10000      # a non-null pointer that is never dereferenced: every call below is refused on the host


def _st(vals=None):
    v = vals if vals is not None else [0, 3 * 8 * 8, 8, 1, 0, 3 * 8 * 8, 8, 1, 0, 8, 1]
    return (ctypes.c_int64 * 11)(*v)


def _fwd(lib, B=1, C=3, H=8, W=8, mask=None, mb=1, mh=8, mw=8, win=11, st=None, ptr=FAKE, ws_bytes=1 << 20,
         maps=(None, None, None, None), ssim=FAKE, strides=True):
    return lib.sc_loss_fwd(ptr, ptr, mask, _st(st) if strides else None, B, C, H, W, mb, mh, mw, win, ssim, FAKE, None,
                           *maps, FAKE, ws_bytes, None)


def _bwd(lib, B=1, C=3, H=8, W=8, mask=None, mb=1, mh=8, mw=8, win=11, maps=(FAKE, None, FAKE, FAKE), g_ssim=FAKE,
         g_l1=FAKE, kept=FAKE, g1=FAKE, g2=None, ptr=FAKE):
    return lib.sc_loss_bwd(ptr, ptr, mask, _st(), B, C, H, W, mb, mh, mw, win, *maps, g_ssim, g_l1, kept, g1, g2, None)


def test_loss_abi_refuses_bad_arguments(lib):
    assert lib.sc_loss_workspace_bytes(1, 3, 8, 8) > 0
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert lib.sc_loss_workspace_bytes(*bad) == 0
    for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-5), dict(W=-5)):
        assert _fwd(lib, **kw) == -1, kw
        assert _bwd(lib, **kw) == -1, kw
    for win in (9, 7, 0, 13):
        assert _fwd(lib, win=win) == -1
        assert _bwd(lib, win=win) == -1
    # a mask whose shape does not broadcast: batch other than 1 / B, rows or columns other than H / W
    assert _fwd(lib, B=2, mask=FAKE, mb=3) == -1
    assert _fwd(lib, mask=FAKE, mh=7) == -1
    assert _fwd(lib, mask=FAKE, mw=9) == -1
    assert _bwd(lib, mask=FAKE, mw=9) == -1
    # null required pointers
    assert _fwd(lib, ptr=None) == -1
    assert _fwd(lib, ssim=None) == -1
    assert _fwd(lib, strides=False) == -1
    assert _bwd(lib, ptr=None) == -1
    assert _bwd(lib, g1=None, g2=None) == -1                         # no gradient asked for
    assert _bwd(lib, maps=(None, None, FAKE, FAKE)) == -1            # grad1 without a1
    assert _bwd(lib, g2=FAKE) == -1                                  # grad2 without a2
    assert _bwd(lib, kept=None) == -1                                # L1 term without the counts
    # incomplete map sets in the forward
    assert _fwd(lib, maps=(FAKE, None, None, FAKE)) == -1
    assert _fwd(lib, maps=(FAKE, None, FAKE, None)) == -1
    assert _fwd(lib, maps=(None, None, FAKE, FAKE)) == -1
    # negative strides, a workspace too small
    assert _fwd(lib, st=[0, 64, 8, -1, 0, 64, 8, 1, 0, 8, 1]) == -1
    assert _fwd(lib, ws_bytes=8) == -2


# ---- Python refusals -------------------------------------------------------------------------------------------
def test_losses_refuse_cpu_tensors():
    from street_crafter_amd import losses
    x = torch.rand(3, 16, 16)
    for fn in (lambda: losses.ssim(x, x), lambda: losses.l1_loss(x, x), lambda: losses.l1_and_ssim(x, x)):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_losses_refuse_other_dtypes(monkeypatch, dtype):
    from street_crafter_amd import losses
    _pretend_hip(monkeypatch)
    x = torch.rand(3, 16, 16).to(dtype)
    for fn in (lambda: losses.ssim(x, x), lambda: losses.l1_loss(x, x), lambda: losses.l1_and_ssim(x, x)):
        with pytest.raises(ValueError, match="float32"):
            fn()


def test_losses_refuse_window_shape_and_3d_per_image(monkeypatch):
    from street_crafter_amd import losses
    _pretend_hip(monkeypatch)
    x, y = torch.rand(3, 16, 16), torch.rand(3, 16, 17)
    with pytest.raises(ValueError, match="window"):
        losses.ssim(x, x, window_size=9)
    with pytest.raises(ValueError, match="mismatch"):
        losses.ssim(x, y)
    with pytest.raises(ValueError, match="mismatch"):
        losses.l1_loss(x, y)
    with pytest.raises(ValueError, match="mismatch"):
        losses.l1_and_ssim(x, y)
    with pytest.raises(ValueError, match="reference raises"):
        losses.ssim(x, x, size_average=False)
    with pytest.raises(ValueError, match="broadcast"):
        losses.ssim(x, x, mask=torch.ones(2, 16, 16, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool"):
        losses.ssim(x, x, mask=torch.ones(1, 16, 16))


def _pretend_hip(monkeypatch):
    """Lets CPU tensors past the device check, so that the checks behind it (dtype, window, shapes) are reached here
    without a GPU; every call in these tests is refused before anything is launched."""
    from street_crafter_amd import losses
    orig = losses._check

    def check(img1, img2, mask, window_size, what):
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
            return orig(img1, img2, mask, window_size, what)
    monkeypatch.setattr(losses, "_check", check)
