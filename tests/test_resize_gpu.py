"""GPU checks of the crop + resize kernels (csrc/resize.hip through street_crafter_amd/resize.py) against torch's own
`F.interpolate` on the CPU in float64 (tests/resize_ref.py), on the same fp32 inputs.

Forward, every element, no exclusions:   |hip - f64| <= 2^-24 (Ty + Tx + 4) A,  Ty, Tx the output's tap counts and
A = sum wy wx |x| over its taps: the dot-product rounding bound of the two nested sums (Tx roundings in the row sum, Ty in
the sum of rows) plus one rounding of each of the two weights, with 2 to spare.  With the affine epilogue out * a + b (one
more fma) the bar is |a| (1 + 2^-24) bar + 2^-24 |f64|: the sum's error scaled, plus the rounding of the result.
Backward, every input element:           |hip - f64| <= 2^-24 (n + 4) S,  n the contributing outputs and S the sum of
|wy wx g| over them (the kernel's nested sum has ny + nx roundings plus the weights', and ny + nx <= ny nx + 1); exactly
+0 outside the crop and where only rows above row_begin reach.
Mask: equal to `F.interpolate(mask.double()) != 0` on every pixel.  A pixel whose float64 value lies in (0, 2^-20) is one
no implementation can be held to; the test asserts that these are exactly the pixels whose only set taps are rounding
residues of ATen's own weights (tests/test_resize_cpu.py: of the tables used here only 30 -> 18 with antialias has one), so
there are none in every other case.

Reached on an MI355X (printed per case): forward 0.37 of the bar at most, backward 0.56; with the affine epilogue 0.92
forward (the last rounding alone can reach 1: a result just above a power of two) and 0.55 backward.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = ref.EPS
TH, TW = ref.TARGET
LAYOUTS = ["contiguous", "raster", "batch"]


@pytest.fixture(scope="module")
def rz():
    from street_crafter_amd import _lib, resize
    _lib.load()
    return resize


def _place(x_np, layout, grad=False):
    """-> (the tensor handed to the operator, the leaf that receives the gradient, leaf gradient -> x's layout)."""
    x = torch.from_numpy(x_np).to(DEV)
    if layout == "raster":                    # the rasterizer's [1,H,W,4] output seen as [3,H,W]
        assert x.dim() == 3 and x.shape[0] == 3
        H, W = x.shape[-2:]
        base = torch.full((1, H, W, 4), 7.0, device=DEV)
        base[0, :, :, :3] = x.permute(1, 2, 0)
        base.requires_grad_(grad)
        return base[0, :, :, :3].permute(2, 0, 1), base, lambda g: g[0, :, :, :3].permute(2, 0, 1)
    x.requires_grad_(grad)
    return x, x, lambda g: g


def _input(shape, layout, seed):
    return ref.image((2,) + shape if layout == "batch" else shape, seed)


def _ratio(err, bar):
    assert (err[bar == 0] == 0).all()
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
@pytest.mark.parametrize("row_begin", [0, ref.UPPER])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=[f"{h}x{w}" for _c, h, w in ref.SHAPES])
def test_forward_and_backward_are_within_the_bars_of_float64_everywhere(rz, shape, layout, row_begin, antialias):
    x_np = _input(shape, layout, seed=shape[1] * 100 + shape[2])
    T = ref.Truth(rz, x_np, ref.TARGET, antialias, row_begin)
    x, leaf, back = _place(x_np, layout, grad=True)
    out = rz.preprocess_tensor(x, TH, TW, antialias, row_begin=row_begin)
    want, bar, _A = T.forward()
    assert out.shape == want.shape and out.is_contiguous() and out.dtype == torch.float32
    err = np.abs(_f64(out) - want)
    what = f"{shape} {layout} row_begin={row_begin} antialias={antialias}"
    print(f"{what}: forward reached {_ratio(err, bar):.3f} of the bar")
    assert (err <= bar).all()

    g = ref.image(want.shape, seed=7 + row_begin)
    out.backward(torch.from_numpy(g).to(DEV))
    got = _f64(back(leaf.grad))
    want_g, bar_g, reached = T.backward(g)
    err = np.abs(got - want_g)
    print(f"{what}: backward reached {_ratio(err, bar_g):.3f} of the bar")
    assert (err <= bar_g).all()
    assert (got[~reached] == 0).all() and not np.signbit(got[~reached]).any()
    if layout == "raster":
        assert (leaf.grad[..., 3] == 0).all()                     # the fourth channel of the render is not an input
    # float64 autograd of crop + interpolate says the same as the closed form the bar is built on
    _y, auto = T.autograd(g)
    assert np.abs(auto - want_g).max() <= 1e-14


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=[f"{h}x{w}" for _c, h, w in ref.SHAPES])
def test_affine_epilogue_and_novel_view_inputs_against_float64_autograd(rz, shape, antialias):
    x_np = _input(shape, "contiguous", seed=shape[1])
    # preprocess_tensor(scale=2, shift=-1): the diffusion inputs' `* 2 - 1`
    for row_begin in (0, ref.UPPER):
        T = ref.Truth(rz, x_np, ref.TARGET, antialias, row_begin)
        x, leaf, back = _place(x_np, "raster", grad=True)
        out = rz.preprocess_tensor(x, TH, TW, antialias, row_begin=row_begin, scale=2.0, shift=-1.0)
        g = ref.image(out.shape, seed=11)
        out.backward(torch.from_numpy(g).to(DEV))
        want, want_g = T.autograd(g, scale=2.0, shift=-1.0)
        _w, bar0, _A = T.forward()
        bar = 2.0 * (1 + EPS) * bar0 + EPS * np.abs(want)
        err = np.abs(_f64(out) - want)
        print(f"{shape} affine row_begin={row_begin} antialias={antialias}: forward reached {_ratio(err, bar):.3f} of the bar")
        assert (err <= bar).all()
        _wg, bar_g, reached = T.backward(g, scale=2.0)
        got = _f64(back(leaf.grad))
        err = np.abs(got - want_g)
        print(f"{shape} affine row_begin={row_begin} antialias={antialias}: backward reached {_ratio(err, bar_g):.3f} of the bar")
        assert (err <= bar_g).all()
        assert (got[~reached] == 0).all() and not np.signbit(got[~reached]).any()
        # a negative factor must not turn the untouched elements into -0
        x2, leaf2, back2 = _place(x_np, "contiguous", grad=True)
        rz.preprocess_tensor(x2, TH, TW, antialias, row_begin=row_begin, scale=-3.0).backward(torch.from_numpy(g).to(DEV))
        got2 = _f64(leaf2.grad)
        assert (got2[~reached] == 0).all() and not np.signbit(got2[~reached]).any()
        assert np.abs(got2 - (-1.5) * want_g).max() <= 1.5 * bar_g.max() + 1e-30

    # novel_view_inputs: train.py:160-169
    T = ref.Truth(rz, x_np, ref.TARGET, antialias, ref.UPPER)
    m_np = ref.mask(shape, 0.7, seed=5)
    x, leaf, back = _place(x_np, "raster", grad=True)
    image_loss, mask_loss, upper = rz.novel_view_inputs(x, torch.from_numpy(m_np).to(DEV), TH, TW, antialias)
    assert upper == ref.UPPER == 7 and image_loss.shape == (3, TH - upper, TW) and mask_loss.shape == (1, TH - upper, TW)
    assert mask_loss.dtype == torch.bool and image_loss.is_contiguous() and mask_loss.is_contiguous()
    g = ref.image(image_loss.shape, seed=13)
    image_loss.backward(torch.from_numpy(g).to(DEV))
    want, want_g = T.autograd(g)
    _w, bar, _A = T.forward()
    assert (np.abs(_f64(image_loss) - want) <= bar).all()
    _wg, bar_g, reached = T.backward(g)
    got = _f64(back(leaf.grad))
    assert (np.abs(got - want_g) <= bar_g).all() and (got[~reached] == 0).all()
    assert np.array_equal(mask_loss.cpu().numpy(), T.mask(m_np)[0])
    # the rows it returns are the rows of the whole result, bit for bit: row_begin only skips work
    with torch.no_grad():
        whole = rz.preprocess_tensor(x, TH, TW, antialias)
        whole_m = rz.preprocess_tensor(torch.from_numpy(m_np).to(DEV), TH, TW, antialias)
        assert torch.equal(whole[:, upper:], image_loss) and torch.equal(whole_m[:, upper:], mask_loss)
        none = rz.novel_view_inputs(x, None, TH, TW, antialias)
        assert none[1] is None and none[2] == upper and torch.equal(none[0], image_loss)


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
@pytest.mark.parametrize("frac", [0.5, 0.05])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=[f"{h}x{w}" for _c, h, w in ref.SHAPES])
def test_mask_is_where_float64_interpolate_is_not_zero(rz, shape, frac, antialias):
    m_np = ref.mask(shape, frac, seed=shape[2] + int(100 * frac))
    H, W = shape[-2:]
    views = {"contiguous": torch.from_numpy(m_np).to(DEV)}
    two = torch.zeros((H, W, 2), dtype=torch.bool, device=DEV)
    two[..., 1] = views["contiguous"][0]
    views["strided"] = two[..., 1][None]
    views["batch"] = torch.stack([views["contiguous"], ~views["contiguous"]])
    residues = 0
    for row_begin in (0, ref.UPPER):
        T = ref.Truth(rz, m_np, ref.TARGET, antialias, row_begin)
        want, v, residue_only = T.mask(m_np)
        undecidable = (v > 0) & (v < 2.0 ** -20)
        assert np.array_equal(undecidable, residue_only)
        residues += int(undecidable.sum())
        for name, m in views.items():
            got = rz.preprocess_tensor(m, TH, TW, antialias, row_begin=row_begin)
            assert got.dtype == torch.bool and got.is_contiguous()
            if name == "batch":
                assert got.shape == (2,) + want.shape and np.array_equal(got[0].cpu().numpy(), want)
                assert np.array_equal(got[1].cpu().numpy(), T.mask(~m_np)[0])
            else:
                assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), name
    print(f"{shape} {frac} antialias={antialias}: {residues} pixels set by residue taps alone")
    assert residues == 0 or (antialias and shape == (3, 30, 64))


def test_resize_takes_any_leading_dimensions_and_both_dtypes(rz):
    x_np = ref.image((2, 2, 3, 29, 50), seed=3)
    T = ref.Truth(rz, x_np, ref.TARGET, True, crop=False)
    want, bar, _A = T.forward()
    x = torch.from_numpy(x_np).to(DEV).requires_grad_(True)
    out = rz.resize(x, ref.TARGET)
    assert out.shape == (2, 2, 3, TH, TW) and (np.abs(_f64(out) - want) <= bar).all()
    g = ref.image(want.shape, seed=4)
    out.backward(torch.from_numpy(g).to(DEV))
    want_g, bar_g, _r = T.backward(g)
    assert (np.abs(_f64(x.grad) - want_g) <= bar_g).all()
    plane = rz.resize(x.detach()[0, 0, 0], ref.TARGET, antialias=False)             # [H,W]
    assert plane.shape == ref.TARGET and not plane.requires_grad
    Tp = ref.Truth(rz, x_np[0, 0, 0], ref.TARGET, False, crop=False)
    wp, bp, _A = Tp.forward()
    assert (np.abs(_f64(plane) - wp) <= bp).all()
    m_np = ref.mask((1, 29, 50), 0.3, seed=9)
    got = rz.resize(torch.from_numpy(m_np).to(DEV), ref.TARGET)
    assert np.array_equal(got.cpu().numpy(), ref.Truth(rz, m_np, ref.TARGET, True, crop=False).mask(m_np)[0])
    up = rz.resize(x.detach()[0, 0], (64, 70))                                     # several workgroups in both axes
    Tu = ref.Truth(rz, x_np[0, 0], (64, 70), True, crop=False)
    wu, bu, _A = Tu.forward()
    assert (np.abs(_f64(up) - wu) <= bu).all()


def test_two_runs_are_bitwise_equal_and_both_bindings_agree(rz):
    from street_crafter_amd import _lib
    x_np, g_np = ref.image((3, 45, 80), seed=1), ref.image((3, TH - ref.UPPER, TW), seed=2)
    runs = []
    for fast in (True, True, False):
        prev = _lib.set_fast_binding(fast)
        try:
            x, leaf, _back = _place(x_np, "raster", grad=True)
            out = rz.preprocess_tensor(x, TH, TW, True, row_begin=ref.UPPER, scale=2.0, shift=-1.0)
            out.backward(torch.from_numpy(g_np).to(DEV))
            runs.append((out.detach().clone(), leaf.grad.clone()))
        finally:
            _lib.set_fast_binding(prev)
    for out, grad in runs[1:]:
        assert torch.equal(out, runs[0][0]) and torch.equal(grad, runs[0][1])


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
@pytest.mark.parametrize("layout", ["contiguous", "raster"])
def test_one_nan_reaches_exactly_the_outputs_whose_tables_hold_it(rz, layout, antialias):
    shape, row_begin = (3, 29, 50), 2
    x_np = ref.image(shape, seed=21)
    T = ref.Truth(rz, x_np, ref.TARGET, antialias, row_begin)
    top, _b, left, _r = T.box
    c, iy, ix = 1, 13, 20                              # a pixel of the cropped region
    with torch.no_grad():
        clean = rz.preprocess_tensor(_place(x_np, layout)[0], TH, TW, antialias, row_begin=row_begin)
        bad_np = x_np.copy()
        bad_np[c, top + iy, left + ix] = np.nan
        bad = rz.preprocess_tensor(_place(bad_np, layout)[0], TH, TW, antialias, row_begin=row_begin)
    hit = np.zeros(clean.shape, dtype=bool)
    hit[c] = (T.My[:, iy] != 0)[:, None] & (T.Mx[:, ix] != 0)[None, :]
    assert hit.any() and np.array_equal(torch.isnan(bad).cpu().numpy(), hit)
    assert torch.equal(bad[~torch.from_numpy(hit).to(DEV)], clean[~torch.from_numpy(hit).to(DEV)])
    # and back: one NaN in the upstream gradient reaches exactly the inputs that output reads
    g_np = ref.image(clean.shape, seed=22)
    oy, ox = 5, 17
    g_np[c, oy, ox] = np.nan
    x, leaf, back = _place(x_np, layout, grad=True)
    rz.preprocess_tensor(x, TH, TW, antialias, row_begin=row_begin).backward(torch.from_numpy(g_np).to(DEV))
    hit_in = np.zeros(shape, dtype=bool)
    hit_in[c, top:top + T.My.shape[1], left:left + T.Mx.shape[1]] = (T.My[oy] != 0)[:, None] & (T.Mx[ox] != 0)[None, :]
    assert hit_in.any() and np.array_equal(torch.isnan(back(leaf.grad)).cpu().numpy(), hit_in)


def test_the_reference_shape_through_novel_view_inputs(rz):
    """1066x1600 -> rows 166..1066 -> 576x1024, rows 230: (the training shape: many workgroups, the real tables)."""
    shape = (3, 1066, 1600)
    x_np = ref.image(shape, seed=31)
    m_np = ref.mask(shape, 0.7, seed=32)
    x, leaf, back = _place(x_np, "raster", grad=True)
    image_loss, mask_loss, upper = rz.novel_view_inputs(x, torch.from_numpy(m_np).to(DEV), 576, 1024)
    assert upper == 230 and image_loss.shape == (3, 346, 1024) and mask_loss.shape == (1, 346, 1024)
    T = ref.Truth(rz, x_np, (576, 1024), True, upper)
    assert T.box == (166, 1066, 0, 1600)
    want, bar, _A = T.forward()
    err = np.abs(_f64(image_loss) - want)
    print(f"1066x1600: forward reached {_ratio(err, bar):.3f} of the bar")
    assert (err <= bar).all()
    want_m, v, residue_only = T.mask(m_np)
    assert not residue_only.any() and not ((v > 0) & (v < 2.0 ** -20)).any()
    assert np.array_equal(mask_loss.cpu().numpy(), want_m)
    g = ref.image(want.shape, seed=33)
    image_loss.backward(torch.from_numpy(g).to(DEV))
    want_g, bar_g, reached = T.backward(g)
    got = _f64(back(leaf.grad))
    err = np.abs(got - want_g)
    print(f"1066x1600: backward reached {_ratio(err, bar_g):.3f} of the bar")
    assert (err <= bar_g).all() and (got[~reached] == 0).all() and not np.signbit(got[~reached]).any()
    first = np.flatnonzero(reached.any(axis=(0, 2)))[0]
    assert 166 < first < 1066 and not reached[:, :first].any()      # rows that only outputs above `upper` read: no gradient


def test_output_feeds_the_losses_unchanged(rz):
    from street_crafter_amd import losses, lpips
    shape = (3, 29, 50)
    x_np, m_np = ref.image(shape, seed=41) * 0.5 + 0.5, ref.mask(shape, 0.7, seed=42)
    gt = torch.from_numpy(ref.image((3, TH, TW), seed=43) * 0.5 + 0.5).to(DEV)
    x, leaf, back = _place(x_np.astype(np.float32), "raster", grad=True)
    image_loss, mask_loss, upper = rz.novel_view_inputs(x, torch.from_numpy(m_np).to(DEV), TH, TW)
    gt_loss = gt[:, upper:, :]
    l1, ssim = losses.l1_and_ssim(image_loss, gt_loss, mask_loss)
    z = lpips.prepare(image_loss, mask_loss)
    assert z.shape == (1, 3, TH - upper, TW)
    loss = 0.8 * l1 + 0.2 * (1.0 - ssim) + 1e-3 * z.square().mean()
    assert torch.isfinite(loss)
    loss.backward()
    grad = _f64(back(leaf.grad))
    _w, _b, reached = ref.Truth(rz, x_np, ref.TARGET, True, upper).backward(np.ones((3, TH - upper, TW), np.float32))
    assert np.isfinite(grad).all() and (grad[~reached] == 0).all() and (grad[reached] != 0).any()
    rows = np.flatnonzero((grad != 0).any(axis=(0, 2)))
    assert rows.min() > 7                                           # inside the crop, below what only the upper rows read


def test_arguments_are_checked(rz):
    x = torch.zeros(3, 29, 50, device=DEV)
    m = torch.zeros(1, 29, 50, dtype=torch.bool, device=DEV)
    for bad in (x.double(), x.half(), x.to(torch.uint8), x[:, :0], x[0, 0]):
        with pytest.raises(ValueError):
            rz.resize(bad, (18, 32))
    for size in (18, (18,), (18, 32, 3), (0, 32), (18, 32.0), (1 << 17, 32)):
        with pytest.raises(ValueError):
            rz.resize(x, size)
    for kw in (dict(row_begin=18), dict(row_begin=-1), dict(row_begin=1.5)):
        with pytest.raises(ValueError):
            rz.preprocess_tensor(x, 18, 32, **kw)
    with pytest.raises(ValueError):
        rz.preprocess_tensor(x[0], 18, 32)                         # [H,W]: the reference function takes images
    with pytest.raises(ValueError):
        rz.preprocess_tensor(x[None, None], 18, 32)
    with pytest.raises(ValueError, match="bool mask"):
        rz.preprocess_tensor(m, 18, 32, scale=2.0)
    for bad_mask in (m[:, :28], m.float(), m[0], torch.zeros(1, 29, 50, dtype=torch.bool)):
        with pytest.raises((ValueError, RuntimeError)):
            rz.novel_view_inputs(x, bad_mask, 18, 32)
    with pytest.raises(ValueError):
        rz.novel_view_inputs(x[None], m, 18, 32)
    with pytest.raises(ValueError):
        rz.novel_view_inputs(x, m, 18, 32, upper_frac=1.0)
    assert rz.resize(x, [18, 32]).shape == (3, 18, 32)             # a list is a size too
