"""The point render's blend kernel alone (`sc_point_rasterize_fwd`, csrc/point_raster.hip) on hand-built records and
tile lists (tests/point_raster_ref.walk_cases): no projection, no sort, the kernel walks exactly the list the test wrote.

Every case runs with 1 and with 4 waves per tile ("point_raster_waves"), into both output layouts (interleaved [H,W,4];
planes [3,H,W] + [H,W]), with and without a depth plane and with and without a background.  Every output buffer has 64
guard floats on either side, pre-filled with a sentinel like the buffer itself.

Verdict on every pixel of every case, none left out (the frames are exact: point_raster_ref.assert_exact):
  * rgb, alpha and depth equal point_raster_ref.blend_f32_replay bit for bit;
  * |hip - f64| <= 2^-24 (3h + 4) S for rgb and depth and <= 2^-24 (2h + 2) for alpha, h the pixel's hit count and S the
    sum of the magnitudes of its blended terms, background included.  T_i carries 2i roundings, w = T a and w c one
    each, the h-term sum at most h - 1 more, the background term 2; second-order terms sit in the + 4
    (point_raster_ref's docstring has the full derivation; tests/test_point_raster_ref_cpu.py asserts the same bars for
    the replay itself);
  * with one alpha a throughout the list, 1 - alpha == (1 - a)^hits as float32 products;
  * every pixel is written (no sentinel is left), the guards keep the sentinel;
  * the 1-wave and the 4-wave results are identical.
The largest |hip - f64| / bar of each case is printed.
"""
import numpy as np
import pytest
import torch

import point_raster_ref as PR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -12345.0
BG = np.array([0.25, 0.5, 0.75], np.float32)
CASES = {c["name"]: c for c in PR.walk_cases()}


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import _lib
    return _lib.load()


def _guarded(n):
    return torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")


def _ptr(t):
    return t.data_ptr() + 4 * GUARD


def _inner(t):
    g = t.cpu().numpy()
    assert (g[:GUARD] == SENTINEL).all() and (g[-GUARD:] == SENTINEL).all(), "a guard float was written"
    return g[GUARD:-GUARD]


def _launch(lib, case, dev, planar, want_depth, bg):
    from street_crafter_amd import _lib, isect
    W, H = case["W"], case["H"]
    tw, th = PR.tiles_of(W, H)
    depth = _guarded(H * W) if want_depth else None
    if planar:
        img, alpha = _guarded(3 * H * W), _guarded(H * W)
        p_img, p_alpha, strides = _ptr(img), _ptr(alpha), (1, H * W, 1)
    else:
        img, alpha = _guarded(4 * H * W), None
        p_img, p_alpha, strides = _ptr(img), _ptr(img) + 12, (4, 1, 4)
    _lib.check(lib.sc_point_rasterize_fwd(dev["records"].data_ptr(), dev["N"], W, H, tw, th, dev["offsets"].data_ptr(),
                                          dev["ids"].data_ptr(), case["n_isects"], case["max_hit"],
                                          dev["bg"].data_ptr() if bg else None, p_img, strides[0], strides[1], p_alpha,
                                          strides[2], _ptr(depth) if want_depth else None,
                                          isect._stream(dev["records"])), "sc_point_rasterize_fwd")
    torch.cuda.synchronize()
    if planar:
        rgb, a = _inner(img).reshape(3, H, W).transpose(1, 2, 0), _inner(alpha).reshape(H, W)
    else:
        out = _inner(img).reshape(H, W, 4)
        rgb, a = out[..., :3], out[..., 3]
    return np.ascontiguousarray(rgb), np.ascontiguousarray(a), _inner(depth).reshape(H, W) if want_depth else None


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_blend_kernel_walks_the_list_it_was_given(lib, name):
    from street_crafter_amd import _lib
    case = CASES[name]
    PR.assert_exact(case)
    args = (case["records"], case["offsets"], case["flatten_ids"], case["n_isects"], case["W"], case["H"],
            case["max_hit"])
    ref = {bg: (PR.blend_f64(*args, BG if bg else None), PR.blend_f32_replay(*args, BG if bg else None))
           for bg in (False, True)}
    ids = case["flatten_ids"] if case["n_isects"] else np.zeros(1, np.int32)     # (an empty tensor has no address)
    dev = {"records": torch.from_numpy(case["records"]).cuda(), "N": case["records"].shape[0],
           "offsets": torch.from_numpy(case["offsets"]).cuda(), "ids": torch.from_numpy(ids).cuda(),
           "bg": torch.from_numpy(BG).cuda()}
    listed = case["records"][np.unique(case["flatten_ids"]), 7]
    one_alpha = np.float32(listed[0]) if listed.size and (listed == listed[0]).all() else None
    worst, first = 0.0, {}
    for waves in (1, 4):
        prev = _lib.set_option("point_raster_waves", waves)
        try:
            for planar in (False, True):
                for want_depth in (False, True):
                    for bg in (False, True):
                        what = f"{name} waves {waves} planar {planar} depth {want_depth} bg {bg}"
                        rgb, alpha, depth = _launch(lib, case, dev, planar, want_depth, bg)
                        f64, f32 = ref[bg]
                        assert np.array_equal(_bits(rgb), _bits(f32["rgb"])), what
                        assert np.array_equal(_bits(alpha), _bits(f32["alpha"])), what
                        if want_depth:
                            assert np.array_equal(_bits(depth), _bits(f32["depth"])), what
                        worst = max(worst, PR.judge(rgb, alpha, depth, f64, what))
                        if one_alpha is not None:
                            T = np.ones_like(alpha)
                            for h in range(1, int(f64["hits"].max()) + 1):
                                T = np.where(f64["hits"] >= h, T * (np.float32(1) - one_alpha), T)
                            assert np.array_equal(_bits(np.float32(1) - T), _bits(alpha)), what
                        # 1 wave == 4 waves == either layout
                        key = (want_depth, bg)
                        if key not in first:
                            first[key] = (rgb, alpha, depth)
                        else:
                            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(first[key], (rgb, alpha, depth))
                                       if x is not None), what
        finally:
            _lib.set_option("point_raster_waves", prev)
    print(f"[point_raster_walk] {name}: worst |hip - f64| / bar = {worst:.3f}")
