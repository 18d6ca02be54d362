"""The two host routes to the C ABI -- the compiled binding layer (`_lib.binding()` by default) and the ctypes adapter
(street_crafter_amd/_ctypes_binding.py, under `set_fast_binding(False)`) -- at the call sites no other route A/B
reaches: the fused `rasterization()` forward (packed records and separate arrays, both depth modes), the planar
rasterizer and the two frame-export entries of `dist.to_uint8_frame`.  Same kernels, same arguments: every tensor must
compare bit for bit.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from street_crafter_amd.scenes import make_camera, make_scene  # noqa: E402

DEV = "cuda"
W, H = 320, 208          # 20 x 13 tiles: several tile rows and columns, empty and full tiles
META_TENSORS = ("radii", "means2d", "depths", "tiles_per_gauss", "flatten_ids", "isect_offsets",
                "isect_ids", "conics", "opacities", "colors")        # (the last four are built on first access)


@pytest.fixture(scope="module")
def frame_inputs():
    from street_crafter_amd import _lib
    _lib.load()
    cams = [make_camera(W, H, 300.0, 300.0).to(DEV), make_camera(W, H, 300.0, 300.0, yaw=0.15, shift=(0.3, 0.0, 0.0)).to(DEV)]
    sc = make_scene(20_000, seed=9, z_range=(1.0, 30.0), scale_range=(0.01, 0.25)).to(DEV)
    viewmats = torch.stack([c.viewmat for c in cams]).contiguous()
    Ks = torch.stack([c.K for c in cams]).contiguous()
    return sc, viewmats, Ks, cams[0].znear, cams[0].zfar


def _one_arm(fast_on, render_mode, packed, frame_inputs):
    """Everything the test compares, computed through one host route: name -> tensor."""
    from street_crafter_amd import _ctypes_binding, _lib, dist
    from street_crafter_amd import rendering as R
    sc, viewmats, Ks, near, far = frame_inputs
    prev_fast = _lib.set_fast_binding(fast_on)
    prev_packed = R.set_packed_records(packed)
    prev_planar = R.set_planar_output(True)
    try:
        assert (_lib.fast() is not None) == fast_on
        assert _lib.binding() is (_lib.fast() if fast_on else _ctypes_binding)
        R.reset_state()
        got = {}
        with torch.no_grad():
            speculative = R._STATE.stats["speculative_ok"]
            for _ in range(2):                      # second frame: predicted sort, warm dispatch list
                colors, alphas, meta = R.rasterization(
                    sc.means, sc.quats, sc.scales, sc.opacities[:, 0], sc.sh, viewmats, Ks, W, H, near_plane=near,
                    far_plane=far, sh_degree=sc.sh_degree, render_mode=render_mode, rasterize_mode="antialiased")
            assert meta["fused"] is True and colors.shape == (2, H, W, 4)
            assert R._STATE.stats["speculative_ok"] == speculative + 1
            got["render_colors"], got["render_alphas"] = colors, alphas
            for k in META_TENSORS:
                got["meta." + k] = meta[k].clone()          # (a clone observes a lazily filled tensor)
            # dist.to_uint8_frame on the renderer's permuted views: the interleaved entry
            fg, sky = colors[0].permute(2, 0, 1)[:3], colors[1].permute(2, 0, 1)[:3]
            assert dist._hwc_view(fg)[2] == 1
            got["u8"] = dist.to_uint8_frame(fg)
            got["u8.sky"] = dist.to_uint8_frame(fg, acc=alphas[0], sky_rgb_chw=sky, rounding="save_image")
            # ... and on the planar rasterizer's output: the strided entry
            pc, pa = R.rasterize_to_pixels(meta["means2d"], meta["conics"], meta["colors"], meta["opacities"], W, H, 16,
                                           meta["isect_offsets"], meta["flatten_ids"])
            assert not pc.is_contiguous()                   # one plane per channel behind the [C,H,W,D] indexing
            fg, sky = pc[0].permute(2, 0, 1)[:3], pc[1].permute(2, 0, 1)[:3]
            assert dist._hwc_view(fg)[2] != 1
            got["planar_colors"], got["planar_alphas"] = pc, pa
            got["u8.planar"] = dist.to_uint8_frame(fg)
            got["u8.planar.sky"] = dist.to_uint8_frame(fg, acc=pa[0], sky_rgb_chw=sky)
        torch.cuda.synchronize()
        return got
    finally:
        R.set_planar_output(prev_planar)
        R.set_packed_records(prev_packed)
        _lib.set_fast_binding(prev_fast)


@pytest.mark.parametrize("packed", [True, False], ids=["records", "arrays"])
@pytest.mark.parametrize("render_mode", ["RGB+D", "RGB+ED"])
def test_fused_forward_and_frame_export_equal_on_both_host_routes(frame_inputs, render_mode, packed):
    compiled = _one_arm(True, render_mode, packed, frame_inputs)
    table = _one_arm(False, render_mode, packed, frame_inputs)
    assert compiled.keys() == table.keys()
    for k in compiled:
        assert compiled[k].dtype == table[k].dtype and compiled[k].shape == table[k].shape, k
        assert torch.equal(compiled[k], table[k]), k
    # (not vacuous: the frame has content, and the composite differs from the plain frame)
    assert compiled["meta.flatten_ids"].numel() > 0 and int(compiled["u8"].max()) > 0
    assert not torch.equal(compiled["u8"], compiled["u8.sky"])
