"""The tile walk of the rasterizers (csrc/raster_walk.h: ScStage, sc_cull_compact, sc_walk_batch, sc_blend_step) on the
hand-built frames of oracle/raster_edge_frames.py: one case per tile -- the 1/255 contour around one pixel, lists of
0 .. 193 entries, batches of which the cull keeps none, one, two, 63 or all, saturation at chosen positions, degenerate
and non-finite records.  Every consumer of the walk is held bit for bit against the reference-shaped kernel
(`raster_fwd` 0), which is held against float64 on EVERY pixel: no decision of these frames is within 1e-4 of its
threshold, so no pixel is left out."""
import numpy as np
import pytest
import torch

from oracle import raster_edge_frames as EF

pytestmark = pytest.mark.gpu
DEV = "cuda"
FINITE = ["finite", "finite129"]
FRAMES = FINITE + ["nonfinite"]


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype).to(DEV)


def _args(p, D):
    return (_t(p["means2d"]), _t(p["conics"]), _t(p["colors"][..., :D]).contiguous(), _t(p["opacities"]),
            _t(p["isect_offsets"], torch.int32), _t(p["flatten_ids"], torch.int32))


def _render(p, D, variant, bg=None, masks=None, order=None):
    """-> colours, alphas, last_ids of sc_rasterize_fwd under `raster_fwd` = variant; `order`: a dispatch list"""
    from street_crafter_amd import _lib
    m2, cn, col, op, offs, fids = _args(p, D)
    work = None
    if order is not None:
        assert order.size == _lib.load().sc_tile_order_len(EF.TW * EF.TH)
        order = _t(order, torch.int32)
        work = torch.zeros(_lib.load().sc_view_slots() * EF.TW * EF.TH, dtype=torch.int32, device=DEV)
    prev = _lib.set_option("raster_fwd", variant)
    try:
        rc, c, a, last = _lib.binding().rasterize_fwd(m2, cn, col, op, bg, masks, EF.W, EF.H, EF.TILE, offs, fids, True,
                                                       order, work, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("raster_fwd", prev)
    _lib.check(rc, "sc_rasterize_fwd")
    return c, a, last


@pytest.fixture(scope="module")
def base():
    """{(frame, D): variant 0's colours, alphas, last_ids}"""
    from street_crafter_amd import _lib
    _lib.load()
    return {(k, D): _render(EF.frame(k), D, 0) for k in FRAMES for D in (3, 4)}


@pytest.mark.parametrize("D", [4, 3])
@pytest.mark.parametrize("kind", FINITE)
def test_reference_shaped_kernel_against_float64_on_every_pixel(base, kind, D):
    p = EF.frame(kind)
    ref = EF.reference(p, D)
    assert ref["margin"].min() >= EF.MARGIN and (ref["margin"] < 2e-5).mean() == 0.0      # the unstable share is exactly 0
    c, a, last = (x.cpu().numpy() for x in base[(kind, D)])
    err_c = np.abs(c[0, ..., :3] - ref["colors"][..., :3]).max()
    err_a = np.abs(a[0, ..., 0] - ref["alphas"]).max()
    print(kind, D, "largest |hip - float64|: colours", err_c, "alpha", err_a)
    assert err_c <= 1e-4 and err_a <= 1e-4
    if D == 4:
        np.testing.assert_allclose(c[0, ..., 3], ref["colors"][..., 3], rtol=1e-5, atol=1e-3)
    np.testing.assert_array_equal(last[0], ref["last"])


@pytest.mark.parametrize("D", [4, 3])
@pytest.mark.parametrize("kind", FRAMES)
def test_wave_kernel_is_bit_identical_to_the_reference_shaped_one(base, kind, D):
    p = EF.frame(kind)
    c0, a0, l0 = base[(kind, D)]
    assert torch.isfinite(c0).all() and torch.isfinite(a0).all()
    c3, a3, l3 = _render(p, D, 3)
    assert torch.equal(c3, c0) and torch.equal(a3, a0) and torch.equal(l3, l0)
    # backgrounds and tile masks (every third tile masked)
    g = torch.Generator().manual_seed(3)
    bg = torch.rand(1, D, generator=g).to(DEV)
    masks = ((torch.arange(EF.TW * EF.TH) % 3) != 1).reshape(1, EF.TH, EF.TW).to(torch.uint8).to(DEV)
    for b, m in ((bg, None), (None, masks), (bg, masks)):
        want, got = _render(p, D, 0, b, m), _render(p, D, 3, b, m)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), (b is not None, m is not None)
    lit = masks[0].bool().repeat_interleave(16, 0).repeat_interleave(16, 1)[: EF.H, : EF.W]
    cm, am, _ = _render(p, D, 3, None, masks)
    assert torch.equal(cm[0][lit], c0[0][lit]) and not am[0][~lit].any()


@pytest.mark.parametrize("D", [4, 3])
@pytest.mark.parametrize("kind", FRAMES)
def test_half_tile_dispatch_items_are_bit_identical(base, kind, D):
    """Every 16-row tile walked as two half-tile waves (NSUB 2) through hand-written dispatch lists, 15 tiles a list."""
    p = EF.frame(kind)
    c0, a0, l0 = base[(kind, D)]
    sets = EF.split_sets()
    assert sorted(t for s in sets for t in s) == [t for t in range(EF.TW * (EF.TH - 1))]
    for split in sets:
        c, a, last = _render(p, D, 3, order=EF.dispatch_list(split))
        assert torch.equal(c, c0) and torch.equal(a, a0) and torch.equal(last, l0), split


@pytest.mark.parametrize("kind", FRAMES)
def test_packed_record_entry_is_bit_identical(base, kind):
    from street_crafter_amd import _lib
    p = EF.frame(kind)
    m2, cn, col, op, offs, fids = _args(p, 4)
    rec = torch.zeros(1, m2.shape[1], 12, device=DEV)
    rec[..., 0:2], rec[..., 2:5], rec[..., 5], rec[..., 6:10] = m2, cn, op, col
    rc, c, a = _lib.binding().rasterize_fwd_packed(rec.contiguous(), None, EF.W, EF.H, offs, fids, None, None, 0,
                                                   torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "sc_rasterize_fwd_packed")
    c0, a0, _ = base[(kind, 4)]
    assert torch.equal(c, c0) and torch.equal(a, a0)


@pytest.mark.parametrize("D", [4, 3])
@pytest.mark.parametrize("kind", FRAMES)
def test_grouped_and_layered_forwards_are_bit_identical(base, kind, D):
    from street_crafter_amd.groups import rasterize_to_pixels_grouped
    from street_crafter_amd.layers import rasterize_to_pixels_layered
    p = EF.frame(kind)
    m2, cn, col, op, offs, fids = _args(p, D)
    c0, a0, _ = base[(kind, D)]
    N = m2.shape[1]
    with torch.no_grad():
        # one group that spans all records: the composite and the group's image are both the plain render
        c, a, gc, ga = rasterize_to_pixels_grouped(m2, cn, col, op, EF.W, EF.H, EF.TILE, offs, fids,
                                                   torch.zeros(N, dtype=torch.uint8, device=DEV), n_groups=1)
        assert torch.equal(c, c0) and torch.equal(a, a0) and torch.equal(gc[0], c0) and torch.equal(ga[0], a0)
        # no record in a group: the composite is the plain render, the group images are empty
        c, a, gc, ga = rasterize_to_pixels_grouped(m2, cn, col, op, EF.W, EF.H, EF.TILE, offs, fids,
                                                   torch.full((N,), 255, dtype=torch.uint8, device=DEV), n_groups=2)
        assert torch.equal(c, c0) and torch.equal(a, a0) and not gc.any() and not ga.any()
        # everything in the front layer / in the back layer
        fc, fa, bc, ba = rasterize_to_pixels_layered(m2, cn, col, op, EF.W, EF.H, EF.TILE, offs, fids, N)
        assert torch.equal(fc, c0) and torch.equal(fa, a0) and not bc.any() and not ba.any()
        fc, fa, bc, ba = rasterize_to_pixels_layered(m2, cn, col, op, EF.W, EF.H, EF.TILE, offs, fids, 0)
        assert torch.equal(bc, c0[..., :3]) and torch.equal(ba, a0) and not fc.any() and not fa.any()


@pytest.mark.parametrize("D", [4, 3])
def test_nonfinite_records_blend_by_the_literal_formula_and_touch_no_other_tile(base, D):
    """Pinned: a NaN sigma or opacity fails both `sigma < 0` and `alpha < 1/255` and the record blends at 0.999 (upstream
    gsplat's kernel does the same: min(0.999f, NaN) is 0.999f); -inf opacity, +-inf conic entries and an infinite x
    are skipped, an infinite y is 0 * inf = NaN in the kernels' order of evaluation and blends.  A tile that does not list such a record is bit-identical to the frame without them."""
    p = EF.frame("nonfinite")
    c0, a0, l0 = base[("nonfinite", D)]
    ref = EF.reference(p, D)
    c, a = c0.cpu().numpy()[0], a0.cpu().numpy()[0, ..., 0]
    assert np.abs(c[..., :3] - ref["colors"][..., :3]).max() <= 1e-4 and np.abs(a - ref["alphas"]).max() <= 1e-4
    np.testing.assert_array_equal(l0.cpu().numpy()[0], ref["last"])
    bad = [e["rec"] for e in p["expect"].values() if "rec" in e]
    clean = EF.without_records(p, bad)
    cc, ca, _ = _render(clean, D, 0)
    blends = {"a-nan", "b-nan", "c-nan", "op-nan", "op-inf", "mx-nan", "my-nan", "my-inf"}      # (my-inf: 0 * inf, b = 0)
    n_same = 0
    for (tx, ty), name in p["names"].items():
        sl = (0, slice(ty * 16, min(ty * 16 + 16, EF.H)), slice(tx * 16, min(tx * 16 + 16, EF.W)))
        same = torch.equal(c0[sl], cc[sl]) and torch.equal(a0[sl], ca[sl])
        kind, _, where = name[len("nonfinite-"):].rpartition("-") if name != "plain" else ("", "", "")
        # unchanged, bit for bit: a tile that does not list such a record, a tile whose record is skipped, and a tile
        # whose pixels had all finished before the record came (an alpha of 0.999 there "terminates again")
        if name == "plain" or kind not in blends or where == "finished":
            assert same, (name, tx, ty)
            n_same += 1
        else:
            assert not same, (name, tx, ty)
    assert n_same >= 15 + 3 * (len(EF.NONFINITE) - len(blends)) + len(blends)
    # and the pinned outcomes, tile by tile: which records blend (alpha 0.999 everywhere) and which are skipped
    for (tx, ty), name in p["names"].items():
        if not name.endswith("-front"):
            continue
        sl = (slice(ty * 16, ty * 16 + 16), slice(tx * 16, tx * 16 + 16))
        kind = name[len("nonfinite-"):-len("-front")]
        if kind in blends:
            assert (a[sl] > 0.999).all(), name          # 0.999, then two faint records
        else:
            assert (a[sl] < 0.03).all(), name           # the two faint records only
