"""The exact tile cull and the lane-to-pixel map of the wave-per-tile rasterizers on the device, through the probe
sc_test_tile_cull (one wave per record, the helpers the tile walk compiles), against the float64 reference of
oracle/cull_cases.py: about 100 k records per family, most of them with the 1 / 255 contour through one to four pixels of
a whole, partial or half tile."""
import numpy as np
import pytest
import torch

from oracle import cull_cases as CC

pytestmark = pytest.mark.gpu
FAMILIES = sorted(CC.FAMILIES)


def probe(rec, geo):
    """-> verdict i32[n], valid u32[n, 8] of the device probe"""
    from street_crafter_amd import _lib
    lib = _lib.load()
    n = rec.shape[0]
    r = torch.from_numpy(np.array(rec, np.float32)).cuda()
    g = torch.from_numpy(np.array(geo, np.int32)).cuda()
    verdict = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    valid = torch.full((n, 8), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.sc_test_tile_cull(r.data_ptr(), g.data_ptr(), n, verdict.data_ptr(), valid.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "sc_test_tile_cull")
    return verdict.cpu().numpy(), valid.cpu().numpy().view(np.uint32)


_probed = {}


def probed(name):
    if name not in _probed:
        fam = CC.family(name)
        _probed[name] = probe(fam["rec"], fam["geo"])
    return _probed[name]


@pytest.mark.parametrize("name", FAMILIES)
def test_cull_is_sound(name):
    """A record the cull drops blends into no pixel: the device's own valid mask is empty, and float64 has no pixel that
    is certainly valid."""
    verdict, valid = probed(name)
    ref = CC.reference(name)
    assert set(np.unique(verdict)) <= {0, 1}
    miss = verdict == 1
    bad_dev = miss & valid.any(axis=1)
    bad_ref = miss & (ref["n_cv"] > 0)
    print(name, "dropped", round(float(miss.mean()), 4), "dropped with a device-valid pixel", int(bad_dev.sum()),
          "dropped with a float64-valid pixel", int(bad_ref.sum()))
    assert not bad_dev.any(), np.nonzero(bad_dev)[0][:10]
    assert not bad_ref.any(), np.nonzero(bad_ref)[0][:10]


@pytest.mark.parametrize("name", FAMILIES)
def test_cull_is_complete_up_to_twice_its_margin(name):
    """A positive definite record whose continuous float64 minimum over the rectangle exceeds ln(255 op) by more than
    twice the documented margin (1e-3 + 1e-3 |L| + 2e-6 S) is dropped.  Twice: the device's evaluation of the minimum is
    within ~1e-6 S of the true one and its threshold within rounding of the formula, i.e. inside one more margin.
    Slack (reported, not asserted): the share of records kept although no pixel of theirs is valid on the device."""
    verdict, valid = probed(name)
    ref = CC.reference(name)
    must = ref["must_drop"]
    kept_empty = (verdict == 0) & ~valid.any(axis=1)
    print(name, "must-drop share", round(float(must.mean()), 4), "of them kept", int((must & (verdict != 1)).sum()),
          "| slack: kept with an empty valid mask", round(float(kept_empty.mean()), 4), "of all records,",
          round(float(kept_empty.sum() / max((verdict == 0).sum(), 1)), 4), "of the kept ones")
    assert must.mean() >= 0.30
    assert not (must & (verdict != 1)).any(), np.nonzero(must & (verdict != 1))[0][:10]


@pytest.mark.parametrize("name", FAMILIES)
def test_valid_mask_matches_the_float64_lattice(name):
    """Every certainly-valid pixel is in the device's mask, no certainly-invalid pixel is (near pixels are free), and no
    bit outside the image is set -- there the walk evaluates x = +inf and relies on alpha = 0."""
    _, valid = probed(name)
    ref = CC.reference(name)
    missing = ref["cv"] & ~valid
    extra = ref["ci"] & valid
    outside = valid & ~ref["inside"]
    print(name, "records with a certainly-valid pixel missing", int(missing.any(axis=1).sum()),
          "with a certainly-invalid pixel set", int(extra.any(axis=1).sum()), "with a bit outside the image",
          int(outside.any(axis=1).sum()))
    assert not outside.any(), np.nonzero(outside.any(axis=1))[0][:10]
    assert not missing.any(), np.nonzero(missing.any(axis=1))[0][:10]
    assert not extra.any(), np.nonzero(extra.any(axis=1))[0][:10]


def test_mask_bits_follow_the_lane_to_pixel_map():
    """One sharp record (conic 50 I, opacity 1) on every pixel that a lane owns, for whole tiles and both halves: the
    mask is exactly that pixel's bit, 16 * row + column of the rectangle, and the record is kept."""
    rec, geo, want = [], [], []
    txi, tyi = 3, 2
    for nsub, ppl in ((1, 4), (2, 2)):
        for sub in range(nsub):
            for lane in range(64):
                for k in range(ppl):
                    lpr = 16 // ppl
                    x = txi * 16 + ppl * (lane % lpr) + k
                    y = tyi * 16 + sub * (16 // nsub) + lane // lpr
                    rec.append((50.0, 0.0, 50.0, 1.0, x + 0.5, y + 0.5))
                    geo.append((txi, tyi, sub, nsub, 80, 64))
                    want.append(CC.lane_bit(nsub, lane, k))
    verdict, valid = probe(np.array(rec, np.float32), np.array(geo, np.int32))
    want = np.array(want)
    expect = np.zeros((len(want), 8), np.uint32)
    expect[np.arange(len(want)), want >> 5] = np.uint32(1) << (want & 31).astype(np.uint32)
    assert (verdict == 0).all()
    assert np.array_equal(valid, expect)


def test_probe_rejects_rectangles_outside_the_image():
    rec = np.tile(np.array([[1.0, 0.0, 1.0, 1.0, 8.0, 8.0]], np.float32), (6, 1))
    geo = np.array([[0, 0, 0, 1, 16, 16], [1, 0, 0, 1, 16, 16], [0, 1, 0, 1, 16, 16], [0, 0, 1, 2, 16, 8],
                    [0, 0, 0, 3, 16, 16], [0, 0, 2, 2, 16, 16]], np.int32)
    verdict, valid = probe(rec, geo)
    assert verdict.tolist() == [0, -1, -1, -1, -1, -1]
    assert valid[0].any() and not valid[1:].any()
