"""The hand-built edge frames (oracle/raster_edge_frames.py) judged without a GPU: every decision of the finite frames
is at least 1e-4 from its threshold, the cases are what their names say, and the frame-wide float64 walk agrees with
blend_f64.walk pixel by pixel -- on the non-finite frame too, where both follow the literal comparison."""
import numpy as np
import pytest

from oracle import blend_f64 as B
from oracle import raster_edge_frames as EF


@pytest.mark.parametrize("kind", ["finite", "finite129"])
def test_no_decision_of_the_finite_frames_is_near_its_threshold(kind):
    p = EF.frame(kind)
    ref = EF.reference(p)
    assert ref["margin"].min() >= EF.MARGIN
    assert (ref["margin"] < 2e-5).mean() == 0.0
    # ... and by the project's own definition (the numpy oracle's windows plus the clamp's, as the backward tests use it)
    from oracle import raster_bwd_f64 as RB
    un = RB.unstable_bwd(p["means2d"], p["conics"], p["colors"], p["opacities"], EF.W, EF.H, EF.TILE, p["isect_offsets"],
                         p["flatten_ids"])
    assert un.mean() == 0.0
    assert np.isfinite(p["means2d"]).all() and np.isfinite(p["conics"]).all() and np.isfinite(p["opacities"]).all()
    assert p["isect_offsets"].shape == (1, EF.TH, EF.TW) and (EF.W, EF.H) == (136, 100)
    assert np.array_equal(np.sort(p["flatten_ids"]), np.arange(p["opacities"].shape[1]))       # every record in one list


def test_cases_are_what_their_names_say():
    p = EF.frame("finite")
    ref = EF.reference(p)
    offs = p["isect_offsets"][0]
    lens = {n: len(p["lists"][t]) for t, n in p["names"].items()}
    for n in (0, 1, 2, 63, 64, 65, 127, 129, 192, 193):
        assert lens[f"len-{n}"] == n
    assert lens["len-128-mid"] == 128 and lens["last-tile-128"] == 128
    assert int(offs[-1, -1]) + 128 == p["flatten_ids"].size               # the last tile's list ends at n_isects
    assert len(EF.frame("finite129")["lists"][(EF.TW - 1, EF.TH - 1)]) == 129
    for t, e in p["expect"].items():
        name = p["names"][t]
        sl = (slice(t[1] * 16, min(t[1] * 16 + 16, EF.H)), slice(t[0] * 16, min(t[0] * 16 + 16, EF.W)))
        s = int(offs[t[1], t[0]])
        if "last" in e:           # every pixel of the tile stops behind the same record
            assert np.unique(ref["last"][sl]).tolist() == [s + e["last"]], name
            assert (ref["alphas"][sl] > 0.998).all(), name
        if e.get("never_saturates") and lens[name]:
            assert (ref["last"][sl] == s + lens[name] - 1).all() and (ref["alphas"][sl] < 0.95).all(), name
        if "rec" in e and p["lists"][t][0] == e["rec"]:
            hit = ref["n_blended"][sl] == 2          # the contour record and the faint cover behind it
            ys, xs = np.nonzero(hit)
            if "only" in e:
                assert sorted(zip(xs.tolist(), ys.tolist())) == sorted(e["only"]), name
            if "rows" in e:
                assert hit.any() and ys.min() >= e["rows"][0] and ys.max() < e["rows"][1], name
            if "column" in e:
                assert hit[:, e["column"]].all() and not np.delete(hit, e["column"], axis=1).any(), name
    # kept / culled patterns: the culled records are the ones 60 pixels away, and they blend nowhere
    t = next(t for t, n in p["names"].items() if n == "keep-none")
    assert (ref["n_blended"][t[1] * 16:t[1] * 16 + 16, t[0] * 16:t[0] * 16 + 16] == 3).all()
    for a, b, c in EF.indefinite_by_rounding():
        assert a * c < b * b and a > 0 and c > 0
        f = np.float32
        assert a * c - float(f(b * b)) > 0 or float(f(a * c)) - b * b > 0      # one fused form of the test passes


@pytest.mark.parametrize("kind", ["finite", "finite129", "nonfinite"])
def test_frame_walk_agrees_with_blend_f64_pixel_by_pixel(kind):
    p = EF.frame(kind)
    ref = EF.reference(p)
    rng = np.random.default_rng(5)
    m2, cn, co, op = p["means2d"][0], p["conics"][0], p["colors"][0], p["opacities"][0]
    pix = [(int(rng.integers(0, EF.W)), int(rng.integers(0, EF.H))) for _ in range(150)]
    pix += [(t[0] * 16 + x, t[1] * 16 + y) for t in p["names"] for x, y in ((0, 0), (7, 3))]
    for x, y in pix:
        s, g = B.tile_list(x, y, EF.TILE, EF.TW, p["isect_offsets"], p["flatten_ids"], tile_height=EF.TH)
        w = B.walk(x + 0.5, y + 0.5, g, m2, cn, co, op)
        assert not w.near, (x, y)
        np.testing.assert_allclose(w.color, ref["colors"][y, x], rtol=1e-12, atol=1e-14)
        assert abs(w.alpha - ref["alphas"][y, x]) <= 1e-14
        assert (s + w.last if w.last >= 0 else 0) == ref["last"][y, x]
