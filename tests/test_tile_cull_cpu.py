"""The tile-cull records and their float64 reference, judged without a GPU (oracle/cull_cases.py): the conditions the
generator has to meet for tests/test_tile_cull_gpu.py to mean something, the reference's own consistency, and a numpy
float32 emulation of splat_misses_rect on the same records -- so that a failure on the device can be told from a mistake
in the generator or the reference."""
import numpy as np
import pytest

from oracle import cull_cases as CC

FAMILIES = sorted(CC.FAMILIES)


@pytest.mark.parametrize("name", FAMILIES)
def test_records_meet_the_generator_conditions(name):
    fam, ref = CC.family(name), CC.reference(name)
    rec, geo, kind = fam["rec"], fam["geo"], fam["kind"]
    n = rec.shape[0]
    assert n == CC.N_RECORDS and np.isfinite(rec).all()
    assert (rec[:, 3] > 0).all() and (rec[:, 3] <= 1).all()
    x0, y0, ncols, nrows = CC.rectangle(geo)
    d = np.hypot(rec[:, 4] - (x0 + 0.5 * (ncols - 1)), rec[:, 5] - (y0 + 0.5 * (nrows - 1)))
    assert d.min() >= 0.25 and d.max() <= 3100.0 and np.quantile(d, 0.1) < 10.0 and np.quantile(d, 0.9) > 300.0
    none = (ref["n_cv"] == 0) & (ref["n_near"] == 0)
    few = (ref["n_cv"] >= 1) & (ref["n_cv"] <= 4)
    shares = dict(none=none.mean(), few=few.mean(), few_big_S=(few & (ref["S_pix"] > 1e3)).mean(),
                  partial=(kind == CC.KIND_PARTIAL).mean(), half=(kind == CC.KIND_HALF).mean(),
                  must_drop=ref["must_drop"].mean(), many=(ref["n_cv"] > 4).mean())
    print(name, {k: round(float(v), 4) for k, v in shares.items()})
    assert shares["none"] >= 0.20
    assert shares["few"] >= 0.15
    assert shares["few_big_S"] >= 0.02
    assert shares["partial"] >= 0.25 and shares["half"] >= 0.25
    assert shares["must_drop"] >= 0.30
    assert shares["many"] >= 0.02                          # the freely drawn opacities: records with many valid pixels
    # partial tiles of every size 1..16 in both directions, both halves
    part = kind == CC.KIND_PARTIAL
    assert set(ncols[part]) == set(range(1, 17)) and set(nrows[part]) == set(range(1, 17))
    half = kind == CC.KIND_HALF
    assert set(geo[half, 2]) == {0, 1} and set(nrows[half]) == set(range(1, 9))


@pytest.mark.parametrize("name", FAMILIES)
def test_continuous_minimum_bounds_the_lattice_minimum(name):
    ref = CC.reference(name)
    # (both are float64 evaluations of the same quadratic: they may differ by rounding of its terms)
    assert (ref["cmin"] <= ref["qmin"] + 1e-12 * np.maximum(ref["S_rect"], 1.0)).all()
    rec = np.asarray(CC.family(name)["rec"], np.float64)
    pd = (rec[:, 0] > 0) & (rec[:, 2] > 0) & (rec[:, 0] * rec[:, 2] > rec[:, 1] ** 2)
    assert (ref["cmin"][pd] >= 0).all()
    # a record the cull must drop has no valid and no near pixel
    assert not (ref["must_drop"] & ((ref["n_cv"] > 0) | (ref["n_near"] > 0))).any()


@pytest.mark.parametrize("name", FAMILIES)
def test_reference_is_symmetric_under_mirroring(name):
    fam = CC.family(name)
    sl = slice(0, 20_000)
    rec = np.asarray(fam["rec"][sl], np.float64)
    x0, y0, ncols, nrows = (v[sl] for v in CC.rectangle(fam["geo"]))
    base = CC.classify(rec, x0, y0, ncols, nrows)
    j = np.arange(16)
    for axis in ("x", "y"):
        m = rec.copy()
        m[:, 1] = -m[:, 1]
        if axis == "x":
            m[:, 4] = 2.0 * x0 + (ncols - 1) - m[:, 4]
            idx = np.clip(ncols[:, None] - 1 - j[None, :], 0, 15)[:, None, :].repeat(16, axis=1)
        else:
            m[:, 5] = 2.0 * y0 + (nrows - 1) - m[:, 5]
            idx = np.clip(nrows[:, None] - 1 - j[None, :], 0, 15)[:, :, None].repeat(16, axis=2)
        got = CC.classify(m, x0, y0, ncols, nrows)
        for k in ("cv", "ci"):
            want = np.take_along_axis(base[k].reshape(-1, 16, 16), idx, axis=2 if axis == "x" else 1)
            want &= base["inside"].reshape(-1, 16, 16)
            assert np.array_equal(got[k].reshape(-1, 16, 16), want), (axis, k)
        assert np.array_equal(got["qmin"], base["qmin"])
        assert np.array_equal(CC.continuous_min(m, x0, y0, ncols, nrows), CC.continuous_min(rec, x0, y0, ncols, nrows))


@pytest.mark.parametrize("name", FAMILIES)
def test_float32_emulation_of_the_cull_is_sound_and_complete(name):
    fam, ref = CC.family(name), CC.reference(name)
    miss = CC.emulate_cull_f32(fam["rec"], *CC.rectangle(fam["geo"]))
    assert not (miss & (ref["n_cv"] > 0)).any()
    assert not (ref["must_drop"] & ~miss).any()
    kept_none = ~miss & (ref["n_cv"] == 0) & (ref["n_near"] == 0)
    print(name, "emulated cull: drops", round(float(miss.mean()), 4), "keeps with no valid or near pixel",
          round(float(kept_none.mean()), 4))


def test_lane_bits_cover_the_rectangle_once():
    for nsub, ppl in ((1, 4), (2, 2)):
        bits = sorted(CC.lane_bit(nsub, lane, k) for lane in range(64) for k in range(ppl))
        assert bits == list(range(256 // nsub))
    assert CC.pack_bits(np.eye(256, dtype=bool))[37].tolist() == [0, 1 << 5, 0, 0, 0, 0, 0, 0]
