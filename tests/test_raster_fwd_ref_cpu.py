"""The float64 forward of rasterize_to_pixels with its per-pixel scale (oracle/raster_fwd_f64.py) judged on its own, no GPU:

* independence: on a few hundred sampled pixels of every case (and on every near pixel) the vectorised truth -- colour,
  alpha, last id, AND the scale -- equals the natural path of the sequential per-pixel blend_f64.walk, an independent
  implementation, to float64 rounding, and its near flag is a superset of the walk's; one case also against float64
  oracle/gsplat_torch.py;
* replays and caps: the two float32 replays (the literal order of oracle/gsplat_oracle.py, the pinned order of
  csrc/raster_common.h; numpy, no kernel) are judged on every pixel of every case; the largest ratio is K_REF, the constant
  of the module may be neither smaller than it nor more than twice it; per case, pixels judged against more than one
  outcome stay under raster_bwd_cases.UNSTABLE_CAP, no enumeration is truncated, some pixel blends, and pixels saturate
  where the case says so;
* sensitivity: four seeded faults of the float64 blend, none of which moves a decision by a visible amount, each push
  more than 1 % of ragged-D3's pixels past K.  The pixel-centre fault (1e-4 px) at the same time PASSES the flat
  1e-4 bar on the pixels the float32 oracle calls stable: that assertion is the gap this module closes, kept as the
  record of why it exists.
"""
import numpy as np
import pytest
import torch

from oracle import blend_f64 as B
from oracle import gsplat_oracle as O
from oracle import gsplat_torch as OT
from oracle import raster_bwd_cases as RC
from oracle import raster_fwd_f64 as RF

CASES = RF.case_ids()
SATURATING = ("deep_hard", "clamp")        # scenes whose lists always saturate
NEVER_SATURATING = ("deep_soft",)          # and whose lists never do


@pytest.fixture(scope="module")
def refs():
    """{case: (inputs, reference)}: computed once, left unchanged."""
    return {cid: RF.case_reference(cid) for cid in CASES}


def test_cases_are_the_backward_modules():
    assert set(RC.CASE_IDS) - set(CASES) == {"one_hot-D4"} and len(CASES) == len(RC.CASE_IDS) - 1


@pytest.mark.parametrize("case_id", CASES)
def test_vectorised_truth_equals_the_sequential_walk(refs, case_id):
    p, ref = refs[case_id]
    C, H, W = ref["alphas"].shape
    rng = np.random.default_rng(CASES.index(case_id))
    lit = np.ones((C, H, W), bool)
    if p["masks"] is not None:
        lit = np.repeat(np.repeat(p["masks"], p["tile_size"], 1), p["tile_size"], 2)[:, :H, :W]
    pool = np.argwhere(lit)
    pick = pool[rng.choice(len(pool), 200, replace=False)]
    pick = np.concatenate([pick, np.argwhere(ref["near"])[:100]])
    th, tw = p["isect_offsets"].shape[1:]
    n_near = 0
    for c, y, x in pick:
        s, g = B.tile_list(x, y, p["tile_size"], tw, p["isect_offsets"], p["flatten_ids"], cam=c, tile_height=th)
        bg = None if p["backgrounds"] is None else p["backgrounds"][c]
        w = B.walk(x + 0.5, y + 0.5, g, p["means2d"], p["conics"], p["colors"], p["opacities"], bg, log_form=True)
        np.testing.assert_allclose(ref["colors"][c, y, x], w.color, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ref["alphas"][c, y, x], w.alpha, rtol=1e-12, atol=1e-14)
        assert ref["last_ids"][c, y, x] == (s + w.last if w.last >= 0 else 0)
        np.testing.assert_allclose(ref["E_colors"][c, y, x], w.scale, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(ref["E_alphas"][c, y, x], w.alpha_scale, rtol=1e-9, atol=1e-12)
        assert bool(ref["blended"][c, y, x]) == (w.n_blended > 0)
        if w.near:
            n_near += 1
            assert ref["near"][c, y, x], (c, y, x, w.near)        # the vectorised flag is a superset of the walk's
    print(f"{case_id}: {len(pick)} pixels, {n_near} of them with a near decision in the walk")


def test_truth_equals_float64_gsplat_torch():
    p = RC.make_case("two_cameras-D4bg-masks")
    ref = RF.reference(p, enumerate_near=False)
    t = [torch.from_numpy(p[k]).double() for k in ("means2d", "conics", "colors", "opacities")]
    rc, ra = OT.rasterize_to_pixels(*t, p["width"], p["height"], p["tile_size"], torch.from_numpy(p["isect_offsets"]),
                                    torch.from_numpy(p["flatten_ids"]), backgrounds=torch.from_numpy(p["backgrounds"]).double(),
                                    masks=p["masks"])
    assert np.abs(rc.numpy() - ref["colors"]).max() <= 1e-12
    assert np.abs(ra.numpy()[..., 0] - ref["alphas"]).max() <= 1e-12
    assert ref["blended"].any() and not ref["blended"].all()          # masked tiles and blending tiles are both present


def test_replays_give_k_ref_and_the_caps_hold(refs):
    top, top_at = 0.0, None
    for cid in CASES:
        p, ref = refs[cid]
        share, n_near = RF.near_share(ref), int(ref["near"].sum())
        row = []
        for name, (c, a, last) in RF.replays(p).items():
            j = RF.judge(ref, c, a, last)
            worst = float(j["ratio"].max())
            row.append(f"{name} colours {j['colors']:.3f} alpha {j['alphas']:.3f} ({j['alt']} px by another outcome; "
                       f"max|x - G| {np.abs(np.asarray(c, np.float64) - ref['colors']).max():.1e})")
            assert worst <= RF.K_REF, (cid, name, worst)
            if worst > top:
                top, top_at = worst, f"{cid} / {name}"
        print(f"[replay] {cid}: " + "; ".join(row) + f" | near pixels {n_near}, with several outcomes {100 * share:.4f} %, "
              f"truncated {ref['truncated']}; blends {100 * ref['blended'].mean():.1f} %, saturates {100 * ref['saturated'].mean():.1f} %")
        assert share < RC.UNSTABLE_CAP, (cid, share)
        assert ref["truncated"] == 0, cid
        assert ref["blended"].any() and (ref["E_colors"] > 0).any(), cid
        assert not ref["E_colors"][~ref["blended"]].any() and not ref["E_alphas"][~ref["blended"]].any(), cid
        if p["scene"] in SATURATING:
            assert ref["saturated"].mean() > 0.5, cid
        if p["scene"] in NEVER_SATURATING:
            assert not ref["saturated"].any(), cid
    print(f"[replay] K_ref over {len(CASES)} cases: {top:.3f} ({top_at}); recorded {RF.K_REF}; K = {RF.K}")
    assert RF.K_REF / 2 <= top <= RF.K_REF          # the constant can be neither too small nor padded
    assert RF.K == 4.0 * RF.K_REF


@pytest.mark.parametrize("fault", RF.FAULTS)
def test_seeded_faults_break_the_per_pixel_bar(refs, fault):
    cid = "ragged-D3"
    p, ref = refs[cid]
    x = RF.reference(p, fault=fault)
    j = RF.judge(ref, x["colors"], x["alphas"])
    past = float((j["ratio"] > RF.K).mean())
    stable = ~O.rasterize_to_pixels(*RF.case_args(p)[0], **RF.case_args(p)[1], return_unstable=True)[3]
    flat = max(float(np.abs(x["colors"] - ref["colors"])[stable].max()), float(np.abs(x["alphas"] - ref["alphas"])[stable].max()))
    print(f"[fault] {cid} {fault}: {100 * past:.2f} % of the pixels past K = {RF.K} (worst ratio colours {j['colors']:.1f}, alpha "
          f"{j['alphas']:.1f}); largest change on the oracle's stable pixels {flat:.2e} (flat bar 1e-4); last_ids changed on "
          f"{100 * (x['last_ids'] != ref['last_ids']).mean():.2f} %")
    assert past >= 0.01, (fault, past)
    if fault == "centre":
        assert flat <= 1e-4          # the flat bar on stable pixels lets this fault through: the gap the module closes
        assert (x["last_ids"] == ref["last_ids"]).all()
