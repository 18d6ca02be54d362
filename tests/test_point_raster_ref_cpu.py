"""tests/point_raster_ref.py judged on its own, without a GPU: the float64 walk is the contract
(`lidar_condition.render_points`) on constant-occ scenes, the float32 replay stays inside the derived float64 bars on
every case the GPU tests use, every case is exact (assert_exact), the binning lists a superset of the covered tiles, and
every case hits the boundary it is named after, so that a generator change cannot quietly empty it.  Last, a numpy model of a
batched tile walk (batches of 64, cull, compaction, early-out every 8th record) equals the replay on every case, and
the same model with one defect switched on is caught by the case aimed at that defect."""
import numpy as np
import pytest

import point_raster_ref as PR
from street_crafter_amd import lidar_condition as lc

BG = np.array([0.25, 0.5, 0.75], np.float32)
CASES = {c["name"]: c for c in PR.walk_cases()}
RUNS = {r["name"]: r for r in PR.scene_runs()}


def _ref(case, bg=None):
    return [f(case["records"], case["offsets"], case["flatten_ids"], case["n_isects"], case["W"], case["H"],
              case["max_hit"], bg) for f in (PR.blend_f64, PR.blend_f32_replay)]


@pytest.fixture(scope="module")
def scenes():
    return {name: PR.reference_render(run) for name, run in RUNS.items()}


def test_names_are_unique():
    assert len(CASES) == len(PR.walk_cases()) and len(RUNS) == len(PR.scene_runs())


@pytest.mark.parametrize("name", CASES)
def test_walk_case_is_exact_and_the_replay_is_within_the_float64_bars(name):
    case = CASES[name]
    PR.assert_exact(case)
    worst = 0.0
    for bg in (None, BG):
        f64, f32 = _ref(case, bg)
        assert np.array_equal(f64["hits"], f32["hits"]), name           # the coverage decisions agree
        worst = max(worst, PR.judge(f32["rgb"], f32["alpha"], f32["depth"], f64, name))
    print(f"[point_raster_ref] {name}: replay, worst |f32 - f64| / bar = {worst:.3f}")


def test_scenes_are_exact_and_the_replay_is_within_the_float64_bars(scenes):
    for name, case in scenes.items():
        PR.assert_exact(case)
        assert np.array_equal(case["f64"]["hits"], case["f32"]["hits"]), name
        worst = PR.judge(case["f32"]["rgb"], case["f32"]["alpha"], case["f32"]["depth"], case["f64"], name)
        print(f"[point_raster_ref] {name}: replay, worst |f32 - f64| / bar = {worst:.3f}")


def test_float64_walk_is_the_contract_on_constant_occ_scenes():
    """blend_f64 over lists_from(project_f64(...)) against lidar_condition.render_points.  With occ = 1 render_points
    loops over (2 ceil(r_max) + 1)^2 offsets, so the discs larger than the image are compared translucent only."""
    K = lambda W, H: np.array([[PR.FOCAL, 0, W / 2], [0, PR.FOCAL, H / 2], [0, 0, 1.0]])
    c2w = np.linalg.inv(PR.W2C)
    assert np.array_equal(np.linalg.inv(c2w), PR.W2C)
    n = 0
    for name, run in RUNS.items():
        if run["kind"] != "hip":
            continue
        for occ in (1.0, run["occ"]):
            if occ == 1.0 and run["scale"] > 1:
                continue
            case = PR.reference_render(dict(run, occ=occ, bg=None))
            W, H = run["W"], run["H"]
            want = lc.render_points(c2w, K(W, H), run["points"], run["colors"], H, W, occ=occ, scale=run["scale"],
                                    max_hit=run["max_hit"], near=run["near"], far=run["far"])[0]
            got = np.concatenate([case["f64"]["rgb"], case["f64"]["alpha"][..., None]], -1)
            if occ == 1.0:
                np.testing.assert_array_equal(got.astype(np.float32), want, err_msg=name)
            else:
                assert np.abs(got.astype(np.float32).astype(np.float64) - want).max() <= 1e-12, name
            n += 1
    assert n >= 12


def test_lists_hold_every_covered_tile_and_the_edge_set_exactly_the_predicted_ones(scenes):
    for name, case in scenes.items():
        run, proj = RUNS[name], case["proj"]
        W, H = run["W"], run["H"]
        tw, th = PR.tiles_of(W, H)
        listed = {}
        for t in range(tw * th):
            s, e = PR.list_range(case["offsets"], case["n_isects"], t)
            for g in case["flatten_ids"][s:e]:
                listed.setdefault(int(g), set()).add(t)
        for i in np.nonzero(proj["keep"])[0]:
            cov = PR.covered_tiles(proj["u"][i], proj["v"][i], proj["r2"][i], W, H)
            assert cov <= listed.get(int(i), set()), (name, i)
        assert set(listed) <= set(np.nonzero(proj["keep"])[0].tolist())
        if "expect_tiles" in run:
            for i, tiles in enumerate(run["expect_tiles"]):
                assert listed[i] == tiles, (name, i, listed[i], tiles)
        if "expect_r" in run:
            assert np.array_equal(proj["r"], run["expect_r"]), name
        if "expect_lists" in run:
            for t in range(tw * th):
                s, e = PR.list_range(case["offsets"], case["n_isects"], t)
                assert e - s == run["expect_lists"].get(t, 0), (name, t)
        if "all_tiles" in run:
            assert case["n_isects"] == run["all_tiles"] * tw * th
            assert proj["R"].max() == (2 ** 30 if proj["r"].max() > 2 ** 30 else proj["r"].max())
        if "expect_keep" in run:
            assert proj["keep"].tolist() == run["expect_keep"], name
            if not any(run["expect_keep"]):
                assert case["n_isects"] == 0 and np.array_equal(case["f32"]["rgb"], np.broadcast_to(BG, (H, W, 3)))


def test_the_edge_discs_touch_pixels_and_r_zero_covers_its_own_pixel():
    exact, down, up = (CASES[f"edge_{t}"] for t in ("exact", "8ulp_down", "8ulp_up"))
    xs, ys = np.meshgrid(np.arange(PR.W0) + 0.5, np.arange(PR.H0) + 0.5)
    cov = lambda u, v, r: (xs - u) ** 2 + (ys - v) ** 2 <= r * r
    n = PR.edge_pixels(exact)
    # (list entry, pixel) pairs with d^2 == r^2: the same number straight from the discs, without the lists
    assert n == 88 == sum(int(((xs - u) ** 2 + (ys - v) ** 2 == r * r).sum()) for u, v, r, _ in PR.EDGE_DISCS), n
    assert PR.edge_pixels(down) == 2 and PR.edge_pixels(up) == 2        # the two r = 0 discs on a pixel centre remain
    h = [_ref(c)[0]["hits"] for c in (exact, down, up)]
    assert (h[0] - h[1]).sum() == n - 2 and np.array_equal(h[0], h[2])  # the touched pixels drop out / nothing changes
    # every radius of the issue is there, and each r > 0 touches a pixel that is the only one of its tile or strip
    assert {r for *_, r, _ in PR.EDGE_DISCS} == set(PR.EDGE_R) | {0.0}
    assert cov(20.5, 8.5, 5.0)[:16, :16].sum() == 1 and cov(11.5, 4.5, 13.0)[16:, 16:32].sum() == 1
    assert cov(44.5, 8.5, 5.0).sum() == 1 and cov(20.5, 28.5, 5.0).sum() == 1 and cov(28.5, 8.5, 5.0)[:4].sum() == 1
    assert cov(36.5, 20.5, 0.0).sum() == 1 and cov(4.0, 20.5, 0.0).sum() == 0 and cov(16.5, 16.5, 0.0)[16, 16]


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("cull_")])
def test_cull_cases_have_the_survivors_they_claim(name):
    case = CASES[name]
    t = case["tile"]
    keep = PR.cull_survivors(case, t)
    assert keep.size == 192
    assert tuple(int(keep[b * 64:(b + 1) * 64].sum()) for b in range(3)) == case["survivors"]
    # a strip sees fewer survivors than the tile wherever a small disc sits in another strip's rows
    per_strip = [int(PR.cull_survivors(case, t, rows=(4 * s, 4 * s + 3)).sum()) for s in range(4)]
    assert max(per_strip) <= keep.sum() and (sum(case["survivors"]) < 20 or min(per_strip) < keep.sum())
    # misses of both kinds, and survivors that cover nothing
    rec = case["records"][case["flatten_ids"]]
    assert ((rec[:, 2] == 1.0) & ~keep).sum() >= 32
    hits = _ref(case)[0]["hits"]
    x0, x1, y0, y1 = PR.tile_pixels(t, case["W"], case["H"])
    assert hits[y0:y1 + 1, x0:x1 + 1].max() <= keep.sum() and hits.sum() == hits[y0:y1 + 1, x0:x1 + 1].sum()


def test_cull_patterns_hold_an_empty_first_batch_and_an_empty_batch_between_two_others():
    assert any(p[0] == 0 and p[1] > 0 for p in PR.CULL_PATTERNS)
    assert any(p[0] > 0 and p[1] == 0 and p[2] > 0 for p in PR.CULL_PATTERNS)
    assert {s for p in PR.CULL_PATTERNS for s in p} == {0, 1, 7, 8, 9, 63, 64}


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("cap_")])
def test_cap_cases_reach_the_cap_where_they_claim(name):
    case = CASES[name]
    cap, t = case["cap"], case["tile"]
    hits = _ref(case)[0]["hits"]
    x0, x1, y0, y1 = PR.tile_pixels(t, case["W"], case["H"])
    assert (hits[y0:y1 + 1, x0:x1 + 1] == cap).all() and hits.sum() == cap * 256
    # how many list entries a pixel walks before its cap binds: the left 8 columns finish 64 entries earlier
    uncapped = _ref(dict(case, max_hit=1000))[0]["hits"][y0:y1 + 1, x0:x1 + 1]
    assert (uncapped[:, 8:] == 130).all() and (uncapped[:, :8] == (194 if case["half"] else 130)).all()


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("opaque_")])
def test_opaque_cases_finish_where_they_claim(name):
    case = CASES[name]
    t, k = case["tile"], case["finish"]
    x0, x1, y0, y1 = PR.tile_pixels(t, case["W"], case["H"])
    win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    f64 = _ref(case)[0]
    assert (f64["T"][win] == 0).all() and (f64["rgb"][win][..., 2] == 0).all()          # nothing bleeds through
    if k is None:
        assert len(np.unique(f64["rgb"][win].reshape(-1, 3), axis=0)) == 16
        return
    s = int(case["offsets"][t])
    cut = lambda m: PR.blend_f64(case["records"], np.where(np.arange(6) <= t, 0, m), case["flatten_ids"][s:s + m], m,
                                 case["W"], case["H"], 1000)["T"][win]
    # every 16 x 4 strip, and so the tile, still has an unfinished pixel after k - 1 records and none after k
    before, after = cut(k - 1), cut(k)
    assert (after == 0).all()
    assert all((before[r:r + 4] > 0).any() for r in range(0, y1 - y0 + 1, 4))
    assert PR.cull_survivors(case, t)[:k].all()
    assert all(PR.cull_survivors(case, t, rows=(r, r + 3))[:k].all() for r in range(0, y1 - y0 + 1, 4))
    assert PR.list_range(case["offsets"], case["n_isects"], t)[1] - s > k


def test_length_partial_and_tie_cases():
    for n in PR.LENGTHS:
        case = CASES[f"lengths_{n}"]
        assert case["n_isects"] == n
        hits = _ref(case)[0]["hits"]
        x0, x1, y0, y1 = PR.tile_pixels(case["tile"], case["W"], case["H"])
        assert hits.sum() == n * (x1 - x0 + 1) * (y1 - y0 + 1) and (hits[y0:y1 + 1, x0:x1 + 1] == n).all()
        assert len(np.unique(case["records"][case["flatten_ids"], 4:7], axis=0)) == n       # distinct colours
    hits = _ref(CASES["partial_tiles"])[0]["hits"]
    assert hits[:16, :32].sum() == 0 and hits[16:].min() >= 3 and hits[:, 32:].min() >= 3
    assert hits[:, 39].max() > 4 and hits[23].max() > 4                 # the discs centred outside reach in
    ties = CASES["ties"]
    z = ties["records"][ties["flatten_ids"], 3]
    assert (z[:6] == 4.0).all() and (z[6:] == 8.0).all() and not np.array_equal(np.sort(ties["flatten_ids"][:6]),
                                                                                  ties["flatten_ids"][:6])


# ---- do the cases bite?  A numpy model of a batched tile walk, with one defect switched on at a time -------------------
def _batched_walk(case, waves, bug=None):
    """The structure the cases are aimed at, restated in numpy float32: one wave per tile (16 rows) or per strip (4 rows),
    the list in batches of 64, cull against the wave's pixel-centre rectangle, compaction in list order, per-pixel done
    flags, an early-out looked at after every 8th surviving record.  `bug` names one defect."""
    f = np.float32
    W, H, max_hit = case["W"], case["H"], case["max_hit"]
    rec, ids, n = case["records"], case["flatten_ids"], case["n_isects"]
    tw, th = PR.tiles_of(W, H)
    rows = 16 // waves
    out = np.full((H, W, 5), np.nan, f)
    for t in range(tw * th):
        s, e = PR.list_range(case["offsets"], n, t)
        tx, ty = t % tw, t // tw
        for sub in range(waves):
            y0 = ty * 16 + sub * rows
            px, py = np.arange(tx * 16, tx * 16 + 16), np.arange(y0, y0 + rows)
            inside = (px[None, :] < W) & (py[:, None] < H)
            pxf, pyf = px.astype(f) + f(.5), py.astype(f) + f(.5)
            T, acc = np.ones((rows, 16), f), np.zeros((rows, 16, 4), f)
            hits, done = np.zeros((rows, 16), int), ~inside
            rx0, rx1 = f(tx * 16) + f(.5), f(min(tx * 16 + 15, W - 1)) + f(.5)
            ry0, ry1 = f(y0) + f(.5), f(min(y0 + rows - 1, H - 1)) + f(.5)
            for base in range(s, e, 64):
                if done.all():
                    break
                g = rec[ids[base:min(base + 64, n if bug == "batch_runs_past_the_list" else e)]]
                ex = np.maximum(np.maximum(rx0 - g[:, 0], g[:, 0] - rx1), f(0))
                ey = np.maximum(np.maximum(ry0 - g[:, 1], g[:, 1] - ry1), f(0))
                d2 = ex * ex + ey * ey
                surv = g[d2 < g[:, 2] if bug == "cull_excludes_the_edge" else d2 <= g[:, 2]]
                if bug == "compaction_reverses_the_batch":
                    surv = surv[::-1]
                if bug == "empty_batch_ends_the_walk" and len(surv) == 0:
                    break
                for k, p in enumerate(surv):
                    dx, dy = pxf - p[0], pyf - p[1]
                    dd = (dx * dx)[None, :] + (dy * dy)[:, None]
                    cov = (dd < p[2] if bug == "coverage_excludes_the_edge" else dd <= p[2]) & ~done
                    w = T * p[7]
                    for ch, val in enumerate((p[4], p[5], p[6], p[3])):
                        acc[..., ch] = np.where(cov, acc[..., ch] + w * val, acc[..., ch])
                    T = np.where(cov, T * (f(1) - p[7]), T)
                    hits = hits + cov
                    done = done | (cov & ((T == 0) | (hits > max_hit if bug == "cap_one_late" else hits >= max_hit)))
                    if bug == "done_is_per_wave" and (done & inside).any():
                        done = done | True
                    if bug == "early_out_on_any_pixel" and (k & 7) == 7 and (done & inside).any():
                        break
                    if (k & 7) == 7 and done.all():
                        break
            ys, xs = np.nonzero(inside)
            out[py[ys], px[xs], :3] = acc[ys, xs, :3]
            out[py[ys], px[xs], 3] = (f(1) - T)[ys, xs]
            out[py[ys], px[xs], 4] = acc[ys, xs, 3]
    return out


def _caught(bug):
    names = []
    for name, case in CASES.items():
        ref = _ref(case)[1]
        want = np.concatenate([ref["rgb"], ref["alpha"][..., None], ref["depth"][..., None]], -1)
        if any(not np.array_equal(_batched_walk(case, waves, bug).view(np.uint32), want.view(np.uint32))
               for waves in (1, 4)):
            names.append(name)
    return names


def test_a_faithful_batched_walk_is_the_replay_on_every_case():
    assert _caught(None) == []


@pytest.mark.parametrize("bug,where", [
    ("coverage_excludes_the_edge", "edge_exact"), ("cull_excludes_the_edge", "edge_exact"),
    ("compaction_reverses_the_batch", "lengths_63"), ("empty_batch_ends_the_walk", "cull_8_0_9"),
    ("batch_runs_past_the_list", "partial_tiles"), ("cap_one_late", "cap_64"), ("done_is_per_wave", "cap_8_left8"),
    ("early_out_on_any_pixel", "cap_9_left8")])
def test_a_defective_batched_walk_is_caught(bug, where):
    names = _caught(bug)
    print(f"[point_raster_ref] {bug}: caught by {len(names)} cases")
    assert where in names, (bug, names)
