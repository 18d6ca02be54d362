"""oracle/poison_cases.py judged on the CPU, oracle only: every recipe lands in the class its entry names, the ladders
cross the float32 steps they are named after, a grafted culled row leaves every oracle output bit-identical to the twin
scene's, the C oracle agrees with numpy on the whole catalogue, and the float64 references stay well-conditioned on the
grafted scenes."""
import functools

import numpy as np
import pytest
import torch

from oracle import gsplat_oracle as O
from oracle import param_grad_f64 as PG
from oracle import poison_cases as PC
from oracle import raster_bwd_cases as RC
from oracle import raster_fwd_f64 as RF
from street_crafter_amd.scenes import make_camera

F = np.float32
W, H = 160, 96


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cams():
    """plain; yawed and off-centre; exact identity (W20 == 0: an infinite x meets 0 * inf)."""
    return dict(plain=PG.make_case("plain")["cameras"][0], yawed=PG.make_case("two_cameras")["cameras"][1],
                identity=make_camera(W, H, 180.0, 180.0))


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _stage(mean, quat, scale, V, K, eps2d=0.3):
    """a1, c1, b, bb * bb, det1 and the conic of ONE row: float32 scalar arithmetic in the projection's op order, written
    out here so that the ladders are checked by something that is neither a kernel nor the oracle."""
    with np.errstate(all="ignore"):
        V, K = np.asarray(V, F), np.asarray(K, F)
        mx, my, mz = (F(v) for v in mean)
        Wm = V[:3, :3]
        x = _dot3(Wm[0, 0], mx, Wm[0, 1], my, Wm[0, 2], mz) + V[0, 3]
        y = _dot3(Wm[1, 0], mx, Wm[1, 1], my, Wm[1, 2], mz) + V[1, 3]
        z = _dot3(Wm[2, 0], mx, Wm[2, 1], my, Wm[2, 2], mz) + V[2, 3]
        qw, qx, qy, qz = (F(v) for v in quat)
        inv = F(1.0) / np.sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
        qw, qx, qy, qz = qw * inv, qx * inv, qy * inv, qz * inv
        one, two = F(1.0), F(2.0)
        R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - qw * qz), two * (qx * qz + qw * qy)],
             [two * (qx * qy + qw * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qw * qx)],
             [two * (qx * qz - qw * qy), two * (qy * qz + qw * qx), one - two * (qx * qx + qy * qy)]]
        s = [F(v) for v in scale]
        M = [[R[i][j] * s[j] for j in range(3)] for i in range(3)]
        S = [[_dot3(M[i][0], M[j][0], M[i][1], M[j][1], M[i][2], M[j][2]) for j in range(3)] for i in range(3)]
        T = [[_dot3(Wm[i, 0], S[0][j], Wm[i, 1], S[1][j], Wm[i, 2], S[2][j]) for j in range(3)] for i in range(3)]
        c = [[_dot3(T[i][0], Wm[j, 0], T[i][1], Wm[j, 1], T[i][2], Wm[j, 2]) for j in range(3)] for i in range(3)]
        fx, fy = K[0, 0], K[1, 1]
        limx, limy = F(1.3) * (F(0.5) * F(W) / fx), F(1.3) * (F(0.5) * F(H) / fy)
        rz = one / z
        rz2 = rz * rz
        tx = z * min(limx, max(-limx, x * rz))
        ty = z * min(limy, max(-limy, y * rz))
        ja, jb, jc, jd = fx * rz, ((-fx) * tx) * rz2, fy * rz, ((-fy) * ty) * rz2
        u0 = ja * c[0][0] + jb * c[0][2]
        u1 = ja * c[0][1] + jb * c[1][2]
        u2 = ja * c[0][2] + jb * c[2][2]
        v1 = jc * c[1][1] + jd * c[1][2]
        v2 = jc * c[1][2] + jd * c[2][2]
        a, b, cc = u0 * ja + u2 * jb, u1 * jc + u2 * jd, v1 * jc + v2 * jd
        a1, c1 = a + F(eps2d), cc + F(eps2d)
        det1 = a1 * c1 - b * b
        bb = F(0.5) * (a1 + c1)
        return dict(z=z, a1=a1, c1=c1, b=b, bb2=bb * bb, det1=det1, conic=(c1 / det1, (-b) / det1, a1 / det1))


def test_every_recipe_lands_in_the_class_its_entry_names():
    cams = _cams()
    cat = PC.catalogue(cams["plain"])
    assert len({r.name for r in cat}) == len(cat)
    got = PC.classes(cat, cams["plain"], W, H)
    assert {r.name: r.cls for r in cat} == got
    assert sum(r.cls == "culled" for r in cat) >= 20 and sum(r.cls == "visible" for r in cat) >= 24
    for name, cam in cams.items():      # the camera-free ones under every camera, the planes under the camera they are built for
        free = PC.camera_free()
        assert {r.name: r.cls for r in free} == PC.classes(free, cam, W, H), name
        if name != "yawed":
            pl = PC.planes(cam)
            assert {r.name: r.cls for r in pl} == PC.classes(pl, cam, W, H), name
    # the geometry the poisoned recipes start from is an ordinary visible row, the twin's row an ordinary culled one
    base = [PC.Recipe("front", "visible", PC._geom(), False), PC.Recipe("twin", "culled", PC._geom(PC.TWIN_MEAN, PC.UNIT), False)]
    for name, cam in cams.items():
        assert PC.classes(base, cam, W, H) == {"front": "visible", "twin": "culled"}, name
    for cid in ("plain", "two_cameras"):
        for cam in PG.make_case(cid)["cameras"]:
            V = cam.viewmat.double().numpy()
            assert V[2, :3] @ np.array(PC.TWIN_MEAN) + V[2, 3] <= -5.0


def test_the_docstring_lists_every_recipe_with_its_class():
    doc = PC.__doc__
    for r in PC.catalogue(_cams()["plain"]):
        name = r.name
        if name.startswith(("iso_", "needle_")):
            name = name.rsplit("_", 1)[0] + "_{"
        line = [ln for ln in doc.splitlines() if ln.startswith(name)]
        assert len(line) == 1 and r.cls in line[0].split() and (("(home)" in line[0]) == r.home), r.name


def test_the_ladders_cross_the_steps_they_are_named_after():
    cam = _cams()["plain"]
    V, K = cam.viewmat.numpy(), cam.K.numpy()
    sub = F(2.0 ** -126)
    happened = {"bb2": lambda d: np.isinf(d["bb2"]), "det1": lambda d: np.isposinf(d["det1"]),
                "subn": lambda d: 0 < abs(d["conic"][0]) < sub}
    lad = PC.ladders()
    seen = set()
    for r in lad:
        kind, step, tag = r.name.split("_")
        d = _stage(r.fields["means"], r.fields["quats"], r.fields["scales"], V, K)
        assert d["z"] == F(10.0) or abs(d["z"] - 10.0) < 2e-6
        assert np.isfinite(d["a1"]) and d["b"] == 0, r.name
        above = tag.startswith("p")
        if step == "det1":
            assert bool(happened["det1"](d)) == above and np.isinf(d["bb2"]), r.name
            assert (d["conic"][0] == 0 and d["conic"][2] == 0) == above, r.name
        elif step == "bb2":
            assert bool(happened["bb2"](d)) == above and np.isfinite(d["det1"]), r.name
        else:
            assert bool(happened["subn"](d)) == above and np.isfinite(d["det1"]) and d["conic"][0] > 0, r.name
        seen.add((kind, step, above))
    assert seen == {(k, s, a) for k, steps in PC.LADDER_STEPS.items() for s, _ in steps for a in (False, True)}
    # a1 walks up: each ladder's rungs are ordered in a1, and the needle's subnormal step sits near 1e38
    for kind in PC.LADDER_STEPS:
        a1 = [float(_stage(r.fields["means"], r.fields["quats"], r.fields["scales"], V, K)["a1"]) for r in lad if r.name.startswith(kind)]
        assert a1 == sorted(a1) and len(set(a1)) > len(a1) // 2
    a1 = float(_stage(*(PC.by_name(lad, "needle_subn_p8")[0].fields[k] for k in ("means", "quats", "scales")), V, K)["a1"])
    assert 5e37 < a1 < 2e38
    # the oracle: every rung visible at the clamped radius
    radii = PC.project(PC.rows(lad, 1), cam, W, H)[0]
    assert (radii == PC.RADIUS_CLAMP).all()


@functools.lru_cache(maxsize=None)
def _grafted(case_id, cls):
    case = PG.make_case(case_id)
    cams = case["cameras"]
    cat = PC.catalogue(cams[0])
    pick = [r for r in cat if r.cls == cls and (len(cams) == 1 or not r.home)] if cls != "judged" else PC.gradient_judged(cat)
    slots = PC.slots_for(case["means"].shape[0], len(pick))
    return pick, slots, PC.graft(case, pick, slots)


def _others(ref, n, slots):
    """The reference's G / S / A restricted to the rows that are not grafted."""
    keep = np.setdiff1d(np.arange(n), slots)
    return keep, {q: {k: (v[:, keep] if k == "means2d" else v[keep]) for k, v in ref[q].items()} for q in ("G", "S", "A")}


@pytest.mark.parametrize("case_id", ["plain", "two_cameras"])
def test_grafted_culled_rows_leave_every_oracle_output_identical_to_the_twin(case_id):
    pick, slots, (p, t) = _grafted(case_id, "culled")
    assert {0, 63, 64, 255, 256, p["means"].shape[0] - 1, 1000, 1001} <= set(slots) and len(pick) >= 19
    assert (p["radii"][:, slots] == 0).all() and (t["radii"][:, slots] == 0).all()
    for k in ("radii", "means2d", "depths", "conics", "compensations", "colors", "isect_offsets", "flatten_ids", "unstable",
              "w_rgb", "w_acc", "w_depth"):
        np.testing.assert_array_equal(_bits(p[k]), _bits(t[k]), err_msg=k)
    C = len(p["cameras"])
    lists = [O.isect_tiles(q["means2d"], q["radii"], q["depths"], 16, 10, 6, n_cameras=C) for q in (p, t)]
    for a, b in zip(*lists):
        np.testing.assert_array_equal(a, b)
    # opacities * compensations of a culled row: NaN * 0 stays NaN where the recipe holds a NaN opacity, nowhere else
    diff = np.nonzero((_bits(p["opacities2d"]) != _bits(t["opacities2d"])).any(0))[0]
    nan_op = {s for r, s in zip(pick, slots) if "opacities" in r.fields}
    assert set(diff) == nan_op


def test_the_c_oracle_agrees_with_numpy_on_the_catalogue():
    from oracle import gsplat_oracle_c as OC
    OC.load()
    cams = _cams()
    cat = PC.catalogue(cams["plain"]) + PC.planes(cams["identity"], "@identity")
    L = PC.rows(cat, 1)
    for name, cam in cams.items():
        for clamp in O.PROJ_CLAMPS:
            for floor in O.RADIUS_FLOORS:
                kw = dict(near_plane=cam.znear, far_plane=cam.zfar, proj_clamp=clamp, radius_floor=floor)
                a = O.fully_fused_projection(L["means"], L["quats"], L["scales"], cam.viewmat.numpy(), cam.K.numpy(), W, H, **kw)
                b = OC.fully_fused_projection(L["means"], L["quats"], L["scales"], cam.viewmat.numpy(), cam.K.numpy(), W, H, **kw)
                for x, y, what in zip(a, b, ("radii", "means2d", "depths", "conics", "compensations")):
                    np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{name} {clamp} {floor} {what}")
        m2, r, d = a[1][None], a[0][None], a[2][None]
        for x, y in zip(O.isect_tiles(m2, r, d, 16, 10, 6), OC.isect_tiles(m2, r, d, 16, 10, 6)):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("case_id", ["plain", "two_cameras"])
def test_the_twin_scene_keeps_the_float64_gradient_reference_well_conditioned(case_id):
    _, _, (_, t) = _grafted(case_id, "culled")
    ref = PG.reference(t)
    rep = PG.worst_ratios(PG.chain(t, torch.float32)["G"], ref)
    k_ref = max(r for r, _ in rep.values())
    print(f"[replay] twin of {case_id}: K_ref {k_ref:.1f}")
    assert all(off == 0.0 for _, off in rep.values()) and PG.K_REF_BAND[0] < k_ref < PG.K_REF_BAND[1]
    assert float(t["unstable"].mean()) < RC.UNSTABLE_CAP


def test_visible_rows_leave_the_float64_gradient_reference_well_conditioned():
    """The twelve visible recipes the float64 chain can judge, grafted together: the float32 replay of the chain stays inside
    K_REF_BAND on every row that is not grafted, and the unstable share under its cap.  The other twelve: the reference
    alone fails its conditions (the reasons are in the catalogue's docstring), which is why they are dropped."""
    pick, slots, (p, _) = _grafted("plain", "judged")
    names = {r.name for r in pick}
    assert len(pick) == 12 and {"quat_3e19", "scale_1e-23", "near_exact", "far_exact", "needle_bb2_p8", "needle_subn_p64"} <= names
    assert (p["radii"][0, slots] == PC.RADIUS_CLAMP).sum() == 8 and float(p["unstable"].mean()) < RC.UNSTABLE_CAP
    n = p["means"].shape[0]
    keep, ref = _others(PG.reference(p), n, slots)
    G = PG.chain(p, torch.float32)["G"]
    rep = PG.worst_ratios({k: (v[:, keep] if k == "means2d" else v[keep]) for k, v in G.items()}, ref)
    k_ref = max(r for r, _ in rep.values())
    print(f"[replay] visible rows grafted: K_ref {k_ref:.1f}")
    assert all(off == 0.0 for _, off in rep.values()) and PG.K_REF_BAND[0] < k_ref < PG.K_REF_BAND[1]
    assert all(np.isfinite(v).all() for q in ref.values() for v in q.values()) and (ref["S"]["means"] > 0).sum() > 1000
    # the dropped ones, one at a time: the oracle's own unstable flag (or, antialiased, the float32 compensation) rules them out
    cat = PC.catalogue(p["cameras"][0])
    dropped = [r for r in cat if r.cls == "visible" and r not in pick]
    assert len(dropped) == 12 and all(r.name.startswith(PC.GRADIENT_DROPPED) for r in dropped)
    for name in ("iso_bb2_m64", "iso_det1_p8"):
        q, _ = PC.graft(PG.make_case("plain"), PC.by_name(cat, name), [5])
        assert float(q["unstable"].mean()) > 0.9, name
    q, _ = PC.graft(PG.make_case("plain"), PC.by_name(cat, "needle_det1_p8"), [5])
    assert q["compensations"][0, 5] == 0 and q["radii"][0, 5] == PC.RADIUS_CLAMP


@pytest.mark.parametrize("rasterize_mode", ["antialiased", "classic"])
def test_visible_rows_leave_the_float64_pixel_reference_usable(rasterize_mode):
    """The share of pixels oracle/raster_fwd_f64.py judges against more than one outcome stays under the cap its GPU test
    asserts, with every visible recipe grafted (classic: the opacities are the leaves', so that a conic of exactly 0 blends)."""
    pick, slots, (p, _) = _grafted("plain", "visible")
    assert len(pick) >= 24 and (p["radii"][:, slots] > 0).all()
    op = p["opacities2d"] if rasterize_mode == "antialiased" else np.broadcast_to(p["opacities"][None, :, 0], p["radii"].shape)
    assert np.isfinite(op).all()
    ref = RF.rasterize_fwd(p["means2d"], p["conics"], p["colors"], np.ascontiguousarray(op), W, H, 16, p["isect_offsets"],
                           p["flatten_ids"])
    assert RF.near_share(ref) < RC.UNSTABLE_CAP and ref["truncated"] == 0
    assert np.isfinite(ref["colors"]).all() and np.isfinite(ref["alphas"]).all()
    # every tile lists the clamped splats
    offs = np.append(p["isect_offsets"].reshape(-1), p["flatten_ids"].shape[0])
    clamped = {s for s in slots if p["radii"][0, s] == PC.RADIUS_CLAMP}
    assert len(clamped) == 20
    assert all(clamped <= set(p["flatten_ids"][offs[i]:offs[i + 1]]) for i in range(offs.size - 1))
