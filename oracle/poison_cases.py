"""Rows a diverging training run produces, as recipes to graft into a scene -- TEST INFRASTRUCTURE ONLY (numpy).

A recipe overwrites the geometry of one Gaussian (mean, quaternion, scale: always all three, so that its fate is the
recipe's and not the replaced row's) and, where it says so, its opacity or SH row.  Its CLASS is what the numpy oracle's
projection (oracle/gsplat_oracle.py::fully_fused_projection) does with it under the recipe's home camera:

  culled   radii == 0.  The row must be indistinguishable from an ordinary culled row: every forward output bit-identical
           to the TWIN scene's (the same scene with the row replaced by a benign one that is culled because it lies behind
           every camera: unit quaternion, scale 0.1, mean (0, 0, -8), opacity and SH of the row it replaces), its own
           gradients exactly +0, every other row's gradient what it is in the twin.
  visible  radii > 0: an ordinary Gaussian with extreme numbers.  Projection and intersection bit-exact with the oracle,
           pixels inside the float64 per-pixel bar; its own gradient may be non-finite, no other row's may.

Out of scope, as in the reference: a NaN opacity or colour on a VISIBLE row poisons every pixel the row covers (a NaN
alpha passes both skip tests and blends at 0.999, raster_common.h).  No recipe does that.  Neither does any recipe reach
a1 = +inf on a visible row: with det1 = +inf that gives the conic entry inf / inf = NaN, the same thing by another road.

The class is never asserted by hand: tests/test_poison_cases_cpu.py computes it and fails if a recipe lands in the other
class than the one written here.  "home" recipes are built for one camera (a depth of exactly near_plane needs that
camera's third row) and are classed under it; the others hold under every camera of the cases below.

name                      class    what it overwrites
mean_nan_x                culled   mean (NaN, -0.2, 8)
mean_nan_all              culled   mean (NaN, NaN, NaN)
mean_pinf_x               culled   mean (+inf, -0.2, 8)
mean_ninf_x               culled   mean (-inf, -0.2, 8)
mean_pinf_z               culled   mean (0.3, -0.2, +inf)
mean_ninf_z               culled   mean (0.3, -0.2, -inf)
mean_3e38_x               culled   mean (3e38, -0.2, 8): fx * x overflows; z finite under a camera without yaw
scale_nan_one             culled   scale (NaN, 0.1, 0.1)
scale_nan_all             culled   scale (NaN, NaN, NaN)
scale_inf_one             culled   scale (+inf, 0.1, 0.1)
scale_inf_all             culled   scale (+inf, +inf, +inf)
scale_2e19                culled   scale 2e19 on all axes: Sigma = +inf, then inf - inf
quat_zero                 culled   quaternion (0, 0, 0, 0): 1 / sqrt(0) = inf, 0 * inf
quat_1e-23                culled   1e-23 x a unit quaternion: n^2 underflows to 0
quat_nan_one              culled   quaternion (0.8, NaN, -0.4, 0.4)
quat_nan_all              culled   quaternion (NaN, NaN, NaN, NaN)
behind_nan_opacity        culled   mean (0.3, -0.2, -8) behind the camera, opacity NaN
behind_nan_sh             culled   the same mean, every SH coefficient NaN
behind_nan_both           culled   the same mean, opacity and SH NaN
near_below        (home)  culled   depth = the float32 below near_plane
far_above         (home)  culled   depth = the float32 above far_plane
near_exact        (home)  visible  depth = near_plane exactly (kept by !(z < near || z > far)), scale 1e-5
far_exact         (home)  visible  depth = far_plane exactly
quat_3e19                 visible  3e19 x a unit quaternion: n^2 = +inf, 1 / sqrt = 0, the rotation degenerates to identity
scale_1e-23               visible  scale 1e-23: Sigma underflows to 0, only eps2d is left (compensation 0)
iso_bb2_{m64,m8,p8,p64}   (home)  visible  isotropic scale around 2.334e8 at depth 10, x / z = 0.3: bb * bb overflows, det1 finite
iso_det1_{m64,m8,p8,p64}  (home)  visible  ... around 2.335e8: det1 = +inf, conic exactly 0, compensation 0
needle_bb2_{...}          (home)  visible  scale (s, 0.1, 0.1) around 3.391e8 on the optical axis at depth 10: bb * bb overflows
needle_subn_{...}         (home)  visible  ... around 5.150e17: a1 = 8.5e37, conic[0] = c1 / det1 goes subnormal
needle_det1_{...}         (home)  visible  ... around 5.474e17: a1 = 9.6e37, det1 = +inf, conic exactly 0, compensation 0

The ladders.  a1 is the x-x entry of the blurred 2-D covariance (pixel variance).  Each step is the smallest float32 scale
s* at which the named thing happens in float32 under the `plain` camera, found once by bisection over the bit patterns;
the rungs are s* - 64, s* - 8, s* + 8, s* + 64 ulps: two below, two above (the CPU test recomputes a1, bb * bb and det1 and
checks every rung's side).  Every rung has radius 2147483520 (clamped) and covers every tile; from the bb * bb step on the
discriminant is inf (radius = ceil(inf)) or inf - inf = NaN (fmaxf / np.fmax: the radius floor).
  An ISOTROPIC splat cannot reach a subnormal conic: its conic is 1 / a1 and its det1 = a1 * c1 overflows at a1 = 1.9e19,
  where the conic is 5e-20.  Its ladder has the two steps it can reach; they are 0.05 % apart in s (bb * bb - det1 =
  ((a1 - c1) / 2)^2, and a1 / c1 = 1.09 off the optical axis).
  The NEEDLE has all three, bb * bb first: bb * bb = a1^2 / 4 overflows at a1 = 3.7e19, the conic c1 / det1 = 1 / a1 goes
  subnormal at a1 = 8.5e37, det1 = a1 * 3.54 overflows at a1 = 9.6e37.  Its mean has y = 0 exactly under a camera whose
  second row is (0, 1, 0, 0): b is then exactly 0 (any other b has b * b = +inf long before and det1 = -inf: culled).

Dropped from the float64 judgements.  Pixels: none -- oracle/raster_fwd_f64.py judges the rasterizer on the float32
records it was given.  GRADIENTS (oracle/param_grad_f64.py, the chain recomputed in float64 from the leaves): twelve
recipes, listed in GRADIENT_DROPPED -- MORE than the three the plan for this catalogue allowed, because the reference
alone cannot meet its own conditions on them:
  iso_bb2_* and iso_det1_* (8)  both diagonal conic entries are <= 6e-20, so sigma is 0 to float32 on every pixel of the
                                frame: it sits AT the forward's hard threshold `sigma < 0`, the oracle flags 98 % of the
                                pixels unstable (cap: 0.5 %) and the case's loss weights are zero there -- nothing is judged;
  needle_det1_* (4)             conic exactly 0: the same in classic mode; antialiased, float32 has compensation 0 (det1 =
                                +inf) where the float64 chain has 0.957, i.e. another scene.
They keep every bit-exact check, the per-pixel judgement and, in the backward, "finite on every row that is not grafted".
The other twelve visible recipes (eight of them needles that reach every tile) are grafted together (gradient_judged) and
every row that is not grafted is held to the per-row float64 bar.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import gsplat_oracle as O

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
FRONT = (0.3, -0.2, 8.0)                 # in front of every camera of the cases used, well inside the frame
BEHIND = (0.3, -0.2, -8.0)
TWIN_MEAN = (0.0, 0.0, -8.0)             # at least 5 units behind every camera (the CPU test checks it)
QUAT = (0.8, 0.2, -0.4, 0.4)             # |q| = 1
UNIT = (1.0, 0.0, 0.0, 0.0)
SCALE = (0.1, 0.1, 0.1)
RADIUS_CLAMP = 2147483520
LADDER_OPACITY = 0.2
# the ladders' home camera is param_grad_f64's `plain` camera: means R^T (3, 0, 10) and R^T (0, 0, 10) with y = 0 (bits)
_ISO_MEAN = (1082060583, 0, 1092249758)
_NEEDLE_MEAN = (1065325268, 0, 1092563807)
# step -> the smallest float32 scale (bits) at which it happens
LADDER_STEPS = {"iso": (("bb2", 0x4d5e9a25), ("det1", 0x4d5eb497)),
                "needle": (("bb2", 0x4da1b6c9), ("subn", 0x5ce4b2b9), ("det1", 0x5cf31a77))}
RUNGS = (("m64", -64), ("m8", -8), ("p8", 8), ("p64", 64))

# fields: dict over a subset of means / quats / scales / opacities / sh ("sh": one value for the whole row); home: the
# recipe is built for one camera
Recipe = namedtuple("Recipe", "name cls fields home")


def _bits(*b):
    return tuple(float(np.uint32(v).view(np.float32)) for v in b)


def _geom(mean=FRONT, quat=QUAT, scale=SCALE, **more):
    return dict(means=mean, quats=quat, scales=scale, **more)


def _mean_at_depth(cam, depth):
    """World mean (0, 0, m) whose camera-space z is exactly float32 `depth` (the view matrix has no translation in z)."""
    V = cam.viewmat.numpy().astype(np.float32)
    assert V[2, 3] == 0.0, "a translated camera cannot reach every float32 depth"
    target = F32(depth)
    m = F32(np.float64(target) / np.float64(V[2, 2]))
    for _ in range(64):
        z = (V[2, 0] * F32(0.0) + V[2, 1] * F32(0.0)) + V[2, 2] * m + V[2, 3]
        if z == target:
            return (0.0, 0.0, float(m))
        m = np.nextafter(m, INF if z < target else -INF, dtype=np.float32)
    raise AssertionError(f"no float32 mean reaches depth {depth}")


def camera_free():
    """The recipes that hold under every camera."""
    q = np.asarray(QUAT, np.float32)
    return [
        Recipe("mean_nan_x", "culled", _geom(mean=(NAN, -0.2, 8.0)), False),
        Recipe("mean_nan_all", "culled", _geom(mean=(NAN, NAN, NAN)), False),
        Recipe("mean_pinf_x", "culled", _geom(mean=(INF, -0.2, 8.0)), False),
        Recipe("mean_ninf_x", "culled", _geom(mean=(-INF, -0.2, 8.0)), False),
        Recipe("mean_pinf_z", "culled", _geom(mean=(0.3, -0.2, INF)), False),
        Recipe("mean_ninf_z", "culled", _geom(mean=(0.3, -0.2, -INF)), False),
        Recipe("mean_3e38_x", "culled", _geom(mean=(3e38, -0.2, 8.0)), False),
        Recipe("scale_nan_one", "culled", _geom(scale=(NAN, 0.1, 0.1)), False),
        Recipe("scale_nan_all", "culled", _geom(scale=(NAN, NAN, NAN)), False),
        Recipe("scale_inf_one", "culled", _geom(scale=(INF, 0.1, 0.1)), False),
        Recipe("scale_inf_all", "culled", _geom(scale=(INF, INF, INF)), False),
        Recipe("scale_2e19", "culled", _geom(scale=(2e19, 2e19, 2e19)), False),
        Recipe("quat_zero", "culled", _geom(quat=(0.0, 0.0, 0.0, 0.0)), False),
        Recipe("quat_1e-23", "culled", _geom(quat=tuple(q * F32(1e-23))), False),
        Recipe("quat_nan_one", "culled", _geom(quat=(0.8, NAN, -0.4, 0.4)), False),
        Recipe("quat_nan_all", "culled", _geom(quat=(NAN, NAN, NAN, NAN)), False),
        Recipe("behind_nan_opacity", "culled", _geom(mean=BEHIND, opacities=NAN), False),
        Recipe("behind_nan_sh", "culled", _geom(mean=BEHIND, sh=NAN), False),
        Recipe("behind_nan_both", "culled", _geom(mean=BEHIND, opacities=NAN, sh=NAN), False),
        Recipe("quat_3e19", "visible", _geom(quat=tuple(q * F32(3e19))), False),
        Recipe("scale_1e-23", "visible", _geom(scale=(1e-23, 1e-23, 1e-23)), False),
    ]


def planes(cam, tag=""):
    """Depths at and just outside the planes of `cam` (home recipes)."""
    near, far = F32(cam.znear), F32(cam.zfar)
    tiny = (1e-5, 1e-5, 1e-5)
    return [
        Recipe("near_below" + tag, "culled", _geom(_mean_at_depth(cam, np.nextafter(near, -INF, dtype=np.float32)), UNIT, tiny), True),
        Recipe("far_above" + tag, "culled", _geom(_mean_at_depth(cam, np.nextafter(far, INF, dtype=np.float32)), UNIT), True),
        Recipe("near_exact" + tag, "visible", _geom(_mean_at_depth(cam, near), UNIT, tiny), True),
        Recipe("far_exact" + tag, "visible", _geom(_mean_at_depth(cam, far), UNIT), True),
    ]


def ladder_scale(kind, step, off):
    return _bits(dict(LADDER_STEPS[kind])[step] + off)[0]


def ladders():
    """The isotropic and the needle ladder (home camera: `plain`)."""
    out = []
    for kind, mean in (("iso", _bits(*_ISO_MEAN)), ("needle", _bits(*_NEEDLE_MEAN))):
        for step, _ in LADDER_STEPS[kind]:
            for tag, off in RUNGS:
                s = ladder_scale(kind, step, off)
                scale = (s, s, s) if kind == "iso" else (s, 0.1, 0.1)
                out.append(Recipe(f"{kind}_{step}_{tag}", "visible", _geom(mean, UNIT, scale, opacities=LADDER_OPACITY), True))
    return out


def catalogue(cam):
    """Every recipe, the home ones built for `cam` (the ladders' scales are those of param_grad_f64's `plain` camera)."""
    return camera_free() + planes(cam) + ladders()


GRADIENT_DROPPED = ("iso_bb2_", "iso_det1_", "needle_det1_")     # name prefixes; the reasons are in the module docstring


def gradient_judged(recipes):
    """The visible recipes on which the float64 gradient chain is a reference."""
    return [r for r in recipes if r.cls == "visible" and not r.name.startswith(GRADIENT_DROPPED)]


def by_name(recipes, *names):
    table = {r.name: r for r in recipes}
    return [table[n] for n in names]


def rows(recipes, sh_k, opacity=0.5, sh=0.1):
    """The recipes as a scene of their own: {means [R,3], quats [R,4], scales [R,3], opacities [R,1], sh [R,K,3]} float32;
    what a recipe leaves alone is `opacity` / `sh`."""
    R = len(recipes)
    out = dict(means=np.zeros((R, 3), np.float32), quats=np.zeros((R, 4), np.float32), scales=np.zeros((R, 3), np.float32),
               opacities=np.full((R, 1), opacity, np.float32), sh=np.full((R, sh_k, 3), sh, np.float32))
    for i, r in enumerate(recipes):
        for k, v in r.fields.items():
            out[k][i] = np.asarray(v, np.float32)
    return out


def project(leaves, cam, width, height, **kw):
    """The numpy oracle's projection of `leaves` under one camera."""
    return O.fully_fused_projection(leaves["means"], leaves["quats"], leaves["scales"], cam.viewmat.numpy(), cam.K.numpy(),
                                    width, height, near_plane=cam.znear, far_plane=cam.zfar, **kw)


def classes(recipes, cam, width, height):
    """{name: "culled" | "visible"} computed by the oracle under `cam`."""
    radii = project(rows(recipes, 1), cam, width, height)[0]
    return {r.name: ("visible" if radii[i] > 0 else "culled") for i, r in enumerate(recipes)}


def slots_for(n_rows, count):
    """`count` distinct rows of a scene of n_rows: row 0, both ends of the first wave boundary (63, 64) and of the first
    256-thread block boundary (255, 256), the last row, two adjacent rows (1000, 1001), then further boundary pairs and
    singles."""
    first = [0, 63, 64, 255, 256, n_rows - 1, 1000, 1001]
    more = [127, 128, 511, 512, 1023, 1024, 191, 192, 319, 320, 767, 768, 1279, 1280, 1535, 1536, 2047, 2048, 2303, 2304,
            5, 700, 1700, 2200, 333, 1111, 1999, 2400]
    out = [s for s in first + more if 0 <= s < n_rows]
    assert len(set(out)) == len(out) and count <= len(out), (n_rows, count)
    return out[:count]


def graft(case, recipes, slots):
    """case: an oracle/param_grad_f64.py::make_case dictionary.  -> (poisoned, twin): the case rebuilt with row slots[i]
    replaced by recipes[i], and with the same rows replaced by the benign culled row.  N and every other row's index are
    the case's (the sort breaks depth ties by index)."""
    from oracle import param_grad_f64 as PG
    assert len(recipes) == len(slots) == len(set(slots))
    poisoned = {k: case[k].copy() for k in PG.LEAVES}
    twin = {k: case[k].copy() for k in PG.LEAVES}
    for r, s in zip(recipes, slots):
        for k, v in r.fields.items():
            poisoned[k][s] = np.asarray(v, np.float32)
        twin["means"][s], twin["quats"][s], twin["scales"][s] = TWIN_MEAN, UNIT, SCALE
    return PG.with_leaves(case["case"], poisoned), PG.with_leaves(case["case"], twin)
