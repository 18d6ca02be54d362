"""Float64 reference of the frame composition (street_crafter_amd/compose.py, csrc/compose.hip), written from the formulas
of the reference project:

  street_gaussian/models/street_gaussian_model.py:273-407   the five get_* properties (order: background, actors, sky;
                                                            :316-318 / :350 the flip, :319-320 / :351-352 the pose)
  street_gaussian/models/gaussian_model_actor.py:67-76      get_features_fourier (the IDFT sum over the DC block)
  street_gaussian/models/gaussian_model_sky.py:62-76        the clamp of the scales and the projection onto the sphere
  street_gaussian/utils/general_utils.py:125-146, 245-267   quaternion_to_matrix (2 / |q|^2), quaternion_raw_multiply
  street_gaussian/models/gaussian_model.py:215-241          exp / sigmoid / normalize

One statement of the formulas, `compose_model(...)`, written column by column on plain operators, runs three ways:
  * on float64 torch tensors: the reference G, differentiable by autograd (`run(case, torch.float64)`);
  * on float32 torch tensors: the fp32 torch restatement whose distance from G defines K_REF (`run(case, torch.float32)`;
    `mut=` applies one of MUTATIONS to it);
  * on tracked values T(v, s): s is S, the sum of the magnitudes of the element's terms with no cancellation (a product
    of sums is the product of the sums of magnitudes; exp, sigmoid, a norm and a quotient by one count as one term of
    their own magnitude).  `track(case)` runs the forward and a hand-written backward this way and returns S for every
    output and gradient; for a pose gradient the sum runs over all the actor's rows.  The hand-written backward's VALUES
    are checked against autograd in tests/test_compose_cpu.py.

The bar: |hip - G| <= 2^-24 K S with K = 4 K_REF, and exactly G where S = 0 (pure copies: background
and sky sh, features_rest everywhere, background means, sky means outside the sphere; gradients nothing reaches).
K_REF is the measured value; test_compose_cpu.py recomputes it over `build_cases()` and fails if it has moved by 1 %.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from street_crafter_amd import scene_io  # noqa: E402

EPS = 2.0 ** -24
K_REF = 5.162               # measured: the largest |fp32 restatement - G| / (2^-24 S) over build_cases()
STATIC, ACTOR, SKY = 0, 1, 2
MAX_SEGMENTS = 16           # sc_compose_max_segments(); the tests assert that it still is
NORM_EPS = float(np.float32(1e-12))
DECISION_MARGIN = 2.0 ** -21    # relative: a sky row this close to ratio == 1 or exp(scaling) == radius is "within one
                                # ulp of the decision" for an fp32 exp / sqrt that is good to a couple of ulps
PARAMS = ("xyz", "scaling", "rotation", "opacity", "features_dc", "features_rest")
OUTPUTS = ("means", "quats", "scales", "opacities", "sh")
MUTATIONS = ("flip_axis", "unit_rot", "clamp_grad", "basis_shift", "norm_rot_first")


# ---------------------------------------------------------------------------------------------------------------------
# tracked values
# ---------------------------------------------------------------------------------------------------------------------
class T:
    """value and S (sum of |terms|), float64 tensors of one shape"""
    __slots__ = ("v", "s")

    def __init__(self, v, s=None):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.s = self.v.abs() if s is None else torch.as_tensor(s, dtype=torch.float64)

    @staticmethod
    def lift(x):
        return x if isinstance(x, T) else T(x)

    def __add__(self, o):
        o = T.lift(o)
        return T(self.v + o.v, self.s + o.s)
    __radd__ = __add__

    def __sub__(self, o):
        o = T.lift(o)
        return T(self.v - o.v, self.s + o.s)

    def __rsub__(self, o):
        return T.lift(o) - self

    def __neg__(self):
        return T(-self.v, self.s)

    def __mul__(self, o):
        o = T.lift(o)
        return T(self.v * o.v, self.s * o.s)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = T.lift(o)
        return T(self.v / o.v, self.s / o.v.abs())

    def __rtruediv__(self, o):
        return T.lift(o) / self


def val(x):
    return x.v if isinstance(x, T) else x


def _one(fn, x):
    if isinstance(x, T):
        return T(fn(x.v))
    return fn(x)


def exp(x):
    return _one(torch.exp, x)


def sigmoid(x):
    return _one(torch.sigmoid, x)


def norm(cols):
    """|cols| per row: one term of its own magnitude; autograd's norm has the zero subgradient at 0, as F.normalize"""
    if isinstance(cols[0], T):
        return T(torch.sqrt(sum(c.v * c.v for c in cols)))
    return torch.linalg.vector_norm(torch.stack(torch.broadcast_tensors(*cols), -1), dim=-1)


def where(c, a, b):
    if isinstance(a, T) or isinstance(b, T):
        a, b = T.lift(a), T.lift(b)
        return T(torch.where(c, a.v, b.v), torch.where(c, a.s, b.s))
    return torch.where(c, a, b)


def rowsum(x):
    if isinstance(x, T):
        return T(x.v.sum(), x.s.sum())
    return x.sum()


def cols(t):
    if isinstance(t, T):
        return [T(v, s) for v, s in zip(t.v.unbind(-1), t.s.unbind(-1))]
    return list(t.unbind(-1))


# ---------------------------------------------------------------------------------------------------------------------
# the formulas
# ---------------------------------------------------------------------------------------------------------------------
def qmul(a, b):
    """Hamilton product, real part first (general_utils.py:245-267)"""
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def qmul_grad_a(g, b):
    return [g[0] * b[0] + g[1] * b[1] + g[2] * b[2] + g[3] * b[3],
            g[1] * b[0] - g[0] * b[1] - g[2] * b[3] + g[3] * b[2],
            g[2] * b[0] - g[0] * b[2] + g[1] * b[3] - g[3] * b[1],
            g[3] * b[0] - g[0] * b[3] - g[1] * b[2] + g[2] * b[1]]


def qmul_grad_b(g, a):
    return [g[0] * a[0] + g[1] * a[1] + g[2] * a[2] + g[3] * a[3],
            g[1] * a[0] - g[0] * a[1] + g[2] * a[3] - g[3] * a[2],
            g[2] * a[0] - g[0] * a[2] - g[1] * a[3] + g[3] * a[1],
            g[3] * a[0] - g[0] * a[3] + g[1] * a[2] - g[2] * a[1]]


def qmatrix(q, unit=False):
    """general_utils.py:125-146: s = 2 / |q|^2 (unit: the mutation that takes q for normalised, s = 2)"""
    r, i, j, k = q
    s = 2.0 if unit else 2.0 / (r * r + i * i + j * j + k * k)
    return [1.0 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
            s * (i * j + k * r), 1.0 - s * (i * i + k * k), s * (j * k - i * r),
            s * (i * k - j * r), s * (j * k + i * r), 1.0 - s * (i * i + j * j)]


def qmatrix_grad(q, G):
    """R = I + s M(q), G = dL/dR (9 values, already reduced or per row) -> dL/dq"""
    r, i, j, k = q
    s = 2.0 / (r * r + i * i + j * j + k * k)
    gs = (G[1] * (i * j - k * r) + G[2] * (i * k + j * r) + G[3] * (i * j + k * r) + G[5] * (j * k - i * r)
          + G[6] * (i * k - j * r) + G[7] * (j * k + i * r)
          - G[0] * (j * j + k * k) - G[4] * (i * i + k * k) - G[8] * (i * i + j * j))
    t = -(s * s) * gs
    return [s * (k * G[3] - k * G[1] + j * G[2] - i * G[5] - j * G[6] + i * G[7]) + t * r,
            s * (j * G[1] + k * G[2] + j * G[3] - 2.0 * i * G[4] - r * G[5] + k * G[6] + r * G[7] - 2.0 * i * G[8]) + t * i,
            s * (i * G[1] - 2.0 * j * G[0] + r * G[2] + i * G[3] + k * G[5] - r * G[6] + k * G[7] - 2.0 * j * G[8]) + t * j,
            s * (i * G[2] - 2.0 * k * G[0] - r * G[1] + r * G[3] - 2.0 * k * G[4] + j * G[5] + i * G[6] + j * G[7]) + t * k]


def normalize(q):
    """F.normalize: q / max(|q|, 1e-12) -> (unit, denominator, floored)"""
    n = norm(q)
    floored = ~(val(n) >= NORM_EPS)
    d = where(floored, NORM_EPS + 0.0 * n, n)
    return [c / d for c in q], d, floored


def normalize_grad(g, u, d, floored):
    dot = g[0] * u[0] + g[1] * u[1] + g[2] * u[2] + g[3] * u[3]
    return [where(floored, gi / d, (gi - ui * dot) / d) for gi, ui in zip(g, u)]


def basis_of(m, frame):
    """the IDFT basis of an actor at `frame` as python floats of fp32 values: scene_io.idft, pinned bit-exact by
    tests/golden/idft_ref.npz (gaussian_model_actor.py:68-71, sh_utils.py:120-130)"""
    F = m["features_dc"].shape[1]
    if m["kind"] != ACTOR or F == 1:
        return [1.0] + [0.0] * (F - 1)
    t = m["fourier_scale"] * (frame - m["start_frame"]) / (m["end_frame"] - m["start_frame"])
    return scene_io.idft(float(t), F)[0].tolist()


def compose_model(m, p, frame, pose, flip, flip_q, mut=None):
    """One sub-model.  p: its six raw tensors (torch, any float dtype, or T); pose: (rot [4 scalars], trans [3]) or None.
    -> dict of column lists: means[3], quats[4], scales[3], opacities, dc[3], plus what the backward needs."""
    x, rot = cols(p["xyz"]), cols(p["rotation"])
    qn, dn, fl_n = normalize(rot)
    e = [exp(c) for c in cols(p["scaling"])]
    out = dict(qn=qn, dn=dn, fl_n=fl_n, e=e, x=x)
    out["opacities"] = sigmoid(cols(p["opacity"])[0])
    basis = basis_of(m, frame)
    if mut == "basis_shift" and m["kind"] == ACTOR and len(basis) > 1:
        basis = basis[1:] + basis[:1]
    out["basis"] = basis
    dc = p["features_dc"]
    dcs = [cols(T(dc.v[:, f], dc.s[:, f]) if isinstance(dc, T) else dc[:, f]) for f in range(len(basis))]
    if m["kind"] == ACTOR and len(basis) > 1:
        out["dc"] = [sum((basis[f] * dcs[f][c] for f in range(1, len(basis))), basis[0] * dcs[0][c]) for c in range(3)]
    else:
        out["dc"] = dcs[0]
    if m["kind"] == ACTOR:
        prot, ptr = pose
        ql, xl = qn, list(x)
        if flip is not None:
            axis = 0 if mut == "flip_axis" else 1
            xl[axis] = where(flip, -xl[axis], xl[axis])
            qf = qmul([float(v) for v in flip_q], qn)
            ql = [where(flip, a, b) for a, b in zip(qf, qn)]
        pr = prot
        if mut == "norm_rot_first":
            pr = normalize(prot)[0]
        R = qmatrix(pr, unit=(mut == "unit_rot"))
        out["means"] = [R[3 * a] * xl[0] + R[3 * a + 1] * xl[1] + R[3 * a + 2] * xl[2] + ptr[a] for a in range(3)]
        w = qmul(prot, ql)
        out["quats"], out["dw"], out["fl_w"] = normalize(w)
        out["scales"] = e
        out.update(ql=ql, xl=xl, R=R)
    elif m["kind"] == SKY:
        rad = float(m["radius"])
        inside = [val(c) <= rad for c in e]
        out["passes"] = inside
        if mut == "clamp_grad":         # the clamp's gradient passed above the radius (fp32 replay only)
            out["scales"] = [c + (torch.where(i, c, torch.full_like(c, rad)) - c).detach() for c, i in zip(e, inside)]
        else:
            out["scales"] = [where(i, c, rad + 0.0 * c) for c, i in zip(e, inside)]
        ctr = [float(v) for v in m["centre"]]
        d = [x[a] - ctr[a] for a in range(3)]
        dist = norm(d)
        ratio = dist / (2.0 * rad)
        proj = val(ratio) < 1.0
        out["means"] = [where(proj, ctr[a] + d[a] / ratio, x[a]) for a in range(3)]
        out["quats"] = qn
        out.update(d=d, dist=dist, ratio=ratio, proj=proj)
    else:
        out["means"], out["quats"], out["scales"] = x, qn, e
    return out


def backward_model(m, f, g, pose, flip, flip_q):
    """The hand-written VJP, on T.  f: compose_model's dict; g: upstream columns (means[3], quats[4], scales[3],
    opacities, dc[3]).  -> (dict of parameter-gradient column lists, pose rot gradient [4] | None, trans [3] | None)"""
    out = {}
    gs = list(g["scales"])
    if m["kind"] == SKY:
        gs = [where(p, c, 0.0 * c) for c, p in zip(gs, f["passes"])]
    out["scaling"] = [c * e for c, e in zip(gs, f["e"])]
    sg = f["opacities"]
    out["opacity"] = [g["opacities"] * (sg * (1.0 - sg))]
    gx, gqn, g_rot, g_tr = list(g["means"]), list(g["quats"]), None, None
    if m["kind"] == ACTOR:
        prot, _ = pose
        R, gm = f["R"], g["means"]
        gx = [R[a] * gm[0] + R[3 + a] * gm[1] + R[6 + a] * gm[2] for a in range(3)]
        if flip is not None:
            gx[1] = where(flip, -gx[1], gx[1])
        gw = normalize_grad(g["quats"], f["quats"], f["dw"], f["fl_w"])
        gql = qmul_grad_b(gw, prot)
        gqn = gql
        if flip is not None:
            gqf = qmul_grad_b(gql, [float(v) for v in flip_q])
            gqn = [where(flip, a, b) for a, b in zip(gqf, gql)]
        G = [gm[a] * f["xl"][b] for a in range(3) for b in range(3)]
        g1, g2 = qmatrix_grad(prot, G), qmul_grad_a(gw, f["ql"])
        g_rot = [rowsum(a + b) for a, b in zip(g1, g2)]
        g_tr = [rowsum(c) for c in gm]
    elif m["kind"] == SKY:
        gm, dist, ratio = g["means"], f["dist"], f["ratio"]
        u = [c / dist for c in f["d"]]
        dot = gm[0] * u[0] + gm[1] * u[1] + gm[2] * u[2]
        gx = [where(f["proj"], (gm[a] - u[a] * dot) / ratio, gm[a]) for a in range(3)]
    out["xyz"] = gx
    out["rotation"] = normalize_grad(gqn, f["qn"], f["dn"], f["fl_n"])
    basis = f["basis"]
    if m["kind"] == ACTOR and len(basis) > 1:
        out["features_dc"] = [[basis[k] * g["dc"][c] for c in range(3)] for k in range(len(basis))]
    else:
        out["features_dc"] = [list(g["dc"])] + [[0.0 * g["dc"][c] for c in range(3)] for _ in basis[1:]]
    return out, g_rot, g_tr


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _model(rng, name, kind, n, K, F=1, **kw):
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    m = dict(name=name, kind=kind, n=n, start_frame=0, end_frame=1, fourier_scale=1.0, centre=(0.0, 0.0, 0.0), radius=1.0)
    m.update(kw)
    m["xyz"] = f32(rng.normal(0, 3.0, (n, 3)))
    m["scaling"] = f32(rng.normal(-1.0, 0.7, (n, 3)))
    m["rotation"] = f32(rng.normal(0, 1.0, (n, 4)) * rng.uniform(0.2, 3.0, (n, 1)))
    m["opacity"] = f32(rng.normal(0, 2.0, (n, 1)))
    m["features_dc"] = f32(rng.normal(0, 0.6, (n, F, 3)))
    m["features_rest"] = f32(rng.normal(0, 0.2, (n, K - 1, 3)))
    if n > 2:
        m["rotation"][n // 2] = 0.0                      # the 1e-12 floor
    return m


def _sky(rng, n, K):
    radius = float(np.float32(37.5))
    centre = tuple(float(np.float32(v)) for v in (1.25, -2.5, 0.75))
    m = _model(rng, "sky", SKY, n, K, centre=centre, radius=radius)
    # rows inside and outside the 2 radius sphere, none near its surface
    dirs = rng.normal(0, 1, (n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dist = np.where(np.arange(n) % 2 == 0, rng.uniform(0.2, 1.8, n), rng.uniform(2.2, 4.0, n)) * radius
    m["xyz"] = torch.from_numpy((np.asarray(centre) + dirs * dist[:, None]).astype(np.float32))
    # exp(scaling) below, above and (row 0, one channel) within one ulp of the radius
    sc = np.where(rng.uniform(size=(n, 3)) < 0.5, rng.uniform(0.0, 3.0, (n, 3)), rng.uniform(4.0, 5.0, (n, 3)))
    if n:
        sc[0, 1] = math.log(radius)
    m["scaling"] = torch.from_numpy(sc.astype(np.float32))
    return m


def _actor(rng, name, n, K, F, first, last, scale=1.0):
    return _model(rng, name, ACTOR, n, K, F, start_frame=first, end_frame=last, fourier_scale=scale)


def _poses(rng, A):
    """poses that are NOT normalised: R carries the 2 / |q|^2 scaling (general_utils.py:125-146)"""
    rots = rng.normal(0, 1, (A, 4))
    rots *= (rng.uniform(0.6, 1.7, (A, 1)) / np.linalg.norm(rots, axis=1, keepdims=True))
    return (torch.from_numpy(rots.astype(np.float32)), torch.from_numpy(rng.normal(0, 10.0, (A, 3)).astype(np.float32)))


def _finish(rng, name, models, frame, K, flip):
    actors = [m for m in models if m["kind"] == ACTOR]
    rots, trans = _poses(rng, max(len(actors), 1))
    N = sum(m["n"] for m in models)
    ups = {k: torch.from_numpy(rng.normal(0, 1.0, (N,) + s).astype(np.float32))
           for k, s in zip(OUTPUTS, ((3,), (4,), (3,), (1,), (K, 3)))}
    case = dict(name=name, models=models, frame=frame, K=K, obj_rots=rots[:len(actors)], obj_trans=trans[:len(actors)],
                flip=flip, flip_q=(0.0, 0.0, 1.0, 0.0), N=N, ups=ups)
    at = 0
    case["ranges"] = {}
    for m in models:
        case["ranges"][m["name"]] = [at, at + m["n"]]
        at += m["n"]
    ex = excluded(case)
    for key in ("means", "scales"):
        ups[key][torch.from_numpy(ex[key])] = 0.0
    case["excluded_rows"] = int((ex["means"] | ex["scales"]).sum())
    return case


def excluded(case):
    """bool [N] per field: sky rows within DECISION_MARGIN of ratio == 1 (means) or of exp(scaling) == radius (scales),
    which get no upstream gradient for that field"""
    out = {"means": np.zeros(case["N"], bool), "scales": np.zeros(case["N"], bool)}
    for m in case["models"]:
        if m["kind"] != SKY or m["n"] == 0:
            continue
        a, b = case["ranges"][m["name"]]
        d = m["xyz"].double() - torch.tensor(m["centre"], dtype=torch.float64)
        ratio = d.norm(dim=1) / (2.0 * m["radius"])
        out["means"][a:b] = ((ratio - 1.0).abs() <= DECISION_MARGIN).numpy()
        e = torch.exp(m["scaling"].double())
        out["scales"][a:b] = ((e / m["radius"] - 1.0).abs() <= DECISION_MARGIN).any(dim=1).numpy()
    return out


def _mixed(rng, n):
    f = torch.from_numpy(rng.uniform(size=n) < 0.5)
    if n > 1:
        f[0], f[1] = True, False
    return f


def build_cases():
    """The inputs of tests/test_compose_gpu.py (and of K_REF).  Segment sizes 0, 1, 63, 64, 65, 257 with starts at odd
    rows; K in {1, 16}; F in {1, 2, 5}; flip absent, all and mixed on actors with different poses; sky rows inside and
    outside the sphere, scales below, above and at the radius; a zero rotation row per sub-model; MAX_SEGMENTS + 1
    non-empty segments."""
    cases = []
    for K in (16, 1):
        rng = np.random.default_rng(100 + K)
        models = [_model(rng, "background", STATIC, 257, K),
                  _actor(rng, "obj_000", 63, K, 5, 0, 40, 1.0), _actor(rng, "obj_001", 64, K, 2, 3, 30, 0.5),
                  _actor(rng, "obj_002", 65, K, 1, 0, 20), _actor(rng, "obj_003", 0, K, 2, 0, 20),
                  _actor(rng, "obj_004", 1, K, 5, 5, 25, 1.0), _sky(rng, 131, K)]
        flip = {"obj_000": _mixed(rng, 63), "obj_001": torch.ones(64, dtype=torch.bool), "obj_004": _mixed(rng, 1)}
        cases.append(_finish(rng, f"main_K{K}", models, 7, K, flip))
    rng = np.random.default_rng(7)
    models = [_actor(rng, "obj_000", 257, 16, 2, 0, 9, 1.0), _actor(rng, "obj_001", 65, 16, 5, 0, 9, 1.0), _sky(rng, 63, 16)]
    cases.append(_finish(rng, "actors_only", models, 4, 16, {"obj_000": _mixed(rng, 257)}))
    rng = np.random.default_rng(8)
    sizes = [1, 3, 7, 0, 64, 2, 5, 65, 1, 0, 9, 4, 63, 2, 6, 11, 8]
    models = [_model(rng, "background", STATIC, 5, 16)] + \
             [_actor(rng, f"obj_{i:03d}", n, 16, (1, 2, 5)[i % 3], 0, 12, 1.0) for i, n in enumerate(sizes)] + \
             [_sky(rng, 9, 16)]
    # MAX_SEGMENTS + 1 NON-EMPTY segments (empty ones take no slot of a launch) and two empty ones among them: the
    # second launch starts inside the table, after segments the first one skipped
    assert sum(1 for m in models if m["n"] > 0) == MAX_SEGMENTS + 1 and len(models) == MAX_SEGMENTS + 3
    cases.append(_finish(rng, "max_segments_plus_1", models, 5, 16, {"obj_004": _mixed(rng, 64)}))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------------------------------------------------
def _actor_index(case):
    rows, k = {}, 0
    for m in case["models"]:
        if m["kind"] == ACTOR:
            rows[m["name"]] = k
            k += 1
    return rows


def run(case, dtype, ups=True, mut=None, pose_grad=True):
    """The torch statement in `dtype` -> dict of float64 numpy arrays: the five outputs, and with `ups` (True: the
    case's; a dict; None: forward only) "g/<model>/<param>", "g/obj_rots", "g/obj_trans" by autograd."""
    ups = case["ups"] if ups is True else ups
    rows = _actor_index(case)
    leaves = {m["name"]: {k: m[k].to(dtype).clone().requires_grad_(ups is not None) for k in PARAMS} for m in case["models"]}
    rots = case["obj_rots"].to(dtype).clone().requires_grad_(ups is not None and pose_grad)
    trans = case["obj_trans"].to(dtype).clone().requires_grad_(ups is not None and pose_grad)
    parts = {k: [] for k in OUTPUTS}
    for m in case["models"]:
        pose = (cols(rots[rows[m["name"]]]), cols(trans[rows[m["name"]]])) if m["kind"] == ACTOR else None
        p = leaves[m["name"]]
        f = compose_model(m, p, case["frame"], pose, case["flip"].get(m["name"]), case["flip_q"], mut)
        n = m["n"]
        stack = lambda cs: torch.stack([c.expand(n) for c in cs], -1)
        parts["means"].append(stack(f["means"])); parts["quats"].append(stack(f["quats"]))
        parts["scales"].append(stack(f["scales"])); parts["opacities"].append(f["opacities"].reshape(n, 1))
        parts["sh"].append(torch.cat((stack(f["dc"]).reshape(n, 1, 3), p["features_rest"]), dim=1))
    outs = {k: torch.cat(v, dim=0) for k, v in parts.items()}
    res = {k: v.detach().double().numpy() for k, v in outs.items()}
    if ups is None:
        return res
    loss = sum((outs[k] * ups[k].to(dtype)).sum() for k in OUTPUTS if ups.get(k) is not None)
    loss.backward()
    for m in case["models"]:
        for k in PARAMS:
            g = leaves[m["name"]][k].grad
            res[f"g/{m['name']}/{k}"] = (torch.zeros_like(leaves[m["name"]][k]) if g is None else g).double().numpy()
    if pose_grad:
        for key, t in (("g/obj_rots", rots), ("g/obj_trans", trans)):
            res[key] = (torch.zeros_like(t) if t.grad is None else t.grad).double().numpy()
    return res


def track(case, ups=True):
    """-> (value dict, S dict) with run()'s keys, from the tracked forward and the hand-written backward."""
    ups = case["ups"] if ups is True else ups
    rows = _actor_index(case)
    A = len(rows)
    V, S = {}, {}
    parts = {k: ([], []) for k in OUTPUTS}
    g_rots, g_trans = [[T(0.0)] * 4 for _ in range(A)], [[T(0.0)] * 3 for _ in range(A)]
    for m in case["models"]:
        n = m["n"]
        a, b = case["ranges"][m["name"]]
        p = {k: T(m[k].double()) for k in PARAMS}
        pose = None
        if m["kind"] == ACTOR:
            r = rows[m["name"]]
            pose = (cols(T(case["obj_rots"][r].double())), cols(T(case["obj_trans"][r].double())))
        flip = case["flip"].get(m["name"])
        f = compose_model(m, p, case["frame"], pose, flip, case["flip_q"])

        def put(key, cs, copy=None):
            v = torch.stack([c.v.expand(n) for c in cs], -1)
            s = torch.stack([c.s.expand(n) for c in cs], -1)
            if copy is not None:
                s = torch.where(copy.reshape(n, 1), torch.zeros_like(s), s)
            parts[key][0].append(v); parts[key][1].append(s)
        everywhere = torch.ones(n, dtype=torch.bool)
        put("means", f["means"], copy=everywhere if m["kind"] == STATIC else (~f["proj"] if m["kind"] == SKY else None))
        put("quats", f["quats"]); put("scales", f["scales"]); put("opacities", [f["opacities"]])
        dc_copy = everywhere if not (m["kind"] == ACTOR and len(f["basis"]) > 1) else None
        dcv = torch.stack([c.v for c in f["dc"]], -1).reshape(n, 1, 3)
        dcs = torch.stack([c.s for c in f["dc"]], -1).reshape(n, 1, 3)
        if dc_copy is not None:
            dcs = torch.zeros_like(dcs)
        rest = m["features_rest"].double()
        parts["sh"][0].append(torch.cat((dcv, rest), 1)); parts["sh"][1].append(torch.cat((dcs, torch.zeros_like(rest)), 1))
        if ups is None:
            continue
        up = lambda key, shape: T(ups[key][a:b].double()) if ups.get(key) is not None else T(torch.zeros((n,) + shape))
        gsh = up("sh", (case["K"], 3))
        g = dict(means=cols(up("means", (3,))), quats=cols(up("quats", (4,))), scales=cols(up("scales", (3,))),
                 opacities=cols(up("opacities", (1,)))[0], dc=cols(T(gsh.v[:, 0], gsh.s[:, 0])))
        grads, g_rot, g_tr = backward_model(m, f, g, pose, flip, case["flip_q"])
        for k in ("xyz", "scaling", "rotation", "opacity"):
            V[f"g/{m['name']}/{k}"] = torch.stack([c.v.expand(n) for c in grads[k]], -1).numpy()
            S[f"g/{m['name']}/{k}"] = torch.stack([c.s.expand(n) for c in grads[k]], -1).numpy()
        if m["kind"] != ACTOR:
            S[f"g/{m['name']}/xyz"] = np.where((f["proj"] if m["kind"] == SKY else ~everywhere).numpy()[:, None],
                                                S[f"g/{m['name']}/xyz"], 0.0)                  # a copy of the upstream
        dcg = grads["features_dc"]
        V[f"g/{m['name']}/features_dc"] = torch.stack([torch.stack([c.v.expand(n) for c in row], -1) for row in dcg], 1).numpy()
        s_dc = torch.stack([torch.stack([c.s.expand(n) for c in row], -1) for row in dcg], 1).numpy()
        S[f"g/{m['name']}/features_dc"] = s_dc if dc_copy is None else np.zeros_like(s_dc)
        V[f"g/{m['name']}/features_rest"] = gsh.v[:, 1:].numpy()
        S[f"g/{m['name']}/features_rest"] = np.zeros_like(V[f"g/{m['name']}/features_rest"])
        if m["kind"] == ACTOR:
            g_rots[rows[m["name"]]], g_trans[rows[m["name"]]] = g_rot, g_tr
    for k in OUTPUTS:
        V[k], S[k] = torch.cat(parts[k][0], 0).numpy(), torch.cat(parts[k][1], 0).numpy()
    if ups is not None:
        for key, rows_ in (("g/obj_rots", g_rots), ("g/obj_trans", g_trans)):
            w = len(rows_[0]) if rows_ else (4 if key.endswith("rots") else 3)
            V[key] = np.array([[float(c.v) for c in r] for r in rows_], dtype=np.float64).reshape(A, w)
            S[key] = np.array([[float(c.s) for c in r] for r in rows_], dtype=np.float64).reshape(A, w)
    return V, S


def frame_models(case, device=None, requires_grad=False):
    """the case's sub-models as street_crafter_amd.compose.FrameModel records (fresh leaves on `device`)"""
    from street_crafter_amd import compose
    out = []
    for m in case["models"]:
        t = {k: m[k].clone().to(device).requires_grad_(requires_grad) for k in PARAMS}
        out.append(compose.FrameModel(name=m["name"], kind=m["kind"], start_frame=m["start_frame"], end_frame=m["end_frame"],
                                      fourier_scale=m["fourier_scale"], centre=m["centre"], radius=m["radius"], **t))
    return out


def worst(got, G, S, keys=None):
    """max over the elements of |got - G| / (2^-24 S); inf where S == 0 and got != G.  -> (ratio, key)"""
    top, at = 0.0, None
    for key in (keys if keys is not None else G):
        if key not in got:
            continue
        err = np.abs(np.asarray(got[key], np.float64) - G[key])
        s = S[key]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(s > 0, err / (EPS * s), np.where(err == 0, 0.0, np.inf))
        r = np.where(np.isnan(r), np.inf, r)
        if r.size and r.max() > top:
            top, at = float(r.max()), key
    return top, at
