"""The actor poses of a frame (include/street_crafter_amd.h, sc_actor_poses_fwd / _bwd), restated three times:

  poses(items, tab, np.float64)   numpy float64 on the fp32 inputs: the truth.  Its slerp is the closed form, no series
                                  (sin(alpha phi) / |v| is well conditioned for every |v| > 0; |v| == 0 gives alpha)
  poses(items, tab, np.float32)   numpy float32, the kernel's operations one by one, each rounded on its own: the replay
                                  (bit-equal to the kernel wherever no cosf / sinf / atan2f is involved)
  TorchActorPose                  plain torch, per actor, with the reference's device-side asserts: the A/B's other side
                                  and the chain test's

`items`: rows of (row, row_prev, row_next, flags, alpha, one_minus_alpha) as the C table has them; `tab`: dict of flat
float32 arrays input_trans [rows,3], input_rots [rows,4], opt_trans [rows,3], opt_rots [rows].
"""
import numpy as np

DELTA, INTERP = 1, 2
NORM_EPS = 1e-12
SERIES_PHI = 1e-3


def qmul(a, b):
    """Hamilton product, real part first; four terms per component, summed left to right"""
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack((((aw * bw - ax * bx) - ay * by) - az * bz,
                     ((aw * bx + ax * bw) + ay * bz) - az * by,
                     ((aw * by - ax * bz) + ay * bw) + az * bx,
                     ((aw * bz + ax * by) - ay * bx) + az * bw), -1)


def conj(q):
    return q * np.array([1, -1, -1, -1], dtype=q.dtype)


def normalize(q):
    T = q.dtype.type
    n = np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])
    return q / np.maximum(n, T(NORM_EPS))[..., None]


def slerp(p, n, alpha):
    """p, n [m,4] of one dtype, alpha [m] of the same: the geometric slerp, its sign following normalize(p)"""
    T = p.dtype.type
    ph, nh = normalize(p), normalize(n)
    r = qmul(conj(ph), nh)
    r = np.where(r[..., :1] < 0, -r, r)
    v = r[..., 1:]
    sv = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    phi = np.arctan2(sv, r[..., 0])
    ap = alpha * phi
    with np.errstate(divide="ignore", invalid="ignore"):
        direct = np.sin(ap) / sv
    if T is np.float64:
        ew, f = np.cos(ap), np.where(sv > 0, direct, alpha)
    else:
        p2, a2 = phi * phi, alpha * alpha
        small = phi <= T(SERIES_PHI)
        ew = np.where(small, T(1) - T(0.5) * (a2 * p2), np.cos(ap))
        f = np.where(small, alpha * (T(1) + ((T(1) - a2) * p2) * T(np.float32(1.0) / np.float32(6.0))), direct)
    e = np.stack((ew, f * v[..., 0], f * v[..., 1], f * v[..., 2]), -1)
    return qmul(ph, e)


def plain(tab, rows, delta, T):
    """P(row) for each of `rows`, with the deltas where `delta` [m] bool -> (t [m,3], q [m,4])"""
    rows = np.asarray(rows, dtype=np.int64)
    delta = np.asarray(delta, dtype=bool)
    t = tab["input_trans"][rows].astype(T)
    a = tab["input_rots"][rows].astype(T)
    if delta.any():
        t = np.where(delta[:, None], t + tab["opt_trans"][rows].astype(T), t)
        half = tab["opt_rots"][rows].astype(T) * T(0.5)
        c, s = np.cos(half), np.sin(half)
        aw, ax, ay, az = (a[:, k] for k in range(4))
        q = np.stack((aw * c - az * s, ax * c + ay * s, ay * c - ax * s, az * c + aw * s), -1)
        a = np.where(delta[:, None], q, a)
    return t, a


def poses(items, tab, T):
    """-> obj_rots [A,4], obj_trans [A,3] of dtype T"""
    items = np.asarray(items, dtype=np.float64).reshape(-1, 6)
    row, prev, nxt, flags = (items[:, k].astype(np.int64) for k in range(4))
    alpha = items[:, 4].astype(np.float32).astype(T)
    oma = items[:, 5].astype(np.float32).astype(T)
    delta, interp = (flags & DELTA) != 0, (flags & INTERP) != 0
    t, q = plain(tab, row, delta, T)
    if interp.any():
        tp, qp = plain(tab, prev, delta, T)
        tn, qn = plain(tab, nxt, delta, T)
        t = np.where(interp[:, None], alpha[:, None] * tn + oma[:, None] * tp, t)
        q = np.where(interp[:, None], slerp(qp, qn, alpha), q)
    return q, t


def backward64(items, tab, g_rots, g_trans, n_rows):
    """float64 closed form -> (grad_opt_trans [rows,3], grad_opt_rots [rows], the bar's sum_k |g_k| (|a1_k| + |a2_k|) [rows])"""
    items = np.asarray(items, dtype=np.float64).reshape(-1, 6)
    gt, gr, mag = np.zeros((n_rows, 3)), np.zeros(n_rows), np.zeros(n_rows)
    for i, it in enumerate(items):
        row, flags = int(it[0]), int(it[3])
        assert not flags & INTERP
        if not flags & DELTA:
            continue
        if g_trans is not None:
            gt[row] = g_trans[i].astype(np.float64)
        if g_rots is not None:
            g = g_rots[i].astype(np.float64)
            aw, ax, ay, az = tab["input_rots"][row].astype(np.float64)
            half = np.float64(tab["opt_rots"][row]) / 2
            dc, ds = -np.sin(half) / 2, np.cos(half) / 2
            gr[row] = g[0] * (aw * dc - az * ds) + g[1] * (ax * dc + ay * ds) + g[2] * (ay * dc - ax * ds) + \
                g[3] * (az * dc + aw * ds)
            mag[row] = abs(g[0]) * (abs(aw) + abs(az)) + abs(g[1]) * (abs(ax) + abs(ay)) + \
                abs(g[2]) * (abs(ay) + abs(ax)) + abs(g[3]) * (abs(az) + abs(aw))
    return gt, gr, mag


def plain_rot_bar(tab, items):
    """|a1| + |a2| per component of the plain rotations: (w: aw, az) (x: ax, ay) (y: ay, ax) (z: az, aw) -> [A,4]"""
    items = np.asarray(items, dtype=np.float64).reshape(-1, 6)
    a = np.abs(tab["input_rots"][items[:, 0].astype(np.int64)].astype(np.float64))
    return np.stack((a[:, 0] + a[:, 3], a[:, 1] + a[:, 2], a[:, 2] + a[:, 1], a[:, 3] + a[:, 0]), -1)


# ---- the cases -----------------------------------------------------------------------------------------------------------
ALPHAS = (0.0, 0.25, 0.5, 0.9, 1.0)


def slerp_pairs(seed=0, n_random=24):
    """(p [m,4], n [m,4], what [m]) float32: random pairs, p == n, n ~ -p, n = p + 1e-5 noise, unnormalised inputs"""
    g = np.random.default_rng(seed)
    unit = lambda m: (lambda q: q / np.linalg.norm(q, axis=-1, keepdims=True))(g.standard_normal((m, 4)))
    P, N, what = [], [], []
    p, n = unit(n_random), unit(n_random)
    P.append(p); N.append(n); what += ["random"] * n_random
    p = unit(6)
    P.append(p); N.append(p.copy()); what += ["equal"] * 6
    p = unit(6)
    P.append(p); N.append(-p + 1e-4 * g.standard_normal((6, 4))); what += ["opposite"] * 6
    P.append(p.copy()); N.append(-p); what += ["opposite"] * 6
    p = unit(6)
    P.append(p); N.append(p + 1e-5 * g.standard_normal((6, 4))); what += ["near"] * 6
    p, n = unit(8), unit(8)
    P.append(p * g.uniform(0.5, 2.0, (8, 1))); N.append(n * g.uniform(0.5, 2.0, (8, 1))); what += ["unnormalised"] * 8
    return np.concatenate(P).astype(np.float32), np.concatenate(N).astype(np.float32), what


def make_table(cams, frames, max_obj, seed=0):
    """-> (camera_tracklets float32 [cams,frames,max_obj,8] with every row valid, camera_timestamps [cams][frames],
    opt_trans [cams,frames,max_obj,3], opt_rots [cams,frames,max_obj,1]).  Rotation rows are scaled by 0.5 .. 2 (the plain
    path does not normalise); theta covers [-pi, pi] with 0 and +-pi among the first rows of every frame.  The slerp pairs
    of slerp_pairs() sit at frames 1 / 3 of camera 0 (objects 0 .. m-1, where they fit), so frame 2 interpolates them."""
    g = np.random.default_rng(seed)
    tr = np.zeros((cams, frames, max_obj, 8), dtype=np.float32)
    tr[..., 0:3] = g.uniform(-50, 50, (cams, frames, max_obj, 3))
    q = g.standard_normal((cams, frames, max_obj, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    tr[..., 3:7] = q * g.uniform(0.5, 2.0, (cams, frames, max_obj, 1))
    tr[..., 7] = 1.0
    P, N, _ = slerp_pairs(seed)
    m = min(len(P), max_obj)
    if frames >= 4:
        tr[0, 1, :m, 3:7], tr[0, 3, :m, 3:7] = P[:m], N[:m]
    ts = [[1000.0 + 0.1 * f + 0.013 * c + 0.004 * np.sin(3.0 * f) for f in range(frames)] for c in range(cams)]
    opt_trans = g.uniform(-0.5, 0.5, (cams, frames, max_obj, 3)).astype(np.float32)
    theta = g.uniform(-np.pi, np.pi, (cams, frames, max_obj, 1)).astype(np.float32)
    special = np.array([0.0, np.pi, -np.pi], dtype=np.float32)
    k = min(3, max_obj)
    theta[:, :, :k, 0] = special[:k]
    return tr, ts, opt_trans, theta


def flat(tr, opt_trans, opt_rots):
    return dict(input_trans=np.ascontiguousarray(tr[..., 0:3]).reshape(-1, 3), input_rots=np.ascontiguousarray(tr[..., 3:7]).reshape(-1, 4),
                opt_trans=np.asarray(opt_trans, dtype=np.float32).reshape(-1, 3), opt_rots=np.asarray(opt_rots, dtype=np.float32).reshape(-1))


def items_of(plan):
    return [(it.row, it.row_prev, it.row_next, it.flags, it.alpha, it.one_minus_alpha) for it in plan.items[:plan.A]]


# ---- plain torch: the reference's per-actor sequence --------------------------------------------------------------------
def torch_quaternion_raw_multiply_theta(a, theta):
    import torch
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bz = torch.cos(theta / 2), torch.sin(theta / 2)
    return torch.stack((aw * bw - az * bz, ax * bw + ay * bz, ay * bw - ax * bz, az * bw + aw * bz), -1)


def torch_qmul(a, b):
    import torch
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def torch_slerp(p, n, alpha):
    """the geometric slerp of the contract in torch ops (what the reference takes from a quaternion library)"""
    import torch
    import torch.nn.functional as F
    ph, nh = F.normalize(p, dim=-1), F.normalize(n, dim=-1)
    r = torch_qmul(ph * ph.new_tensor([1.0, -1.0, -1.0, -1.0]), nh)
    r = torch.where(r[..., :1] < 0, -r, r)
    v = r[..., 1:]
    sv = torch.linalg.norm(v, dim=-1, keepdim=True)
    phi = torch.atan2(sv, r[..., :1])
    small = phi <= SERIES_PHI
    ew = torch.where(small, 1 - 0.5 * (alpha * phi) ** 2, torch.cos(alpha * phi))
    f = torch.where(small, alpha * (1 + (1 - alpha * alpha) * phi * phi / 6),
                    torch.sin(alpha * phi) / torch.where(small, torch.ones_like(sv), sv))
    return torch_qmul(ph, torch.cat((ew, f * v), -1))


class TorchActorPose:
    """ActorPose (actor_pose.py:12-30, :83-144) restated: the tables and the valid mask live on the device, and every
    lookup asserts on the device mask, as the reference does -- a host wait each."""

    def __init__(self, camera_tracklets, camera_timestamps, opt_trans, opt_rots, device, opt_track=True):
        import torch
        t = torch.from_numpy(np.asarray(camera_tracklets)).float().to(device)
        self.camera_timestamps = camera_timestamps
        self.valid_mask = t[..., -1].int()
        self.input_trans, self.input_rots = t[..., :3], t[..., 3:7]
        self.opt_track, self.opt_trans, self.opt_rots = opt_track, opt_trans, opt_rots

    def _trans(self, cam, f, i, lidar):
        if self.opt_track and not lidar:
            return self.input_trans[cam, f, i] + self.opt_trans[cam, f, i]
        return self.input_trans[cam, f, i]

    def _rots(self, cam, f, i, lidar):
        if self.opt_track and not lidar:
            return torch_quaternion_raw_multiply_theta(self.input_rots[cam, f, i], self.opt_rots[cam, f, i, 0])
        return self.input_rots[cam, f, i]

    def _interp(self, cam, f, i, is_val):
        return self.opt_track and is_val and f > 0 and f < self.valid_mask.shape[1] - 1 and \
            self.valid_mask[cam, f - 1, i] == 1 and self.valid_mask[cam, f + 1, i] == 1

    def _alpha(self, cam, f, timestamp):
        pre, nxt = self.camera_timestamps[cam][f - 1], self.camera_timestamps[cam][f + 1]
        return (timestamp - pre) / (nxt - pre)

    def translation(self, i, cam, f, timestamp, is_val=False, is_novel_view=False):
        assert self.valid_mask[cam, f, i] == 1, "Invalid object"
        if self._interp(cam, f, i, is_val):
            alpha = self._alpha(cam, f, timestamp)
            return alpha * self._trans(cam, f + 1, i, is_novel_view) + (1. - alpha) * self._trans(cam, f - 1, i, is_novel_view)
        return self._trans(cam, f, i, is_novel_view)

    def rotation(self, i, cam, f, timestamp, is_val=False, is_novel_view=False):
        assert self.valid_mask[cam, f, i] == 1, "Invalid object"
        if self._interp(cam, f, i, is_val):
            alpha = self._alpha(cam, f, timestamp)
            return torch_slerp(self._rots(cam, f - 1, i, is_novel_view), self._rots(cam, f + 1, i, is_novel_view), alpha)
        return self._rots(cam, f, i, is_novel_view)

    def poses(self, ids, cam, f, timestamp, **kw):
        """parse_camera's two stacks (street_gaussian_model.py:243-249) -> obj_rots [A,4], obj_trans [A,3]"""
        import torch
        return (torch.stack([self.rotation(i, cam, f, timestamp, **kw) for i in ids], dim=0),
                torch.stack([self.translation(i, cam, f, timestamp, **kw) for i in ids], dim=0))
