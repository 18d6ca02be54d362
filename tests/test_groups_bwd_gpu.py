"""rasterize_to_pixels_grouped_train (csrc/raster_groups.hip with last positions, csrc/raster_groups_bwd.hip): the forward
bit for bit against the forward-only operator, the gradients PER ROW against the float64 closed form.

Reference.  The gradient is linear in the upstream images, so

    G = RB(full lists, v_composite) + sum_k scatter_k(RB(group k's own lists, v_group_k))

with RB = oracle/raster_bwd_f64.py and group k's lists from the numpy oracle's isect_tiles on the `group_ids == k` rows (as
oracle/raster_bwd_cases.py builds the full ones); S and A are summed the same way.  absgrad is the composite's alone:
RB(full)["G"]["absgrad"], judged with the composite's S / A of means2d.  Bar, as tests/test_raster_bwd_rows_gpu.py
derives it:

    |hip - G| <= 2^-24 (K S + A)          and exactly 0 where S == 0

K = 4 K_ref, K_ref the largest ratio the float32 REPLAY of the same sum (dtype=np.float32, no kernel) reaches over all
rows, outputs and cases of this module.  Pixels that `RB.unstable_bwd` flags for the full render OR for either group's
render get zero upstream gradient in every image; their share is asserted below RC.UNSTABLE_CAP per scene (exactly 0 on
the hand-built frames).

Scenes (oracle/raster_bwd_cases.py, tile 16): ragged (partial last tile row and column), two_cameras (group_ids shared by
the cameras), the two hand-built frames of oracle/raster_edge_frames.py (a group's own lists are the full ones without
the other rows; judged under the K of the other scenes), deep_soft (long lists that never saturate), deep_hard (the composite saturates while the 20 % group keeps
going: the sets stop at different positions), street (tiles without a group-1 record); 4 and 3 channels.
Group ids: u = default_rng(7).random(N); 0 where u < 0.7, 1 where u < 0.9, else 255 (composite only).
Upstream forms: "all" = normal draws on all four images; "train" = composite colours + alphas and group_alphas[1] only,
nothing else differentiated (null pointers in the kernel); "one_group" = n_groups = 1, normal draws on all images.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gsplat_oracle as O              # noqa: E402  (checker only)
from oracle import raster_bwd_cases as RC          # noqa: E402
from oracle import raster_bwd_f64 as RB            # noqa: E402

DEV = "cuda"
SCENES = ("ragged", "two_cameras", "deep_soft", "deep_hard", "street")
EDGE_SCENES = ("edge:finite", "edge:finite129")      # oracle/raster_edge_frames.py: hand-built lists, judged under the K of SCENES
CHANNELS = (4, 3)
FORMS = ("all", "train", "one_group")
NAMES = ("means2d", "conics", "colors", "opacities", "absgrad")
GRADS = ("means2d", "conics", "colors", "opacities")


def group_ids_of(n):
    u = np.random.default_rng(7).random(n)
    return np.where(u < 0.7, 0, np.where(u < 0.9, 1, 255)).astype(np.uint8)


def make_inputs(scene, D):
    """Everything of one (scene, D): the projected scene, colours, group ids, each group's own rows and lists, the union
    of the unstable pixels and the four upstream draws (already zero at those pixels)."""
    p = dict(RC.projected(scene, 16))
    C, N = p["opacities"].shape
    W, H = p["width"], p["height"]
    rng = np.random.default_rng(5000 + 10 * (SCENES + EDGE_SCENES).index(scene) + D)
    p["colors"] = rng.uniform(0, 1, (C, N, D)).astype(np.float32)
    gids = group_ids_of(N)
    th, tw = p["isect_offsets"].shape[1:]
    un = RB.unstable_bwd(p["means2d"], p["conics"], p["colors"], p["opacities"], W, H, 16, p["isect_offsets"],
                         p["flatten_ids"])
    sub = []
    for k in (0, 1):
        rows = np.nonzero(gids == k)[0]
        if scene in EDGE_SCENES:      # hand-built lists: the group's own lists are the full ones without the other rows
            keep = np.isin(p["flatten_ids"], rows)
            offs = np.concatenate([[0], np.cumsum(keep)])[p["isect_offsets"].reshape(-1)].astype(np.int32)
            offs = offs.reshape(p["isect_offsets"].shape)
            fids = np.searchsorted(rows, p["flatten_ids"][keep]).astype(np.int32)
        else:
            _, ids, fids = O.isect_tiles(p["means2d"][:, rows], p["radii"][:, rows], p["depths"][:, rows], 16, tw, th,
                                         n_cameras=C)
            offs = O.isect_offset_encode(ids, C, tw, th)
        sub.append(dict(rows=rows, isect_offsets=offs, flatten_ids=fids))
        un = un | RB.unstable_bwd(p["means2d"][:, rows], p["conics"][:, rows], p["colors"][:, rows], p["opacities"][:, rows],
                                  W, H, 16, offs, fids)
    up = dict(rc=rng.normal(size=(C, H, W, D)), ra=rng.normal(size=(C, H, W, 1)), gc=rng.normal(size=(2, C, H, W, D)),
              ga=rng.normal(size=(2, C, H, W, 1)))
    up = {k: v.astype(np.float32) for k, v in up.items()}
    up["rc"][un] = 0.0
    up["ra"][un] = 0.0
    up["gc"][:, un] = 0.0
    up["ga"][:, un] = 0.0
    p.update(scene=scene, D=D, group_ids=gids, sub=sub, unstable=un, up=up)
    return p


def _rb(p, dtype, k=None, v_c=None, v_a=None):
    """RB on the full lists (k None) or on group k's own lists, scattered back to [C,N,*] rows."""
    if k is None:
        return RB.rasterize_bwd(p["means2d"], p["conics"], p["colors"], p["opacities"], p["width"], p["height"], 16,
                                p["isect_offsets"], p["flatten_ids"], v_c, v_a, dtype=dtype)
    g = p["sub"][k]
    rows = g["rows"]
    r = RB.rasterize_bwd(p["means2d"][:, rows], p["conics"][:, rows], p["colors"][:, rows], p["opacities"][:, rows],
                         p["width"], p["height"], 16, g["isect_offsets"], g["flatten_ids"], v_c, v_a, dtype=dtype)
    out = {}
    for part in ("G", "S", "A"):
        out[part] = {}
        for name in GRADS:
            full = np.zeros(p["opacities"].shape + r[part][name].shape[2:], np.float64)
            full[:, rows] = r[part][name]
            out[part][name] = full
    return out


def build_references(p):
    """{form: (float64 reference, float32 replay's G)} for one (scene, D).  The pieces are computed once and shared: the
    composite's by all three forms, group 0's by "all" and "one_group"."""
    up = p["up"]
    zero_c = np.zeros_like(up["gc"][1])
    pieces = {}
    for dt in (np.float64, np.float32):
        pieces[dt] = dict(full=_rb(p, dt, None, up["rc"], up["ra"]), g0=_rb(p, dt, 0, up["gc"][0], up["ga"][0]),
                          g1=_rb(p, dt, 1, up["gc"][1], up["ga"][1]), g1_alpha=_rb(p, dt, 1, zero_c, up["ga"][1]))
    forms = {"all": ("g0", "g1"), "train": ("g1_alpha",), "one_group": ("g0",)}

    def summed(dt, parts):
        full = pieces[dt]["full"]
        out = {part: {n: full[part][n].copy() for n in GRADS} for part in ("G", "S", "A")}
        for key in parts:
            for part in ("G", "S", "A"):
                for n in GRADS:
                    out[part][n] += pieces[dt][key][part][n]
        out["G"]["absgrad"] = full["G"]["absgrad"]             # the composite's terms only ...
        out["S"]["absgrad"], out["A"]["absgrad"] = full["S"]["means2d"], full["A"]["means2d"]     # ... and its scales
        return out

    refs = {form: (summed(np.float64, parts), summed(np.float32, parts)["G"]) for form, parts in forms.items()}
    refs["full_only"] = pieces[np.float64]["full"]
    return refs


@pytest.fixture(scope="module")
def table():
    """{(scene, D): (inputs, references)} and K: ONE number for the module."""
    tab, k_ref, own_of = {}, 0.0, {}
    for scene in SCENES + EDGE_SCENES:
        for D in CHANNELS:
            p = make_inputs(scene, D)
            refs = build_references(p)
            share = float(p["unstable"].mean())
            for form in FORMS:
                ref, replay = refs[form]
                rep = RC.worst_ratios(replay, ref, NAMES)
                assert all(off == 0.0 for _, off in rep.values()), (scene, D, form, rep)
                own = max(r for r, _ in rep.values())
                print(f"[replay] {scene}-D{D}-{form}: K_ref {own:.1f} ({max(rep, key=lambda k: rep[k][0])}); left out {100 * share:.3f} %")
                if scene in SCENES:           # K comes from the random scenes; the hand-built frames are judged under it
                    k_ref = max(k_ref, own)
                own_of[(scene, D)] = max(own_of.get((scene, D), 0.0), own)
            tab[(scene, D)] = (p, refs)
    print(f"[replay] K_ref over {len(SCENES) * len(CHANNELS) * len(FORMS)} cases: {k_ref:.1f}; K = {4 * k_ref:.1f}")
    assert 1.0 < k_ref < 1000.0
    K = {key: 4.0 * k_ref for key in tab}
    for key in tab:
        if key[0] in EDGE_SCENES and own_of[key] > k_ref:     # past K_ref on its own replay: that case alone gets 4x its own
            K[key] = 4.0 * own_of[key]
            print(f"[replay] {key}: own ratio {own_of[key]:.1f} > K_ref {k_ref:.1f}: judged under {K[key]:.1f}")
    K[None] = 4.0 * k_ref
    return tab, K


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _hip(p, form, absgrad=True, group_ids=None):
    """forward + backward of the operator under test -> ({output: numpy gradient}, the four images, the means2d leaf)."""
    from street_crafter_amd.groups import rasterize_to_pixels_grouped_train
    src = [_t(p[k]).requires_grad_(True) for k in GRADS]
    n_groups = 1 if form == "one_group" else 2
    gids = _t(p["group_ids"] if group_ids is None else group_ids, torch.uint8)
    imgs = rasterize_to_pixels_grouped_train(*src, p["width"], p["height"], 16, _t(p["isect_offsets"], torch.int32),
                                             _t(p["flatten_ids"], torch.int32), gids, n_groups=n_groups, absgrad=absgrad)
    rc, ra, gc, ga = imgs
    up = {k: _t(v) for k, v in p["up"].items()}
    loss = (rc * up["rc"]).sum() + (ra * up["ra"]).sum()
    if form == "train":
        loss = loss + (ga[1] * up["ga"][1]).sum()
    else:
        loss = loss + (gc * up["gc"][:n_groups]).sum() + (ga * up["ga"][:n_groups]).sum()
    loss.backward()
    torch.cuda.synchronize()
    out = {k: t.grad.cpu().numpy() for k, t in zip(GRADS, src)}
    if absgrad:
        out["absgrad"] = src[0].absgrad.cpu().numpy()
    return out, tuple(t.detach() for t in imgs), src[0]


def _judge(tag, got, ref, K, names=NAMES, rows=None):
    if rows is not None:
        got = {k: got[k][:, rows] for k in names}
        ref = {part: {k: ref[part][k][:, rows] for k in names} for part in ("G", "S", "A")}
    worst = RC.worst_ratios(got, ref, names)
    print(f"[hip] {tag}: " + ", ".join(f"{k} {r:.1f}" + (f" (|x| {off:.1e} where S = 0)" if off else "") for k, (r, off) in worst.items())
          + f"; bar {K:.1f}")
    for k, (r, off) in worst.items():
        assert np.isfinite(got[k]).all(), (tag, k)
        assert off == 0.0, (tag, k, off)
        assert r <= K, (tag, k, r, K)


@pytest.mark.parametrize("fast_on", [True, False])
@pytest.mark.parametrize("scene,D", [("ragged", 4), ("deep_hard", 3), ("two_cameras", 4)])
def test_forward_equals_the_forward_only_operator_on_both_binding_routes(table, scene, D, fast_on):
    from street_crafter_amd import _ctypes_binding, _lib
    from street_crafter_amd.groups import rasterize_to_pixels_grouped, rasterize_to_pixels_grouped_train
    p = table[0][(scene, D)][0]
    args = [_t(p[k]) for k in GRADS]
    tail = (p["width"], p["height"], 16, _t(p["isect_offsets"], torch.int32), _t(p["flatten_ids"], torch.int32),
            _t(p["group_ids"], torch.uint8))
    prev = _lib.set_fast_binding(fast_on)
    try:
        assert _lib.binding() is (_lib.fast() if fast_on else _ctypes_binding)
        for n_groups in (2, 1):
            got = rasterize_to_pixels_grouped_train(*[a.clone().requires_grad_(True) for a in args], *tail, n_groups=n_groups)
            with torch.no_grad():
                want = rasterize_to_pixels_grouped(*args, *tail, n_groups=n_groups)
                plain = rasterize_to_pixels_grouped_train(*args, *tail, n_groups=n_groups)      # nothing requires grad
            assert all(g.requires_grad for g in got) and not any(x.requires_grad for x in plain)
            for g, w, x in zip(got, want, plain):
                assert g.shape == w.shape and torch.equal(g.detach(), w) and torch.equal(x, w)
    finally:
        _lib.set_fast_binding(prev)
    assert bool((want[3][0] > 0).any())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("D", CHANNELS)
@pytest.mark.parametrize("scene", SCENES + EDGE_SCENES)
def test_gradient_rows_against_the_float64_closed_form(table, scene, D, form):
    tab, K = table
    K = K[(scene, D)]
    p, refs = tab[(scene, D)]
    ref = refs[form][0]
    assert float(p["unstable"].mean()) < RC.UNSTABLE_CAP, (scene, 100 * float(p["unstable"].mean()))
    if scene in EDGE_SCENES:              # hand-built: no decision near a threshold, in the full render or in a group's own
        assert float(p["unstable"].mean()) == 0.0, scene
    assert (ref["S"]["colors"] > 0).any() and np.abs(ref["G"]["means2d"]).max() > 0            # the case is not empty
    got, imgs, _ = _hip(p, form)
    _judge(f"{scene}-D{D}-{form}", got, ref, K)
    # a Gaussian of no group (id 255; with one group also id 1) has the composite's gradient and nothing else
    alone = np.nonzero(p["group_ids"] >= (1 if form == "one_group" else 2))[0]
    assert alone.size > 0
    _judge(f"{scene}-D{D}-{form} rows of no group", got, refs["full_only"], K, names=GRADS, rows=alone)
    if scene == "deep_hard" and form != "one_group":
        # the sets stop at different positions: the 20 % group goes on where the composite is opaque
        ra, ga = imgs[1].cpu().numpy(), imgs[3].cpu().numpy()
        assert ((ra[..., 0] > 0.999) & (ga[1][..., 0] < 0.99) & (ga[1][..., 0] > 0)).any()
    if scene == "street" and form != "one_group":
        g1 = p["sub"][1]
        counts = np.diff(np.append(g1["isect_offsets"].reshape(-1), g1["flatten_ids"].size))
        full = np.diff(np.append(p["isect_offsets"].reshape(-1), p["flatten_ids"].size))
        assert ((counts == 0) & (full > 0)).any()             # tiles that hold no group-1 record


def test_no_intersections_give_zero_gradients(table):
    p = dict(table[0][("ragged", 4)][0])
    p["isect_offsets"] = np.zeros_like(p["isect_offsets"])
    p["flatten_ids"] = np.zeros(0, np.int32)
    got, imgs, _ = _hip(p, "all")
    for k in NAMES:
        assert got[k].shape[:2] == p["opacities"].shape and not got[k].any(), k
    assert not any(bool(t.any()) for t in imgs)


def test_an_empty_group_adds_nothing(table):
    """group 1 has no Gaussian: its images are zero and the gradient is the composite's plus group 0's."""
    tab, K = table
    K = K[None]
    p, refs = tab[("ragged", 4)]
    gids = np.where(p["group_ids"] == 1, 255, p["group_ids"]).astype(np.uint8)
    got, imgs, _ = _hip(p, "all", group_ids=gids)
    assert not imgs[2][1].any() and not imgs[3][1].any()
    _judge("ragged-D4 group 1 empty", got, refs["one_group"][0], K)


def test_absgrad_off_attaches_nothing(table):
    p = table[0][("ragged", 3)][0]
    got, _, leaf = _hip(p, "train", absgrad=False)
    assert not hasattr(leaf, "absgrad") and "absgrad" not in got and np.abs(got["means2d"]).max() > 0


def test_a_second_backward_is_within_the_reordering_of_the_atomics(table):
    """Two runs add the same per-tile partial sums into a row in another order.  A row gets one partial sum per tile list
    it is in (n_g of them: the sets are summed before the atomic), their magnitudes add up to at most S, so one order is
    within (n_g - 1) 2^-24 S of the exact sum and two orders are within 2 n_g 2^-24 S of each other
    (tests/test_raster_bwd_rows_gpu.py::test_python_and_compiled_autograd_routes_give_the_same_rows)."""
    p, refs = table[0][("two_cameras", 4)]
    first, second = _hip(p, "all")[0], _hip(p, "all")[0]
    n_g = np.bincount(p["flatten_ids"], minlength=p["opacities"].size).reshape(p["opacities"].shape).astype(np.float64)
    for k in NAMES:
        a, b = first[k].astype(np.float64), second[k].astype(np.float64)
        S = refs["all"][0]["S"][k]
        bound = RB.EPS24 * 2.0 * n_g.reshape(n_g.shape + (1,) * (S.ndim - 2)) * S
        worst = float((np.abs(a - b) / np.where(bound > 0, bound, 1.0)).max())
        print(f"[again] two_cameras-D4 {k}: largest |first - second| / (2 n 2^-24 S) = {worst:.3f}")
        assert (np.abs(a - b) <= bound).all(), (k, worst)
