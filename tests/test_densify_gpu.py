"""GPU checks of the fused densify-and-prune (csrc/densify.hip through street_crafter_amd/densify.py) against the torch
restatement of the reference's clone / split / prune sequence in tests/test_densify_cpu.py.

Inputs are generated so that, in float64, no decision quantity lies within relative MARGIN = 1e-4 of its threshold (g,
max s of every candidate, sigmoid(o), the sphere distance, the box samples, max_radii): rows that come too close have
their noise redrawn, and `assert_margins` asserts the condition on the finished inputs before they are used.  fp32
rounding of exp, sigmoid and the norm is orders of magnitude below that, so no row is excluded from any comparison:
src_row, slot, n' and the six counters are EQUAL to the restatement's, every copied value and every moment is
bit-identical (torch.equal) to its source row.

The children's values are judged against the float64 restatement with the bound 2^-24 K A.  K counts, to first order,
the fp32 roundings of the kernel's own expression (u = 2^-24 is the relative error of one rounding; the ulp bounds are
those of the HIP math API: expf 1 ulp, logf 1 ulp = 2u each; sqrtf and division correctly rounded, u):
  xyz'_r = x_r + sum_j R_rj (noise_j s_j),  A = |x_r| + sum_j |noise_j| s_j
    s_j = expf(.)                              2u                   d_j = noise_j s_j                      3u |d_j|
    |q|^2: 4 squares + 3 adds of positives     4u                   |q| = sqrtf                            4u/2 + u = 3u
    q / |q|                                    4u per component     a product of two components            9u
    off-diagonal 2 (ab -+ cd): |ab| + |cd| <= 1/2, so 9u/2 + u/2 (the difference), doubled                10u absolute
    diagonal 1 - 2 (aa + bb): aa + bb <= 1: 9u + u, doubled, + u for the subtraction (result <= 1)         21u absolute
    R_rj d_j with |R_rj| <= 1: (21 + 3 + 1) u |d_j|                                                        25u |d_j|
    three adds whose partial sums are bounded by A                                                         3u A
  K_XYZ = 25 + 3 = 28, + 1 for all second-order terms (each below 2^-18 of the first-order sum) = 29.
  scaling'_j = logf(s_j / 1.6f),  A = max(1, |scaling'_j|)
    s_j 2u, the division u: the argument is off by 3u relative, i.e. the logarithm by 3u absolute; logf 2u |scaling'|
  K_SCALING = 3 + 2 = 5, + 1 for the second-order terms = 6.
A fused multiply-add in place of a product and a sum removes roundings, never adds one.  The fp32 restatement (torch's own
exp / log / bmm in fp32: the same operations in another order) must lie inside the same bounds: that is the check on K.
"""
from types import SimpleNamespace

import pytest
import torch

from test_densify_cpu import COUNTERS, SPLIT_DIV, U, quat_matrix, restate
from test_optim_cpu import adam_judge, make_grad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-4
K_XYZ, K_SCALING = 29, 6
EXTENT, PERCENT_DENSE, PERCENT_BIG = 10.0, 0.01, 0.1          # clone / split at max s = 0.1, big above 1.0
MAX_GRAD, MIN_OPACITY, MAX_SCREEN = 0.0002, 0.05, 20.0
SPHERE = ((0.5, -1.0, 2.0), 5.0)
BOX = ((-4.0, -3.0, -5.0), (4.0, 5.0, 3.0))
NAMES = ("xyz", "scaling", "rotation", "opacity", "f_dc", "f_rest", "semantic")


@pytest.fixture(scope="module")
def D():
    from street_crafter_amd import _lib, densify
    _lib.load()
    return densify


def _block():
    from street_crafter_amd import _lib
    try:
        return _lib.load().sc_densify_scan_block()
    except Exception:                                   # collected without the library: the fixture fails the tests
        return 256


B = _block()
SIZES = [0, 1, 63, 64, 65, 2 * B + 1, 3 * B + 5]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _pick(gen, n, ranges, weights):
    """log-uniform values from the interval ranges[k] chosen with probability weights[k]"""
    which = torch.multinomial(torch.tensor(weights, dtype=torch.float64), n, replacement=True, generator=gen) if n else \
        torch.zeros(0, dtype=torch.long)
    lo = torch.tensor([r[0] for r in ranges], dtype=torch.float64)[which]
    hi = torch.tensor([r[1] for r in ranges], dtype=torch.float64)[which]
    return torch.exp(torch.log(lo) + torch.rand(n, generator=gen, dtype=torch.float64) * (torch.log(hi) - torch.log(lo)))


def make_case(n, seed, mode="mixed", region=None, use_abs=False, rest=45, sem=5, stateless=()):
    """-> namespace(tensors, moments, acc, denom, max_radii, split_noise, box_noise, cfg), everything fp32 on the CPU.
    mode: none | clone | split | pruned | below | big | screen | mixed (which rows are selected and why rows are pruned)."""
    gen = torch.Generator().manual_seed(seed)
    hot_w = {"none": (1, 0), "clone": (0, 1), "split": (0, 1)}.get(mode, (1, 1))
    # max s of a row: far below / above the clone-split threshold 0.1; above 1.0 big; between 1.0 and 1.6 a parent that
    # is not big has children that are not either, above 1.7 its children (s / 1.6) are big too
    size_r = [(0.02, 0.09), (0.12, 0.9), (1.1, 1.5), (1.7, 3.0)]
    size_w = {"none": (1, 1, 0, 0), "clone": (1, 0, 0, 0), "split": (0, 1, 0, 0), "below": (1, 1, 0, 0),
              "screen": (1, 1, 0, 0), "pruned": (1, 1, 1, 1)}.get(mode, (2, 2, 1, 1))
    low_op = {"pruned": 1.0, "below": 0.4, "mixed": 0.3}.get(mode, 0.0)
    big_r = {"screen": 0.4, "mixed": 0.3}.get(mode, 0.0)
    smax = _pick(gen, n, size_r, size_w)
    s = smax[:, None] * (0.3 + 0.7 * torch.rand(n, 3, generator=gen, dtype=torch.float64))
    if n:
        s[torch.arange(n), torch.randint(0, 3, (n,), generator=gen)] = smax
    hot = torch.multinomial(torch.tensor(hot_w, dtype=torch.float64), n, replacement=True, generator=gen).bool() if n \
        else torch.zeros(0, dtype=torch.bool)
    denom = torch.randint(1 if mode in ("clone", "split") else 0, 5, (n,), generator=gen).double()   # 0: never seen
    g = torch.where(hot, _pick(gen, n, [(3.0, 50.0)], [1.0]), _pick(gen, n, [(0.01, 0.3)], [1.0])) * MAX_GRAD
    acc = torch.stack((g * denom, _pick(gen, n, [(0.01, 0.3)], [1.0]) * MAX_GRAD * denom), dim=1)   # 0 / 0 -> NaN -> cold
    if use_abs:
        acc = acc.flip(1)
    low = torch.rand(n, generator=gen) < low_op
    opacity = torch.where(low, -6.0 + 2.0 * torch.rand(n, generator=gen), -1.0 + 4.0 * torch.rand(n, generator=gen))
    max_radii = torch.where(torch.rand(n, generator=gen) < big_r, 25.0 + 10 * torch.rand(n, generator=gen),
                            15.0 * torch.rand(n, generator=gen))
    # positions: inside or outside the sphere, never near its surface (children move: they are repaired below)
    direction = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=torch.float64), dim=1)
    radius = torch.where(torch.rand(n, generator=gen) < 0.5, 0.5 + 4.0 * torch.rand(n, generator=gen, dtype=torch.float64),
                         5.5 + 3.5 * torch.rand(n, generator=gen, dtype=torch.float64))
    xyz = torch.tensor(SPHERE[0], dtype=torch.float64) + direction * radius[:, None]
    f = lambda t: t.to(torch.float32).contiguous()                                          # noqa: E731
    tensors = {"xyz": f(xyz), "scaling": f(torch.log(s)), "rotation": f(torch.randn(n, 4, generator=gen) * 1.7),
               "opacity": f(opacity)[:, None], "f_dc": f(torch.randn(n, 1, 3, generator=gen)),
               "f_rest": f(torch.randn(n, rest // 3, 3, generator=gen)), "semantic": f(torch.randn(n, sem, generator=gen))}
    moments = {k: None if k in stateless else (f(torch.randn(v.shape, generator=gen)), f(torch.rand(v.shape, generator=gen)))
               for k, v in tensors.items()}
    cfg = dict(max_grad=MAX_GRAD, use_abs=use_abs, extent=EXTENT, percent_dense=PERCENT_DENSE, min_opacity=MIN_OPACITY,
               prune_big_points=mode in ("big", "mixed", "pruned") or region is not None, percent_big_ws=PERCENT_BIG,
               max_screen_size=MAX_SCREEN if mode in ("screen", "mixed") else None,
               sphere=SPHERE if region == "sphere" else None, box=BOX if region == "box" else None)
    case = SimpleNamespace()
    case.tensors, case.moments, case.cfg = tensors, moments, cfg
    case.acc, case.denom, case.max_radii = f(acc), f(denom)[:, None], f(max_radii)
    case.split_noise = torch.randn(2, n, 3, generator=gen)
    case.box_noise = torch.randn(4, n, 2, 3, generator=gen)
    for _ in range(100):                          # redraw the noise of the rows whose candidates come too close
        close = ~margins(case)[1]
        if not close.any():
            break
        k = int(close.sum())
        case.split_noise[:, close] = torch.randn(2, k, 3, generator=gen)
        case.box_noise[:, close] = torch.randn(4, k, 2, 3, generator=gen)
    return case


def margins(case):
    """Every decision quantity of every candidate, in float64 from the fp32 inputs -> (smallest relative distance to its
    threshold, per-row mask 'all far enough')."""
    T = {k: v.double() for k, v in case.tensors.items()}
    cfg, n = case.cfg, case.tensors["xyz"].shape[0]
    ok = torch.ones(n, dtype=torch.bool)
    worst = [float("inf")]

    def far(q, thr):
        if n == 0:
            return ok
        d = (q - thr).abs() / abs(thr)
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d).reshape(n, -1)
        if d.numel():
            worst[0] = min(worst[0], float(d.min()))
        return (d > MARGIN).all(dim=1)

    g = case.acc.double()[:, 1 if cfg["use_abs"] else 0] / case.denom.double()[:, 0]
    g[g.isnan()] = 0.0
    ok &= far(g, cfg["max_grad"])
    s = torch.exp(T["scaling"])
    s_child = torch.exp(torch.log(s / SPLIT_DIV))
    ok &= far(s.max(dim=1).values, cfg["percent_dense"] * cfg["extent"])
    ok &= far(torch.sigmoid(T["opacity"]), cfg["min_opacity"])
    ok &= far(case.max_radii.double(), MAX_SCREEN)
    R = quat_matrix(T["rotation"])
    child = T["xyz"][None] + torch.einsum("nij,knj->kni", R, case.split_noise.double() * s[None])     # [2,n,3]
    cands = [(T["xyz"], s), (T["xyz"], s), (child[0], s_child), (child[1], s_child)]                # by slot
    for slot, (p, sc) in enumerate(cands):
        ok &= far(sc.max(dim=1).values, cfg["extent"] * cfg["percent_big_ws"])
        ok &= far(torch.linalg.norm(p - torch.tensor(SPHERE[0], dtype=torch.float64), dim=1), SPHERE[1])
        pts = p[:, None] + torch.einsum("nij,nmj->nmi", R, case.box_noise[slot].double() * sc[:, None])
        for d in range(3):
            ok &= far(pts[:, :, d], BOX[0][d]) & far(pts[:, :, d], BOX[1][d])
    return worst[0], ok


def assert_margins(case):
    worst, ok = margins(case)
    assert bool(ok.all()) and worst > MARGIN, f"a decision quantity lies within {MARGIN} of its threshold ({worst:.3e})"


# ---- running and judging ------------------------------------------------------------------------------------------------------
def build_job(D, case, cls=None, explicit_noise=True):
    from street_crafter_amd import optim
    params = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in case.tensors.items()}
    opt = (cls or optim.Adam)([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    for k, p in params.items():
        if case.moments[k] is not None:
            opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": case.moments[k][0].clone().to(DEV),
                            "exp_avg_sq": case.moments[k][1].clone().to(DEV)}
    cfg = case.cfg
    job = D.DensifyJob(
        optimizer=opt, xyz_gradient_accum=case.acc.to(DEV), denom=case.denom.to(DEV), max_radii2D=case.max_radii.to(DEV),
        max_grad=cfg["max_grad"], extent=cfg["extent"], min_opacity=cfg["min_opacity"], percent_dense=cfg["percent_dense"],
        use_abs=cfg["use_abs"], prune_big_points=cfg["prune_big_points"], percent_big_ws=cfg["percent_big_ws"],
        max_screen_size=cfg["max_screen_size"], sphere=cfg["sphere"], box=cfg["box"],
        split_noise=case.split_noise.to(DEV) if explicit_noise else None,
        box_noise=case.box_noise.to(DEV) if explicit_noise and cfg["box"] is not None else None)
    return job, opt, params


def judge(case, res, opt, old_params):
    """One job's result against the float64 and the float32 restatement.  -> (worst error / bound of xyz', scaling')"""
    ref = {dt: restate(case.tensors, case.moments, case.acc, case.denom, case.max_radii, case.cfg, case.split_noise,
                       case.box_noise, dtype=dt) for dt in (torch.float64, torch.float32)}
    r64, r32 = ref[torch.float64], ref[torch.float32]
    src, slot = res.src_row.cpu().long(), res.slot.cpu().long()
    for r in (r64, r32):
        assert res.n_out == r.n_out and res.scalar_dict == r.counters
        assert torch.equal(src, r.src_row) and torch.equal(slot, r.slot)
    assert tuple(res.scalar_dict) == COUNTERS
    n_out, copied = res.n_out, slot < 2
    by_name = {g["name"]: g for g in opt.param_groups}
    for name in NAMES:
        old, new = case.tensors[name], res.params[name]
        assert by_name[name]["params"][0] is new and isinstance(new, torch.nn.Parameter) and new.requires_grad
        assert new.shape == (n_out, *old.shape[1:]) and new.is_contiguous() and new.device.type == "cuda"
        assert old_params[name] not in opt.state
        got = new.detach().cpu()
        rows = copied if name in ("xyz", "scaling") else torch.ones(n_out, dtype=torch.bool)
        assert torch.equal(got[rows], old[src][rows]), name                              # every copied value, bit for bit
        if case.moments[name] is None:
            assert len(opt.state.get(new, {})) == 0, name                                 # still no state
            continue
        state = opt.state[new]
        assert set(state) == {"step", "exp_avg", "exp_avg_sq"} and float(state["step"]) == 3.0
        keep = (slot == 0).reshape(-1, *([1] * (old.dim() - 1))).to(old.dtype)
        for key, m_old in zip(("exp_avg", "exp_avg_sq"), case.moments[name]):
            assert state[key].shape == new.shape and state[key].is_contiguous()
            assert torch.equal(state[key].cpu(), m_old[src] * keep), (name, key)
    for t, shape in ((res.xyz_gradient_accum, (n_out, 2)), (res.denom, (n_out, 1)), (res.max_radii2D, (n_out,))):
        assert t.shape == shape and t.dtype == torch.float32 and not t.any()
    # the children, against float64
    kids = ~copied
    ratios = [0.0, 0.0]
    if kids.any():
        parent = src[kids]
        s = torch.exp(case.tensors["scaling"].double()[parent])
        noise = case.split_noise.double()[slot[kids] - 2, parent]
        A = case.tensors["xyz"].double()[parent].abs() + (noise.abs() * s).sum(dim=1, keepdim=True)
        want_x, want_s = r64.tensors["xyz"][kids], r64.tensors["scaling"][kids]
        As = torch.clamp(want_s.abs(), min=1.0)
        for who, x, sc in (("kernel", res.params["xyz"].detach().cpu()[kids], res.params["scaling"].detach().cpu()[kids]),
                           ("fp32 restatement", r32.tensors["xyz"][kids], r32.tensors["scaling"][kids])):
            rx = float(((x.double() - want_x).abs() / (U * K_XYZ * A)).max())
            rs = float(((sc.double() - want_s).abs() / (U * K_SCALING * As)).max())
            print(f"{who}: worst error / bound: xyz' {rx:.3f}, scaling' {rs:.3f} over {int(kids.sum())} children")
            assert rx <= 1.0 and rs <= 1.0, (who, rx, rs)
            if who == "kernel":
                ratios = [rx, rs]
    return ratios


def run_case(D, case, **kw):
    assert_margins(case)
    job, opt, params = build_job(D, case, **kw)
    res = D.densify_and_prune_many([job])[0]
    judge(case, res, opt, params)
    return res, opt


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_scan_block(D, n):
    """One job of every size at which the plan changes path (a wave, a block, several blocks with a ragged last one), mixed
    population with every prune reason; f_rest width 45 / 0 and semantic width 0 / 5 alternate."""
    wide = SIZES.index(n) % 2 == 0
    res, _ = run_case(D, make_case(n, 100 + n, "mixed", rest=45 if wide else 0, sem=0 if wide else 5))
    print(f"n = {n}: n' = {res.n_out}, {res.scalar_dict}")


@pytest.mark.parametrize("mode", ["none", "clone", "split", "pruned", "below", "big", "screen", "mixed"])
def test_populations(D, mode):
    n = 2 * B + 1
    case = make_case(n, 7, mode)
    res, opt = run_case(D, case)
    c = res.scalar_dict
    print(f"{mode}: n' = {res.n_out}, {c}")
    if mode == "none":                       # nothing selected: every tensor and moment bit-identical, step untouched
        assert res.n_out == n and c["points_clone"] == c["points_split"] == c["points_pruned"] == 0
        for name in NAMES:
            assert torch.equal(res.params[name].detach().cpu(), case.tensors[name])
            assert torch.equal(opt.state[res.params[name]]["exp_avg"].cpu(), case.moments[name][0])
            assert torch.equal(opt.state[res.params[name]]["exp_avg_sq"].cpu(), case.moments[name][1])
            assert float(opt.state[res.params[name]]["step"]) == 3.0
    elif mode == "clone":
        assert c["points_clone"] == n and c["points_split"] == 0 and res.n_out == 2 * n
    elif mode == "split":
        assert c["points_split"] == n and c["points_clone"] == 0 and res.n_out == 2 * n
    elif mode == "pruned":
        assert res.n_out == 0 and c["points_pruned"] == c["points_below_min_opacity"] > 0
    elif mode == "below":
        assert 0 < c["points_pruned"] == c["points_below_min_opacity"] and c["points_big_ws"] == 0
    elif mode == "big":
        assert 0 < c["points_pruned"] == c["points_big_ws"] and c["points_below_min_opacity"] == 0
    elif mode == "screen":
        assert c["points_pruned"] > 0 and c["points_below_min_opacity"] == c["points_big_ws"] == 0
    else:
        assert min(c.values()) > 0 and c["points_pruned"] > max(c["points_below_min_opacity"], c["points_big_ws"])


@pytest.mark.parametrize("region,use_abs", [("sphere", False), ("box", False), ("sphere", True), (None, True)])
def test_regions_and_the_abs_column(D, region, use_abs):
    n = 2 * B + 1
    case = make_case(n, 11, "mixed", region=region, use_abs=use_abs)
    res, _ = run_case(D, case)
    if region == "sphere":                   # rows on both sides of the radius, and the rule made a difference
        d = torch.linalg.norm(case.tensors["xyz"].double() - torch.tensor(SPHERE[0], dtype=torch.float64), dim=1)
        assert (d < SPHERE[1]).any() and (d > SPHERE[1]).any()
        plain = restate(case.tensors, case.moments, case.acc, case.denom, case.max_radii, dict(case.cfg, sphere=None),
                        case.split_noise)
        assert plain.counters["points_big_ws"] > res.scalar_dict["points_big_ws"] > 0
    if region == "box":
        plain = restate(case.tensors, case.moments, case.acc, case.denom, case.max_radii, dict(case.cfg, box=None),
                        case.split_noise)
        assert plain.n_out > res.n_out > 0
    print(f"{region}, use_abs {use_abs}: n' = {res.n_out}, {res.scalar_dict}")


def test_groups_without_state_and_torch_adam(D):
    """Two groups whose state is still empty get only the parameter; torch.optim.Adam is handled like optim.Adam."""
    case = make_case(B + 3, 13, "mixed", stateless=("f_rest", "opacity"))
    run_case(D, case)
    run_case(D, make_case(65, 14, "mixed"), cls=torch.optim.Adam)


def test_seventy_jobs_in_one_call(D):
    """70 tiny jobs (more than fit one launch table), an empty one in the middle, every region kind: one call."""
    from street_crafter_amd import _lib
    assert 70 > 2 * _lib.load().sc_densify_max_jobs()
    cases = []
    for k in range(70):
        n = 0 if k == 35 else 1 + (7 * k) % 23
        cases.append(make_case(n, 500 + k, "mixed", region=(None, "sphere", "box")[k % 3], use_abs=k % 2 == 1,
                               rest=(45, 0)[k % 2], sem=(0, 5)[k % 2]))
    for case in cases:
        assert_margins(case)
    built = [build_job(D, case) for case in cases]
    results = D.densify_and_prune_many([b[0] for b in built])
    assert len(results) == 70 and results[35].n_out == 0 and results[35].scalar_dict["points_total"] == 0
    for case, res, (_, opt, params) in zip(cases, results, built):
        judge(case, res, opt, params)
    assert sum(r.scalar_dict["points_clone"] for r in results) > 0 and sum(r.scalar_dict["points_split"] for r in results) > 0


def _everything(res, opt):
    out = [res.src_row, res.slot]
    for name in NAMES:
        p = res.params[name]
        out += [p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]]
    return [t.cpu().contiguous().view(torch.uint8) for t in out], res.scalar_dict


def test_both_host_routes_and_two_runs_are_bit_identical(D):
    from street_crafter_amd import _lib
    case = make_case(3 * B + 5, 21, "mixed", region="box")
    assert_margins(case)
    runs = []
    for fast in (True, False, True):
        prev = _lib.set_fast_binding(fast)
        try:
            job, opt, _ = build_job(D, case)
            runs.append(_everything(D.densify_and_prune_many([job])[0], opt))
        finally:
            _lib.set_fast_binding(prev)
    for other in runs[1:]:
        assert other[1] == runs[0][1]
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], other[0]))


def test_drawn_noise_follows_the_generator(D):
    """Without noise in the job it is drawn from `generator`: the same seed gives the same result, and the layout is the
    one the restatement gives for that noise (children's values: see judge)."""
    case = make_case(B + 1, 31, "split")
    outs = []
    for _ in range(2):
        job, opt, _ = build_job(D, case, explicit_noise=False)
        gen = torch.Generator(device=DEV).manual_seed(5)
        outs.append(_everything(D.densify_and_prune_many([job], generator=gen)[0], opt))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][0], outs[1][0]))
    noise = torch.randn((2, B + 1, 3), generator=torch.Generator(device=DEV).manual_seed(5), device=DEV).cpu()
    job, opt, _ = build_job(D, case, explicit_noise=False)
    res = D.densify_and_prune_many([job], generator=torch.Generator(device=DEV).manual_seed(5))[0]
    want = restate(case.tensors, case.moments, case.acc, case.denom, case.max_radii, case.cfg, noise, dtype=torch.float64)
    assert res.n_out == want.n_out == 2 * (B + 1)
    err = (res.params["xyz"].detach().cpu().double() - want.tensors["xyz"]).abs().max()
    assert float(err) < 1e-4, float(err)          # (the drawn noise was used; the bound itself is judged with given noise)


def test_adam_steps_on_the_new_parameters(D):
    """optim.step_many on the new parameters with fresh gradients: judged per element like tests/test_optim_gpu.py (4u
    bounds against float64 from the state before the step), next to torch.optim.Adam on a copy of parameters and state."""
    from street_crafter_amd import optim
    case = make_case(2 * B + 1, 41, "mixed", stateless=("semantic",))
    job, opt, _ = build_job(D, case)
    res = D.densify_and_prune_many([job])[0]
    betas, eps = opt.defaults["betas"], opt.defaults["eps"]
    twin_params, before = {}, {}
    for k, (name, p) in enumerate(res.params.items()):
        p.grad = make_grad(p.shape, 1e-2, 900 + k, device=DEV)
        st = opt.state.get(p)
        m0 = st["exp_avg"].clone() if st else torch.zeros_like(p)
        v0 = st["exp_avg_sq"].clone() if st else torch.zeros_like(p)
        before[name] = (p.detach().clone(), p.grad.clone(), m0, v0, float(st["step"]) if st else 0.0)
        twin_params[name] = torch.nn.Parameter(p.detach().clone())
        twin_params[name].grad = p.grad.clone()
    twin = torch.optim.Adam([{"params": [p], "lr": 1e-3, "name": k} for k, p in twin_params.items()], lr=0.0, eps=eps,
                            betas=betas)
    for name, p in twin_params.items():
        if before[name][4]:
            twin.state[p] = {"step": torch.tensor(before[name][4]), "exp_avg": before[name][2].clone(),
                             "exp_avg_sq": before[name][3].clone()}
    optim.step_many([opt])
    twin.step()
    for name, p in res.params.items():
        p0, g, m0, v0, t0 = before[name]
        st = opt.state[p]
        assert float(st["step"]) == t0 + 1
        r = adam_judge((p0, g, m0, v0), (p.detach(), st["exp_avg"], st["exp_avg_sq"]), 1e-3, betas, eps, t0 + 1)
        assert max(r) <= 1.0, (name, r)
        tp = twin_params[name].detach()
        rt = adam_judge((p0, g, m0, v0), (tp, twin.state[twin_params[name]]["exp_avg"],
                                          twin.state[twin_params[name]]["exp_avg_sq"]), 1e-3, betas, eps, t0 + 1)
        # both lie within their ratio x 4u (|p64| + |U64|) of the same float64 step
        scale = tp.abs().double() + (p0 - tp).abs().double()
        assert bool(((p.detach() - tp).abs().double() <= (r[2] + rt[2]) * 4 * U * scale * 1.001 + 1e-45).all()), name
        print(f"{name}: error / bound m, v, p = {r[0]:.3f} {r[1]:.3f} {r[2]:.3f}; torch.optim.Adam p {rt[2]:.3f}")
