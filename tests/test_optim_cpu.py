"""No-GPU checks of the training tail (csrc/optim.hip, street_crafter_amd/optim.py, densify_stats.accumulate_fused), and
the float64 references and input builders that tests/test_optim_gpu.py and tests/test_densify_stats_gpu.py import.

Adam reference.  Staged, so that cancellation in one stage cannot hide an error in the next: from the fp32 (p, g, m, v)
before a step, m64 and v64 in double; from the fp32 m', v' UNDER JUDGEMENT, the update U64 and p64 = p - U64 in double.
The constants are the fp32 values the kernel receives (1 - b1, b2, 1 - b2, eps, step_size, bias2_sqrt).  With u = 2^-24:

    |m' - m64| <= 4u (|m| + |g|)      |v' - v64| <= 4u (v + g^2)      |p' - p64| <= 4u (|p64| + |U64|)

The factor 4 covers the handful of roundings of each stage.  The bounds assume fp32's relative precision, i.e. results in
the normal range: (1 - b2) g^2 for |g| = 1e-20 is 1e-43, where fp32's spacing is 1.4e-45 (a relative 1e-2), so no fp32
second moment can meet the v bound for such a gradient over v = 0.  Gradients of that size are therefore judged over
moments that a normal-sized gradient has already filled, as they are in training; the bounds themselves are as stated.
test_torch_adam_stays_inside_the_bounds holds torch's own fp32 Adam (foreach and single-tensor) to the same bounds, so
the reference and the bounds are themselves tested.

Densification statistics.  stats_case() builds the inputs of every case of the GPU test; stats_f64() evaluates the torch
mirror's expression (DensificationStats.add_densification_stats) in float64; the bound per accumulator entry is
4u (acc_before + norm64).  test_mirror_stays_inside_the_stats_bound holds the torch mirror itself to it on those inputs.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -24
ADAM_LENGTHS = [0, 1, 3, 4, 5, 255, 256, 257, 4099]
BIG = 1_048_579


# ---- Adam: float64 reference ------------------------------------------------------------------------------------
def adam_constants(lr, betas, t):
    """step_size, bias2_sqrt in double, as torch's _single_tensor_adam computes them."""
    b1, b2 = betas
    return lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5


def _f32(x):
    return float(np.float32(x))


def _ratio(err, scale):
    """max over elements of err / (4u scale); an entry with scale 0 must have err 0 (-> 0, else inf)."""
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / (4 * U * scale), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def adam_judge(before, after, lr, betas, eps, t):
    """before = (p, g, m, v), after = (p', m', v'): fp32 tensors or arrays.  -> the three ratios error / bound (<= 1
    passes) of the module docstring, for the step with count t (after the increment)."""
    p, g, m, v = (np.asarray(torch.as_tensor(x).detach().cpu().numpy(), dtype=np.float64).ravel() for x in before)
    p2, m2, v2 = (np.asarray(torch.as_tensor(x).detach().cpu().numpy(), dtype=np.float64).ravel() for x in after)
    step_size, bias2_sqrt = adam_constants(lr, betas, t)
    omb1, b2, omb2 = _f32(1.0 - betas[0]), _f32(betas[1]), _f32(1.0 - betas[1])
    m64 = m + omb1 * (g - m)
    v64 = b2 * v + omb2 * g * g
    U64 = _f32(step_size) * m2 / (np.sqrt(v2) / _f32(bias2_sqrt) + _f32(eps))
    p64 = p - U64
    return (_ratio(np.abs(m2 - m64), np.abs(m) + np.abs(g)), _ratio(np.abs(v2 - v64), v + g * g),
            _ratio(np.abs(p2 - p64), np.abs(p64) + np.abs(U64)))


def adam_trajectory_f64(p0, grads, lrs, betas, eps):
    """The float64 Adam trajectory from fp32 p0 over the fp32 gradient sequence `grads` (one per step)."""
    p = np.asarray(p0.detach().cpu().numpy(), dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    b1, b2 = betas
    for t, (g, lr) in enumerate(zip(grads, lrs), start=1):
        g = np.asarray(g.detach().cpu().numpy(), dtype=np.float64)
        m = m + (1.0 - b1) * (g - m)
        v = b2 * v + (1.0 - b2) * g * g
        step_size, bias2_sqrt = adam_constants(lr, betas, t)
        p = p - step_size * m / (np.sqrt(v) / bias2_sqrt + eps)
    return p


def make_grad(shape, scale, seed, zeros=0.3, device="cpu"):
    """randn * scale with a fraction of exact zeros (a Gaussian no camera saw)."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(shape, generator=gen) * scale
    g[torch.rand(shape, generator=gen) < zeros] = 0.0
    return g.to(device)


# ---- densification statistics: inputs and float64 reference ----------------------------------------------------------
STATS_NS = [0, 1, 63, 64, 65, 4099]
STATS_W, STATS_H = 1600, 1066


def stats_segments(N, kind):
    """kind "none" | "all" | "five": five segments with gaps between them, an empty one and one of length 1 (clamped
    into [0, N] for the smallest N)."""
    if kind == "none":
        return []
    if kind == "all":
        return [(0, N)]
    cut = lambda x: max(0, min(N, x))                                  # noqa: E731
    raw = [(0, N // 5), (N // 5 + 1, N // 5 + 2), (N // 2, N // 2), (N // 2, N // 2 + N // 4),
           (N - N // 8 - 1, N - 1)]
    return [(cut(a), max(cut(a), cut(b))) for a, b in raw]


def stats_case(N, seed, absgrad=True, batched=False, radii_float=False, visible="random", device="cpu"):
    """-> (viewspace_points with .grad [, .absgrad], radii, visibility_filter) of one render."""
    gen = torch.Generator().manual_seed(1000 + seed)
    shape = (1, N, 2) if batched else (N, 2)
    vp = torch.zeros(shape, device=device)
    # per-pixel gradients of a street scene: a wide range, some exact zeros
    mag = 10.0 ** (-8.0 + 6.0 * torch.rand(N, 1, generator=gen))
    g = torch.randn(N, 2, generator=gen) * mag
    g[torch.rand(N, generator=gen) < 0.1] = 0.0
    vp.grad = g.reshape(shape).to(device)
    if absgrad:
        vp.absgrad = (g.abs() * (1.0 + torch.rand(N, 2, generator=gen))).reshape(shape).to(device)
    radii = torch.randint(0, 60, (N,), generator=gen, dtype=torch.int32)
    if radii_float:
        radii = radii.float() / float(max(STATS_W, STATS_H))
    vis = {"random": torch.rand(N, generator=gen) < 0.6, "all": torch.ones(N, dtype=torch.bool),
           "none": torch.zeros(N, dtype=torch.bool)}[visible]
    return vp, radii.to(device), vis.to(device)


def stats_buffers(N, seed, radii_float=False, device="cpu"):
    """Pre-filled accumulators over all N rows (segments take slices of them, so rows outside every segment exist and can
    be checked): xyz_gradient_accum [N,2], denom [N,1], max_radii2D [N]."""
    gen = torch.Generator().manual_seed(2000 + seed)
    acc = torch.rand(N, 2, generator=gen) * 3.0
    den = torch.randint(0, 40, (N, 1), generator=gen).float()
    mr = torch.randint(0, 60, (N,), generator=gen).float()
    if radii_float:
        mr = mr / float(max(STATS_W, STATS_H))
    return acc.to(device), den.to(device), mr.to(device)


def stats_f64(vp, vis, acc_before, W=STATS_W, H=STATS_H):
    """-> (acc64, bound) over all N rows for rows that are visible: the mirror's expression in float64 on top of the fp32
    accumulator, and 4u (acc_before + norm64)."""
    g = vp.grad.detach().cpu().double().reshape(-1, 2)
    a0 = acc_before.detach().cpu().double()
    if hasattr(vp, "absgrad"):
        a = vp.absgrad.detach().cpu().double().reshape(-1, 2)
        scale = torch.tensor([W, H], dtype=torch.float64)
        n0 = torch.linalg.norm(a * 0.5 * scale, dim=-1)
        n1 = torch.linalg.norm(g * 0.5 * scale, dim=-1)
    else:
        n0, n1 = torch.linalg.norm(g, dim=-1), torch.zeros(g.shape[0], dtype=torch.float64)
    norm = torch.stack([n0, n1], dim=-1)
    v = vis.detach().cpu().reshape(-1, 1).double()
    return a0 + v * norm, 4 * U * (a0 + norm)


def mirror_run(segments, buffers, vp, radii, vis, W=STATS_W, H=STATS_H):
    """The torch mirror on clones of the buffers -> (acc, denom, max_radii2D) over all N rows."""
    from street_crafter_amd.densify_stats import DensificationStats
    acc, den, mr = (b.clone() for b in buffers)
    ranges = {f"m{k}": se for k, se in enumerate(segments)}
    st = DensificationStats(ranges, device=acc.device)
    for k, (s, e) in enumerate(segments):
        st.xyz_gradient_accum[f"m{k}"], st.denom[f"m{k}"], st.max_radii2D[f"m{k}"] = acc[s:e], den[s:e], mr[s:e]
    st.set_max_radii2D(radii, vis)
    st.add_densification_stats(vp, vis, W, H)
    return acc, den, mr


def covered(N, segments):
    c = torch.zeros(N, dtype=torch.bool)
    for s, e in segments:
        c[s:e] = True
    return c


# ---- tests ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


def test_adam_step_argument_handling(lib):
    """Rejected (or accepted as empty) before any launch: nothing here touches a device."""
    from street_crafter_amd import _lib
    assert lib.sc_adam_max_tensors() >= 7
    args = (0.1, 0.999, 0.001, 1e-15, None)
    assert lib.sc_adam_step(None, 0, *args) == 0                                  # no tensors
    assert lib.sc_adam_step(None, 3, *args) == -1                                 # null table
    table = (_lib.AdamTensor * 2)()
    assert lib.sc_adam_step(table, 2, *args) == 0                                 # numel == 0 twice: nothing to launch
    assert lib.sc_adam_step(table, -1, *args) == -1
    table[1].numel = -1
    assert lib.sc_adam_step(table, 2, *args) == -1                                # negative numel
    for hole in range(4):
        table[1].numel = 8
        ptrs = [64, 128, 192, 256]
        ptrs[hole] = None
        table[1].param, table[1].grad, table[1].exp_avg, table[1].exp_avg_sq = ptrs
        assert lib.sc_adam_step(table, 2, *args) == -1, hole                      # a null pointer with numel > 0
    assert C.sizeof(_lib.AdamTensor) == 48


def test_densify_stats_argument_handling(lib):
    from street_crafter_amd import _lib
    tail = (1, None, 100, 800.0, 533.0)
    assert lib.sc_densify_stats(None, None, None, *tail, None, 0, None) == 0              # no segments
    assert lib.sc_densify_stats(None, None, None, *tail, None, 2, None) == -1             # null segment table
    seg = (_lib.StatsSegment * 2)()

    def fill(k, start, end, ptrs=(64, 128, 192)):
        seg[k].start, seg[k].end = start, end
        seg[k].grad_accum, seg[k].denom, seg[k].max_radii = ptrs

    fill(0, 0, 0)
    fill(1, 7, 7)
    assert lib.sc_densify_stats(None, None, None, *tail, seg, 2, None) == 0               # only empty segments
    assert lib.sc_densify_stats(None, None, None, *tail, seg, -2, None) == -1
    fill(1, 8, 7)
    assert lib.sc_densify_stats(None, None, None, *tail, seg, 2, None) == -1              # start > end
    fill(1, 90, 101)
    assert lib.sc_densify_stats(None, None, None, *tail, seg, 2, None) == -1              # end > N
    fill(1, -1, 4)
    assert lib.sc_densify_stats(None, None, None, *tail, seg, 2, None) == -1              # start < 0
    for hole in range(3):
        ptrs = [64, 128, 192]
        ptrs[hole] = None
        fill(1, 10, 20, ptrs)
        assert lib.sc_densify_stats(None, None, None, *tail, seg, 2, None) == -1, hole    # a null accumulator
    fill(1, 10, 20)
    assert lib.sc_densify_stats(None, None, None, *tail, seg, 2, None) == -1              # rows to do, no inputs
    assert C.sizeof(_lib.StatsSegment) == 40


def test_binding_layer_has_the_two_entries_and_refuses_cpu_tensors(lib):
    from street_crafter_amd import _lib
    fast = _lib.fast()
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP device"):
        fast.adam_step([z(4)], [z(4)], [z(4)], [z(4)], [1e-3], [1.0], 0.1, 0.999, 0.001, 1e-15, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        fast.densify_stats(z(4, 2), None, z(4, dtype=torch.int32), z(4, dtype=torch.bool), 4, 800.0, 533.0, [0, 4],
                           [z(4, 2)], [z(4, 1)], [z(4)], 0)


def test_adam_refusals():
    from street_crafter_amd.optim import Adam, step_many
    w = torch.nn.Parameter(torch.zeros(5))
    for bad in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True), dict(capturable=True),
                dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            Adam([w], **bad)
    with pytest.raises(ValueError):
        Adam([w], lr=-1.0)
    opt = Adam([{"params": [w], "lr": 1e-3, "name": "xyz"}], lr=0.0, eps=1e-15)       # the reference's constructor call
    with pytest.raises(NotImplementedError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "amsgrad": True})
    opt.step()                                                                        # no grads: nothing to do, no refusal
    assert len(opt.state) == 0
    w.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="HIP device"):
        opt.step()
    assert len(opt.state) == 0 and torch.equal(w.detach(), torch.zeros(5))            # refused before anything changed
    w.grad = torch.ones(5).to_sparse()
    with pytest.raises((NotImplementedError, RuntimeError)):
        opt.step()
    opt.param_groups[0]["weight_decay"] = 0.5                                         # options are read afresh per step
    with pytest.raises(NotImplementedError):
        opt.step()
    with pytest.raises(TypeError):
        step_many([torch.optim.Adam([w])])
    opt.zero_grad()                                                                   # inherited
    assert w.grad is None


def _stepped_torch_adam(shapes, steps=3):
    params = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(i))) for i, s in enumerate(shapes)]
    groups = [{"params": [p], "lr": 1e-3 * (i + 1), "name": f"g{i}"} for i, p in enumerate(params)]
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for k in range(steps):
        for i, p in enumerate(params):
            p.grad = make_grad(p.shape, 1.0, 10 * k + i)
        opt.step()
    return params, groups, opt


def _same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert type(x) is type(y) and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (k, name)


def test_state_dict_round_trip_with_torch_adam():
    from street_crafter_amd.optim import Adam
    shapes = [(6, 3), (6, 1, 3), (6, 15, 3), (6, 1), (6, 4)]
    params, groups, topt = _stepped_torch_adam(shapes)
    sd = topt.state_dict()
    mine = Adam([{"params": [torch.nn.Parameter(p.detach().clone())], "lr": 0.5, "name": "other"} for p in params],
                lr=0.0, eps=1e-8)
    mine.load_state_dict(sd)
    _same_state_dict(mine.state_dict(), sd)
    for p, q in zip(params, (g["params"][0] for g in mine.param_groups)):
        st = mine.state[q]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"], topt.state[p]["exp_avg"])
    # ... and the other way round: what optim.Adam saves, torch.optim.Adam loads and saves back unchanged
    back = torch.optim.Adam([{"params": [torch.nn.Parameter(p.detach().clone())]} for p in params])
    back.load_state_dict(mine.state_dict())
    _same_state_dict(back.state_dict(), mine.state_dict())
    # a fresh optim.Adam has the same default keys in its groups as torch's
    fresh_t = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=0.0, eps=1e-15)
    fresh_m = Adam([torch.nn.Parameter(torch.zeros(2))], lr=0.0, eps=1e-15)
    assert fresh_m.state_dict() == fresh_t.state_dict() and fresh_m.defaults == fresh_t.defaults


def _prune(optimizer, mask):
    """gaussian_model.py:363-382 prune_optimizer, restated."""
    for group in optimizer.param_groups:
        stored = optimizer.state.get(group["params"][0], None)
        if stored is not None:
            stored["exp_avg"] = stored["exp_avg"][mask]
            stored["exp_avg_sq"] = stored["exp_avg_sq"][mask]
            del optimizer.state[group["params"][0]]
            group["params"][0] = torch.nn.Parameter(group["params"][0][mask].requires_grad_(True))
            optimizer.state[group["params"][0]] = stored
        else:
            group["params"][0] = torch.nn.Parameter(group["params"][0][mask].requires_grad_(True))


def _cat(optimizer, extension):
    """gaussian_model.py:384-408 cat_optimizer, restated; `extension`: group name -> new rows."""
    for group in optimizer.param_groups:
        ext = extension[group["name"]]
        stored = optimizer.state.get(group["params"][0], None)
        if stored is not None:
            stored["exp_avg"] = torch.cat((stored["exp_avg"], torch.zeros_like(ext)), dim=0)
            stored["exp_avg_sq"] = torch.cat((stored["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
            del optimizer.state[group["params"][0]]
            group["params"][0] = torch.nn.Parameter(torch.cat((group["params"][0], ext), dim=0).requires_grad_(True))
            optimizer.state[group["params"][0]] = stored
        else:
            group["params"][0] = torch.nn.Parameter(torch.cat((group["params"][0], ext), dim=0).requires_grad_(True))


def _reset(optimizer, name, tensor):
    """gaussian_model.py:344-361 reset_optimizer, restated."""
    for group in optimizer.param_groups:
        if group["name"] == name:
            stored = optimizer.state.get(group["params"][0], None)
            if stored is not None:
                stored["exp_avg"] = torch.zeros_like(tensor)
                stored["exp_avg_sq"] = torch.zeros_like(tensor)
                del optimizer.state[group["params"][0]]
                group["params"][0] = torch.nn.Parameter(tensor.requires_grad_(True))
                optimizer.state[group["params"][0]] = stored


def test_reference_prune_cat_reset_edits_keep_torch_state_layout():
    from street_crafter_amd.optim import Adam
    shapes = [(6, 3), (6, 15, 3), (6, 1)]
    params, groups, topt = _stepped_torch_adam(shapes)
    mine = Adam([{"params": [torch.nn.Parameter(p.detach().clone())], "lr": g["lr"], "name": g["name"]}
                 for p, g in zip(params, groups)], lr=0.0, eps=1e-15)
    mine.load_state_dict(topt.state_dict())
    mask = torch.tensor([True, False, True, True, False, True])
    ext = {g["name"]: torch.ones((2,) + tuple(s[1:])) for g, s in zip(groups, shapes)}
    for opt in (topt, mine):
        _prune(opt, mask)
        _cat(opt, ext)
        _reset(opt, "g2", torch.full((6, 1), 0.25))
    _same_state_dict(mine.state_dict(), topt.state_dict())
    for gm, gt in zip(mine.param_groups, topt.param_groups):
        pm, pt = gm["params"][0], gt["params"][0]
        assert pm.shape == pt.shape == (6,) + tuple(pm.shape[1:]) and torch.equal(pm, pt)
        assert set(mine.state[pm]) == {"step", "exp_avg", "exp_avg_sq"} and len(mine.state) == len(shapes)
        for key in ("exp_avg", "exp_avg_sq"):
            assert mine.state[pm][key].shape == pm.shape and torch.equal(mine.state[pm][key], topt.state[pt][key])
        assert float(mine.state[pm]["step"]) == 3.0


@pytest.mark.parametrize("foreach", [True, False], ids=["foreach", "single"])
def test_torch_adam_stays_inside_the_bounds(foreach):
    """torch's own fp32 Adam on the CPU, 12 steps, gradients scaled 1e-7, 1e-3 and 1 with 30 % exact zeros, judged per
    step by the staged reference: it stays inside all three bounds, so the reference and the bounds are sound."""
    betas, eps = (0.9, 0.999), 1e-15
    worst = [0.0, 0.0, 0.0]
    for i, scale in enumerate((1e-7, 1e-3, 1.0)):
        p = torch.nn.Parameter(torch.randn(4099, generator=torch.Generator().manual_seed(i)))
        opt = torch.optim.Adam([p], lr=1e-2, eps=eps, betas=betas, foreach=foreach)
        for t in range(1, 13):
            lr = 1e-2 * 0.9 ** t
            opt.param_groups[0]["lr"] = lr
            p.grad = make_grad(p.shape, scale, 100 * i + t)
            st = opt.state.get(p, {})
            before = (p.detach().clone(), p.grad.clone(), st["exp_avg"].clone() if st else torch.zeros_like(p),
                      st["exp_avg_sq"].clone() if st else torch.zeros_like(p))
            opt.step()
            r = adam_judge(before, (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]), lr, betas, eps, t)
            worst = [max(a, b) for a, b in zip(worst, r)]
    print("torch fp32 Adam (cpu, %s): error / bound for m, v, p = %.3f %.3f %.3f (in units of u: %.2f %.2f %.2f)"
          % (("foreach" if foreach else "single",) + tuple(worst) + tuple(4 * w for w in worst)))
    assert all(w <= 1.0 for w in worst), worst


def test_reference_flags_a_wrong_step():
    """The judge is not vacuous: a result that is off by a few ulp, or computed with a stale constant, fails it."""
    betas, eps, lr, t = (0.9, 0.999), 1e-15, 1e-2, 4
    gen = torch.Generator().manual_seed(5)
    p, g, m = (torch.randn(1000, generator=gen) for _ in range(3))
    v = torch.rand(1000, generator=gen)
    step_size, bias2_sqrt = adam_constants(lr, betas, t)
    m2 = (m.double() + 0.1 * (g.double() - m.double())).float()
    v2 = (0.999 * v.double() + 0.001 * g.double() ** 2).float()
    p2 = (p.double() - step_size * m2.double() / (v2.double().sqrt() / bias2_sqrt + eps)).float()
    assert max(adam_judge((p, g, m, v), (p2, m2, v2), lr, betas, eps, t)) <= 1.0
    off = adam_judge((p, g, m, v), (p2 * (1 + 2.0 ** -20), m2 * (1 + 2.0 ** -20), v2 * (1 + 2.0 ** -20)), lr, betas, eps, t)
    assert min(off) > 1.0
    stale = adam_constants(lr, betas, t - 1)
    p3 = (p.double() - stale[0] * m2.double() / (v2.double().sqrt() / stale[1] + eps)).float()
    assert adam_judge((p, g, m, v), (p3, m2, v2), lr, betas, eps, t)[2] > 1.0


@pytest.mark.parametrize("N", STATS_NS)
def test_mirror_stays_inside_the_stats_bound(N):
    """The torch mirror (fp32, CPU) on every input of the GPU test: accumulators within 4u (acc_before + norm64) of the
    float64 evaluation; denom and max_radii2D follow their definitions exactly; untouched rows stay bit-identical."""
    worst = 0.0
    for seed, (absgrad, batched, radii_float, visible, kind) in enumerate([
            (True, False, False, "random", "five"), (False, True, True, "random", "all"),
            (True, True, True, "all", "five"), (False, False, False, "none", "all"), (True, False, False, "random", "none")]):
        segments = stats_segments(N, kind)
        vp, radii, vis = stats_case(N, seed, absgrad, batched, radii_float, visible)
        buffers = stats_buffers(N, seed, radii_float)
        acc, den, mr = mirror_run(segments, buffers, vp, radii, vis)
        live = covered(N, segments) & vis
        acc64, bound = stats_f64(vp, vis, buffers[0])
        err = (acc.double() - acc64).abs()
        assert bool((err[live] <= bound[live]).all())
        if live.any():
            worst = max(worst, float((err[live] / bound[live].clamp_min(1e-300)).max()))
        assert torch.equal(acc[~live], buffers[0][~live]) and torch.equal(den[~live], buffers[1][~live])
        assert torch.equal(mr[~live], buffers[2][~live])
        assert torch.equal(den[live], buffers[1][live] + 1)
        assert torch.equal(mr[live], torch.maximum(buffers[2][live], radii.float()[live]))
    print(f"torch mirror, N = {N}: worst error / bound = {worst:.3f}")


def test_accumulate_fused_checks_its_arguments():
    from street_crafter_amd.densify_stats import DensificationStats, accumulate_fused
    vp, radii, vis = stats_case(8, 0)
    acc, den, mr = stats_buffers(8, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        accumulate_fused([(0, 8, acc, den, mr)], radii, vis, vp, 64, 64)
    with pytest.raises(RuntimeError, match="grad"):
        accumulate_fused([(0, 8, acc, den, mr)], radii, vis, torch.zeros(8, 2), 64, 64)
    st = DensificationStats({"background": (0, 8)}, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        st.accumulate_from_render_fused({"radii": radii, "visibility_filter": vis, "viewspace_points": vp}, 64, 64)
    assert math.isclose(float(st.denom["background"].sum()), 0.0)
