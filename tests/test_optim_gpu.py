"""GPU checks of the fused Adam step (csrc/optim.hip through street_crafter_amd/optim.py).

Every step of every case is judged per element by the staged float64 reference of tests/test_optim_cpu.py from the fp32
state before that step: |m' - m64| <= 4u (|m| + |g|), |v' - v64| <= 4u (v + g^2), |p' - p64| <= 4u (|p64| + |U64|),
u = 2^-24.  Gradients of magnitude 1e-20 are applied over second moments that a normal-sized gradient has filled (see
the CPU file's docstring: (1 - b2) 1e-40 is below fp32's normal range, where no fp32 result can meet a relative bound).
"""
import numpy as np
import pytest
import torch

from test_optim_cpu import ADAM_LENGTHS, BIG, U, adam_judge, adam_trajectory_f64, make_grad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETAS, EPS = (0.9, 0.999), 1e-15


@pytest.fixture(scope="module")
def O():
    from street_crafter_amd import _lib, optim
    _lib.load()
    return optim


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _params(lengths, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in lengths]


def _snapshot(opt, p):
    st = opt.state.get(p)
    if not st:
        return p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p), 0.0
    return p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"])


def _judged_steps(O, params, grads_of_step, lrs, lr0_index=None, skip=None, stepper=None):
    """Builds one optimizer with a group per parameter (the reference's layout), runs len(lrs) steps and judges each.
    lr0_index: that parameter's group keeps lr = 0 (p must stay bit-identical, the moments move).  skip = (step, index):
    that parameter has .grad = None on that step (p, m, v bit-identical, step count not advanced)."""
    opt = O.Adam([{"params": [p], "lr": 0.0, "name": f"g{i}"} for i, p in enumerate(params)], lr=0.0, eps=EPS, betas=BETAS)
    worst = [0.0, 0.0, 0.0]
    for k, lr in enumerate(lrs, start=1):
        before = []
        for i, p in enumerate(params):
            opt.param_groups[i]["lr"] = 0.0 if i == lr0_index else lr * (1 + i % 3)
            p.grad = None if skip == (k, i) else grads_of_step(k, i, p)
            before.append(_snapshot(opt, p))
        (stepper or (lambda o: o.step()))(opt)
        for i, p in enumerate(params):
            p0, m0, v0, t0 = before[i]
            p1, m1, v1, t1 = _snapshot(opt, p)
            if p.grad is None:
                assert t1 == t0 and torch.equal(_bits(p1), _bits(p0)), (k, i)
                assert torch.equal(_bits(m1), _bits(m0)) and torch.equal(_bits(v1), _bits(v0)), (k, i)
                continue
            assert t1 == t0 + 1, (k, i)
            r = adam_judge((p0, p.grad, m0, v0), (p1, m1, v1), opt.param_groups[i]["lr"], BETAS, EPS, t1)
            assert max(r) <= 1.0, (k, i, p.numel(), r)
            worst = [max(a, b) for a, b in zip(worst, r)]
            if i == lr0_index:
                assert torch.equal(_bits(p1), _bits(p0)), (k, i)
                assert p.numel() == 0 or not torch.equal(m1, m0) or float(p.grad.abs().sum()) == 0.0
    return opt, worst


def _plain_grads(k, i, p):
    return make_grad(p.shape, (1e-3, 1.0, 30.0)[(k + i) % 3], 1000 * k + i, device=DEV)


def _table_sizes():
    from street_crafter_amd import _lib
    try:
        mx = _lib.load().sc_adam_max_tensors()
    except Exception:                                   # collected without the library: the fixture fails the tests
        mx = 64
    return [1, 7, mx, mx + 1, 2 * mx + 3]


@pytest.mark.parametrize("n_tensors", _table_sizes())
def test_lengths_and_table_sizes(O, n_tensors):
    """Every tensor length of the list in tables of 1, 7, MAX, MAX + 1 and 2 MAX + 3 entries (the launch split and its
    last partial piece), three steps, lr changed between them, one group at lr = 0, one parameter without a gradient on
    step 2."""
    from street_crafter_amd import _lib
    assert _table_sizes()[2] == _lib.load().sc_adam_max_tensors()
    lengths = [ADAM_LENGTHS[(j + n_tensors) % len(ADAM_LENGTHS)] for j in range(n_tensors)]
    params = _params(lengths, n_tensors)
    nonempty = [j for j, n in enumerate(lengths) if n > 0]
    _, worst = _judged_steps(O, params, _plain_grads, [1e-2, 3e-3, 2e-2], lr0_index=nonempty[-1],
                             skip=(2, nonempty[len(nonempty) // 2]))
    print(f"{n_tensors} tensors: worst error / bound for m, v, p = {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")


def test_every_length_alone(O):
    """Each length as the only tensor of a call (0 included: no launch), one step each."""
    for n in ADAM_LENGTHS:
        _judged_steps(O, _params([n], n), _plain_grads, [1e-2])


def test_one_large_tensor_among_one_element_tensors(O):
    """1 048 579 elements (257 chunks with a ragged last one and a 3-element scalar tail) between 1-element tensors: the
    grid follows the chunks, not the entries."""
    params = _params([1, 1, BIG, 1, 1, 1], 3)
    _, worst = _judged_steps(O, params, _plain_grads, [1e-2, 5e-3, 1e-2], lr0_index=0, skip=(2, 3))
    print(f"large + tiny: worst error / bound for m, v, p = {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")


def test_parameter_at_storage_offset_one(O):
    """A parameter that is a view at storage offset 1 (4-byte aligned only) takes the scalar path, next to aligned
    tensors in the same table; results obey the same bounds and neighbours of the view are not written."""
    gen = torch.Generator().manual_seed(9)
    store = torch.randn(2 + 8195, generator=gen).to(DEV)
    keep = store.clone()
    view = torch.nn.Parameter(store[1:-1])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and view.numel() == 8195
    params = [_params([257], 1)[0], view, _params([4099], 2)[0]]
    _judged_steps(O, params, _plain_grads, [1e-2, 3e-3, 2e-2])
    assert store[0] == keep[0] and store[-1] == keep[-1] and not torch.equal(store[1:-1], keep[1:-1])


def test_gradient_magnitudes(O):
    """eps = 1e-15 with gradients that are exactly zero, of magnitude 1e-20, 1 and 1e4, mixed per element and re-drawn per
    step.  Step 1 fills every second moment with a normal-sized gradient (module docstring); steps 2-4 draw the classes."""
    def grads(k, i, p):
        gen = torch.Generator().manual_seed(77 * k + i)
        g = torch.randn(p.shape, generator=gen)
        if k == 1:
            return (torch.sign(g) * (0.5 + torch.rand(p.shape, generator=gen))).to(DEV)
        cls = torch.randint(0, 4, p.shape, generator=gen)
        return (g * torch.tensor([0.0, 1e-20, 1.0, 1e4])[cls]).to(DEV)

    _, worst = _judged_steps(O, _params([4099, 257, 5], 11), grads, [1e-2, 1e-3, 1e-2, 1e-2], lr0_index=1)
    print(f"magnitudes: worst error / bound for m, v, p = {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")
    # all-zero gradients on fresh state: nothing moves, nothing becomes NaN (0 / (0 + 1e-15))
    params = _params([4099], 12)
    start = params[0].detach().clone()
    opt, _ = _judged_steps(O, params, lambda k, i, p: torch.zeros_like(p), [1e-2, 1e-2])
    assert torch.equal(_bits(params[0]), _bits(start)) and float(opt.state[params[0]]["exp_avg_sq"].abs().sum()) == 0.0


def _three_optimizers(O, seed):
    opts, params = [], []
    for j, lengths in enumerate(([4099, 3, 256], [BIG // 4, 1], [0, 257, 5, 4])):
        ps = _params(lengths, seed + j)
        params += ps
        opts.append(O.Adam([{"params": [p], "lr": 1e-3 * (i + 1 + j)} for i, p in enumerate(ps)], lr=0.0, eps=EPS))
    return opts, params


def _run_three(O, how, seed=21):
    opts, params = _three_optimizers(O, seed)
    for k in range(1, 4):
        for i, p in enumerate(params):
            p.grad = None if (k, i) == (2, 4) else _plain_grads(k, i, p)
        if how == "many":
            O.step_many(opts)
        else:
            for o in opts:
                o.step()
    out = []
    for o in opts:
        for g in o.param_groups:
            p = g["params"][0]
            st = o.state[p]
            out += [_bits(p), _bits(st["exp_avg"]), _bits(st["exp_avg_sq"]), st["step"].clone()]
    return out


def test_step_many_equals_separate_steps_and_runs_repeat(O):
    """step_many over three optimizers == three step() calls, bit for bit; two runs from the same state are bit-identical;
    the ctypes route gives the same bits as the compiled binding."""
    from street_crafter_amd import _lib
    many, again, each = _run_three(O, "many"), _run_three(O, "many"), _run_three(O, "each")
    prev = _lib.set_fast_binding(False)
    try:
        assert _lib.fast() is None
        ctypes_route = _run_three(O, "many")
    finally:
        _lib.set_fast_binding(prev)
    for other in (again, each, ctypes_route):
        assert len(other) == len(many)
        for a, b in zip(many, other):
            assert torch.equal(a, b)


def test_refusals_modify_nothing(O):
    """A table with one unsupported parameter is refused whole: the parameters before it are not stepped either."""
    good = _params([257], 1)[0]
    good.grad = torch.ones_like(good)
    start = good.detach().clone()
    half = torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.float16))
    half.grad = torch.ones_like(half)
    strided = torch.nn.Parameter(torch.zeros(8, 4, device=DEV).t())
    strided.grad = torch.ones(4, 8, device=DEV)
    for bad in (half, strided):
        opt = O.Adam([good, bad], lr=1e-2)
        with pytest.raises(ValueError):
            opt.step()
        assert len(opt.state) == 0 and torch.equal(good.detach(), start)
    # a non-contiguous GRADIENT is taken through .contiguous()
    p = torch.nn.Parameter(torch.zeros(16, 4, device=DEV))
    p.grad = torch.randn(4, 16, device=DEV).t()
    assert not p.grad.is_contiguous()
    opt = O.Adam([p], lr=1e-2, eps=EPS)
    opt.step()
    r = adam_judge((torch.zeros_like(p), p.grad.contiguous(), torch.zeros_like(p), torch.zeros_like(p)),
                   (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]), 1e-2, BETAS, EPS, 1)
    assert max(r) <= 1.0, r


def test_no_host_wait(O):
    """step_many under set_sync_debug_mode("error") raises nothing, state creation included."""
    opts, params = _three_optimizers(O, 31)
    for i, p in enumerate(params):
        p.grad = _plain_grads(1, i, p)
    warm, wp = _three_optimizers(O, 32)
    for i, p in enumerate(wp):
        p.grad = _plain_grads(1, i, p)
    O.step_many(warm)                                       # library and binding loaded
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        O.step_many(opts)
        O.step_many(opts)
        with pytest.raises(RuntimeError):
            params[0].sum().item()                          # the mode is active
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in params)


def test_ten_step_trajectory_against_float64_and_torch(O):
    """Ten steps from the same start over the same fp32 gradient sequence, per gradient-scale class (1e-7, 1e-3, 1, each
    with 30 % exact zeros): dist(hip, f64) <= 2 dist(torch fp32 Adam on this GPU, f64) + 4u |p|, for the max and for the
    mean over the class.  The factor 2 allows for a different rounding order."""
    n, steps = 65537, 10
    lrs = [1e-2 * 0.8 ** k for k in range(steps)]
    for c, scale in enumerate((1e-7, 1e-3, 1.0)):
        p0 = torch.randn(n, generator=torch.Generator().manual_seed(40 + c))
        grads = [make_grad((n,), scale, 400 + 10 * c + k, device=DEV) for k in range(steps)]
        ref = adam_trajectory_f64(p0, grads, lrs, BETAS, EPS)
        got = {}
        for name, cls in (("hip", O.Adam), ("torch32", torch.optim.Adam)):
            p = torch.nn.Parameter(p0.clone().to(DEV))
            opt = cls([p], lr=0.0, eps=EPS, betas=BETAS)
            for g, lr in zip(grads, lrs):
                opt.param_groups[0]["lr"] = lr
                p.grad = g
                opt.step()
            got[name] = np.abs(p.detach().cpu().numpy().astype(np.float64) - ref)
        slack = 4 * U * np.abs(ref)
        print(f"grad scale {scale:g}: dist(hip, f64) max {got['hip'].max():.3e} mean {got['hip'].mean():.3e}; "
              f"dist(torch32, f64) max {got['torch32'].max():.3e} mean {got['torch32'].mean():.3e}")
        assert got["hip"].max() <= 2 * got["torch32"].max() + slack.max()
        assert got["hip"].mean() <= 2 * got["torch32"].mean() + slack.mean()
