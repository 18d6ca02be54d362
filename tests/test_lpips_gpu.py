"""GPU tests of the perceptual loss (street_crafter_amd/lpips.py, csrc/lpips.hip) against the float64 reference of
tests/lpips_ref.py on the same fp32 inputs.

Head, every tap and every element, no exclusions (a = fhx, b = fhy, u = a - b; lpips_ref.py's docstring):
    forward   |hip - f64| <= 2^-24 K_FWD (1/P) sum_pc |w_c| (2 |u| (|a| + |b|) + u^2),  the total: the tap bars plus one
              rounding per addition
    backward  |hip - f64| <= 2^-24 K_BWD (r A_k + |f_k| (r^2 / n) sum_c A_c |f_c|),  finite and equal to the limit at n == 0
with K = 4 x the constants a float32 numpy replay of the same formulas reaches.  Both binding routes are run.
The prep kernel is bit-identical to the torch expression and its autograd.  The criterion is run whole at 67x95 with
random AlexNet-shaped weights.
"""
import numpy as np
import pytest
import torch

import lpips_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = ref.EPS
K_FWD, K_BWD = 4.0 * ref.K_FWD_REPLAY, 4.0 * ref.K_BWD_REPLAY
H, W = 67, 95

_REF = {}


def _reference(name):
    """float64 results and bar units of a case, computed once and left unchanged."""
    if name not in _REF:
        case = ref.cases()[name]
        taps, g = case["taps"], case["g"]
        d, total = ref.head_fwd(taps)
        _REF[name] = {"d": d, "total": total, "fwd_units": ref.fwd_units(taps), "grads": ref.head_bwd(taps, g),
                      "bwd_units": ref.bwd_units(taps, g)}
    return _REF[name]


@pytest.fixture(scope="module")
def lp():
    from street_crafter_amd import _lib, lpips
    _lib.load()
    return lpips


@pytest.fixture(params=["compiled", "ctypes"])
def route(request):
    from street_crafter_amd import _lib
    prev = _lib.set_fast_binding(request.param == "compiled")
    yield request.param
    _lib.set_fast_binding(prev)


def _shape(P):
    """[h, w] with h * w == P: a second spatial dimension where P has a small factor."""
    for h in (16, 7, 3):
        if P % h == 0 and P > h:
            return h, P // h
    return 1, P


def _device_taps(case, need_x=True, need_y=True, batched=False):
    """The case on the device: features [C,h,w] ([1,C,h,w] and weights [1,C,1,1] with batched), tap 0 a sliced view of a
    wider buffer on each side the case gives a channel stride for."""
    fx, fy, ws = [], [], []
    for k, (x, y, w) in enumerate(case["taps"]):
        C, P = x.shape
        h, wd = (1, P) if case["stride"] and k == 0 else _shape(P)      # (a sliced tap is [C,1,P] on both sides)
        pair = []
        for side, (a, need) in enumerate(((x, need_x), (y, need_y))):
            stride = case["stride"][side] if case["stride"] and k == 0 else None
            if stride:
                buf = torch.full((C, stride), float("nan"), device=DEV)      # what lies between the rows is never read
                buf[:, :P] = torch.from_numpy(a).to(DEV)
                t = buf[:, :P].view(C, 1, P)
                assert t.stride(0) == stride and not t.is_contiguous()
            else:
                t = torch.from_numpy(a).to(DEV).view(C, h, wd)
            t = t[None] if batched else t
            pair.append(t.requires_grad_(need))
        fx.append(pair[0])
        fy.append(pair[1])
        wt = torch.from_numpy(w).to(DEV)
        ws.append(wt.view(1, C, 1, 1) if batched else wt)
    return fx, fy, ws


def _run(lp, case, **kw):
    fx, fy, ws = _device_taps(case, **kw)
    total, taps = lp.lpips_distance(fx, fy, ws, return_taps=True)
    assert tuple(total.shape) == (1, 1, 1, 1) and taps.grad_fn is None
    if total.requires_grad:
        total.backward(torch.tensor(case["g"], device=DEV).view(1, 1, 1, 1))
    return total, taps, fx, fy


@pytest.mark.parametrize("name", list(ref.cases()))
def test_head_forward_and_backward_are_within_the_bars_everywhere(lp, route, name):
    case, want = ref.cases()[name], _reference(name)
    total, taps, fx, fy = _run(lp, case, batched=(name == "multi"))
    d = taps.cpu().numpy().astype(np.float64)
    bars = EPS * K_FWD * want["fwd_units"]
    err = np.abs(d - want["d"])
    live = want["fwd_units"] > 0
    reached = (err[live] / (EPS * want["fwd_units"][live])).max() if live.any() else 0.0
    terr, tbar = abs(float(total.detach()) - want["total"]), ref.total_bar(want["d"], bars)
    kb = 0.0
    for k, (pair_w, pair_u) in enumerate(zip(want["grads"], want["bwd_units"])):
        for t, gw, u in zip((fx[k], fy[k]), pair_w, pair_u):
            got = t.grad.reshape(gw.shape).cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            e = np.abs(got - gw)
            if (u > 0).any():
                kb = max(kb, float((e[u > 0] / (EPS * u[u > 0])).max()))
            assert (e <= EPS * K_BWD * u).all(), (name, k)
    print(f"{name} [{route}]: k_fwd reached {reached:.3f} of {K_FWD:.2f}, total err {terr:.3e} of bar {tbar:.3e}, "
          f"k_bwd reached {kb:.3f} of {K_BWD:.2f}")
    assert (err <= bars).all(), (name, err, bars)
    assert terr <= tbar
    if name.startswith("same"):                                  # y == x: exactly 0, value and every gradient
        assert float(total.detach()) == 0.0 and (d == 0).all()
        assert all((t.grad == 0).all() for t in fx + fy)


def test_gradients_at_all_zero_pixels_are_the_finite_limit(lp):
    case, want = ref.cases()["c192_p77"], _reference("c192_p77")
    _total, _taps, fx, fy = _run(lp, case)
    x, y, w = case["taps"][0]
    gx, gy = fx[0].grad.reshape(x.shape).cpu().numpy(), fy[0].grad.reshape(x.shape).cpu().numpy()
    zx, zy = (x == 0).all(axis=0), (y == 0).all(axis=0)
    assert zx[0] and zy[1] and zx[2] and zy[2]
    assert np.isfinite(gx[:, zx]).all() and np.isfinite(gy[:, zy]).all()
    assert (gx[:, 2] == 0).all() and (gy[:, 2] == 0).all()        # zero in both: u = 0
    assert (gx[:, 0] != 0).any() and (gy[:, 1] != 0).any()        # zero on one side: r a_k, r = 1 / 1e-10f
    assert (np.abs(gx[:, 0] - want["grads"][0][0][:, 0]) <= EPS * K_BWD * want["bwd_units"][0][0][:, 0]).all()
    assert (np.abs(gy[:, 1] - want["grads"][0][1][:, 1]) <= EPS * K_BWD * want["bwd_units"][0][1][:, 1]).all()


@pytest.mark.parametrize("name", ["multi", "c64_p4099"])
def test_two_runs_are_bit_identical(lp, route, name):
    case = ref.cases()[name]
    runs = []
    for _ in range(2):
        total, taps, fx, fy = _run(lp, case)
        runs.append([total.detach(), taps] + [t.grad for t in fx + fy])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_a_gradient_nobody_needs_is_not_computed(lp, route):
    case = ref.cases()["multi"]
    _t, _d, fx_both, fy_both = _run(lp, case)
    _t, _d, fx, fy = _run(lp, case, need_y=False)
    assert all(t.grad is None for t in fy) and all(torch.equal(a.grad, b.grad) for a, b in zip(fx, fx_both))
    _t, _d, fx, fy = _run(lp, case, need_x=False)
    assert all(t.grad is None for t in fx) and all(torch.equal(a.grad, b.grad) for a, b in zip(fy, fy_both))
    # one tap of one side only
    fx, fy, ws = _device_taps(case, need_x=False, need_y=False)
    fy[1].requires_grad_(True)
    lp.lpips_distance(fx, fy, ws).backward(torch.tensor(case["g"], device=DEV).view(1, 1, 1, 1))
    assert torch.equal(fy[1].grad, fy_both[1].grad) and fy[0].grad is None and fx[1].grad is None


def test_nothing_is_kept_without_a_gradient(lp):
    case = ref.cases()["c64_p4099"]
    P = 4099
    fx, fy, ws = _device_taps(case)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = lp.lpips_distance(fx, fy, ws)
    torch.cuda.synchronize()
    assert out.grad_fn is None and torch.cuda.memory_allocated() - base < P * 4          # not even one tap's norms
    fx2, fy2, _ = _device_taps(case, need_x=False, need_y=False)
    base = torch.cuda.memory_allocated()
    out2 = lp.lpips_distance(fx2, fy2, ws)
    assert out2.grad_fn is None and torch.cuda.memory_allocated() - base < P * 4 and torch.equal(out, out2)
    base = torch.cuda.memory_allocated()
    out3 = lp.lpips_distance(fx, fy, ws)
    assert out3.grad_fn is not None and torch.cuda.memory_allocated() - base >= 2 * P * 4      # the norms, for the backward


# ---- prep ----------------------------------------------------------------------------------------------------------
def _image(layout, h, w, seed):
    """-> (leaf, its [3,h,w] view): contiguous, the rasterizer's [H,W,4] image viewed as [3,H,W], or a row crop."""
    g = torch.Generator().manual_seed(seed)
    if layout == "contiguous":
        leaf = torch.rand(3, h, w, generator=g).to(DEV).requires_grad_(True)
        return leaf, leaf
    if layout == "hwc4":
        leaf = torch.rand(h, w, 4, generator=g).to(DEV).requires_grad_(True)
        return leaf, leaf.permute(2, 0, 1)[:3]
    leaf = torch.rand(3, h + 9, w, generator=g).to(DEV).requires_grad_(True)
    return leaf, leaf[:, 9:, :]


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("layout", ["contiguous", "hwc4", "crop"])
@pytest.mark.parametrize("size", [(67, 95), (16, 129)])
def test_prep_is_bit_identical_to_the_torch_expression_and_its_autograd(lp, route, size, layout, with_mask):
    h, w = size
    mask = (torch.rand(1, h, w, generator=torch.Generator().manual_seed(3)) < 0.7).to(DEV) if with_mask else None
    mean, std = torch.tensor(lp.MEAN, device=DEV)[None, :, None, None], torch.tensor(lp.STD, device=DEV)[None, :, None, None]
    up = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(4)).to(DEV)
    leaf, view = _image(layout, h, w, 5)
    assert (layout == "contiguous") == view.is_contiguous()
    z = lp.prepare(view, mask)
    assert tuple(z.shape) == (1, 3, h, w) and z.is_contiguous()
    z.backward(up)
    got_grad = leaf.grad.clone()
    leaf.grad = None
    x = view * mask if with_mask else view
    want = (x[None] - mean) / std
    want.backward(up)
    assert torch.equal(z, want)
    assert torch.equal(got_grad, leaf.grad)
    if with_mask:                                                  # a uint8 mask and a [1,3,H,W] image are the same thing
        assert torch.equal(lp.prepare(view[None].detach(), mask.to(torch.uint8)), want)


@pytest.mark.parametrize("kind", ["row_stride", "column_stride"])
def test_prep_reads_the_mask_through_its_strides(lp, kind):
    h, w = 16, 129
    g = torch.Generator().manual_seed(8)
    if kind == "row_stride":
        mask = (torch.rand(1, h, w + 5, generator=g) < 0.7).to(DEV)[:, :, :w]          # rows w + 5 apart
    else:
        mask = (torch.rand(w, h, generator=g) < 0.7).to(DEV).T[None]                   # columns h apart
    assert tuple(mask.shape) == (1, h, w) and not mask.is_contiguous()
    leaf, view = _image("hwc4", h, w, 6)
    up = torch.randn(1, 3, h, w, generator=g).to(DEV)
    z = lp.prepare(view, mask)
    z.backward(up)
    got_grad = leaf.grad.clone()
    leaf.grad = None
    mean, std = torch.tensor(lp.MEAN, device=DEV)[None, :, None, None], torch.tensor(lp.STD, device=DEV)[None, :, None, None]
    want = ((view * mask)[None] - mean) / std
    want.backward(up)
    assert torch.equal(z, want) and torch.equal(got_grad, leaf.grad)


# ---- the whole criterion at 67x95, random AlexNet-shaped weights -------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(21)
    gt = torch.rand(3, H, W, generator=g)
    image = (gt + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    mask = torch.rand(1, H, W, generator=g) < 0.7
    return image, gt, mask


def _fused(crit, image, gt_or_target, mask):
    leaf = image.clone().requires_grad_(True)
    out = crit(leaf, gt_or_target, mask)
    out.backward()
    return out.detach(), leaf.grad


def _plain(standin, image, gt, mask):
    leaf = image.clone().requires_grad_(True)
    out = ref.plain_lpips(standin, leaf, gt, mask)
    out.backward()
    return out.detach(), leaf.grad


def test_criterion_taps_through_the_float64_head(lp, scene):
    """(a) the taps of the fused route, handed to the float64 head: value and the taps' gradients within the bars.  The
    taps are cut loose from the network for this (a tap's gradient inside the chain also holds what the later layers send
    back); the chain itself is then run to the image."""
    standin = ref.standin("alex", seed=7).to(DEV)
    crit = lp.LPIPS.from_reference(standin)
    image, gt, mask = (t.to(DEV) for t in scene)
    leaf = image.clone().requires_grad_(True)
    chain = crit.features(leaf, mask)
    with torch.no_grad():
        fy = crit.features(gt, mask)
    assert [tuple(t.shape) for t in chain] == [(1, 64, 16, 23), (1, 192, 7, 11), (1, 384, 3, 5), (1, 256, 3, 5), (1, 256, 3, 5)]
    fx = [t.detach().requires_grad_(True) for t in chain]
    out, d = lp.lpips_distance(fx, fy, crit.lin_weights, return_taps=True)
    out.backward()
    taps = [(x.detach()[0].flatten(1).cpu().numpy(), y[0].flatten(1).cpu().numpy(), w.cpu().numpy())
            for x, y, w in zip(fx, fy, crit.lin_weights)]
    d64, total64 = ref.head_fwd(taps)
    units = ref.fwd_units(taps)
    err = np.abs(d.cpu().numpy().astype(np.float64) - d64)
    print(f"criterion: k_fwd reached {(err / (EPS * units)).max():.3f} of {K_FWD:.2f}")
    assert (err <= EPS * K_FWD * units).all()
    assert abs(float(out.detach()) - total64) <= ref.total_bar(d64, EPS * K_FWD * units)
    kb = 0.0
    for t, (gw, _gy), (u, _uy) in zip(fx, ref.head_bwd(taps, 1.0), ref.bwd_units(taps, 1.0)):
        e = np.abs(t.grad[0].flatten(1).cpu().numpy().astype(np.float64) - gw)
        kb = max(kb, float((e[u > 0] / (EPS * u[u > 0])).max()))
        assert (e <= EPS * K_BWD * u).all()
    print(f"criterion: k_bwd reached {kb:.3f} of {K_BWD:.2f}")
    whole = lp.lpips_distance(chain, fy, crit.lin_weights)
    assert torch.equal(whole.detach(), out.detach())
    whole.backward()
    assert torch.isfinite(leaf.grad).all() and (leaf.grad[:, ~mask[0]] == 0).all() and (leaf.grad != 0).any()


@pytest.fixture
def repeatable_convolutions():
    """torch's convolutions (MIOpen) asked for their deterministic solvers.  Left to themselves they do not repeat bit
    for bit at 67x95, forward included: 40 steps on the same inputs gave 40 different last-tap gradients and image
    gradients on an MI355X (one value: the differences are in the features' last bits), with this setting one."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def test_criterion_with_a_cached_target_is_the_criterion(lp, scene, repeatable_convolutions):
    """(b) crit(image, crit.target(gt, mask), mask) is crit(image, gt, mask): value and image gradient, bit for bit.
    Both routes run the convolution stack on torch; the comparison is made with its solvers held to the repeatable ones,
    or two runs of ONE route would already differ."""
    crit = lp.LPIPS.from_reference(ref.standin("alex", seed=7).to(DEV))
    image, gt, mask = (t.to(DEV) for t in scene)
    target = crit.target(gt, mask)
    assert all(t.grad_fn is None and not t.requires_grad for t in target.feats) and target.size == (H, W)
    assert target.nbytes() == 4 * (64 * 368 + 192 * 77 + 384 * 15 + 2 * 256 * 15)
    v1, g1 = _fused(crit, image, gt, mask)
    v2, g2 = _fused(crit, image, target, mask)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    # from_state_dicts builds the same criterion; the free function finds it once registered
    net_sd = {"features." + k: v for k, v in ref.standin("alex", seed=7).to(DEV).net.layers.state_dict().items()}
    lin_sd = {f"lin{i}.model.1.weight": w.view(1, -1, 1, 1) for i, w in enumerate(crit.lin_weights)}
    crit2 = lp.LPIPS.from_state_dicts("alex", net_sd, lin_sd)
    v3, g3 = _fused(crit2, image, gt, mask)
    assert torch.equal(v1, v3) and torch.equal(g1, g3)
    prev = lp.set_criterion("alex", crit)
    try:
        m = mask.to(torch.float32)
        assert torch.equal(lp.lpips(image * m, gt * m), crit(image * m, gt * m))
    finally:
        lp.set_criterion("alex", prev)


def test_criterion_is_as_close_to_float64_as_plain_torch(lp, scene):
    """(c) the image gradient against a float64 CPU evaluation of the whole chain: its relative L2 distance is at most
    twice that of the plain-torch fp32 route on the same device (the factor absorbs ReLU and max-pool decisions fp32 and
    float64 make differently, which hit both routes alike)."""
    standin = ref.standin("alex", seed=7)
    image, gt, mask = scene
    v64, g64 = _plain(standin.double(), image.double(), gt.double(), mask.double())
    standin = ref.standin("alex", seed=7).to(DEV)
    dev = [t.to(DEV) for t in scene]
    vp, gp = _plain(standin, dev[0], dev[1], dev[2].to(torch.float32))
    vf, gf = _fused(lp.LPIPS.from_reference(standin), *dev)
    rel = lambda g: float((g.double().cpu() - g64).norm() / g64.norm())
    print(f"criterion: value f64 {float(v64):.9f} plain {float(vp):.9f} fused {float(vf):.9f}; "
          f"gradient rel L2 to f64: plain {rel(gp):.3e}, fused {rel(gf):.3e}")
    assert rel(gf) <= 2 * rel(gp)


def test_an_all_zero_tap_pixel_gives_finite_gradients_and_plain_torch_nan_in_the_tap_gradient(lp, scene):
    """(d) zero biases and a masked corner: the first tap's corner pixel is all zero in both images.  The z-score of a
    masked pixel is -mean / std, not 0, so this criterion is built with mean 0: then the corner of the network input is 0
    and a convolution without bias keeps it 0.

    Where the NaN is: the plain-torch head gives NaN in that pixel's TAP gradient, the fused head gives 0 there (u = 0).
    It was expected to reach the image gradient of the plain route; measured on an MI355X it does not: every tap of AlexNet
    (and of VGG16) is a ReLU's output, ReLU's backward selects by the activation, which is 0 at such a pixel, and so drops
    the NaN.  Both image gradients are finite and agree; a caller who taps anything but a ReLU gets the NaN in plain torch."""
    standin = ref.standin("alex", seed=9, zero_bias=True, mean=(0.0, 0.0, 0.0)).to(DEV)
    crit = lp.LPIPS.from_reference(standin)
    image, gt, mask = (t.to(DEV) for t in scene)
    mask = mask.clone()
    mask[:, :16, :16] = False
    with torch.no_grad():
        taps_x, taps_y = crit.features(image, mask), crit.features(gt, mask)
    assert (taps_x[0][0, :, 0, 0] == 0).all() and (taps_y[0][0, :, 0, 0] == 0).all() and (taps_x[0][0, :, 8, 8] != 0).any()
    grads = {}
    for name, head in (("plain", ref.plain_distance), ("fused", lp.lpips_distance)):
        fx = [t.clone().requires_grad_(True) for t in taps_x]
        head(fx, taps_y, crit.lin_weights).backward()
        grads[name] = [t.grad for t in fx]
    assert torch.isnan(grads["plain"][0][0, :, 0, 0]).all()          # sqrt's derivative at 0 meets a zero
    assert all(torch.isfinite(g).all() for g in grads["fused"]) and (grads["fused"][0][0, :, 0, 0] == 0).all()
    ok = ~torch.isnan(grads["plain"][0])
    assert float((grads["fused"][0][ok] - grads["plain"][0][ok]).norm() / grads["plain"][0][ok].norm()) <= 1e-5
    vp, gp = _plain(standin, image, gt, mask.to(torch.float32))
    vf, gf = _fused(crit, image, gt, mask)
    assert torch.isfinite(gf).all() and (gf != 0).any() and (gf[:, ~mask[0]] == 0).all()
    assert torch.isfinite(gp).all()                      # (ReLU's backward has dropped the NaN: see above)
    assert float((gf - gp).norm() / gp.norm()) <= 1e-4
    assert torch.isfinite(vp).all() and abs(float(vf) - float(vp)) <= 1e-5 * abs(float(vp))
