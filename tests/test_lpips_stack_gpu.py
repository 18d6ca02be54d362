"""The HIP convolution stack of the perceptual loss on the GPU (street_crafter_amd/lpips_stack.py, csrc/lpips_stack.hip).

Per stage: every stage is judged on its own against a float64 evaluation on the CPU of EXACTLY the tensors the HIP stage
got, so that a bar never has to account for an earlier stage's error.  The bars (derived in tests/lpips_stack_ref.py):

    conv + ReLU forward   |hip - f64| <= gamma(K + 2)  (|b| + sum_k |x_k| |w_k|),       K  = Cin kh kw
    data gradients        |hip - f64| <= gamma(K' + 3) (|add| + sum_k |g'_k| |w_k|),    K' = Cout kh kw
    gamma(n) = n u / (1 - n u), u = 2^-24

valid for ANY summation order of one-rounding-per-product float32 arithmetic; every element is judged.  Max-pool forward
and backward are bit-equal to torch on the CPU.  Whole term: LPIPS(stack="hip") against LPIPS(stack="torch") (the parent
commit's route, the yardstick) and against lpips_ref.plain_lpips in float64, on inputs conditioned so that no ReLU or
arg-max decision can differ between routes (lpips_stack_ref.condition).
"""
import copy
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref  # noqa: E402
import lpips_stack_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(67, 95), (35, 39), (43, 531)]


@pytest.fixture(scope="module")
def S():
    from street_crafter_amd import lpips_stack
    return lpips_stack


@pytest.fixture(scope="module")
def L():
    from street_crafter_amd import lpips
    return lpips


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _conv_record(S, L, w, b, stride, padding):
    layer = L.Conv(w.to(DEV), None if b is None else b.to(DEV), stride, padding)
    return S.pack([layer])[0]


@functools.lru_cache(maxsize=None)
def _chain(net, H, W):
    """The HIP stages of AlexNet (all five convolutions and the two pools between them) or of VGG16's first two
    convolutions over a random [3,H,W] input, run once: per stage its input and output on the device and, for a
    convolution, the float64 reference of that input (computed once, shared by the tests, never changed)."""
    from street_crafter_amd import lpips as L
    from street_crafter_amd import lpips_stack as S
    mod = lpips_ref.standin(net, seed=5 if net == "alex" else 6)
    layers = list(mod.net.layers)[:12 if net == "alex" else 4]
    gen = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn(3, H, W, generator=gen).to(DEV)
    out = []
    for layer in layers:
        if isinstance(layer, nn.Conv2d):
            w, b = layer.weight.detach(), layer.bias.detach()
            stride, padding = _pair(layer.stride), _pair(layer.padding)
            pk = _conv_record(S, L, w, b, stride, padding)
            y = S.conv_relu(x, pk)
            y64, bar, _pre = R.conv_fwd_ref(x, w, b, stride, padding)
            out.append(dict(kind="conv", x=x, y=y, pk=pk, w=w, b=b, stride=stride, padding=padding, y64=y64, bar=bar))
            x = y
        elif isinstance(layer, nn.MaxPool2d):
            k, s = _pair(layer.kernel_size), _pair(layer.stride)
            y = S.max_pool(x, k, s)
            out.append(dict(kind="pool", x=x, y=y, k=k, s=s))
            x = y
    return out


def _judge(name, got, want64, bar):
    ok, worst, at = R.within(got, want64, bar)
    print(f"{name}: {tuple(got.shape)} worst error {worst:.4f} of its bar")
    assert ok, (name, worst, at)


# ---- convolution + ReLU forward ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_conv_relu_forward_is_within_the_bar_everywhere(S, net, size):
    """AlexNet's five geometries (11x11/4 K = 363, 5x5 K = 1600, 3x3 K = 1728 / 3456 / 2304) and VGG's first two (K = 27,
    576) at full channel counts; 35x39 shrinks the 3x3 layers to 1x1, 43x531 makes a pixel row cross a 128-pixel tile."""
    convs = [r for r in _chain(net, *size) if r["kind"] == "conv"]
    assert len(convs) == (5 if net == "alex" else 2)
    for i, r in enumerate(convs):
        assert tuple(r["y"].shape) == tuple(r["y64"].shape) and r["y"].numel() > 0
        _judge(f"{net} conv{i + 1} {size}", r["y"], r["y64"], r["bar"])
        assert (r["y"] >= 0).all()
    if net == "alex" and size == (35, 39):
        assert tuple(convs[2]["y"].shape) == (384, 1, 1)
    if net == "alex" and size == (43, 531):
        assert tuple(convs[0]["y"].shape) == (64, 10, 132)


@pytest.mark.parametrize("cout", [33, 40])
def test_conv_relu_forward_off_every_tile_multiple(S, L, cout):
    """Cin = 5, 3x3 (K = 45), Cout = 33 / 40, 19x23 pixels (7 pixel tiles, the last one partial): N and K off every tile
    multiple, with and without the ReLU and the bias."""
    gen = torch.Generator().manual_seed(cout)
    w, b = torch.randn(cout, 5, 3, 3, generator=gen), torch.randn(cout, generator=gen)
    x = torch.randn(5, 19, 23, generator=gen).to(DEV)
    for bias, relu in ((b, True), (b, False), (None, True)):
        pk = _conv_record(S, L, w, bias, (1, 1), (1, 1))
        y = S.conv_relu(x, pk, relu=relu)
        y64, bar, _ = R.conv_fwd_ref(x, w, bias, (1, 1), (1, 1), relu=relu)
        _judge(f"synthetic cout {cout} bias {bias is not None} relu {relu}", y, y64, bar)
        assert tuple(S.conv_relu(x[None], pk, relu=relu).shape) == (1, cout, 19, 23)
    # the data gradient of the same layer: N = 5, K' = 9 cout
    pk = _conv_record(S, L, w, b, (1, 1), (1, 1))
    y = S.conv_relu(x, pk)
    g = torch.randn(cout, 19, 23, generator=gen).to(DEV)
    add = torch.randn(5, 19, 23, generator=gen).to(DEV)
    for a in (None, add):
        gi64, gbar = R.conv_dgrad_ref(g, y, w, (1, 1), (1, 1), (19, 23), a)
        _judge(f"synthetic dgrad cout {cout} add {a is not None}", S.conv_dgrad(g, y, pk, (19, 23), a), gi64, gbar)


def test_input_smaller_than_the_kernel(S, L):
    """7x9 under 11x11, stride 4, padding 2: one output position whose window hangs over all four edges."""
    gen = torch.Generator().manual_seed(3)
    w, b = torch.randn(64, 3, 11, 11, generator=gen), torch.randn(64, generator=gen)
    x = torch.randn(3, 7, 9, generator=gen).to(DEV)
    pk = _conv_record(S, L, w, b, (4, 4), (2, 2))
    y = S.conv_relu(x, pk)
    assert tuple(y.shape) == (64, 1, 1)
    y64, bar, _ = R.conv_fwd_ref(x, w, b, (4, 4), (2, 2))
    _judge("7x9 under 11x11", y, y64, bar)
    g = torch.randn(64, 1, 1, generator=gen).to(DEV)
    gi64, gbar = R.conv_dgrad_ref(g, y, w, (4, 4), (2, 2), (7, 9))
    _judge("7x9 under 11x11, data gradient", S.conv_dgrad(g, y, pk, (7, 9)), gi64, gbar)


# ---- data gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_stride1_data_gradient_is_within_the_bar_everywhere(S, net, size, with_add):
    """The same geometries and shapes as the forward; the mask is the SAME saved ReLU output on both sides."""
    convs = [r for r in _chain(net, *size) if r["kind"] == "conv" and r["stride"] == (1, 1)]
    assert len(convs) == (4 if net == "alex" else 2)
    gen = torch.Generator().manual_seed(17)
    for i, r in enumerate(convs):
        g = torch.randn(r["y"].shape, generator=gen).to(DEV)
        add = torch.randn(r["x"].shape, generator=gen).to(DEV) if with_add else None
        hw = tuple(r["x"].shape[1:])
        gi = S.conv_dgrad(g, r["y"], r["pk"], hw, add)
        gi64, bar = R.conv_dgrad_ref(g, r["y"], r["w"], r["stride"], r["padding"], hw, add)
        _judge(f"{net} stride-1 dgrad {i} {size}", gi, gi64, bar)


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_strided_data_gradient_is_within_the_bar_everywhere(S, size, with_add):
    """11x11 / 4 / padding 2, 64 -> 3: W is no multiple of the stride and the last output column reads a partial
    window; K' = 64 * 121."""
    r = _chain("alex", *size)[0]
    assert r["stride"] == (4, 4) and r["pk"].dgrad is None
    gen = torch.Generator().manual_seed(19)
    g = torch.randn(r["y"].shape, generator=gen).to(DEV)
    add = torch.randn(r["x"].shape, generator=gen).to(DEV) if with_add else None
    gi = S.conv_dgrad(g, r["y"], r["pk"], size, add)
    gi64, bar = R.conv_dgrad_ref(g, r["y"], r["w"], (4, 4), (2, 2), size, add)
    _judge(f"strided dgrad {size}", gi, gi64, bar)
    # without a mask every gradient counts
    gi64, bar = R.conv_dgrad_ref(g, None, r["w"], (4, 4), (2, 2), size, add)
    _judge(f"strided dgrad {size}, no mask", S.conv_dgrad(g, None, r["pk"], size, add), gi64, bar)


# ---- max-pool ------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(5, 17, 23), (5, 16, 22), (64, 10, 132)]


@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
def test_max_pool_forward_is_bit_equal_to_torch(S, k, s):
    gen = torch.Generator().manual_seed(k)
    for shape in POOL_SHAPES + [(3, k, k)]:                     # ... and an input exactly one window large
        x = torch.randn(shape, generator=gen)
        x = torch.where(torch.rand(shape, generator=gen) < 0.3, torch.zeros(()), x)
        got = S.max_pool(x.to(DEV), k, s)
        assert torch.equal(got.cpu(), R.pool_ref(x, k, s)), shape
    for r in _chain("alex", 67, 95):
        if r["kind"] == "pool":
            assert torch.equal(r["y"].cpu(), R.pool_ref(r["x"], r["k"], r["s"]))


@pytest.mark.parametrize("k,s", [(3, 2), (2, 2)])
def test_max_pool_backward_is_bit_equal_to_cpu_autograd_ties_included(S, k, s):
    gen = torch.Generator().manual_seed(10 + k)

    def check(x, name):
        oh, ow = S.pool_out_hw(x.shape[1], x.shape[2], (k, k), (s, s))
        g = torch.randn(x.shape[0], oh, ow, generator=gen)
        want = R.pool_bwd_ref(g, x, k, s)
        got = S.max_pool_bwd(g.to(DEV), x.to(DEV), k, s)
        assert torch.equal(got.cpu(), want), name
        add = torch.randn(x.shape, generator=gen)
        got = S.max_pool_bwd(g.to(DEV), x.to(DEV), k, s, add.to(DEV))
        assert torch.equal(got.cpu(), want + add), name + " + add"

    # all zero: every gradient lands on its window's first element
    check(torch.zeros(4, 9, 11), "zeros")
    got = S.max_pool_bwd(torch.ones(1, 1, 1, device=DEV), torch.zeros(1, k, k, device=DEV), k, s)
    assert got.flatten().tolist() == [1.0] + [0.0] * (k * k - 1)
    # equal positive maxima at every pair of positions of the window at (1, 1), one pair per channel; the overlapping
    # neighbours see them too
    pairs = [(i, j) for i in range(k * k) for j in range(i + 1, k * k)]
    x = torch.zeros(len(pairs), 2 * s + k + 2, 2 * s + k + 2)
    for c, (i, j) in enumerate(pairs):
        for q in (i, j):
            x[c, s + q // k, s + q % k] = 1.0
    check(x, "pairs")
    check(x - 0.5, "pairs over a negative floor")
    # random, with many ties
    for shape in POOL_SHAPES:
        check((torch.randn(shape, generator=gen) * 2).round() / 2, f"random {shape}")
        check(torch.randn(shape, generator=gen), f"random {shape}, no ties")


# ---- determinism ---------------------------------------------------------------------------------------------------------
def test_every_stage_run_twice_is_bit_identical(S):
    gen = torch.Generator().manual_seed(23)
    for net, size in (("alex", (43, 531)), ("vgg", (67, 95))):
        for r in _chain(net, *size):
            if r["kind"] == "conv":
                assert torch.equal(S.conv_relu(r["x"], r["pk"]), r["y"])
                g = torch.randn(r["y"].shape, generator=gen).to(DEV)
                add = torch.randn(r["x"].shape, generator=gen).to(DEV)
                hw = tuple(r["x"].shape[1:])
                assert torch.equal(S.conv_dgrad(g, r["y"], r["pk"], hw, add), S.conv_dgrad(g, r["y"], r["pk"], hw, add))
            else:
                assert torch.equal(S.max_pool(r["x"], r["k"], r["s"]), r["y"])
                g = torch.randn(r["y"].shape, generator=gen).to(DEV)
                assert torch.equal(S.max_pool_bwd(g, r["x"], r["k"], r["s"]), S.max_pool_bwd(g, r["x"], r["k"], r["s"]))


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_feature_stack_three_times_is_bit_identical(S, L, net):
    crit = L.LPIPS.from_reference(lpips_ref.standin(net, seed=9).to(DEV), stack="hip")
    H, W = (67, 95) if net == "alex" else (35, 39)
    gen = torch.Generator().manual_seed(29)
    z = torch.randn(1, 3, H, W, generator=gen).to(DEV)
    ups = None
    runs = []
    for _ in range(3):
        leaf = z.clone().requires_grad_(True)
        taps = S.feature_stack(crit.layers, crit.taps, leaf)
        assert len(taps) == 5 and all(t.dim() == 4 and t.grad_fn is not None for t in taps)
        if ups is None:
            ups = [torch.randn(t.shape, generator=gen).to(DEV) for t in taps]
        torch.autograd.backward(taps, ups)
        runs.append(([t.detach() for t in taps], leaf.grad))
    for taps, grad in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(taps, runs[0][0])) and torch.equal(grad, runs[0][1])
    assert torch.isfinite(runs[0][1]).all() and (runs[0][1] != 0).any()
    # a gradient for the last tap alone, and for the first alone, reaches the image too
    for only in (0, 4):
        leaf = z.clone().requires_grad_(True)
        taps = S.feature_stack(crit.layers, crit.taps, leaf)
        taps[only].backward(ups[only])
        assert torch.isfinite(leaf.grad).all() and (leaf.grad != 0).any()
    # nothing is kept without a gradient
    with torch.no_grad():
        assert all(t.grad_fn is None and not t.requires_grad for t in S.feature_stack(crit.layers, crit.taps, z.clone().requires_grad_(True)))
    assert all(t.grad_fn is None for t in S.feature_stack(crit.layers, crit.taps, z))


# ---- the whole term --------------------------------------------------------------------------------------------------------
@pytest.fixture
def repeatable_convolutions():
    """The torch route's convolutions (MIOpen) held to their repeatable solvers: left alone two runs of that route differ
    in the last bits.  The hip route needs no such setting: it never calls MIOpen."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


# The seed of each scene's images, chosen on the CPU: the float64 value of the whole term has to lie away from every
# float32 (value_margin below), or the quotient of two routes' value errors is decided by rounding alone.  A value 0.03
# of a unit in the last place from a float32 (VGG16 with seed 37) gives a route that returns that float32 an error of 0.03
# units and a route that returns the next one 0.97: a quotient of 28 between two results that are both as good as a float32
# gets.  At least 0.2 units away the two float32 that bracket the value are within a factor of 4 of one another; VGG16's
# seed is the first from 37 up that is at least 0.4 away, where the next float32 on either side is within the factor too.
SCENE_SEED = {"alex": 37, "vgg": 46}
VALUE_MARGIN = 0.2


def value_margin(v64):
    """Distance of a float64 number from the nearest float32, in units of that float32's last place (at most 0.5)."""
    import numpy as np
    near = np.float32(float(v64))
    return abs(float(near) - float(v64)) / float(np.spacing(near))


@functools.lru_cache(maxsize=None)
def _scene(net, H, W):
    """A conditioned stand-in with its images: (module on the CPU, image, gt, mask, float64 value, float64 gradient)."""
    mod = lpips_ref.standin(net, seed=31)
    gen = torch.Generator().manual_seed(SCENE_SEED[net])
    gt = torch.rand(3, H, W, generator=gen)
    image = (gt + 0.1 * torch.randn(3, H, W, generator=gen)).clamp(0, 1)
    mask = torch.rand(1, H, W, generator=gen) < 0.7                     # drops about 30 %
    R.condition(mod, [image, gt], [mask, mask])
    leaf = image.double().requires_grad_(True)
    v64 = lpips_ref.plain_lpips(copy.deepcopy(mod).double(), leaf, gt.double(), mask.double())
    v64.backward()
    return mod, image, gt, mask, v64.detach(), leaf.grad


def _run(crit, image, gt_or_target, mask):
    leaf = image.clone().requires_grad_(True)
    out = crit(leaf, gt_or_target, mask)
    out.backward()
    return out.detach(), leaf.grad


@functools.lru_cache(maxsize=None)
def _route_errors(net, H, W):
    """form -> route -> (value error, gradient error) against float64, error = max |route - f64| / max |f64|; both routes
    run once per scene and the tests below share the numbers."""
    from street_crafter_amd import lpips as L
    mod, image, gt, mask, v64, g64 = _scene(net, H, W)
    crit = L.LPIPS.from_reference(copy.deepcopy(mod).to(DEV))
    dev = [t.to(DEV) for t in (image, gt, mask)]
    out = {}
    for route in ("torch", "hip"):
        crit.set_stack(route)
        runs = {"both": _run(crit, *dev), "target": _run(crit, dev[0], crit.target(dev[1], dev[2]), dev[2])}
        for form, (v, g) in runs.items():
            assert torch.isfinite(g).all() and (g[:, ~dev[2][0]] == 0).all()
            out.setdefault(form, {})[route] = (abs(float(v.double().cpu().reshape(())) - float(v64)) / abs(float(v64)),
                                               float((g.double().cpu() - g64).abs().max() / g64.abs().max()))
    for form, err in out.items():
        print(f"{net} {H}x{W} {form}: value error torch {err['torch'][0]:.3e} hip {err['hip'][0]:.3e}; "
              f"gradient error torch {err['torch'][1]:.3e} hip {err['hip'][1]:.3e} "
              f"(ratio {err['hip'][1] / max(err['torch'][1], 1e-300):.2f})")
    return out


WHOLE = [("alex", 67, 95), ("vgg", 35, 39)]


@pytest.mark.parametrize("net,H,W", WHOLE)
def test_whole_term_inputs_are_conditioned(net, H, W):
    """Asserted on the float64 evaluation alone: no pre-activation lies within its forward bar of zero (no ReLU decision
    can differ between routes) and in no pooling window are the two largest positive entries closer than the sum of
    their bars (no arg-max can differ); the mask drops about 30 %; the float64 value lies at least VALUE_MARGIN units in
    the last place from every float32, so that the two float32 bracketing it have errors within a factor of 4 of one
    another and the value test below compares routes, not roundings."""
    mod, image, gt, mask, v64, _g64 = _scene(net, H, W)
    assert R.violations(mod, [image, gt], [mask, mask]) == (0, 0)
    assert 0.25 < float((~mask).float().mean()) < 0.35
    assert value_margin(v64) >= VALUE_MARGIN, (net, float(v64), value_margin(v64))


@pytest.mark.parametrize("net,H,W", WHOLE)
def test_whole_term_gradient_is_as_close_to_float64_as_the_torch_route(net, H, W):
    """Image gradient of LPIPS(stack="hip") and of LPIPS(stack="torch") (the parent's route, the yardstick) against
    lpips_ref.plain_lpips in float64, both images and the cached-target form: err_hip <= 4 err_torch.  The routes add
    the same K terms in different orders, which moves such an error by a small factor either way; a wrong offset, tap or
    mask moves it by orders of magnitude."""
    for form, err in _route_errors(net, H, W).items():
        assert err["hip"][1] <= 4 * err["torch"][1], (form, err)


@pytest.mark.parametrize("net,H,W", WHOLE)
def test_whole_term_value_is_as_close_to_float64_as_the_torch_route(net, H, W):
    """The same for the value, one float32 number: err_hip <= 4 err_torch.  The taps' errors largely average out over
    the thousands of elements a tap has, so both routes end within a few units in the last place of float64's value and
    the quotient is only meaningful on a scene whose float64 value keeps away from every float32
    (test_whole_term_inputs_are_conditioned asserts that)."""
    for form, err in _route_errors(net, H, W).items():
        assert err["hip"][0] <= 4 * err["torch"][0], (form, err)


def test_hip_route_cached_target_switching_and_graphs(L, repeatable_convolutions):
    mod, image, gt, mask, _v64, _g64 = _scene("alex", 67, 95)
    crit = L.LPIPS.from_reference(copy.deepcopy(mod).to(DEV))
    image, gt, mask = (t.to(DEV) for t in (image, gt, mask))
    parent = _run(crit, image, gt, mask)                               # the torch route, as the parent commit runs it
    assert crit.set_stack("hip") == "torch"
    target = crit.target(gt, mask)
    assert all(t.grad_fn is None and not t.requires_grad for t in target.feats) and target.size == (67, 95)
    assert [tuple(t.shape) for t in target.feats] == [(1, 64, 16, 23), (1, 192, 7, 11), (1, 384, 3, 5), (1, 256, 3, 5),
                                                      (1, 256, 3, 5)]
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = False                         # the hip route does not depend on it
    try:
        v1, g1 = _run(crit, image, gt, mask)
        v2, g2 = _run(crit, image, target, mask)
    finally:
        torch.backends.cudnn.deterministic = prev
    assert torch.equal(v1, v2) and torch.equal(g1, g2)
    # the weights are packed once and again only when they change
    packed = crit._packed
    _run(crit, image, target, mask)
    assert all(a is b for a, b in zip(packed, crit._packed))
    first = next(l for l in crit.layers if isinstance(l, L.Conv))
    first.weight.mul_(1.0)                                             # same values, a new version
    _run(crit, image, target, mask)
    assert crit._packed[0] is not packed[0] and all(a is b for a, b in zip(packed[1:], crit._packed[1:]))
    assert crit.set_stack("torch") == "hip"
    back = _run(crit, image, gt, mask)
    assert torch.equal(back[0], parent[0]) and torch.equal(back[1], parent[1])
