"""No-GPU checks of the perceptual loss (street_crafter_amd/lpips.py): the float64 reference of tests/lpips_ref.py against
torch's autograd, its replay constants, its normalisation against the reference's own (tests/golden/lpips_norm_ref.npz),
the criterion's construction from a stand-in module and from state dicts, and every check the module makes before it
touches a device."""
import os

import numpy as np
import pytest
import torch

import lpips_ref as ref
from street_crafter_amd import lpips as _module_under_test      # noqa: F401  (every test here is about it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lp():
    from street_crafter_amd import lpips
    return lpips


def _torch_head(taps, g):
    """float64 torch autograd of the formula, written out: -> (value, [(grad_fx, grad_fy)])."""
    leaves, total = [], 0
    for fx, fy, w in taps:
        x = torch.from_numpy(fx).double().requires_grad_(True)
        y = torch.from_numpy(fy).double().requires_grad_(True)
        a = x / (torch.sqrt(torch.sum(x ** 2, dim=0)) + ref.LPIPS_EPS)
        b = y / (torch.sqrt(torch.sum(y ** 2, dim=0)) + ref.LPIPS_EPS)
        total = total + (torch.from_numpy(w).double()[:, None] * (a - b) ** 2).sum() / x.shape[1]
        leaves.append((x, y))
    total.backward(torch.tensor(float(g), dtype=torch.float64))
    return float(total.detach()), [(x.grad.numpy(), y.grad.numpy()) for x, y in leaves]


@pytest.mark.parametrize("name", list(ref.cases()))
def test_closed_form_backward_is_autograd_away_from_zero_norms_and_its_limit_at_them(name):
    case = ref.cases()[name]
    taps, g = case["taps"], case["g"]
    value, auto = _torch_head(taps, g)
    d, total = ref.head_fwd(taps)
    assert abs(total - value) <= 1e-13 * max(abs(value), float(np.sum(ref.fwd_units(taps))))
    closed, units = ref.head_bwd(taps, g), ref.bwd_units(taps, g)
    for (fx, fy, w), pair_c, pair_a, pair_u in zip(taps, closed, auto, units):
        for f, gc, ga, u in zip((fx, fy), pair_c, pair_a, pair_u):
            zero = (f.astype(np.float64) ** 2).sum(axis=0) == 0
            assert np.isfinite(gc).all()
            assert (np.abs(gc - ga)[:, ~zero] <= 1e-12 * u[:, ~zero]).all()
            if zero.any():
                assert np.isnan(ga[:, zero]).all()              # sqrt's derivative at 0 is infinite and meets a zero
        # the limit at n == 0: r a_k with fh = 0 on that side
        nx, a = ref.normalize(fx)
        ny, b = ref.normalize(fy)
        ac = 2.0 * g * w.astype(np.float64)[:, None] * (a - b) / fx.shape[1]
        r0 = 1.0 / ref.LPIPS_EPS
        assert np.array_equal(pair_c[0][:, nx == 0], (r0 * ac)[:, nx == 0])
        assert np.array_equal(pair_c[1][:, ny == 0], (-r0 * ac)[:, ny == 0])
    if name.startswith("same"):
        assert total == 0 and all((gx == 0).all() and (gy == 0).all() for gx, gy in closed)


def test_cases_hold_what_the_bars_assume():
    """Entries exactly 0 or of magnitude in [1e-3, 1e3]; zero pixels in x only, y only and both; signed and zero weights."""
    seen_zero_w = seen_neg_w = False
    for name, case in ref.cases().items():
        for fx, fy, w in case["taps"]:
            for f in (fx, fy):
                nz = f[f != 0]
                assert f.dtype == np.float32 and (nz >= np.float32(1e-3)).all() and (nz <= np.float32(1e3)).all(), name
            if fx.shape[1] >= 3 and not name.startswith("same"):
                zx, zy = (fx == 0).all(axis=0), (fy == 0).all(axis=0)
                assert (zx & ~zy).any() and (zy & ~zx).any() and (zx & zy).any(), name
            seen_zero_w |= bool((w == 0).any())
            seen_neg_w |= bool((w < 0).any())
    assert seen_zero_w and seen_neg_w
    assert {(t[0].shape) for c in ref.cases().values() for t in c["taps"]} >= set(ref.SHAPES) | set(ref.MULTI)


def test_the_replay_constants_are_what_a_fresh_float32_replay_reaches():
    k, kb = ref.replay_constants()
    assert 0.75 * ref.K_FWD_REPLAY <= k <= ref.K_FWD_REPLAY, k
    assert 0.75 * ref.K_BWD_REPLAY <= kb <= ref.K_BWD_REPLAY, kb


def test_normalisation_is_the_references_own(golden_dir):
    """tests/golden/lpips_norm_ref.npz: outputs of the reference's normalize_activation (tools/make_golden.py)."""
    z = np.load(os.path.join(golden_dir, "lpips_norm_ref.npz"))
    k = 0
    while f"f{k}" in z:
        f = z[f"f{k}"]
        C = f.shape[1]
        _n, fh = ref.normalize(f.reshape(C, -1))
        assert np.allclose(fh.reshape(f.shape), z[f"n64_{k}"], rtol=1e-14, atol=0)
        _n, fh32 = ref.normalize(f.reshape(C, -1), np.float32)
        assert fh32.dtype == np.float32 and np.allclose(fh32.reshape(f.shape), z[f"n32_{k}"], rtol=2e-6, atol=0)
        if f.shape[2] * f.shape[3] >= 2:
            assert (z[f"n64_{k}"][:, :, 0, 0] == 0).all() and (fh.reshape(f.shape)[:, :, 0, 0] == 0).all()
        k += 1
    assert k == 4


@pytest.mark.parametrize("with_mask", [False, True])
def test_prep_reference_is_the_torch_expression(with_mask):
    rng = np.random.default_rng(5)
    img = rng.random((3, 16, 129), dtype=np.float32)
    mask = rng.random((16, 129)) < 0.7 if with_mask else None
    mean, std = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
    t = torch.from_numpy(img).requires_grad_(True)
    x = t * torch.from_numpy(mask)[None] if with_mask else t
    want = (x - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]
    got = ref.prep(img, mask, mean, std, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want.detach().numpy())
    g = rng.standard_normal((3, 16, 129)).astype(np.float32)
    want.backward(torch.from_numpy(g))
    assert np.array_equal(ref.prep_bwd(g, mask, std, np.float32), t.grad.numpy())
    assert np.allclose(ref.prep(img, mask, mean, std), got, rtol=1e-6, atol=1e-7)


# ---- the criterion's construction --------------------------------------------------------------------------------------
@pytest.mark.parametrize("net_type", ["alex", "vgg"])
def test_from_reference_reads_a_standin_module_and_shares_its_weights(lp, net_type):
    import torch.nn as nn
    crit = ref.standin(net_type, seed=3)
    L = lp.LPIPS.from_reference(crit)
    rows = ref.ALEX_FEATURES if net_type == "alex" else ref.vgg_features()
    taps = ref.ALEX_TAPS if net_type == "alex" else ref.VGG_TAPS
    assert L.taps == taps and len(L.layers) == taps[-1]                 # nothing behind the last tap is kept
    for row, layer, module in zip(rows, L.layers, crit.net.layers):
        if row[0] == "conv":
            assert isinstance(layer, lp.Conv) and tuple(layer.weight.shape) == (row[2], row[1], row[3], row[3])
            assert layer.stride == (row[4], row[4]) and layer.padding == (row[5], row[5])
            assert layer.weight.data_ptr() == module.weight.data_ptr() and layer.bias.data_ptr() == module.bias.data_ptr()
        elif row[0] == "relu":
            assert isinstance(layer, lp.Relu)
        else:
            assert layer == lp.MaxPool((row[1], row[1]), (row[2], row[2]), (0, 0), False)
    assert L.mean == tuple(crit.net.mean.reshape(-1).tolist()) and L.std == tuple(crit.net.std.reshape(-1).tolist())
    for w, lin in zip(L.lin_weights, crit.lin):
        assert w.dim() == 1 and w.data_ptr() == lin[1].weight.data_ptr()
    # the records run the stand-in's network (the stack is torch, so this part runs on the CPU)
    H, W = (67, 95) if net_type == "alex" else (20, 33)
    x = torch.rand(1, 3, H, W)
    mine = L._stack((x - crit.net.mean) / crit.net.std)
    theirs = ref.plain_taps(crit, x)
    assert len(mine) == 5 and all(torch.equal(a, b) for a, b in zip(mine, theirs))
    if net_type == "alex":
        assert [tuple(t.shape[1:]) for t in mine] == [(64, 16, 23), (192, 7, 11), (384, 3, 5), (256, 3, 5), (256, 3, 5)]

    class Fire(nn.Module):
        def forward(self, x):
            return x

    crit.net.layers = nn.Sequential(*list(crit.net.layers)[:3], Fire(), *list(crit.net.layers)[3:])
    with pytest.raises(NotImplementedError, match="Fire"):
        lp.LPIPS.from_reference(crit)


@pytest.mark.parametrize("net_type", ["alex", "vgg"])
def test_from_state_dicts_builds_the_same_criterion_from_either_lin_spelling(lp, net_type):
    crit = ref.standin(net_type, seed=4)
    want = lp.LPIPS.from_reference(crit)
    net_sd = {"features." + k: v for k, v in crit.net.layers.state_dict().items()}
    net_sd["classifier.1.weight"] = torch.zeros(2, 2)                  # what else a torchvision state dict holds
    lin_published = {f"lin{i}.model.1.weight": l[1].weight for i, l in enumerate(crit.lin)}
    lin_renamed = {f"{i}.1.weight": l[1].weight for i, l in enumerate(crit.lin)}
    for lin_sd in (lin_published, lin_renamed):
        L = lp.LPIPS.from_state_dicts(net_type, net_sd, lin_sd)
        assert L.taps == want.taps and len(L.layers) == len(want.layers)
        # (the same three fp32 numbers reach the kernel: the module's buffers are the published constants in fp32)
        assert np.array_equal(np.float32(L.mean), np.float32(want.mean)) and np.array_equal(np.float32(L.std), np.float32(want.std))
        for a, b in zip(L.layers, want.layers):
            assert type(a) is type(b)
            if isinstance(a, lp.Conv):
                assert a.weight.data_ptr() == b.weight.data_ptr() and a.bias.data_ptr() == b.bias.data_ptr()
                assert a[2:] == b[2:]
            else:
                assert a == b
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(L.lin_weights, want.lin_weights))
    with pytest.raises(ValueError, match="keys"):
        lp.LPIPS.from_state_dicts(net_type, net_sd, {"lin0.weight": torch.zeros(1)})
    with pytest.raises(NotImplementedError, match="squeeze"):
        lp.LPIPS.from_state_dicts("squeeze", net_sd, lin_published)


# ---- checks before the device ------------------------------------------------------------------------------------------
def test_every_validation_error_is_raised_without_a_device(lp):
    f = lambda C=4, h=3, w=5: torch.rand(C, h, w)
    w4 = torch.rand(4)
    # lpips_distance
    with pytest.raises(ValueError, match="mismatched tap lists"):
        lp.lpips_distance([f(), f()], [f()], [w4, w4])
    with pytest.raises(ValueError, match="mismatched tap lists"):
        lp.lpips_distance([f()], [f()], [])
    with pytest.raises(ValueError, match="taps"):
        lp.lpips_distance([f()] * 9, [f()] * 9, [w4] * 9)
    with pytest.raises(ValueError, match="taps"):
        lp.lpips_distance([], [], [])
    with pytest.raises(ValueError, match="float32"):
        lp.lpips_distance([f().double()], [f()], [w4])
    with pytest.raises(ValueError, match="float32"):
        lp.lpips_distance([f()], [f()], [w4.half()])
    with pytest.raises(ValueError, match="shape mismatch"):
        lp.lpips_distance([f()], [f(4, 3, 6)], [w4])
    with pytest.raises(ValueError, match=r"\[C,h,w\]"):
        lp.lpips_distance([torch.rand(4, 15)], [torch.rand(4, 15)], [w4])
    with pytest.raises(ValueError, match="lin_weights"):
        lp.lpips_distance([f()], [f()], [torch.rand(5)])
    with pytest.raises(ValueError, match="lin_weights"):
        lp.lpips_distance([f()], [f()], [torch.rand(1, 1, 4, 1)])
    with pytest.raises(NotImplementedError, match="one image"):
        lp.lpips_distance([torch.rand(2, 4, 3, 5)], [torch.rand(2, 4, 3, 5)], [w4])
    with pytest.raises(TypeError):
        lp.lpips_distance(f(), f(), w4)
    with pytest.raises(RuntimeError, match="HIP device"):
        lp.lpips_distance([f()], [f()[None]], [w4.reshape(1, 4, 1, 1)])
    # prepare
    img = torch.rand(3, 8, 9)
    with pytest.raises(ValueError, match="float32"):
        lp.prepare(img.double())
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        lp.prepare(torch.rand(4, 8, 9))
    with pytest.raises(ValueError, match="mask"):
        lp.prepare(img, torch.ones(1, 8, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        lp.prepare(img, torch.ones(1, 8, 9))
    with pytest.raises(ValueError, match="std"):
        lp.prepare(img, None, lp.MEAN, (0.5, 0.0, 0.5))
    with pytest.raises(ValueError, match="3 numbers"):
        lp.prepare(img, None, (0.0, 0.0), lp.STD)
    with pytest.raises(NotImplementedError, match="one image"):
        lp.prepare(torch.rand(2, 3, 8, 9))
    with pytest.raises(RuntimeError, match="HIP device"):
        lp.prepare(img[None], torch.ones(1, 8, 9, dtype=torch.bool))
    # the criterion
    crit = lp.LPIPS.from_reference(ref.standin("alex"))
    with pytest.raises(NotImplementedError, match="one image"):
        crit(torch.rand(2, 3, 67, 95), torch.rand(2, 3, 67, 95))
    with pytest.raises(ValueError, match="shape mismatch"):
        crit(torch.rand(3, 67, 95), torch.rand(3, 67, 96))
    with pytest.raises(ValueError, match="target was computed"):
        crit(torch.rand(3, 67, 95), lp.LPIPSTarget([], (67, 96)))
    with pytest.raises(RuntimeError, match="HIP device"):
        crit(torch.rand(3, 67, 95), torch.rand(3, 67, 95))
    with pytest.raises(RuntimeError, match="HIP device"):
        crit.target(torch.rand(3, 67, 95))
    with pytest.raises(ValueError, match="taps"):
        lp.LPIPS(crit.layers, [2, 2], lp.MEAN, lp.STD, crit.lin_weights[:2])
    with pytest.raises(ValueError, match="lin weights"):
        lp.LPIPS(crit.layers, [2, 5], lp.MEAN, lp.STD, crit.lin_weights[:1])


def test_the_c_entries_refuse_bad_arguments_before_any_launch():
    import ctypes
    from street_crafter_amd import _lib, build
    build.build()
    lib = _lib.load()
    EINVAL, EWORKSPACE = -1, -2
    one = ctypes.c_void_p(64)                                       # a non-null pointer nobody follows
    st = (ctypes.c_int64 * 5)(70, 10, 1, 10, 1)
    mean, std, bad_std = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(1, 0, 1)
    assert lib.sc_lpips_prep_fwd(one, None, st, 0, 10, mean, std, one, None) == EINVAL            # a size <= 0
    assert lib.sc_lpips_prep_fwd(one, None, st, 7, 10, mean, bad_std, one, None) == EINVAL        # std == 0
    assert lib.sc_lpips_prep_fwd(None, None, st, 7, 10, mean, std, one, None) == EINVAL           # null required pointer
    assert lib.sc_lpips_prep_fwd(one, None, st, 7, 10, None, std, one, None) == EINVAL
    assert lib.sc_lpips_prep_fwd(one, None, (ctypes.c_int64 * 5)(70, -10, 1, 0, 0), 7, 10, mean, std, one, None) == EINVAL
    assert lib.sc_lpips_prep_bwd(one, None, st, 7, 10, bad_std, one, None) == EINVAL
    assert lib.sc_lpips_prep_bwd(one, None, st, 7, 10, std, None, None) == EINVAL
    assert lib.sc_lpips_prep_bwd(one, None, st, 7, -1, std, one, None) == EINVAL

    def table(n=1, **kw):
        t = (_lib.LpipsTap * max(n, 1))()
        for row in t:
            row.fx = row.fy = row.weight = row.norm_x = row.norm_y = row.grad_fx = 64
            row.channels, row.pixels, row.stride_x, row.stride_y = 4, 100, 100, 100
            for k, v in kw.items():
                setattr(row, k, v)
        return t

    ws_ok = lib.sc_lpips_head_workspace_bytes(table(), 1)
    assert ws_ok == 2 * 8 and lib.sc_lpips_head_workspace_bytes(table(3), 3) == 3 * 2 * 8
    assert lib.sc_lpips_head_workspace_bytes(table(9), 9) == 0 and lib.sc_lpips_head_workspace_bytes(None, 1) == 0
    assert lib.sc_lpips_head_workspace_bytes(table(pixels=0), 1) == 0
    for bad in (dict(channels=0), dict(pixels=0), dict(pixels=-3), dict(stride_x=99), dict(stride_y=99), dict(fx=None),
                dict(fy=None), dict(weight=None)):
        assert lib.sc_lpips_head_fwd(table(**bad), 1, one, one, 1024, None) == EINVAL, bad
        assert lib.sc_lpips_head_bwd(table(**bad), 1, one, None) == EINVAL, bad
    assert lib.sc_lpips_head_fwd(table(9), 9, one, one, 1024, None) == EINVAL                     # more than 8 taps
    assert lib.sc_lpips_head_fwd(table(), 0, one, one, 1024, None) == EINVAL
    assert lib.sc_lpips_head_fwd(None, 1, one, one, 1024, None) == EINVAL
    assert lib.sc_lpips_head_fwd(table(), 1, None, one, 1024, None) == EINVAL
    assert lib.sc_lpips_head_fwd(table(), 1, one, one, ws_ok - 1, None) == EWORKSPACE
    assert lib.sc_lpips_head_fwd(table(), 1, one, None, 1024, None) == EWORKSPACE
    assert lib.sc_lpips_head_bwd(table(), 1, None, None) == EINVAL                                # no upstream gradient
    assert lib.sc_lpips_head_bwd(table(norm_x=None), 1, one, None) == EINVAL                      # the forward's norms
    assert lib.sc_lpips_head_bwd(table(grad_fx=None), 1, one, None) == 0                          # nobody wants a gradient


def test_lpips_without_a_registered_criterion_raises_and_fetches_nothing(lp, monkeypatch):
    import socket
    import urllib.request

    def forbidden(*a, **k):
        raise AssertionError("lpips() tried to reach the network")

    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", forbidden)
    monkeypatch.setattr(torch.hub, "download_url_to_file", forbidden)
    monkeypatch.setattr(urllib.request, "urlopen", forbidden)
    monkeypatch.setattr(socket.socket, "connect", forbidden)
    prev = lp.set_criterion("alex", None)
    try:
        x = torch.rand(3, 67, 95)
        with pytest.raises(RuntimeError, match="set_criterion"):
            lp.lpips(x, x)
        with pytest.raises(RuntimeError, match="vgg"):
            lp.lpips(x, x, net_type="vgg")
        with pytest.raises(ValueError, match="version"):
            lp.lpips(x, x, version="0.0")
        crit = lp.LPIPS.from_reference(ref.standin("alex"))
        assert lp.set_criterion("alex", crit) is None
        with pytest.raises(RuntimeError, match="HIP device"):          # registered: now it is the device that is missing
            lp.lpips(x, x)
        assert lp.set_criterion("alex", None) is crit
        with pytest.raises(TypeError):
            lp.set_criterion("alex", ref.standin("alex"))
    finally:
        lp.set_criterion("alex", prev)
