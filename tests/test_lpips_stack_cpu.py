"""No-GPU checks of the HIP convolution stack of the perceptual loss (street_crafter_amd/lpips_stack.py, csrc/
lpips_stack.hip): the C entries reject bad arguments before any launch, supported() draws the route's border, the size
arithmetic matches torch's, and the float64 reference with its bars (tests/lpips_stack_ref.py) is right on a case worked
out by hand."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref  # noqa: E402
import lpips_stack_ref as R  # noqa: E402

from street_crafter_amd import lpips as L  # noqa: E402
from street_crafter_amd import lpips_stack as S  # noqa: E402

ENTRIES = ("sc_conv_pack_bytes", "sc_conv_pack_fwd", "sc_conv_pack_dgrad", "sc_conv2d_relu_fwd", "sc_conv2d_dgrad",
           "sc_conv2d_dgrad_strided", "sc_maxpool2d_fwd", "sc_maxpool2d_bwd")
SIZES = [(67, 95), (35, 39), (43, 531), (7, 9)]


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


def test_entries_are_declared_exported_and_built(lib):
    from street_crafter_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "street_crafter_amd.h")).read()
    for n in ENTRIES:
        assert n in _lib.SIGNATURES and n + "(" in header and hasattr(lib, n), n
    assert "lpips_stack.hip" in build.SOURCES
    # the reference lines each entry serves are cited next to them
    assert "networks.py:53-63" in header and "train.py:172,185" in header


def test_argument_validation_without_gpu(lib):
    # rejected before any launch: nothing here touches a device.  A fake non-null pointer is never dereferenced on the host.
    P = 4096
    # -- pack
    assert lib.sc_conv_pack_bytes(3, 64, 11, 11, 0) == (384 * 128 + 384) * 4          # K 363 -> 384, N 64 -> 128
    assert lib.sc_conv_pack_bytes(64, 192, 5, 5, 1) == (4800 * 128 + 4800) * 4        # dgrad: K = 192 * 25, N = 64 -> 128
    assert lib.sc_conv_pack_bytes(3, 64, 12, 11, 0) == 0 and lib.sc_conv_pack_bytes(0, 64, 3, 3, 0) == 0
    for fn in (lib.sc_conv_pack_fwd, lib.sc_conv_pack_dgrad):
        assert fn(None, 3, 64, 3, 3, None, 0, None) == -1                             # null pointers with work
        assert fn(P, 3, 64, 3, 3, P + 4, 1 << 20, None) == -1                         # pack not 16-byte aligned
        assert fn(P, 3, 64, 3, 3, P, 16, None) == -2                                  # pack too small
        assert fn(P, 3, 64, 12, 3, P, 1 << 20, None) == -1                            # kernel > 11
        assert fn(P, -1, 64, 3, 3, P, 1 << 20, None) == -1                            # negative size
        assert fn(None, 0, 64, 3, 3, None, 0, None) == 0                              # empty work
    # -- forward: (x, packed, bytes, bias, cin, h, w, cout, kh, kw, sy, sx, py, px, oh, ow, relu, y, stream)
    fwd = lib.sc_conv2d_relu_fwd
    big = 1 << 30
    assert fwd(None, None, 0, None, 3, 67, 95, 64, 11, 11, 4, 4, 2, 2, 16, 23, 1, None, None) == -1      # null pointers
    assert fwd(P, P, big, None, 3, 67, 95, 64, 12, 11, 4, 4, 2, 2, 16, 23, 1, P, None) == -1            # kernel > 11
    assert fwd(P, P, big, None, 3, 67, 95, 64, 11, 11, 0, 4, 2, 2, 16, 23, 1, P, None) == -1            # stride 0
    assert fwd(P, P, big, None, 3, 67, 95, 64, 11, 11, 4, 5, 2, 2, 16, 23, 1, P, None) == -1            # stride > 4
    assert fwd(P, P, big, None, 3, -67, 95, 64, 11, 11, 4, 4, 2, 2, 16, 23, 1, P, None) == -1           # negative size
    assert fwd(P, P, big, None, 3, 67, 95, 64, 11, 11, 4, 4, 2, 2, 17, 23, 1, P, None) == -1            # oh does not follow
    assert fwd(P, P, big, None, 3, 67, 95, 64, 11, 11, 4, 4, 2, 2, 16, 24, 1, P, None) == -1            # ow does not follow
    assert fwd(P, P, big, None, 3, 67, 95, 64, 3, 3, 1, 1, 3, 1, 71, 95, 1, P, None) == -1              # padding >= kernel
    assert fwd(P, P, big, None, 3, 67, 95, 64, 11, 11, 4, 4, 2, 2, 16, 23, 2, P, None) == -1            # relu not 0 / 1
    assert fwd(P, P, 16, None, 3, 67, 95, 64, 11, 11, 4, 4, 2, 2, 16, 23, 1, P, None) == -2             # pack too small
    assert fwd(P, P, big, None, 40000, 8, 8, 64, 3, 3, 1, 1, 1, 1, 8, 8, 1, P, None) == -1              # channels
    assert fwd(None, None, 0, None, 3, 5, 5, 64, 11, 11, 4, 4, 2, 2, 0, 0, 1, None, None) == 0          # no output position
    assert fwd(None, None, 0, None, 3, 67, 95, 0, 11, 11, 4, 4, 2, 2, 16, 23, 1, None, None) == 0       # no output channel
    # -- stride-1 dgrad: (g, relu_out, packed, bytes, add, cin, h, w, cout, kh, kw, py, px, oh, ow, grad_in, stream)
    dg = lib.sc_conv2d_dgrad
    assert dg(None, None, None, 0, None, 64, 7, 11, 192, 5, 5, 2, 2, 7, 11, None, None) == -1
    assert dg(P, None, P, big, None, 64, 7, 11, 192, 12, 5, 2, 2, 7, 11, P, None) == -1                 # kernel > 11
    assert dg(P, None, P, big, None, 64, 7, 11, 192, 5, 5, 2, 2, 7, 12, P, None) == -1                  # ow does not follow
    assert dg(P, None, P, big, None, 64, 7, -11, 192, 5, 5, 2, 2, 7, 11, P, None) == -1                 # negative size
    assert dg(P, None, P, 16, None, 64, 7, 11, 192, 5, 5, 2, 2, 7, 11, P, None) == -2                   # pack too small
    assert dg(None, None, None, 0, None, 0, 7, 11, 192, 5, 5, 2, 2, 7, 11, None, None) == 0             # no element of grad_in
    # -- strided dgrad: (g, relu_out, weight, add, cin, h, w, cout, kh, kw, sy, sx, py, px, oh, ow, grad_in, stream)
    ds = lib.sc_conv2d_dgrad_strided
    assert ds(None, None, None, None, 3, 67, 95, 64, 11, 11, 4, 4, 2, 2, 16, 23, None, None) == -1
    assert ds(P, None, P, None, 3, 67, 95, 64, 11, 11, 0, 4, 2, 2, 16, 23, P, None) == -1               # stride 0
    assert ds(P, None, P, None, 3, 67, 95, 64, 11, 11, 5, 4, 2, 2, 16, 23, P, None) == -1               # stride > 4
    assert ds(P, None, P, None, 3, 67, 95, 64, 11, 12, 4, 4, 2, 2, 16, 23, P, None) == -1               # kernel > 11
    assert ds(P, None, P, None, 3, 67, 95, 64, 11, 11, 4, 4, 2, 2, 15, 23, P, None) == -1               # oh does not follow
    assert ds(P, None, P, None, 3, 67, 95, -64, 11, 11, 4, 4, 2, 2, 16, 23, P, None) == -1              # negative size
    assert ds(None, None, None, None, 3, 0, 95, 64, 11, 11, 4, 4, 2, 2, 0, 23, None, None) == 0         # no element of grad_in
    # -- pools: (x, c, h, w, kh, kw, sy, sx, oh, ow, y, stream) / (g, x, add, c, h, w, kh, kw, sy, sx, oh, ow, grad_in, stream)
    pf, pb = lib.sc_maxpool2d_fwd, lib.sc_maxpool2d_bwd
    assert pf(None, 64, 16, 23, 3, 3, 2, 2, 7, 11, None, None) == -1 and pb(None, None, None, 64, 16, 23, 3, 3, 2, 2, 7, 11, None, None) == -1
    assert pf(P, 64, 16, 23, 3, 3, 0, 2, 7, 11, P, None) == -1 and pb(P, P, None, 64, 16, 23, 3, 3, 2, 0, 7, 11, P, None) == -1
    assert pf(P, 64, 16, 23, 17, 3, 2, 2, 7, 11, P, None) == -1 and pb(P, P, None, 64, 16, 23, 0, 3, 2, 2, 7, 11, P, None) == -1
    assert pf(P, 64, 16, 23, 3, 3, 2, 2, 8, 11, P, None) == -1 and pb(P, P, None, 64, 16, 23, 3, 3, 2, 2, 7, 12, P, None) == -1
    assert pf(P, -64, 16, 23, 3, 3, 2, 2, 7, 11, P, None) == -1 and pb(P, P, None, 64, -16, 23, 3, 3, 2, 2, 7, 11, P, None) == -1
    assert pf(None, 64, 2, 23, 3, 3, 2, 2, 0, 11, None, None) == 0 and pb(None, None, None, 0, 16, 23, 3, 3, 2, 2, 7, 11, None, None) == 0


def _alex_vgg():
    out = {}
    for net in ("alex", "vgg"):
        out[net] = L.LPIPS.from_reference(lpips_ref.standin(net, seed=1))
    return out


def test_supported_takes_alexnet_and_vgg16_and_names_what_it_refuses():
    for net, crit in _alex_vgg().items():
        assert S.supported(crit.layers, crit.taps) is None, net
        assert L.LPIPS(crit.layers, crit.taps, crit.mean, crit.std, crit.lin_weights, stack="hip").stack == "hip"
    table, taps = L._TABLES["alex"]()
    assert [r[0] for r in table[:2]] == ["conv", "relu"] and taps == [2, 5, 8, 10, 12]
    w, b = torch.zeros(8, 3, 3, 3), torch.zeros(8)
    conv, relu, pool = L.Conv(w, b, (1, 1), (1, 1)), L.Relu(), L.MaxPool((2, 2), (2, 2), (0, 0), False)
    lin = [torch.ones(8)]
    assert S.supported([conv, relu, pool], [3]) is None and S.supported([conv, relu, pool], [2, 3]) is None
    cases = {
        "a tap on a Conv": ([conv, relu], [1], "tap on a Conv"),
        "a Conv without ReLU": ([conv, pool], [2], "not followed by a Relu"),
        "a padded pool": ([conv, relu, L.MaxPool((3, 3), (2, 2), (1, 1), False)], [3], "padded max-pool"),
        "a ceil_mode pool": ([conv, relu, L.MaxPool((3, 3), (2, 2), (0, 0), True)], [3], "ceil_mode"),
        "a dilated conv": ([L.Conv(w, b, (1, 1), (1, 1), (2, 2)), relu], [2], "dilated convolution"),
        "a large kernel": ([L.Conv(torch.zeros(8, 3, 13, 13), b, (1, 1), (1, 1)), relu], [2], "kernel 13x13"),
        "a large stride": ([L.Conv(w, b, (5, 5), (1, 1)), relu], [2], "stride 5x5"),
        "a wide padding": ([L.Conv(w, b, (1, 1), (3, 3)), relu], [2], "padding 3x3"),
        "a pool behind a pool": ([conv, relu, pool, pool], [4], "does not follow a Relu"),
    }
    for name, (layers, tp, word) in cases.items():
        why = S.supported(layers, tp)
        assert why is not None and word in why, (name, why)
        with pytest.raises(NotImplementedError, match=word):
            L.LPIPS(layers, tp, L.MEAN, L.STD, lin * len(tp), stack="hip")           # at construction
        crit = L.LPIPS(layers, tp, L.MEAN, L.STD, lin * len(tp))                      # the torch route takes them all
        with pytest.raises(NotImplementedError, match=word):
            crit.set_stack("hip")                                                     # ... or at switch time
        assert crit.stack == "torch"
    with pytest.raises(ValueError, match="'torch' or 'hip'"):
        L.LPIPS([conv, relu], [2], L.MEAN, L.STD, lin, stack="triton")


def test_set_stack_returns_the_previous_value_and_constructors_pass_it_through():
    ref = lpips_ref.standin("alex", seed=2)
    crit = L.LPIPS.from_reference(ref)
    assert crit.stack == "torch" and crit.set_stack("hip") == "torch" and crit.stack == "hip"
    assert crit.set_stack("torch") == "hip" and crit.stack == "torch"
    assert L.LPIPS.from_reference(ref, stack="hip").stack == "hip"
    net_sd = {k: v for k, v in ref.net.layers.state_dict().items()}
    lin_sd = {f"lin{k}.model.1.weight": l[1].weight for k, l in enumerate(ref.lin)}
    assert L.LPIPS.from_state_dicts("alex", net_sd, lin_sd, stack="hip").stack == "hip"
    assert L.LPIPS.from_state_dicts("alex", net_sd, lin_sd).stack == "torch"


def test_stage_functions_check_shapes_then_refuse_cpu_tensors():
    """Shapes and dtypes first, then the device; a CPU tensor is a RuntimeError, never a fall-back to torch."""
    x = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        S.max_pool(x, 3, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        S.max_pool_bwd(torch.zeros(3, 3, 3), x, 3, 2)
    with pytest.raises(ValueError, match="float32"):
        S.max_pool(x.double(), 3, 2)
    with pytest.raises(ValueError, match="does not give a gradient"):
        S.max_pool_bwd(torch.zeros(3, 4, 3), x, 3, 2)
    with pytest.raises(TypeError, match="PackedConv"):
        S.conv_relu(x, None)
    crit = L.LPIPS.from_reference(lpips_ref.standin("alex", seed=1), stack="hip")
    with pytest.raises(RuntimeError, match="HIP device"):
        S.pack(crit.layers)                                     # CPU weights
    with pytest.raises(RuntimeError, match="HIP device"):
        S.feature_stack(crit.layers, crit.taps, torch.zeros(1, 3, 67, 95))
    with pytest.raises(ValueError, match=r"\[1,3,H,W\]"):
        S.feature_stack(crit.layers, crit.taps, torch.zeros(1, 4, 67, 95))
    with pytest.raises(RuntimeError, match="HIP device"):
        crit(torch.zeros(3, 67, 95), torch.zeros(3, 67, 95))


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_planned_sizes_are_torchs(net):
    """plan() / conv_out_hw / pool_out_hw (the arithmetic the C entries insist on) against the shapes F.conv2d and
    F.max_pool2d give on the CPU, layer by layer."""
    crit = _alex_vgg()[net]
    for H, W in SIZES:
        shapes = S.plan(crit.layers, 3, H, W)
        x = torch.zeros(1, 3, H, W)
        for layer, want in zip(crit.layers, shapes):
            if isinstance(layer, L.Conv):
                if x.shape[2] + 2 * layer.padding[0] < layer.weight.shape[2] or x.shape[3] + 2 * layer.padding[1] < layer.weight.shape[3]:
                    assert want[1] == 0 or want[2] == 0
                    break
                x = F.conv2d(x, layer.weight, layer.bias, layer.stride, layer.padding)
            elif isinstance(layer, L.MaxPool):
                if x.shape[2] < layer.kernel[0] or x.shape[3] < layer.kernel[1]:
                    assert want[1] == 0 or want[2] == 0
                    break
                x = F.max_pool2d(x, layer.kernel, layer.stride)
            assert tuple(x.shape[1:]) == want, (net, H, W, want)
    assert S.conv_out_hw(7, 9, (11, 11), (4, 4), (2, 2)) == (1, 1) and S.conv_out_hw(43, 531, (11, 11), (4, 4), (2, 2)) == (10, 132)
    assert S.conv_out_hw(6, 9, (11, 11), (4, 4), (2, 2)) == (0, 1) and S.pool_out_hw(3, 2, (3, 3), (2, 2)) == (1, 0)


def test_reference_and_bars_on_a_case_worked_out_by_hand():
    """One channel, 3x3 input 1..9, a Sobel kernel, bias 0.5, padding 1: the centre sums (1-3) + 2 (4-6) + (7-9) = -8,
    the corner (0,0) sees -2*2 - 5 = -9, the corner (0,2) sees 2*2 + 5 = 9; sum |x||w| at the centre is
    1 + 3 + 2*4 + 2*6 + 7 + 9 = 40.  The data gradient of an all-ones upstream: the centre is read by all nine outputs
    through all nine taps (sum of the kernel: 0), the corner (0,0) through w[1][1], w[1][0], w[0][1], w[0][0] = 3."""
    x = torch.arange(1.0, 10.0).reshape(1, 3, 3)
    w = torch.tensor([[1.0, 0.0, -1.0], [2.0, 0.0, -2.0], [1.0, 0.0, -1.0]]).reshape(1, 1, 3, 3)
    b = torch.tensor([0.5])
    y, bar, pre = R.conv_fwd_ref(x, w, b, (1, 1), (1, 1))
    assert y.dtype == torch.float64 and pre[0, 1, 1] == -7.5 and pre[0, 0, 0] == -8.5 and pre[0, 0, 2] == 9.5
    assert y[0, 1, 1] == 0 and y[0, 0, 0] == 0 and y[0, 0, 2] == 9.5
    u = 2.0 ** -24
    assert R.gamma(11) == 11 * u / (1 - 11 * u)
    assert bar[0, 1, 1] == pytest.approx(R.gamma(9 + 2) * 40.5, rel=1e-15)
    assert bar[0, 0, 0] == pytest.approx(R.gamma(11) * (2 * 2 + 5 + 0.5), rel=1e-15)
    # the float32 evaluation of the same sums is exact here (small integers), hence inside any bar
    ok, worst, _ = R.within(F.conv2d(x[None], w, b, 1, 1)[0].clamp_min(0), y, bar)
    assert ok and worst == 0.0
    ok, worst, _ = R.within(y.float() + 1e-3, y, bar)
    assert not ok and worst > 1.0
    g = torch.ones(1, 3, 3)
    relu_out = torch.ones(1, 3, 3)
    gi, gbar = R.conv_dgrad_ref(g, relu_out, w, (1, 1), (1, 1), (3, 3))
    assert gi[0, 1, 1] == 0 and gi[0, 0, 0] == 3 and gi[0, 0, 2] == -3
    assert gbar[0, 1, 1] == pytest.approx(R.gamma(9 + 3) * 8.0, rel=1e-15)
    # the mask: only the output (0,2), whose ReLU output above is 9.5, passes; the input (0,2) reads it through the centre
    # tap w[1][1] = 0, the input (0,1) through w[1][0] = 2, the input (2,0) not at all
    gm, _ = R.conv_dgrad_ref(g, (y == 9.5).double(), w, (1, 1), (1, 1), (3, 3), add=torch.full((1, 3, 3), 0.25))
    assert gm[0, 0, 2] == 0.25 and gm[0, 0, 1] == 2.25 and gm[0, 2, 0] == 0.25
    # a strided case: 1x1 kernel of weight 2, stride 2, on 3x3 -> 2x2 outputs; the gradient lands on the even positions
    gs, _ = R.conv_dgrad_ref(torch.ones(1, 2, 2), None, torch.full((1, 1, 1, 1), 2.0), (2, 2), (0, 0), (3, 3))
    assert gs[0].tolist() == [[2, 0, 2], [0, 0, 0], [2, 0, 2]]
    # max-pool on the CPU: the first maximum takes the gradient (checked here once, relied upon by the GPU tests)
    z = torch.zeros(1, 3, 3)
    assert R.pool_bwd_ref(torch.ones(1, 1, 1), z, 3, 2)[0].tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]
    t = torch.tensor([[[0.0, 5.0, 5.0], [5.0, 1.0, 5.0], [0.0, 0.0, 0.0]]])
    assert R.pool_bwd_ref(torch.ones(1, 1, 1), t, 3, 2)[0].tolist() == [[0, 1, 0], [0, 0, 0], [0, 0, 0]]


def test_conditioned_inputs_meet_the_conditions_the_whole_term_test_asserts():
    """lpips_stack_ref.condition: a stand-in as drawn has pre-activations within their bars of zero and pooling windows
    whose two largest entries are closer than their bars; after conditioning it has none, on the float64 evaluation."""
    crit = lpips_ref.standin("alex", seed=3)
    gen = torch.Generator().manual_seed(11)
    img, gt = torch.rand(3, 67, 95, generator=gen), torch.rand(3, 67, 95, generator=gen)
    mask = torch.rand(1, 67, 95, generator=gen) > 0.3
    before = R.violations(crit, [img, gt], [mask, mask])
    assert before[0] > 0 and before[1] > 0
    R.condition(crit, [img, gt], [mask, mask])
    assert R.violations(crit, [img, gt], [mask, mask]) == (0, 0)


def test_module_imports_alone_without_a_gpu_or_the_conv_path():
    """lpips_stack on its own: importable without a device, and it neither imports the torch route (lpips.py) nor
    names a torch convolution."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import street_crafter_amd.lpips_stack as S; "
            "print('street_crafter_amd.lpips' in sys.modules, callable(S.feature_stack))" % root)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-500:]
    assert out.stdout.split() == ["False", "True"]
    src = open(os.path.join(root, "street_crafter_amd", "lpips_stack.py")).read()
    for word in ("torch.nn.functional", "F.conv2d", "F.max_pool2d", "F.relu"):
        assert word not in src, word
