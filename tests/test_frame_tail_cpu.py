"""No-GPU checks of the frame tail (street_crafter_amd/frame_tail.py): the references of tests/frame_tail_ref.py against
each other and against torch's own float64 autograd, torch's fp32 autograd of the reference lines against the bars the GPU
module holds the kernels to (a bar the reference itself cannot keep would be no bar), and every argument error of the
public interface, all of which are raised before a device is looked at.

Worst ratios of fp32 torch autograd of `tail_reference` on the host, over SIZES and the variants, in units of EPS24 times
the scale: forward 4.1 M (bar 8), per-pixel gradients 3.9 S (bar 16), affine gradient 1.1 S (bar 32, reached at 1x1; 0.02
at 1066x1600).  The host restatement of the kernel's 16 + 8 + float64 reduction stays below 0.2 S at every size.
"""
import ctypes

import pytest
import torch

import frame_tail_ref as FR

VARIANTS = [(sky, aff, D) for sky in FR.SKY_KINDS for aff in (False, True) for D in (3, 4)]
SMALL = [s for s in FR.SIZES if s[0] * s[1] <= 64 * 1031]


def _ref(c, a, s, A):
    return FR.tail_reference(c, a, s, A)


def _within(x, G, S, rel):
    return bool(((x.double() - G).abs() <= rel * S + 1e-300).all())


@pytest.mark.parametrize("H,W", SMALL)
def test_closed_form_equals_float64_autograd_of_the_reference_lines(H, W):
    inp = FR.inputs(H, W, seed=H * 10007 + W)
    if H * W >= 37 * 53:      # both kinds of pixel around the clamp are in the draw: the mask passes at equality only
        a = inp["a"]
        assert int((a == torch.tensor(1e-10, dtype=torch.float32)).sum()) > 0 and int((a == 1e-12).sum()) > 0
    for sky, aff, D in VARIANTS:
        cs = FR.case(inp, sky, aff, D, dtype=torch.float64)
        g, h = inp["g"].double(), inp["h"].double()
        for gg, hh in ((g, h), (g, None), (None, h)):
            if hh is None and gg is None or (gg is None and D == 3):
                continue
            _, grads = FR.autograd_grads(_ref, cs, gg, hh)
            G, S = FR.tail_closed_f64(cs["colors"], cs["alphas"], cs["sky"], cs["affine"], gg, hh)
            for k in ("colors", "alphas", "sky", "affine"):
                if G[k] is None:
                    assert grads[k] is None
                    continue
                got = torch.zeros_like(G[k]) if grads[k] is None else grads[k]
                assert _within(got, G[k], S[k], 1e-12), (sky, aff, D, k, gg is None, hh is None)


@pytest.mark.parametrize("H,W", SMALL)
def test_left_to_right_form_equals_the_reference_lines_in_float64(H, W):
    inp = FR.inputs(H, W, seed=H * 10007 + W)
    for sky, aff, D in VARIANTS:
        for clamp in (False, True):
            cs = FR.case(inp, sky, aff, D, dtype=torch.float64)
            args = (cs["colors"], cs["alphas"], cs["sky"], cs["affine"], clamp)
            want, got = FR.tail_reference(*args), FR.tail_l2r(*args)
            M = FR.forward_scale(*args[:4])
            assert _within(got[0], want[0], M, 1e-12), (sky, aff, D, clamp)
            assert torch.equal(got[1], want[1]) and got[1].data_ptr() == cs["alphas"].data_ptr()
            assert (got[2] is None and want[2] is None) if D == 3 else torch.equal(got[2], want[2])
            assert got[0].shape == (3, H, W) and (D == 3 or got[2].shape == (1, H, W))


@pytest.mark.parametrize("H,W", FR.SIZES)
def test_fp32_torch_autograd_of_the_reference_lines_keeps_the_bars(H, W):
    inp = FR.inputs(H, W, seed=H * 10007 + W)
    big = H * W > 64 * 1031
    variants = [("view4", True, 4), ("planes", True, 3), ("none", False, 4)] if big else VARIANTS
    worst = {"forward": 0.0, "pixel": 0.0, "affine": 0.0}
    for sky, aff, D in variants:
        cs = FR.case(inp, sky, aff, D)
        g, h = inp["g"], (inp["h"] if D == 4 else None)
        out, grads = FR.autograd_grads(_ref, cs, g, h)
        f64 = FR.tail_reference(*(None if t is None else t.double() for t in cs.values()))
        M = FR.forward_scale(*cs.values())
        worst["forward"] = max(worst["forward"], FR.ratio(out[0], f64[0], M, 1.0))
        G, S = FR.tail_closed_f64(cs["colors"], cs["alphas"], cs["sky"], cs["affine"], g, h)
        for k in ("colors", "alphas", "sky", "affine"):
            if G[k] is None:
                continue
            got = torch.zeros_like(G[k]) if grads[k] is None else grads[k]
            key = "affine" if k == "affine" else "pixel"
            worst[key] = max(worst[key], FR.ratio(got, G[k], S[k], 1.0))
    print(f"[frame_tail] {H}x{W}: fp32 torch autograd, worst ratios in EPS24 x scale: " +
          ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert worst["forward"] <= FR.FWD_BAR and worst["pixel"] <= FR.PIXEL_BAR and worst["affine"] <= FR.AFFINE_BAR


@pytest.mark.parametrize("H,W", [(37, 53), (64, 1031), (1066, 1600)])
def test_restated_16_8_float64_reduction_keeps_the_affine_bar(H, W):
    """The kernel's order of additions, restated on the host (frame_tail_ref.affine_sums_restated): no term passes through
    more than 24 fp32 additions, so the sums stay within the affine bar at every frame size."""
    inp = FR.inputs(H, W, seed=H * 10007 + W)
    for sky in ("view4", "none"):
        cs = FR.case(inp, sky, True, 4)
        G, S = FR.tail_closed_f64(cs["colors"], cs["alphas"], cs["sky"], cs["affine"], inp["g"], None)
        got = FR.affine_sums_restated(cs["colors"], cs["alphas"], cs["sky"], inp["g"])
        r = FR.ratio(got, G["affine"], S["affine"], 1.0)
        print(f"[frame_tail] {H}x{W} sky {sky}: restated reduction, worst |x - G| / (EPS24 S) = {r:.2f}")
        assert r <= FR.AFFINE_BAR


def test_a_wrong_term_sign_or_index_breaks_the_bars():
    """What the bars are for: a dropped term, a flipped sign and a transposed affine are off by S itself."""
    inp = FR.inputs(37, 53, seed=5)
    cs = FR.case(inp, "view4", True, 4, dtype=torch.float64)
    G, S = FR.tail_closed_f64(cs["colors"], cs["alphas"], cs["sky"], cs["affine"], inp["g"], inp["h"])
    assert FR.ratio(G["alphas"], G["alphas"], S["alphas"], FR.PIXEL_BAR) == 0.0
    assert FR.ratio(-G["alphas"], G["alphas"], S["alphas"], FR.PIXEL_BAR) > 1e3
    assert FR.ratio(G["affine"][:, [1, 0, 2, 3]], G["affine"], S["affine"], FR.AFFINE_BAR) > 1e3
    At = cs["affine"].clone()
    At[:, :3] = At[:, :3].t()
    Gt, _ = FR.tail_closed_f64(cs["colors"], cs["alphas"], cs["sky"], At, inp["g"], inp["h"])
    assert FR.ratio(Gt["colors"], G["colors"], S["colors"], FR.PIXEL_BAR) > 1e3
    G0, _ = FR.tail_closed_f64(cs["colors"], cs["alphas"], cs["sky"], cs["affine"], inp["g"], None)
    assert FR.ratio(G0["alphas"], G["alphas"], S["alphas"], FR.PIXEL_BAR) > 1e3


def test_argument_errors_are_raised_on_cpu_tensors():
    from street_crafter_amd.frame_tail import FrameTail, frame_tail
    H, W = 5, 7
    z = torch.zeros
    c4, c3, a = z(1, H, W, 4), z(1, H, W, 3), z(1, H, W, 1)
    assert FrameTail._fields == ("rgb", "acc", "depth")
    bad = [
        (dict(render_colors=c4.double(), render_alphas=a), ValueError, "float32"),
        (dict(render_colors=c4, render_alphas=a.half()), ValueError, "float32"),
        (dict(render_colors=c4, render_alphas=a, sky=z(1, H, W, 3, dtype=torch.float64)), ValueError, "float32"),
        (dict(render_colors=c4, render_alphas=a, affine=z(3, 4, dtype=torch.float64)), ValueError, "float32"),
        (dict(render_colors=z(H, W, 4), render_alphas=a), ValueError, r"\[1,H,W,D\]"),
        (dict(render_colors=z(2, H, W, 4), render_alphas=z(2, H, W, 1)), ValueError, "batches"),
        (dict(render_colors=z(1, H, W, 5), render_alphas=a), NotImplementedError, "3 or 4 channels"),
        (dict(render_colors=z(1, H, W, 2), render_alphas=a), NotImplementedError, "3 or 4 channels"),
        (dict(render_colors=z(1, 0, W, 4), render_alphas=z(1, 0, W, 1)), ValueError, "empty"),
        (dict(render_colors=c4, render_alphas=z(1, H, W)), ValueError, "render_alphas"),
        (dict(render_colors=c4, render_alphas=z(1, H, W + 1, 1)), ValueError, "render_alphas"),
        (dict(render_colors=z(1, H, W, 8)[..., :4], render_alphas=a), ValueError, "contiguous"),
        (dict(render_colors=c4, render_alphas=z(1, H, W, 2)[..., :1]), ValueError, "contiguous"),
        (dict(render_colors=c4, render_alphas=a, sky=z(1, H, W, 4)), ValueError, "sky"),
        (dict(render_colors=c4, render_alphas=a, sky=z(3, H, W + 1)), ValueError, "sky"),
        (dict(render_colors=c4, render_alphas=a, sky=z(H, W, 3)), ValueError, "sky"),
        (dict(render_colors=c4, render_alphas=a, affine=z(4, 4)), ValueError, "affine"),
        (dict(render_colors=c4, render_alphas=a, affine=z(12)), ValueError, "affine"),
        (dict(render_colors=c4, render_alphas=a, clamp=1), ValueError, "clamp"),
        (dict(render_colors=[1.0], render_alphas=a), ValueError, "torch.Tensor"),
        (dict(render_colors=c4.clone().requires_grad_(True), render_alphas=a, clamp=True), NotImplementedError, "forward only"),
        (dict(render_colors=c3, render_alphas=a, affine=z(3, 4).requires_grad_(True), clamp=True), NotImplementedError,
         "forward only"),
        # well-formed, but on the CPU: raised as the other modules do
        (dict(render_colors=c4, render_alphas=a), ValueError, "HIP device"),
        (dict(render_colors=c3, render_alphas=a, sky=z(3, H, W), affine=z(3, 4), clamp=True), ValueError, "HIP device"),
    ]
    for kwargs, exc, match in bad:
        with pytest.raises(exc, match=match):
            frame_tail(**kwargs)
    with torch.no_grad(), pytest.raises(ValueError, match="HIP device"):     # clamp with a leaf that requires grad, no grad mode
        frame_tail(c4.clone().requires_grad_(True), a, clamp=True)


def test_entry_points_reject_bad_arguments_before_any_launch():
    from street_crafter_amd import _lib, build
    build.build()
    lib = _lib.load()
    st = (ctypes.c_int64 * 3)(1, 28, 4)
    neg = (ctypes.c_int64 * 3)(1, -28, 4)
    one = 0x1000       # (a non-null stand-in: every call below is rejected before a pointer is used)
    assert lib.sc_frame_tail_workspace_bytes(0, 7) == 0 and lib.sc_frame_tail_workspace_bytes(1 << 16, 1 << 15) == 0
    assert lib.sc_frame_tail_workspace_bytes(1, 1) == 48 and lib.sc_frame_tail_workspace_bytes(64, 64) == 48
    assert lib.sc_frame_tail_workspace_bytes(17, 241) == 96 and lib.sc_frame_tail_workspace_bytes(1280, 1920) == 600 * 48
    fwd = lambda *v: lib.sc_frame_tail_fwd(*v, None)            # noqa: E731
    assert fwd(one, 4, 0, one, None, None, None, 0, 7, 0, one, one) == -1              # H == 0
    assert fwd(one, 4, 0, one, None, None, None, 1 << 16, 1 << 15, 0, one, one) == -1  # H W == 2^31
    assert fwd(one, 5, 0, one, None, None, None, 5, 7, 0, one, one) == -1              # channels
    assert fwd(one, 3, 0, one, None, None, None, 5, 7, 0, one, one) == -1              # depth without a depth channel
    assert fwd(one, 4, 0, one, None, None, None, 5, 7, 2, one, one) == -1              # clamp flag
    assert fwd(one, 4, 2, one, None, None, None, 5, 7, 0, one, one) == -1              # layout flag
    assert fwd(None, 4, 0, one, None, None, None, 5, 7, 0, one, one) == -1             # null inputs / output
    assert fwd(one, 4, 0, None, None, None, None, 5, 7, 0, one, one) == -1
    assert fwd(one, 4, 0, one, None, None, None, 5, 7, 0, None, one) == -1
    assert fwd(one, 4, 0, one, one, None, None, 5, 7, 0, one, one) == -1               # sky without strides
    assert fwd(one, 4, 0, one, one, neg, None, 5, 7, 0, one, one) == -1                # negative stride
    bwd = lambda *v: lib.sc_frame_tail_bwd(*v, None)            # noqa: E731
    ok = dict(colors=one, D=4, cplanar=0, alphas=one, sky=one, st=st, affine=one, H=5, W=7, g=one, h=one, gc=one, ga=one,
              gs=one, planar=0, gA=one, ws=one, ws_bytes=48)
    assert bwd(*{**ok, "H": 0}.values()) == -1
    assert bwd(*{**ok, "D": 2}.values()) == -1
    assert bwd(*{**ok, "cplanar": 2}.values()) == -1
    assert bwd(*{**ok, "g": None, "h": None}.values()) == -1                         # no upstream gradient
    assert bwd(*{**ok, "gc": None, "ga": None, "gs": None, "gA": None}.values()) == -1     # nothing asked for
    assert bwd(*{**ok, "D": 3}.values()) == -1                                      # grad_depth without a depth channel
    assert bwd(*{**ok, "sky": None}.values()) == -1                                 # grad_sky without sky
    assert bwd(*{**ok, "affine": None}.values()) == -1                              # grad_affine without affine
    assert bwd(*{**ok, "g": None}.values()) == -1                                   # grad_sky / grad_affine without grad_rgb
    assert bwd(*{**ok, "planar": 2}.values()) == -1
    assert bwd(*{**ok, "st": neg}.values()) == -1
    assert bwd(*{**ok, "ws_bytes": 47}.values()) == -2 and bwd(*{**ok, "ws": None}.values()) == -2
