"""The frame tail's kernels (csrc/frame_tail.hip behind street_crafter_amd/frame_tail.py) against the references and bars
of tests/frame_tail_ref.py (tests/test_frame_tail_cpu.py judges those on their own).

Sizes: frame_tail_ref.SIZES plus one size on each side of every boundary of the kernels:
  pixels per lane (4)                              1x3 | 1x4 | 1x5         the scalar tail, no tail, one group + tail
  pixels per forward block and backward pass (1024)   3x341 | 32x32 | 25x41   1023 | 1024 | 1025: a second block / pass
  pixels per backward block (4096 = 16 per lane)   63x65 | 64x64 | 17x241  4095 | 4096 | 4097: a second row of partials
  block partials per finishing-stage lane (256)    1024x1024 | 1024x1025   256 | 257 blocks: a lane adds a second partial
H*W is a multiple of 4 at some sizes and not at others, so planes 1 and 2 of rgb, the upstream gradient and a planar sky
take the 16-byte path at the former and the scalar one at the latter.

Variants: sky in {none, the [..., :3] view of 4 channels, contiguous [1,H,W,3], [3,H,W] planes, an odd-strided view} x
affine {none, given} x D {3, 4}; thinned to four at the largest size, 1066x1600.
"""
import pytest
import torch

import frame_tail_ref as FR

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUNDARY = [(1, 4), (1, 5), (3, 341), (32, 32), (25, 41), (63, 65), (64, 64), (17, 241), (1024, 1024), (1024, 1025)]
ALL_SIZES = FR.SIZES + BOUNDARY
VARIANTS = [(sky, aff, D) for sky in FR.SKY_KINDS for aff in (False, True) for D in (3, 4)]
THIN = [("view4", True, 4), ("planes", True, 3), ("odd", False, 4), ("none", False, 3)]


def _variants(H, W):
    return THIN if (H, W) == max(ALL_SIZES, key=lambda s: s[0] * s[1]) else VARIANTS


@pytest.fixture(scope="module")
def T():
    from street_crafter_amd import _lib
    _lib.load()
    from street_crafter_amd import frame_tail
    yield frame_tail
    _INPUTS.clear()                  # the module's draws are not kept for the rest of the suite


_INPUTS = {}


def _inputs(H, W):
    """One draw per size for the whole module, on the device, never written to."""
    if (H, W) not in _INPUTS:
        _INPUTS[(H, W)] = {k: v.to(DEV) for k, v in FR.inputs(H, W, seed=H * 10007 + W).items()}
    return _INPUTS[(H, W)]


def _tail(T):
    return lambda c, a, s, A: T.frame_tail(c, a, s, A)


@pytest.mark.parametrize("H,W", ALL_SIZES)
def test_forward_is_the_left_to_right_form_bit_for_bit_and_within_the_float64_bar(T, H, W):
    inp = _inputs(H, W)
    worst = 0.0
    for sky, aff, D in _variants(H, W):
        cs = FR.case(inp, sky, aff, D, device=DEV)
        args = (cs["colors"], cs["alphas"], cs["sky"], cs["affine"])
        with torch.no_grad():
            for clamp in (False, True):
                got = T.frame_tail(*args, clamp=clamp)
                want = FR.tail_l2r(*args, clamp)
                assert got.rgb.shape == (3, H, W) and got.rgb.is_contiguous()
                assert torch.equal(got.rgb, want[0]), (sky, aff, D, clamp, float((got.rgb - want[0]).abs().max()))
                assert got.acc.shape == (1, H, W) and got.acc.data_ptr() == cs["alphas"].data_ptr()
                assert got.acc.stride() == cs["alphas"][..., 0].stride()
                if D == 3:
                    assert got.depth is None
                else:
                    assert got.depth.shape == (1, H, W) and got.depth.is_contiguous()
                    assert torch.equal(got.depth, want[2]), (sky, aff, D, clamp)
            got = T.frame_tail(*args)
            # (the reference's einsum in float64 runs on the host: this module launches elementwise kernels and sums only)
            f64 = [None if o is None else o.to(DEV) for o in
                   FR.tail_reference(*(None if t is None else t.double().cpu() for t in args))]
            r = FR.ratio(got.rgb, f64[0], FR.forward_scale(*args), FR.FWD_BAR)
            assert r <= 1.0, (sky, aff, D, r)
            worst = max(worst, r)
            if D == 4:     # one rounded quotient; the clamp's constant is float32(1e-10) here and 1e-10 there: 2 EPS24 |depth|
                assert FR.ratio(got.depth, f64[2], f64[2].abs(), 2.0) <= 1.0, (sky, aff, D)
    print(f"[frame_tail] {H}x{W}: forward, worst |rgb - f64| / (8 EPS24 M) = {worst:.3f}")


@pytest.mark.parametrize("H,W", ALL_SIZES)
def test_backward_against_the_float64_closed_form(T, H, W):
    """Every entry of every gradient, with both upstream gradients, with g only and with h only; a gradient that an
    absent upstream gradient leaves identically zero is not computed."""
    inp = _inputs(H, W)
    for sky, aff, D in _variants(H, W):
        cs = FR.case(inp, sky, aff, D, device=DEV)
        ups = [("g+h", inp["g"], inp["h"]), ("g", inp["g"], None), ("h", None, inp["h"])] if D == 4 else [("g", inp["g"], None)]
        for name, g, h in ups:
            _, grads = FR.autograd_grads(_tail(T), cs, g, h)
            G, S = FR.tail_closed_f64(cs["colors"], cs["alphas"], cs["sky"], cs["affine"], g, h)
            none = set()
            if g is None:
                none |= {"sky", "affine"}
            if h is None and sky == "none":
                none.add("alphas")
            FR.judge_backward(f"{H}x{W} sky {sky} affine {aff} D {D} upstream {name}", grads, G, S, expect_none=none)


def test_gradients_nobody_asked_for_are_not_computed(T):
    inp = _inputs(37, 53)
    cs = FR.case(inp, "view4", True, 4, device=DEV)
    G, S = FR.tail_closed_f64(cs["colors"], cs["alphas"], cs["sky"], cs["affine"], inp["g"], inp["h"])
    for asked in (("colors", "alphas"), ("alphas",), ("sky",), ("affine",), ("colors", "affine")):
        leaves = {k: t.detach().clone().requires_grad_(k in asked) for k, t in cs.items()}
        out = T.frame_tail(leaves["colors"], leaves["alphas"], leaves["sky"], leaves["affine"])
        ((out.rgb * inp["g"]).sum() + (out.depth * inp["h"]).sum()).backward()
        for k, t in leaves.items():
            if k in asked:
                assert FR.ratio(t.grad, G[k], S[k], FR.AFFINE_BAR if k == "affine" else FR.PIXEL_BAR) <= 1.0, (asked, k)
            else:
                assert t.grad is None, (asked, k)
    # nothing requires grad: no graph at all
    out = T.frame_tail(cs["colors"], cs["alphas"], cs["sky"], cs["affine"])
    assert not out.rgb.requires_grad and not out.depth.requires_grad and not out.acc.requires_grad


def test_what_flows_into_acc_is_added_to_the_tails_own_gradient(T):
    inp = _inputs(37, 53)
    cs = FR.case(inp, "planes", True, 4, device=DEV)
    u = torch.randn(1, 37, 53, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    _, own = FR.autograd_grads(_tail(T), cs, inp["g"], inp["h"])
    a = cs["alphas"].clone().requires_grad_(True)
    out = T.frame_tail(cs["colors"], a, cs["sky"], cs["affine"])
    assert out.acc.data_ptr() == a.data_ptr() and out.acc.requires_grad
    ((out.rgb * inp["g"]).sum() + (out.depth * inp["h"]).sum() + (out.acc * u).sum()).backward()
    assert torch.equal(a.grad, own["alphas"] + u[..., None])


def test_clamp_is_forward_only_and_takes_the_rasterizers_planar_output(T):
    """clamp=True with an input that requires grad is refused; under no_grad it runs on the rasterizer's output as it
    comes there: the permuted view of [1,D,H,W] planes (rendering.set_planar_output), the sky pass's `[..., :3]` of one."""
    inp = _inputs(37, 53)
    cs = FR.case(inp, "view4", True, 4, device=DEV)
    with pytest.raises(NotImplementedError, match="forward only"):
        T.frame_tail(cs["colors"].clone().requires_grad_(True), cs["alphas"], cs["sky"], cs["affine"], clamp=True)
    planes = cs["colors"].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    sky_planes = inp["sky4"].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)[..., :3]
    assert not planes.is_contiguous() and torch.equal(planes, cs["colors"])
    for clamp in (False, True):
        with torch.no_grad():
            want = T.frame_tail(cs["colors"], cs["alphas"], cs["sky"], cs["affine"], clamp=clamp)
            got = T.frame_tail(planes, cs["alphas"], sky_planes, cs["affine"], clamp=clamp)
            got3 = T.frame_tail(planes[..., :3].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), cs["alphas"], sky_planes,
                                cs["affine"], clamp=clamp)
        assert torch.equal(got.rgb, want.rgb) and torch.equal(got.depth, want.depth)
        assert torch.equal(got3.rgb, want.rgb) and got3.depth is None
    # the planar layout also trains (the same gradients, grad_colors arriving interleaved)
    _, a = FR.autograd_grads(_tail(T), cs, inp["g"], inp["h"])
    _, b = FR.autograd_grads(_tail(T), {**cs, "colors": planes, "sky": sky_planes}, inp["g"], inp["h"])
    assert all(torch.equal(a[k], b[k]) for k in a)


def _run(T, cs, g, h):
    out, grads = FR.autograd_grads(_tail(T), cs, g, h)
    return {"rgb": out[0], "depth": out[2], **grads}


def _same(tag, a, b, sky_layouts=None):
    for k in a:
        x, y = a[k], b[k]
        assert (x is None) == (y is None), (tag, k)
        if x is None:
            continue
        if k == "sky" and sky_layouts is not None and x.dim() != y.dim():      # [3,H,W] against [1,H,W,3]: the same values
            x, y = (x if x.dim() == 3 else x[0].permute(2, 0, 1)), (y if y.dim() == 3 else y[0].permute(2, 0, 1))
        assert torch.equal(x, y), (tag, k, float((x - y).abs().max()))


def _shifted(t):
    """The same values as a view one element into a larger buffer: every 16-byte access of it would be misaligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("H,W", [(1, 3), (37, 53), (64, 64), (64, 1031), (17, 241)])
def test_results_are_bit_identical_across_runs_routes_layouts_and_alignment(T, H, W):
    from street_crafter_amd import _lib
    inp = _inputs(H, W)
    g, h = inp["g"], inp["h"]
    for aff, D in ((True, 4), (False, 3)):
        hh = h if D == 4 else None
        base = {sky: _run(T, FR.case(inp, sky, aff, D, device=DEV), g, hh) for sky in FR.SKY_KINDS}
        for sky in FR.SKY_KINDS:
            cs = FR.case(inp, sky, aff, D, device=DEV)
            _same(f"second run, sky {sky}", base[sky], _run(T, cs, g, hh))
            prev = _lib.set_fast_binding(False)
            try:
                assert _lib.fast() is None
                _same(f"ctypes route, sky {sky}", base[sky], _run(T, cs, g, hh))
            finally:
                _lib.set_fast_binding(prev)
            assert _lib.fast() is not None
            if sky != "none":           # a strided view against its contiguous copy, and every layout against every other
                _same(f"sky {sky} against its contiguous copy", base[sky], _run(T, {**cs, "sky": cs["sky"].contiguous()}, g, hh))
                _same(f"sky {sky} against dense3", base[sky], base["dense3"], sky_layouts=True)
            msky = cs["sky"]            # (the odd-strided view starts 5 (W + 3) + 1 elements into its buffer as it is)
            if sky == "view4":
                msky = FR.make_sky(_shifted(inp["sky4"]), sky)
            elif sky in ("dense3", "planes"):
                msky = _shifted(cs["sky"])
            if sky in ("view4", "dense3", "planes"):
                assert msky.data_ptr() % 16 == 4 and msky.stride() == cs["sky"].stride()
            mis = {"colors": _shifted(cs["colors"]), "alphas": _shifted(cs["alphas"]), "sky": msky,
                   "affine": None if cs["affine"] is None else _shifted(cs["affine"])}
            _same(f"misaligned inputs, sky {sky}", base[sky], _run(T, mis, _shifted(g), None if hh is None else _shifted(hh)))


@pytest.mark.parametrize("H,W", [(37, 53), (17, 241), (1024, 1025)])
def test_affine_sums_are_the_restated_order_of_additions_bit_for_bit(T, H, W):
    """The twelve sums do not depend on anything but the documented order: lane-serial over 16 pixels, 8 tree levels,
    block partials in float64 (frame_tail_ref.affine_sums_restated, fp32 host arithmetic)."""
    inp = _inputs(H, W)
    for sky in ("view4", "none"):
        cs = FR.case(inp, sky, True, 4, device=DEV)
        grads = _run(T, cs, inp["g"], None)
        want = FR.affine_sums_restated(cs["colors"], cs["alphas"], cs["sky"], inp["g"])
        assert torch.equal(grads["affine"].cpu(), want), (sky, grads["affine"].cpu() - want)


def test_no_host_wait(T):
    """Forward + backward enqueue behind a long kernel under set_sync_debug_mode("error") and raise nothing; reading a
    value back under the same mode raises, so the check is active.  That mode sees torch's own waits only, so the
    stream must also still be busy when the calls have returned: a wait inside the host entries would drain it.  The
    work in front is 200 passes reading and writing 256 MB, 12.8 ms at the 8 TB/s of the memory's specification and
    more in practice, against well under a millisecond of host work for the step."""
    inp = _inputs(1066, 1600)
    cs = FR.case(inp, "view4", True, 4, device=DEV)
    _run(T, cs, inp["g"], inp["h"])                       # warm-up: library and binding loaded
    leaves = {k: t.detach().clone().requires_grad_(True) for k, t in cs.items()}
    big = torch.ones(64 * 1024 * 1024, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        done = torch.cuda.Event()
        for _ in range(200):
            big.mul_(1.0001)                              # the stream is busy while the tail is enqueued
        out = T.frame_tail(leaves["colors"], leaves["alphas"], leaves["sky"], leaves["affine"])
        ((out.rgb * inp["g"]).sum() + (out.depth * inp["h"]).sum() + out.acc.sum()).backward()
        done.record()
        pending = not done.query()
        with pytest.raises(RuntimeError):
            float(out.rgb.detach()[0, 0, 0])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert pending, "the stream had drained when forward + backward returned: something in them waited for the GPU"
    assert all(torch.isfinite(t.grad).all() for t in leaves.values())


# ---- end to end --------------------------------------------------------------------------------------------------------
def _projected(n, seed, opacity_factor, W, H, tile):
    """A small scene through the numpy oracle's projection and tile intersection (as oracle/raster_bwd_cases.projected)."""
    import math
    import numpy as np
    from oracle import gsplat_oracle as O
    from street_crafter_amd.scenes import make_camera, make_scene
    sc = make_scene(n, seed=seed, z_range=(1.0, 20.0), scale_range=(0.02, 0.3))
    cam = make_camera(W, H, 60.0, 60.0)
    radii, m2, d, con, comp = O.fully_fused_projection(sc.means.numpy(), sc.quats.numpy(), sc.scales.numpy(), cam.viewmat.numpy(),
                                                       cam.K.numpy(), W, H, near_plane=0.001, far_plane=1000.0,
                                                       calc_compensations=True)
    op = (sc.opacities.numpy().reshape(-1) * comp * np.float32(opacity_factor)).astype(np.float32)
    tw, th = math.ceil(W / tile), math.ceil(H / tile)
    _, ids, fids = O.isect_tiles(m2[None], radii[None], d[None], tile, tw, th, n_cameras=1)
    offs = O.isect_offset_encode(ids, 1, tw, th)
    rng = np.random.default_rng(seed)
    return dict(means2d=m2[None].astype(np.float32), conics=con[None].astype(np.float32), opacities=op[None],
                colors=rng.uniform(0, 1, (1, n, 4)).astype(np.float32), isect_offsets=offs, flatten_ids=fids, width=W,
                height=H, tile_size=tile, backgrounds=None, masks=None)


def test_train_step_end_to_end(T):
    """One step at 37x53: a foreground and a sky rasterize_to_pixels, the tail, losses.l1_and_ssim + regularizers.sky_loss,
    backward -- through frame_tail and through the torch tail (tail_reference in fp32).  The gradients that reach the
    rasterizers' inputs through frame_tail are judged per row by the rasterizer tests' own bar, |x - G| <= 2^-24 (K S + A)
    with K = 4 K_ref (tests/test_raster_bwd_rows_gpu.py; G, S, A: oracle/raster_bwd_f64.py on the upstream gradients the
    torch tail hands the rasterizers, K_ref: the closed form's float32 replay on the same two passes); affine.grad by the
    affine bar against the closed form on the torch route's upstream gradient."""
    import numpy as np
    import gsplat.rendering as R
    from oracle import raster_bwd_cases as RC
    from oracle import raster_bwd_f64 as RB
    from street_crafter_amd import losses, regularizers
    W, H, tile = 53, 37, 16
    passes = {"foreground": _projected(400, 2, 0.5, W, H, tile), "sky": _projected(300, 4, 1.0, W, H, tile)}
    for p in passes.values():           # no pixel next to a threshold of the forward: every pixel takes part in the loss
        assert not RB.unstable_bwd(p["means2d"], p["conics"], p["colors"], p["opacities"], W, H, tile, p["isect_offsets"],
                                   p["flatten_ids"]).any()
    gen = torch.Generator().manual_seed(11)
    gt = torch.rand(3, H, W, generator=gen).to(DEV)
    sky_mask = (torch.rand(1, H, W, generator=gen) > 0.7).to(DEV)
    A0 = (torch.eye(3, 4) + 0.1 * torch.randn(3, 4, generator=gen)).to(DEV)
    names = ("means2d", "conics", "colors", "opacities")

    def step(tail):
        leaves, renders = {}, {}
        for key, p in passes.items():
            src = [torch.from_numpy(p[k]).to(DEV).requires_grad_(True) for k in names]
            rc, ra = R.rasterize_to_pixels(*src, W, H, tile, torch.from_numpy(p["isect_offsets"]).to(DEV, torch.int32),
                                           torch.from_numpy(p["flatten_ids"]).to(DEV, torch.int32), absgrad=True)
            rc.retain_grad()
            ra.retain_grad()
            leaves[key], renders[key] = src, (rc, ra)
        A = A0.clone().requires_grad_(True)
        rgb, acc, depth = tail(renders["foreground"][0], renders["foreground"][1], renders["sky"][0][..., :3], A)
        rgb.retain_grad()
        l1, ssim = losses.l1_and_ssim(rgb, gt)
        loss = 0.8 * l1 + 0.2 * (1.0 - ssim) + 0.05 * regularizers.sky_loss(acc, sky_mask)
        loss.backward()
        torch.cuda.synchronize()
        got = {key: {k: t.grad.cpu().numpy() for k, t in zip(names, src)} for key, src in leaves.items()}
        for key, src in leaves.items():
            got[key]["absgrad"] = src[0].absgrad.cpu().numpy()
        return got, A.grad, rgb.grad, {key: (rc, ra) for key, (rc, ra) in renders.items()}, float(loss.detach())

    hip, A_hip, _, _, loss_hip = step(lambda c, a, s, A: T.frame_tail(c, a, s, A))
    ref, A_ref, g_ref, renders, loss_ref = step(lambda c, a, s, A: FR.tail_reference(c, a, s, A))
    assert abs(loss_hip - loss_ref) <= 1e-5 * abs(loss_ref)
    outs = [k for k in RB.OUTPUTS if k != "backgrounds"]
    for key, p in passes.items():
        rc, ra = renders[key]
        v_a = np.zeros((1, H, W, 1), np.float32) if ra.grad is None else ra.grad.cpu().numpy()
        q = dict(p, v_colors=rc.grad.cpu().numpy(), v_alphas=v_a)
        f64 = RC.reference(q)
        k_ref = max(r for r, _ in RC.worst_ratios(RC.reference(q, np.float32)["G"], f64, outs).values())
        K = 4.0 * k_ref
        for tag, got in (("frame_tail", hip[key]), ("torch tail", ref[key])):
            worst = RC.worst_ratios(got, f64, outs)
            print(f"[frame_tail] end to end, {key} pass through the {tag}: " +
                  ", ".join(f"{k} {r:.1f}" for k, (r, _) in worst.items()) + f"; K_ref {k_ref:.1f}, bar {K:.1f}")
            if tag == "frame_tail":
                for k, (r, off) in worst.items():
                    assert off == 0.0 and r <= K, (key, k, r, K)
    fg, sk = renders["foreground"], renders["sky"]
    G, S = FR.tail_closed_f64(fg[0].detach(), fg[1].detach(), sk[0].detach()[..., :3], A0, g_ref, None)
    r_hip = FR.ratio(A_hip, G["affine"], S["affine"], FR.AFFINE_BAR)
    print(f"[frame_tail] end to end: affine.grad |x - G| / (32 EPS24 S): frame_tail {r_hip:.3f}, "
          f"torch tail {FR.ratio(A_ref, G['affine'], S['affine'], FR.AFFINE_BAR):.3f}")
    assert r_hip <= 1.0
