"""References, inputs and bars of the frame-tail tests (street_crafter_amd/frame_tail.py) -- TEST INFRASTRUCTURE ONLY.

    tail_reference   the reference's lines (street_gaussian_renderer.py:282-300, :116-132, color_correction.py:135-138)
                     as they stand, einsum included, in any dtype
    tail_l2r         the same values in the evaluation order of include/street_crafter_amd.h, elementwise torch ops only:
                     what the kernel must equal bit for bit in fp32
    tail_closed_f64  the closed-form gradients in float64 and, for every gradient entry, S: the sum of the absolute values
                     of its terms (a term that the clamp's mask switches off is not there)
    inputs           the inputs every test draws from

Shared by tests/test_frame_tail_cpu.py (the references against each other, torch's own fp32 against the bars) and
tests/test_frame_tail_gpu.py (the kernels against them).  Nothing in this file needs a GPU.

Bars (EPS24 = 2^-24, half an ulp of a number in [1, 2)):
  forward   |rgb - f64| <= 8 EPS24 M,  M_i = sum_j |A_ij| (|c_j| + |s_j keep|) + |A_i3|: seven rounded operations on the
            longest path (keep, s keep, c + ., three products and three sums share four levels), the eighth for second order
  per pixel |x - G| <= 16 EPS24 S: at most 12 rounded operations on any path of the closed form
  affine    |x - G| <= 32 EPS24 S: 4 roundings in a term plus at most 24 fp32 additions; the float64 stage adds nothing
"""
from __future__ import annotations

import torch

EPS24 = 2.0 ** -24
FWD_BAR, PIXEL_BAR, AFFINE_BAR = 8.0, 16.0, 32.0
SIZES = [(1, 1), (1, 3), (7, 13), (37, 53), (64, 1031), (1066, 1600)]
SKY_KINDS = ("none", "view4", "dense3", "planes", "odd")


def _clamp01(x):
    return torch.clamp(x, 0., 1.)


def tail_reference(render_colors, render_alphas, sky=None, affine=None, clamp=False):
    """-> (rgb [3,H,W], acc [1,H,W], depth [1,H,W] | None).  sky: [1,H,W,3] (a sky pass's rendered colour) or [3,H,W]
    (SkyCubeMap's sky_color)."""
    if render_colors.shape[-1] == 4:
        rendered_color = render_colors[..., :-1]
        rendered_depth = render_colors[..., -1:] / render_alphas.clamp(min=1e-10)
    else:
        rendered_color = render_colors
        rendered_depth = None
    rendered_acc = render_alphas
    if clamp:
        rendered_color = torch.clamp(rendered_color, 0., 1.)
    rgb = rendered_color[0].permute(2, 0, 1)
    acc = rendered_acc[..., 0]
    depth = None if rendered_depth is None else rendered_depth[..., 0]
    if sky is not None:
        sky_rgb = sky if sky.dim() == 3 else sky[0].permute(2, 0, 1)
        if clamp:
            sky_rgb = torch.clamp(sky_rgb, 0., 1.)
        rgb = rgb + sky_rgb * (1 - acc)
    if affine is not None:
        rgb = torch.einsum('ij, jhw -> ihw', affine[:3, :3], rgb) + affine[:3, 3].unsqueeze(-1).unsqueeze(-1)
    if clamp:
        rgb = torch.clamp(rgb, 0., 1.)
    return rgb, acc, depth


def _sky_channels(sky):
    return [sky[j] for j in range(3)] if sky.dim() == 3 else [sky[0, :, :, j] for j in range(3)]


def tail_l2r(render_colors, render_alphas, sky=None, affine=None, clamp=False):
    """The header's order, one rounded torch op per arithmetic op: keep = 1 - a; v_j = c_j + s_j keep;
    rgb_i = ((A_i0 v_0 + A_i1 v_1) + A_i2 v_2) + A_i3; depth = c_3 / max(a, 1e-10).  -> (rgb, acc, depth | None)"""
    a = render_alphas[0, :, :, 0]
    c = [render_colors[0, :, :, j] for j in range(render_colors.shape[-1])]
    keep = 1 - a
    v = [(_clamp01(c[j]) if clamp else c[j]) for j in range(3)]
    if sky is not None:
        s = _sky_channels(sky)
        v = [v[j] + (_clamp01(s[j]) if clamp else s[j]) * keep for j in range(3)]
    if affine is not None:
        v = [((affine[i, 0] * v[0] + affine[i, 1] * v[1]) + affine[i, 2] * v[2]) + affine[i, 3] for i in range(3)]
    if clamp:
        v = [_clamp01(x) for x in v]
    depth = (c[3] / a.clamp(min=1e-10))[None] if len(c) == 4 else None
    return torch.stack(v), render_alphas[..., 0], depth


def forward_scale(render_colors, render_alphas, sky=None, affine=None):
    """M [3,H,W] in float64 (see the module text)."""
    c, a = render_colors.double(), render_alphas.double()[0, :, :, 0]
    m = [c[0, :, :, j].abs() for j in range(3)]
    if sky is not None:
        s = _sky_channels(sky.double())
        m = [m[j] + (s[j] * (1 - a)).abs() for j in range(3)]
    if affine is not None:
        A = affine.double().abs()
        m = [A[i, 0] * m[0] + A[i, 1] * m[1] + A[i, 2] * m[2] + A[i, 3] for i in range(3)]
    return torch.stack(m)


def tail_closed_f64(render_colors, render_alphas, sky=None, affine=None, g=None, h=None):
    """Closed-form gradients of sum(rgb g) + sum(depth h) in float64 (g [3,H,W], h [1,H,W]; an absent one is zero).
    -> (G, S): dicts with "colors" [1,H,W,D], "alphas" [1,H,W,1], "sky" (in sky's shape; None without sky) and "affine"
    [3,4] (None without affine); S holds the sum of the absolute values of the terms of each entry."""
    D = render_colors.shape[-1]
    c, a = render_colors.double()[0], render_alphas.double()[0, :, :, 0]
    H, W = a.shape
    zero = torch.zeros(H, W, dtype=torch.float64, device=c.device)
    gg = [zero] * 3 if g is None else [g.double()[i] for i in range(3)]
    hh = zero if h is None or D == 3 else h.double()[0]
    keep = 1 - a
    s = None if sky is None else _sky_channels(sky.double())
    A = None if affine is None else affine.double()
    if A is None:
        gv, Sgv = gg, [x.abs() for x in gg]
    else:
        gv = [A[0, j] * gg[0] + A[1, j] * gg[1] + A[2, j] * gg[2] for j in range(3)]
        Sgv = [(A[0, j] * gg[0]).abs() + (A[1, j] * gg[1]).abs() + (A[2, j] * gg[2]).abs() for j in range(3)]
    m = a.clamp(min=1e-10)
    passes = (a >= 1e-10).double()
    G, S = {}, {}
    cols, Scols = list(gv), list(Sgv)
    if D == 4:
        cols.append(hh / m)
        Scols.append((hh / m).abs())
    G["colors"], S["colors"] = torch.stack(cols, -1)[None], torch.stack(Scols, -1)[None]
    da, Sa = zero.clone(), zero.clone()
    if s is not None:
        da = da - (gv[0] * s[0] + gv[1] * s[1] + gv[2] * s[2])
        Sa = Sa + Sgv[0] * s[0].abs() + Sgv[1] * s[1].abs() + Sgv[2] * s[2].abs()
    if D == 4:
        t = passes * hh * c[:, :, 3] / (m * m)
        da, Sa = da - t, Sa + t.abs()
    G["alphas"], S["alphas"] = da[None, :, :, None], Sa[None, :, :, None]
    G["sky"] = S["sky"] = None
    if s is not None:
        ds, Ss = [gv[j] * keep for j in range(3)], [Sgv[j] * keep.abs() for j in range(3)]
        if sky.dim() == 3:
            G["sky"], S["sky"] = torch.stack(ds), torch.stack(Ss)
        else:
            G["sky"], S["sky"] = torch.stack(ds, -1)[None], torch.stack(Ss, -1)[None]
    G["affine"] = S["affine"] = None
    if A is not None:
        v = [c[:, :, j] if s is None else c[:, :, j] + s[j] * keep for j in range(3)]
        Sv = [c[:, :, j].abs() if s is None else c[:, :, j].abs() + (s[j] * keep).abs() for j in range(3)]
        G["affine"] = torch.stack([torch.stack([(gg[i] * v[j]).sum() for j in range(3)] + [gg[i].sum()]) for i in range(3)])
        S["affine"] = torch.stack([torch.stack([(gg[i].abs() * Sv[j]).sum() for j in range(3)] + [gg[i].abs().sum()])
                                   for i in range(3)])
    return G, S


LANES, PIXELS_PER_LANE, PASSES, FINISH_LANES = 256, 4, 4, 256      # the kernels' shape, restated (csrc/frame_tail.hip)
FWD_BLOCK = LANES * PIXELS_PER_LANE                                 # pixels per forward block and backward pass
BWD_BLOCK = FWD_BLOCK * PASSES                                      # pixels per backward block: 16 per lane


def _tree(x):
    """Pairwise halving over the last axis (a power of two): what a butterfly of commutative additions leaves in lane 0."""
    while x.shape[-1] > 1:
        d = x.shape[-1] // 2
        x = x[..., :d] + x[..., d:]
    return x[..., 0]


def affine_sums_restated(render_colors, render_alphas, sky, g):
    """grad_affine [3,4] by the kernel's own order of additions, in fp32 torch ops on the host: every lane adds its 16
    pixels serially (pass by pass, four consecutive pixels each), 6 + 2 tree levels per block, the block partials in
    float64 (finishing lane t takes blocks t, t + 256, ...; the same tree), rounded once.  The terms are fl(g_i fl(v_j)),
    v as tail_l2r computes it."""
    c = render_colors.float().cpu()
    a = render_alphas.float().cpu()[0, :, :, 0]
    v = [c[0, :, :, j] for j in range(3)]
    if sky is not None:
        s = _sky_channels(sky.float().cpu())
        v = [v[j] + s[j] * (1 - a) for j in range(3)]
    gg = g.float().cpu()
    P = a.numel()
    nblk = -(-P // BWD_BLOCK)
    out = torch.zeros(3, 4, dtype=torch.float32)
    for i in range(3):
        for j in range(4):
            t = (gg[i] * v[j] if j < 3 else gg[i]).reshape(-1)
            t = torch.cat([t, torch.zeros(nblk * BWD_BLOCK - P)]).reshape(nblk, PASSES, LANES, PIXELS_PER_LANE)
            lane = torch.zeros(nblk, LANES)
            for ps in range(PASSES):
                for k in range(PIXELS_PER_LANE):
                    lane = lane + t[:, ps, :, k]
            waves = _tree(lane.reshape(nblk, LANES // 64, 64))
            part = ((waves[:, 0] + waves[:, 1]) + (waves[:, 2] + waves[:, 3])).double()
            pad = -(-nblk // FINISH_LANES) * FINISH_LANES
            rows = torch.cat([part, torch.zeros(pad - nblk, dtype=torch.float64)]).reshape(-1, FINISH_LANES)
            fl = torch.zeros(FINISH_LANES, dtype=torch.float64)
            for r in range(rows.shape[0]):
                fl = fl + rows[r]
            w = _tree(fl.reshape(FINISH_LANES // 64, 64))
            out[i, j] = ((w[0] + w[1]) + (w[2] + w[3])).float()
    return out


def inputs(H, W, seed):
    """CPU fp32 tensors: c [1,H,W,4] in [0, 1.2) with c_3 = a (1 + 60 u); a [1,H,W,1] uniform with 10 % exactly 0, 10 %
    exactly 1, 5 % exactly float32(1e-10) and 5 % equal to 1e-12; sky4 [1,H,W,4] in [0, 1.2); A = I + 0.1 N [3,4];
    g ~ N / (H W) [3,H,W]; h ~ 0.01 N / (H W) [1,H,W]."""
    gen = torch.Generator().manual_seed(seed)
    c = 1.2 * torch.rand(1, H, W, 4, generator=gen)
    a = torch.rand(1, H, W, 1, generator=gen)
    r = torch.rand(1, H, W, 1, generator=gen)
    a[r < 0.10] = 0.0
    a[(r >= 0.10) & (r < 0.20)] = 1.0
    a[(r >= 0.20) & (r < 0.25)] = 1e-10
    a[(r >= 0.25) & (r < 0.30)] = 1e-12
    c[..., 3:] = a * (1 + 60 * torch.rand(1, H, W, 1, generator=gen))
    sky4 = 1.2 * torch.rand(1, H, W, 4, generator=gen)
    A = torch.eye(3, 4) + 0.1 * torch.randn(3, 4, generator=gen)
    g = torch.randn(3, H, W, generator=gen) / (H * W)
    h = 0.01 * torch.randn(1, H, W, generator=gen) / (H * W)
    return {"c": c, "a": a, "sky4": sky4, "A": A, "g": g, "h": h}


def make_sky(sky4, kind):
    """The sky operand of one variant, built from sky4 [1,H,W,4] on its device; every kind holds the same values.
    "view4": the [..., :3] view of the 4-channel render; "dense3": a contiguous [1,H,W,3]; "planes": a contiguous
    [3,H,W]; "odd": a [1,H,W,3] view with strides no fast path takes (rows of W + 2 pixels of 5 channels)."""
    if kind == "none":
        return None
    if kind == "view4":
        return sky4[..., :3]
    if kind == "dense3":
        return sky4[..., :3].contiguous()
    if kind == "planes":
        return sky4[0, :, :, :3].permute(2, 0, 1).contiguous()
    if kind == "odd":
        _, H, W, _ = sky4.shape
        big = torch.zeros(1, H + 1, W + 2, 5, dtype=sky4.dtype, device=sky4.device)
        view = big[:, 1:, 1:W + 1, 1:4]
        view.copy_(sky4[..., :3])
        return view
    raise ValueError(kind)


def case(inp, sky_kind, use_affine, D, device="cpu", dtype=torch.float32):
    """-> dict(colors, alphas, sky, affine) for one variant, detached, on `device`."""
    colors = inp["c"][..., :D].to(device=device, dtype=dtype).contiguous()
    alphas = inp["a"].to(device=device, dtype=dtype)
    sky = make_sky(inp["sky4"].to(device=device, dtype=dtype), sky_kind)
    affine = inp["A"].to(device=device, dtype=dtype) if use_affine else None
    return {"colors": colors, "alphas": alphas, "sky": sky, "affine": affine}


def autograd_grads(fn, cs, g, h):
    """Gradients of sum(rgb g) + sum(depth h) through `fn` (tail_reference, tail_l2r or frame_tail) with respect to the
    four inputs of `cs`, each None where unused or absent.  -> ((rgb, acc, depth), {"colors", "alphas", "sky", "affine"})"""
    leaves = {k: (None if t is None else t.detach().requires_grad_(True)) for k, t in cs.items()}
    out = fn(leaves["colors"], leaves["alphas"], leaves["sky"], leaves["affine"])
    outs, gos = [], []
    if g is not None:
        outs.append(out[0])
        gos.append(g)
    if h is not None and out[2] is not None:
        outs.append(out[2])
        gos.append(h)
    names = [k for k, t in leaves.items() if t is not None]
    grads = torch.autograd.grad(outs, [leaves[k] for k in names], gos, allow_unused=True)
    res = {k: None for k in leaves}
    res.update(dict(zip(names, grads)))
    return tuple(None if o is None else o.detach() for o in out), res


def ratio(x, G, S, bar):
    """The largest |x - G| / (bar EPS24 S) over the entries (those with S == 0 must equal G exactly: inf otherwise)."""
    x, G, S = x.double().reshape(-1), G.double().reshape(-1), S.double().reshape(-1)
    if x.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(x).all()):
        return float("inf")
    err = (x - G).abs()
    r = torch.where(S > 0, err / (bar * EPS24 * S).clamp(min=1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    return float(r.max())


def judge_backward(tag, grads, G, S, expect_none=()):
    """Every entry of every gradient within its bar; `expect_none`: the gradients that must not have been computed."""
    worst = {}
    for k in ("colors", "alphas", "sky", "affine"):
        if k in expect_none or G[k] is None:
            assert grads[k] is None, (tag, k, "computed although nothing asked for it")
            continue
        assert grads[k] is not None, (tag, k)
        assert tuple(grads[k].shape) == tuple(G[k].shape), (tag, k, tuple(grads[k].shape), tuple(G[k].shape))
        worst[k] = ratio(grads[k], G[k], S[k], AFFINE_BAR if k == "affine" else PIXEL_BAR)
    print(f"[frame_tail] {tag}: worst |x - G| / bar: " + ", ".join(f"{k} {r:.3f}" for k, r in worst.items()))
    for k, r in worst.items():
        assert r <= 1.0, (tag, k, r)
    return worst
