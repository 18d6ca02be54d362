"""rasterize_to_pixels_layered / novel_view_frame (csrc/raster_layers.hip) against the public operators, bit for bit.

Expected images of a layer: projection, intersection and `rasterize_to_pixels` on that layer's OWN rows, through its own
tile lists (the pattern of `_separate` in tests/test_groups_gpu.py).  The layered operator sees the concatenated rows
once: one projection, one `isect_tiles` on `layered_depths`, one kernel.  Every comparison is `torch.equal`: there are no
tolerances here.  Camera: identity rotation at the origin looking down +z, fx = fy = 60, principal point centred.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = 60.0
TILE = 16
NEAR, FAR = 0.01, 1000.0


def _K(W, H):
    return torch.tensor([[F, 0.0, W / 2.0], [0.0, F, H / 2.0], [0.0, 0.0, 1.0]])


def _yaw(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    V = torch.eye(4)
    V[:3, :3] = torch.tensor([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
    return V


def _gaussians(n, W, H, seed, z=None, x_range=(-1.0, 1.0), scale=(0.02, 0.3), opac=(0.05, 0.95)):
    """means uniform in the frustum (x inside `x_range` of the half width) at depth 2..20 unless `z` is given, scales
    log-uniform, random unit quats, opacities and colours uniform."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g)
    if z is None:
        z = 2.0 + 18.0 * u(n)
    z = torch.as_tensor(z, dtype=torch.float32).expand(n).clone()
    x = (x_range[0] + (x_range[1] - x_range[0]) * u(n)) * (W / 2.0 / F) * z
    y = (u(n) * 2 - 1) * (H / 2.0 / F) * z
    means = torch.stack([x, y, z], -1)
    scales = torch.exp(math.log(scale[0]) + (math.log(scale[1]) - math.log(scale[0])) * u(n, 3))
    quats = torch.randn(n, 4, generator=g)
    quats = quats / quats.norm(dim=-1, keepdim=True)
    return means, quats, scales, opac[0] + (opac[1] - opac[0]) * u(n), u(n, 3)


def _covering(n, z, opacity, seed):
    """Gaussians centred on the 16x16 image's tile that cover all of it: 1.5 world units wide at any depth <= 20."""
    g = torch.Generator().manual_seed(seed)
    z = torch.as_tensor(z, dtype=torch.float32).expand(n).clone()
    xy = (torch.rand(n, 2, generator=g) * 2 - 1) * 0.05
    means = torch.cat([xy * z[:, None] / 10.0, z[:, None]], -1)
    scales = 1.5 + torch.rand(n, 3, generator=g)
    quats = torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(n, 4).clone()
    return means, quats, scales, torch.as_tensor(opacity, dtype=torch.float32).expand(n).clone(), torch.rand(n, 3, generator=g)


def _cat(a, b):
    return tuple(torch.cat([s, t]) for s, t in zip(a, b))


def _front_ops(means, quats, scales, opac, rgb, viewmats, W, H, D, n_front=None):
    """The public operators in front of the rasterizer -> its arguments; with `n_front` the sort keys are layered."""
    from gsplat.rendering import fully_fused_projection, isect_offset_encode, isect_tiles
    from street_crafter_amd.layers import layered_depths
    C = viewmats.shape[0]
    Ks = _K(W, H).to(DEV)[None].expand(C, -1, -1).contiguous()
    radii, means2d, depths, conics, _ = fully_fused_projection(means, None, quats, scales, viewmats, Ks, W, H,
                                                               packed=False, near_plane=NEAR, far_plane=FAR)
    tw, th = math.ceil(W / TILE), math.ceil(H / TILE)
    keys = depths if n_front is None else layered_depths(depths, n_front)
    _, isect_ids, flatten_ids = isect_tiles(means2d, radii, keys, TILE, tw, th, packed=False, n_cameras=C)
    isect_offsets = isect_offset_encode(isect_ids, C, tw, th)
    colors = rgb[None].expand(C, -1, -1)
    if D == 4:
        colors = torch.cat((colors, depths[..., None]), dim=-1)
    flatten_ids = flatten_ids.plain() if hasattr(flatten_ids, "plain") else flatten_ids
    return means2d, conics, colors.contiguous(), opac[None].expand(C, -1).contiguous(), isect_offsets, flatten_ids


def _separate(gauss, viewmats, W, H, D):
    """rasterize_to_pixels on `gauss` through its own projection and intersection; zeros for an empty set."""
    from gsplat.rendering import rasterize_to_pixels
    C = viewmats.shape[0]
    if gauss[0].shape[0] == 0:
        return torch.zeros(C, H, W, D, device=DEV), torch.zeros(C, H, W, 1, device=DEV)
    m2, cn, col, op, offs, fids = _front_ops(*gauss, viewmats, W, H, D)
    return rasterize_to_pixels(m2, cn, col, op, W, H, TILE, offs, fids, backgrounds=None, packed=False)


def _case(front, back, W, H, D, viewmats=None):
    """-> dict: the layered operator's outputs, its inputs, and the expected images from the two separate renders."""
    from street_crafter_amd.layers import rasterize_to_pixels_layered
    viewmats = (torch.eye(4)[None] if viewmats is None else viewmats).to(DEV).contiguous()
    front = tuple(t.to(DEV).contiguous() for t in front)
    back = tuple(t.to(DEV).contiguous() for t in back)
    n_front = front[0].shape[0]
    with torch.no_grad():
        args = _front_ops(*_cat(front, back), viewmats, W, H, D, n_front=n_front)
        fc, fa, bc, ba, lb = rasterize_to_pixels_layered(*args[:4], W, H, TILE, *args[4:], n_front,
                                                         return_layer_begin=True)
        out = dict(fc=fc, fa=fa, bc=bc, ba=ba, lb=lb, args=args, n_front=n_front, N=n_front + back[0].shape[0],
                   W=W, H=H, D=D, viewmats=viewmats, front=front, back=back)
        out["ref_front"] = _separate(front, viewmats, W, H, D)
        out["ref_back"] = _separate(back, viewmats, W, H, D)
    return out


def _check(o):
    C = o["viewmats"].shape[0]
    H, W, D = o["H"], o["W"], o["D"]
    assert o["fc"].shape == (C, H, W, D) and o["fa"].shape == (C, H, W, 1)
    assert o["bc"].shape == (C, H, W, 3) and o["ba"].shape == (C, H, W, 1)
    assert all(o[k].dtype == torch.float32 and o[k].is_contiguous() for k in ("fc", "fa", "bc", "ba"))
    assert torch.equal(o["fc"], o["ref_front"][0]), "front colours differ from the front layer's own render"
    assert torch.equal(o["fa"], o["ref_front"][1]), "front alphas differ from the front layer's own render"
    assert torch.equal(o["bc"], o["ref_back"][0][..., :3]), "back colours differ from the back layer's own render"
    assert torch.equal(o["ba"], o["ref_back"][1]), "back alphas differ from the back layer's own render"
    _check_layer_begin(o)


def _check_layer_begin(o):
    """`layer_begin` is the first position of each tile's list whose Gaussian is a back row (the list's end if none)."""
    offs, fids = o["args"][4], o["args"][5]
    starts = offs.reshape(-1).to(torch.int64)
    ends = torch.cat([starts[1:], torch.tensor([fids.numel()], device=DEV)])
    tiles_per_cam = offs.shape[1] * offs.shape[2]
    cam = torch.arange(starts.numel(), device=DEV) // tiles_per_cam
    pos = torch.arange(fids.numel(), device=DEV)
    tile_of = torch.searchsorted(ends, pos, right=True)                # the number of lists that end at or before it
    is_back = (fids.to(torch.int64) - cam[tile_of] * o["N"]) >= o["n_front"]
    want = ends.clone()
    back_pos = pos[is_back]
    want.scatter_reduce_(0, tile_of[is_back], back_pos, reduce="amin")
    assert torch.equal(o["lb"].to(torch.int64), want)


@pytest.fixture(scope="module")
def mixed():
    W, H = 64, 48
    return {D: _case(_gaussians(600, W, H, 1), _gaussians(60, W, H, 2), W, H, D) for D in (4, 3)}


@pytest.mark.parametrize("D", [4, 3])
def test_mixed_layers_equal_their_own_renders(mixed, D):
    o = mixed[D]
    _check(o)
    assert o["fa"].max() > 0.5 and o["ba"].max() > 0.2 and (o["lb"] < o["args"][5].numel()).any()


def test_back_layer_nearer_than_the_front_layer():
    W, H = 64, 48
    g = torch.Generator().manual_seed(5)
    o = _case(_gaussians(400, W, H, 3, z=5.0 + 0.5 * torch.rand(400, generator=g)),
              _gaussians(50, W, H, 4, z=1.0 + 0.2 * torch.rand(50, generator=g), scale=(0.01, 0.05)), W, H, 4)
    _check(o)
    assert o["ba"].max() > 0.2


def test_front_wall_does_not_hide_the_back_layer_from_its_own_image():
    # three opaque front Gaussians cover the single tile: the front set terminates inside the first batch, 300 more front
    # records follow, then the 5 back records -- which the back image must still show
    W = H = 16
    wall = _covering(3, [2.0, 2.1, 2.2], 0.999, 11)
    behind = _covering(300, 3.0 + torch.arange(300) * 0.05, 0.5, 12)
    back = _covering(5, [4.0, 2.5, 30.0, 1.0, 6.0], 0.3, 13)
    o = _case(_cat(wall, behind), back, W, H, 4)
    _check(o)
    assert int(o["lb"][0]) == 303 and o["fa"].min() > 0.98 and o["ba"].min() > 0.3
    # the mirror: an opaque back wall followed by 200 more back records
    o = _case(_covering(40, 3.0 + torch.arange(40) * 0.1, 0.05, 14),
              _cat(_covering(3, [2.0, 2.1, 2.2], 0.999, 15), _covering(200, 3.0 + torch.arange(200) * 0.05, 0.5, 16)), W, H, 3)
    _check(o)
    assert int(o["lb"][0]) == 40 and o["ba"].min() > 0.98 and 0.1 < o["fa"].max() < 0.99


@pytest.mark.parametrize("nf,nb", [(63, 1), (64, 1), (65, 1), (64, 64), (128, 65), (1, 200), (0, 70), (70, 0)])
def test_boundary_against_the_batch_size(nf, nb):
    # one tile, every Gaussian covers it, none opaque enough to terminate a pixel: both runs are walked to their ends
    W = H = 16
    g = torch.Generator().manual_seed(100 + nf + nb)
    front = _covering(nf, 2.0 + 10.0 * torch.rand(nf, generator=g), 0.01 + 0.01 * torch.rand(nf, generator=g), nf)
    back = _covering(nb, 2.0 + 10.0 * torch.rand(nb, generator=g), 0.01 + 0.01 * torch.rand(nb, generator=g), 1000 + nb)
    o = _case(front, back, W, H, 4)
    _check(o)
    assert o["args"][5].numel() == nf + nb and int(o["lb"][0]) == nf
    assert (o["fa"].max() > 0) == (nf > 0) and (o["ba"].max() > 0) == (nb > 0) and o["fa"].max() < 0.99


def test_tiles_with_one_layer_or_none_and_absent_layers():
    W, H = 96, 32          # 6 x 2 tiles: front only on the left, back only on the right, nothing in the middle
    front = _gaussians(150, W, H, 21, x_range=(-0.98, -0.45), scale=(0.01, 0.03))
    back = _gaussians(40, W, H, 22, x_range=(0.45, 0.98), scale=(0.01, 0.03))
    o = _case(front, back, W, H, 4)
    _check(o)
    counts = torch.diff(torch.cat([o["args"][4].reshape(-1), torch.tensor([o["args"][5].numel()], device=DEV)]))
    assert (counts == 0).any() and o["fa"][..., 64:, :].max() == 0 and o["ba"][..., :32, :].max() == 0
    assert o["fa"].max() > 0 and o["ba"].max() > 0
    # no back layer at all: the plain render, and a zero back image; no front layer: the mirror
    both = _cat(_gaussians(300, 64, 48, 23), _gaussians(30, 64, 48, 24))
    none = tuple(t[:0] for t in both)
    o = _case(both, none, 64, 48, 4)
    _check(o)
    assert not o["bc"].any() and not o["ba"].any() and o["fa"].max() > 0.5
    o = _case(none, both, 64, 48, 4)
    _check(o)
    assert not o["fc"].any() and not o["fa"].any() and o["ba"].max() > 0.5


@pytest.mark.parametrize("D", [4, 3])
def test_partial_tiles(D):
    W, H = 70, 45
    _check(_case(_gaussians(500, W, H, 31), _gaussians(60, W, H, 32), W, H, D))


def test_ties_inside_and_across_the_layers():
    W, H = 64, 48
    g = torch.Generator().manual_seed(41)
    zf = torch.tensor([3.0, 5.0, 8.0])[torch.randint(0, 3, (300,), generator=g)]
    zb = torch.tensor([3.0, 5.0, 40.0])[torch.randint(0, 3, (50,), generator=g)]
    _check(_case(_gaussians(300, W, H, 42, z=zf), _gaussians(50, W, H, 43, z=zb), W, H, 4))


def test_two_cameras():
    W, H = 64, 48
    o = _case(_gaussians(500, W, H, 51), _gaussians(60, W, H, 52), W, H, 4, viewmats=torch.stack([torch.eye(4), _yaw(8.0)]))
    _check(o)
    assert o["fa"][1].max() > 0.5 and o["ba"][1].max() > 0.1 and not torch.equal(o["fc"][0], o["fc"][1])


def test_dead_entries_in_the_front_run(mixed):
    """Ids outside [0, C*N) in a tile's front run are blended into nothing and count as front for the boundary.  The
    reference is the front layer's own render from its own list with the same positions edited."""
    from gsplat.rendering import rasterize_to_pixels
    from street_crafter_amd.layers import rasterize_to_pixels_layered
    o = mixed[4]
    W, H, n_front, N = o["W"], o["H"], o["n_front"], o["N"]
    m2, cn, col, op, offs, fids = o["args"]
    starts = offs.reshape(-1).tolist()
    lb = o["lb"].tolist()
    tile = max(range(len(starts)), key=lambda t: lb[t] - starts[t])
    assert lb[tile] - starts[tile] >= 8
    edits = {1: -1, 3: N, 6: -7, lb[tile] - starts[tile] - 1: 2 ** 31 - 1}       # offset in the front run -> dead id
    with torch.no_grad():
        fm2, fcn, fcol, fop, foffs, ffids = _front_ops(*o["front"], o["viewmats"], W, H, 4)
        fstart = foffs.reshape(-1).tolist()[tile]
        assert torch.equal(ffids[fstart:fstart + 8], fids[starts[tile]:starts[tile] + 8])
        fids_e, ffids_e = fids.clone(), ffids.clone()
        for k, dead in edits.items():
            fids_e[starts[tile] + k] = dead
            ffids_e[fstart + k] = dead if dead != N else n_front       # (N is a live row of nothing in the front's own set)
        fc, fa, bc, ba, lb_e = rasterize_to_pixels_layered(m2, cn, col, op, W, H, TILE, offs, fids_e, n_front,
                                                           return_layer_begin=True)
        ref_c, ref_a = rasterize_to_pixels(fm2, fcn, fcol, fop, W, H, TILE, foffs, ffids_e, backgrounds=None, packed=False)
    assert torch.equal(lb_e, o["lb"])
    assert torch.equal(fc, ref_c) and torch.equal(fa, ref_a)
    assert torch.equal(bc, o["bc"]) and torch.equal(ba, o["ba"])
    ty, tx = divmod(tile, offs.shape[2])
    inside = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    inside[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    assert torch.equal(fc[0][~inside], o["fc"][0][~inside]) and not torch.equal(fc[0][inside], o["fc"][0][inside])


def _frame(o, epilogue, rounding=0, out=None):
    from street_crafter_amd import _lib
    from street_crafter_amd.isect import _stream
    m2, cn, col, op, offs, fids = o["args"]
    return _lib.binding().rasterize_fwd_layers(m2, cn, col, op, o["n_front"], o["W"], o["H"], TILE,
                                               offs.as_subclass(torch.Tensor), fids, epilogue, rounding, False, out,
                                               _stream(m2))


@pytest.mark.parametrize("D", [4, 3])
def test_frame_epilogues(mixed, D):
    from street_crafter_amd.dist import to_uint8_frame
    o = mixed[D]
    (f_c, f_a), (b_c, _) = o["ref_front"], o["ref_back"]
    rc, rgb, acc, depth, unused, lb = _frame(o, 1)
    assert rc == 0 and unused is None and lb is None
    want = torch.clamp(torch.clamp(f_c[..., :3], 0.0, 1.0) + torch.clamp(b_c[..., :3], 0.0, 1.0) * (1 - f_a), 0.0, 1.0)
    assert torch.equal(rgb, want) and torch.equal(acc, f_a)
    assert 0.01 < float((want > torch.clamp(f_c[..., :3], 0.0, 1.0)).float().mean())       # the back layer shows through
    if D == 4:
        assert torch.equal(depth, f_c[..., 3:] / f_a.clamp(min=1e-10))
    else:
        assert depth is None
    for rounding, code in (("video", 0), ("save_image", 1)):
        rc, u8, *rest = _frame(o, 2, code)
        assert rc == 0 and u8.dtype == torch.uint8 and u8.shape == (1, o["H"], o["W"], 3) and rest[:3] == [None] * 3
        two_pass = to_uint8_frame(f_c[0, ..., :3].permute(2, 0, 1), acc=f_a[0, ..., 0],
                                  sky_rgb_chw=b_c[0, ..., :3].permute(2, 0, 1), rounding=rounding)
        assert torch.equal(u8[0], two_pass)
    assert not torch.equal(_frame(o, 2, 0)[1], _frame(o, 2, 1)[1])
    slot = torch.zeros(o["H"], o["W"], 3, dtype=torch.uint8, device=DEV)
    assert _frame(o, 2, 0, slot)[1].data_ptr() == slot.data_ptr() and torch.equal(slot, _frame(o, 2, 0)[1][0])


def test_frame_epilogue_on_partial_tiles():
    # a width that is no multiple of 4: the epilogue's per-pixel stores instead of the 12-value ones
    from street_crafter_amd.dist import to_uint8_frame
    W, H = 70, 45
    o = _case(_gaussians(500, W, H, 61), _gaussians(80, W, H, 62), W, H, 4)
    (f_c, f_a), (b_c, _) = o["ref_front"], o["ref_back"]
    _, rgb, acc, depth, _, _ = _frame(o, 1)
    want = torch.clamp(torch.clamp(f_c[..., :3], 0.0, 1.0) + torch.clamp(b_c[..., :3], 0.0, 1.0) * (1 - f_a), 0.0, 1.0)
    assert torch.equal(rgb, want) and torch.equal(acc, f_a) and torch.equal(depth, f_c[..., 3:] / f_a.clamp(min=1e-10))
    two_pass = to_uint8_frame(f_c[0, ..., :3].permute(2, 0, 1), acc=f_a[0, ..., 0],
                              sky_rgb_chw=b_c[0, ..., :3].permute(2, 0, 1), rounding="video")
    assert torch.equal(_frame(o, 2, 0)[1][0], two_pass)


def test_both_binding_routes_give_identical_tensors(mixed):
    from street_crafter_amd import _ctypes_binding, _lib
    from street_crafter_amd.layers import rasterize_to_pixels_layered
    o = mixed[4]
    m2, cn, col, op, offs, fids = o["args"]
    assert _lib.fast() is not None and _lib.binding() is _lib.fast()
    prev = _lib.set_fast_binding(False)
    try:
        assert _lib.binding() is _ctypes_binding
        got = rasterize_to_pixels_layered(m2, cn, col, op, o["W"], o["H"], TILE, offs, fids, o["n_front"],
                                          return_layer_begin=True)
        frames = [_frame(o, 1), _frame(o, 2, 1)]
    finally:
        _lib.set_fast_binding(prev)
    for a, b in zip(got, (o["fc"], o["fa"], o["bc"], o["ba"], o["lb"])):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for slow, fast in zip(frames, [_frame(o, 1), _frame(o, 2, 1)]):
        assert slow[0] == fast[0] == 0
        for a, b in zip(slow[1:], fast[1:]):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b))


def test_novel_view_frame_equals_the_two_pass_frame():
    from harness.caller import render_novel_view, render_novel_view_u8
    from street_crafter_amd.layers import novel_view_frame
    from street_crafter_amd.scenes import make_camera, make_street_scene
    W, H = 160, 96
    fg, sky = make_street_scene(4096, n_sky=256)
    fg, sky, cam = fg.to(DEV), sky.to(DEV), make_camera(W, H, 2050.0 * W / 1920.0, 2050.0 * W / 1920.0).to(DEV)
    cat = lambda name: torch.cat([getattr(fg, name), getattr(sky, name)]).contiguous()
    args = (cat("means"), cat("quats"), cat("scales"), cat("opacities").reshape(-1), cat("sh"), cam.viewmat, cam.K, W, H,
            fg.means.shape[0])
    kw = dict(near_plane=cam.znear, far_plane=cam.zfar, sh_degree=fg.sh_degree, camera_center=cam.camera_center)
    with torch.no_grad():
        ref = render_novel_view(fg, sky, cam)
    for rounding in ("video", "save_image"):
        want = render_novel_view_u8(fg, sky, cam, rounding=rounding, fused=True)
        got = novel_view_frame(*args, **kw, output="u8", rounding=rounding)
        assert got.shape == (H, W, 3) and got.dtype == torch.uint8 and torch.equal(got, want)
    assert want.float().std() > 1 and ref["_sky"]["acc"].max() > 0.5 and ref["acc"].min() < 0.5       # a frame with a visible sky
    slot = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    assert novel_view_frame(*args, **kw, output="u8", rounding="save_image", out=slot) is not None and torch.equal(slot, want)
    # the frame does not depend on the lift: the default is the smallest the planes allow, 2^64 is the largest accepted
    assert torch.equal(novel_view_frame(*args, **kw, output="u8", rounding="save_image", lift=2.0 ** 64), want)
    out = novel_view_frame(*args, **kw)
    assert out["rgb"].shape == (3, H, W) and torch.equal(out["rgb"], ref["rgb"])
    assert torch.equal(out["acc"], ref["acc"]) and torch.equal(out["depth"], ref["depth"])
    # the camera centre derived from the view matrix gives a frame too (not compared bit for bit: another centre)
    kw.pop("camera_center")
    assert novel_view_frame(*args, **kw, output="u8").shape == (H, W, 3)
