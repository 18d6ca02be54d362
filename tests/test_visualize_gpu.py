"""Visualizer frames on the GPU (street_crafter_amd/visualize.py, csrc/frame_viz.hip) against the numpy restatement of
the reference's visualizer lines (tests/visualize_ref.py): every output byte equal, every range bit-equal.

Sizes: the block is 256 lanes x 4 pixels = 1024 pixels per step and a launch has at most 1024 blocks, so 1023 / 1025
sit on either side of one block, n mod 4 != 0 takes the scalar tail, and MAXN = 1024 * 1024 + 1024 pixels is the one
count that fills every block partial and sends block 0 round the grid-stride loop once more."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visualize_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAXN = 1024 * 1024 + 1024
COUNTS = [(1, 1), (1, 3), (1, 4), (1, 5), (1, 255), (1, 256), (1, 257), (1, 1023), (1, 1025), (37, 53), (1, MAXN)]


def _V():
    from street_crafter_amd import visualize
    return visualize


def _luts():
    g = np.random.default_rng(7)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1).copy()
    rand = g.integers(0, 256, size=(256, 3), dtype=np.uint8)
    return {"ramp": ramp, "rand": rand}


LUTS = _luts()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _layouts(v):
    """v float32 [H,W] -> {name: device view with those values}: dense and aligned; the [..., 3] view of an [H,W,4]
    render; dense from a base pointer one float past an aligned address."""
    H, W = v.shape
    t = _dev(v)
    four = torch.full((H, W, 4), -7.0, device=DEV)
    four[..., 3] = t
    off = torch.full((H * W + 1,), -7.0, device=DEV)
    off[1:] = t.reshape(-1)
    out = {"dense": t, "hwc4": four[..., 3], "offset": off[1:].view(H, W)}
    assert out["dense"].data_ptr() % 16 == 0 and out["offset"].data_ptr() % 16 == 4 and out["hwc4"].stride() == (4 * W, 4)
    return out


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


def _check_map(v, lut_name="rand", layouts=("dense", "hwc4", "offset")):
    V = _V()
    lut = LUTS[lut_name]
    want_range = R.value_range(v)
    want = R.colorize(v, lut)
    dl = _dev(lut)
    for name, t in _layouts(v).items():
        if name not in layouts:
            continue
        got_range = V.value_range(t).cpu().numpy()
        assert _bits(got_range) == _bits(want_range), (name, got_range, want_range)
        got = V.colorize(t, dl).cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.uint8
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _depth(H, W, seed, lo=0.5, hi=80.0, holes=True):
    g = np.random.default_rng(seed)
    v = g.uniform(lo, hi, size=(H, W)).astype(np.float32)
    if holes and H * W > 8:
        v[g.random((H, W)) < 0.05] = 0.0                # pixels no Gaussian reached: below mi, a wrapped table entry
    return v


@pytest.mark.parametrize("H,W", COUNTS)
def test_pixel_counts_and_layouts(H, W):
    _check_map(_depth(H, W, H * W), "rand" if (H * W) % 2 else "ramp")


@pytest.mark.parametrize("n", [2053, MAXN + 5])
def test_range_placement(n):
    """The extremes alone in the first and the last pixel (a dropped tail or block partial shows here), a denormal minimum,
    every special value, no positive pixel, a constant map."""
    base = _depth(1, n, n, 2.0, 3.0, holes=False)
    cases = {}
    a = base.copy(); a[0, -1] = 1.0; a[0, 0] = 10.0
    cases["min last, max first"] = a
    a = base.copy(); a[0, 0] = 1.0; a[0, -1] = 10.0
    cases["min first, max last"] = a
    a = base.copy(); a[0, n // 2] = np.float32(1e-45); a[0, 7] = 0.0
    cases["denormal min"] = a
    a = base.copy()
    a[0, 1::7] = 0.0; a[0, 2::11] = -4.5; a[0, 3::13] = np.nan; a[0, 5] = np.inf; a[0, -2] = -np.inf; a[0, 9] = np.float32(3e-39)
    cases["specials"] = a
    a = np.zeros((1, n), np.float32); a[0, 1::3] = -2.0; a[0, 2::5] = np.nan; a[0, 4] = -np.inf
    cases["no positive"] = a
    cases["constant"] = np.full((1, n), 7.5, np.float32)
    for name, v in cases.items():
        mi, ma = R.value_range(v)
        if name == "no positive":
            assert mi == 0 and ma == 0
        if name == "denormal min":
            assert 0 < mi < np.finfo(np.float32).tiny
        if name == "specials":
            assert ma == np.finfo(np.float32).max and mi == np.float32(3e-39)
        _check_map(v, "ramp", layouts=("dense", "hwc4") if n < 10000 else ("dense",))


@pytest.mark.parametrize("d", [7, 25, 41, 55])
def test_division_is_true_division_with_separate_rounding(d):
    """v = 1 + j on j = 0..d: a reciprocal-multiply changes 4 / 1 / 5 bytes at d = 25 / 41 / 55, a prescaled
    j * (255 / den) one byte at d = 7 and one at d = 41; true division with every operation rounded matches numpy."""
    v = (1.0 + np.arange(d + 1, dtype=np.float32))[None]
    _check_map(v, "ramp")
    _check_map(np.tile(v, (3, 1)), "rand")


def test_callers_range_and_joined_frames():
    V = _V()
    a, b = _depth(37, 53, 1), _depth(37, 53, 2, 20.0, 200.0)
    ta, tb = _dev(a), _dev(b)
    lut = LUTS["ramp"]
    dl = _dev(lut)
    # pixels below mi and above ma wrap: floats, and a device pair
    for mm in ((10.0, 40.0), (3.25, 3.5)):
        want = R.colorize(a, lut, minmax=mm)
        assert len(np.unique(want)) > 100                      # (the wrap rule is exercised: far more than 0..255 once)
        assert np.array_equal(V.colorize(ta, dl, minmax=mm).cpu().numpy(), want)
        pair = torch.tensor(mm, dtype=torch.float32, device=DEV)
        assert np.array_equal(V.colorize(ta, dl, minmax=pair).cpu().numpy(), want)
    # frames joined side by side (concat_cameras): one range, the min of the mins and the max of the maxes
    ra, rb = V.value_range(ta), V.value_range(tb)
    joined_np = np.concatenate([a, b], axis=1)
    joined = V.value_range(_dev(joined_np))
    mm = torch.stack([torch.minimum(ra[0], rb[0]), torch.maximum(ra[1], rb[1])])
    assert torch.equal(joined, mm) and _bits(joined.cpu().numpy()) == _bits(R.value_range(joined_np))
    want = R.colorize(joined_np, lut)
    halves = torch.cat([V.colorize(ta, dl, minmax=mm), V.colorize(tb, dl, minmax=mm)], dim=1)
    assert np.array_equal(halves.cpu().numpy(), want)
    # out= is written in place and returned
    slot = torch.zeros(2, 37, 53, 3, dtype=torch.uint8, device=DEV)
    ret = V.colorize(ta, dl, out=slot[1])
    assert ret.data_ptr() == slot[1].data_ptr() and np.array_equal(slot[1].cpu().numpy(), R.colorize(a, lut))
    assert not slot[0].any()


def _images(H, W, seed):
    g = np.random.default_rng(seed)
    rgb = g.uniform(0, 1, size=(3, H, W)).astype(np.float32)
    gt = np.clip(rgb + g.normal(0, 0.2, size=(3, H, W)), 0, 1).astype(np.float32)
    return rgb, gt


def _image_layouts(x):
    """[3,H,W] values as planes, planes from an unaligned base, and permuted views of [H,W,3] / [H,W,4] renders."""
    _, H, W = x.shape
    t = _dev(x)
    off = torch.zeros(3 * H * W + 1, device=DEV)
    off[1:] = t.reshape(-1)
    four = torch.full((H, W, 4), 9.0, device=DEV)
    four[..., :3] = t.permute(1, 2, 0)
    return {"planes": t, "planes_offset": off[1:].view(3, H, W), "hwc3": t.permute(1, 2, 0).contiguous().permute(2, 0, 1),
            "hwc4": four.permute(2, 0, 1)[:3]}


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (37, 53), (1, 1025), (4, 1024)])
def test_diff_maps(H, W):
    V = _V()
    rgb, gt = _images(H, W, H * W)
    g = np.random.default_rng(H + W)
    some = g.random((H, W)) < 0.7
    hidden = np.argwhere(~some)
    if len(hidden):
        rgb[0, hidden[0][0], hidden[0][1]] = np.nan             # (hidden by the mask; shown without one)
    lut = LUTS["rand"]
    dl = _dev(lut)
    for mname, mask in (("none", None), ("some", some), ("all false", np.zeros((H, W), bool))):
        m = R.diff_map(rgb, gt, mask)
        want_range, want = R.value_range(m), R.colorize(m, lut)
        for (ln, r), (_, t) in zip(_image_layouts(rgb).items(), _image_layouts(gt).items()):
            for dm in ((None,) if mask is None else (_dev(mask), _dev(mask)[None], _dev(mask.astype(np.uint8)))):
                got_range = V.diff_range(r, t, dm).cpu().numpy()
                assert _bits(got_range) == _bits(want_range), (mname, ln, got_range, want_range)
                got = V.colorize_diff(r, t, dl, mask=dm).cpu().numpy()
                assert np.array_equal(got, want), (mname, ln, int((got != want).sum()))
    # mixed layouts and a caller's range
    r, t = _image_layouts(rgb)["hwc4"], _image_layouts(gt)["planes"]
    m = R.diff_map(rgb, gt, some)
    assert np.array_equal(V.colorize_diff(r, t, dl, mask=_dev(some), minmax=(0.01, 0.05)).cpu().numpy(),
                          R.colorize(m, lut, minmax=(0.01, 0.05)))


def test_grey_maps():
    V = _V()
    vals = [0.0, 1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 1.004, 1.01, -0.0, -0.01, 2.0, np.nan, np.inf, -np.inf, 1e10, -1e10]
    vals += [k / 255 for k in range(256)] + [np.float32(k) / np.float32(255) for k in range(256)]
    a = np.array(vals, dtype=np.float32)
    for n in (len(a), len(a) - 1, 5, 1):
        v = a[:n][None]
        want = R.gray(v)
        for t in (_dev(v), _dev(v)[None], _dev(v)[..., None], _layouts(v)["offset"], _layouts(v)["hwc4"]):
            got = V.gray_u8(t)              # ([1,n,1] reads as n rows of one pixel: the same pixels in the same order)
            assert got.shape in ((1, n, 1), (n, 1, 1)) and np.array_equal(got.cpu().numpy().reshape(1, n, 1), want)
    g = np.random.default_rng(3)
    v = g.uniform(0, 1, size=(37, 53)).astype(np.float32)
    slot = torch.zeros(37, 53, 1, dtype=torch.uint8, device=DEV)
    assert V.gray_u8(_dev(v), out=slot) is slot and np.array_equal(slot.cpu().numpy(), R.gray(v))
    assert np.array_equal(V.gray_u8(_dev(v > 0.5)).cpu().numpy(), R.gray((v > 0.5).astype(np.float32)))


def _result(H, W, seed):
    """A synthetic render as the rasterizers hand it over: [H,W,4] colour + depth behind permuted views, planes for the
    background / object images, [1,H,W] accumulations."""
    g = np.random.default_rng(seed)
    rgb, gt = _images(H, W, seed)
    depth = _depth(H, W, seed + 1)
    four = torch.empty(H, W, 4, device=DEV)
    four[..., :3] = _dev(rgb).permute(1, 2, 0)
    four[..., 3] = _dev(depth)
    np_res = {"rgb": rgb, "depth": depth, "acc": g.uniform(0, 1, (H, W)).astype(np.float32),
              "rgb_background": g.uniform(0, 1, (3, H, W)).astype(np.float32),
              "rgb_object": g.uniform(0, 1, (3, H, W)).astype(np.float32),
              "acc_object": g.uniform(0, 1, (H, W)).astype(np.float32)}
    res = {"rgb": four.permute(2, 0, 1)[:3], "depth": four.permute(2, 0, 1)[3:4], "acc": _dev(np_res["acc"])[None],
           "rgb_background": _dev(np_res["rgb_background"]), "rgb_object": _dev(np_res["rgb_object"]),
           "acc_object": _dev(np_res["acc_object"])[None]}
    mask = g.random((H, W)) < 0.8
    return res, np_res, gt, mask, four


def test_whole_frame_functions():
    from street_crafter_amd.dist import to_uint8_frame
    V = _V()
    H, W = 64, 96
    res, ref, gt, mask, four = _result(H, W, 11)
    before = {k: v.clone() for k, v in res.items()}
    four_before = four.clone()
    jet, turbo = LUTS["rand"], LUTS["ramp"]
    djet, dturbo = _dev(jet), _dev(turbo)
    # visualize_novel_view + summarize(), one camera
    want = {"rgb": R.rgb_u8(ref["rgb"]), "acc": R.gray(ref["acc"]), "depth": R.colorize(ref["depth"], jet)}
    got = V.novel_view_frames(res, djet)
    assert sorted(got) == ["acc", "depth", "rgb"]
    for k in want:
        assert got[k].dtype == torch.uint8 and np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert torch.equal(got["rgb"], to_uint8_frame(res["rgb"]))
    assert torch.equal(V.novel_view_frames(res, djet, rounding="save_image")["rgb"], to_uint8_frame(res["rgb"], rounding="save_image"))
    ring = torch.zeros(3, H, W, 3, dtype=torch.uint8, device=DEV)
    acc_slot = torch.zeros(H, W, 1, dtype=torch.uint8, device=DEV)
    again = V.novel_view_frames(res, djet, out={"rgb": ring[0], "depth": ring[2], "acc": acc_slot})
    assert again["rgb"].data_ptr() == ring[0].data_ptr() and again["depth"].data_ptr() == ring[2].data_ptr()
    assert again["acc"] is acc_slot and not ring[1].any()
    for k in want:
        assert torch.equal(again[k], got[k])
    # visualize() + summarize(), one camera
    diff = R.diff_map(ref["rgb"], gt, mask)
    want = {"rgb": R.rgb_u8(ref["rgb"]), "rgb_background": R.rgb_u8(ref["rgb_background"]),
            "rgb_object": R.rgb_u8(ref["rgb_object"]), "acc_object": R.gray(ref["acc_object"]),
            "depth": R.colorize(ref["depth"], jet), "diff": R.colorize(diff, turbo)}
    dgt, dmask = _dev(gt), _dev(mask)[None]
    got = V.trajectory_frames(res, dgt, dmask, djet, dturbo)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    slots = {k: torch.zeros_like(v) for k, v in got.items()}
    again = V.trajectory_frames(res, dgt, dmask, djet, dturbo, out=slots)
    for k in want:
        assert again[k] is slots[k] and torch.equal(slots[k], got[k]), k
    nomask = V.trajectory_frames(res, dgt, None, djet, dturbo)
    assert np.array_equal(nomask["diff"].cpu().numpy(), R.colorize(R.diff_map(ref["rgb"], gt), turbo))
    # inputs are unchanged
    for k, v in before.items():
        assert torch.equal(res[k], v), k
    assert torch.equal(four, four_before)


def test_full_size_frame():
    g = np.random.default_rng(5)
    v = g.uniform(1.5, 81.5, size=(1280, 1920)).astype(np.float32)
    _check_map(v, "rand", layouts=("dense",))


# ---- guard zones: each entry point with every buffer between guards, under both fills -----------------------------------------
def test_entry_points_between_guard_zones():
    from test_abi_guards_gpu import _direct, _st
    from street_crafter_amd import _lib
    V = _V()
    lib = _lib.load()
    n = 1029
    rgb, gt = _images(1, n, 21)
    depth = _depth(1, n, 22)
    g = np.random.default_rng(23)
    acc, obj = g.uniform(0, 1, n).astype(np.float32), g.uniform(0, 1, n).astype(np.float32)
    mask = g.random(n) < 0.8
    four = np.full((n, 4), -3.0, np.float32)
    four[:, 3] = depth[0]
    ws_bytes = lib.sc_frame_viz_workspace_bytes()
    jet, turbo = LUTS["rand"], LUTS["ramp"]
    d = {k: _dev(v) for k, v in dict(rgb=rgb, gt=gt, depth=depth, acc=acc, obj=obj, mask=mask.astype(np.uint8), jet=jet,
                                     turbo=turbo, four=four).items()}
    plain = V.trajectory_frames({"rgb": d["rgb"], "rgb_background": d["rgb"], "rgb_object": d["rgb"], "acc_object": d["obj"][None],
                                 "depth": d["depth"]}, d["gt"], d["mask"][None], d["jet"], d["turbo"])
    plain_acc = V.gray_u8(d["acc"][None])
    plain_range = torch.cat([V.value_range(d["depth"]), V.diff_range(d["rgb"], d["gt"], d["mask"][None])])
    outs = dict(range4=torch.float32, o_depth=torch.uint8, o_diff=torch.uint8, o_acc=torch.uint8, o_obj=torch.uint8)

    def run(depth_name, depth_off, depth_stride, given_range):
        def call(ar):
            dp = ar.ptr(depth_name) + depth_off
            src = (dp, depth_stride, ar.ptr("rgb"), 1, n, ar.ptr("gt"), 1, n, ar.ptr("mask"))
            rc = 0
            if not given_range:
                rc = rc or lib.sc_frame_viz_range(*src, n, ar.ptr("ws"), ws_bytes, _st())
                rc = rc or lib.sc_frame_viz_range_finish(ar.ptr("ws"), ws_bytes, n, 3, ar.ptr("range4"), _st())
            return rc or lib.sc_frame_viz_u8(*src, ar.ptr("acc"), ar.ptr("obj"), n, ar.ptr("jet"), ar.ptr("turbo"),
                                             ar.ptr("range4") if given_range else None,
                                             None if given_range else ar.ptr("ws"), 0 if given_range else ws_bytes,
                                             ar.ptr("o_depth"), ar.ptr("o_diff"), ar.ptr("o_acc"), ar.ptr("o_obj"), _st())
        bufs = dict(rgb=d["rgb"], gt=d["gt"], mask=d["mask"], acc=d["acc"], obj=d["obj"], jet=d["jet"], turbo=d["turbo"],
                    o_depth=3 * n, o_diff=3 * n, o_acc=n, o_obj=n)
        bufs[depth_name] = d[depth_name]
        if given_range:
            bufs["range4"] = plain_range
            o = {k: v for k, v in outs.items() if k != "range4"}
        else:
            bufs["range4"] = 16
            bufs["ws"] = ws_bytes
            o = outs
        got = _direct(bufs, call, o)
        if not given_range:
            assert got["range4"].view(torch.int32).tolist() == plain_range.view(torch.int32).tolist()
        assert torch.equal(got["o_depth"].view(1, n, 3), plain["depth"]) and torch.equal(got["o_diff"].view(1, n, 3), plain["diff"])
        assert torch.equal(got["o_acc"].view(1, n, 1), plain_acc) and torch.equal(got["o_obj"].view(1, n, 1), plain["acc_object"])

    run("depth", 0, 1, False)           # dense, partials from the workspace: range + finish + u8
    run("four", 12, 4, False)           # the [..., 3] view of an [n,4] render: its last float is the buffer's last
    run("depth", 0, 1, True)            # a caller's range4, no workspace
    assert np.array_equal(plain["depth"].cpu().numpy(), R.colorize(depth, jet))
    assert np.array_equal(plain["diff"].cpu().numpy(), R.colorize(R.diff_map(rgb, gt, mask[None]), turbo))
