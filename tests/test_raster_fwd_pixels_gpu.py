"""Every forward entry of the rasterizer judged PER PIXEL against the float64 forward of oracle/raster_fwd_f64.py
(tests/test_raster_fwd_ref_cpu.py judges that reference on its own), no pixel left out.

Bar, for every pixel and every channel of render_colors (a depth channel included) and for render_alphas:

    |hip - G| <= 2^-24 K E,     exactly G (the background, or 0) where E == 0,     last_ids exactly equal

E: the first-order error scale derived in the reference's module text; K = 4 K_REF, K_REF the largest ratio two float32
replays of the blend in numpy reach (no kernel involved), recorded in the module and re-measured by the CPU test.  A pixel
with a decision no float32 evaluation can resolve passes iff colour, alpha and last_ids together are within the bar of
one of the float64 outcomes blend_f64 enumerates, judged by that outcome's scale; such pixels are below 0.5 % per case.

Cases: oracle/raster_bwd_cases.py (partial last tile row and column, tiles 8 / 12 / 16 / 32, 1 to 32 channels, two cameras
with per-camera backgrounds and masked tiles, lists that never saturate and that always do, clamped alphas, the
street-shaped scene, the two finite hand-built frames).  Entries, i.e. every instantiation rasterize_fwd_impl can launch:
the reference-shaped kernel (D 3, 4, generic) on every case; the wave kernel through rasterize_to_pixels without and with
last_ids; the same through half-tile dispatch lists (isect_tiles' on a warm second frame; hand-written ones for the
hand-built frames); the planar output; the depth-normalising epilogue; the packed-record entry with and without it.
Grouped and layered forwards are held bit for bit against the plain render elsewhere.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import raster_bwd_cases as RC          # noqa: E402  (checker only)
from oracle import raster_fwd_f64 as RF            # noqa: E402

DEV = "cuda"
CASES = RF.case_ids()
_SPEC = {c[0]: c for c in RC.CASES}
T16 = [c for c in CASES if _SPEC[c][2] == 16 and _SPEC[c][3] in (3, 4)]          # what the wave kernel takes
T16_D4 = [c for c in T16 if _SPEC[c][3] == 4]
T16_D4_NOMASK = [c for c in T16_D4 if "masks" not in _SPEC[c][5]]
HALF = [c for c in CASES if c.startswith("half_tiles")]
EDGE = [c for c in CASES if c in RC.EDGE_IDS]


@pytest.fixture(scope="module")
def ops():
    from street_crafter_amd import _lib
    _lib.load()
    import gsplat.rendering as R
    return R


@lru_cache(maxsize=None)
def _ref(case_id):
    """(inputs, float64 reference) of a case: computed once, left unchanged."""
    p, ref = RF.case_reference(case_id)
    assert RF.near_share(ref) < RC.UNSTABLE_CAP and ref["truncated"] == 0, case_id
    assert ref["blended"].any(), case_id
    return p, ref


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _tensors(p):
    bg = None if p["backgrounds"] is None else _t(p["backgrounds"])
    masks = None if p["masks"] is None else _t(p["masks"], torch.uint8)
    return [_t(p[k]) for k in ("means2d", "conics", "colors", "opacities")], bg, masks


def _lists(p):
    return _t(p["isect_offsets"], torch.int32), _t(p["flatten_ids"], torch.int32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _binding_fwd(p, variant, want_last=True, order=None, work=None):
    """sc_rasterize_fwd under `raster_fwd` = variant -> colours, alphas, last_ids (None unless asked for)"""
    from street_crafter_amd import _lib
    src, bg, masks = _tensors(p)
    offs, fids = _lists(p)
    prev = _lib.set_option("raster_fwd", variant)
    try:
        rc, c, a, last = _lib.binding().rasterize_fwd(*src, bg, masks, p["width"], p["height"], p["tile_size"], offs, fids,
                                                       bool(want_last), order, work, _stream())
        torch.cuda.synchronize()
    finally:
        _lib.set_option("raster_fwd", prev)
    _lib.check(rc, "sc_rasterize_fwd")
    return c, a, last


def _operator(ops, p, grad, offs=None, fids=None):
    """rasterize_to_pixels under `raster_fwd` 3, interleaved output: without grad the instantiation without last_ids, with
    inputs that require grad the one that records them."""
    from street_crafter_amd import _lib, rendering
    src, bg, masks = _tensors(p)
    o, f = _lists(p)
    offs, fids = (o if offs is None else offs), (f if fids is None else fids)
    prev = _lib.set_option("raster_fwd", 3)
    prev_planar = rendering.set_planar_output(False)
    try:
        if grad:
            src = [t.requires_grad_(True) for t in src]
            c, a = ops.rasterize_to_pixels(*src, p["width"], p["height"], p["tile_size"], offs, fids, backgrounds=bg, masks=masks)
            assert c.requires_grad
        else:
            with torch.no_grad():
                c, a = ops.rasterize_to_pixels(*src, p["width"], p["height"], p["tile_size"], offs, fids, backgrounds=bg,
                                               masks=masks)
        torch.cuda.synchronize()
    finally:
        rendering.set_planar_output(prev_planar)
        _lib.set_option("raster_fwd", prev)
    return c.detach(), a.detach()


def _judge(tag, ref, c, a, last=None, depth_normalise=False):
    assert tuple(c.shape) == ref["colors"].shape and a.numel() == ref["alphas"].size, tag
    j = RF.judge(ref, c.cpu().numpy(), a.cpu().numpy(), None if last is None else last.cpu().numpy(), depth_normalise)
    worst = float(j["ratio"].max())
    print(f"[hip] {tag}: colours {j['colors']:.3f}, alpha {j['alphas']:.3f}" + ("" if last is None else ", last_ids equal")
          + f"; {j['ratio'].size} pixels judged, {len(ref['alts'])} against several outcomes ({j['alt']} by another than the "
          f"natural one); bar K = {RF.K}")
    assert j["ratio"].shape == ref["alphas"].shape          # every pixel has its verdict
    if not worst <= RF.K:
        at = np.unravel_index(int(np.argmax(j["ratio"])), j["ratio"].shape)
        G_c, E_c = ref["colors"], ref["E_colors"]
        if depth_normalise:
            G_c, E_c = RF.depth_normalised(G_c, ref["alphas"], E_c, ref["E_alphas"])
        pytest.fail(f"{tag}: ratio {worst:.3f} > K = {RF.K} at (camera, y, x) = {tuple(int(v) for v in at)}: hip colour "
                    f"{c.cpu().numpy()[at]}, float64 {G_c[at]}, E {E_c[at]}; hip alpha "
                    f"{a.cpu().numpy().reshape(ref['alphas'].shape)[at]!r}, float64 {ref['alphas'][at]!r}, E {ref['E_alphas'][at]}; "
                    f"last_ids {None if last is None else int(last.cpu().numpy()[at])} / {int(ref['last_ids'][at])}")


@pytest.mark.parametrize("case_id", CASES)
def test_reference_shaped_kernel(case_id):
    """`raster_fwd` 0: raster_fwd_ref_kernel<3>, <4> and the generic <0>, any tile size, with last_ids."""
    p, ref = _ref(case_id)
    c, a, last = _binding_fwd(p, 0)
    _judge(f"{case_id} raster_fwd=0", ref, c, a, last)


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("case_id", T16)
def test_wave_kernel_through_the_operator(ops, case_id, grad):
    """`raster_fwd` 3 through rasterize_to_pixels.  The operator does not hand last_ids out: they are read from the entry
    that returns them (the same instantiation), whose image must be the operator's bit for bit."""
    p, ref = _ref(case_id)
    c, a = _operator(ops, p, grad)
    last = None
    if grad:
        c2, a2, last = _binding_fwd(p, 3)
        assert torch.equal(c2, c) and torch.equal(a2, a), case_id
    _judge(f"{case_id} raster_fwd=3 grad={grad}", ref, c, a, last)


@pytest.mark.parametrize("case_id", HALF)
def test_wave_kernel_through_the_half_tile_dispatch_items(ops, case_id):
    """The lists come from ops.isect_tiles on a warm second frame, so that isect_offsets carries the dispatch list with its
    half tiles (as tests/test_raster_bwd_rows_gpu.py does for the backward); they are bit-equal to the numpy oracle's, which
    the reference was computed from."""
    from street_crafter_amd import rendering
    p, ref = _ref(case_id)
    th, tw = p["isect_offsets"].shape[1:]
    assert (tw, th) == (25, 17)
    src, _, _ = _tensors(p)
    m2, radii, depths = src[0], _t(p["radii"], torch.int32), _t(p["depths"])
    prev_order = rendering.set_tile_order(True)
    try:
        for frame in range(2):
            _, ids, fids = ops.isect_tiles(m2, radii, depths, 16, tw, th, n_cameras=1)
            offs = ops.isect_offset_encode(ids, 1, tw, th)
            if frame == 0:        # the forward leaves what every tile walked: the next frame's list is built from it
                with torch.no_grad():
                    ops.rasterize_to_pixels(*src, p["width"], p["height"], 16, offs, fids)
        sched = getattr(offs, "_sc_sched", None)
        assert sched is not None
        n_halves = int(((sched[0].cpu().numpy()[: 425 + 425 // 8 + 8] & 3) == 1).sum())
        assert n_halves > 0
        fids = fids.plain() if hasattr(fids, "plain") else fids
        np.testing.assert_array_equal(offs.cpu().numpy(), p["isect_offsets"])
        np.testing.assert_array_equal(fids.cpu().numpy(), p["flatten_ids"])
        assert rendering._sched_of(offs, tw * th)[0] is sched[0]
        c, a = _operator(ops, p, False, offs, fids)
        c2, a2, last = _binding_fwd(p, 3, True, sched[0], sched[1])
    finally:
        rendering.set_tile_order(prev_order)
    _judge(f"{case_id} raster_fwd=3 ({n_halves} half tiles) no last_ids", ref, c, a)
    _judge(f"{case_id} raster_fwd=3 ({n_halves} half tiles) last_ids", ref, c2, a2, last)


@pytest.mark.parametrize("want_last", [False, True])
@pytest.mark.parametrize("case_id", EDGE)
def test_hand_built_frames_through_hand_written_dispatch_lists(case_id, want_last):
    """Every 16-row tile of the hand-built frames walked as two half-tile items in one of the lists
    (oracle/raster_edge_frames.py: dispatch_list)."""
    from oracle import raster_edge_frames as EF
    from street_crafter_amd import _lib
    p, ref = _ref(case_id)
    n_tiles = EF.TW * EF.TH
    for tiles in EF.split_sets():
        order = _t(EF.dispatch_list(tiles), torch.int32)
        assert order.numel() == _lib.load().sc_tile_order_len(n_tiles)
        work = torch.zeros(_lib.load().sc_view_slots() * n_tiles, dtype=torch.int32, device=DEV)
        c, a, last = _binding_fwd(p, 3, want_last, order, work)
        assert (last is not None) == want_last
        _judge(f"{case_id} raster_fwd=3 tiles {tiles[0]}..{tiles[-1]} halved, last_ids={want_last}", ref, c, a, last)


@pytest.mark.parametrize("case_id", T16)
def test_planar_output(case_id):
    """sc_rasterize_fwd_planar (D 3 and 4): one plane per channel, read back as the same [C,H,W,D] tensor by value."""
    from street_crafter_amd import _lib
    p, ref = _ref(case_id)
    src, bg, masks = _tensors(p)
    offs, fids = _lists(p)
    prev = _lib.set_option("raster_fwd", 3)
    try:
        rc, c, a = _lib.binding().rasterize_fwd_planar(*src, bg, masks, p["width"], p["height"], 16, offs, fids, None, None,
                                                        _stream())
        torch.cuda.synchronize()
    finally:
        _lib.set_option("raster_fwd", prev)
    _lib.check(rc, "sc_rasterize_fwd_planar")
    assert not c.is_contiguous() and c.permute(0, 3, 1, 2).is_contiguous()
    _judge(f"{case_id} planar", ref, c.contiguous(), a)


@pytest.mark.parametrize("case_id", T16_D4)
def test_depth_normalising_epilogue(case_id):
    """sc_rasterize_fwd_ed: channel 3 leaves as its sum / max(alpha, 1e-10); the bound goes through the quotient."""
    from street_crafter_amd import _lib
    from street_crafter_amd._ctypes_binding import _p
    p, ref = _ref(case_id)
    src, bg, masks = _tensors(p)
    offs, fids = _lists(p)
    C, N = p["opacities"].shape
    th, tw = p["isect_offsets"].shape[1:]
    c = torch.empty((C, p["height"], p["width"], 4), dtype=torch.float32, device=DEV)
    a = torch.empty((C, p["height"], p["width"], 1), dtype=torch.float32, device=DEV)
    prev = _lib.set_option("raster_fwd", 3)
    try:
        rc = _lib.load().sc_rasterize_fwd_ed(*(_p(t) for t in src), _p(bg), _p(masks), C, N, 4, p["width"], p["height"], 16, tw, th,
                                             _p(offs), _p(fids), fids.numel(), _p(c), _p(a), None, None, _stream())
        torch.cuda.synchronize()
    finally:
        _lib.set_option("raster_fwd", prev)
    _lib.check(rc, "sc_rasterize_fwd_ed")
    _judge(f"{case_id} depth-normalised", ref, c, a, depth_normalise=True)


@pytest.mark.parametrize("depth_normalise", [0, 1])
@pytest.mark.parametrize("case_id", T16_D4_NOMASK)
def test_packed_record_entry(case_id, depth_normalise):
    """sc_rasterize_fwd_packed: the 48-B records built as tests/test_raster_edges_gpu.py builds them."""
    from street_crafter_amd import _lib
    p, ref = _ref(case_id)
    (m2, cn, col, op), bg, _ = _tensors(p)
    offs, fids = _lists(p)
    rec = torch.zeros(m2.shape[0], m2.shape[1], 12, device=DEV)
    rec[..., 0:2], rec[..., 2:5], rec[..., 5], rec[..., 6:10] = m2, cn, op, col
    prev = _lib.set_option("raster_fwd", 3)
    try:
        rc, c, a = _lib.binding().rasterize_fwd_packed(rec.contiguous(), bg, p["width"], p["height"], offs, fids, None, None,
                                                        depth_normalise, _stream())
        torch.cuda.synchronize()
    finally:
        _lib.set_option("raster_fwd", prev)
    _lib.check(rc, "sc_rasterize_fwd_packed")
    _judge(f"{case_id} packed depth_normalise={depth_normalise}", ref, c, a, depth_normalise=bool(depth_normalise))
