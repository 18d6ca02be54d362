"""rasterize_to_pixels backward, both HIP kernels, judged PER GRADIENT ROW against the float64 closed form
(oracle/raster_bwd_f64.py; tests/test_raster_bwd_ref_cpu.py judges that reference on its own).

Bar, for every row of v_means2d, v_conics, v_colors, v_opacities, absgrad and for v_backgrounds:

    |hip - G| <= 2^-24 (K S + A)          and exactly 0 where S == 0

S: the sum of the magnitudes of the row's terms; A: the same with each pixel's terms times 0.5 / T_final (half an ulp
of the stored float32 alpha the backward rebuilds T_final from) -- both derived in the reference's module text.
K = 4 K_ref, K_ref the largest ratio (|replay - G| - 2^-24 A)+ / (2^-24 S) the float32 REPLAY of the closed form
(numpy, no kernel) reaches over all rows, outputs and cases of this module; the factor 4 covers v_exp_f32 / v_rcp_f32
(1 ulp where numpy rounds correctly), FMA contraction and atomics in arbitrary order.  absgrad is judged with the S and A
of its v_means2d row.  Pixels within 2e-5 (relative) of a hard threshold of the forward or of the clamp at 0.999 get
zero upstream gradient; their share is asserted < 0.5 % per case.

Cases: oracle/raster_bwd_cases.py (partial last tile column and row; tile sizes 8 / 12 / 32: one wave, a partial wave,
16 waves; 1..32 channels; the LDS sizing of tile 32 with 7 and 32 channels; two cameras with per-camera backgrounds
and masked tiles; lists of 900 entries that never saturate, and that always do; clamped alphas; an upstream gradient
in one tile only; the forward's half-tile dispatch items; a street-shaped scene; the 950-entry scene again at tile 32
with 7 and 32 channels and at tile 12, where the generic kernel walks 3 to 6 staging batches).  Every case runs under both
`raster_bwd` settings; 1 (one wave per tile) takes the generic kernel outside tile 16 / 3-4 channels.  The two hand-built
frames of oracle/raster_edge_frames.py (the walk's boundaries around the batch of 64, the cull's contour, degenerate
records: no pixel left out) are judged under the K of the other cases, also through hand-written half-tile dispatch lists.
The forward the backward starts from is held, colours and alphas of every pixel, to the per-pixel bar of
oracle/raster_fwd_f64.py (tests/test_raster_fwd_pixels_gpu.py judges every forward entry by it).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import raster_bwd_cases as RC          # noqa: E402  (checker only)
from oracle import raster_bwd_f64 as RB            # noqa: E402
from oracle import raster_fwd_f64 as RF            # noqa: E402

DEV = "cuda"
HALF = [c for c in RC.CASE_IDS if c.startswith("half_tiles")]
PLAIN = [c for c in RC.CASE_IDS if c not in HALF]


@pytest.fixture(scope="module")
def ops():
    from street_crafter_amd import _lib
    _lib.load()
    import gsplat.rendering as R
    return R


@pytest.fixture(scope="module")
def refs():
    """{case: (inputs, float64 reference)} and K: ONE number for the module (on a saturated scene such as deep_hard A
    swallows the whole replay error and the case's own ratio is 0, which must not become its bar)."""
    table, k_ref, own_of = {}, 0.0, {}
    for cid in RC.CASE_IDS:
        p = RC.make_case(cid)
        ref = RC.reference(p)
        rep = RC.worst_ratios(RC.reference(p, np.float32)["G"], ref, RC.outputs_of(p))
        assert all(off == 0.0 for _, off in rep.values()), (cid, rep)
        own = own_of[cid] = max(r for r, _ in rep.values())
        print(f"[replay] {cid}: K_ref {own:.1f} ({max(rep, key=lambda k: rep[k][0])}); left out {100 * p['unstable'].mean():.3f} %")
        if cid not in RC.EDGE_IDS:        # K comes from the random scenes; the hand-built frames are judged under it
            k_ref = max(k_ref, own)
        table[cid] = (p, ref)
    print(f"[replay] K_ref over {len(table) - len(RC.EDGE_IDS)} cases: {k_ref:.1f}; K = {4 * k_ref:.1f}")
    assert 1.0 < k_ref < 1000.0
    K = {cid: 4.0 * k_ref for cid in table}
    for cid in RC.EDGE_IDS:
        assert float(table[cid][0]["unstable"].mean()) == 0.0, cid
        if own_of[cid] > k_ref:           # its own float32 replay is already past K_ref: that case alone gets 4x its own
            K[cid] = 4.0 * own_of[cid]
            print(f"[replay] {cid}: own ratio {own_of[cid]:.1f} > K_ref {k_ref:.1f}: judged under {K[cid]:.1f}")
    return table, K


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _hip(ops, p, variant, offs=None, fids=None):
    """The operator's backward under `raster_bwd` = variant -> ({output: numpy gradient}, render_colors, render_alphas)."""
    from street_crafter_amd import _lib
    src = [_t(p[k]).requires_grad_(True) for k in ("means2d", "conics", "colors", "opacities")]
    bg = None if p["backgrounds"] is None else _t(p["backgrounds"]).requires_grad_(True)
    masks = None if p["masks"] is None else torch.from_numpy(p["masks"]).to(DEV)
    rc, ra = ops.rasterize_to_pixels(*src, p["width"], p["height"], p["tile_size"],
                                     _t(p["isect_offsets"], torch.int32) if offs is None else offs,
                                     _t(p["flatten_ids"], torch.int32) if fids is None else fids,
                                     backgrounds=bg, masks=masks, absgrad=True)
    prev = _lib.set_option("raster_bwd", variant)
    try:
        ((rc * _t(p["v_colors"])).sum() + (ra * _t(p["v_alphas"])).sum()).backward()
        torch.cuda.synchronize()
    finally:
        _lib.set_option("raster_bwd", prev)
    out = {k: t.grad.cpu().numpy() for k, t in zip(("means2d", "conics", "colors", "opacities"), src)}
    out["absgrad"] = src[0].absgrad.cpu().numpy()
    if bg is not None:
        out["backgrounds"] = bg.grad.cpu().numpy()
    return out, rc.detach(), ra.detach()


def _judge(tag, got, p, ref, K):
    assert float(p["unstable"].mean()) < RC.UNSTABLE_CAP, tag
    worst = RC.worst_ratios(got, ref, RC.outputs_of(p))
    print(f"[hip] {tag}: " + ", ".join(f"{k} {r:.1f}" + (f" (|x| {off:.1e} where S = 0)" if off else "") for k, (r, off) in worst.items())
          + f"; bar {K:.1f}")
    for k, (r, off) in worst.items():
        assert np.isfinite(got[k]).all(), (tag, k)
        assert off == 0.0, (tag, k, off)
        assert r <= K, (tag, k, r, K)
    assert (np.abs(ref["G"]["means2d"]).max() > 0) and (ref["S"]["colors"] > 0).any(), tag      # the case is not empty


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case_id", PLAIN)
def test_backward_rows_against_the_float64_closed_form(ops, refs, case_id, variant):
    table, K = refs
    p, ref = table[case_id]
    K = K[case_id]
    got, rc, ra = _hip(ops, p, variant)
    if "one_hot" in p["extras"]:
        ts = p["tile_size"]
        th, tw = p["isect_offsets"].shape[1:]
        lit = np.zeros(p["unstable"].shape, bool)
        lit[:, (th // 2) * ts:(th // 2 + 1) * ts, (tw // 2) * ts:(tw // 2 + 1) * ts] = True
        assert not p["v_colors"][~lit].any() and not p["v_alphas"][~lit].any()
        assert (ref["S"]["colors"].sum(-1) == 0).mean() > 0.9            # nearly every row lies outside that tile
    if p["scene"] == "clamp":
        assert p["stats"]["clamped"] >= 0.01 * p["stats"]["live"]
    if case_id.startswith("deep-tile"):
        # the reference-shaped kernel walks SEVERAL staging batches here; at tile 32 a batch is smaller than the block
        # (the `tr < B` staging guard decides, the batch stride is not the block size), at tile 12 the block's last wave
        # is partly outside the tile
        threads, batch = RC.generic_kernel_batch(p["tile_size"], p["D"])
        assert RC.longest_list(p) > 2 * batch, (RC.longest_list(p), batch)
        assert (batch < threads) if p["tile_size"] == 32 else (threads > p["tile_size"] ** 2)
    # the forward both sides start from is the same picture (stored alphas within the blend's own bar), and colours and
    # alphas of EVERY pixel are within the per-pixel bar of the float64 forward (oracle/raster_fwd_f64.py)
    stable = ~p["unstable"]
    assert np.abs(ra.cpu().numpy()[..., 0] - ref["render_alphas"])[stable].max() <= 1e-4
    fwd = RF.judge(RF.case_reference(case_id, p)[1], rc.cpu().numpy(), ra.cpu().numpy())
    assert fwd["ratio"].max() <= RF.K, (case_id, fwd["colors"], fwd["alphas"], RF.K)
    _judge(f"{case_id} raster_bwd={variant}", got, p, ref, K)


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case_id", HALF)
def test_backward_rows_through_the_half_tile_dispatch_items(ops, refs, case_id, variant, split):
    """The lists come from ops.isect_tiles on a warm second frame, so that isect_offsets carries the dispatch list with
    its half tiles (as tests/test_gpu_parity.py::test_tile_dispatch_order_in_training); they are bit-equal to the numpy
    oracle's, which the reference was computed from."""
    from street_crafter_amd import _lib, rendering
    table, K = refs
    p, ref = table[case_id]
    K = K[case_id]
    th, tw = p["isect_offsets"].shape[1:]
    assert (tw, th) == (25, 17)
    m2, radii, depths = _t(p["means2d"]), _t(p["radii"], torch.int32), _t(p["depths"])
    prev_split = _lib.set_option("raster_bwd_split", split)
    prev_order = rendering.set_tile_order(True)
    try:
        for frame in range(2):
            _, ids, fids = ops.isect_tiles(m2, radii, depths, 16, tw, th, n_cameras=1)
            offs = ops.isect_offset_encode(ids, 1, tw, th)
            if frame == 0:        # the forward leaves what every tile walked: the next frame's list is built from it
                with torch.no_grad():
                    ops.rasterize_to_pixels(m2, _t(p["conics"]), _t(p["colors"]), _t(p["opacities"]), p["width"], p["height"], 16,
                                            offs, fids)
        sched = getattr(offs, "_sc_sched", None)
        assert sched is not None
        n_halves = int(((sched[0].cpu().numpy()[: 425 + 425 // 8 + 8] & 3) == 1).sum())
        assert n_halves > 0
        fids = fids.plain() if hasattr(fids, "plain") else fids
        np.testing.assert_array_equal(offs.cpu().numpy(), p["isect_offsets"])
        np.testing.assert_array_equal(fids.cpu().numpy(), p["flatten_ids"])
        got, _, _ = _hip(ops, p, variant, offs, fids)
    finally:
        rendering.set_tile_order(prev_order)
        _lib.set_option("raster_bwd_split", prev_split)
    _judge(f"{case_id} raster_bwd={variant} raster_bwd_split={split} ({n_halves} half tiles)", got, p, ref, K)


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case_id", RC.EDGE_IDS)
def test_hand_built_frames_through_the_half_tile_dispatch_items(ops, refs, case_id, variant, split):
    """The hand-built lists cannot come from isect_tiles, so the dispatch list is written by hand as well
    (oracle/raster_edge_frames.py: dispatch_list) and travels on isect_offsets the way isect_tiles leaves it: every
    16-row tile is walked as two half-tile items in one of the lists, by the forward and (raster_bwd_split 1) the backward."""
    from oracle import raster_edge_frames as EF
    from street_crafter_amd import _lib, rendering
    table, K = refs
    p, ref = table[case_id]
    K = K[case_id]
    n_tiles = EF.TW * EF.TH
    prev_split = _lib.set_option("raster_bwd_split", split)
    prev_order = rendering.set_tile_order(True)
    try:
        for tiles in EF.split_sets():
            offs = _t(p["isect_offsets"], torch.int32)
            order = _t(EF.dispatch_list(tiles), torch.int32)
            assert order.numel() == _lib.load().sc_tile_order_len(n_tiles)
            offs._sc_sched = (order, torch.zeros(_lib.load().sc_view_slots() * n_tiles, dtype=torch.int32, device=DEV))
            assert rendering._sched_of(offs, n_tiles)[0] is order
            got, _, _ = _hip(ops, p, variant, offs, _t(p["flatten_ids"], torch.int32))
            _judge(f"{case_id} raster_bwd={variant} raster_bwd_split={split} (tiles {tiles[0]}..{tiles[-1]} halved)", got, p, ref, K)
    finally:
        rendering.set_tile_order(prev_order)
        _lib.set_option("raster_bwd_split", prev_split)


@pytest.mark.parametrize("case_id", ["ragged-D4bg", "two_cameras-D4bg-masks"])
def test_python_and_compiled_autograd_routes_give_the_same_rows(ops, refs, case_id):
    """The Python torch.autograd.Function and the compiled binding's autograd function launch the same kernels on the
    same inputs: the same forward bit for bit, the same v_backgrounds (no atomics in it), each route within the per-row
    bar, and the two routes within the reordering of the float atomics OF EACH OTHER.  The wave kernel adds one partial
    sum per tile into a row, n_g = the number of tile lists the splat is in; every partial sum is bounded by the row's S,
    so one order of the n_g additions is within (n_g - 1) 2^-24 S of the exact sum of the partials and two orders are
    within 2 n_g 2^-24 S of each other -- no K, no A in it."""
    from street_crafter_amd import _lib, rendering
    if _lib.fast() is None:
        pytest.fail("compiled binding layer not loaded")
    table, K = refs
    p, ref = table[case_id]
    K = K[case_id]
    res = {}
    for native in (True, False):
        prev = rendering.set_native_autograd(native)
        try:
            res[native] = _hip(ops, p, 1)
        finally:
            rendering.set_native_autograd(prev)
        _judge(f"{case_id} native_autograd={native}", res[native][0], p, ref, K)
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])
    if p["backgrounds"] is not None:
        np.testing.assert_array_equal(res[True][0]["backgrounds"], res[False][0]["backgrounds"])
    n_g = np.bincount(p["flatten_ids"], minlength=p["opacities"].size).reshape(p["opacities"].shape).astype(np.float64)
    for k in ("means2d", "conics", "colors", "opacities", "absgrad"):
        a, b = res[True][0][k].astype(np.float64), res[False][0][k].astype(np.float64)
        S = ref["S"][k]
        bound = RB.EPS24 * 2.0 * n_g.reshape(n_g.shape + (1,) * (S.ndim - 2)) * S
        worst = float((np.abs(a - b) / np.where(bound > 0, bound, 1.0)).max())
        print(f"[routes] {case_id} {k}: largest |native - python| / (2 n 2^-24 S) = {worst:.3f}")
        assert (np.abs(a - b) <= bound).all(), (k, worst)
