"""The scenes and cases of the per-row rasterizer-backward tests -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_raster_bwd_ref_cpu.py (the reference judged on its own, the exclusion caps) and
tests/test_raster_bwd_rows_gpu.py (both HIP backward kernels against it), so that the two modules speak of the
same inputs.  Projection and tile lists come from the numpy oracle; colours, backgrounds, tile masks and the
upstream gradients are drawn here.  Nothing in this file touches a GPU.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

from oracle import gsplat_oracle as O
from oracle import raster_bwd_f64 as RB

# name -> (n, seed, z_range, scale_range, width, height, focal, yaws, opacity factor | "set:<value>", street)
SCENES = {
    "ragged": (4000, 21, (1.0, 40.0), (0.01, 0.3), 200, 120, 220.0, (0.0,), 1.0, False),
    "two_cameras": (3000, 33, (1.0, 40.0), (0.01, 0.3), 150, 90, 170.0, (0.0, 0.2), 1.0, False),
    "deep_soft": (6000, 5, (1.0, 20.0), (0.02, 0.3), 80, 48, 90.0, (0.0,), 0.05, False),
    "deep_hard": (6000, 5, (1.0, 20.0), (0.02, 0.3), 80, 48, 90.0, (0.0,), 1.0, False),
    "clamp": (4000, 21, (1.0, 40.0), (0.01, 0.3), 200, 120, 220.0, (0.0,), "set:1.5", False),
    "half_tiles": (40_000, 8, None, None, 400, 272, 2050.0 * 400 / 1920.0, (0.0,), 1.0, False),
    "street": (1500, 1, None, None, 160, 100, 170.0, (0.0,), 1.0, True),
}

# (case id, scene, tile_size, D, background, extras); extras: "masks" = 20 % of the tiles masked, "one_hot" = the
# upstream gradient is non-zero in ONE tile only
CASES = (
    [("ragged-D4bg", "ragged", 16, 4, True, ()), ("ragged-D3", "ragged", 16, 3, False, ())]
    + [(f"tile{ts}-D{D}{'bg' if bg else ''}", "ragged", ts, D, bg, ()) for ts in (8, 12, 32) for D, bg in ((3, False), (4, True))]
    + [(f"channels-D{D}{'bg' if D % 2 else ''}", "ragged", 16, D, bool(D % 2), ()) for D in (1, 2, 5, 7, 16, 32)]
    + [(f"lds-tile{ts}-D{D}", "ragged", ts, D, False, ()) for ts in (32, 8) for D in (7, 32)]
    + [("two_cameras-D4bg-masks", "two_cameras", 16, 4, True, ("masks",))]
    + [("deep_soft-D4", "deep_soft", 16, 4, False, ()), ("deep_soft-D3bg", "deep_soft", 16, 3, True, ()),
       ("deep_hard-D4bg", "deep_hard", 16, 4, True, ())]
    + [("clamp-D3", "clamp", 16, 3, False, ()), ("one_hot-D4", "ragged", 16, 4, False, ("one_hot",))]
    + [("half_tiles-D4", "half_tiles", 16, 4, False, ()), ("half_tiles-D3", "half_tiles", 16, 3, False, ())]
    + [("street-D4bg", "street", 16, 4, True, ())]
    # the generic kernel's staging loop over SEVERAL batches: lists longer than a batch at tile 32 (a batch is 960 splats
    # at D 7, 384 at D 32: fewer than the block's 1024 threads) and at tile 12 (192 threads, the last wave partly outside)
    + [("deep-tile32-D7bg", "deep_soft", 32, 7, True, ()), ("deep-tile32-D32", "deep_soft", 32, 32, False, ()),
       ("deep-tile12-D3", "deep_soft", 12, 3, False, ())]
    # the hand-built finite frames of oracle/raster_edge_frames.py (scene "edge:<frame>"): one case per tile around the
    # batch of 64, the cull's contour and degenerate records; no pixel of them is unstable
    + [("edge-finite-D4bg", "edge:finite", 16, 4, True, ()), ("edge-finite129-D3", "edge:finite129", 16, 3, False, ())]
)
CASE_IDS = [c[0] for c in CASES]
EDGE_IDS = [c[0] for c in CASES if c[1].startswith("edge:")]      # judged under the K of the other cases (or 4x their own)
UNSTABLE_CAP = 0.005          # share of pixels that may be left out of a case's loss


@lru_cache(maxsize=None)
def projected(scene, tile_size):
    """The scene through the numpy oracle's projection and tile intersection: dict of means2d [C,N,2], conics [C,N,3],
    opacities [C,N], depths [C,N], radii [C,N], isect_offsets i32[C,th,tw], flatten_ids i32[I], width, height."""
    if scene.startswith("edge:"):
        from oracle import raster_edge_frames as EF
        assert tile_size == EF.TILE
        f = EF.frame(scene[5:])
        return dict(means2d=f["means2d"], conics=f["conics"], opacities=f["opacities"], depths=None, radii=None,
                    isect_offsets=f["isect_offsets"], flatten_ids=f["flatten_ids"], width=f["width"], height=f["height"],
                    n_cameras=1)
    from street_crafter_amd.scenes import make_camera, make_scene, make_street_scene
    n, seed, zr, sr, w, h, f, yaws, opf, street = SCENES[scene]
    if street:
        sc = make_street_scene(n, seed=seed)[0]
    elif zr is None:
        sc = make_scene(n, seed=seed)
    else:
        sc = make_scene(n, seed=seed, z_range=zr, scale_range=sr)
    per_cam = []
    for yaw in yaws:
        cam = make_camera(w, h, f, f, yaw=yaw)
        radii, m2, d, con, comp = O.fully_fused_projection(sc.means.numpy(), sc.quats.numpy(), sc.scales.numpy(),
                                                           cam.viewmat.numpy(), cam.K.numpy(), w, h, near_plane=0.001,
                                                           far_plane=1000.0, calc_compensations=True)
        per_cam.append((radii, m2, d, con, sc.opacities.numpy().reshape(-1) * comp))
    radii, m2, d, con, op = (np.stack(x) for x in zip(*per_cam))
    if isinstance(opf, str):      # the operator does not restrict opacities: above 1 an alpha can reach the clamp
        op = np.full_like(op, float(opf.split(":")[1]))
    else:
        op = (op * np.float32(opf)).astype(np.float32)
    C = len(yaws)
    tw, th = math.ceil(w / tile_size), math.ceil(h / tile_size)
    _, ids, fids = O.isect_tiles(m2, radii, d, tile_size, tw, th, n_cameras=C)
    offs = O.isect_offset_encode(ids, C, tw, th)
    return dict(means2d=m2.astype(np.float32), conics=con.astype(np.float32), opacities=op.astype(np.float32),
                depths=d, radii=radii, isect_offsets=offs, flatten_ids=fids, width=w, height=h, n_cameras=C)


def make_case(case_id):
    """Everything rasterize_to_pixels and its backward take for one case (numpy arrays), the pixels left out
    (`unstable`, already applied to v_colors / v_alphas) and the reference's statistics of live / clamped pairs."""
    cid, scene, ts, D, use_bg, extras = CASES[CASE_IDS.index(case_id)]
    p = dict(projected(scene, ts))
    C, N = p["opacities"].shape
    W, H = p["width"], p["height"]
    rng = np.random.default_rng(1000 + CASE_IDS.index(case_id))
    p["colors"] = rng.uniform(0, 1, (C, N, D)).astype(np.float32)
    p["backgrounds"] = rng.uniform(0, 1, (C, D)).astype(np.float32) if use_bg else None
    th, tw = p["isect_offsets"].shape[1:]
    p["masks"] = (rng.random((C, th, tw)) >= 0.2) if "masks" in extras else None
    v_c = rng.normal(size=(C, H, W, D)).astype(np.float32)
    v_a = rng.normal(size=(C, H, W, 1)).astype(np.float32)
    if "one_hot" in extras:
        ty, tx = th // 2, tw // 2
        keep = np.zeros((C, H, W), bool)
        keep[:, ty * ts:(ty + 1) * ts, tx * ts:(tx + 1) * ts] = True
        v_c[~keep] = 0.0
        v_a[~keep] = 0.0
    un, stats = RB.unstable_bwd(p["means2d"], p["conics"], p["colors"], p["opacities"], W, H, ts, p["isect_offsets"],
                                p["flatten_ids"], masks=p["masks"], return_stats=True)
    v_c[un] = 0.0
    v_a[un] = 0.0
    p.update(case=cid, scene=scene, tile_size=ts, D=D, v_colors=v_c, v_alphas=v_a, unstable=un, stats=stats, extras=extras)
    return p


def reference(p, dtype=np.float64, **kw):
    return RB.rasterize_bwd(p["means2d"], p["conics"], p["colors"], p["opacities"], p["width"], p["height"], p["tile_size"],
                            p["isect_offsets"], p["flatten_ids"], p["v_colors"], p["v_alphas"], backgrounds=p["backgrounds"],
                            masks=p["masks"], dtype=dtype, **kw)


def generic_kernel_batch(tile_size, D):
    """(threads per block, splats staged per batch) of the reference-shaped backward kernel, restated from the host code
    of csrc/raster_bwd.hip so that tests can assert that a case walks several batches."""
    threads = (tile_size * tile_size + 63) // 64 * 64
    return threads, min(threads, (64 * 1024 // (40 + 4 * D)) // 64 * 64)


def longest_list(p):
    return int(np.diff(np.append(p["isect_offsets"].reshape(-1), p["flatten_ids"].size)).max())


def outputs_of(p):
    return [k for k in RB.OUTPUTS if k != "backgrounds" or p["backgrounds"] is not None]


def worst_ratios(x, ref, names):
    """{name: (largest per-row ratio, largest |x| where S == 0)} of the gradients `x` (dict name -> array)."""
    out = {}
    for k in names:
        r, off = RB.row_ratio(x[k], ref, k)
        out[k] = (float(r.max()) if r.size else 0.0, off)
    return out
