"""Guard zones around every buffer of every operator: no stray write, no stray read, nothing left unwritten.

The sweep.  One case per host call of the ctypes adapter (street_crafter_amd/_ctypes_binding.py; a forward and its
backward share a case).  Each case runs the PUBLIC operator on the ctypes route three times from identical inputs:

  plain   ordinary torch allocations: what the other modules judge;
  A       under guarded_adapter(GuardedAlloc(0xA5, 0xA5)): every output and workspace the adapter allocates, every
          float / uint8 / bool input and every buffer updated in place lies in a block of its own between guard zones
          (tests/guard_arena.py), inputs and interiors prefilled with 0xA5;
  B       the same with GuardedAlloc(0x3F, 0x00): floats 0.747 (finite, harmless), masks false.

Integer index inputs (flatten_ids, isect_offsets, radii, group_ids, src_row, tap tables) are ordinary tensors in all runs.
In A and B the adapter's `_ws` hands out exactly the bytes `*_workspace_bytes()` reported (not its floor of 256), so the
guard of a workspace sits at the reported size; the sites that allocate `max(ws_bytes, 8)` themselves (loss_fwd,
depth_trim_fwd, acc_reg_fwd, frame_tail_bwd) hide a reported size below 8 bytes only.

Asserted, after one synchronize per run:
 1. no guard byte changed in A or B, and every guarded input still holds the bits that were put in;
 2. the sequence of adapter calls and their return codes is the same in the three runs, the case's own calls return 0,
    and EVERY tensor an adapter call returned -- and every output, gradient and in-place buffer of the operator -- is
    bit-identical between plain, A and B (an element never written holds 0xA5 / 0x3F, a value read from past an input
    differs between A and B);
 3. where include/street_crafter_amd.h says a region is not written (WRITTEN below), only the written region is
    compared and the rest must still hold the prefill in A and in B;
 4. the outputs accumulated with float atomics (ATOMIC below, each with its kernel line) are not bit-stable from run to
    run: they, and only they, are judged in all three runs by the float64 reference and bar of their own module;
    workspaces the adapter hands back (SCRATCH) have no specified contents and are compared by shape only; the
    rasterizer's dispatch list (UNORDERED) is placed by integer atomics and compared as the set of items it holds;
 5. the compiled binding returns tensors of the same shapes and dtypes for the same case.

The direct cases at the end call the entry points the operators reach outside the adapter through raw pointers into one
Arena, with exactly *_workspace_bytes() of workspace, under both fills.
"""
import contextlib
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guard_arena import Arena, GuardedAlloc, guarded_adapter  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = {"A": (0xA5, 0xA5), "B": (0x3F, 0x00)}

# adapter function -> why no sweep case has it as its subject.  Only calls that launch no kernel belong here.
EXEMPT = {"wait_i64": "host-side spin on a pinned word (sc_wait_i64): launches no kernel, takes no device buffer"}

# (adapter function, index in its return tuple) -> the float atomics that accumulate that output
ATOMIC = {}
for _i in range(1, 6):
    ATOMIC[("rasterize_bwd", _i)] = "raster_bwd.hip:160-170 (generic kernel) and :381 (wave kernel): atomicAdd per splat"
    ATOMIC[("rasterize_bwd_groups", _i)] = "raster_groups_bwd.hip:221: atomicAdd of a tile's partial sum into the row"
ATOMIC[("cubemap_bwd", 1)] = "cubemap.hip:137: atomicAdd of w * g * act' into the four texels"
ATOMIC[("compose_bwd", 7)] = "compose.hip:388: atomicAdd of a block's pose-rotation partial sums"
ATOMIC[("compose_bwd", 8)] = "compose.hip:393: atomicAdd of a block's pose-translation partial sums"

# workspaces an adapter call hands back for its partner call: contents unspecified
SCRATCH = {("isect_bin_count", 4), ("depth_trim_fwd", 4)}


# ---- regions the header leaves unwritten: (function, index) -> mask(args, plain returns, k) of the WRITTEN elements ----
def _isect_written(args, ret, k, leaf):
    """sc_isect_bin_sort: I = meta_dev[0] entries of isect_ids / flatten_ids; nothing at all when a capacity is too small."""
    meta = [int(v) for v in args[7].cpu().tolist()]
    ran = meta[0] <= args[9] and meta[2] <= args[10] and meta[3] <= args[11]
    mask = torch.zeros(leaf.shape, dtype=torch.bool, device=leaf.device)
    if ran:
        mask[:meta[0]] = True
    return mask


def _order_written(args, ret, k, leaf):
    """sc_tile_order_len: the forward's list (tiles + tiles / 8 + 8 items, padded), a whole-tile list of `tiles` items that
    is built only under raster_bwd_split 0, the word that says whether it was, the view slot."""
    n, tiles = leaf.numel(), args[1].shape[0] * args[4] * args[5]
    first = tiles + tiles // 8 + 8
    assert first + tiles + 2 == n
    mask = torch.ones(n, dtype=torch.bool, device=leaf.device)
    if int(leaf[first + tiles]) == 0:
        mask[first:first + tiles] = False
    return mask


def _plan_rows_written(args, ret, k, leaf):
    """sc_densify_plan: src_row / slot hold n' = counters[6] entries of their 2 n."""
    mask = torch.zeros(leaf.shape, dtype=torch.bool, device=leaf.device)
    mask[:int(ret[1][k, 6])] = True
    return mask


def _plan_children_written(args, ret, k, leaf):
    """sc_densify_plan: child_xyz / child_scaling [2,n,3] hold the rows of split parents only: hot && !small, from the
    header's formulae in float64 on the job's inputs (the cases keep every decision away from its threshold)."""
    scaling, accum, denom = args[1][k].double(), args[4][k].double(), args[5][k].double().reshape(-1)
    f, ip = args[9][11 * k:11 * k + 11], args[10][3 * k:3 * k + 3]
    g = accum[:, int(ip[0])] / denom
    g[g.isnan()] = 0.0
    split = (g >= f[0]) & ~(torch.exp(scaling).max(dim=1).values <= f[1])
    mask = torch.zeros(leaf.shape, dtype=torch.bool, device=leaf.device)
    mask[:, split] = True
    return mask


def _order_lists(args, ret, k, leaf):
    """The two lists of the dispatch buffer as (begin, end).  isect_bin.hip:496 hands a tile its slot inside its work class
    with an integer atomicAdd, so a list is the same SET of items in every run (the header's contract: every tile exactly
    once as kind 0 or once as each of kinds 1 and 2; scheduling only) but not the same sequence."""
    tiles = args[1].shape[0] * args[4] * args[5]
    first = tiles + tiles // 8 + 8
    return [(0, first), (first, first + tiles)]


# outputs whose elements are placed by integer atomics: compared list by list as sorted sequences, the rest bit for bit
UNORDERED = {("isect_bin_count", 5): _order_lists}

WRITTEN = {("isect_bin_sort", 1): _isect_written, ("isect_bin_sort", 2): _isect_written,
           ("isect_bin_count", 5): _order_written,
           ("densify_plan", 2): _plan_rows_written, ("densify_plan", 3): _plan_rows_written,
           ("densify_plan", 4): _plan_children_written, ("densify_plan", 5): _plan_children_written}


# ---- the harness ------------------------------------------------------------------------------------------------------
def _public():
    from street_crafter_amd import _ctypes_binding as CB
    return [n for n, f in vars(CB).items()
            if inspect.isfunction(f) and f.__module__ == CB.__name__ and not n.startswith("_")]


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _rand(shape, seed, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * torch.rand(shape, generator=torch.Generator().manual_seed(seed))).to(DEV)


class Run:
    """What a case body sees of one run: `g` guards an input (a plain copy in the plain run)."""

    def __init__(self, alloc):
        self.alloc, self.kept = alloc, []

    def g(self, t, inplace=False):
        if t is None:
            return None
        t = t.detach().to(DEV)
        if self.alloc is None:
            return t.clone(memory_format=torch.preserve_format) if inplace else t
        gt = self.alloc.guard(t)
        if not inplace:
            self.kept.append((t, gt))
        return gt


@contextlib.contextmanager
def _recorded(exact_ws):
    """Every public adapter function records (name, rc, args, returns); with exact_ws, `_ws` allocates what it is asked."""
    from street_crafter_amd import _ctypes_binding as CB
    calls, saved = [], {}

    def wrap(name, fn):
        def inner(*a, **kw):
            ret = fn(*a, **kw)
            calls.append((name, int(ret if isinstance(ret, int) else ret[0]), a, () if isinstance(ret, int) else ret))
            return ret
        return inner

    for name in _public():
        saved[name] = getattr(CB, name)
        setattr(CB, name, wrap(name, saved[name]))
    saved["_ws"] = CB._ws
    if exact_ws:
        CB._ws = lambda nbytes, device: CB.torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(CB, name, fn)


def _one_run(body, tag):
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    alloc = GuardedAlloc(*FILLS[tag]) if tag in FILLS else None
    prev = _lib.set_fast_binding(tag == "compiled")
    R.reset_state()
    run = Run(alloc)
    try:
        with _recorded(alloc is not None) as calls, (guarded_adapter(alloc) if alloc else contextlib.nullcontext()):
            out = body(run)
            torch.cuda.synchronize()
    finally:
        R.reset_state()
        _lib.set_fast_binding(prev)
    out = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    if alloc is not None:
        bad = [(i, side, off, tuple(alloc.records[i]["shape"]), alloc.records[i]["dtype"])
               for i, side, off in alloc.broken_guards()]
        assert bad == [], f"run {tag}: guard bytes changed (tensor #, side, first byte offset, shape, dtype): {bad}"
        for n, (orig, gt) in enumerate(run.kept):
            assert _same(orig, gt), f"run {tag}: guarded input #{n} {tuple(orig.shape)} {orig.dtype} was written"
    return out, calls, alloc


def _leaves(ret):
    """(top-level index, index inside a list or None, tensor or None) of everything behind the return code."""
    for i, v in enumerate(ret):
        if i == 0:
            continue
        if isinstance(v, (list, tuple)):
            for k, t in enumerate(v):
                yield i, k, t
        else:
            yield i, None, v


def _compare_calls(runs):
    plain = runs["plain"][1]
    for tag in FILLS:
        calls = runs[tag][1]
        assert [(c[0], c[1]) for c in calls] == [(c[0], c[1]) for c in plain], f"run {tag}: other calls or return codes"
    for n, (name, rc, args, ret) in enumerate(plain):
        others = {tag: list(_leaves(runs[tag][1][n][3])) for tag in FILLS}
        for j, (i, k, t) in enumerate(_leaves(ret)):
            where = f"call {n} {name} return [{i}]" + ("" if k is None else f"[{k}]")
            for tag in FILLS:
                o = others[tag][j][2]
                assert (o is None) == (t is None), where
                if t is None:
                    continue
                assert o.shape == t.shape and o.dtype == t.dtype and o.stride() == t.stride(), (where, tag)
                if (name, i) in SCRATCH or (name, i) in ATOMIC:
                    continue
                rule = WRITTEN.get((name, i))
                if rule is None:
                    assert _same(o, t), f"{where}: run {tag} differs from the plain run"
                    continue
                mask = rule(args, ret, k, t)
                exact = mask.clone()
                for a, b in (UNORDERED[(name, i)](args, ret, k, t) if (name, i) in UNORDERED else ()):
                    exact[a:b] = False               # (a list is written as a whole or not at all)
                    if bool(mask[a:b].all()):
                        assert torch.equal(o[a:b].sort().values, t[a:b].sort().values), f"{where}: other items in run {tag}"
                    else:
                        assert not bool(mask[a:b].any()), where
                assert torch.equal(o[exact], t[exact]), f"{where}: the written region differs in run {tag}"
                rest = _bits(o[~mask])
                fill = runs[tag][2].fill_of(o.dtype)
                assert bool((rest == fill).all()), f"{where}: run {tag}: an element the header leaves unwritten was written"


def sweep(body, covers, atomic=(), judge=None):
    """body(run) -> {name: tensor}; covers: the adapter functions this case is about; atomic: the names of `body`'s outputs
    that ATOMIC outputs flow into, judged by judge(outputs, tag) instead of compared."""
    runs = {tag: _one_run(body, tag) for tag in ("plain", "A", "B")}
    for tag, (out, calls, _) in runs.items():
        names = [c[0] for c in calls]
        for fn in covers:
            assert fn in names, f"run {tag}: the case never reached {fn}"
        assert all(rc == 0 for name, rc, _, _ in calls if name in covers), [(c[0], c[1]) for c in calls]
    _compare_calls(runs)
    plain = runs["plain"][0]
    for tag in FILLS:
        out = runs[tag][0]
        assert out.keys() == plain.keys()
        for k, v in plain.items():
            if k in atomic:
                continue
            if isinstance(v, torch.Tensor):
                assert _same(out[k], v), f"output {k}: run {tag} differs from the plain run"
            else:
                assert out[k] == v, (k, tag)
    assert (len(atomic) > 0) == (judge is not None)
    if judge is not None:
        for tag in runs:
            judge(runs[tag][0], tag)
    # the compiled binding allocates in C++: same shapes and dtypes for the same case
    fast, _, _ = _one_run(body, "compiled")
    assert fast.keys() == plain.keys()
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert fast[k].shape == v.shape and fast[k].dtype == v.dtype, (k, fast[k].shape, v.shape)
    return runs


# ---- inputs shared by the cases ----------------------------------------------------------------------------------------
W0, H0 = 53, 37          # neither W, H nor W * H a multiple of 4, 16 or 64
PIXEL_SIZES = [(37, 53), (37, 1), (1, 53)]
COUNTS = (1, 63, 65, 257)
_CACHE = {}


def _cameras(W=W0, H=H0):
    from street_crafter_amd.scenes import make_camera
    cams = [make_camera(W, H, 40.0, 40.0), make_camera(W, H, 40.0, 40.0, yaw=0.2, shift=(0.2, 0.0, 0.0))]
    return (torch.stack([c.viewmat for c in cams]).contiguous().to(DEV), torch.stack([c.K for c in cams]).contiguous().to(DEV))


def _scene(n, sh_degree=1):
    from street_crafter_amd.scenes import make_scene
    return make_scene(n, sh_degree=sh_degree, seed=100 + n, z_range=(1.0, 12.0), scale_range=(0.02, 0.4)).to(DEV)


def _frame(n=257, C=2, D=3, W=W0, H=H0):
    """A projected small frame with its tile lists (computed once, on the default route): plain device tensors."""
    key = (n, C, D, W, H)
    if key not in _CACHE:
        from street_crafter_amd import rendering as R
        sc = _scene(n)
        vm, Ks = _cameras(W, H)
        vm, Ks = vm[:C].contiguous(), Ks[:C].contiguous()
        tw, th = math.ceil(W / 16), math.ceil(H / 16)
        with torch.no_grad():
            radii, m2, d, con, comp = R.fully_fused_projection(sc.means, None, sc.quats, sc.scales, vm, Ks, W, H,
                                                               near_plane=0.01, far_plane=100.0, calc_compensations=True)
            prev = R.set_isect_mode("radix")
            try:
                _, ids, fids = R.isect_tiles(m2, radii, d, 16, tw, th, n_cameras=C)
                offs = R.isect_offset_encode(ids, C, tw, th)
            finally:
                R.set_isect_mode(prev)
        torch.cuda.synchronize()
        R.reset_state()
        assert fids.numel() > 0
        _CACHE[key] = dict(means2d=m2.clone(), conics=con.clone(), opacities=(sc.opacities[:, 0][None] * comp).contiguous(),
                           colors=_rand((C, n, D), 7 * n + D), radii=radii.clone(), depths=d.clone(),
                           isect_offsets=offs.clone(), flatten_ids=torch.as_tensor(fids).clone(), W=W, H=H, C=C, N=n, D=D,
                           tw=tw, th=th, scene=sc, viewmats=vm, Ks=Ks)
    return _CACHE[key]


def _grads(leaves, outs, ups):
    torch.autograd.backward(list(outs), list(ups))
    return [t.grad for t in leaves]


# ---- the cases: name -> () -> dict(body=, covers=, atomic=, judge=) ---------------------------------------------------
def case_projection():
    """fully_fused_projection and its backward: 1, 63, 65 and 257 Gaussians, two cameras, compensations."""
    from street_crafter_amd import rendering as R
    vm, Ks = _cameras()
    scenes = {n: _scene(n) for n in COUNTS}
    ups = {n: [_randn(s, 10 * n + j) for j, s in enumerate(((2, n, 2), (2, n), (2, n, 3), (2, n)))] for n in COUNTS}

    def body(r):
        out = {}
        for n, sc in scenes.items():
            leaves = [r.g(t).requires_grad_(True) for t in (sc.means, sc.quats, sc.scales)]
            radii, m2, d, con, comp = R.fully_fused_projection(leaves[0], None, leaves[1], leaves[2], r.g(vm), r.g(Ks), W0, H0,
                                                               near_plane=0.01, far_plane=100.0, calc_compensations=True)
            gs = _grads(leaves, (m2, d, con, comp), [r.g(u) for u in ups[n]])
            for k, t in zip(("radii", "means2d", "depths", "conics", "comps", "v_means", "v_quats", "v_scales"),
                            (radii, m2, d, con, comp, *gs)):
                out[f"{n}/{k}"] = t
        return out
    return dict(body=body, covers=("projection_fwd", "projection_bwd"))


def case_sh():
    """spherical_harmonics and its backward: degree 0 with K = 1, degree 3 with K = 16, degree 0 on rows padded to K = 16,
    with and without masks; 1, 63, 65 and 257 rows."""
    from street_crafter_amd import rendering as R
    cfgs = [(0, 1, 65, True), (3, 16, 257, True), (0, 16, 63, False), (3, 16, 1, False), (2, 9, 65, True)]

    def body(r):
        out = {}
        for j, (deg, K, M, masked) in enumerate(cfgs):
            dirs = r.g(_randn((M, 3), 300 + j)).requires_grad_(True)
            coeffs = r.g(_randn((M, K, 3), 400 + j)).requires_grad_(True)
            masks = r.g(_rand((M,), 500 + j) < 0.7) if masked else None
            colors = R.spherical_harmonics(deg, dirs, coeffs, masks)
            g = _grads([dirs, coeffs], [colors], [r.g(_randn((M, 3), 600 + j))])
            out.update({f"{j}/colors": colors, f"{j}/v_dirs": g[0], f"{j}/v_coeffs": g[1]})
        return out
    return dict(body=body, covers=("sh_fwd", "sh_bwd"))


def case_isect_bin():
    """isect_tiles on the tile-bucketed route, eager isect_ids: a 53x37 frame with tile 16 and 257 Gaussians under two
    cameras, and the "big splats" shape of test_isect_bucketed_route_is_bit_exact (buckets above the LDS capacity); each on
    the first call of its shape (exact sizes) and on the second (predicted capacities: the id tensors have a tail the
    header leaves unwritten)."""
    from street_crafter_amd import rendering as R
    from street_crafter_amd.scenes import make_camera, make_scene
    f = _frame()
    frames = [(f["means2d"], f["radii"], f["depths"], f["tw"], f["th"], 2)]
    sc = make_scene(25_000, seed=31, scale_range=(0.5, 4.0)).to(DEV)
    cam = make_camera(1920, 1280, 2050.0, 2050.0).to(DEV)
    with torch.no_grad():
        radii, m2, d, _, _ = R.fully_fused_projection(sc.means, None, sc.quats, sc.scales, cam.viewmat[None].contiguous(),
                                                      cam.K[None].contiguous(), 1920, 1280, near_plane=0.001, far_plane=1000.0)
    frames.append((m2.clone(), radii.clone(), d.clone(), 120, 80, 1))
    torch.cuda.synchronize()

    def body(r):
        out = {}
        prev = (R.set_isect_mode("bin"), R.set_lazy_isect_ids(False), R.set_deferred_isect(False))
        try:
            for j, (m2, radii, d, tw, th, C) in enumerate(frames):
                gm, gd = r.g(m2), r.g(d)
                for rep in range(2):
                    tpg, ids, fids = R.isect_tiles(gm, radii, gd, 16, tw, th, n_cameras=C)
                    offs = R.isect_offset_encode(ids, C, tw, th)
                    out.update({f"{j}.{rep}/tiles_per_gauss": tpg, f"{j}.{rep}/isect_ids": torch.as_tensor(ids),
                                f"{j}.{rep}/flatten_ids": torch.as_tensor(fids), f"{j}.{rep}/offsets": offs})
        finally:
            R.set_isect_mode(prev[0]), R.set_lazy_isect_ids(prev[1]), R.set_deferred_isect(prev[2])
        return out
    return dict(body=body, covers=("isect_bin_count", "isect_bin_sort"))


RASTER_CASES = ("two_cameras-D4bg-masks", "ragged-D3", "channels-D1bg", "channels-D7bg", "edge-finite129-D3")


def case_rasterize():
    """rasterize_to_pixels under grad (sc_rasterize_fwd with last_ids) and its backward with absgrad, on cases of
    oracle/raster_bwd_cases.py: two cameras with backgrounds and masked tiles, 1, 3, 4 and 7 channels on the ragged frame
    (partial last tile row and column) and the hand-built lists of 63 / 64 / 65 / 129 records.  The five gradients are
    float atomics: judged per row by RC.worst_ratios under K = 4 K_ref, K_ref the largest ratio of the float32 replay over
    the random scenes USED HERE (a subset of that module's cases: never above its K)."""
    from oracle import raster_bwd_cases as RC
    from street_crafter_amd import rendering as R
    table, k_ref, own = {}, 0.0, {}
    for cid in RASTER_CASES:
        p = RC.make_case(cid)
        ref = RC.reference(p)
        rep = RC.worst_ratios(RC.reference(p, np.float32)["G"], ref, RC.outputs_of(p))
        own[cid] = max(v for v, _ in rep.values())
        if cid not in RC.EDGE_IDS:
            k_ref = max(k_ref, own[cid])
        table[cid] = (p, ref)
    K = {cid: 4.0 * (own[cid] if cid in RC.EDGE_IDS and own[cid] > k_ref else k_ref) for cid in table}
    names = ("means2d", "conics", "colors", "opacities")

    def body(r):
        out = {}
        for cid, (p, _) in table.items():
            src = [r.g(_dev(p[k])).requires_grad_(True) for k in names]
            bg = None if p["backgrounds"] is None else r.g(_dev(p["backgrounds"])).requires_grad_(True)
            masks = None if p["masks"] is None else r.g(_dev(p["masks"]))
            rc, ra = R.rasterize_to_pixels(*src, p["width"], p["height"], p["tile_size"], _dev(p["isect_offsets"], torch.int32),
                                           _dev(p["flatten_ids"], torch.int32), backgrounds=bg, masks=masks, absgrad=True)
            torch.autograd.backward([rc, ra], [r.g(_dev(p["v_colors"])), r.g(_dev(p["v_alphas"]))])
            out.update({f"{cid}/render_colors": rc, f"{cid}/render_alphas": ra, f"{cid}/g/absgrad": src[0].absgrad})
            out.update({f"{cid}/g/{k}": t.grad for k, t in zip(names, src)})
            if bg is not None:
                out[f"{cid}/backgrounds_grad"] = bg.grad
        return out

    def judge(out, tag):
        for cid, (p, ref) in table.items():
            got = {k: out[f"{cid}/g/{k}"].cpu().numpy() for k in names + ("absgrad",)}
            if p["backgrounds"] is not None:
                got["backgrounds"] = out[f"{cid}/backgrounds_grad"].cpu().numpy()
            for k, (ratio, off) in RC.worst_ratios(got, ref, RC.outputs_of(p)).items():
                assert np.isfinite(got[k]).all() and off == 0.0 and ratio <= K[cid], (tag, cid, k, ratio, off, K[cid])

    atomic = [f"{cid}/g/{k}" for cid in table for k in names + ("absgrad",)]
    return dict(body=body, covers=("rasterize_fwd", "rasterize_bwd"), atomic=atomic, judge=judge)


def case_rasterize_planar():
    """rasterize_to_pixels under no_grad with planar output (tile 16, 3 and 4 channels): 257 Gaussians on 53x37 under two
    cameras with backgrounds, and the hand-built lists of 63 / 64 / 65 / 129 records."""
    from oracle import raster_bwd_cases as RC
    from street_crafter_amd import rendering as R
    frames = []
    for D in (3, 4):
        f = _frame(D=D)
        frames.append(({k: f[k] for k in ("means2d", "conics", "colors", "opacities")}, f["W"], f["H"], f["isect_offsets"],
                       f["flatten_ids"], _rand((2, D), 900 + D)))
    for cid in ("edge-finite-D4bg", "edge-finite129-D3"):
        p = RC.make_case(cid)
        frames.append(({k: _dev(p[k]) for k in ("means2d", "conics", "colors", "opacities")}, p["width"], p["height"],
                       _dev(p["isect_offsets"], torch.int32), _dev(p["flatten_ids"], torch.int32), None))

    def body(r):
        out = {}
        prev = R.set_planar_output(True)
        try:
            with torch.no_grad():
                for j, (src, W, H, offs, fids, bg) in enumerate(frames):
                    rc, ra = R.rasterize_to_pixels(*[r.g(t) for t in src.values()], W, H, 16, offs, fids, backgrounds=r.g(bg))
                    assert not rc.is_contiguous()
                    out.update({f"{j}/render_colors": rc, f"{j}/render_alphas": ra})
        finally:
            R.set_planar_output(prev)
        return out
    return dict(body=body, covers=("rasterize_fwd_planar",))


def _group_ids(n):
    u = np.random.default_rng(7).random(n)
    return _dev(np.where(u < 0.7, 0, np.where(u < 0.9, 1, 255)).astype(np.uint8))


def case_rasterize_groups():
    """rasterize_to_pixels_grouped (forward only, with the extents): 3 and 4 channels (the operator takes no others), 257
    and 65 Gaussians, two cameras, one and two groups."""
    from street_crafter_amd.groups import rasterize_to_pixels_grouped
    frames = [_frame(D=3), _frame(D=4), _frame(n=65, D=4)]

    def body(r):
        out = {}
        with torch.no_grad():
            for f in frames:
                for G in (2, 1):
                    res = rasterize_to_pixels_grouped(*[r.g(f[k]) for k in ("means2d", "conics", "colors", "opacities")], f["W"], f["H"],
                                                      16, f["isect_offsets"], f["flatten_ids"], _group_ids(f["N"]), n_groups=G,
                                                      return_extents=True)
                    out.update({f"N{f['N']}D{f['D']}G{G}/{k}": t for k, t in enumerate(res)})
        return out
    return dict(body=body, covers=("rasterize_fwd_groups",))


def case_rasterize_groups_train():
    """rasterize_to_pixels_grouped_train and its backward on the "ragged" and "two_cameras" scenes of
    tests/test_groups_bwd_gpu.py (4 channels, all four images differentiated, absgrad).  The gradients are float atomics:
    judged per row by that module's reference under K = 4 K_ref, K_ref from the float32 replay of the cases used here."""
    import test_groups_bwd_gpu as GB
    from oracle import raster_bwd_cases as RC
    from street_crafter_amd.groups import rasterize_to_pixels_grouped_train
    table, k_ref = {}, 0.0
    for scene in ("ragged", "two_cameras"):
        p = GB.make_inputs(scene, 4)
        ref, replay = GB.build_references(p)["all"]
        k_ref = max(k_ref, max(v for v, _ in RC.worst_ratios(replay, ref, GB.NAMES).values()))
        table[scene] = (p, ref)

    def body(r):
        out = {}
        for scene, (p, _) in table.items():
            src = [r.g(_dev(p[k])).requires_grad_(True) for k in GB.GRADS]
            imgs = rasterize_to_pixels_grouped_train(*src, p["width"], p["height"], 16, _dev(p["isect_offsets"], torch.int32),
                                                     _dev(p["flatten_ids"], torch.int32), _dev(p["group_ids"]), n_groups=2,
                                                     absgrad=True)
            torch.autograd.backward(list(imgs), [r.g(_dev(p["up"][k])) for k in ("rc", "ra", "gc", "ga")])
            out.update({f"{scene}/image{k}": t for k, t in enumerate(imgs)})
            out.update({f"{scene}/g/{k}": t.grad for k, t in zip(GB.GRADS, src)})
            out[f"{scene}/g/absgrad"] = src[0].absgrad
        return out

    def judge(out, tag):
        for scene, (p, ref) in table.items():
            got = {k: out[f"{scene}/g/{k}"].cpu().numpy() for k in GB.NAMES}
            for k, (ratio, off) in RC.worst_ratios(got, ref, GB.NAMES).items():
                assert np.isfinite(got[k]).all() and off == 0.0 and ratio <= 4.0 * k_ref, (tag, scene, k, ratio, off, 4.0 * k_ref)

    atomic = [f"{scene}/g/{k}" for scene in table for k in GB.NAMES]
    return dict(body=body, covers=("rasterize_fwd_groups_ids", "rasterize_bwd_groups"), atomic=atomic, judge=judge)


def case_rasterize_layers():
    """rasterize_to_pixels_layered (four images and layer_begin) on 257 Gaussians of which 65 are the back layer, 3 and 4
    channels, two cameras; novel_view_frame with float output and with uint8 output into a guarded `out`, both roundings."""
    from street_crafter_amd import layers as L
    from street_crafter_amd import rendering as R
    n_front = 192
    frames = []
    for D in (3, 4):
        f = dict(_frame(D=D))
        with torch.no_grad():
            keys = L.layered_depths(f["depths"], n_front)
            prev = R.set_isect_mode("radix")
            try:
                _, ids, fids = R.isect_tiles(f["means2d"], f["radii"], keys, 16, f["tw"], f["th"], n_cameras=2)
                f["isect_offsets"], f["flatten_ids"] = R.isect_offset_encode(ids, 2, f["tw"], f["th"]).clone(), torch.as_tensor(fids).clone()
            finally:
                R.set_isect_mode(prev)
        frames.append(f)
    torch.cuda.synchronize()
    R.reset_state()
    sc = _scene(257, sh_degree=3)
    vm, Ks = _cameras()

    def body(r):
        out = {}
        with torch.no_grad():
            for f in frames:
                res = L.rasterize_to_pixels_layered(*[r.g(f[k]) for k in ("means2d", "conics", "colors", "opacities")], W0, H0, 16,
                                                    f["isect_offsets"], f["flatten_ids"], n_front, return_layer_begin=True)
                out.update({f"D{f['D']}/{k}": t for k, t in enumerate(res)})
            args = [r.g(t) for t in (sc.means, sc.quats, sc.scales, sc.opacities[:, 0].contiguous(), sc.sh, vm[0].contiguous(),
                                     Ks[0].contiguous())]
            kw = dict(near_plane=0.01, far_plane=100.0, sh_degree=3)
            fl = L.novel_view_frame(*args, W0, H0, n_front, output="float", **kw)
            out.update({f"float/{k}": t for k, t in fl.items()})
            for rounding in ("video", "save_image"):
                buf = r.g(torch.zeros(H0, W0, 3, dtype=torch.uint8), inplace=True)
                got = L.novel_view_frame(*args, W0, H0, n_front, output="u8", rounding=rounding, out=buf, **kw)
                assert got.data_ptr() == buf.data_ptr()
                out[f"u8/{rounding}"] = buf
        return out
    return dict(body=body, covers=("rasterize_fwd_layers",))


def case_projection_sh():
    """The fused projection + SH node of rasterization() under grad (_ProjectionSh: sc_projection_sh_fwd with the separate
    arrays, sc_projection_sh_bwd): SH degree 0 with K = 1 and degree 3 with K = 16; 1, 63, 65 and 257 Gaussians; two
    cameras.  The node is applied directly, so that its upstream gradients are guarded inputs and not the rasterizer's
    atomically summed ones."""
    from street_crafter_amd import rendering as R
    vm, Ks = _cameras()
    centers = R.camera_centers(vm)
    cfgs = [(1, 0), (63, 3), (65, 0), (257, 3)]
    scenes = {n: _scene(n, sh_degree=deg) for n, deg in cfgs}
    shapes = lambda n: ((2, n, 2), (2, n), (2, n, 3), (2, n), (2, n, 4))          # noqa: E731
    torch.cuda.synchronize()

    def body(r):
        out = {}
        for n, deg in cfgs:
            sc = scenes[n]
            assert sc.sh.shape[1] == (deg + 1) ** 2
            leaves = [r.g(t).requires_grad_(True) for t in (sc.means, sc.quats, sc.scales, sc.opacities[:, 0].contiguous(), sc.sh)]
            res = R._ProjectionSh.apply(*leaves, r.g(vm), r.g(Ks), r.g(centers), deg, W0, H0, 0.3, 0.01, 100.0, 0.0, True)
            gs = _grads(leaves, res[1:], [r.g(_randn(s, 40 * n + j)) for j, s in enumerate(shapes(n))])
            out.update({f"{n}/out{k}": t for k, t in enumerate(res)})
            out.update({f"{n}/grad{k}": t for k, t in enumerate(gs)})
        return out
    return dict(body=body, covers=("projection_sh_fwd", "projection_sh_bwd"))


def case_rasterization_fused():
    """rasterization() under no_grad, fused: packed records into sc_rasterize_fwd_packed (both depth modes) and the
    separate arrays; SH degree 3 with K = 16, 257 and 65 Gaussians, two cameras, backgrounds."""
    from street_crafter_amd import rendering as R
    vm, Ks = _cameras()
    scenes = [_scene(n, sh_degree=3) for n in (257, 65)]
    bg = _rand((2, 3), 77)

    def body(r):
        out = {}
        with torch.no_grad():
            for sc in scenes:
                args = [r.g(t) for t in (sc.means, sc.quats, sc.scales, sc.opacities[:, 0].contiguous(), sc.sh, vm, Ks)]
                for packed in (True, False):
                    prev = R.set_packed_records(packed)
                    try:
                        for mode in ("RGB+ED", "RGB+D"):
                            colors, alphas, meta = R.rasterization(*args, W0, H0, near_plane=0.01, far_plane=100.0, sh_degree=3,
                                                                   render_mode=mode, rasterize_mode="antialiased", backgrounds=r.g(bg))
                            assert meta["fused"] is True
                            tag = f"{sc.means.shape[0]}/{packed}/{mode}"
                            out.update({f"{tag}/colors": colors, f"{tag}/alphas": alphas})
                            out.update({f"{tag}/{k}": meta[k].clone()
                                        for k in ("radii", "means2d", "depths", "conics", "opacities", "colors", "flatten_ids")})
                    finally:
                        R.set_packed_records(prev)
        return out
    return dict(body=body, covers=("projection_sh_fwd", "rasterize_fwd_packed"))


def case_frame_composite_u8():
    """dist.to_uint8_frame on the renderer's permuted [H,W,4] views (the interleaved entry) and on planes (the strided
    entry): 1, 3, 5 and 37 * 53 pixels -- the 4-pixel epilogue's tails --, with and without the sky composite, both
    roundings, into a guarded `out`."""
    from street_crafter_amd import dist
    sizes = [(1, 1), (1, 3), (5, 1), (37, 53)]

    def body(r):
        out = {}
        for H, W in sizes:
            hwc = [r.g(_rand((H, W, 4), 10 * H + W + j, -0.2, 1.2)) for j in range(2)]
            planes = [r.g(_rand((4, H, W), 20 * H + W + j, -0.2, 1.2)) for j in range(2)]
            acc = r.g(_rand((H, W, 1), 30 * H + W))
            for name, (fg, sky) in (("hwc", [t.permute(2, 0, 1)[:3] for t in hwc]), ("planes", [t[:3] for t in planes])):
                for rounding in ("video", "save_image"):
                    for with_sky in (False, True):
                        buf = r.g(torch.zeros(H, W, 3, dtype=torch.uint8), inplace=True)
                        dist.to_uint8_frame(fg, acc=acc if with_sky else None, sky_rgb_chw=sky if with_sky else None,
                                            rounding=rounding, out=buf)
                        out[f"{H}x{W}/{name}/{rounding}/{with_sky}"] = buf
        return out
    return dict(body=body, covers=("frame_composite_u8", "frame_composite_u8_strided"))


def case_loss():
    """l1_and_ssim and its backward with respect to both images, with a mask: 37x53, width 1, height 1, and a batch of
    two through ssim(size_average=False).
  (The adapter allocates max(ws_bytes, 8) here and passes ws_bytes on: a reported size below 8 bytes is hidden.)"""
    from street_crafter_amd import losses

    def body(r):
        out = {}
        for H, W in PIXEL_SIZES:
            a = r.g(_rand((3, H, W), H + W)).requires_grad_(True)
            b = r.g(_rand((3, H, W), H + W + 1)).requires_grad_(True)
            m = r.g(_rand((1, H, W), H + W + 2) < 0.8)
            l1, s = losses.l1_and_ssim(a, b, m)
            (0.8 * l1 + 0.2 * (1.0 - s)).backward()
            out.update({f"{H}x{W}/l1": l1, f"{H}x{W}/ssim": s, f"{H}x{W}/g1": a.grad, f"{H}x{W}/g2": b.grad})
        a = r.g(_rand((2, 3, H0, W0), 5)).requires_grad_(True)
        b = r.g(_rand((2, 3, H0, W0), 6))
        s = losses.ssim(a, b, size_average=False)
        s.sum().backward()
        out.update({"batch/ssim": s, "batch/g1": a.grad})
        return out
    return dict(body=body, covers=("loss_fwd", "loss_bwd"))


def case_depth_trim():
    """lidar_depth_loss and its backward (depth and LiDAR depth), with a mask: 37x53, width 1, height 1.
  (The adapter allocates max(ws_bytes, 8) here and passes ws_bytes on: a reported size below 8 bytes is hidden.)"""
    from street_crafter_amd import regularizers as RG

    def body(r):
        out = {}
        for H, W in PIXEL_SIZES:
            depth = r.g(_rand((1, H, W), 3 * H + W, 0.5, 30.0)).requires_grad_(True)
            lidar = _rand((1, H, W), 3 * H + W + 1, 0.5, 30.0)
            lidar[_rand((1, H, W), 3 * H + W + 2) < 0.3] = 0.0
            lidar = r.g(lidar).requires_grad_(True)
            mask = r.g(_rand((1, H, W), 3 * H + W + 3) < 0.9)
            v = RG.lidar_depth_loss(depth, lidar, mask)
            v.backward()
            fw = RG.lidar_depth_forward(depth.detach(), lidar.detach(), mask)
            out.update({f"{H}x{W}/value": v, f"{H}x{W}/g_depth": depth.grad, f"{H}x{W}/g_lidar": lidar.grad})
            out.update({f"{H}x{W}/fw{k}": t for k, t in enumerate(fw)})
        return out
    return dict(body=body, covers=("depth_trim_fwd", "depth_trim_bwd"))


def case_acc_reg():
    """sky_loss and obj_acc_loss with their backward: 37x53, width 1, height 1; a mask of one and of three channels.
  (The adapter allocates max(ws_bytes, 8) here and passes ws_bytes on: a reported size below 8 bytes is hidden.)"""
    from street_crafter_amd import regularizers as RG

    def body(r):
        out = {}
        for H, W in PIXEL_SIZES:
            for name, fn, Cm in (("sky", RG.sky_loss, 1), ("obj", RG.obj_acc_loss, 1), ("sky3", RG.sky_loss, 3)):
                acc = r.g(_rand((1, H, W), 5 * H + W + Cm)).requires_grad_(True)
                mask = r.g(_rand((Cm, H, W), 5 * H + W + 1 + Cm) < 0.4)
                v = fn(acc, mask)
                v.backward()
                out.update({f"{H}x{W}/{name}/value": v, f"{H}x{W}/{name}/grad": acc.grad})
        return out
    return dict(body=body, covers=("acc_reg_fwd", "acc_reg_bwd"))


def case_frame_tail():
    """frame_tail and its backward (colours, alphas, sky, affine): 37x53, width 1, height 1; 3 and 4 channels; the sky as the
    [..., :3] view of a 4-channel render and as planes; the clamped forward.
  (The adapter allocates max(ws_bytes, 8) here and passes ws_bytes on: a reported size below 8 bytes is hidden.)"""
    import frame_tail_ref as FT
    from street_crafter_amd import frame_tail as M

    def body(r):
        out = {}
        for H, W in PIXEL_SIZES:
            inp = FT.inputs(H, W, 11 * H + W)
            for D, kind in ((4, "view4"), (3, "planes")):
                cs = FT.case(inp, kind, True, D, device=DEV)
                sky = r.g(cs["sky"])
                assert sky.stride() == cs["sky"].stride()
                leaves = [r.g(cs["colors"]), r.g(cs["alphas"]), sky, r.g(cs["affine"])]
                for t in leaves:
                    t.requires_grad_(True)
                res = M.frame_tail(*leaves)
                outs, ups = [res.rgb], [r.g(inp["g"])]
                if res.depth is not None:
                    outs.append(res.depth)
                    ups.append(r.g(inp["h"]))
                gs = _grads(leaves, outs, ups)
                with torch.no_grad():
                    clamped = M.frame_tail(*[t.detach() for t in leaves], clamp=True)
                tag = f"{H}x{W}/D{D}"
                out.update({f"{tag}/rgb": res.rgb, f"{tag}/depth": res.depth, f"{tag}/rgb_clamped": clamped.rgb})
                out.update({f"{tag}/grad{k}": t for k, t in enumerate(gs)})
        return out
    return dict(body=body, covers=("frame_tail_fwd", "frame_tail_bwd"))


def case_cubemap():
    """texture_cube (R = 5, n = 37 * 61 directions, 1, 3 and 4 channels, with the sigmoid) and sky_color (37 wide, 61 high,
    acc mask, perturbation) with their backward.  grad_tex is accumulated with float atomics: judged per texel-channel by
    tests/cubemap_ref.py's reference under the bars of tests/test_cubemap_gpu.py (k_b = 4 K_BWD_REPLAY; for sky_color with
    that module's term for the directions formed in the kernel)."""
    import cubemap_ref as CR
    from street_crafter_amd import cubemap as CM
    R, n = 5, 37 * 61
    EPS, K_BWD = CR.EPS, 4.0 * CR.K_BWD_REPLAY
    dirs = CR.random_dirs(R)[:n]
    tp = CR.taps(dirs, R)
    excluded = CR.excluded(tp, R)
    table = {}
    for C in CR.CHANNELS:
        tex, g = CR.texture(R, C), CR.upstream(n, C)
        g[excluded] = 0
        table[C] = (tex, g, CR.backward(tex, dirs, g, "sigmoid", tp=tp))
    import test_cubemap_gpu as TC
    H, W = TC.H, TC.W                                       # 61 x 37
    Kc, Rm, T = TC._camera(R)
    perturb = np.random.default_rng(4).uniform(0, 1, (H, W, 2)).astype(np.float32)
    acc = np.random.default_rng(1).uniform(0.99, 1, (1, H, W)).astype(np.float32)
    sky_mask = ((1 - torch.from_numpy(acc)[0]) > 1e-3).numpy().reshape(-1)          # torch's fp32 expression, as that module
    assert 0 < sky_mask.sum() < sky_mask.size
    sky_dirs, e_rel = TC._sky_reference(CM, Kc, Rm, perturb)
    sky_tp = CR.taps(sky_dirs, R)
    sky_g = CR.upstream(H * W, 3, seed=R)
    sky_g[CR.excluded(sky_tp, R)] = 0
    sky_b = CR.backward(table[3][0], sky_dirs, sky_g * sky_mask[:, None], "sigmoid", tp=sky_tp)

    def body(r):
        out = {}
        for C, (tex, g, _) in table.items():
            t = r.g(_dev(tex)).requires_grad_(True)
            o = CM.texture_cube(t, r.g(_dev(dirs)), "sigmoid")
            o.backward(r.g(_dev(g)))
            out.update({f"C{C}/out": o, f"C{C}/grad_tex": t.grad})
        cube = r.g(_dev(table[3][0])).requires_grad_(True)
        sky = CM.sky_color(cube, Kc, torch.tensor(Rm), T, H, W, acc=r.g(_dev(acc)), perturb=r.g(_dev(perturb)),
                           white_background=True)
        sky.backward(r.g(_dev(np.ascontiguousarray(sky_g.T.reshape(3, H, W)))))
        out.update({"sky/out": sky, "sky/grad_tex": cube.grad})
        return out

    def judge(out, tag):
        for C, (tex, g, b) in table.items():
            grad = out[f"C{C}/grad_tex"].cpu().numpy().astype(np.float64).reshape(-1, C)
            bar = EPS * (b["n"] * b["S"] + K_BWD * (b["S"] + R * b["A"]))
            assert (np.abs(grad - b["grad"]) <= bar).all() and (grad[b["n"] == 0] == 0).all(), (tag, C)
        # sky_color forms its directions in the kernel in fp32: that module's extra term 4 R max(e / ma) A
        grad = out["sky/grad_tex"].cpu().numpy().astype(np.float64).reshape(-1, 3)
        bar = TC._bwd_bar(sky_b, R, extra=4 * R * float(e_rel.max()))
        assert (np.abs(grad - sky_b["grad"]) <= bar).all() and (grad[sky_b["n"] == 0] == 0).all(), (tag, "sky")

    atomic = [f"C{C}/grad_tex" for C in table] + ["sky/grad_tex"]
    return dict(body=body, covers=("cubemap_fwd", "cubemap_bwd"), atomic=atomic, judge=judge)


def case_lpips_prep():
    """lpips.prepare and its backward on [3,H,W] images read through the strides of an [H,W,4] render, with a mask:
    37x53, width 1, height 1."""
    from street_crafter_amd import lpips as LP

    def body(r):
        out = {}
        for H, W in PIXEL_SIZES:
            img = r.g(_rand((H, W, 4), 7 * H + W)).requires_grad_(True)
            mask = r.g(_rand((1, H, W), 7 * H + W + 1) < 0.8)
            z = LP.prepare(img.permute(2, 0, 1)[:3], mask)
            z.backward(r.g(_randn((1, 3, H, W), 7 * H + W + 2)))
            out.update({f"{H}x{W}/z": z, f"{H}x{W}/grad": img.grad})
        return out
    return dict(body=body, covers=("lpips_prep_fwd", "lpips_prep_bwd"))


def case_lpips_head():
    """lpips_distance and its backward over taps of (channels, pixels) = (1, 1), (3, 63), (3, 65), (64, 77) and (7, 257), one
    of them a strided view; gradients of both feature lists.  (The workspace is allocated in whole float64 words, at least
    one, and the reported byte count is passed on.)"""
    from street_crafter_amd import lpips as LP
    shapes = [(1, 1, 1), (3, 7, 9), (3, 5, 13), (64, 7, 11), (7, 1, 257)]

    def body(r):
        fx, fy, ws = [], [], []
        for j, (C, h, w) in enumerate(shapes):
            if j == 3:           # channel stride above h * w: a slice of a larger feature map, read in place
                big = [r.g(_randn((C, h + 2, w), 50 + j + k)) for k in range(2)]
                x, y = (t[:, :h].requires_grad_(True) for t in big)
                assert not x.is_contiguous()
            else:
                x, y = (r.g(_randn((C, h, w), 50 + j + 10 * k)).requires_grad_(True) for k in range(2))
            fx.append(x), fy.append(y), ws.append(r.g(_rand((C,), 90 + j)))
        total, taps = LP.lpips_distance(fx, fy, ws, return_taps=True)
        total.backward(r.g(_dev(torch.full((1, 1, 1, 1), 0.7))))
        out = {"total": total, "taps": taps}
        for j, (x, y) in enumerate(zip(fx, fy)):
            out.update({f"gx{j}": x.grad, f"gy{j}": y.grad})
        return out
    return dict(body=body, covers=("lpips_head_fwd", "lpips_head_bwd"))


def case_resize():
    """preprocess_tensor (crop + antialiased resize, rows from row_begin, scale and shift) of fp32 images and bool masks
    with the backward, on the shapes of tests/resize_ref.py and a 37x53 image; resize of one plane, of a column and a row."""
    import resize_ref as RR
    from street_crafter_amd import resize as RZ
    TH, TW = RR.TARGET
    shapes = [RR.SHAPES[0], RR.SHAPES[2], (3, 37, 53)]

    def body(r):
        out = {}
        for j, shape in enumerate(shapes):
            x = r.g(_dev(RR.image(shape, j))).requires_grad_(True)
            m = r.g(_dev(RR.mask(shape, 0.6, j)))
            for aa in (True, False):
                y = RZ.preprocess_tensor(x, TH, TW, aa, row_begin=RR.UPPER, scale=2.0, shift=-1.0)
                y.backward(r.g(_randn(tuple(y.shape), 70 + j)))
                out.update({f"{j}/{aa}/out": y, f"{j}/{aa}/grad": x.grad.clone(), f"{j}/{aa}/mask": RZ.preprocess_tensor(m, TH, TW, aa)})
                x.grad = None
        for name, shape, size in (("plane", (29, 50), (18, 32)), ("column", (3, 37, 1), (18, 1)), ("row", (3, 1, 53), (1, 32))):
            x = r.g(_rand(shape, 80 + len(name), -1.0, 1.0)).requires_grad_(True)
            y = RZ.resize(x, size)
            y.backward(r.g(_randn(tuple(y.shape), 85 + len(name))))
            out.update({f"{name}/out": y, f"{name}/grad": x.grad})
        return out
    return dict(body=body, covers=("resize_fwd", "resize_mask_fwd", "resize_bwd"))


def case_adam():
    """One table of tensors of 1, 3, 5, 257 and 4099 elements through two Adam steps: the parameters and both moments are
    guarded in-place buffers, the gradients guarded inputs."""
    from street_crafter_amd import optim
    lengths = [1, 3, 5, 257, 4099]

    def body(r):
        params = [torch.nn.Parameter(r.g(_randn((n,), n), inplace=True)) for n in lengths]
        opt = optim.Adam([{"params": [p], "lr": 1e-2 * (1 + i), "name": f"g{i}"} for i, p in enumerate(params)], lr=0.0, eps=1e-15)
        for i, p in enumerate(params):
            opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": r.g(_randn((p.numel(),), 1000 + i, 0.1), inplace=True),
                            "exp_avg_sq": r.g(_rand((p.numel(),), 2000 + i, 0.0, 0.1), inplace=True)}
        for step in range(2):
            for i, p in enumerate(params):
                p.grad = r.g(_randn((p.numel(),), 3000 + 10 * step + i))
            opt.step()
        out = {}
        for i, p in enumerate(params):
            out.update({f"{i}/param": p.detach(), f"{i}/exp_avg": opt.state[p]["exp_avg"], f"{i}/exp_avg_sq": opt.state[p]["exp_avg_sq"]})
        return out
    return dict(body=body, covers=("adam_step",))


def case_densify_stats():
    """accumulate_fused over renders of 1, 63, 65 and 257 rows cut into segments with a gap: the accumulators are guarded
    in-place buffers (rows outside every segment included), gradients and the visibility mask guarded inputs."""
    from street_crafter_amd import densify_stats as DS
    from test_optim_cpu import stats_buffers, stats_case

    def body(r):
        out = {}
        for N in COUNTS:
            vp, radii, vis = stats_case(N, N, device=DEV)
            vp.grad, vp.absgrad, vis = r.g(vp.grad), r.g(vp.absgrad), r.g(vis)
            acc, den, mr = (r.g(t, inplace=True) for t in stats_buffers(N, N, device=DEV))
            spans = [(0, N // 3), (N // 3 + 1, N)] if N > 3 else [(0, N)]          # (row N // 3 lies in no segment)
            segs = [(a, b, acc[a:b], den[a:b], mr[a:b]) for a, b in spans]
            DS.accumulate_fused(segs, radii.to(DEV), vis, vp, 1600, 1066)
            out.update({f"{N}/acc": acc, f"{N}/denom": den, f"{N}/max_radii": mr})
        return out
    return dict(body=body, covers=("densify_stats",))


def case_densify():
    """densify_and_prune_many (sc_densify_plan, then sc_densify_apply) over three jobs of 1, 65 and 2 B + 1 rows (B the
    scan block): sphere, box and no region; parameters, moments, statistics and noise are guarded inputs."""
    import test_densify_gpu as TD
    from street_crafter_amd import densify, optim
    B = densify.scan_block()
    cases = [TD.make_case(n, 40 + j, mode="mixed", region=reg) for j, (n, reg) in enumerate(((1, "sphere"), (65, "box"), (2 * B + 1, None)))]
    for c in cases:
        TD.assert_margins(c)

    def body(r):
        jobs = []
        for c in cases:
            params = {k: torch.nn.Parameter(r.g(v.to(DEV))) for k, v in c.tensors.items()}
            opt = optim.Adam([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
            for k, p in params.items():
                if c.moments[k] is not None:
                    opt.state[p] = {"step": torch.tensor(5.0), "exp_avg": r.g(c.moments[k][0].to(DEV)),
                                    "exp_avg_sq": r.g(c.moments[k][1].to(DEV))}
            jobs.append(densify.DensifyJob(optimizer=opt, xyz_gradient_accum=r.g(c.acc.to(DEV)), denom=r.g(c.denom.to(DEV)),
                                           max_radii2D=r.g(c.max_radii.to(DEV)), split_noise=r.g(c.split_noise.to(DEV)),
                                           box_noise=r.g(c.box_noise.to(DEV)), **c.cfg))
        out = {}
        for j, (job, res) in enumerate(zip(jobs, densify.densify_and_prune_many(jobs))):
            out.update({f"{j}/{k}": p.detach() for k, p in res.params.items()})
            for k, p in res.params.items():
                st = job.optimizer.state.get(p)
                if st:
                    out.update({f"{j}/{k}/exp_avg": st["exp_avg"], f"{j}/{k}/exp_avg_sq": st["exp_avg_sq"]})
            out.update({f"{j}/src_row": res.src_row, f"{j}/slot": res.slot, f"{j}/counters": tuple(sorted(res.scalar_dict.items())),
                        f"{j}/n_out": res.n_out})
        return out
    return dict(body=body, covers=("densify_plan", "densify_apply"))


def case_compose():
    """compose_frame and its backward on the "actors_only" case of tests/compose_ref.py (segments of 257, 65 and 63 rows at
    odd starts, K = 16, Fourier dimensions 2 and 5, a mixed flip mask, sky rows).  The pose gradients are summed with float
    atomics: judged by compose_ref.worst under K = 4 K_REF, as tests/test_compose_gpu.py judges them."""
    import compose_ref as CRF
    from street_crafter_amd import compose as CP
    case = [c for c in CRF.build_cases() if c["name"] == "actors_only"][0]
    G, S = CRF.run(case, torch.float64), CRF.track(case)[1]
    K_BAR = 4.0 * CRF.K_REF

    def body(r):
        models = []
        for m in case["models"]:
            t = {k: r.g(m[k]).requires_grad_(True) for k in CRF.PARAMS}
            models.append(CP.FrameModel(name=m["name"], kind=m["kind"], start_frame=m["start_frame"], end_frame=m["end_frame"],
                                        fourier_scale=m["fourier_scale"], centre=m["centre"], radius=m["radius"], **t))
        rots, trans = (r.g(case[k]).requires_grad_(True) for k in ("obj_rots", "obj_trans"))
        flip = {k: r.g(v) for k, v in case["flip"].items()}
        rows = {m.name: i for i, m in enumerate(m for m in models if m.kind == CP.ACTOR)}
        *outs, _ranges = CP.compose_frame(models, rots, trans, case["frame"], flip=flip, flip_q=case["flip_q"], actor_rows=rows)
        live = [(t, r.g(case["ups"][k])) for k, t in zip(CRF.OUTPUTS, outs) if case["ups"].get(k) is not None]
        torch.autograd.backward([t for t, _ in live], [g for _, g in live])
        out = dict(zip(CRF.OUTPUTS, outs))
        for m in models:
            out.update({f"g/{m.name}/{k}": getattr(m, k).grad for k in CRF.PARAMS})
        out.update({"g/obj_rots": rots.grad, "g/obj_trans": trans.grad})
        return out

    def judge(out, tag):
        for key in ("g/obj_rots", "g/obj_trans"):
            ratio, _ = CRF.worst({key: out[key].cpu().double().numpy()}, G, S, [key])
            assert ratio <= K_BAR, (tag, key, ratio, K_BAR)

    return dict(body=body, covers=("compose_fwd", "compose_bwd"), atomic=["g/obj_rots", "g/obj_trans"], judge=judge)


CASES = {name[5:]: fn for name, fn in sorted(globals().items()) if name.startswith("case_") and callable(fn)}
COVERS = {"projection": ("projection_fwd", "projection_bwd"), "sh": ("sh_fwd", "sh_bwd"),
          "isect_bin": ("isect_bin_count", "isect_bin_sort"), "rasterize": ("rasterize_fwd", "rasterize_bwd"),
          "rasterize_planar": ("rasterize_fwd_planar",), "rasterize_groups": ("rasterize_fwd_groups",),
          "rasterize_groups_train": ("rasterize_fwd_groups_ids", "rasterize_bwd_groups"),
          "rasterize_layers": ("rasterize_fwd_layers",), "projection_sh": ("projection_sh_fwd", "projection_sh_bwd"),
          "rasterization_fused": ("projection_sh_fwd", "rasterize_fwd_packed"),
          "frame_composite_u8": ("frame_composite_u8", "frame_composite_u8_strided"), "loss": ("loss_fwd", "loss_bwd"),
          "depth_trim": ("depth_trim_fwd", "depth_trim_bwd"), "acc_reg": ("acc_reg_fwd", "acc_reg_bwd"),
          "frame_tail": ("frame_tail_fwd", "frame_tail_bwd"), "cubemap": ("cubemap_fwd", "cubemap_bwd"),
          "lpips_prep": ("lpips_prep_fwd", "lpips_prep_bwd"), "lpips_head": ("lpips_head_fwd", "lpips_head_bwd"),
          "resize": ("resize_fwd", "resize_mask_fwd", "resize_bwd"), "adam": ("adam_step",),
          "densify_stats": ("densify_stats",), "densify": ("densify_plan", "densify_apply"),
          "compose": ("compose_fwd", "compose_bwd")}
COVERED = {fn: case for case, fns in COVERS.items() for fn in fns}          # adapter function -> its sweep case
assert COVERS.keys() == CASES.keys()


@pytest.fixture(scope="module", autouse=True)
def _library():
    from street_crafter_amd import _lib
    _lib.load()
    if _lib.fast() is None:
        pytest.fail("compiled binding layer not loaded")


@pytest.mark.parametrize("name", sorted(CASES))
def test_sweep(name):
    spec = CASES[name]()
    assert tuple(spec["covers"]) == COVERS[name]          # (what the CPU coverage check reads is what the case asserts)
    sweep(spec["body"], spec["covers"], spec.get("atomic", ()), spec.get("judge"))


def test_the_atomic_list_names_only_outputs_that_exist():
    public = set(_public())
    assert {fn for fn, _ in ATOMIC} | {fn for fn, _ in SCRATCH} | {fn for fn, _ in WRITTEN} <= public
    assert set(COVERED) | set(EXEMPT) == public and not set(COVERED) & set(EXEMPT)


def test_a_store_counted_as_guard_is_reported_with_buffer_and_offset():
    """The detector on the GPU path, no kernel touched: after a guarded run of the SH forward the recorded extent of its
    output [257,3] is shrunk by one element, so the kernel's last legitimate store counts as guard -- the allocation is
    physically as large as before, nothing is written out of bounds."""
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    prev = _lib.set_fast_binding(False)
    try:
        for tag in FILLS:
            alloc = GuardedAlloc(*FILLS[tag])
            with guarded_adapter(alloc), torch.no_grad():
                colors = R.spherical_harmonics(3, alloc.guard(_randn((257, 3), 1)), alloc.guard(_randn((257, 16, 3), 2)))
            torch.cuda.synchronize()
            assert alloc.broken_guards() == []
            index = alloc.index_at(colors.data_ptr())
            rec = alloc.records[index]
            assert index == 2 and rec["shape"] == (257, 3) and rec["nbytes"] == 257 * 3 * 4
            rec["nbytes"] -= 4
            assert alloc.broken_guards() == [(2, "after", 257 * 3 * 4 - 4)]
    finally:
        _lib.set_fast_binding(prev)


# ---- entries the operators call outside the adapter: raw pointers into one Arena, exact workspace sizes ------------------
def _direct(buffers, call, outs):
    """buffers: {name: tensor (an input, copied in) | int (bytes of an output or a workspace)}, laid out in one Arena per
    fill; call(arena) -> rc.  Both fills: rc 0, guards intact, inputs unchanged, the `outs` {name: dtype} equal bit for
    bit between the fills.  -> {name: tensor} of the 0xA5 run."""
    res = {}
    for fill in (0xA5, 0x3F):
        sizes = {k: (v.numel() * v.element_size() if torch.is_tensor(v) else int(v)) for k, v in buffers.items()}
        assert all(n > 0 for n in sizes.values()), sizes
        ar = Arena(sizes, DEV, fill=fill)
        for k, v in buffers.items():
            if torch.is_tensor(v):
                ar.view(k).copy_(_bits(v))
        rc = call(ar)
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert ar.broken_guards() == [], (fill, ar.broken_guards(), ar.span)
        for k, v in buffers.items():
            if torch.is_tensor(v) and k not in outs:
                assert torch.equal(ar.view(k), _bits(v)), f"input {k} was written"
        res[fill] = {k: ar.view(k, dt).clone() for k, dt in outs.items()}
    for k in outs:
        assert _same(res[0xA5][k], res[0x3F][k]), f"{k} differs between the fills"
    return res[0xA5]


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def lists():
    """The small frame's tile lists through the operators on the radix route: what the direct cases must reproduce."""
    from street_crafter_amd import rendering as R
    f = _frame(D=4)
    prev = (R.set_isect_mode("radix"), R.set_lazy_isect_ids(False))
    try:
        with torch.no_grad():
            tpg, ids, fids = R.isect_tiles(f["means2d"], f["radii"], f["depths"], 16, f["tw"], f["th"], n_cameras=2)
            ids, fids = torch.as_tensor(ids).clone(), torch.as_tensor(fids).clone()
            offs = R.isect_offset_encode(ids.clone(), 2, f["tw"], f["th"]).clone()
    finally:
        R.set_isect_mode(prev[0]), R.set_lazy_isect_ids(prev[1])
    torch.cuda.synchronize()
    return dict(f, tiles_per_gauss=tpg.clone(), isect_ids=ids, flatten_ids=fids, isect_offsets=offs)


def test_direct_radix_route_count_emit_sort(lists):
    """sc_isect_count + sc_isect_emit + sc_radix_sort_pairs_u64_i32 as isect.py's radix route calls them, with exactly
    sc_isect_workspace_bytes / sc_radix_sort_workspace_bytes of workspace (the operator rounds both up to 256)."""
    from street_crafter_amd import _lib
    lib, f = _lib.load(), lists
    C, N, n = 2, f["N"], f["flatten_ids"].numel()
    tiles = f["tw"] * f["th"]
    end_bit = 32 + int(math.floor(math.log2(tiles))) + 1 + int(math.floor(math.log2(C))) + 1

    def call(ar):
        grid = (C, N, 16, f["tw"], f["th"])
        rc = lib.sc_isect_count(ar.ptr("means2d"), ar.ptr("radii"), *grid, ar.ptr("tpg"), ar.ptr("total"), ar.ptr("ws"),
                                ar.nbytes("ws"), _st())
        rc = rc or lib.sc_isect_emit(ar.ptr("means2d"), ar.ptr("radii"), ar.ptr("depths"), *grid, ar.ptr("tpg"), n, ar.ptr("ids"),
                                     ar.ptr("fids"), ar.ptr("ws"), ar.nbytes("ws"), _st())
        return rc or lib.sc_radix_sort_pairs_u64_i32(ar.ptr("ids"), ar.ptr("fids"), ar.ptr("tmp_k"), ar.ptr("tmp_v"), n, end_bit,
                                                     ar.ptr("sws"), ar.nbytes("sws"), _st())

    got = _direct(dict(means2d=f["means2d"], radii=f["radii"], depths=f["depths"], tpg=4 * C * N, total=8, ids=8 * n, fids=4 * n,
                       tmp_k=8 * n, tmp_v=4 * n, ws=lib.sc_isect_workspace_bytes(C * N), sws=lib.sc_radix_sort_workspace_bytes(n)),
                  call, dict(tpg=torch.int32, total=torch.int64, ids=torch.int64, fids=torch.int32))
    assert int(got["total"]) == n and torch.equal(got["tpg"].view(C, N), f["tiles_per_gauss"])
    assert torch.equal(got["ids"], f["isect_ids"]) and torch.equal(got["fids"], f["flatten_ids"])


def test_direct_isect_offsets_and_ids_rebuild(lists):
    from street_crafter_amd import _lib
    lib, f = _lib.load(), lists
    C, N, n, tw, th = 2, f["N"], f["flatten_ids"].numel(), f["tw"], f["th"]
    got = _direct(dict(ids=f["isect_ids"], offsets=4 * C * tw * th),
                  lambda ar: lib.sc_isect_offsets(ar.ptr("ids"), n, C, tw, th, ar.ptr("offsets"), _st()), dict(offsets=torch.int32))
    assert torch.equal(got["offsets"].view(C, th, tw), f["isect_offsets"])
    got = _direct(dict(fids=f["flatten_ids"], offsets=f["isect_offsets"], depths=f["depths"], ids=8 * n),
                  lambda ar: lib.sc_isect_ids_rebuild(ar.ptr("fids"), ar.ptr("offsets"), ar.ptr("depths"), C, N, tw, th, n,
                                                      ar.ptr("ids"), _st()), dict(ids=torch.int64))
    assert torch.equal(got["ids"], f["isect_ids"])


@pytest.mark.parametrize("C", [1, 3])
def test_direct_camera_centers(C):
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    from street_crafter_amd.scenes import make_camera
    lib = _lib.load()
    vm = torch.stack([make_camera(W0, H0, 40.0, 40.0, yaw=0.3 * c, shift=(0.1 * c, 0.2, -0.3)).viewmat for c in range(C)]).contiguous().to(DEV)
    got = _direct(dict(viewmats=vm, out=12 * C), lambda ar: lib.sc_camera_centers(ar.ptr("viewmats"), C, ar.ptr("out"), _st()),
                  dict(out=torch.float32))
    assert torch.equal(got["out"].view(C, 3), R.camera_centers(vm))


@pytest.mark.parametrize("CN", [1, 65, 257])
def test_direct_records_unpack(CN):
    """sc_records_unpack on the packed records of the fused projection: equal to the separate arrays of the same call."""
    from street_crafter_amd import _ctypes_binding as CB
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    lib = _lib.load()
    sc = _scene(CN, sh_degree=3)
    vm, Ks = _cameras()
    vm, Ks = vm[:1].contiguous(), Ks[:1].contiguous()
    args = (sc.means, sc.quats, sc.scales, sc.opacities[:, 0].contiguous(), sc.sh, vm, Ks, R.camera_centers(vm), 3, W0, H0, 0.3, 0.01,
            100.0, 0.0, True)
    rc, _, _, _, records, _, _, _ = CB.projection_sh_fwd(*args, True, _st())
    rc2, _, _, _, _, conics, opac, cols = CB.projection_sh_fwd(*args, False, _st())
    assert rc == 0 and rc2 == 0
    got = _direct(dict(records=records, conics=12 * CN, opacities=4 * CN, colors=16 * CN),
                  lambda ar: lib.sc_records_unpack(ar.ptr("records"), CN, ar.ptr("conics"), ar.ptr("opacities"), ar.ptr("colors"), _st()),
                  dict(conics=torch.float32, opacities=torch.float32, colors=torch.float32))
    assert _same(got["conics"].view(1, CN, 3), conics) and _same(got["opacities"].view(1, CN), opac)
    assert _same(got["colors"].view(1, CN, 4), cols)


def test_direct_rasterize_fwd_ed(lists):
    """sc_rasterize_fwd_ed as rasterization() calls it: equal to rasterize_to_pixels and the division the reference's
    caller does (the composition that call is documented to equal bit for bit)."""
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    lib, f = _lib.load(), lists
    C, N, n = 2, f["N"], f["flatten_ids"].numel()
    bg = _rand((C, 4), 21)
    px = C * H0 * W0

    def call(ar):
        return lib.sc_rasterize_fwd_ed(ar.ptr("means2d"), ar.ptr("conics"), ar.ptr("colors"), ar.ptr("opacities"), ar.ptr("bg"), None,
                                       C, N, 4, W0, H0, 16, f["tw"], f["th"], ar.ptr("offsets"), ar.ptr("fids"), n, ar.ptr("rc"),
                                       ar.ptr("ra"), None, None, _st())

    got = _direct(dict(means2d=f["means2d"], conics=f["conics"], colors=f["colors"], opacities=f["opacities"], bg=bg,
                       offsets=f["isect_offsets"], fids=f["flatten_ids"], rc=16 * px, ra=4 * px), call,
                  dict(rc=torch.float32, ra=torch.float32))
    prev = R.set_planar_output(False)
    try:
        with torch.no_grad():
            rc, ra = R.rasterize_to_pixels(f["means2d"], f["conics"], f["colors"], f["opacities"], W0, H0, 16, f["isect_offsets"],
                                           f["flatten_ids"], backgrounds=bg)
    finally:
        R.set_planar_output(prev)
    want = torch.cat([rc[..., :-1], rc[..., -1:] / ra.clamp(min=1e-10)], dim=-1)
    assert _same(got["ra"].view(C, H0, W0, 1), ra) and _same(got["rc"].view(C, H0, W0, 4), want)


@pytest.mark.parametrize("planar", [False, True])
def test_direct_point_rasterize_fwd(planar):
    """sc_point_rasterize_fwd at 53x37 on a tile list of 65 points (one more than the wave's batch), interleaved and
    planar outputs with depth: equal to the same entry on ordinary allocations, the way point_render.py calls it (the
    blend itself is judged by tests/test_point_render_exact_gpu.py)."""
    from street_crafter_amd import _lib
    from street_crafter_amd import rendering as R
    lib = _lib.load()
    N, tw, th = 65, 4, 3
    gen = torch.Generator().manual_seed(9)
    uv = 22.0 + 4.0 * torch.rand(N, 2, generator=gen)               # all inside tile (1, 1), radius 3: one list of 65
    z = 1.0 + torch.arange(N, dtype=torch.float32) * 0.25
    rec = torch.cat([uv, torch.full((N, 1), 9.0), z[:, None], torch.rand(N, 3, generator=gen),
                     0.02 + 0.1 * torch.rand(N, 1, generator=gen)], dim=1).contiguous().to(DEV)
    prev = R.set_isect_mode("radix")
    try:
        _, ids, fids = R.isect_tiles(uv[None].contiguous().to(DEV), torch.full((1, N), 3, dtype=torch.int32, device=DEV),
                                     z[None].contiguous().to(DEV), 16, tw, th, n_cameras=1)
        offs, fids = R.isect_offset_encode(ids, 1, tw, th).clone(), torch.as_tensor(fids).clone()
    finally:
        R.set_isect_mode(prev)
    n = fids.numel()
    assert n == N and int(offs.reshape(-1)[5]) == 0 and int(offs.reshape(-1)[6]) == N
    bg = _rand((3,), 4)
    px = H0 * W0
    strides = (1, px, 1) if planar else (4, 1, 4)

    def entry(p_rec, p_offs, p_fids, p_bg, p_img, p_alpha, p_depth):
        return lib.sc_point_rasterize_fwd(p_rec, N, W0, H0, tw, th, p_offs, p_fids, n, 50, p_bg, p_img, strides[0], strides[1],
                                          p_alpha, strides[2], p_depth, _st())

    def call(ar):
        alpha = ar.ptr("alpha") if planar else ar.ptr("img") + 12
        return entry(ar.ptr("records"), ar.ptr("offsets"), ar.ptr("fids"), ar.ptr("bg"), ar.ptr("img"), alpha, ar.ptr("depth"))

    buffers = dict(records=rec, offsets=offs, fids=fids, bg=bg, img=(12 if planar else 16) * px, depth=4 * px)
    outs = dict(img=torch.float32, depth=torch.float32)
    if planar:
        buffers["alpha"], outs["alpha"] = 4 * px, torch.float32
    got = _direct(buffers, call, outs)
    img = torch.empty((3, H0, W0) if planar else (H0, W0, 4), dtype=torch.float32, device=DEV)
    alpha = torch.empty(px, dtype=torch.float32, device=DEV)
    depth = torch.empty(px, dtype=torch.float32, device=DEV)
    assert entry(rec.data_ptr(), offs.data_ptr(), fids.data_ptr(), bg.data_ptr(), img.data_ptr(),
                 alpha.data_ptr() if planar else img.data_ptr() + 12, depth.data_ptr()) == 0
    torch.cuda.synchronize()
    assert _same(got["img"], img.reshape(-1)) and _same(got["depth"], depth)
    assert not planar or _same(got["alpha"], alpha)
    assert float(got["depth"].max()) > 0


@pytest.mark.parametrize("rounding", [0, 1])
@pytest.mark.parametrize("n_pixels", [1, 3, 5, 37 * 53])
def test_direct_frame_composite_u8(n_pixels, rounding):
    """sc_frame_composite_u8 on 3-float pixels and sc_frame_composite_u8_strided on the [..., :3] view of a 4-channel render:
    the tails of the 4-pixel epilogue.  Equal to what dist.to_uint8_frame returns for the same pixels."""
    from street_crafter_amd import _lib
    lib = _lib.load()
    fg, sky = _rand((n_pixels, 4), n_pixels, -0.2, 1.2), _rand((n_pixels, 4), n_pixels + 1, -0.2, 1.2)
    acc = _rand((n_pixels,), n_pixels + 2)
    from street_crafter_amd import dist
    want = dist.to_uint8_frame(fg[None].permute(2, 0, 1)[:3], acc=acc.view(1, n_pixels, 1), sky_rgb_chw=sky[None].permute(2, 0, 1)[:3],
                               rounding="save_image" if rounding else "video")          # the operator on a 1 x n frame
    fg3, sky3 = fg[:, :3].contiguous(), sky[:, :3].contiguous()
    got = _direct(dict(fg=fg3, sky=sky3, acc=acc, out=3 * n_pixels),
                  lambda ar: lib.sc_frame_composite_u8(ar.ptr("fg"), 3, ar.ptr("acc"), ar.ptr("sky"), 3, n_pixels, rounding,
                                                       ar.ptr("out"), _st()), dict(out=torch.uint8))
    plain = torch.empty(n_pixels, 3, dtype=torch.uint8, device=DEV)
    assert lib.sc_frame_composite_u8(fg3.data_ptr(), 3, acc.data_ptr(), sky3.data_ptr(), 3, n_pixels, rounding, plain.data_ptr(), _st()) == 0
    assert torch.equal(got["out"].view(n_pixels, 3), plain)
    # the [..., :3] view of 4-channel renders: the last pixel's fourth float is the last float of the buffer
    strided = _direct(dict(fg=fg, sky=sky, acc=acc, out=3 * n_pixels),
                      lambda ar: lib.sc_frame_composite_u8_strided(ar.ptr("fg"), 4, 1, ar.ptr("acc"), ar.ptr("sky"), 4, 1, n_pixels,
                                                                   rounding, ar.ptr("out"), _st()), dict(out=torch.uint8))
    assert torch.equal(strided["out"], got["out"])
    assert torch.equal(got["out"].view(1, n_pixels, 3), want)
