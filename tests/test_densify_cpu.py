"""No-GPU checks of the fused densify-and-prune (street_crafter_amd/densify.py, csrc/densify.hip), and the yardstick the
GPU tests judge it by.

`restate` is a torch restatement of the reference's sequence, in the reference's order and with its intermediate
populations: densify_and_clone (gaussian_model.py:493-519: select, `cat`), densify_and_split (gaussian_model.py:452-491:
select on the gradients padded with zeros, `cat` of 2 children per selected row, mask out the parents), then the prune
tests of gaussian_model_bkgd.py:119-148 / gaussian_model_actor.py:222-263 on the population after the split and
prune_points (gaussian_model.py:416-431: mask).  The optimizer moments travel as cat_optimizer / prune_optimizer move them
(gaussian_model.py:363-408).  The only change is that the normal samples are injected: torch.normal(0, std) is
randn * std, and the randn is `split_noise[k, row]` / `box_noise[slot, row, m]`, indexed by ORIGINAL row.  It runs in any
dtype on any device: in float64 it is the judge of the children's values, in float32 it is what the reference computes.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

U = 2.0 ** -24
SPLIT_DIV = float(np.float32(0.8 * 2))          # gaussian_model.py:473 with N = 2, as the fp32 tensor division sees it
COUNTERS = ("points_total", "points_clone", "points_split", "points_below_min_opacity", "points_big_ws", "points_pruned")


# ---- the restatement ------------------------------------------------------------------------------------------------------
def quat_matrix(r):
    """general_utils.py:125-146 (w-x-y-z, normalised first)."""
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros((q.shape[0], 3, 3), dtype=r.dtype, device=r.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def restate(tensors, moments, acc, denom, max_radii, cfg, split_noise, box_noise=None, dtype=torch.float32):
    """tensors: name -> [n, ...] with the keys xyz, scaling, rotation, opacity and any passengers; moments: name ->
    (exp_avg, exp_avg_sq) or None.  cfg: max_grad, use_abs, extent, percent_dense, min_opacity, prune_big_points,
    percent_big_ws, max_screen_size, sphere, box.  -> namespace(tensors, moments, src_row, slot, counters, n_out)."""
    c = lambda t: t.detach().to(dtype).clone()                                           # noqa: E731
    T = {k: c(v) for k, v in tensors.items()}
    M = {k: (None if v is None else (c(v[0]), c(v[1]))) for k, v in moments.items()}
    acc, denom, max_radii, split_noise = c(acc), c(denom).reshape(-1, 1), c(max_radii), c(split_noise)
    dev = acc.device
    n0 = T["xyz"].shape[0]
    src = torch.arange(n0, device=dev)
    slot = torch.zeros(n0, dtype=torch.long, device=dev)
    counters = {"points_total": n0, "points_below_min_opacity": 0, "points_big_ws": 0}

    def cat(new, new_src, new_slot):                          # densification_postfix + cat_optimizer
        nonlocal src, slot, max_radii
        for k in T:
            if M[k] is not None:
                M[k] = tuple(torch.cat((m, torch.zeros_like(new[k])), dim=0) for m in M[k])
            T[k] = torch.cat((T[k], new[k]), dim=0)
        src, slot = torch.cat((src, new_src)), torch.cat((slot, new_slot))
        max_radii = torch.cat((max_radii, torch.zeros(new_src.shape[0], dtype=dtype, device=dev)))

    def mask(keep):                                           # prune_points + prune_optimizer
        nonlocal src, slot, max_radii
        for k in T:
            if M[k] is not None:
                M[k] = tuple(m[keep] for m in M[k])
            T[k] = T[k][keep]
        src, slot, max_radii = src[keep], slot[keep], max_radii[keep]

    col = 1 if cfg["use_abs"] else 0
    grads = acc[:, col:col + 1] / denom
    grads[grads.isnan()] = 0.0
    dense = cfg["percent_dense"] * cfg["extent"]
    # clone
    sel = (torch.norm(grads, dim=-1) >= cfg["max_grad"]) & (torch.exp(T["scaling"]).max(dim=1).values <= dense)
    counters["points_clone"] = int(sel.sum())
    cat({k: v[sel] for k, v in T.items()}, src[sel], torch.ones(int(sel.sum()), dtype=torch.long, device=dev))
    # split
    padded = torch.zeros(T["xyz"].shape[0], dtype=dtype, device=dev)
    padded[:n0] = grads.squeeze(-1)
    sel = (padded >= cfg["max_grad"]) & (torch.exp(T["scaling"]).max(dim=1).values > dense)
    m = int(sel.sum())
    counters["points_split"] = m
    stds = torch.exp(T["scaling"][sel]).repeat(2, 1)
    samples = split_noise[:, src[sel]].reshape(2 * m, 3) * stds
    rots = quat_matrix(T["rotation"][sel]).repeat(2, 1, 1)
    new = {k: v[sel].repeat(2, *([1] * (v.dim() - 1))) for k, v in T.items()}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + T["xyz"][sel].repeat(2, 1)
    new["scaling"] = torch.log(torch.exp(T["scaling"][sel]).repeat(2, 1) / SPLIT_DIV)
    new_slot = torch.cat((torch.full((m,), 2, device=dev), torch.full((m,), 3, device=dev)))
    parents = torch.cat((sel, torch.zeros(2 * m, dtype=torch.bool, device=dev)))
    cat(new, src[sel].repeat(2), new_slot)
    mask(~parents)
    # prune
    prune = (torch.sigmoid(T["opacity"]) < cfg["min_opacity"]).reshape(-1)
    counters["points_below_min_opacity"] = int(prune.sum())
    if cfg["prune_big_points"]:
        s = torch.exp(T["scaling"])
        big = s.max(dim=1).values > cfg["extent"] * cfg["percent_big_ws"]
        if cfg.get("sphere") is not None:
            centre = torch.tensor(cfg["sphere"][0], dtype=dtype, device=dev)
            dists = torch.linalg.norm(T["xyz"] - centre, dim=1)
            big[dists > cfg["sphere"][1]] = False
        counters["points_big_ws"] = int(big.sum())
        prune = prune | big
        if cfg.get("box") is not None:
            lo = torch.tensor(cfg["box"][0], dtype=dtype, device=dev)
            hi = torch.tensor(cfg["box"][1], dtype=dtype, device=dev)
            smp = c(box_noise)[slot, src] * s[:, None, :]                                  # [N,2,3]
            rots = quat_matrix(torch.nn.functional.normalize(T["rotation"]))[:, None]
            pts = torch.matmul(rots, smp.unsqueeze(-1)).squeeze(-1) + T["xyz"][:, None, :]
            inside = (pts >= lo).flatten(1).all(dim=-1) & (pts <= hi).flatten(1).all(dim=-1)
            prune = prune | ~inside
    if cfg.get("max_screen_size"):
        prune = prune | (max_radii > cfg["max_screen_size"])
    counters["points_pruned"] = int(prune.sum())
    mask(~prune)
    return SimpleNamespace(tensors=T, moments=M, src_row=src, slot=slot, counters=counters, n_out=int(src.shape[0]))


CFG = dict(max_grad=1.0, use_abs=False, extent=10.0, percent_dense=0.01, min_opacity=0.1, prune_big_points=True,
           percent_big_ws=0.1, max_screen_size=20.0, sphere=None, box=None)


def hand_case():
    """Eight rows, identity rotations; thresholds: clone / split at max s = 0.1, big above 1.0, opacity below 0.1,
    screen radius above 20.
      0 cold (0 / 0 -> NaN -> 0)                 stays
      1 hot, s 0.05                              stays + clone
      2 hot, s 0.5                               two children, s' = 0.3125
      3 cold, sigmoid(-5) < 0.1                  pruned (opacity)
      4 cold, s 2                                pruned (big)
      5 hot, s 1.8                               two children with s' = 1.125: both pruned (big)
      6 cold, radius 30                          pruned (screen)
      7 hot, s 0.05, radius 30                   pruned (screen), its clone (radius 0) stays"""
    n = 8
    f = lambda v: torch.tensor(v, dtype=torch.float32)                                   # noqa: E731
    s = f([0.05, 0.05, 0.5, 0.05, 2.0, 1.8, 0.05, 0.05])
    tensors = {
        "xyz": torch.arange(n, dtype=torch.float32)[:, None] + f([[1.0, 2.0, 3.0]]),
        "scaling": torch.log(s)[:, None] * torch.ones(1, 3),
        "rotation": f([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1),
        "opacity": f([3.0, 3.0, 3.0, -5.0, 3.0, 3.0, 3.0, 3.0])[:, None],
        "f_dc": torch.arange(n * 3, dtype=torch.float32).reshape(n, 1, 3),
    }
    moments = {k: (torch.full_like(v, 0.5) + torch.arange(n).reshape(-1, *([1] * (v.dim() - 1))),
                   torch.full_like(v, 0.25)) for k, v in tensors.items()}
    moments["f_dc"] = None
    acc = f([[0.0, 9.0], [4.0, 0.0], [6.0, 0.0], [0.5, 9.0], [0.5, 9.0], [3.0, 0.0], [0.5, 9.0], [8.0, 0.0]])
    denom = f([0.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0, 4.0])[:, None]
    max_radii = f([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 30.0, 30.0])
    noise = torch.zeros(2, n, 3)
    noise[0, 2] = f([1.0, 0.0, -1.0])
    noise[1, 2] = f([0.0, 2.0, 0.0])
    return tensors, moments, acc, denom, max_radii, noise


def test_restatement_on_the_hand_worked_case():
    tensors, moments, acc, denom, max_radii, noise = hand_case()
    for dtype in (torch.float32, torch.float64):
        r = restate(tensors, moments, acc, denom, max_radii, CFG, noise, dtype=dtype)
        assert r.src_row.tolist() == [0, 1, 1, 7, 2, 2] and r.slot.tolist() == [0, 0, 1, 1, 2, 3] and r.n_out == 6
        assert r.counters == dict(points_total=8, points_clone=2, points_split=2, points_below_min_opacity=1,
                                  points_big_ws=3, points_pruned=6)
        x2 = tensors["xyz"][2].to(dtype)
        assert torch.allclose(r.tensors["xyz"][4], x2 + torch.tensor([0.5, 0.0, -0.5], dtype=dtype), rtol=1e-6, atol=0)
        assert torch.allclose(r.tensors["xyz"][5], x2 + torch.tensor([0.0, 1.0, 0.0], dtype=dtype), rtol=1e-6, atol=0)
        assert torch.allclose(r.tensors["scaling"][4:], torch.full((2, 3), float(np.log(0.5 / 1.6)), dtype=dtype), rtol=1e-6)
        assert torch.equal(r.tensors["f_dc"], tensors["f_dc"].to(dtype)[r.src_row])
        assert torch.equal(r.tensors["xyz"][:4], tensors["xyz"].to(dtype)[r.src_row[:4]])
        m, v = r.moments["xyz"]
        assert torch.equal(m[:2], moments["xyz"][0].to(dtype)[:2]) and not m[2:].any() and not v[2:].any()
        assert r.moments["f_dc"] is None
    # column 1 of the statistics: rows 0 (9 / 0 = inf), 3, 4, 6 are hot instead, 1, 2, 5, 7 cold: 0, 3, 6 clone, 4 splits
    r = restate(tensors, moments, acc, denom, max_radii, dict(CFG, use_abs=True), noise)
    assert r.counters["points_clone"] == 3 and r.counters["points_split"] == 1
    r = restate(tensors, moments, acc, denom, max_radii, dict(CFG, prune_big_points=False, max_screen_size=None), noise)
    assert r.counters["points_pruned"] == 1 and r.n_out == 8 + 2 + 2 - 1


# ---- refusals: before anything is modified ------------------------------------------------------------------------------------
def _cpu_job(D, n=6, **over):
    gen = torch.Generator().manual_seed(3)
    shapes = {"xyz": (n, 3), "scaling": (n, 3), "rotation": (n, 4), "opacity": (n, 1), "f_dc": (n, 1, 3),
              "f_rest": (n, 15, 3), "semantic": (n, 0)}
    dtype = over.pop("param_dtype", torch.float32)
    params = {k: torch.nn.Parameter(torch.randn(s, generator=gen).to(dtype)) for k, s in shapes.items()}
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    for p in params.values():
        opt.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    kw = dict(optimizer=opt, xyz_gradient_accum=torch.zeros(n, 2), denom=torch.zeros(n, 1), max_radii2D=torch.zeros(n),
              max_grad=0.0002, extent=10.0, min_opacity=0.005)
    kw.update(over)
    return D.DensifyJob(**kw), opt, params


def _untouched(opt, params):
    for group, (name, p) in zip(opt.param_groups, params.items()):
        assert group["params"][0] is p and group["name"] == name
        assert set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(opt.state[p]["step"]) == 3.0


def test_refusals_happen_before_anything_is_modified():
    from street_crafter_amd import densify as D
    n = 6
    cases = [
        (RuntimeError, "HIP device", {}),                                              # CPU tensors
        (ValueError, "float32", {"param_dtype": torch.float64}),
        (ValueError, "float32", {"denom": torch.zeros(n, 1, dtype=torch.float16)}),
        (ValueError, "contiguous", {"xyz_gradient_accum": torch.zeros(2, n).t()}),
        (ValueError, "shape", {"max_radii2D": torch.zeros(n + 1)}),
        (ValueError, "max_grad", {"max_grad": 0.0}),
        (ValueError, "max_grad", {"max_grad": -1.0}),
        (ValueError, "max_grad", {"max_grad": float("nan")}),
        (ValueError, "split_noise", {"split_noise": torch.zeros(2, n, 4)}),
        (ValueError, "split_noise", {"split_noise": torch.zeros(n, 2, 3)}),
        (ValueError, "box_noise", {"box_noise": torch.zeros(4, n, 3), "box": ([-1.0] * 3, [1.0] * 3)}),
        (ValueError, "not both", {"sphere": ([0.0] * 3, 1.0), "box": ([-1.0] * 3, [1.0] * 3)}),
        (ValueError, "no group named", {"passengers": ("f_dc", "nope")}),
        (ValueError, "three numbers", {"sphere": ([0.0] * 2, 1.0)}),
    ]
    for exc, match, over in cases:
        job, opt, params = _cpu_job(D, n, **over)
        with pytest.raises(exc, match=match):
            D.densify_and_prune_many([job])
        _untouched(opt, params)
    # a state whose shape does not match its parameter; and a good first job does not get modified by a bad second one
    job, opt, params = _cpu_job(D, n)
    opt.state[params["xyz"]]["exp_avg"] = torch.zeros(n + 1, 3)
    with pytest.raises(ValueError, match="exp_avg"):
        D.densify_and_prune_many([job])
    _untouched(opt, params)
    good, opt, params = _cpu_job(D, n)
    bad, _, _ = _cpu_job(D, n, max_grad=0.0)
    with pytest.raises(ValueError, match="job 1"):
        D.densify_and_prune_many([good, bad])
    _untouched(opt, params)
    with pytest.raises(TypeError, match="optimizer"):
        D.densify_and_prune_many([D.DensifyJob(**dict(job.__dict__, optimizer=torch.optim.SGD([torch.zeros(1)], lr=1.0)))])


def test_no_jobs_is_no_call():
    from street_crafter_amd import densify as D
    assert D.densify_and_prune_many([]) == []


# ---- the C entries: refused before any HIP call ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import build
    build.build()
    from street_crafter_amd import _lib
    return _lib.load()


FAKE = 0x1000          # a non-null device address that no refused call may look at


def _job(_lib, n=1000, **over):
    j = _lib.DensifyJob()
    j.n = n
    for name in ("xyz", "scaling", "rotation", "opacity", "grad_accum", "denom", "max_radii", "split_noise", "src_row",
                 "slot", "child_xyz", "child_scaling", "counters"):
        setattr(j, name, FAKE)
    j.max_grad, j.dense_size, j.min_opacity, j.big_size = 0.0002, 0.1, 0.005, 1.0
    for k, v in over.items():
        setattr(j, k, v)
    return j


def test_plan_entry_validates_without_a_gpu(lib):
    from street_crafter_amd import _lib
    B = lib.sc_densify_scan_block()
    assert B >= 64 and B & (B - 1) == 0 and lib.sc_densify_max_jobs() >= 1 and lib.sc_densify_max_groups() >= 1
    one = lambda j: (_lib.DensifyJob * 1)(j)                                              # noqa: E731
    assert lib.sc_densify_plan(None, 0, None, 0, None) == 0                                 # no jobs: no launch
    assert lib.sc_densify_plan(None, -1, None, 0, None) == -1
    assert lib.sc_densify_plan(None, 1, None, 0, None) == -1
    bad = [dict(n=-1), dict(n=1 << 29), dict(xyz=None), dict(scaling=None), dict(rotation=None), dict(opacity=None),
           dict(grad_accum=None), dict(denom=None), dict(max_radii=None), dict(split_noise=None), dict(src_row=None),
           dict(slot=None), dict(child_xyz=None), dict(child_scaling=None), dict(counters=None), dict(grad_col=2),
           dict(grad_col=-1), dict(region=3), dict(region=-1), dict(max_grad=0.0), dict(max_grad=-1.0),
           dict(max_grad=float("nan")), dict(prune_big=1, region=2)]                        # a box without its noise
    for over in bad:
        assert lib.sc_densify_plan(one(_job(_lib, **over)), 1, FAKE, 1 << 20, None) == -1, over
    assert lib.sc_densify_plan(one(_job(_lib, n=0, counters=None)), 1, None, 0, None) == -1   # counters even when empty
    # the workspace: the keep masks (n bytes) and four counts per block, each rounded up to 16 bytes
    n = 2 * B + 1
    need = lib.sc_densify_plan_workspace_bytes(one(_job(_lib, n=n)), 1)
    assert need == (n + 15) // 16 * 16 + 4 * 3 * 4
    two = (_lib.DensifyJob * 2)(_job(_lib, n=n), _job(_lib, n=0))
    assert lib.sc_densify_plan_workspace_bytes(two, 2) == need
    assert lib.sc_densify_plan_workspace_bytes(one(_job(_lib, n=-1)), 1) == 0
    assert lib.sc_densify_plan_workspace_bytes(None, 1) == 0
    assert lib.sc_densify_plan(one(_job(_lib, n=n)), 1, FAKE, need - 1, None) == -2
    assert lib.sc_densify_plan(one(_job(_lib, n=n)), 1, None, need, None) == -2
    assert lib.sc_densify_plan(one(_job(_lib, n=n)), 1, FAKE + 4, need, None) == -1           # not 16-byte aligned
    # every job empty: nothing to launch, no workspace needed
    assert lib.sc_densify_plan(one(_job(_lib, n=0)), 1, None, 0, None) == 0


def _group(_lib, **over):
    g = _lib.DensifyGroup()
    for name in ("src_param", "dst_param", "src_row", "slot"):
        setattr(g, name, FAKE)
    g.n, g.n_out, g.width = 10, 12, 3
    for k, v in over.items():
        setattr(g, k, v)
    return g


def test_apply_entry_validates_without_a_gpu(lib):
    from street_crafter_amd import _lib
    one = lambda g: (_lib.DensifyGroup * 1)(g)                                            # noqa: E731
    assert lib.sc_densify_apply(None, 0, None) == 0
    assert lib.sc_densify_apply(None, -1, None) == -1
    assert lib.sc_densify_apply(None, 1, None) == -1
    bad = [dict(n=-1), dict(n_out=-1), dict(width=-1), dict(n_out=21), dict(n=0, n_out=1), dict(src_param=None),
           dict(dst_param=None), dict(src_row=None), dict(slot=None), dict(src_exp_avg=FAKE),
           dict(src_exp_avg=FAKE, src_exp_avg_sq=FAKE, dst_exp_avg=FAKE), dict(dst_exp_avg_sq=FAKE)]
    for over in bad:
        assert lib.sc_densify_apply(one(_group(_lib, **over)), 1, None) == -1, over
    # groups that move nothing are legal and launch nothing: no rows out, no rows at all, width 0
    for over in (dict(n_out=0), dict(n=0, n_out=0), dict(width=0),
                 dict(width=0, src_param=None, dst_param=None, src_row=None, slot=None)):
        assert lib.sc_densify_apply(one(_group(_lib, **over)), 1, None) == 0, over


def test_structures_match_the_header():
    """sizeof / field order of the ctypes structures against the typedefs of include/street_crafter_amd.h."""
    import os
    import re
    from street_crafter_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "street_crafter_amd.h")).read()
    for cname, struct in (("sc_densify_job", _lib.DensifyJob), ("sc_densify_group", _lib.DensifyGroup)):
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", src).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[\d+\]", "", part.split()[-1].lstrip("*")) for part in decl.split(",")]
        assert names == [f[0] for f in struct._fields_], cname
    assert ctypes.sizeof(_lib.DensifyJob) == 176 and ctypes.sizeof(_lib.DensifyGroup) == 96
