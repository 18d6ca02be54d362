"""GPU checks of the fused densification statistics (csrc/optim.hip sc_densify_stats through
densify_stats.accumulate_fused) against the torch mirror DensificationStats on the same inputs and GPU.

denom and max_radii2D: bit-identical to the mirror.  xyz_gradient_accum: every entry within 4u (acc_before + norm64) of
the float64 evaluation of the mirror's expression (tests/test_optim_cpu.py stats_f64, where the mirror itself is held to
the same bound).  Rows outside every segment and invisible rows: bit-identical to the pre-filled pattern.
"""
import pytest
import torch

from test_optim_cpu import (STATS_H, STATS_NS, STATS_W, covered, mirror_run, stats_buffers, stats_case, stats_f64,
                            stats_segments)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def D():
    from street_crafter_amd import _lib, densify_stats
    _lib.load()
    return densify_stats


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _fused(D, segments, buffers, vp, radii, vis):
    """accumulate_fused on clones of the buffers, the segments' accumulators being slices of them."""
    acc, den, mr = (b.clone() for b in buffers)
    D.accumulate_fused([(s, e, acc[s:e], den[s:e], mr[s:e]) for s, e in segments], radii, vis, vp, STATS_W, STATS_H)
    return acc, den, mr


def _check(D, N, kind, seed, what, buffers=None, **case):
    segments = stats_segments(N, kind)
    vp, radii, vis = stats_case(N, seed, device=DEV, **case)
    if buffers is None:
        buffers = stats_buffers(N, seed, case.get("radii_float", False), device=DEV)
    got = _fused(D, segments, buffers, vp, radii, vis)
    want = mirror_run(segments, buffers, vp, radii, vis)
    live = (covered(N, segments) & vis.cpu())
    for g, b in zip(got, buffers):                                   # untouched rows: not written at all
        assert torch.equal(_bits(g)[~live], _bits(b)[~live]), what
    assert torch.equal(_bits(got[1]), _bits(want[1])), what          # denom
    assert torch.equal(_bits(got[2]), _bits(want[2])), what          # max_radii2D
    acc64, bound = stats_f64(vp, vis, buffers[0])
    err = (got[0].cpu().double() - acc64).abs()
    assert bool((err[live] <= bound[live]).all()), (what, float((err[live] / bound[live]).max()))
    if not case.get("absgrad", True):
        assert torch.equal(_bits(got[0])[:, 1], _bits(buffers[0])[:, 1]), what       # column 1 += 0
    return got


@pytest.mark.parametrize("kind", ["none", "all", "five"])
@pytest.mark.parametrize("N", STATS_NS)
def test_sizes_and_segment_layouts(D, N, kind):
    _check(D, N, kind, seed=N % 7, what=(N, kind))


@pytest.mark.parametrize("absgrad", [True, False], ids=["absgrad", "grad-only"])
@pytest.mark.parametrize("batched", [False, True], ids=["N2", "1N2"])
@pytest.mark.parametrize("radii_float", [False, True], ids=["int32", "fp32"])
def test_input_forms(D, absgrad, batched, radii_float):
    for N in (65, 4099):
        _check(D, N, "five", seed=3, what=(N, absgrad, batched, radii_float), absgrad=absgrad, batched=batched,
               radii_float=radii_float)


@pytest.mark.parametrize("visible", ["all", "none"])
def test_all_and_none_visible(D, visible):
    for kind in ("all", "five"):
        _check(D, 4099, kind, seed=5, what=(visible, kind), visible=visible)


def test_three_accumulations_and_routes_agree(D):
    """Three renders accumulated into the same buffers, each judged from the fp32 state before it; the ctypes route and
    the class method give the same bits as the compiled binding; more segments than one launch takes."""
    from street_crafter_amd import _lib
    N = 4099
    buffers = stats_buffers(N, 8, device=DEV)
    for seed in (1, 2, 3):
        buffers = _check(D, N, "five", seed=seed, what=seed, buffers=buffers)
    segments = [(k * 20, k * 20 + 19) for k in range(150)]           # 150 segments: three launches inside the call
    vp, radii, vis = stats_case(N, 4, device=DEV)
    start = stats_buffers(N, 9, device=DEV)
    fast = _fused(D, segments, start, vp, radii, vis)
    want = mirror_run(segments, start, vp, radii, vis)
    assert torch.equal(_bits(fast[1]), _bits(want[1])) and torch.equal(_bits(fast[2]), _bits(want[2]))
    prev = _lib.set_fast_binding(False)
    try:
        assert _lib.fast() is None
        slow = _fused(D, segments, start, vp, radii, vis)
    finally:
        _lib.set_fast_binding(prev)
    st = D.DensificationStats({f"m{k}": se for k, se in enumerate(segments)}, device=DEV)
    for k, (s, e) in enumerate(segments):
        st.xyz_gradient_accum[f"m{k}"], st.denom[f"m{k}"], st.max_radii2D[f"m{k}"] = (b[s:e].clone() for b in start)
    st.accumulate_from_render_fused({"radii": radii, "visibility_filter": vis, "viewspace_points": vp}, STATS_W, STATS_H)
    for k, (s, e) in enumerate(segments):
        assert torch.equal(_bits(st.xyz_gradient_accum[f"m{k}"]), _bits(fast[0][s:e]))
        assert torch.equal(_bits(st.denom[f"m{k}"]), _bits(fast[1][s:e]))
    for a, b in zip(fast, slow):
        assert torch.equal(_bits(a), _bits(b))


def test_argument_checks_on_device_tensors(D):
    vp, radii, vis = stats_case(16, 0, device=DEV)
    acc, den, mr = stats_buffers(16, 0, device=DEV)
    keep = acc.clone()
    with pytest.raises(ValueError):
        D.accumulate_fused([(0, 17, acc, den, mr)], radii, vis, vp, 64, 64)                  # end > N
    with pytest.raises(ValueError):
        D.accumulate_fused([(0, 8, acc, den, mr)], radii, vis, vp, 64, 64)                   # accumulators of 16 rows
    with pytest.raises(ValueError):
        D.accumulate_fused([(0, 16, acc, den, mr)], radii.long(), vis, vp, 64, 64)           # int64 radii
    with pytest.raises(ValueError):
        D.accumulate_fused([(0, 16, acc, den, mr)], radii, vis.float(), vp, 64, 64)          # a float mask
    with pytest.raises(ValueError):
        D.accumulate_fused([(0, 16, acc.double(), den, mr)], radii, vis, vp, 64, 64)
    with pytest.raises(ValueError):
        D.accumulate_fused([(0, 16, acc, den, mr)], radii[:8], vis, vp, 64, 64)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.accumulate_fused([(0, 16, acc, den.cpu(), mr)], radii, vis, vp, 64, 64)
    assert torch.equal(acc, keep)


def test_no_host_wait(D):
    """accumulate_fused under set_sync_debug_mode("error") raises nothing; the torch mirror (boolean-mask indexing: a
    nonzero) raises under the same mode, so the check is active."""
    N = 4099
    segments = stats_segments(N, "five")
    vp, radii, vis = stats_case(N, 6, device=DEV)
    buffers = stats_buffers(N, 6, device=DEV)
    _fused(D, segments, buffers, vp, radii, vis)                  # warm-up: library and binding loaded
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _fused(D, segments, buffers, vp, radii, vis)
        with pytest.raises(RuntimeError):
            mirror_run(segments, buffers, vp, radii, vis)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(got[0]).all()
