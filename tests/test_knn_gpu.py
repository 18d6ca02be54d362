"""simple_knn._C.distCUDA2 (csrc/knn.hip) where its hierarchy changes shape, bit for bit.

knn_mean_dist_kernel walks four fixed levels of 32 / 1024 / 32 768 / 1 048 576 points.  The cases here sit on and one
past every level boundary (one past is where a one-point leaf and one-child parents appear at every level) and, once,
beyond 2 * 2^20, where the top level has more than one box.  The brute-force oracle is O(n^2), so from 63 points up the
expectation is the closed form of tests/knn_ref.py: clusters on a lattice, exact at any n, certified on the CPU by
test_knn_ref_cpu.py (it equals the oracle where the oracle is affordable; the large cloud has hundreds of clusters
whose members lie in different boxes of every level, and three simulated broken walks fail on it).

Then the inputs a LiDAR sweep brings: degenerate Morton orders, NaN and infinite rows, squares that overflow float32
(oracle/knn_oracle.py: a distance that is not < FLT_MAX is never a neighbour), the tensor forms distCUDA2 accepts, and
the workspace contract of the C entry read back through guard zones.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as ref  # noqa: E402
from guard_arena import Arena  # noqa: E402
from oracle import knn_oracle as KO  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _knn(pts):
    from simple_knn._C import distCUDA2
    return distCUDA2(torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(DEV)).cpu().numpy()


def _same_bits(got, want):
    np.testing.assert_array_equal(_bits(got), _bits(want))


# ---- level boundaries ---------------------------------------------------------------------------------------------------
# n -> points per cluster (31..33 are one cluster); the remainder joins the last cluster, so none has fewer than 4
BOUNDARY = {31: 31, 32: 32, 33: 33, 63: 8, 64: 8, 65: 8, 1023: 11, 1024: 11, 1025: 11, 32767: 37, 32768: 37, 32769: 37}


@pytest.mark.parametrize("n", sorted(BOUNDARY))
def test_level_boundary_bit_exact(n):
    pts, cl = ref.clustered(n, BOUNDARY[n], seed=n)
    _same_bits(_knn(pts), ref.ref_clustered(pts, cl))


def test_three_top_level_boxes_bit_exact():
    """2 * 2^20 + 33 points: lv.count[3] = 3, the last top-level box holding one full leaf and a one-point leaf."""
    pts, cl = ref.clustered(**ref.LARGE)
    _same_bits(_knn(pts), ref.ref_clustered(pts, cl))


# ---- small clouds against the brute-force oracle ----------------------------------------------------------------------
def _cloud(kind, n, seed=0):
    rng = np.random.default_rng([seed, n])
    if kind == "uniform":
        return rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    return (rng.normal(size=(n, 3)) * np.array([5.0, 0.2, 3e-3])).astype(np.float32)      # anisotropic


@pytest.mark.parametrize("kind", ["uniform", "anisotropic"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 33, 1025, 4097])
def test_small_cloud_bit_exact(kind, n):
    pts = _cloud(kind, n)
    got = _knn(pts)
    _same_bits(got, KO.dist_cuda2(pts))
    if n < 4:
        assert (got > 1e38).all()           # a FLT_MAX term per missing neighbour


def test_one_past_two_pow_20_uniform_vs_ckdtree():
    """2^20 + 1 uniform points: two top-level boxes, the second a single point.  cKDTree in float64, the project's bar."""
    pts = np.random.default_rng(11).uniform(-30.0, 30.0, size=((1 << 20) + 1, 3)).astype(np.float32)
    got = _knn(pts)
    want = ref.ckdtree_mean_dist2(pts, workers=16)
    print("worst relative error vs cKDTree:", float(np.max(np.abs(got - want) / want)))
    np.testing.assert_allclose(got, want, rtol=3e-5, atol=1e-9)


# ---- degenerate Morton orders -------------------------------------------------------------------------------------------
def _degenerate(kind):
    rng = np.random.default_rng(7)
    if kind == "identical":                 # one key, every distance 0
        return np.tile(np.array([[0.25, -3.0, 7.5]], dtype=np.float32), (4097, 1))
    if kind == "one_axis":                  # two extents are zero
        p = np.zeros((4097, 3), dtype=np.float32)
        p[:, 1] = rng.normal(size=4097)
        return p
    blob = rng.uniform(0.0, 1.0, size=(4096, 3)).astype(np.float32)      # blob_and_outlier: all keys but one are 0,
    return np.concatenate([blob, np.full((1, 3), 1e6, dtype=np.float32)])    # so the curve is the index order


@pytest.mark.parametrize("kind", ["identical", "one_axis", "blob_and_outlier"])
def test_degenerate_morton_order_bit_exact(kind):
    pts = _degenerate(kind)
    if kind == "blob_and_outlier":
        np.testing.assert_array_equal(ref.curve_pos(pts), np.arange(4097))
    _same_bits(_knn(pts), KO.dist_cuda2(pts))


# ---- rows and distances that are not finite ---------------------------------------------------------------------------
def test_non_finite_rows_are_invisible_and_return_inf():
    """NaN, +inf and -inf rows: every distance from or to such a row is NaN or +inf, neither is < FLT_MAX, so the row
    has no neighbour (((FLT_MAX + FLT_MAX) + FLT_MAX) / 3 = +inf) and is nobody's neighbour: the finite rows come out
    as if the cloud had never held it."""
    fin = np.random.default_rng(3).normal(size=(2000, 3)).astype(np.float32) * np.float32(4.0)
    bad = np.array([[np.nan, 1.0, -2.0], [0.5, np.inf, 0.0], [-np.inf, 0.0, 3.0]], dtype=np.float32)
    mixed = np.concatenate([bad[:1], fin[:777], bad[1:2], fin[777:], bad[2:]])
    is_bad = ~np.isfinite(mixed).all(axis=1)
    assert is_bad.sum() == 3 and is_bad[0] and is_bad[778] and is_bad[-1]
    clean = _knn(fin)
    _same_bits(clean, KO.dist_cuda2(fin))
    got = _knn(mixed)
    _same_bits(got[~is_bad], clean)
    assert (got[is_bad] == np.inf).all(), got[is_bad]
    _same_bits(got, KO.dist_cuda2(mixed))
    # NaN rows alone: the bounding box ignores them (fminf / fmaxf) and the curve keeps its shape
    nan_only = np.concatenate([fin[:1000], bad[:1], fin[1000:], bad[:1]])
    got = _knn(nan_only)
    _same_bits(got[[i for i in range(2002) if i not in (1000, 2001)]], clean)
    assert (got[[1000, 2001]] == np.inf).all()


def test_overflowing_distances_bit_exact():
    """Groups of 1..5 points at +-3e19 on the axes: d^2 between groups is +inf in float32 and never a neighbour, so a
    group of three keeps one FLT_MAX term (a finite result near FLT_MAX / 3) and smaller groups overflow to +inf."""
    a, step = 3e19, 2.0 ** 44                        # float32 spacing at 3e19 is 2^41; squares inside a group < 2^99
    rng = np.random.default_rng(5)
    groups = []
    for size, centre in zip((1, 2, 3, 4, 5), ([a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, a])):
        groups.append(np.array(centre)[None, :] + rng.integers(0, 16, size=(size, 3)) * step)
    pts = np.concatenate(groups).astype(np.float32)
    size_of = np.repeat([1, 2, 3, 4, 5], [1, 2, 3, 4, 5])
    perm = rng.permutation(15)
    pts, size_of = pts[perm], size_of[perm]
    want = KO.dist_cuda2(pts)
    assert (want[size_of <= 2] == np.inf).all() and np.isfinite(want[size_of >= 3]).all()
    assert (want[size_of == 3] > 1e38).all() and (want[size_of >= 4] < 1e32).all()
    _same_bits(_knn(pts), want)


# ---- the tensor forms distCUDA2 accepts -------------------------------------------------------------------------------
def test_input_forms_give_the_plain_result():
    from simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(2)
    wide = torch.randn(3001, 6, generator=g, dtype=torch.float64).to(DEV)
    plain = wide[:, :3].to(torch.float32).contiguous()
    want = distCUDA2(plain)
    _same_bits(want.cpu().numpy(), KO.dist_cuda2(plain.cpu().numpy()))
    view = wide.to(torch.float32)[:, :3]
    assert not view.is_contiguous()
    assert torch.equal(distCUDA2(view), want)                                   # a [N,3] view of [N,6]
    assert torch.equal(distCUDA2(wide[:, :3]), want)                            # float64 (and strided)
    assert torch.equal(distCUDA2(wide[:, :3].contiguous()), want)               # float64, contiguous
    leaf = plain.clone().requires_grad_(True)
    out = distCUDA2(leaf)
    assert torch.equal(out, want) and not out.requires_grad                     # requires_grad
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        made = (wide[:, :3] * 2.0 - wide[:, :3]).to(torch.float32)              # produced on the side stream
        out = distCUDA2(made)
    side.synchronize()
    assert torch.equal(made, plain) and torch.equal(out, want)


# ---- the workspace contract of the C entry ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 32769])
def test_c_entry_stays_inside_its_workspace_and_output(n):
    """sc_knn3_mean_dist2 with exactly sc_knn_workspace_bytes(n) bytes: guard zones around the workspace and around
    `out` are intact afterwards, and the result is the expected one."""
    from street_crafter_amd import _lib
    lib = _lib.load()
    pts, cl = ref.clustered(n, BOUNDARY[n], seed=n)
    ar = Arena({"points": n * 12, "out": n * 4, "ws": lib.sc_knn_workspace_bytes(n)}, DEV)
    ar.view("points", torch.float32).copy_(torch.from_numpy(pts.reshape(-1)))
    rc = lib.sc_knn3_mean_dist2(ar.ptr("points"), n, ar.ptr("out"), ar.ptr("ws"), ar.nbytes("ws"),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    got = ar.view("out", torch.float32).cpu().numpy()
    assert ar.broken_guards() == []
    _same_bits(ar.view("points", torch.float32).cpu().numpy(), pts.reshape(-1))
    _same_bits(got, ref.ref_clustered(pts, cl))
