"""sc_radix_sort_pairs_u64_i32 (csrc/radix_sort.hip) at its structural sizes, against numpy's stable argsort.

The contract (include/street_crafter_amd.h): a stable sort of (u64 key, i32 value) pairs over key bits [0, end_bit).  So

    order = np.argsort(keys & mask(end_bit), kind="stable");  keys_out == keys[order];  vals_out == vals[order]

with keys compared as whole 64-bit words: bits at and above end_bit take no part in the order and travel with their
key.  Everything is an integer; nothing has a tolerance.

Sizes sit on and beside every unit of the kernels: 64 keys (a round of one wave), 256 (a round of the histogram), 1024
(one wave's share of a tile), 4096 (a tile, one workgroup), 2^20 + 1 keys = 257 tiles (the second trip of the
cross-workgroup scan, carrying into a single live thread) and 2^20 + 4097 = 258 tiles.  end_bit gives 1, 1, 1, 2, 2, 4,
5, 6, 8 and 8 passes: an odd count ends in tmp_* and is copied back.  Every call runs inside one arena with guard zones
(guard_arena.py) and exactly sc_radix_sort_workspace_bytes(n) bytes of workspace.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guard_arena import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL = (2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
LARGE = (1 << 20, (1 << 20) + 1, (1 << 20) + 4097)
END_BITS = (1, 7, 8, 9, 16, 30, 33, 47, 63, 64)
FAMILIES = ("random64", "in_range", "all_ones", "constant_digit", "two_values", "sorted", "reversed", "isect_like")
U64 = np.uint64


def mask_of(end_bit):
    return U64(0xFFFFFFFFFFFFFFFF) if end_bit >= 64 else U64((1 << end_bit) - 1)


def make_keys(family, n, end_bit, rng):
    m = mask_of(end_bit)
    rand = lambda: rng.integers(0, 1 << 64, size=n, dtype=U64)      # noqa: E731
    if family == "random64":            # the contract case: bits above end_bit are set and must not order anything
        return rand()
    if family == "in_range":            # what today's callers pass
        return rand() & m
    if family == "all_ones":            # shares digit 0xff with the ~0 padding of a ragged tile's invalid lanes
        return np.full(n, 0xFFFFFFFFFFFFFFFF, dtype=U64)
    if family == "constant_digit":      # every 8-bit digit equal: one bucket in every pass, 64 equal lanes per round
        return np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=U64)
    if family == "two_values":
        a, b = rng.integers(0, 1 << 64, size=2, dtype=U64)
        return np.where(np.arange(n) % 2 == 0, a, b).astype(U64)
    if family in ("sorted", "reversed"):    # in order over [0, end_bit), random above it
        k = np.sort(rand() & m) | (rand() & ~m)
        return k if family == "sorted" else np.ascontiguousarray(k[::-1])
    if family == "isect_like":          # tile << 32 | float32 depth bits: ~50 tiles, few distinct depths
        tile = rng.integers(0, 50, size=n, dtype=np.int64).astype(U64)
        depth = rng.choice(rng.uniform(0.2, 80.0, size=97).astype(np.float32), size=n).view(np.uint32).astype(U64)
        return (tile << U64(32)) | depth
    raise KeyError(family)


def make_vals(n, rng):
    """Random int32 over the whole range, every third from seven values: negatives and duplicates."""
    v = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int32)
    v[::3] = v[::3] % 7 - 3
    return v


def cases():
    out = [("random64", n, eb) for n in SMALL for eb in END_BITS]
    out += [("random64", n, eb) for n in LARGE for eb in (9, 30, 64)]
    out += [(f, n, eb) for f in FAMILIES[1:] for n in SMALL + LARGE for eb in (30, 64)]
    return out


@pytest.fixture(scope="module")
def lib():
    from street_crafter_amd import _lib
    return _lib.load()          # ImportError if the HIP library is missing: no fallback


def _arena(lib, n_alloc, n_ws):
    return Arena({"keys": n_alloc * 8, "vals": n_alloc * 4, "tmp_keys": n_alloc * 8, "tmp_vals": n_alloc * 4,
                  "ws": lib.sc_radix_sort_workspace_bytes(n_ws)}, DEV)


def _sort(lib, ar, n, end_bit):
    rc = lib.sc_radix_sort_pairs_u64_i32(ar.ptr("keys"), ar.ptr("vals"), ar.ptr("tmp_keys"), ar.ptr("tmp_vals"), n,
                                         end_bit, ar.ptr("ws"), ar.nbytes("ws"),
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("family,n,end_bit", cases(), ids=lambda v: str(v))
def test_sort_matches_stable_argsort_over_end_bit(lib, family, n, end_bit):
    rng = np.random.default_rng([FAMILIES.index(family), n, end_bit])
    keys, vals = make_keys(family, n, end_bit, rng), make_vals(n, rng)
    order = np.argsort(keys & mask_of(end_bit), kind="stable")
    ar = _arena(lib, n, n)
    ar.view("keys", torch.int64).copy_(torch.from_numpy(keys.view(np.int64)))
    ar.view("vals", torch.int32).copy_(torch.from_numpy(vals))
    assert _sort(lib, ar, n, end_bit) == 0
    got_k = ar.view("keys", torch.int64).cpu().numpy().view(U64)
    got_v = ar.view("vals", torch.int32).cpu().numpy()
    assert ar.broken_guards() == []
    np.testing.assert_array_equal(got_k, keys[order])
    np.testing.assert_array_equal(got_v, vals[order])


@pytest.mark.parametrize("n,end_bit", [(0, 30), (1, 30), (1, 64), (8, 0), (4097, 0)])
def test_noop_leaves_every_array_unchanged(lib, n, end_bit):
    """n = 0, n = 1 and end_bit = 0 sort nothing: keys, vals and both temporaries keep every bit."""
    n_alloc = max(n, 8)
    rng = np.random.default_rng([n, end_bit])
    ar = _arena(lib, n_alloc, n)
    before = {}
    for name, dt, npdt in (("keys", torch.int64, np.int64), ("vals", torch.int32, np.int32),
                           ("tmp_keys", torch.int64, np.int64), ("tmp_vals", torch.int32, np.int32)):
        before[name] = rng.integers(np.iinfo(npdt).min, np.iinfo(npdt).max, size=n_alloc, dtype=npdt)
        ar.view(name, dt).copy_(torch.from_numpy(before[name]))
    assert _sort(lib, ar, n, end_bit) == 0
    for name, dt in (("keys", torch.int64), ("vals", torch.int32), ("tmp_keys", torch.int64), ("tmp_vals", torch.int32)):
        np.testing.assert_array_equal(ar.view(name, dt).cpu().numpy(), before[name])
    assert ar.broken_guards() == []
