"""tests/guard_arena.py on host memory, and the two checks that keep the GPU sweep (tests/test_abi_guards_gpu.py) from
being bypassed silently: every allocator the ctypes adapter calls is one the proxy intercepts, and every public function
of the adapter is the subject of a sweep case or exempt because it launches no kernel."""
import ast
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as GA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTER = os.path.join(ROOT, "street_crafter_amd", "_ctypes_binding.py")

# every allocation pattern of the adapter: (function, args, kwargs)
F32, I32, I64, U8, F64, BOOL = torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64, torch.bool
PATTERNS = [
    ("empty", ((2, 5),), dict(dtype=I32)), ("empty", ((2, 5, 3),), dict(dtype=F32)), ("empty", (4,), dict(dtype=I64)),
    ("empty", (300,), dict(dtype=U8)), ("empty", ((), ), dict(dtype=F32)), ("empty", (0,), dict(dtype=I64)),
    ("empty", (3, 7, 5), dict(dtype=F32)), ("empty", (1, 7, 5, 4), dict(dtype=F32)), ("empty", ((0, 3),), dict(dtype=F32)),
    ("empty", ((2, 3, 4, 5),), dict(dtype=BOOL)), ("empty", (3,), dict(dtype=F64)), ("empty", ((2, 0, 3),), dict(dtype=F32)),
    ("empty", (7,), dict(dtype=U8)), ("empty", ((2, 1, 37, 53, 7),), dict(dtype=F32)), ("empty", ((37, 53, 3),), dict(dtype=U8)),
    ("zeros", (11,), dict(dtype=F32)), ("zeros", ((3, 8),), dict(dtype=I32)), ("zeros", (0,), dict(dtype=F32)),
]


def _real(fn, args, kw):
    return getattr(torch, fn)(*args, device="cpu", **kw)


@pytest.mark.parametrize("fill", [(0xA5, 0xA5), (0x3F, 0x00)])
def test_the_proxy_returns_what_torch_returns(fill):
    alloc = GA.GuardedAlloc(*fill)
    proxy = GA.TorchProxy(alloc)
    assert proxy.float32 is torch.float32 and proxy.split is torch.split          # everything else is torch's
    for fn, args, kw in PATTERNS:
        want = _real(fn, args, kw)
        got = getattr(proxy, fn)(*args, device="cpu", **kw)
        assert (got.shape, got.dtype, got.stride(), got.is_contiguous()) == \
               (want.shape, want.dtype, want.stride(), want.is_contiguous()), (fn, args)
        assert got.numel() == 0 or got.data_ptr() % 256 == 0
        raw = got.reshape(-1).view(torch.uint8)
        assert bool((raw == (0 if fn == "zeros" else alloc.fill_of(got.dtype))).all()), (fn, args)
    # the *_like forms: a contiguous tensor, a permuted dense one (strides preserved), a sliced one (made contiguous)
    base = torch.arange(2 * 3 * 4, dtype=F32).reshape(2, 3, 4)
    for src in (base, base.permute(2, 0, 1), base[:, :, :3], torch.zeros((), dtype=F32), torch.zeros(0, 3)):
        for fn in ("empty_like", "zeros_like"):
            want, got = getattr(torch, fn)(src), getattr(proxy, fn)(src)
            assert (got.shape, got.dtype, got.stride(), got.is_contiguous()) == \
                   (want.shape, want.dtype, want.stride(), want.is_contiguous()), (fn, src.shape)
    full = proxy.full((3, 2), 7.0, dtype=F32, device="cpu")
    assert torch.equal(full, torch.full((3, 2), 7.0)) and full.stride() == (2, 1)
    assert alloc.broken_guards() == [] and len(alloc.records) == len(PATTERNS) + 11
    assert alloc.fill_of(F32) == alloc.fill_of(I32) == alloc.fill_of(I64) == fill[0]
    assert alloc.fill_of(U8) == alloc.fill_of(BOOL) == fill[1]


def test_guard_copies_keep_shape_strides_and_bytes():
    alloc = GA.GuardedAlloc()
    base = torch.arange(2 * 5 * 4, dtype=F32).reshape(2, 5, 4)
    for src in (base, base[..., :3], base.permute(2, 0, 1)[:3], torch.tensor(3.0), torch.zeros(0, 2), base[0, :, 0] > 7):
        g = alloc.guard(src)
        assert (g.shape, g.dtype, g.stride()) == (src.shape, src.dtype, src.stride()) and torch.equal(g, src)
        assert g.numel() == 0 or (g.data_ptr() % 256 == 0 and g.data_ptr() != src.data_ptr())
    assert alloc.broken_guards() == []
    assert alloc.index_at(alloc.records[1]["tensor"].data_ptr()) == 1


def test_a_byte_outside_is_reported_and_a_byte_inside_is_not():
    alloc = GA.GuardedAlloc(0xA5, 0xA5)
    first = alloc.empty((3, 5), F32, "cpu")
    t = alloc.empty((3, 37, 53), F32, "cpu")
    rec = alloc.record_of(t)
    assert alloc.index_of(t) == 1 and rec["nbytes"] == 3 * 37 * 53 * 4 and rec["off"] >= GA.ZONE
    assert rec["base"].numel() - rec["off"] - rec["nbytes"] >= GA.ZONE
    t.fill_(1.5)                                           # every byte inside: not a guard
    first.zero_()
    assert alloc.broken_guards() == []
    raw = rec["base"]
    end = rec["off"] + rec["nbytes"]
    raw[end] = 0                                           # one past the end
    assert alloc.broken_guards() == [(1, "after", rec["nbytes"])]
    raw[end] = 0xA5
    raw[rec["off"] - 1] = 0                                # one before the start
    raw[end + 100] = 1                                     # the FIRST changed offset is reported
    raw[end + 7] = 1
    assert alloc.broken_guards() == [(1, "before", -1), (1, "after", rec["nbytes"] + 7)]
    # the same through Arena, whose guard byte is now a parameter
    for fill in (0xA5, 0x3F):
        arena = GA.Arena({"a": 10, "b": 300}, device="cpu", fill=fill)
        assert bool((arena.mem == fill).all()) and arena.broken_guards() == []
        arena.view("a").fill_(7)
        assert arena.broken_guards() == []
        arena.mem[arena.span["b"][1]] = 1
        assert [b[2] for b in arena.broken_guards()] == [arena.span["b"][1]]


def test_guarded_adapter_swaps_the_name_and_puts_it_back():
    from street_crafter_amd import _ctypes_binding as CB
    assert CB.torch is torch
    alloc = GA.GuardedAlloc()
    with pytest.raises(RuntimeError, match="inside"):
        with GA.guarded_adapter(alloc):
            assert isinstance(CB.torch, GA.TorchProxy)
            ws = CB._ws(10, "cpu")                         # the adapter's own helper allocates from `alloc`
            assert ws.numel() == 256 and alloc.records[0]["tensor"] is ws
            raise RuntimeError("inside")
    assert CB.torch is torch


# torch.<name>(...) calls of the adapter that allocate nothing
NON_ALLOCATING = {"split"}


def test_every_allocator_of_the_adapter_is_intercepted():
    """A torch.full (or any other torch call) the adapter gains must be handled by the proxy, or listed above as
    allocating nothing, before this passes again."""
    tree = ast.parse(open(ADAPTER).read())
    called = {node.func.attr for node in ast.walk(tree)
              if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
              and isinstance(node.func.value, ast.Name) and node.func.value.id == "torch"}
    assert {"empty", "zeros", "empty_like"} <= called
    assert called <= set(GA.TorchProxy.INTERCEPTED) | NON_ALLOCATING, called - set(GA.TorchProxy.INTERCEPTED) - NON_ALLOCATING
    for name in GA.TorchProxy.INTERCEPTED:
        assert name in vars(GA.TorchProxy), name           # intercepted means overridden, not forwarded
    # nothing reaches torch under another name
    names = {a.name for node in ast.walk(tree) if isinstance(node, (ast.Import, ast.ImportFrom)) for a in node.names}
    assert names == {"annotations", "ctypes", "torch", "_lib"}


def test_every_adapter_function_is_swept_or_exempt_as_kernel_less():
    import test_abi_guards_gpu as sweep
    from street_crafter_amd import _ctypes_binding as CB
    public = {n for n, f in vars(CB).items() if inspect.isfunction(f) and f.__module__ == CB.__name__ and not n.startswith("_")}
    assert len(public) >= 42
    assert set(sweep.COVERED) | set(sweep.EXEMPT) == public
    assert not set(sweep.COVERED) & set(sweep.EXEMPT)
    assert set(sweep.COVERED.values()) == set(sweep.CASES)
    # an exemption is for a call that launches no kernel: it allocates nothing and its entry point takes no stream
    for name, reason in sweep.EXEMPT.items():
        src = inspect.getsource(getattr(CB, name))
        assert reason and "torch." not in src and "stream" not in src, name
    assert set(sweep.EXEMPT) == {"wait_i64"}
