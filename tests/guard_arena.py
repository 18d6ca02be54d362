"""One device allocation cut into named buffers with guard zones between and around them (GPU tests only).

Every byte of the arena that belongs to no buffer holds 0xA5.  A buffer starts on a 256-byte boundary and its guard
begins at its very last byte + 1, so a kernel that writes one element past a buffer it was given -- or past the
workspace size its own *_workspace_bytes() reports -- changes a guard byte, and intact() reads that back.  Nothing is
under-sized to see what happens: the sizes are the ones the C ABI asks for.

GuardedAlloc / TorchProxy / guarded_adapter put the same guards around everything the ctypes adapter
(street_crafter_amd/_ctypes_binding.py) allocates: inside `with guarded_adapter(alloc):` the name `torch` of that one
module is a proxy whose `empty` / `zeros` / `empty_like` (and `zeros_like` / `full`) come from `alloc`, each tensor cut
from a block of its own, so every output and workspace of every operator on the ctypes route lies between guards
without an argument list being restated.  Two fills make a stray READ visible as well: what a kernel takes from past an
input, or leaves unwritten in an output, differs between a run under 0xA5 and one under 0x3F (0.747 as a float)."""
import contextlib

import torch

ZONE = 256
FILL = 0xA5


def _up(x, a=256):
    return (x + a - 1) // a * a


class Arena:
    def __init__(self, sizes, device="cuda", fill=FILL):
        """sizes: {name: bytes}, laid out in that order; fill: the guard byte (and what every buffer holds at first)."""
        self.fill = int(fill)
        self.span = {}
        o = ZONE
        for name, nbytes in sizes.items():
            o = _up(o)
            self.span[name] = (o, o + int(nbytes))
            o += int(nbytes) + ZONE
        self.mem = torch.full((_up(o),), self.fill, dtype=torch.uint8, device=device)

    def view(self, name, dtype=torch.uint8):
        s, e = self.span[name]
        return self.mem[s:e].view(dtype)

    def ptr(self, name):
        return self.mem.data_ptr() + self.span[name][0]

    def nbytes(self, name):
        s, e = self.span[name]
        return e - s

    def guards(self):
        """The byte ranges outside every buffer."""
        edges = [0]
        for s, e in self.span.values():
            edges += [s, e]
        edges.append(self.mem.numel())
        return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2)]

    def broken_guards(self):
        """[(start, end, first changed offset)] of the guard ranges that no longer hold the fill byte throughout."""
        bad = []
        for s, e in self.guards():
            assert e - s >= ZONE
            ne = self.mem[s:e] != self.fill
            if bool(ne.any()):
                bad.append((s, e, s + int(ne.nonzero()[0])))
        return bad


_BYTE_DTYPES = (torch.uint8, torch.bool, torch.int8)


def _extent(shape, strides):
    """Elements of storage a tensor of this shape and these strides spans from its first element (0 = it has none)."""
    if any(n == 0 for n in shape):
        return 0
    return 1 + sum((n - 1) * s for n, s in zip(shape, strides))


class GuardedAlloc:
    """Hands out tensors, each inside a uint8 block of its own: 256-byte aligned start, at least ZONE guard bytes before
    the first byte and after the last one, the guard beginning at the last byte + 1.  Remembers every tensor handed out."""

    def __init__(self, fill_float=FILL, fill_byte=FILL):
        self.fill_float, self.fill_byte = int(fill_float), int(fill_byte)
        self.records = []          # dicts: base, off, nbytes, fill, tensor, shape, dtype

    def fill_of(self, dtype):
        return self.fill_byte if dtype in _BYTE_DTYPES else self.fill_float

    def _cut(self, shape, strides, dtype, device, zero=False):
        shape, strides = tuple(int(n) for n in shape), tuple(int(s) for s in strides)
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = _extent(shape, strides) * item
        fill = self.fill_of(dtype)
        base = torch.full((ZONE + 256 + nbytes + ZONE,), fill, dtype=torch.uint8, device=device)
        off = ZONE + (-(base.data_ptr() + ZONE)) % 256
        inner = base[off:off + nbytes]
        if zero:
            inner.zero_()
        t = torch.as_strided(inner.view(dtype), shape, strides)
        assert nbytes == 0 or (t.data_ptr() % 256 == 0 and t.data_ptr() == base.data_ptr() + off)
        self.records.append(dict(base=base, off=off, nbytes=nbytes, fill=fill, tensor=t, shape=shape, dtype=dtype))
        return t

    def empty(self, shape, dtype, device, strides=None, zero=False):
        if strides is None:
            strides = torch.empty(tuple(shape), dtype=dtype, device="meta").stride()
        return self._cut(shape, strides, dtype, device, zero)

    def zeros(self, shape, dtype, device, strides=None):
        return self.empty(shape, dtype, device, strides, zero=True)

    def guard(self, t):
        """A guarded copy of `t`: same shape, dtype, strides and -- element for element of the storage it spans -- bytes."""
        g = self._cut(t.shape, t.stride(), t.dtype, t.device)
        n = _extent(tuple(t.shape), tuple(t.stride()))
        if n:
            torch.as_strided(g, (n,), (1,)).copy_(torch.as_strided(t.detach(), (n,), (1,)))
        return g

    def record_of(self, t):
        for r in self.records:
            if r["tensor"] is t:
                return r
        raise KeyError("not a tensor of this allocator")

    def index_of(self, t):
        for i, r in enumerate(self.records):
            if r["tensor"] is t:
                return i
        raise KeyError("not a tensor of this allocator")

    def index_at(self, data_ptr):
        """The hand-out index of the tensor that starts at this address (a view an operator returns keeps the address)."""
        for i, r in enumerate(self.records):
            if r["nbytes"] and r["base"].data_ptr() + r["off"] == data_ptr:
                return i
        raise KeyError("no tensor of this allocator starts there")

    def broken_guards(self):
        """[(index of the tensor in hand-out order, "before" | "after", first changed byte offset counted from the tensor's
        first byte: negative before it, >= its recorded size after it)]."""
        bad = []
        for i, r in enumerate(self.records):
            base, off, end = r["base"], r["off"], r["off"] + r["nbytes"]
            for side, s, e in (("before", 0, off), ("after", end, base.numel())):
                assert e - s >= ZONE
                ne = base[s:e] != r["fill"]
                if bool(ne.any()):
                    bad.append((i, side, s + int(ne.nonzero()[0]) - off))
        return bad


class TorchProxy:
    """Stands in for the name `torch` of one module: every attribute is real torch's, the allocators come from `alloc`
    with the shape, dtype, device and strides real torch would give."""
    INTERCEPTED = ("empty", "zeros", "empty_like", "zeros_like", "full")

    def __init__(self, alloc):
        self._alloc = alloc

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _meta(fn, args, kw):
        return fn(*args, **{**kw, "device": "meta"})

    def empty(self, *args, **kw):
        m = self._meta(torch.empty, args, kw)
        return self._alloc.empty(m.shape, m.dtype, kw.get("device", "cpu"), m.stride())

    def zeros(self, *args, **kw):
        m = self._meta(torch.zeros, args, kw)
        return self._alloc.zeros(m.shape, m.dtype, kw.get("device", "cpu"), m.stride())

    def full(self, size, fill_value, **kw):
        m = self._meta(torch.full, (size, fill_value), kw)
        return self._alloc.empty(m.shape, m.dtype, kw.get("device", "cpu"), m.stride()).fill_(fill_value)

    def empty_like(self, t, **kw):
        m = self._meta(torch.empty_like, (t,), kw)
        return self._alloc.empty(m.shape, m.dtype, kw.get("device", t.device), m.stride())

    def zeros_like(self, t, **kw):
        m = self._meta(torch.zeros_like, (t,), kw)
        return self._alloc.zeros(m.shape, m.dtype, kw.get("device", t.device), m.stride())


@contextlib.contextmanager
def guarded_adapter(alloc):
    """The ctypes adapter allocates from `alloc` inside the block (use with _lib.set_fast_binding(False))."""
    from street_crafter_amd import _ctypes_binding
    prev = _ctypes_binding.torch
    _ctypes_binding.torch = TorchProxy(alloc)
    try:
        yield alloc
    finally:
        _ctypes_binding.torch = prev
