"""One device allocation cut into named buffers with guard zones between and around them (GPU tests only).

Every byte of the arena that belongs to no buffer holds 0xA5.  A buffer starts on a 256-byte boundary and its guard
begins at its very last byte + 1, so a kernel that writes one element past a buffer it was given -- or past the
workspace size its own *_workspace_bytes() reports -- changes a guard byte, and intact() reads that back.  Nothing is
under-sized to see what happens: the sizes are the ones the C ABI asks for."""
import torch

ZONE = 256
FILL = 0xA5


def _up(x, a=256):
    return (x + a - 1) // a * a


class Arena:
    def __init__(self, sizes, device="cuda"):
        """sizes: {name: bytes}, laid out in that order."""
        self.span = {}
        o = ZONE
        for name, nbytes in sizes.items():
            o = _up(o)
            self.span[name] = (o, o + int(nbytes))
            o += int(nbytes) + ZONE
        self.mem = torch.full((_up(o),), FILL, dtype=torch.uint8, device=device)

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
        """[(start, end, first changed offset)] of the guard ranges that no longer hold 0xA5 throughout."""
        bad = []
        for s, e in self.guards():
            assert e - s >= ZONE
            ne = self.mem[s:e] != FILL
            if bool(ne.any()):
                bad.append((s, e, s + int(ne.nonzero()[0])))
        return bad
