"""float64 helpers for the crop + resize tests (tests/test_resize_cpu.py, tests/test_resize_gpu.py).

The truth is torch's own `F.interpolate(mode="bilinear", align_corners=False, antialias=A)` on the CPU in float64 (what
torchvision's Resize does to a tensor), applied to the cropped input.  The bars need, per output, the tap counts and the
sum of |terms|; those come from `tap_table` turned into dense float64 matrices, which test_resize_cpu.py first checks
against the oracle itself.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
TARGET = (18, 32)
UPPER = int(TARGET[0] * 0.4)                      # 7
# (shape, what the reference's crop does to it at 18x32)
CASES = [((3, 29, 50), "row crop, 4 taps"), ((3, 30, 64), "column crop"), ((3, 45, 80), "ratio 2.5, 5 taps"),
         ((3, 10, 17), "upsampling"), ((3, 18, 32), "identity")]
SHAPES = [c[0] for c in CASES]
PAIRS = [(29, 18), (50, 32), (45, 18), (80, 32), (18, 18), (10, 18), (17, 32), (900, 576), (1600, 1024)]


def interpolate64(x, size, antialias):
    """x float64 numpy [..., H, W] -> [..., h, w] by torch on the CPU."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    lead = t.shape[:-2]
    t4 = t.reshape((-1, 1) + tuple(t.shape[-2:]))
    out = F.interpolate(t4, size=tuple(size), mode="bilinear", align_corners=False, antialias=bool(antialias))
    return out.reshape(tuple(lead) + tuple(size)).numpy()


def dense(table, use64=True):
    """The table as a float64 matrix [n_out, n_in] (float64 weights, or the stored fp32 ones)."""
    m = np.zeros((table.n_out, table.n_in))
    w = table.weight64 if use64 else table.weight.astype(np.float64)
    for i in range(table.n_out):
        a, b = table.offset[i], table.offset[i + 1]
        m[i, table.start[i]:table.start[i] + (b - a)] = w[a:b]
    return m


def dense_transposed(table):
    """The transposed table as a float64 matrix [n_out, n_in] of its fp32 weights (must equal dense(table, False))."""
    m = np.zeros((table.n_out, table.n_in))
    for k in range(table.n_in):
        a, b = table.t_offset[k], table.t_offset[k + 1]
        m[table.t_start[k]:table.t_start[k] + (b - a), k] += table.t_weight[a:b].astype(np.float64)
    return m


def apply_tables(x, ty, tx):
    """x float64 [..., in_h, in_w] -> [..., h_out, w_out] through the float64 weights."""
    return dense(ty) @ x @ dense(tx).T


def image(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


def mask(shape, frac_true, seed):
    rng = np.random.default_rng(seed)
    return rng.random((1,) + tuple(shape[-2:])) < frac_true


class Truth:
    """Everything float64 about one case: x fp32 numpy [..., C, H, W], the reference's crop at `size`, rows row_begin:."""

    def __init__(self, resize_mod, x, size, antialias, row_begin=0, crop=True):
        H, W = x.shape[-2:]
        self.box = resize_mod.crop_box(H, W, size[0], size[1]) if crop else (0, H, 0, W)
        t, b, l, r = self.box
        self.x, self.size, self.antialias, self.row_begin = x, tuple(size), bool(antialias), row_begin
        self.crop = x[..., t:b, l:r].astype(np.float64)
        self.ty = resize_mod.tap_table(b - t, size[0], antialias)
        self.tx = resize_mod.tap_table(r - l, size[1], antialias)
        self.My, self.Mx = dense(self.ty)[row_begin:], dense(self.tx)

    def forward(self):
        """(want, bar) over the rows row_begin:  want from torch, bar = 2^-24 (Ty + Tx + 4) sum wy wx |x|."""
        want = interpolate64(self.crop, self.size, self.antialias)[..., self.row_begin:, :]
        A = self.My @ np.abs(self.crop) @ self.Mx.T
        taps = self.ty.counts()[self.row_begin:, None] + self.tx.counts()[None, :]
        return want, EPS * (taps + 4) * A, A

    def backward(self, g, scale=1.0):
        """g fp32 numpy in the output's layout -> (want, bar, reached) in x's layout: want the float64 sum of the
        contributing terms (zero outside the crop), bar = 2^-24 (n + 4) S, reached = inputs with a contributing output."""
        t, b, l, r = self.box
        g = g.astype(np.float64) * scale
        want, S, n = (np.zeros(self.x.shape) for _ in range(3))
        want[..., t:b, l:r] = self.My.T @ g @ self.Mx
        S[..., t:b, l:r] = self.My.T @ np.abs(g) @ self.Mx
        n[..., t:b, l:r] = ((self.My != 0).sum(0)[:, None] * (self.Mx != 0).sum(0)[None, :])
        return want, EPS * (n + 4) * S, n > 0

    def autograd(self, g, scale=1.0, shift=0.0):
        """The same gradient from torch's autograd on crop + F.interpolate in float64."""
        t, b, l, r = self.box
        x = torch.from_numpy(self.x.astype(np.float64)).requires_grad_(True)
        c = x[..., t:b, l:r]
        c4 = c.reshape((-1, 1) + tuple(c.shape[-2:]))
        y = F.interpolate(c4, size=self.size, mode="bilinear", align_corners=False, antialias=self.antialias)
        y = y.reshape(tuple(c.shape[:-2]) + self.size)[..., self.row_begin:, :] * scale + shift
        y.backward(torch.from_numpy(g.astype(np.float64)))
        return y.detach().numpy(), x.grad.numpy()

    def mask(self, m):
        """m bool numpy [..., H, W] -> (want bool, the float64 value, residue_only) over rows row_begin:.
        residue_only marks the outputs whose only set taps are residue taps (weight below RESIDUE: what float64
        rounding leaves of a weight that is zero in exact arithmetic); their value is positive but far below any real
        weight, and float32 arithmetic may as well call it zero."""
        t, b, l, r = self.box
        c = m[..., t:b, l:r].astype(np.float64)
        v = interpolate64(c, self.size, self.antialias)[..., self.row_begin:, :]
        solid = ((self.My >= RESIDUE).astype(np.float64) @ c @ (self.Mx >= RESIDUE).astype(np.float64).T) != 0
        return v != 0, v, (v != 0) & ~solid


RESIDUE = 2.0 ** -40
