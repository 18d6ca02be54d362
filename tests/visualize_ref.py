"""numpy restatement of what the reference's visualizer computes for its videos (checker only): visualize_depth_numpy
(street_gaussian/utils/img_utils.py:239-252) with the colour table spelled `lut[...]` for cv2.applyColorMap,
visualize_diff's map (street_gaussian_visualizer.py:108-114) and the `* 255` casts (:66-75, :97-99).

float32 throughout, as NumPy >= 2 evaluates those lines (a Python float next to a float32 array or scalar stays
float32).  `.astype(np.uint8)` of a value outside [0, 256) is platform-defined in numpy and warns; q() spells what the
x86 hosts of the reference give -- the low 8 bits of the truncated value, 0 for NaN / inf -- with integer operations, and
asserts that the plain cast agrees wherever it is defined."""
import numpy as np

F32 = np.float32


def q(t):
    """(t).astype(np.uint8) on x86: trunc -> two's-complement integer -> low 8 bits; NaN / inf -> 0.  Magnitudes of 2^63
    and more are multiples of 256 (low bits 0) and are not pushed through the int64 conversion."""
    t = np.asarray(t, dtype=F32)
    ok = np.isfinite(t) & (np.abs(t) < F32(2.0 ** 62))
    i = np.trunc(np.where(ok, t, F32(0))).astype(np.int64)
    out = (i & 255).astype(np.uint8)
    inr = ok & (t >= 0) & (t < 256)
    assert np.array_equal(out[inr], t[inr].astype(np.uint8)), "q() disagrees with the plain cast inside [0, 256)"
    return out


def nan_to_num(v):
    return np.nan_to_num(np.asarray(v, dtype=F32))


def value_range(v):
    """(mi, ma) as float32 scalars: the smallest x > 0 (0 where there is none: np.min raises there) and the largest x."""
    x = nan_to_num(v)
    pos = x[x > 0]
    mi = np.min(pos) if pos.size else F32(0)
    return F32(mi), F32(np.max(x))


def colorize(v, lut, minmax=None):
    """visualize_depth_numpy(v, minmax, cmap)[0][..., [2, 1, 0]] with lut = the RGB table of cmap; v [H,W] -> [H,W,3]."""
    x = nan_to_num(v)
    mi, ma = value_range(x) if minmax is None else (F32(minmax[0]), F32(minmax[1]))
    with np.errstate(all="ignore"):
        x = (x - mi) / (ma - mi + F32(1e-8))
        t = F32(255) * x
    assert x.dtype == F32 and t.dtype == F32
    return np.asarray(lut)[q(t)]


def diff_map(rgb, gt, mask=None):
    """visualize_diff's map; rgb, gt [3,H,W], mask bool [H,W] or None -> [H,W].  numpy adds the three squares of the last
    axis left to right."""
    rgb, gt = np.asarray(rgb, dtype=F32), np.asarray(gt, dtype=F32)
    if mask is None:
        mask = np.ones(rgb.shape[1:], dtype=bool)
    m = np.asarray(mask).astype(bool)[None]
    a = np.where(m, rgb, F32(0)).transpose(1, 2, 0)
    b = np.where(m, gt, F32(0)).transpose(1, 2, 0)
    with np.errstate(all="ignore"):
        d = (a - b) ** 2
        out = (d[..., 0] + d[..., 1]) + d[..., 2]
        assert np.array_equal(out, d.sum(axis=-1), equal_nan=True)
    return out


def gray(a):
    """(a * 255).astype(np.uint8) of an accumulation map [H,W] -> [H,W,1]."""
    with np.errstate(all="ignore"):
        return q(np.asarray(a, dtype=F32) * 255)[..., None]


def rgb_u8(img_chw):
    """(img.transpose(1, 2, 0) * 255).astype(np.uint8) of a [3,H,W] image in [0, 1]."""
    return q(np.asarray(img_chw, dtype=F32).transpose(1, 2, 0) * 255)
