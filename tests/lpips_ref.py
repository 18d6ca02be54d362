"""Reference for the perceptual-loss kernels (street_crafter_amd/lpips.py, csrc/lpips.hip), in numpy, and the inputs
their tests share.

Every function is written once and runs in the dtype it is handed.  In float64 on the fp32 inputs it is the reference the
kernels are judged against; in float32 it is the "replay": the same formulas in the kernels' precision, with no kernel,
whose distance from the float64 result says how much error the precision alone explains (K_FWD_REPLAY, K_BWD_REPLAY).

The formulas (include/street_crafter_amd.h), for one tap with features fx, fy [C,P] and weights w [C]:

    n(f)_p = sqrt(sum_c f_cp^2)       fh_cp = f_cp / (n_p + eps)        eps = 1e-10 rounded to fp32
    d      = (1 / P) sum_p sum_c w_c (fhx_cp - fhy_cp)^2                 out = sum over taps of d
    backward, upstream g:  r = 1 / (n + eps),  u_c = fhx_c - fhy_c,  a_c = 2 g w_c u_c / P
        grad_fx_k = r a_k - fx_k (r^2 / n) sum_c a_c fx_c                (second term 0 where n == 0)
        grad_fy_k = -(r a_k) + fy_k (r^2 / n) sum_c a_c fy_c             (r, n of fy)

Where n == 0 every f of the pixel is 0 and fh = 0.  The second term is bounded by |f_k| (r^2 / n) n |a|_2 <= r^2 n |a|_2
(Cauchy-Schwarz, |f_k| <= n), with r <= 1 / eps and a bounded: it vanishes with n, so its limit along f -> 0 is 0 and the
gradient there is r a_k, finite.  torch's autograd gives NaN at such a pixel (test_lpips_cpu.py shows it).

The bars, with a = fhx, b = fhy, u = a - b, in float64:

    forward, per tap:       |hip - f64| <= 2^-24 K (1/P) sum_pc |w_c| (2 |u| (|a| + |b|) + u^2)
    total:                  the sum of the tap bars plus one rounding per addition: 2^-24 (|partial sum| + the bars so far)
    backward, per element:  |hip - f64| <= 2^-24 K (r A_k + |fx_k| (r^2 / n) sum_c A_c |fx_c|),
                            A_c = 2 |g| |w_c| (|a_c| + |b_c|) / P        (second term 0 where n == 0)

K = 4 x the replay constants below: the kernel may sum in another order and fuse multiply-adds, which the replay does not.
Every tap and every element is judged; inputs are exactly 0 or of magnitude in [1e-3, 1e3], so nothing has to be left out
(features small enough for f^2 to underflow in fp32 are outside the kernels' contract).
"""
import numpy as np

EPS = 2.0 ** -24
LPIPS_EPS = float(np.float32(1e-10))

# What the float32 replay reaches over every case of cases(), in bar units (test_lpips_cpu.py checks both against a fresh
# replay).  Measured on the CPU with
#     python -c "import sys; sys.path.insert(0, 'tests'); import lpips_ref; print(lpips_ref.replay_constants())"
# -> (0.8879, 16.1429).  The backward's constant is large because the replay adds the squares of up to 512 channels one
# after the other in fp32 and the norm's error enters r^2 / n three times; it is what fp32 gives for these formulas.
K_FWD_REPLAY = 0.89
K_BWD_REPLAY = 16.2


# ---- prep ----------------------------------------------------------------------------------------------------------
def prep(img, mask, mean, std, dtype=np.float64):
    """img [3,H,W], mask bool [H,W] or None, mean / std 3 numbers -> z [3,H,W] = (where(mask, img, 0) - mean) / std."""
    x = np.asarray(img).astype(dtype)
    if mask is not None:
        x = np.where(np.asarray(mask, bool)[None], x, dtype(0))
    m = np.asarray(mean, np.float32).astype(dtype).reshape(3, 1, 1)
    s = np.asarray(std, np.float32).astype(dtype).reshape(3, 1, 1)
    return ((x - m) / s).astype(dtype)


def prep_bwd(grad, mask, std, dtype=np.float64):
    g = np.asarray(grad).astype(dtype) / np.asarray(std, np.float32).astype(dtype).reshape(3, 1, 1)
    if mask is not None:
        g = np.where(np.asarray(mask, bool)[None], g, dtype(0))
    return g.astype(dtype)


# ---- head ----------------------------------------------------------------------------------------------------------
def normalize(f, dtype=np.float64):
    """f [C,P] -> (n [P], fh [C,P])"""
    f = np.asarray(f).astype(dtype)
    n = np.sqrt(np.sum(f * f, axis=0)).astype(dtype)
    return n, (f / (n + dtype(LPIPS_EPS))).astype(dtype)


def head_fwd(taps, dtype=np.float64):
    """taps: [(fx [C,P], fy [C,P], w [C])] -> (d [n_taps], total), total added in tap order in `dtype`."""
    d = np.zeros(len(taps), dtype)
    for l, (fx, fy, w) in enumerate(taps):
        _nx, a = normalize(fx, dtype)
        _ny, b = normalize(fy, dtype)
        u = a - b
        P = dtype(fx.shape[1])
        d[l] = np.sum(np.asarray(w).astype(dtype)[:, None] * (u * u)) / P
    total = dtype(0)
    for v in d:
        total = dtype(total + v)
    return d, total


def head_bwd(taps, g, dtype=np.float64):
    """-> [(grad_fx [C,P], grad_fy [C,P])], the closed form with the n == 0 rule."""
    out = []
    g = dtype(g)
    with np.errstate(divide="ignore", invalid="ignore"):
        for fx, fy, w in taps:
            fx, fy = np.asarray(fx).astype(dtype), np.asarray(fy).astype(dtype)
            nx, a = normalize(fx, dtype)
            ny, b = normalize(fy, dtype)
            rx, ry = dtype(1) / (nx + dtype(LPIPS_EPS)), dtype(1) / (ny + dtype(LPIPS_EPS))
            P = dtype(fx.shape[1])
            ac = dtype(2) * g * np.asarray(w).astype(dtype)[:, None] * (a - b) / P
            kx = np.where(nx > 0, (rx * rx / nx) * np.sum(ac * fx, axis=0), dtype(0))
            ky = np.where(ny > 0, (ry * ry / ny) * np.sum(ac * fy, axis=0), dtype(0))
            out.append(((rx * ac - fx * kx).astype(dtype), (fy * ky - ry * ac).astype(dtype)))
    return out


def fwd_units(taps):
    """Per tap, in float64: (1/P) sum_pc |w_c| (2 |u| (|a| + |b|) + u^2)."""
    units = np.zeros(len(taps))
    for l, (fx, fy, w) in enumerate(taps):
        _nx, a = normalize(fx)
        _ny, b = normalize(fy)
        u = a - b
        aw = np.abs(np.asarray(w, np.float64))[:, None]
        units[l] = np.sum(aw * (2 * np.abs(u) * (np.abs(a) + np.abs(b)) + u * u)) / fx.shape[1]
    return units


def total_bar(d64, tap_bars):
    """The bar of the total: the tap bars, plus one rounding per addition of the running sum."""
    bar, s = 0.0, 0.0
    for k, (v, b) in enumerate(zip(d64, tap_bars)):
        s += float(v)
        bar += float(b)
        if k:
            bar += EPS * (abs(s) + bar)
    return bar


def bwd_units(taps, g):
    """Per element, in float64: r A_k + |f_k| (r^2 / n) sum_c A_c |f_c|, for fx and for fy."""
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for fx, fy, w in taps:
            fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
            nx, a = normalize(fx)
            ny, b = normalize(fy)
            rx, ry = 1.0 / (nx + LPIPS_EPS), 1.0 / (ny + LPIPS_EPS)
            A = 2 * abs(float(g)) * np.abs(np.asarray(w, np.float64))[:, None] * (np.abs(a) + np.abs(b)) / fx.shape[1]
            kx = np.where(nx > 0, (rx * rx / nx) * np.sum(A * np.abs(fx), axis=0), 0.0)
            ky = np.where(ny > 0, (ry * ry / ny) * np.sum(A * np.abs(fy), axis=0), 0.0)
            out.append((rx * A + np.abs(fx) * kx, ry * A + np.abs(fy) * ky))
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------
def _features(rng, C, P):
    """Post-ReLU-like: about half exactly 0, the rest of magnitude 10^U(-3, 3)."""
    mag = 10.0 ** rng.uniform(-3.0, 3.0, (C, P))
    return np.where(rng.random((C, P)) < 0.5, 0.0, mag).astype(np.float32)


def _weights(rng, C):
    """Signed, about a sixth exactly 0, magnitude 10^U(-3, 3)."""
    w = 10.0 ** rng.uniform(-3.0, 3.0, C) * rng.choice([-1.0, 1.0], C)
    return np.where(rng.random(C) < 1.0 / 6.0, 0.0, w).astype(np.float32)


def _tap(rng, C, P, zero_pixels=True):
    fx, fy, w = _features(rng, C, P), _features(rng, C, P), _weights(rng, C)
    if zero_pixels and P >= 3:       # an all-zero pixel in x only, in y only, in both
        fx[:, 0] = 0
        fy[:, 1] = 0
        fx[:, 2] = 0
        fy[:, 2] = 0
    return fx, fy, w


SHAPES = [(1, 1), (3, 63), (3, 64), (3, 65), (64, 368), (192, 77), (384, 15), (256, 15), (512, 5), (64, 4099)]
STRIDED = (64, 77)                   # (C, P) of the taps that are sliced views on the device
# name -> channel strides of (fx, fy), None = contiguous: the two sides' strides are independent of one another
STRIDES = {"strided": (100, 100), "strided_x_only": (100, None), "strided_both_differently": (83, 100)}
MULTI = [(64, 368), (192, 77), (7, 1)]

_CASES = None


def cases():
    """name -> {"taps": [(fx, fy, w)], "g": upstream gradient, "stride": channel strides (fx, fy) of tap 0 or None}.  Built once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = {}
    for i, (C, P) in enumerate(SHAPES):
        rng = np.random.default_rng(1000 + i)
        out[f"c{C}_p{P}"] = {"taps": [_tap(rng, C, P)], "g": 0.5, "stride": None}
    for i, (name, strides) in enumerate(STRIDES.items()):
        rng = np.random.default_rng(2000 + 10 * i)
        out[name] = {"taps": [_tap(rng, *STRIDED)], "g": 0.5, "stride": strides}
    rng = np.random.default_rng(2001)
    out["multi"] = {"taps": [_tap(rng, C, P) for C, P in MULTI], "g": -3.0, "stride": None}
    # y == x: value and gradients exactly 0
    for name, shapes in (("same_c3_p65", [(3, 65)]), ("same_c192_p77", [(192, 77)]), ("same_multi", MULTI)):
        rng = np.random.default_rng(3000 + len(out))
        taps = []
        for C, P in shapes:
            fx, _fy, w = _tap(rng, C, P)
            taps.append((fx, fx.copy(), w))
        out[name] = {"taps": taps, "g": 0.5, "stride": None}
    # y close to x: where training spends its time, and where an expanded form would cancel
    rng = np.random.default_rng(4000)
    fx, _fy, w = _tap(rng, 64, 368)
    fy = (fx * (1.0 + 1e-4 * rng.standard_normal(fx.shape))).astype(np.float32)
    fy = np.where(fy > 0, np.clip(fy, 1e-3, 1e3), 0.0).astype(np.float32)
    fy[:, 0] = _features(rng, 64, 1)[:, 0]          # (pixel 0 stays zero in x only)
    fy[:, 1] = 0
    out["close_c64_p368"] = {"taps": [(fx, fy, w)], "g": 0.5, "stride": None}
    # single magnitudes: every entry 1e-3, every entry 1e3
    for name, mag in (("tiny_c64_p77", 1e-3), ("huge_c64_p77", 1e3)):
        rng = np.random.default_rng(5000 + len(out))
        fx, fy, w = _tap(rng, 64, 77)
        fx, fy = (np.where(fx > 0, mag, 0.0).astype(np.float32), np.where(fy > 0, mag, 0.0).astype(np.float32))
        out[name] = {"taps": [(fx, fy, w)], "g": 0.5, "stride": None}
    _CASES = out
    return out


def replay_constants():
    """(k_fwd, k_bwd): the largest error of the float32 replay against float64 over all cases, in bar units."""
    k_fwd = k_bwd = 0.0
    for case in cases().values():
        taps, g = case["taps"], case["g"]
        d64, _t = head_fwd(taps)
        d32, _t = head_fwd(taps, np.float32)
        for e, u in zip(np.abs(d32.astype(np.float64) - d64), fwd_units(taps)):
            if u > 0:
                k_fwd = max(k_fwd, e / (EPS * u))
            else:
                assert e == 0
        g64, g32, units = head_bwd(taps, g), head_bwd(taps, g, np.float32), bwd_units(taps, g)
        for pair64, pair32, pairu in zip(g64, g32, units):
            for v64, v32, u in zip(pair64, pair32, pairu):
                err = np.abs(v32.astype(np.float64) - v64)
                assert np.all(np.isfinite(v32)) and np.all(err[u == 0] == 0)
                if np.any(u > 0):
                    k_bwd = max(k_bwd, float(np.max(err[u > 0] / (EPS * u[u > 0]))))
    return k_fwd, k_bwd


# ---- the criterion: a stand-in for the reference's module, and the plain-torch statement of its call -------------------
ALEX_FEATURES = [("conv", 3, 64, 11, 4, 2), ("relu",), ("pool", 3, 2), ("conv", 64, 192, 5, 1, 2), ("relu",), ("pool", 3, 2),
                 ("conv", 192, 384, 3, 1, 1), ("relu",), ("conv", 384, 256, 3, 1, 1), ("relu",),
                 ("conv", 256, 256, 3, 1, 1), ("relu",), ("pool", 3, 2)]
ALEX_TAPS, ALEX_CHANNELS = [2, 5, 8, 10, 12], [64, 192, 384, 256, 256]
VGG_TAPS, VGG_CHANNELS = [4, 9, 16, 23, 30], [64, 128, 256, 512, 512]


def vgg_features():
    rows, cin = [], 3
    for width, convs in ((64, 2), (128, 2), (256, 3), (512, 3), (512, 3)):
        for _ in range(convs):
            rows += [("conv", cin, width, 3, 1, 1), ("relu",)]
            cin = width
        rows.append(("pool", 2, 2))
    return rows


def standin(net_type="alex", seed=0, zero_bias=False, mean=(-0.030, -0.088, -0.188), std=(0.458, 0.448, 0.450)):
    """A module with the attribute names of the reference's LPIPS criterion (.net.layers / .target_layers / .mean / .std,
    .lin[i][1].weight), built from torch.nn alone with random weights in the layer shapes of AlexNet or VGG16."""
    import torch
    import torch.nn as nn
    rows, taps, channels = ((ALEX_FEATURES, ALEX_TAPS, ALEX_CHANNELS) if net_type == "alex"
                            else (vgg_features(), VGG_TAPS, VGG_CHANNELS))
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        layers = []
        for row in rows:
            if row[0] == "conv":
                layers.append(nn.Conv2d(row[1], row[2], row[3], row[4], row[5]))
            elif row[0] == "relu":
                layers.append(nn.ReLU(inplace=True))
            else:
                layers.append(nn.MaxPool2d(row[1], row[2]))
        net = nn.Module()
        net.layers = nn.Sequential(*layers)
        net.target_layers = list(taps)
        net.n_channels_list = list(channels)
        net.register_buffer("mean", torch.tensor(mean)[None, :, None, None])
        net.register_buffer("std", torch.tensor(std)[None, :, None, None])
        crit = nn.Module()
        crit.net = net
        crit.lin = nn.ModuleList()
        for c in channels:               # what from_reference reads is lin[i][1].weight, [1,C,1,1]
            weighting = nn.Conv2d(in_channels=c, out_channels=1, kernel_size=1, bias=False)
            weighting.weight.data.uniform_(0.0, 1.0)
            pair = nn.Sequential()
            pair.add_module("0", nn.Identity())
            pair.add_module("1", weighting)
            crit.lin.append(pair)
        if zero_bias:
            for m in net.layers:
                if isinstance(m, nn.Conv2d):
                    m.bias.data.zero_()
    for p in crit.parameters():
        p.requires_grad_(False)
    return crit


def plain_taps(crit, x):
    """The stand-in's raw taps of a [1,3,H,W] input: the z-scored input goes through the layers up to the last tap
    position; the output of every layer whose position (counted from 1) is a tap position is kept."""
    wanted = sorted(int(t) for t in crit.net.target_layers)
    z = (x - crit.net.mean) / crit.net.std
    kept = {}
    for index, layer in enumerate(list(crit.net.layers)[:wanted[-1]]):
        z = layer(z)
        if index + 1 in wanted:
            kept[index + 1] = z
    return [kept[t] for t in wanted]


def plain_distance(feats_x, feats_y, lin_weights):
    """The head in plain torch, in the dtype of its inputs: what autograd differentiates (NaN at an all-zero pixel)."""
    import torch
    total = 0
    for fx, fy, w in zip(feats_x, feats_y, lin_weights):
        a = fx / (torch.sqrt(torch.sum(fx ** 2, dim=1, keepdim=True)) + 1e-10)
        b = fy / (torch.sqrt(torch.sum(fy ** 2, dim=1, keepdim=True)) + 1e-10)
        total = total + (w.reshape(1, -1, 1, 1) * (a - b) ** 2).sum(dim=1, keepdim=True).mean(dim=(2, 3), keepdim=True)
    return total


def plain_lpips(crit, image, gt, mask=None):
    """The reference's call lpips(image * mask, gt * mask) restated in plain torch over the stand-in -> [1,1,1,1]."""
    if mask is not None:
        image, gt = image * mask, gt * mask
    lin = [l[1].weight for l in crit.lin]
    return plain_distance(plain_taps(crit, image[None]), plain_taps(crit, gt[None]), lin)
