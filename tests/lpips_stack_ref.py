"""Float64 references and error bars for the stages of the HIP convolution stack (street_crafter_amd/lpips_stack.py,
csrc/lpips_stack.hip), shared by test_lpips_stack_cpu.py and test_lpips_stack_gpu.py.  Everything runs on the CPU.

The bars.  The kernels evaluate a sum of K products in float32 with ONE rounding per product-sum (an fmaf chain, in some
order; rows the kernel fills with zeros add exact zeros), then at most two more rounded operations (the bias or `add`).
With u = 2^-24 every rounding multiplies a partial result by (1 + d), |d| <= u, so a term that passes through at most n
roundings carries a factor within [(1 - u)^n, (1 + u)^n], and |(1 + u)^n - 1| <= gamma(n) = n u / (1 - n u) (Higham,
Accuracy and Stability of Numerical Algorithms, lemma 3.1).  In ANY summation order a product passes through at most K
roundings of the chain (its own fmaf and the K - 1 after it), hence

    forward:   |hip - f64| <= gamma(K + 2)  (|b| + sum_k |x_k| |w_k|),     K  = Cin kh kw
    dgrad:     |hip - f64| <= gamma(K' + 3) (|add| + sum_k |g'_k| |w_k|),  K' = Cout kh kw,  g' = g where relu_out > 0

(the + 2 / + 3 leave room for the bias / add rounding and one more; ReLU and the mask are exact).  The sums of absolute
values come from a float64 convolution of |x| with |w|.  Float64's own error, gamma_64(K) ~ 1e-13 relative to the same
sums, is nine orders below the bars.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def conv_fwd_ref(x, w, b, stride, padding, relu=True):
    """x [Cin,h,w], w [Cout,Cin,kh,kw], b [Cout] or None (float32, any device) -> (y, bar, pre) in float64 on the CPU."""
    x64, w64 = x.detach().cpu().double(), w.detach().cpu().double()
    b64 = None if b is None else b.detach().cpu().double()
    pre = F.conv2d(x64[None], w64, b64, stride, padding)[0]
    mag = F.conv2d(x64.abs()[None], w64.abs(), None if b64 is None else b64.abs(), stride, padding)[0]
    K = int(w.shape[1] * w.shape[2] * w.shape[3])
    return (pre.clamp_min(0) if relu else pre), gamma(K + 2) * mag, pre


def conv_dgrad_ref(g, relu_out, w, stride, padding, in_hw, add=None):
    """g, relu_out [Cout,oh,ow], w [Cout,Cin,kh,kw], add [Cin,h,w] or None -> (grad_in, bar) in float64 on the CPU."""
    g64, w64 = g.detach().cpu().double(), w.detach().cpu().double()
    if relu_out is not None:
        g64 = torch.where(relu_out.detach().cpu() > 0, g64, torch.zeros_like(g64))
    kh, kw = int(w.shape[2]), int(w.shape[3])
    op = tuple(in_hw[d] - ((g64.shape[1 + d] - 1) * stride[d] - 2 * padding[d] + (kh, kw)[d]) for d in range(2))
    gi = F.conv_transpose2d(g64[None], w64, None, stride, padding, op)[0]
    mag = F.conv_transpose2d(g64.abs()[None], w64.abs(), None, stride, padding, op)[0]
    if add is not None:
        a64 = add.detach().cpu().double()
        gi, mag = gi + a64, mag + a64.abs()
    K = int(w.shape[0] * kh * kw)
    return gi, gamma(K + 3) * mag


def within(got, want64, bar):
    """-> (ok, worst error in bar units, index of the worst element); an element with bar 0 must be exact."""
    err = (got.detach().cpu().double() - want64).abs()
    if not bool(torch.isfinite(got).all()):
        return False, float("inf"), None
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                         torch.zeros_like(err)))
    if ratio.numel() == 0:
        return True, 0.0, None
    worst = int(ratio.argmax())
    return bool((ratio <= 1.0).all()), float(ratio.reshape(-1)[worst]), worst


# ---- inputs on which no route can take another ReLU or arg-max decision ------------------------------------------------
# Two routes that round differently may decide a ReLU or a pooling window differently where the float64 values are closer
# than the bars; such a flip moves the image gradient by far more than rounding does and would drown the comparison of
# the routes.  With random weights about 1 pre-activation in 1000 and 1 window in 200 is that close (the bars are worst
# cases), so no seed of the whole network avoids them.  condition() therefore draws, per output channel, small relative
# perturbations of that channel's weights and bias (seeded, on the CPU, judged on the float64 evaluation alone) until
#   (a) no pre-activation of the channel lies within its forward bar of zero, and
#   (b) in every window of the max-pool behind it the two largest positive entries differ by more than the sum of their
#       bars,
# for every image it is given; violations() counts what is left and the tests assert that it is nothing.
def _prepared64(crit, image, mask):
    x = image.detach().cpu().double()
    if mask is not None:
        x = x * mask.detach().cpu().double()
    return (x[None] - crit.net.mean.detach().cpu().double()) / crit.net.std.detach().cpu().double()


def _channel_flags(pre, bar, pool):
    """pre, bar [B,C,h,w] float64 -> (bool [C]: a pre-activation within its bar of zero, bool [C]: a window too close)."""
    B, C = pre.shape[:2]
    relu_bad = (pre.abs() <= bar).permute(1, 0, 2, 3).reshape(C, -1).any(dim=1)
    pool_bad = torch.zeros(C, dtype=torch.bool)
    if pool is not None and pre.shape[2] >= pool[0][0] and pre.shape[3] >= pool[0][1]:
        k, s = pool
        v = F.unfold(pre.clamp_min(0).reshape(B * C, 1, *pre.shape[2:]), k, stride=s)
        b = F.unfold(bar.reshape(B * C, 1, *bar.shape[2:]), k, stride=s)
        v, idx = v.sort(dim=1, descending=True)
        b = b.gather(1, idx)
        close = (v[:, 1] > 0) & ((v[:, 0] - v[:, 1]) <= b[:, 0] + b[:, 1])
        pool_bad = close.reshape(B, C, -1).permute(1, 0, 2).reshape(C, -1).any(dim=1)
    return relu_bad, pool_bad


def _walk(crit, images, masks, fix):
    """The float64 evaluation of every image through the stand-in's layers up to the last tap; fix=True perturbs the
    convolutions' channels (in place, float32) until (a) and (b) hold.  -> (ReLU violations, window violations) left."""
    import torch.nn as nn
    layers = list(crit.net.layers)[:max(int(t) for t in crit.net.target_layers)]
    x = torch.cat([_prepared64(crit, im, m) for im, m in zip(images, masks)])
    n_relu = n_pool = 0
    for i, layer in enumerate(layers):
        if isinstance(layer, nn.Conv2d):
            nxt = layers[i + 2] if i + 2 < len(layers) else None
            pool = None
            if isinstance(nxt, nn.MaxPool2d):
                pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
                pool = (pair(nxt.kernel_size), pair(nxt.stride))
            K = layer.weight[0].numel()
            gen = torch.Generator().manual_seed(7000 + i)
            C = layer.weight.shape[0]
            out = torch.empty(0)
            dirty = torch.arange(C)
            for attempt in range(400):
                w64, b64 = layer.weight.detach()[dirty].double(), layer.bias.detach()[dirty].double()
                pre = F.conv2d(x, w64, b64, layer.stride, layer.padding)
                bar = gamma(K + 2) * F.conv2d(x.abs(), w64.abs(), b64.abs(), layer.stride, layer.padding)
                if attempt == 0:
                    out = pre.clone()
                relu_bad, pool_bad = _channel_flags(pre, bar, pool)
                bad = relu_bad | pool_bad
                out[:, dirty[~bad]] = pre[:, ~bad]
                if not fix or not bool(bad.any()):
                    n_relu += int(relu_bad.sum())
                    n_pool += int(pool_bad.sum())
                    out[:, dirty] = pre
                    break
                dirty = dirty[bad]
                with torch.no_grad():
                    scale_w = 1.0 + 0.05 * torch.randn(layer.weight[dirty].shape, generator=gen)
                    scale_b = 1.0 + 0.05 * torch.randn(len(dirty), generator=gen)
                    layer.weight[dirty] = layer.weight[dirty] * scale_w
                    layer.bias[dirty] = layer.bias[dirty] * scale_b
            else:
                raise AssertionError(f"condition(): layer {i + 1} still has close channels after 400 draws")
            x = out
        elif isinstance(layer, nn.ReLU):
            x = x.clamp_min(0)
        else:
            x = F.max_pool2d(x, layer.kernel_size, layer.stride)
    return n_relu, n_pool


def condition(crit, images, masks):
    """Perturbs the stand-in's convolution channels in place until (a) and (b) hold for every image (float32 [3,H,W]
    with a bool [1,H,W] mask or None each)."""
    _walk(crit, images, masks, True)
    return crit


def violations(crit, images, masks):
    """(channels with a pre-activation within its bar of zero, channels with a pooling window too close), summed over
    the layers, on the float64 evaluation alone."""
    return _walk(crit, images, masks, False)


def pool_ref(x, kernel, stride):
    """F.max_pool2d on the CPU in the input's own float32."""
    return F.max_pool2d(x.detach().cpu()[None], kernel, stride)[0]


def pool_bwd_ref(g, x, kernel, stride):
    """CPU autograd of F.max_pool2d in float32."""
    xc = x.detach().cpu().clone().requires_grad_(True)
    y = F.max_pool2d(xc[None], kernel, stride)
    y.backward(g.detach().cpu()[None])
    return xc.grad
