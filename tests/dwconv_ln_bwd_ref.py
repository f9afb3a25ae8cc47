"""The backward of depthwise 7x7 (pad 3) + bias + LayerNorm over C restated in fp64, the case table of its tests, and the two
autograd runs (fp64 = the oracle, fp32 = the yardstick of the bar) over the repository's fallback graph.  CPU only.

    forward   u = b + sum_tap w x(shifted)    mu, var over c (biased)    r = 1 / sqrt(var + eps)    xh = (u - mu) r    y = gamma xh + beta
    backward  dbeta = sum_pix g    dgamma = sum_pix g xh    gh = g gamma    du = r (gh - mean_c(gh) - xh mean_c(gh xh))    db = sum_pix du
              dw[c,ky,kx] = sum_pix du[p] x[p + (ky-3, kx-3)]               dx[p] = sum_tap w[c,ky,kx] du[p - (ky-3, kx-3)]
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-6
NAMES = ("dx", "dw", "db", "dgamma", "dbeta")

# (N, H, W, C): the smallest shapes at which each mechanism of csrc/dwconv_ln_bwd.hip can go wrong.  A thread holds a channel quad
# of 4 (passes A, dx) or 8 (pass dw) pixels of one image row; a workgroup holds 256 / (C / 4) such tiles; at most 512 (pass A) and 64
# (pass dw, per kernel row) workgroups walk the tile groups.
CASES = (
    (1, 1, 1, 4),        # one quad; every tap but the centre is padding
    (3, 3, 5, 8),        # image smaller than the kernel; N = 3; two lanes per pixel (shuffle sums)
    (2, 7, 7, 16),       # 7 x 7; four lanes per pixel
    (3, 5, 13, 32),      # W no multiple of 4 or 8; eight lanes per pixel
    (1, 9, 10, 64),      # 16 lanes per pixel (one DPP row)
    (1, 7, 7, 128),      # half a wave per pixel
    (1, 5, 13, 128),
    (1, 16, 16, 256),    # one wave per pixel; several workgroups
    (1, 7, 7, 512),      # a pixel spans two waves: sums through LDS
    (1, 3, 5, 1024),     # 256 quads: a pixel is the whole workgroup
    (3, 1, 1, 1024),
    (3, 9, 10, 4),       # 64 tiles per workgroup, most of the last group idle
    (3, 76, 76, 128),    # 542 tile groups > 512 slots (pass A), 285 > 64 (pass dw): workgroups walk several tiles and images
)
PERSISTENT_CASE = CASES[-1]


def case_id(case):
    return "n%d_%dx%d_c%d" % case


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """Seeded O(1) fp32 inputs of a case: x, g (N,C,H,W) channels_last; weight [C,1,7,7]; bias, gamma, beta [C].  Do not modify."""
    n, h, w, c = case
    gen = torch.Generator().manual_seed(1000 * c + 100 * n + 10 * h + w)

    def rnd(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=gen, dtype=torch.float32) * scale + shift

    x = rnd(n, c, h, w).contiguous(memory_format=torch.channels_last)
    g = rnd(n, c, h, w).contiguous(memory_format=torch.channels_last)
    return dict(x=x, g=g, weight=rnd(c, 1, 7, 7, scale=1.0 / 7.0), bias=rnd(c, scale=0.5), gamma=rnd(c, scale=0.5, shift=1.0), beta=rnd(c, scale=0.5))


def restated_backward(x, weight, bias, gamma, beta, g, eps=EPS):
    """The formulas above in fp64, tap by tap, without autograd -> dict of y, du (N,C,H,W) and the five gradients (``NAMES``)."""
    x, weight, bias, gamma, beta, g = (t.detach().double().contiguous() for t in (x, weight, bias, gamma, beta, g))
    n, c, h, w = x.shape
    xp = F.pad(x, (3, 3, 3, 3))
    u = bias.view(1, c, 1, 1).expand(n, c, h, w).clone()
    for ky in range(7):
        for kx in range(7):
            u += weight[:, 0, ky, kx].view(1, c, 1, 1) * xp[:, :, ky:ky + h, kx:kx + w]
    mu = u.mean(1, keepdim=True)
    var = ((u - mu) ** 2).mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xh = (u - mu) * r
    y = gamma.view(1, c, 1, 1) * xh + beta.view(1, c, 1, 1)
    gh = g * gamma.view(1, c, 1, 1)
    du = r * (gh - gh.mean(1, keepdim=True) - xh * (gh * xh).mean(1, keepdim=True))
    dup = F.pad(du, (3, 3, 3, 3))
    dw = torch.zeros(c, 1, 7, 7, dtype=torch.float64)
    dx = torch.zeros_like(x)
    for ky in range(7):
        for kx in range(7):
            dw[:, 0, ky, kx] = (du * xp[:, :, ky:ky + h, kx:kx + w]).sum((0, 2, 3))
            # dx[p] += w du[p - (ky-3, kx-3)]: the padded du read at offset (6 - ky, 6 - kx)
            dx += weight[:, 0, ky, kx].view(1, c, 1, 1) * dup[:, :, 6 - ky:6 - ky + h, 6 - kx:6 - kx + w]
    return dict(y=y, du=du, dx=dx, dw=dw, db=du.sum((0, 2, 3)), dgamma=(g * xh).sum((0, 2, 3)), dbeta=g.sum((0, 2, 3)))


def autograd_backward(x, weight, bias, gamma, beta, g, dtype, eps=EPS):
    """The repository's fallback graph (``hip_layers.dwconv_ln`` without its kernels: Conv2d(C, C, 7, padding=3, groups=C), then
    F.layer_norm over the NHWC view) under torch.autograd on the CPU in ``dtype`` -> dict of y and the five gradients."""
    x, weight, bias, gamma, beta = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, weight, bias, gamma, beta))
    c = x.shape[1]
    u = F.conv2d(x, weight, bias, stride=1, padding=3, dilation=1, groups=c)     # what the module's forward calls
    y = F.layer_norm(u.permute(0, 2, 3, 1), (c,), gamma, beta, eps).permute(0, 3, 1, 2)
    grads = torch.autograd.grad(y, (x, weight, bias, gamma, beta), g.detach().to(dtype))
    return dict(y=y.detach(), **dict(zip(NAMES, grads)))


@functools.lru_cache(maxsize=None)
def references(case):
    """(fp64 autograd, fp32 autograd) of a case on the CPU, computed once per process.  Do not modify."""
    t = make_inputs(case)
    args = (t["x"], t["weight"], t["bias"], t["gamma"], t["beta"], t["g"])
    return autograd_backward(*args, torch.float64), autograd_backward(*args, torch.float32)


def bar(ref64, ref32):
    """2 max|fp32 - ref64| + 1 ulp (fp32) of max|ref64|."""
    ref64 = ref64.double()
    top = float(ref64.abs().max())
    return 2.0 * float((ref32.double() - ref64).abs().max()) + float(np.spacing(np.float32(top)))


def ratio_to_bar(got, ref64, ref32):
    """max|got - ref64| over the bar: at most 1 passes."""
    return float((got.detach().double().cpu().reshape(ref64.shape) - ref64.double()).abs().max()) / bar(ref64, ref32)
