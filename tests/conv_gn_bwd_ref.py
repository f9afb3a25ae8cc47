"""The backward of the geometry head's layers restated in fp64, the case tables of its tests, and the two autograd runs (fp64 = the
oracle, fp32 = the yardstick of the bar) over F.conv2d / F.group_norm / F.gelu / F.interpolate(align_corners=True) /
F.conv_transpose2d.  CPU only; tensors are logical NCHW as torch holds them.

    forward   z = conv3x3(x, W) (+ b)    xhat = (z - mean) rstd    a = gamma xhat + beta    y = gelu(a) or a        m = HW C / G
    backward  dA = g gelu'(a)    dbeta = sum dA    dgamma = sum dA xhat    s1 = sum_group gamma dA    s2 = sum_group gamma dA xhat
              dz = rstd (gamma dA - (s1 + xhat s2) / m)
              dW[co][ci][ky][kx] = sum_{n,y,x} dz[n,co,y,x] x[n,ci,y+ky-1,x+kx-1]      dx = conv3x3(dz, W'),  W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx]
    bilinear  y[oy, ox] = sum U_h[oy, i] U_w[ox, j] x[i, j],  src = o (in - 1) / (2 in - 1);  dx = U_h^T g U_w
    deconv    dcols[n,h,w,ky,kx,co] = dy[n,co,h s - p + ky, w s - p + kx] or 0;  dx = dcols Wmat;  dW = x^T dcols
"""
import functools
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mlp_bwd_ref import bar, gelu_grad64, ratio_to_bar  # noqa: E402,F401

# ---- wgrad: the row plan of csrc/conv_gn_bwd.hip (wgrad_plan): 512-row chunks of the N H W pixels dealt to at most
# min(64, 512 // tiles) slots, tiles = 9 (Cout / 128) (Cin / 128); fp32 chains of 128 rows, 32-row stages
WG_CHUNK, WG_SLOT_CAP, WG_GRID, WG_STAGE = 512, 64, 512, 32


def wgrad_slots(m, cin, cout):
    tiles = 9 * (cout // 128) * (cin // 128)
    cap = max(1, min(WG_SLOT_CAP, WG_GRID // tiles))
    chunks = -(-m // WG_CHUNK)
    per = -(-chunks // cap)
    return -(-chunks // per), per * WG_CHUNK


# (N, H, W, Cin, Cout): one pixel (the eight off-centre taps are zero); every pixel on a border; two output-channel tiles; 576 rows,
# the 512-row chunk ends mid image row; a chunk that spans two images; 29584 rows = 58 chunks against a cap of 56 slots: two chunks
# per slot, 29 slots, the last one with 912 of 1024 rows
WGRAD_BIG = (1, 172, 172, 128, 128)
WGRAD_EXACT = ((1, 1, 1, 128, 128), (1, 2, 3, 128, 128), (1, 16, 16, 128, 256), (1, 24, 24, 128, 128), (3, 16, 16, 256, 128), WGRAD_BIG)
WGRAD_RANDOM = ((2, 16, 16, 128, 128), (1, 32, 32, 256, 256))
# the exact convolution: (N, H, W) x (Cin, Cout)
CONV_SPATIAL = ((1, 1, 1), (1, 2, 3), (2, 5, 7), (1, 16, 16))
CONV_CHANNELS = ((128, 128), (256, 128))
CONV_RANDOM = (2, 16, 16, 256, 256)
# GroupNorm backward (N, H, W, C, G): one pixel (8 elements per group); an odd image of 15 pixels; P = 8 partials and two channel
# widths; three images; 1089 pixels: P = 64 partials, 35 slots of 32 pixels with a short last one
GN_CASES = ((1, 1, 1, 128, 16), (2, 3, 5, 128, 16), (1, 16, 16, 256, 32), (3, 16, 16, 128, 16), (1, 33, 33, 128, 16))
UP_CASES = ((1, 1, 1, 4), (1, 1, 5, 4), (1, 2, 2, 8), (2, 3, 5, 128), (1, 8, 8, 128), (1, 32, 32, 256))
# (N, H, W, Cin, Cout, k, pad, out_pad) at stride 2: the head's two forms
DECONV_CASES = ((2, 4, 4, 128, 128, 3, 1, 1), (1, 8, 8, 256, 128, 3, 1, 1), (2, 4, 4, 128, 128, 2, 0, 0), (1, 8, 8, 256, 128, 2, 0, 0))
# the restatement is checked on these (N, H, W, Cin, Cout, G, gelu)
LAYER_CASES = ((1, 1, 1, 128, 128, 16, True), (2, 3, 5, 128, 128, 16, True), (1, 6, 4, 256, 128, 16, False), (1, 16, 16, 128, 256, 32, True))


def case_id(case):
    return "x".join(str(int(v)) for v in case)


def _gen(case, salt):
    return torch.Generator().manual_seed(salt + sum((31 ** i) * int(v) for i, v in enumerate(case)) % (2 ** 31))


# ---- convolution gradients ----------------------------------------------------------------------------------------------------
def wgrad64(dz, x):
    """dW [Cout,Cin,3,3] in fp64 from dz [N,Cout,H,W] and x [N,Cin,H,W]: nine products over the pixels, one per tap."""
    dz, x = dz.double(), x.double()
    n, cout, h, w = dz.shape
    xp = F.pad(x, (1, 1, 1, 1))
    d2 = dz.permute(1, 0, 2, 3).reshape(cout, -1)
    out = torch.empty(cout, x.shape[1], 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = d2 @ xp[:, :, ky:ky + h, kx:kx + w].permute(0, 2, 3, 1).reshape(n * h * w, -1)
    return out


def flipped(weight):
    """W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx]"""
    return weight.flip(2, 3).transpose(0, 1)


def dx64(dz, weight):
    with torch.no_grad():
        return F.conv2d(dz.double(), flipped(weight.double()), padding=1)


@functools.lru_cache(maxsize=None)
def wgrad_lattice(case):
    """Integer operands in [-8, 8]: every product is at most 64 and M 64 < 2^24, so any order of fp32 sums is exact."""
    n, h, w, cin, cout = case
    assert n * h * w * 64 < 2 ** 24
    gen = _gen(case, 1)
    dz = torch.randint(-8, 9, (n, cout, h, w), generator=gen).float()
    x = torch.randint(-8, 9, (n, cin, h, w), generator=gen).float()
    return dz, x, wgrad64(dz, x)


@functools.lru_cache(maxsize=None)
def wgrad_onehot(case):
    """dz one-hot at channel pix % Cout, x[pix, ci] = 1 + (131 pix + 17 ci) % 509 (pix = the pixel's row n H W): dW[co, ci, tap] is
    the sum of x at the tap's neighbour over the pixels = co (mod Cout), so an element names the pixels that feed it."""
    n, h, w, cin, cout = case
    m = n * h * w
    pix = torch.arange(m)
    d2 = torch.zeros(m, cout)
    d2[pix, pix % cout] = 1.0
    x2 = (1 + (131 * pix[:, None] + 17 * torch.arange(cin)[None, :]) % 509).float()
    dz = d2.view(n, h, w, cout).permute(0, 3, 1, 2).contiguous()
    x = x2.view(n, h, w, cin).permute(0, 3, 1, 2).contiguous()
    want = wgrad64(dz, x)
    assert float(want.max()) < 2 ** 24
    return dz, x, want


def wgrad_report(got, want, case, limit=6):
    """Text naming the first wrong elements of a weight gradient: tap, tile, and the pixels (image, row, column, chunk, slot, stage)
    of the one-hot operand that feed the element."""
    n, h, w, cin, cout = case
    m = n * h * w
    slots, rows = wgrad_slots(m, cin, cout)
    bad = (got != want).nonzero()
    lines = [f"{len(bad)} wrong elements of {got.numel()}; {case}: M={m}, {slots} slot(s) of {rows} rows"]
    for co, ci, ky, kx in bad[:limit].tolist():
        feed = list(range(co, m, cout))[:4]
        lines.append(f"  dW[{co},{ci},{ky},{kx}] tap {3 * ky + kx} tile ({co // 128},{ci // 128}) got {float(got[co, ci, ky, kx])} want "
                     f"{float(want[co, ci, ky, kx])}; one-hot pixels " + ", ".join(
                         f"{r} (n {r // (h * w)}, y {r % (h * w) // w}, x {r % w}, chunk {r // WG_CHUNK}, slot {r // rows}, stage {(r % rows) // WG_STAGE})"
                         for r in feed))
    return "\n".join(lines)


@functools.lru_cache(maxsize=None)
def conv_random(case):
    """Seeded O(1) operands of a convolution case -> dict x, w (scaled by (9 Cin)^-0.5), dz, and the fp64 / fp32 CPU autograd results
    (z, dx, dw).  Do not modify."""
    n, h, w, cin, cout = case
    gen = _gen(case, 2)
    x = torch.randn(n, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, 3, 3, generator=gen) * (9 * cin) ** -0.5
    dz = torch.randn(n, cout, h, w, generator=gen)
    refs = []
    for dtype in (torch.float64, torch.float32):
        xa, wa = x.to(dtype).clone().requires_grad_(True), wt.to(dtype).clone().requires_grad_(True)
        z = F.conv2d(xa, wa, padding=1)
        gx, gw = torch.autograd.grad(z, (xa, wa), dz.to(dtype))
        refs.append(dict(z=z.detach(), dx=gx, dw=gw))
    return dict(x=x, w=wt, dz=dz, ref64=refs[0], ref32=refs[1])


def conv_lattice(spatial, channels):
    n, h, w = spatial
    cin, cout = channels
    assert 9 * cin * 64 < 2 ** 24
    gen = _gen((n, h, w, cin, cout), 3)
    x = torch.randint(-8, 9, (n, cin, h, w), generator=gen).float()
    wt = torch.randint(-8, 9, (cout, cin, 3, 3), generator=gen).float()
    wt[:, ::7] = 0.0
    wt[1::2, 3, 0, 2] = 8.0      # asymmetric: a flipped or transposed tap shows
    bias = torch.randint(-64, 65, (cout,), generator=gen).float()
    return x, wt, bias


# ---- GroupNorm (+ GELU) ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gn_inputs(case):
    """Seeded fp32 z, g [N,C,H,W], gamma = 1 +- 0.5, beta = +- 0.5.  Do not modify."""
    n, h, w, c, _ = case
    gen = _gen(case, 4)
    return dict(z=torch.randn(n, c, h, w, generator=gen) * 1.5 + 0.25, g=torch.randn(n, c, h, w, generator=gen),
                gamma=torch.randn(c, generator=gen) * 0.5 + 1.0, beta=torch.randn(c, generator=gen) * 0.5)


def gn_restated(z, gamma, beta, groups, eps, gelu, g):
    """The formulas above in fp64 without autograd -> dict y, dz, dgamma, dbeta."""
    z, gamma, beta, g = (t.detach().double() for t in (z, gamma, beta, g))
    n, c, h, w = z.shape
    zg = z.reshape(n, groups, -1)
    mean = zg.mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(zg.var(2, unbiased=False, keepdim=True) + eps)
    xhat = ((zg - mean) * rstd).reshape(n, c, h, w)
    ga, be = gamma.view(1, c, 1, 1), beta.view(1, c, 1, 1)
    a = ga * xhat + be
    y = 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0))) if gelu else a
    dA = g * gelu_grad64(a) if gelu else g
    m = zg.shape[2]
    s1 = (ga * dA).reshape(n, groups, -1).sum(2, keepdim=True)
    s2 = (ga * dA * xhat).reshape(n, groups, -1).sum(2, keepdim=True)
    dz = rstd * ((ga * dA).reshape(n, groups, -1) - (s1 + xhat.reshape(n, groups, -1) * s2) / m)
    return dict(y=y, dz=dz.reshape(n, c, h, w), dgamma=(dA * xhat).sum((0, 2, 3)), dbeta=dA.sum((0, 2, 3)))


def gn_autograd(z, gamma, beta, groups, eps, gelu, g, dtype):
    z, gamma, beta = (t.detach().to(dtype).clone().requires_grad_(True) for t in (z, gamma, beta))
    y = F.group_norm(z, groups, gamma, beta, eps)
    if gelu:
        y = F.gelu(y)
    grads = torch.autograd.grad(y, (z, gamma, beta), g.detach().to(dtype))
    return dict(y=y.detach(), dz=grads[0], dgamma=grads[1], dbeta=grads[2])


@functools.lru_cache(maxsize=None)
def gn_references(case, gelu, eps=1e-5):
    """(fp64 autograd, fp32 autograd) of a GroupNorm case on the CPU, computed once per process.  Do not modify."""
    t = gn_inputs(case)
    args = (t["z"], t["gamma"], t["beta"], case[4], eps, gelu, t["g"])
    return gn_autograd(*args, torch.float64), gn_autograd(*args, torch.float32)


# ---- bilinear x2 ----------------------------------------------------------------------------------------------------------------
def up_matrix64(size):
    """U f64[2 size, size] of nn.UpsamplingBilinear2d(2) (align_corners=True) along one axis."""
    out = 2 * size
    u = torch.zeros(out, size, dtype=torch.float64)
    for o in range(out):
        src = o * (size - 1) / (out - 1) if out > 1 else 0.0
        i0 = min(int(src), size - 1)
        i1 = min(i0 + 1, size - 1)
        lam = src - i0
        u[o, i0] += 1.0 - lam
        u[o, i1] += lam
    return u


def up_restated(x, g):
    """-> (y, dx) in fp64 from the interpolation matrices."""
    uh, uw = up_matrix64(x.shape[2]), up_matrix64(x.shape[3])
    y = torch.einsum("oi,ncij,pj->ncop", uh, x.double(), uw)
    dx = torch.einsum("oi,ncop,pj->ncij", uh, g.double(), uw)
    return y, dx


@functools.lru_cache(maxsize=None)
def up_references(case):
    """dict x, g and (fp64, fp32) CPU autograd (y, dx) of F.interpolate(scale 2, bilinear, align_corners=True).  Do not modify."""
    n, h, w, c = case
    gen = _gen(case, 5)
    x, g = torch.randn(n, c, h, w, generator=gen), torch.randn(n, c, 2 * h, 2 * w, generator=gen)
    refs = []
    for dtype in (torch.float64, torch.float32):
        xa = x.to(dtype).clone().requires_grad_(True)
        y = F.interpolate(xa, scale_factor=2, mode="bilinear", align_corners=True)
        refs.append(dict(y=y.detach(), dx=torch.autograd.grad(y, xa, g.to(dtype))[0]))
    return dict(x=x, g=g, ref64=refs[0], ref32=refs[1])


# ---- transposed convolution -----------------------------------------------------------------------------------------------------
def deconv_im2col64(dy, h, w, k, stride, pad):
    """dcols f64[N,h,w,k,k,Cout] from dy [N,Cout,OH,OW]: the adjoint of the col2im gather, values copied or 0."""
    n, cout, oh, ow = dy.shape
    out = torch.zeros(n, h, w, k, k, cout, dtype=torch.float64)
    d = dy.double().permute(0, 2, 3, 1)
    for ky in range(k):
        for kx in range(k):
            for i in range(h):
                oy = i * stride - pad + ky
                if not 0 <= oy < oh:
                    continue
                for j in range(w):
                    ox = j * stride - pad + kx
                    if 0 <= ox < ow:
                        out[:, i, j, ky, kx] = d[:, oy, ox]
    return out


def deconv_restated(x, weight, dy, k, pad):
    """-> (dx [N,Cin,h,w], dW [Cin,Cout,k,k]) in fp64 from the gather and the two products."""
    n, cin, h, w = x.shape
    cout = weight.shape[1]
    dcols = deconv_im2col64(dy, h, w, k, 2, pad).reshape(n * h * w, k * k * cout)
    wmat = weight.double().permute(2, 3, 1, 0).reshape(k * k * cout, cin)          # rows (ky, kx, co)
    x2 = x.double().permute(0, 2, 3, 1).reshape(n * h * w, cin)
    dx = (dcols @ wmat).reshape(n, h, w, cin).permute(0, 3, 1, 2)
    dw = (x2.t() @ dcols).reshape(cin, k, k, cout).permute(0, 3, 1, 2)
    return dx, dw


@functools.lru_cache(maxsize=None)
def deconv_references(case):
    """dict x, w [Cin,Cout,k,k] (scaled by (k k Cin / 4)^-0.5), b, dy and (fp64, fp32) CPU autograd (y, dx, dw, db).  Do not modify."""
    n, h, w, cin, cout, k, pad, op = case
    gen = _gen(case, 6)
    x = torch.randn(n, cin, h, w, generator=gen)
    wt = torch.randn(cin, cout, k, k, generator=gen) * (k * k * cin / 4) ** -0.5
    b = torch.randn(cout, generator=gen) * 0.5
    oh, ow = (h - 1) * 2 - 2 * pad + k + op, (w - 1) * 2 - 2 * pad + k + op
    dy = torch.randn(n, cout, oh, ow, generator=gen)
    refs = []
    for dtype in (torch.float64, torch.float32):
        xa, wa, ba = (t.to(dtype).clone().requires_grad_(True) for t in (x, wt, b))
        y = F.conv_transpose2d(xa, wa, ba, stride=2, padding=pad, output_padding=op)
        gx, gw, gb = torch.autograd.grad(y, (xa, wa, ba), dy.to(dtype))
        refs.append(dict(y=y.detach(), dx=gx, dw=gw, db=gb))
    return dict(x=x, w=wt, b=b, dy=dy, ref64=refs[0], ref32=refs[1])


# ---- the whole [conv3x3, GroupNorm(, GELU)] layer -------------------------------------------------------------------------------
NAMES = ("dx", "dw", "dgamma", "dbeta")


@functools.lru_cache(maxsize=None)
def layer_inputs(case):
    n, h, w, cin, cout, _, _ = case
    gen = _gen(case, 7)
    return dict(x=torch.randn(n, cin, h, w, generator=gen), w=torch.randn(cout, cin, 3, 3, generator=gen) * (9 * cin) ** -0.5,
                gamma=torch.randn(cout, generator=gen) * 0.5 + 1.0, beta=torch.randn(cout, generator=gen) * 0.5,
                g=torch.randn(n, cout, h, w, generator=gen))


def layer_restated(x, w, gamma, beta, groups, eps, gelu, g):
    with torch.no_grad():
        z = F.conv2d(x.double(), w.double(), padding=1)
    r = gn_restated(z, gamma, beta, groups, eps, gelu, g)
    return dict(y=r["y"], dx=dx64(r["dz"], w), dw=wgrad64(r["dz"], x), dgamma=r["dgamma"], dbeta=r["dbeta"])


def layer_autograd(x, w, gamma, beta, groups, eps, gelu, g, dtype):
    x, w, gamma, beta = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, w, gamma, beta))
    y = F.group_norm(F.conv2d(x, w, padding=1), groups, gamma, beta, eps)
    if gelu:
        y = F.gelu(y)
    grads = torch.autograd.grad(y, (x, w, gamma, beta), g.detach().to(dtype))
    return dict(y=y.detach(), **dict(zip(NAMES, grads)))
