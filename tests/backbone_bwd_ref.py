"""The backward of the ConvNeXt stem and downsample layers restated in fp64, the case tables of their tests, the slot-count formulas the
workspace sizes are held against, and the two autograd runs (fp64 = the oracle, fp32 = the yardstick of the bar) over F.conv2d /
F.layer_norm.  CPU only; tensors are logical NCHW as torch holds them.

    stem        P = patches(x) [M,48], columns (ci, ky, kx), M = N H/4 W/4      u = P W^T + b      y = LN(u) = gamma xh + beta
                dbeta = colsum(g)   dgamma = colsum(g xh)   gh = g gamma   du = r (gh - mean_c(gh) - xh mean_c(gh xh))
                dW = du^T P   db = colsum(du)                                   without LayerNorm: du = g
    downsample  y = LN(x)   A = patch2x2(y) [N H/2 W/2, 4C], columns (ky, kx, ci)   Wp = W.permute(0,2,3,1) [Cout,4C]   z = A Wp^T + b
                dA = dz Wp   dWp = dz^T A   db = colsum(dz)   dy = unpatch2x2(dA)   dx, dgamma, dbeta = the LayerNorm backward of dy

The ``mutate`` arguments build deliberately wrong restatements (tests/test_backbone_bwd_cpu.py shows that the lattice and locator checks
catch them).
"""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mlp_bwd_ref import bar, ratio_to_bar  # noqa: E402,F401

EPS = 1e-6
STEM_C, STEM_K = 128, 48

# the stem kernel's row plan (csrc/backbone_bwd.hip: stem_plan): 32-pixel stages, each one fp32 chain, slots of a multiple of 256
# pixels, at most 256 of them; a slot holds dW [128][48] and three [128] sums in fp64
STEM_STAGE, STEM_CHAIN, STEM_SLOT_ROWS, STEM_SLOT_CAP, STEM_PART = 32, 32, 256, 256, 128 * 48 + 3 * 128
# (N, H, W): four pixels; 24 pixels; a pixel row of 12; the width limit; 320 pixels (two slots, the second with two stages); then M one
# step below, at and above the 32-pixel chain and the 256-pixel slot chunk — M is a multiple of 4 (W % 16 == 0), so the steps are 4
STEM_CASES = ((1, 4, 16), (3, 8, 16), (2, 12, 48), (1, 4, 1024), (5, 32, 32),
              (7, 4, 16), (8, 4, 16), (9, 4, 16), (63, 4, 16), (64, 4, 16), (65, 4, 16))
STEM_DEEP = (65, 128, 128)      # 66560 pixels: 130 slots of 512 pixels, sixteen chains each (exact checks only)

# the LayerNorm adjoint (layernorm_patch_bwd_kernel): a workgroup holds 256 / (C / 4) pixels x 4 at a time, at most 512 workgroups = slots
LN_PIX, LN_SLOT_CAP = 4, 512
# (N, H, W, C, Cout); the last: 2304 pixels of 1024 channels = 576 groups for the 512 slots, so workgroups walk a second group
DOWN_CASES = ((1, 2, 2, 128, 128), (3, 2, 6, 128, 256), (2, 8, 4, 256, 512), (1, 4, 4, 512, 1024), (1, 2, 2, 1024, 128), (5, 16, 16, 128, 256),
              (1, 48, 48, 1024, 128))
# 16 900 pixels of 1024 channels = 4225 groups: past the 4096 workgroups of the copy and LayerNorm kernels (bit checks only)
DOWN_GRID_STRIDE = (1, 130, 130, 1024, 128)


def case_id(case):
    return "x".join(str(int(v)) for v in case)


def _gen(case, salt):
    return torch.Generator().manual_seed(salt + sum((31 ** i) * int(v) for i, v in enumerate(case)) % (2 ** 31))


def stem_slots(m):
    """(slots, pixels per slot) of the stem backward for M pixels."""
    chunks = -(-m // STEM_SLOT_ROWS)
    per = -(-chunks // STEM_SLOT_CAP)
    return -(-chunks // per), per * STEM_SLOT_ROWS


def stem_workspace_bytes(n, h, w):
    return stem_slots(n * (h // 4) * (w // 4))[0] * STEM_PART * 8


def ln_patch_slots(n_pix, c):
    per = (256 // (c // 4)) * LN_PIX
    return min(-(-n_pix // per), LN_SLOT_CAP)


def ln_patch_workspace_bytes(n, h, w, c):
    return ln_patch_slots(n * h * w, c) * 2 * c * 8


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
def patches4x4(x, mutate=None):
    """x [N,3,H,W] -> P [N H/4 W/4, 48], row = output pixel, column (ci, ky, kx).  mutate "kykx": ky and kx transposed."""
    n, c, h, w = x.shape
    p = x.reshape(n, c, h // 4, 4, w // 4, 4)
    return (p.permute(0, 2, 4, 1, 5, 3) if mutate == "kykx" else p.permute(0, 2, 4, 1, 3, 5)).reshape(-1, 16 * c)


def patch2x2(t, mutate=None):
    """t [N,H,W,C] -> [N H/2 W/2, 4C], row = output pixel, column (ky, kx, ci).  mutate "order": (kx, ky, ci)."""
    n, h, w, c = t.shape
    p = t.reshape(n, h // 2, 2, w // 2, 2, c)
    return (p.permute(0, 1, 3, 4, 2, 5) if mutate == "order" else p.permute(0, 1, 3, 2, 4, 5)).reshape(-1, 4 * c)


def unpatch2x2(a, n, h, w, c):
    """The inverse of ``patch2x2``: [N H/2 W/2, 4C] -> [N,H,W,C]."""
    return a.reshape(n, h // 2, w // 2, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, c)


def rows_of(t_nchw):
    """[N,C,H,W] -> [N H W, C]"""
    return t_nchw.permute(0, 2, 3, 1).reshape(-1, t_nchw.shape[1])


# ---- the restatements -----------------------------------------------------------------------------------------------------------------
def layernorm_backward(u, gamma, g, eps=EPS, mutate=None):
    """rows u, g [M,C] -> (xh, du, dgamma, dbeta).  mutate "no_mean": the mean_c(gh) term dropped."""
    mu = u.mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(((u - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (u - mu) * r
    gh = g * gamma
    m1 = 0.0 if mutate == "no_mean" else gh.mean(1, keepdim=True)
    du = r * (gh - m1 - xh * (gh * xh).mean(1, keepdim=True))
    return xh, du, (g * xh).sum(0), g.sum(0)


def stem_restated(x, weight, bias, ln_w, ln_b, g, eps=EPS, mutate=None):
    """fp64, no autograd -> dict y [N,128,H/4,W/4], dW, db (and dln_w, dln_b with a LayerNorm).  ``ln_w`` None: no LayerNorm."""
    x, weight, bias, g = (t.detach().double() for t in (x, weight, bias, g))
    n, _, h, w = x.shape
    P = patches4x4(x, mutate)
    u = P @ weight.reshape(weight.shape[0], -1).t() + bias
    g2 = rows_of(g)
    out = {}
    if ln_w is None:
        y, du = u, g2
    else:
        xh, du, out["dln_w"], out["dln_b"] = layernorm_backward(u, ln_w.double(), g2, eps, mutate)
        y = xh * ln_w.double() + ln_b.double()
    out.update(y=y.reshape(n, h // 4, w // 4, -1).permute(0, 3, 1, 2), dW=(du.t() @ P).reshape(weight.shape), db=du.sum(0))
    return out


def down_restated(x, ln_w, ln_b, weight, bias, g, eps=EPS, mutate=None):
    """fp64, no autograd -> dict A, z [N,Cout,H/2,W/2], dA, dx [N,C,H,W], dW [Cout,C,2,2], db (and dln_w, dln_b with a LayerNorm)."""
    x, weight, bias, g = (t.detach().double() for t in (x, weight, bias, g))
    n, c, h, w = x.shape
    cout = weight.shape[0]
    xr = rows_of(x)
    y = xr if ln_w is None else layernorm_backward(xr, ln_w.double(), xr, eps)[0] * ln_w.double() + ln_b.double()
    A = patch2x2(y.reshape(n, h, w, c), mutate)
    Wp = weight.permute(0, 2, 3, 1).reshape(cout, 4 * c)
    dz = rows_of(g)
    dA = dz @ Wp
    dy = unpatch2x2(dA, n, h, w, c).reshape(-1, c)
    out = dict(A=A, z=(A @ Wp.t() + bias).reshape(n, h // 2, w // 2, cout).permute(0, 3, 1, 2), dA=dA,
               dW=(dz.t() @ A).reshape(cout, 2, 2, c).permute(0, 3, 1, 2), db=dz.sum(0))
    if ln_w is None:
        dx = dy
    else:
        _, dx, out["dln_w"], out["dln_b"] = layernorm_backward(xr, ln_w.double(), dy, eps, mutate)
    out["dx"] = dx.reshape(n, h, w, c).permute(0, 3, 1, 2)
    return out


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
STEM_NAMES = ("dW", "db", "dln_w", "dln_b")
DOWN_NAMES = ("dx", "dln_w", "dln_b", "dW", "db")


def stem_autograd(x, weight, bias, ln_w, ln_b, g, dtype, eps=EPS):
    """F.conv2d(stride 4) + F.layer_norm under autograd on the CPU in ``dtype`` -> dict y and the four gradients."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (weight, bias, ln_w, ln_b)]
    z = F.conv2d(x.to(dtype), leaves[0], leaves[1], stride=4)
    y = F.layer_norm(z.permute(0, 2, 3, 1), (z.shape[1],), leaves[2], leaves[3], eps).permute(0, 3, 1, 2)
    return dict(y=y.detach(), **dict(zip(STEM_NAMES, torch.autograd.grad(y, leaves, g.to(dtype)))))


def down_autograd(x, ln_w, ln_b, weight, bias, g, dtype, eps=EPS):
    """F.layer_norm + F.conv2d(stride 2) under autograd on the CPU in ``dtype`` -> dict z and the five gradients."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (x, ln_w, ln_b, weight, bias)]
    y = F.layer_norm(leaves[0].permute(0, 2, 3, 1), (x.shape[1],), leaves[1], leaves[2], eps).permute(0, 3, 1, 2)
    z = F.conv2d(y, leaves[3], leaves[4], stride=2)
    return dict(z=z.detach(), **dict(zip(DOWN_NAMES, torch.autograd.grad(z, leaves, g.to(dtype)))))


@functools.lru_cache(maxsize=None)
def stem_inputs(case):
    """Seeded fp32 (x [N,3,H,W] like a normalised image, weight [128,3,4,4] variance-preserving, bias, ln_w, ln_b, g).  Do not modify."""
    n, h, w = case
    gen = _gen(case, 3)

    def rnd(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=gen, dtype=torch.float32) * scale + shift

    return (rnd(n, 3, h, w), rnd(STEM_C, 3, 4, 4, scale=STEM_K ** -0.5), rnd(STEM_C, scale=0.1), rnd(STEM_C, scale=0.1, shift=1.0),
            rnd(STEM_C, scale=0.1), rnd(n, STEM_C, h // 4, w // 4))


@functools.lru_cache(maxsize=None)
def stem_references(case):
    """(fp64 autograd, fp32 autograd) of a stem case, computed once per process.  Do not modify."""
    t = stem_inputs(case)
    return stem_autograd(*t, torch.float64), stem_autograd(*t, torch.float32)


@functools.lru_cache(maxsize=None)
def down_inputs(case):
    """Seeded fp32 (x [N,C,H,W], ln_w, ln_b, weight [Cout,C,2,2] variance-preserving, bias, g [N,Cout,H/2,W/2]).  Do not modify."""
    n, h, w, c, cout = case
    gen = _gen(case, 5)

    def rnd(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=gen, dtype=torch.float32) * scale + shift

    return (rnd(n, c, h, w, shift=0.2), rnd(c, scale=0.1, shift=1.0), rnd(c, scale=0.1), rnd(cout, c, 2, 2, scale=(4 * c) ** -0.5),
            rnd(cout, scale=0.1), rnd(n, cout, h // 2, w // 2))


@functools.lru_cache(maxsize=None)
def down_references(case):
    """(fp64 autograd, fp32 autograd) of a downsample case, computed once per process.  Do not modify."""
    t = down_inputs(case)
    return down_autograd(*t, torch.float64), down_autograd(*t, torch.float32)


# ---- exact operands -------------------------------------------------------------------------------------------------------------------
LATTICE = 8      # integers in [-8, 8]


def lattice_ok(terms, chain):
    """Every product of two lattice values is at most 64; an fp32 chain of ``chain`` of them and the whole sum of ``terms`` stay below
    2^24, so every partial sum in any order, fp32 or fp64, and the rounded result are exact."""
    return LATTICE * LATTICE * min(terms, chain) < 2 ** 24 and LATTICE * LATTICE * terms < 2 ** 24


def _ints(gen, *shape):
    return torch.randint(-LATTICE, LATTICE + 1, shape, generator=gen).float()


@functools.lru_cache(maxsize=None)
def stem_lattice(case):
    """Integer (x, g) and the int64 results (dW [128,3,4,4], db [128]) of the stem without LayerNorm.  Do not modify."""
    n, h, w = case
    gen = _gen(case, 17)
    x, g = _ints(gen, n, 3, h, w), _ints(gen, n, STEM_C, h // 4, w // 4)
    assert lattice_ok(n * (h // 4) * (w // 4), STEM_CHAIN)
    P, g2 = patches4x4(x).long(), rows_of(g).long()
    return x, g, (g2.t() @ P).reshape(STEM_C, 3, 4, 4), g2.sum(0)


def stem_coded_x(case):
    """x whose every element is its own flat index + 1: a dW element that equals it names (n, ci, y, x)."""
    n, h, w = case
    assert n * 3 * h * w < 2 ** 24
    return (torch.arange(n * 3 * h * w, dtype=torch.float32) + 1).reshape(n, 3, h, w)


def stem_probes(case):
    """(pixel, channel) of the one-hot probes: the first and last pixel, and those on either side of a wave's 8 pixels, of a 32-pixel
    stage (= chain), of 128 pixels and of the 256-pixel slot chunk that the case has; channels on either side of a wave's 32 rows."""
    n, h, w = case
    m = n * (h // 4) * (w // 4)
    pix = sorted({p for p in (0, 7, 8, 31, 32, 127, 128, 255, 256, m // 2, m - 1) if p < m})
    chans = (0, 31, 32, 63, 64, 97, 127)
    return [(p, chans[i % len(chans)]) for i, p in enumerate(pix)]


def stem_onehot(case, probe):
    n, h, w = case
    p, co = probe
    g = torch.zeros(n * (h // 4) * (w // 4), STEM_C)
    g[p, co] = 1.0
    return g.reshape(n, h // 4, w // 4, STEM_C).permute(0, 3, 1, 2).contiguous()


def stem_probe_patch(case, x, probe):
    """The [3,4,4] patch of x behind pixel ``probe[0]``, said directly."""
    n, h, w = case
    ow = w // 4
    row, ox = divmod(probe[0], ow)
    b, oy = divmod(row, h // 4)
    return x[b, :, 4 * oy:4 * oy + 4, 4 * ox:4 * ox + 4]


@functools.lru_cache(maxsize=None)
def down_lattice(case):
    """Integer (x, weight, g) of a downsample case without LayerNorm and the fp64 restatement's results (exact: ``lattice_ok``)."""
    n, h, w, c, cout = case
    gen = _gen(case, 19)
    x, weight, g = _ints(gen, n, c, h, w), _ints(gen, cout, c, 2, 2), _ints(gen, n, cout, h // 2, w // 2)
    assert lattice_ok(n * (h // 2) * (w // 2), 128) and lattice_ok(cout, 128) and lattice_ok(4 * c, 128)
    return x, weight, g, down_restated(x, None, None, weight, torch.zeros(cout), g)


def down_coded_x(case):
    """x [N,C,H,W] whose element (n, ci, y, x) is ((n H + y) W + x) C + ci + 1: its NHWC flat index + 1."""
    n, h, w, c, _ = case
    assert n * h * w * c < 2 ** 24
    return (torch.arange(n * h * w * c, dtype=torch.float32) + 1).reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
