"""The backward of the ConvNeXt MLP tail restated in fp64, the case tables of its tests, and the two autograd runs (fp64 = the
oracle, fp32 = the yardstick of the bar) over nn.Linear / F.gelu / addcmul.  CPU only.

    forward   pre = x W1^T + b1    h = gelu(pre)    z = h W2^T + b2    y = s + gamma (.) z                     x [M,C], pre [M,4C]
    backward  ds = g    dh = g (diag(gamma) W2)    dpre = dh (.) gelu'(pre)    db1 = colsum(dpre)    dx = dpre W1    dW1 = dpre^T x
              G = g^T h    dW2 = diag(gamma) G    sg = colsum(g)    db2 = gamma (.) sg    dgamma = rowsum(W2 (.) G) + b2 (.) sg
The last identity (z is never formed: sum_m g z = sum_m g (h W2^T + b2)) is what the layer-scale finalize of csrc/mlp_bwd.hip computes.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

NAMES = ("dx", "dw1", "db1", "dw2", "db2", "dgamma")

# (M, C): one row; fewer rows than a column-sum slot of 64 and no multiple of the 32-row staging block; a second width with five
# column-sum slots, the last one short; more rows than two 512-row chunks of the TN GEMM (three slots, the last with 6 rows).
CASES = ((1, 128), (50, 128), (257, 256), (1030, 128))

# the TN GEMM's row plan (csrc/mlp_bwd.hip: tn_plan): 512-row chunks dealt to at most 64 slots, fp32 chains of 128 rows
TN_CHUNK, TN_SLOT_CAP, TN_GRID, TN_CHAIN, TN_STAGE = 512, 64, 512, 128, 32
TN_M = (1, 2, 3, 31, 32, 33, TN_CHUNK - 1, TN_CHUNK, TN_CHUNK + 1, 2 * TN_CHUNK + 1, TN_SLOT_CAP * TN_CHUNK + 33)
TN_SHAPES = ((128, 128), (128, 512), (512, 128), (256, 1024))
TN_RANDOM = ((33, 128, 128), (513, 128, 512), (1025, 256, 1024))
PACK_SHAPES = ((128, 128), (128, 512), (512, 128))      # (N, K) of the packed (transposed) weight: W is [K, N]

# the exact forward-shaped product (gemm_rows_kernel): 128 x 128 tiles, 32-deep stages, fp32 chains of 128 — one row, a partial tile,
# a full one, one row more, three row tiles; one stage, a depth past the chain that is no multiple of it, the deepest of the tests
EXACT_M = (1, 31, 127, 128, 129, 257)
EXACT_NK = ((128, 32), (128, 288), (384, 1024))
EXACT_ONE_SLOT = (8200, 512, 288)      # (M, N, K): 65 x 4 = 260 tiles fill the grid, so the whole depth (past one chain) stays in one workgroup
ROWS_GRID = 256


def rows_slots(m, n, k):
    """(depth slots, depth per slot) of the exact forward-shaped product: K is cut, in multiples of 128, until the grid has 256 workgroups."""
    tiles = -(-m // 128) * (n // 128)
    chunks = -(-k // 128)
    want = min(chunks, max(1, -(-ROWS_GRID // tiles)))
    per = -(-chunks // want)
    return -(-chunks // per), per * 128

# the column-sum passes (colsum_kernel): at most 256 slots of at least 64 rows, a workgroup spans 4 rows x 256 columns
COL_SLOT_ROWS, COL_SLOT_CAP = 64, 256


def tn_slots(m, n1=128, n2=128):
    """(slots, rows per slot) of the TN GEMM for M rows of a [N1, N2] result: at most 64 slots, and no more than bring the grid to
    512 workgroups."""
    tiles = (n1 // 128) * (n2 // 128)
    cap = max(1, min(TN_SLOT_CAP, -(-TN_GRID // tiles)))
    chunks = -(-m // TN_CHUNK)
    per = -(-chunks // cap)
    return -(-chunks // per), per * TN_CHUNK


def col_slots(m):
    want = min(-(-m // COL_SLOT_ROWS), COL_SLOT_CAP)
    rows = -(-m // want)
    return -(-m // rows), rows


def case_id(case):
    return "m%d_c%d" % case


@functools.lru_cache(maxsize=None)
def make_inputs(case, gamma_scale=None):
    """Seeded fp32 inputs of a case: x, s (the shortcut), g [M,C]; w1 [4C,C], b1 [4C], w2 [C,4C], b2 [C], gamma [C] (O(1), or the
    constant ``gamma_scale``).  Do not modify."""
    m, c = case
    gen = torch.Generator().manual_seed(7919 * c + m)

    def rnd(*shape, scale=1.0, shift=0.0):
        return torch.randn(*shape, generator=gen, dtype=torch.float32) * scale + shift

    d = dict(x=rnd(m, c), s=rnd(m, c), g=rnd(m, c), w1=rnd(4 * c, c, scale=c ** -0.5), b1=rnd(4 * c, scale=0.5),
             w2=rnd(c, 4 * c, scale=(4 * c) ** -0.5), b2=rnd(c, scale=0.5), gamma=rnd(c, scale=0.5, shift=1.0))
    if gamma_scale is not None:
        d["gamma"] = torch.full((c,), gamma_scale, dtype=torch.float32)
    return d


def gelu_grad64(pre):
    """gelu'(x) = Phi(x) + x phi(x) in fp64."""
    pre = pre.double()
    return 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)


def restated_backward(x, s, w1, b1, w2, b2, gamma, g):
    """The formulas above in fp64 without autograd -> dict of y, pre, h, dpre and the six gradients (``NAMES``)."""
    x, s, w1, b1, w2, b2, gamma, g = (t.detach().double() for t in (x, s, w1, b1, w2, b2, gamma, g))
    pre = x @ w1.t() + b1
    h = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    y = s + gamma * (h @ w2.t() + b2)
    dh = g @ (gamma[:, None] * w2)
    dpre = dh * gelu_grad64(pre)
    G = g.t() @ h
    sg = g.sum(0)
    return dict(y=y, pre=pre, h=h, dpre=dpre, dx=dpre @ w1, dw1=dpre.t() @ x, db1=dpre.sum(0), dw2=gamma[:, None] * G, db2=gamma * sg,
                dgamma=(w2 * G).sum(1) + b2 * sg, ds=g)


def autograd_backward(x, s, w1, b1, w2, b2, gamma, g, dtype):
    """torch.addcmul(s, fc2(gelu(fc1(x))), gamma) under torch.autograd on the CPU in ``dtype`` -> dict of y, ds and the six gradients."""
    x, s, w1, b1, w2, b2, gamma = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, s, w1, b1, w2, b2, gamma))
    y = torch.addcmul(s, F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2), gamma)
    grads = torch.autograd.grad(y, (x, w1, b1, w2, b2, gamma, s), g.detach().to(dtype))
    return dict(y=y.detach(), ds=grads[6], **dict(zip(NAMES, grads[:6])))


@functools.lru_cache(maxsize=None)
def references(case, gamma_scale=None):
    """(fp64 autograd, fp32 autograd) of a case on the CPU, computed once per process.  Do not modify."""
    t = make_inputs(case, gamma_scale)
    args = (t["x"], t["s"], t["w1"], t["b1"], t["w2"], t["b2"], t["gamma"], t["g"])
    return autograd_backward(*args, torch.float64), autograd_backward(*args, torch.float32)


def bar(ref64, ref32):
    """2 max|fp32 - ref64| + 1 ulp (fp32) of max|ref64|."""
    ref64 = ref64.double()
    top = float(ref64.abs().max())
    return 2.0 * float((ref32.double() - ref64).abs().max()) + float(np.spacing(np.float32(top)))


def ratio_to_bar(got, ref64, ref32):
    """max|got - ref64| over the bar: at most 1 passes."""
    return float((got.detach().double().cpu().reshape(ref64.shape) - ref64.double()).abs().max()) / bar(ref64, ref32)


# ---- exact operands of the TN GEMM --------------------------------------------------------------------------------------------------
def tn_lattice(m, n1, n2, seed=0):
    """Integer operands in [-8, 8]: every product is at most 64 and every partial sum over at most 2^15 + 64 rows below 2^24, so
    any summation order in fp32 is exact and the result must EQUAL the fp64 product."""
    gen = torch.Generator().manual_seed(1 + seed + 31 * m + n1 + 7 * n2)
    a = torch.randint(-8, 9, (m, n1), generator=gen).float()
    b = torch.randint(-8, 9, (m, n2), generator=gen).float()
    assert m * 64 < 2 ** 24
    return a, b


def tn_onehot(m, n1, n2):
    """Row r of A is one-hot at column r % N1, B[r, k] = 1 + (131 r + 17 k) % 509: G[c, k] is the sum of B[r, k] over the rows
    r = c (mod N1) — for M <= N1 row c of G IS row c of B, so an element says which row (hence which chunk, slot and 32-row stage)
    and which tile it came from.  Exact: at most 257 terms below 510."""
    r = torch.arange(m)
    a = torch.zeros(m, n1)
    a[r, r % n1] = 1.0
    b = (1 + (131 * r[:, None] + 17 * torch.arange(n2)[None, :]) % 509).float()
    return a, b


def tn_report(got, want, m, n1, limit=6):
    """Text naming the first wrong elements of a TN product: tile, and the rows (chunk, slot, stage) that feed the element."""
    bad = (got != want).nonzero()
    slots, rows = tn_slots(m, *got.shape)
    lines = [f"{len(bad)} wrong elements of {got.numel()}; M={m}: {slots} slot(s) of {rows} rows"]
    for c, k in bad[:limit].tolist():
        feed = list(range(c, m, n1))[:4]
        lines.append(f"  G[{c},{k}] tile ({c // 128},{k // 128}) got {float(got[c, k])} want {float(want[c, k])}; one-hot rows "
                     + ", ".join(f"{r} (chunk {r // TN_CHUNK}, slot {r // rows}, stage {(r % rows) // TN_STAGE})" for r in feed))
    return "\n".join(lines)
