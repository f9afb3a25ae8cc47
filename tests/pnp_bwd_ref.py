"""The backward of Patch-PnP's layers restated in torch, the case tables of its tests, and the two autograd runs (fp64 = the oracle,
fp32 = the yardstick of the bar) over F.conv2d(stride=2, padding=1) / flatten / F.linear / F.gelu.  CPU only; tensors are logical NCHW
as torch holds them.

    z = conv3x3 / stride 2 / pad 1 (x, W)                           x [N,Cin,H,W], z [N,Cout,H/2,W/2], H and W even
    wgrad    dW[co][ci][ky][kx] = sum_{n,oy,ox} dz[n,co,oy,ox] x[n,ci,2oy+ky-1,2ox+kx-1]        zero outside the image
    dinput   dx[n,ci,y,x] = sum dz[n,co,oy,ox] W[co,ci,ky,kx] over 2oy+ky-1 = y and 2ox+kx-1 = x, by the parity of (y, x):
                 y = 2i      ky = 1 reads oy = i
                 y = 2i + 1  ky = 0 reads oy = i + 1 (none for i = OH - 1: there is no output row OH), ky = 2 reads oy = i
             and the columns alike: 1 / 2 / 2 / 4 taps for (even, even) / (even, odd) / (odd, even) / (odd, odd)
    flatten  NHWC [B,HW,C] -> [B, C HW] (x.flatten(1) of the NCHW tensor) and back
    heads    rot = f W_r^T + b_r, t = f W_t^T + b_t:  df = g_r W_r + g_t W_t,  dW = g^T f,  db = colsum(g)
"""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mlp_bwd_ref import bar, ratio_to_bar  # noqa: E402,F401

# (N, H, W, Cin, pitch, Cout): one chunk, every border; the pitched first layer, 48 rows; H != W; 1280 rows = 2.5 chunks of 512 and
# chains of 128; the real first layer; two column tiles
CASES = ((1, 4, 4, 128, 128, 128), (3, 8, 8, 69, 96, 128), (2, 8, 16, 128, 128, 128), (5, 32, 32, 69, 96, 128), (2, 64, 64, 69, 96, 128),
         (1, 8, 8, 128, 128, 256))
REAL_SCALE = (2, 64, 64, 69, 96, 128)      # the case whose x has the scale of Patch-PnP's real input
FC_BATCHES = (1, 3, 8)
FC_DIMS = (8192, 1024, 256, 6)             # fc1 in, fc1 out, fc2 out, rot_dim

# the wgrad's row plan (csrc/pnp_bwd.hip: wgrad_plan, that of conv_gn_bwd.hip with Cin rounded up to 128)
WG_CHUNK, WG_SLOT_CAP, WG_GRID = 512, 64, 512


def wgrad_slots(m, cin, cout):
    tiles = 9 * (cout // 128) * (-(-cin // 128))
    cap = max(1, min(WG_SLOT_CAP, WG_GRID // tiles))
    chunks = -(-m // WG_CHUNK)
    per = -(-chunks // cap)
    return -(-chunks // per), per * WG_CHUNK


def case_id(case):
    return "x".join(str(int(v)) for v in case)


def _gen(case, salt):
    return torch.Generator().manual_seed(salt + sum((31 ** i) * int(v) for i, v in enumerate(case)) % (2 ** 31))


# ---- the four formulas ---------------------------------------------------------------------------------------------------------------
def wgrad_s2(dz, x):
    """dW [Cout,Cin,3,3] from dz [N,Cout,OH,OW] and x [N,Cin,2 OH,2 OW]: nine products over the output pixels, one per tap."""
    n, cout, oh, ow = dz.shape
    xp = F.pad(x, (1, 1, 1, 1))
    d2 = dz.permute(1, 0, 2, 3).reshape(cout, -1)
    out = torch.empty(cout, x.shape[1], 3, 3, dtype=dz.dtype)
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = d2 @ xp[:, :, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2].permute(0, 2, 3, 1).reshape(n * oh * ow, -1)
    return out


def parity_taps(p):
    """The (k, shift) of one axis for input parity ``p``: input index 2 i + p is read through tap k from output index i + shift."""
    return ((1, 0),) if p == 0 else ((0, 1), (2, 0))


def _shifted(dz, sy, sx):
    """dz[..., i + sy, j + sx] with zero where that index is OH or OW: the output row / column that does not exist."""
    out = torch.zeros_like(dz)
    oh, ow = dz.shape[2:]
    out[:, :, :oh - sy, :ow - sx] = dz[:, :, sy:, sx:]
    return out


def dinput_s2(dz, weight):
    """dx [N,Cin,2 OH,2 OW] from dz [N,Cout,OH,OW] and weight [Cout,Cin,3,3], class by class: nine taps per 2 x 2 block."""
    n, cout, oh, ow = dz.shape
    dx = torch.zeros(n, weight.shape[1], 2 * oh, 2 * ow, dtype=dz.dtype)
    for py in range(2):
        for px in range(2):
            for ky, sy in parity_taps(py):
                for kx, sx in parity_taps(px):
                    dx[:, :, py::2, px::2] += torch.einsum("nohw,oc->nchw", _shifted(dz, sy, sx), weight[:, :, ky, kx])
    return dx


def tap_table(h, w):
    """count[y][x] = the (oy, ky, ox, kx) with 2 oy + ky - 1 = y, 2 ox + kx - 1 = x, 0 <= oy < h / 2, 0 <= ox < w / 2, by brute force,
    and the largest oy / ox that reaches each row / column."""
    cnt = torch.zeros(h, w, dtype=torch.long)
    top_y, top_x = [-1] * h, [-1] * w
    for oy in range(h // 2):
        for ky in range(3):
            y = 2 * oy + ky - 1
            if not 0 <= y < h:
                continue
            top_y[y] = max(top_y[y], oy)
            for ox in range(w // 2):
                for kx in range(3):
                    x = 2 * ox + kx - 1
                    if 0 <= x < w:
                        cnt[y, x] += 1
                        top_x[x] = max(top_x[x], ox)
    return cnt, top_y, top_x


def flatten_nchw(x_nhwc):
    """[B,HW,C] -> [B, C HW]"""
    b, hw, c = x_nhwc.shape
    return x_nhwc.transpose(1, 2).reshape(b, c * hw)


def unflatten_nchw(x2d, hw, c):
    return x2d.view(x2d.shape[0], c, hw).transpose(1, 2).contiguous()


def heads_backward(g_r, g_t, feat, w_r, w_t):
    """-> (dfeat, dW_r, db_r, dW_t, db_t); a source given as None contributes nothing."""
    b, k = feat.shape
    zr, zt = torch.zeros(b, w_r.shape[0], dtype=feat.dtype), torch.zeros(b, 3, dtype=feat.dtype)
    g_r, g_t = zr if g_r is None else g_r, zt if g_t is None else g_t
    return g_r @ w_r + g_t @ w_t, g_r.t() @ feat, g_r.sum(0), g_t.t() @ feat, g_t.sum(0)


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def autograd_conv(x, weight, g, dtype):
    """F.conv2d(stride=2, padding=1) under autograd on the CPU in ``dtype`` -> dict z, dx, dW."""
    x, weight = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, weight))
    z = F.conv2d(x, weight, None, 2, 1)
    dx, dw = torch.autograd.grad(z, (x, weight), g.detach().to(dtype))
    return dict(z=z.detach(), dx=dx, dW=dw)


def autograd_heads(g_r, g_t, feat, w_r, b_r, w_t, b_t, dtype):
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (feat, w_r, b_r, w_t, b_t)]
    f, wr, br, wt, bt = leaves
    loss = (F.linear(f, wr, br) * g_r.to(dtype)).sum() + (F.linear(f, wt, bt) * g_t.to(dtype)).sum()
    return torch.autograd.grad(loss, leaves)


@functools.lru_cache(maxsize=None)
def conv_inputs(case):
    """Seeded fp32 (x [N,Cin,H,W], weight [Cout,Cin,3,3] variance-preserving, g [N,Cout,H/2,W/2]).  ``REAL_SCALE``: x as Patch-PnP's
    input is — xyz times the extent around 0.1, coordinates in [0, 1), softmax weights over the 64 regions.  Do not modify."""
    n, h, w, cin, _, cout = case
    gen = _gen(case, 11)
    if case == REAL_SCALE:
        xyz = (torch.rand(n, 3, h, w, generator=gen) - 0.5) * 0.2
        coord = torch.rand(n, 2, h, w, generator=gen)
        region = torch.softmax(torch.randn(n, 64, h, w, generator=gen) * 3.0, dim=1)
        x = torch.cat([xyz, coord, region], 1)
    else:
        x = torch.randn(n, cin, h, w, generator=gen)
    weight = torch.randn(cout, cin, 3, 3, generator=gen) * (9 * cin) ** -0.5
    g = torch.randn(n, cout, h // 2, w // 2, generator=gen)
    return x, weight, g


@functools.lru_cache(maxsize=None)
def conv_references(case):
    """(fp64 autograd, fp32 autograd) of a case on the CPU, once per process.  Do not modify."""
    x, weight, g = conv_inputs(case)
    return autograd_conv(x, weight, g, torch.float64), autograd_conv(x, weight, g, torch.float32)


@functools.lru_cache(maxsize=None)
def conv_lattice(case):
    """Integer operands in [-8, 8]: every product is at most 64 and every sum has fewer than 2^18 terms, so any order of fp32 sums is
    exact and the results must EQUAL the fp64 ones -> (x, weight, dz, dW64, dx64)."""
    n, h, w, cin, _, cout = case
    assert n * (h // 2) * (w // 2) * 64 < 2 ** 24 and 4 * cout * 64 < 2 ** 24
    gen = _gen(case, 1)
    x = torch.randint(-8, 9, (n, cin, h, w), generator=gen).float()
    weight = torch.randint(-8, 9, (cout, cin, 3, 3), generator=gen).float()
    dz = torch.randint(-8, 9, (n, cout, h // 2, w // 2), generator=gen).float()
    return x, weight, dz, wgrad_s2(dz.double(), x.double()), dinput_s2(dz.double(), weight.double())


def probe_positions(case):
    """(n, oy, ox, co) of the one-hot probes: the four corners of the last image, the last output row and column away from the corners
    (they alone reach the last — odd — input row and column), and a pixel of the first output row, whose ky = 0 taps leave the image."""
    n, h, w, _, _, cout = case
    oh, ow = h // 2, w // 2
    pos = [(0, 0), (0, ow - 1), (oh - 1, 0), (oh - 1, ow - 1), (oh - 1, ow // 2), (oh // 2, ow - 1), (0, ow // 2)]
    seen, out = set(), []
    for k, (oy, ox) in enumerate(pos):
        if (oy, ox) not in seen:
            seen.add((oy, ox))
            out.append((n - 1, oy, ox, (37 * k + 5) % cout))
    return out


def coded_x(case):
    """x[n, ci, y, x] = 1 + (131 pix + 17 ci) % 509 with pix the pixel's row n H W: an element of dW names the pixel it came from."""
    n, h, w, cin, _, _ = case
    pix = torch.arange(n * h * w)
    x2 = (1 + (131 * pix[:, None] + 17 * torch.arange(cin)[None, :]) % 509).float()
    return x2.view(n, h, w, cin).permute(0, 3, 1, 2).contiguous()


def coded_weight(case):
    """W[co, ci, ky, kx] = 1 + (131 (ky 3 + kx) + 17 ci + 7 co) % 509: an element of dx names the tap and channel it came from."""
    _, _, _, cin, _, cout = case
    co, ci, t = torch.arange(cout)[:, None, None], torch.arange(cin)[None, :, None], torch.arange(9)[None, None, :]
    return (1 + (131 * t + 17 * ci + 7 * co) % 509).float().view(cout, cin, 3, 3)


def onehot_dz(case, probe):
    n, h, w, _, _, cout = case
    dz = torch.zeros(n, cout, h // 2, w // 2)
    b, oy, ox, co = probe
    dz[b, co, oy, ox] = 1.0
    return dz


# ---- fc tail ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fc_inputs(b):
    """Seeded fp32 inputs of the fc tail at ``b`` rows: x [b,8192], variance-preserving weights, O(0.1) biases, g_r [b,6], g_t [b,3]."""
    k0, k1, k2, rd = FC_DIMS
    gen = torch.Generator().manual_seed(4409 + b)

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen) * scale

    return dict(x=rnd(b, k0), w1=rnd(k1, k0, scale=k0 ** -0.5), b1=rnd(k1, scale=0.1), w2=rnd(k2, k1, scale=k1 ** -0.5), b2=rnd(k2, scale=0.1),
                w_r=rnd(rd, k2, scale=k2 ** -0.5), b_r=rnd(rd, scale=0.1), w_t=rnd(3, k2, scale=k2 ** -0.5), b_t=rnd(3, scale=0.1),
                g_r=rnd(b, rd), g_t=rnd(b, 3))


FC_LEAVES = ("x", "w1", "b1", "w2", "b2", "w_r", "b_r", "w_t", "b_t")


def autograd_fc(t, dtype):
    """gelu(fc1) -> gelu(fc2) -> (fc_r, fc_t) under autograd on the CPU in ``dtype`` -> dict h1, h2, rot, t and d<leaf> of ``FC_LEAVES``."""
    v = {k: t[k].detach().to(dtype).clone().requires_grad_(True) for k in FC_LEAVES}
    h1 = F.gelu(F.linear(v["x"], v["w1"], v["b1"]))
    h2 = F.gelu(F.linear(h1, v["w2"], v["b2"]))
    rot, tr = F.linear(h2, v["w_r"], v["b_r"]), F.linear(h2, v["w_t"], v["b_t"])
    loss = (rot * t["g_r"].to(dtype)).sum() + (tr * t["g_t"].to(dtype)).sum()
    grads = torch.autograd.grad(loss, [v[k] for k in FC_LEAVES])
    return dict(h1=h1.detach(), h2=h2.detach(), rot=rot.detach(), t=tr.detach(), **{"d" + k: g for k, g in zip(FC_LEAVES, grads)})


@functools.lru_cache(maxsize=None)
def fc_references(b):
    t = fc_inputs(b)
    return autograd_fc(t, torch.float64), autograd_fc(t, torch.float32)


def real_scale_input(n, h, w, seed=3):
    """Patch-PnP's prepared input [n,96,h,w]: xyz times the extent around 0.1, coordinates in [0, 1), softmax weights, zero padding."""
    gen = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(n, 3, h, w, generator=gen) - 0.5) * 0.2
    coord = torch.rand(n, 2, h, w, generator=gen)
    region = torch.softmax(torch.randn(n, 64, h, w, generator=gen) * 3.0, dim=1)
    return torch.cat([xyz, coord, region, torch.zeros(n, 27, h, w)], 1)
