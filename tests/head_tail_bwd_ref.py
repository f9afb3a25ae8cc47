"""The geometry head's tail written on torch operators, its backward restated by hand, and the case tables of its tests.  CPU only; the
dtype is an argument: fp64 autograd is the oracle, fp32 autograd the yardstick of the bar (tests/mlp_bwd_ref.py: ``bar``).

    forward   out[b] = feat[b] W[sel[b]]^T + bias[sel[b]]        feat [B,hw,K], W [C,n,K] = weight[cls_rows], out [B,hw,n]
              channels of out: [vis | full (double mask) | x | y | z | region 0..64], kx = the first xyz channel, kr = kx + 3
              p = softmax(out[kr + 1 :])        pnp_in = [(xyz - 0.5) extent | coord2d | p]        planes = out[: kr] per channel
    backward  d_out[k < kx] = g_planes[k]        d_out[kx + c] = g_planes[kx + c] + g_pnp_in[c] extent[c]        d_out[kr] = 0
              d_out[kr + j] = p_j (g_pnp_in[4 + j] - sum_i p_i g_pnp_in[4 + i]),  j = 1..64;        everything + g_out
              dfeat[b] = d_out[b] W[sel[b]]        dW[cls_rows[c]] = sum_{b: sel[b] = c} d_out[b]^T feat[b]        db likewise, column sums
The reference's own form (GDRN_double_mask.py:107-160, conv_pnp_net.py:120-134) is the full-width layer followed by the class gather;
``tail_forward(full_width=True)`` holds those lines, and tests/test_head_tail_bwd_cpu.py ties the sliced form to them.
"""
import functools

import torch
import torch.nn.functional as F

N_REGIONS = 64


def class_rows(n_classes, double_mask):
    """heads.class_channel_index for one channel per mask: the rows of the full-width layer that class c keeps, i64[C, n]."""
    C, n_masks, R = n_classes, 2 if double_mask else 1, N_REGIONS + 1
    rows = []
    for c in range(C):
        r = [blk * C + c for blk in range(n_masks)]
        r += [n_masks * C + k * C + c for k in range(3)]
        r += [n_masks * C + 3 * C + c * R + j for j in range(R)]
        rows.append(r)
    return torch.tensor(rows, dtype=torch.long)


def tail_forward(feat, weight, bias, cls_rows, sel, coord2d, extents, double_mask, full_width=False):
    """feat [B,hw,K], weight [out_ch,K], bias [out_ch], sel i64[B], coord2d [B,2,hw], extents [B,3] -> (out [B,hw,n], pnp_in [B,hw,69],
    planes [P,B,hw]) in the dtype of ``feat``."""
    B, hw, _ = feat.shape
    C = cls_rows.shape[0]
    kx = 2 if double_mask else 1
    if full_width:
        # the reference: every class's maps, then t.view(bs, C, k, h, w)[arange(bs), roi_classes] block by block
        full = (feat @ weight.t() + bias).transpose(1, 2)                       # [B, out_ch, hw]
        ar = torch.arange(B)
        mask_dim = kx * C
        vis = full[:, :C].reshape(B, C, 1, hw)[ar, sel]
        fullm = full[:, C:mask_dim].reshape(B, C, 1, hw)[ar, sel] if double_mask else None
        xyz = full[:, mask_dim:mask_dim + 3 * C].reshape(B, 3, C, hw)
        cx, cy, cz = (xyz[:, k].reshape(B, C, 1, hw)[ar, sel] for k in range(3))
        region = full[:, mask_dim + 3 * C:].reshape(B, C, N_REGIONS + 1, hw)[ar, sel]
        out = torch.cat([vis] + ([fullm] if double_mask else []) + [cx, cy, cz, region], dim=1).transpose(1, 2)
    else:
        w, b = weight[cls_rows], bias[cls_rows]                                   # [C,n,K], [C,n]
        out = torch.baddbmm(b[sel].unsqueeze(1), feat, w[sel].transpose(1, 2))  # [B,hw,n]
    kr = kx + 3
    region_softmax = F.softmax(out[..., kr + 1:], dim=-1)                      # channel 0 of the region block is the background
    coor = (out[..., kx:kr] - 0.5) * extents.view(B, 1, 3)
    pnp_in = torch.cat([coor, coord2d.transpose(1, 2), region_softmax], dim=-1)
    planes = out[..., :kr].permute(2, 0, 1)
    return out, pnp_in, planes


def restated_tail_backward(out, extents, double_mask, g_pnp=None, g_planes=None, g_out=None):
    """d_out [B,hw,n] in fp64 by the formulas above.  g_pnp [B,hw,69+] (channels 3, 4 and 69.. ignored), g_planes [P,B,hw],
    g_out [B,hw,n]; each may be None."""
    out = out.detach().double()
    B, hw, n = out.shape
    kx = 2 if double_mask else 1
    kr = kx + 3
    d = torch.zeros_like(out)
    if g_planes is not None:
        d[..., :kr] += g_planes.double().permute(1, 2, 0)
    if g_pnp is not None:
        g = g_pnp.double()
        d[..., kx:kr] += g[..., :3] * extents.double().view(B, 1, 3)
        p = torch.softmax(out[..., kr + 1:], dim=-1)
        gr = g[..., 5:5 + N_REGIONS]
        d[..., kr + 1:] += p * (gr - (p * gr).sum(-1, keepdim=True))
    if g_out is not None:
        d += g_out.double()
    return d


def restated_dinput(d_out, w_sliced, sel):
    """dfeat [B,hw,K] = d_out[b] W[sel[b]] in fp64."""
    return d_out.double() @ w_sliced.double()[sel]


def restated_wgrad(d_out, feat, sel, cls_rows, out_rows):
    """(dW [out_rows,K], db [out_rows]) in fp64: per class the sum over its ROIs, scattered through the row table; other rows 0."""
    d_out, feat = d_out.double(), feat.double()
    dW = torch.zeros(out_rows, feat.shape[-1], dtype=torch.float64)
    db = torch.zeros(out_rows, dtype=torch.float64)
    for c in range(cls_rows.shape[0]):
        for b in (sel == c).nonzero().flatten().tolist():
            dW[cls_rows[c]] += d_out[b].t() @ feat[b]
            db[cls_rows[c]] += d_out[b].sum(0)
    return dW, db


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
# (B, hw, K, classes, double mask, selectors).  hw = 256 is one 512-row slot of the weight gradient cut short by the ROI's end, 512 a
# full one, 768 two slots with a short last one; K = 128 one column tile, 256 two; selectors with a class that has no ROI (class 1 of
# the third case), all ROIs on one class, one slice only (the class-agnostic head), and ROIs of a class apart from one another.
CASES = (
    (1, 256, 128, 1, False, (0,)),
    (2, 512, 256, 2, True, (1, 0)),
    (5, 256, 128, 3, True, (2, 0, 2, 0, 2)),
    (3, 512, 128, 3, False, (1, 1, 1)),
    (2, 768, 256, 2, True, (0, 1)),
)


def case_id(case):
    return "b%d_hw%d_k%d_c%d_%s" % (case[0], case[1], case[2], case[3], "double" if case[4] else "single")


def wgrad_slots(B, hw, K):
    """(slots per ROI, rows per slot) of the weight gradient (csrc/head_tail_bwd.hip: wgrad_plan): 512-row chunks dealt to at most 16
    slots, and no more than bring the grid to 1024 workgroups."""
    tiles = B * (K // 128)
    cap = max(1, min(16, -(-1024 // tiles)))
    chunks = -(-hw // 512)
    per = -(-chunks // cap)
    return -(-chunks // per), per * 512


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """Seeded fp32 inputs of a case.  The region rows of the weight are four times the others: their logits have a standard deviation
    of 4, spread over [-8, 8] and beyond, so the softmax saturates in some pixels (a probability above 0.999, the others near 0).
    Do not modify."""
    B, hw, K, C, double, sel = case
    gen = torch.Generator().manual_seed(1009 * K + 31 * hw + 7 * B + C + int(double))
    rows = class_rows(C, double)
    n = rows.shape[1]
    out_ch = C * n
    kx = 2 if double else 1

    def rnd(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen, dtype=torch.float32) * scale

    weight, bias = rnd(out_ch, K, scale=K ** -0.5), rnd(out_ch, scale=0.5)
    region_rows = rows[:, kx + 3:].reshape(-1)
    weight[region_rows] *= 4.0
    feat = rnd(B, hw, K)
    feat[:, :8] *= 4.0          # and eight pixels per ROI four times further out
    return dict(feat=feat, weight=weight, bias=bias, cls_rows=rows, sel=torch.tensor(sel, dtype=torch.long),
                coord2d=torch.rand(B, 2, hw, generator=gen), extents=torch.rand(B, 3, generator=gen) * 0.2 + 0.05,
                g_pnp=rnd(B, hw, 96), g_planes=rnd(kx + 3, B, hw), g_out=rnd(B, hw, n), double_mask=double)


def autograd_tail(t, dtype, full_width=False):
    """The tail under torch.autograd on the CPU in ``dtype`` with the loss  sum(g_pnp pnp_in) + sum(g_planes planes) + sum(g_out out)
    -> dict of out, pnp_in, planes, d_out, dfeat, dW, db."""
    feat, weight, bias = (t[k].detach().to(dtype).clone().requires_grad_(True) for k in ("feat", "weight", "bias"))
    out, pnp_in, planes = tail_forward(feat, weight, bias, t["cls_rows"], t["sel"], t["coord2d"].to(dtype), t["extents"].to(dtype),
                                       t["double_mask"], full_width)
    loss = (pnp_in * t["g_pnp"][..., :69].to(dtype)).sum() + (planes * t["g_planes"].to(dtype)).sum() + (out * t["g_out"].to(dtype)).sum()
    d_out, dfeat, dW, db = torch.autograd.grad(loss, (out, feat, weight, bias))
    return dict(out=out.detach(), pnp_in=pnp_in.detach(), planes=planes.detach(), d_out=d_out, dfeat=dfeat, dW=dW, db=db)


@functools.lru_cache(maxsize=None)
def references(case):
    """(fp64 autograd, fp32 autograd) of a case on the CPU, computed once per process.  Do not modify."""
    t = make_inputs(case)
    return autograd_tail(t, torch.float64), autograd_tail(t, torch.float32)


# ---- exact operands of the two products -----------------------------------------------------------------------------------------------
def lattice(case, seed=0):
    """Integer operands in [-4, 4] for d_out [B,hw,n], feat [B,hw,K] and the sliced weight [C,n,K]: products at most 16, sums over at
    most 5 x 768 rows (or 72 columns) below 2^24, so any fp32 summation order is exact and the results must EQUAL the fp64 ones."""
    B, hw, K, C, double, _ = case
    n = 70 if double else 69
    gen = torch.Generator().manual_seed(3 + seed + B + hw + K)
    assert B * hw * 16 < 2 ** 24
    return (torch.randint(-4, 5, (B, hw, n), generator=gen).float(), torch.randint(-4, 5, (B, hw, K), generator=gen).float(),
            torch.randint(-4, 5, (C, n, K), generator=gen).float())


def locator(case):
    """One-hot probes that say where an element came from.  d_out row r of every ROI is one-hot at column r % n with value 1;
    feat[b, r, k] = 1 + (131 (b hw + r) + 17 k) % 509;  W[c, j, k] = 1 + (7 c + 29 j + 3 k) % 251.  Then dfeat[b, r] IS row r % n of
    W[sel[b]], and dW's row j of class c is the sum of the feat rows r = j (mod n) of the class's ROIs: exact, at most 60 terms
    below 510."""
    B, hw, K, C, double, _ = case
    n = 70 if double else 69
    r = torch.arange(hw)
    d = torch.zeros(B, hw, n)
    d[:, r, r % n] = 1.0
    rows = (torch.arange(B)[:, None] * hw + r[None, :])
    feat = (1 + (131 * rows[:, :, None] + 17 * torch.arange(K)[None, None, :]) % 509).float()
    w = (1 + (7 * torch.arange(C)[:, None, None] + 29 * torch.arange(n)[None, :, None] + 3 * torch.arange(K)[None, None, :]) % 251).float()
    return d, feat, w
