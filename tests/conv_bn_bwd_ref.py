"""The forward and backward of YOLOX's BaseConv (convolution, BatchNorm with batch statistics, SiLU) restated in fp64, the case tables
of its tests, and the two autograd runs (fp64 = the oracle, fp32 on the CPU = the yardstick of the bar) over F.conv2d /
F.batch_norm(training=True) / F.silu.  CPU only; tensors are logical NCHW as torch holds them.

    forward   z = conv(x, W) (+ b), k x k / stride / pad (k - 1) / 2      mean, var over the M = N OH OW values of a channel, var biased
              invstd = 1 / sqrt(var + eps)    xhat = (z - mean) invstd    a = gamma xhat + beta    y = a sigmoid(a)
              running_mean = (1 - mom) running_mean + mom mean      running_var = (1 - mom) running_var + mom var M / (M - 1)
    backward  dA = g s (1 + a (1 - s)), s = sigmoid(a)    dbeta = sum dA    dgamma = sum dA xhat
              dz = gamma invstd (dA - dbeta / M - xhat dgamma / M)
              dW[co][ci][ky][kx] = sum_{n,oy,ox} dz[n,co,oy,ox] x[n,ci,stride oy + ky - pad,stride ox + kx - pad]
              dx[n,ci,y,x] = sum dz[n,co,oy,ox] W[co,ci,ky,kx] over stride oy + ky - pad = y, stride ox + kx - pad = x

The bar is the project's (tests/mlp_bwd_ref.py): max|hip - ref64| <= 2 max|torch fp32 on the CPU - ref64| + 1 ulp of max|ref64|."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mlp_bwd_ref import bar, ratio_to_bar  # noqa: E402,F401

EPS, MOMENTUM = 1e-3, 0.03      # what YOLOX.init_yolo sets

# ---- wgrad: the row plan of csrc/conv_bn_bwd.hip (wgrad_plan): 512-row chunks of the N OH OW output pixels dealt to at most
# min(64, 512 // tiles) slots, tiles = k k ceil(Cout / 128) ceil(Cin / 128); fp32 chains of 128 rows, 32-row stages
WG_CHUNK, WG_SLOT_CAP, WG_GRID, WG_STAGE = 512, 64, 512, 32


def out_hw(h, w, ks, stride):
    pad = (ks - 1) // 2
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def wgrad_slots(m, cin, cout, ks):
    tiles = ks * ks * -(-cout // 128) * -(-cin // 128)
    cap = max(1, min(WG_SLOT_CAP, WG_GRID // tiles))
    chunks = -(-m // WG_CHUNK)
    per = -(-chunks // cap)
    return -(-chunks // per), per * WG_CHUNK


# (N, H, W, Cin, Cout, ks, stride): the smallest shape; the eight off-centre taps are zero; the Focus shape, every pixel on a border;
# an odd image, narrow both ways; both widths 4 and 8 past a 128 tile at stride 2; 576 rows, a 512-row chunk ends mid image row; a
# chunk spans two images; 33124 rows = 65 chunks against the cap of 64 slots: two chunks per slot, 33 slots, the last with 356 rows
WGRAD_LONG = (1, 182, 182, 4, 8, 1, 1)
WGRAD_EXACT = ((1, 1, 1, 4, 4, 1, 1), (1, 1, 1, 4, 4, 3, 1), (1, 2, 3, 12, 80, 3, 1), (2, 5, 7, 40, 24, 1, 1), (1, 6, 4, 132, 136, 3, 2),
               (1, 24, 24, 32, 64, 3, 1), (3, 16, 16, 160, 40, 1, 1), WGRAD_LONG)
# the stride-2 data gradient (N, H, W, Cin, Cout): the four parity classes at their smallest; narrow widths; both widths past a tile;
# depth 9 x 1280 = 11520, 90 chains
DINPUT_EXACT = ((1, 2, 2, 4, 4), (2, 4, 6, 80, 160), (1, 8, 8, 132, 136), (1, 2, 2, 640, 1280))
# random operands (N, H, W, Cin, Cout) x the four (ks, stride) forms
RANDOM_CASES = ((2, 16, 16, 80, 160), (1, 32, 32, 64, 64), (1, 4, 4, 640, 1280))
FORMS = ((1, 1), (3, 1), (1, 2), (3, 2))
# BatchNorm (N, H, W, C): M = 2; an odd image; 256 channels; three images; 1089 rows: 18 slots of 61 rows, the last with 52; the
# widest channel count
BN_CASES = ((1, 1, 2, 4), (2, 3, 5, 40), (1, 16, 16, 256), (3, 16, 16, 80), (1, 33, 33, 24), (1, 2, 2, 1280))
BN_COL_SLOT_ROWS, BN_COL_SLOTS = 64, 256
# the layer: (N, H, W, Cin, Cout) at the four forms; the restatement also on a biased convolution and the BatchNorm cases' odd sizes
LAYER_CASE = (2, 8, 8, 40, 80)
RESTATED_CASES = ((2, 8, 8, 40, 80, 1, 1, False), (2, 8, 8, 40, 80, 3, 1, True), (2, 8, 8, 40, 80, 1, 2, False), (2, 8, 8, 40, 80, 3, 2, False),
                  (1, 1, 2, 4, 4, 3, 1, False), (2, 3, 5, 12, 16, 3, 1, True))
BLOCK_CASE = (2, 8, 8, 64)


def bn_slots(m):
    want = min(-(-m // BN_COL_SLOT_ROWS), BN_COL_SLOTS)
    rows = -(-m // want)
    return -(-m // rows), rows


def case_id(case):
    return "x".join(str(int(v)) for v in case)


def _gen(case, salt):
    return torch.Generator().manual_seed(salt + sum((31 ** i) * int(v) for i, v in enumerate(case)) % (2 ** 31))


# ---- convolution gradients, restated ----------------------------------------------------------------------------------------------
def _tap_view(xp, ky, kx, oh, ow, stride):
    return xp[:, :, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride]


def conv64(x, weight, stride, bias=None):
    """z in fp64: one product per tap."""
    x, weight = x.double(), weight.double()
    ks = weight.shape[2]
    pad = (ks - 1) // 2
    oh, ow = out_hw(x.shape[2], x.shape[3], ks, stride)
    xp = F.pad(x, (pad,) * 4)
    z = torch.zeros(x.shape[0], weight.shape[0], oh, ow, dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            z += torch.einsum("nchw,oc->nohw", _tap_view(xp, ky, kx, oh, ow, stride), weight[:, :, ky, kx])
    return z if bias is None else z + bias.double().view(1, -1, 1, 1)


def wgrad64(dz, x, ks, stride):
    """dW [Cout,Cin,ks,ks] in fp64 from dz [N,Cout,OH,OW] and x [N,Cin,H,W]: one product over the output pixels per tap."""
    dz, x = dz.double(), x.double()
    pad = (ks - 1) // 2
    oh, ow = dz.shape[2:]
    xp = F.pad(x, (pad,) * 4)
    out = torch.empty(dz.shape[1], x.shape[1], ks, ks, dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            out[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", dz, _tap_view(xp, ky, kx, oh, ow, stride))
    return out


def dinput64(dz, weight, stride, hw):
    """dx [N,Cin,H,W] in fp64: every tap's product scattered to the input pixels it read."""
    dz, weight = dz.double(), weight.double()
    ks = weight.shape[2]
    pad = (ks - 1) // 2
    oh, ow = dz.shape[2:]
    dxp = torch.zeros(dz.shape[0], weight.shape[1], hw[0] + 2 * pad, hw[1] + 2 * pad, dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            _tap_view(dxp, ky, kx, oh, ow, stride).add_(torch.einsum("nohw,oc->nchw", dz, weight[:, :, ky, kx]))
    return dxp[:, :, pad:pad + hw[0], pad:pad + hw[1]].contiguous()


@functools.lru_cache(maxsize=None)
def wgrad_lattice(case):
    """Integer operands in [-8, 8]: every product is at most 64 and M 64 < 2^24, so any order of fp32 sums is exact."""
    n, h, w, cin, cout, ks, stride = case
    oh, ow = out_hw(h, w, ks, stride)
    assert n * oh * ow * 64 < 2 ** 24
    gen = _gen(case, 1)
    dz = torch.randint(-8, 9, (n, cout, oh, ow), generator=gen).float()
    x = torch.randint(-8, 9, (n, cin, h, w), generator=gen).float()
    return dz, x, wgrad64(dz, x, ks, stride)


@functools.lru_cache(maxsize=None)
def wgrad_onehot(case):
    """dz one-hot at channel pix % Cout (pix = the output pixel's row n OH OW), x[p, ci] = 1 + (131 p + 17 ci) % 509 (p = the input
    pixel's row): dW[co, ci, tap] is the sum of x at the tap's neighbour over the output pixels = co (mod Cout), so an element names
    the pixels that feed it."""
    n, h, w, cin, cout, ks, stride = case
    oh, ow = out_hw(h, w, ks, stride)
    m = n * oh * ow
    pix = torch.arange(m)
    d2 = torch.zeros(m, cout)
    d2[pix, pix % cout] = 1.0
    x2 = (1 + (131 * torch.arange(n * h * w)[:, None] + 17 * torch.arange(cin)[None, :]) % 509).float()
    dz = d2.view(n, oh, ow, cout).permute(0, 3, 1, 2).contiguous()
    x = x2.view(n, h, w, cin).permute(0, 3, 1, 2).contiguous()
    return dz, x, wgrad64(dz, x, ks, stride)


def wgrad_report(got, want, case, limit=6):
    """Text naming the first wrong elements of a weight gradient: tap, tile, and the output pixels (image, row, column, chunk, slot,
    stage) of the one-hot operand that feed the element."""
    n, h, w, cin, cout, ks, stride = case
    oh, ow = out_hw(h, w, ks, stride)
    m = n * oh * ow
    slots, rows = wgrad_slots(m, cin, cout, ks)
    bad = (got != want).nonzero()
    lines = [f"{len(bad)} wrong elements of {got.numel()}; {case}: M={m}, {slots} slot(s) of {rows} rows"]
    for co, ci, ky, kx in bad[:limit].tolist():
        feed = list(range(co, m, cout))[:4]
        lines.append(f"  dW[{co},{ci},{ky},{kx}] tap {ks * ky + kx} tile ({co // 128},{ci // 128}) got {float(got[co, ci, ky, kx])} want "
                     f"{float(want[co, ci, ky, kx])}; one-hot pixels " + ", ".join(
                         f"{r} (n {r // (oh * ow)}, y {r % (oh * ow) // ow}, x {r % ow}, chunk {r // WG_CHUNK}, slot {r // rows}, stage {(r % rows) // WG_STAGE})"
                         for r in feed))
    return "\n".join(lines)


@functools.lru_cache(maxsize=None)
def dinput_lattice(case, n_images=None):
    """Integer operands in [-8, 8] of the stride-2 data gradient: the depth 9 Cout 64 < 2^24, so any order of fp32 sums is exact.
    ``n_images``: the batch is that many images, image 0 being the case's own first image (the order of a sum must not depend on N)."""
    n, h, w, cin, cout = case
    assert 9 * cout * 64 < 2 ** 24
    gen = _gen(case, 4)
    dz = torch.randint(-8, 9, (n, cout, h // 2, w // 2), generator=gen).float()
    wt = torch.randint(-8, 9, (cout, cin, 3, 3), generator=gen).float()
    wt[:, ::7] = 0.0
    wt[1::2, 3 % cin, 0, 2] = 8.0      # asymmetric: a flipped or transposed tap shows
    if n_images is not None:
        more = torch.randint(-8, 9, (n_images - 1, cout, h // 2, w // 2), generator=gen).float()
        dz = torch.cat([dz[:1], more], 0)
    return dz, wt, dinput64(dz, wt, 2, (h, w))


@functools.lru_cache(maxsize=None)
def conv_random(case, form):
    """Seeded O(1) operands of a convolution case at a (ks, stride) form -> dict x, w (scaled by (k k Cin)^-0.5), dz, and the fp64 /
    fp32 CPU autograd results (z, dx, dw).  Do not modify."""
    n, h, w, cin, cout = case
    ks, stride = form
    gen = _gen(case + form, 2)
    oh, ow = out_hw(h, w, ks, stride)
    x = torch.randn(n, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, ks, ks, generator=gen) * (ks * ks * cin) ** -0.5
    dz = torch.randn(n, cout, oh, ow, generator=gen)
    refs = []
    for dtype in (torch.float64, torch.float32):
        xa, wa = x.to(dtype).clone().requires_grad_(True), wt.to(dtype).clone().requires_grad_(True)
        z = F.conv2d(xa, wa, stride=stride, padding=(ks - 1) // 2)
        gx, gw = torch.autograd.grad(z, (xa, wa), dz.to(dtype))
        refs.append(dict(z=z.detach(), dx=gx, dw=gw))
    return dict(x=x, w=wt, dz=dz, ref64=refs[0], ref32=refs[1])


# ---- BatchNorm with batch statistics + SiLU ---------------------------------------------------------------------------------------
BN_NAMES = ("y", "mean", "invstd", "running_mean", "running_var", "dz", "dgamma", "dbeta")


@functools.lru_cache(maxsize=None)
def bn_inputs(case):
    """Seeded inputs of a BatchNorm case: z with a per-channel offset and spread, gamma about 1, beta, the running statistics before the
    step and the gradient g.  Do not modify."""
    n, h, w, c = case
    gen = _gen(case, 5)
    z = torch.randn(n, c, h, w, generator=gen) * (0.5 + torch.rand(1, c, 1, 1, generator=gen)) + torch.randn(1, c, 1, 1, generator=gen)
    return dict(z=z, gamma=torch.randn(c, generator=gen) * 0.5 + 1.0, beta=torch.randn(c, generator=gen) * 0.5,
                running_mean=torch.randn(c, generator=gen) * 0.1, running_var=torch.rand(c, generator=gen) + 0.5,
                g=torch.randn(n, c, h, w, generator=gen))


def bn_restated(z, gamma, beta, running_mean, running_var, g, eps=EPS, momentum=MOMENTUM):
    """The formulas of the docstring in fp64 without autograd -> dict of ``BN_NAMES``."""
    z, gamma, beta, running_mean, running_var, g = (t.detach().double() for t in (z, gamma, beta, running_mean, running_var, g))
    m = z.numel() // z.shape[1]
    mean = z.mean((0, 2, 3))
    var = ((z - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(var + eps)

    def ch(v):
        return v.view(1, -1, 1, 1)

    xhat = (z - ch(mean)) * ch(invstd)
    a = ch(gamma) * xhat + ch(beta)
    s = torch.sigmoid(a)
    d_a = g * s * (1.0 + a * (1.0 - s))
    dbeta, dgamma = d_a.sum((0, 2, 3)), (d_a * xhat).sum((0, 2, 3))
    dz = ch(gamma * invstd) * (d_a - ch(dbeta) / m - xhat * ch(dgamma) / m)
    return dict(y=a * s, mean=mean, invstd=invstd, running_mean=(1 - momentum) * running_mean + momentum * mean,
                running_var=(1 - momentum) * running_var + momentum * var * m / (m - 1), dz=dz, dgamma=dgamma, dbeta=dbeta)


def bn_autograd(z, gamma, beta, running_mean, running_var, g, dtype, eps=EPS, momentum=MOMENTUM):
    """F.silu(F.batch_norm(z, training=True)) under autograd on the CPU in ``dtype`` -> dict of ``BN_NAMES``; mean and invstd are
    what the operator saves, taken from its native form."""
    z, gamma, beta = (t.detach().to(dtype).clone().requires_grad_(True) for t in (z, gamma, beta))
    rm, rv = running_mean.detach().to(dtype).clone(), running_var.detach().to(dtype).clone()
    y = F.silu(F.batch_norm(z, rm, rv, gamma, beta, True, momentum, eps))
    dz, dgamma, dbeta = torch.autograd.grad(y, (z, gamma, beta), g.detach().to(dtype))
    _, mean, invstd = torch.native_batch_norm(z.detach(), gamma.detach(), beta.detach(), None, None, True, momentum, eps)
    return dict(y=y.detach(), mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dz=dz, dgamma=dgamma, dbeta=dbeta)


@functools.lru_cache(maxsize=None)
def bn_references(case):
    """(fp64 autograd, fp32 autograd) of a BatchNorm case on the CPU, computed once per process.  Do not modify."""
    t = bn_inputs(case)
    args = (t["z"], t["gamma"], t["beta"], t["running_mean"], t["running_var"], t["g"])
    return bn_autograd(*args, torch.float64), bn_autograd(*args, torch.float32)


# ---- the layer --------------------------------------------------------------------------------------------------------------------
LAYER_NAMES = ("y", "dx", "dw", "dgamma", "dbeta", "running_mean", "running_var")


@functools.lru_cache(maxsize=None)
def layer_inputs(case, form, bias=False):
    n, h, w, cin, cout = case
    ks, stride = form
    gen = _gen(case + form, 6)
    oh, ow = out_hw(h, w, ks, stride)
    d = dict(x=torch.randn(n, cin, h, w, generator=gen), w=torch.randn(cout, cin, ks, ks, generator=gen) * (ks * ks * cin) ** -0.5,
             gamma=torch.randn(cout, generator=gen) * 0.5 + 1.0, beta=torch.randn(cout, generator=gen) * 0.5,
             running_mean=torch.randn(cout, generator=gen) * 0.1, running_var=torch.rand(cout, generator=gen) + 0.5,
             g=torch.randn(n, cout, oh, ow, generator=gen))
    d["b"] = torch.randn(cout, generator=gen) * 0.5 if bias else None
    return d


def layer_restated(t, stride):
    """The layer in fp64 from the formulas above, no autograd -> dict of ``LAYER_NAMES`` (+ db with a bias, + num_batches_tracked = 1)."""
    z = conv64(t["x"], t["w"], stride, t["b"])
    r = bn_restated(z, t["gamma"], t["beta"], t["running_mean"], t["running_var"], t["g"])
    ks = t["w"].shape[2]
    out = dict(y=r["y"], dx=dinput64(r["dz"], t["w"], stride, t["x"].shape[2:]), dw=wgrad64(r["dz"], t["x"], ks, stride), dgamma=r["dgamma"],
               dbeta=r["dbeta"], running_mean=r["running_mean"], running_var=r["running_var"], num_batches_tracked=1)
    if t["b"] is not None:
        out["db"] = r["dz"].sum((0, 2, 3))
    return out


def layer_autograd(t, stride, dtype):
    """F.silu(F.batch_norm(F.conv2d(x, w, b), training=True)) under autograd on the CPU in ``dtype``, through nn.BatchNorm2d so that
    num_batches_tracked is the module's."""
    x, w, gamma, beta = (t[k].detach().to(dtype).clone().requires_grad_(True) for k in ("x", "w", "gamma", "beta"))
    b = None if t["b"] is None else t["b"].detach().to(dtype).clone().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(w.shape[0], eps=EPS, momentum=MOMENTUM).to(dtype).train()
    with torch.no_grad():
        bn.running_mean.copy_(t["running_mean"]), bn.running_var.copy_(t["running_var"])
    ks = w.shape[2]
    y = F.silu(F.batch_norm(F.conv2d(x, w, b, stride=stride, padding=(ks - 1) // 2), bn.running_mean, bn.running_var, gamma, beta, True, MOMENTUM, EPS))
    bn.num_batches_tracked += 1
    params = (x, w, gamma, beta) + (() if b is None else (b,))
    grads = torch.autograd.grad(y, params, t["g"].detach().to(dtype))
    out = dict(y=y.detach(), dx=grads[0], dw=grads[1], dgamma=grads[2], dbeta=grads[3], running_mean=bn.running_mean.clone(),
               running_var=bn.running_var.clone(), num_batches_tracked=int(bn.num_batches_tracked))
    if b is not None:
        out["db"] = grads[4]
    return out


@functools.lru_cache(maxsize=None)
def layer_references(case, form):
    t = layer_inputs(case, form)
    return layer_autograd(t, form[1], torch.float64), layer_autograd(t, form[1], torch.float32)


def load_base_conv(mod, t):
    """Put the inputs of ``layer_inputs`` into a BaseConv (any dtype / device)."""
    with torch.no_grad():
        mod.conv.weight.copy_(t["w"]), mod.bn.weight.copy_(t["gamma"]), mod.bn.bias.copy_(t["beta"])
        mod.bn.running_mean.copy_(t["running_mean"]), mod.bn.running_var.copy_(t["running_var"])
    mod.bn.eps, mod.bn.momentum = EPS, MOMENTUM
    return mod


# ---- a block and the model --------------------------------------------------------------------------------------------------------
def _seeded_module(build, seed):
    """A train-mode module with seeded parameters: default initialisation, BatchNorm affine parameters and running statistics moved
    off 1 / 0 so that a swapped pair shows, YOLOX's eps and momentum."""
    torch.manual_seed(seed)
    mod = build()
    gen = torch.Generator().manual_seed(seed + 1)
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps, m.momentum = EPS, MOMENTUM
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.num_features, generator=gen) * 0.2 + 1.0), m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.2)
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1), m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.5)
    return mod.train()


def build_block():
    from gdrnpp_bop2022_amd.det.yolox.models.network_blocks import CSPLayer

    n, h, w, c = BLOCK_CASE
    return _seeded_module(lambda: CSPLayer(c, c, n=1), 11)


def _run_block(dtype):
    n, h, w, c = BLOCK_CASE
    gen = torch.Generator().manual_seed(12)
    x0, g = torch.randn(n, c, h, w, generator=gen), torch.randn(n, c, h, w, generator=gen)
    block = build_block().to(dtype)
    x = x0.to(dtype).requires_grad_(True)
    y = block(x)
    y.backward(g.to(dtype))
    return dict(x=x0, g=g, y=y.detach(), dx=x.grad, grads={k: p.grad for k, p in block.named_parameters()},
                buffers={k: b.detach().clone() for k, b in block.named_buffers()})


@functools.lru_cache(maxsize=None)
def block_references():
    """(fp64, fp32) runs of the train-mode CSPLayer on the CPU: x, g, y, dx, grads by parameter name, buffers after the step."""
    return _run_block(torch.float64), _run_block(torch.float32)


MODEL_ARGS = dict(depth=0.33, width=0.25, num_classes=3)
MODEL_INPUT = (2, 3, 64, 96)
MODEL_MARGIN = 1e-3      # the smallest selection margin asked of the fixture (tests/golden/make_golden_yolox_loss.py asks the same)
LOSS_KEYS = ("loss_iou", "loss_conf", "loss_l1", "loss_cls")


def build_model(seed):
    from gdrnpp_bop2022_amd.det.yolox.models import build_yolox

    return _seeded_module(lambda: build_yolox(**MODEL_ARGS), seed)


def model_inputs(seed):
    """The image batch and targets f32[2,3,5] = (class, cx, cy, w, h): three boxes in image 0, two and a zero row in image 1; centres
    and sizes off the 8-pixel lattice of the anchors."""
    gen = torch.Generator().manual_seed(seed + 2)
    b, _, h, w = MODEL_INPUT
    x = torch.randn(*MODEL_INPUT, generator=gen)
    t = torch.zeros(b, 3, 5)
    for i, n_box in enumerate((3, 2)):
        t[i, :n_box, 0] = torch.randint(0, MODEL_ARGS["num_classes"], (n_box,), generator=gen).float()
        t[i, :n_box, 1] = (0.2 + 0.6 * torch.rand(n_box, generator=gen)) * w
        t[i, :n_box, 2] = (0.2 + 0.6 * torch.rand(n_box, generator=gen)) * h
        t[i, :n_box, 3:5] = 14.0 + 26.0 * torch.rand(n_box, 2, generator=gen)
    return x, t


def run_model(model, x, targets):
    """model(x, targets) and the backward of the sum of its losses -> dict: losses (detached, by key), raw (the head's undecoded rows, as
    ``get_losses`` received them), anchors [A,3], grads by parameter name."""
    seen = {}
    get_losses = model.head.get_losses

    def spy(raw, labels):
        seen["raw"] = raw.detach().clone()
        grids, strides = model.head.grids_and_strides(raw.dtype, raw.device)
        seen["anchors"] = torch.cat([grids[0], strides[0]], 1)
        return get_losses(raw, labels)

    model.head.get_losses = spy
    try:
        model.zero_grad(set_to_none=True)
        _, loss_dict = model(x, targets)
        sum(loss_dict[k] for k in LOSS_KEYS).backward()
    finally:
        del model.head.get_losses
    return dict(losses={k: loss_dict[k].detach() for k in LOSS_KEYS}, raw=seen["raw"], anchors=seen["anchors"],
                grads={k: p.grad for k, p in model.named_parameters()})


def base_conv_parameters(model):
    """Names of the parameters of every BaseConv of ``model`` (convolution weight, BatchNorm weight and bias)."""
    from gdrnpp_bop2022_amd.det.yolox.models.network_blocks import BaseConv

    return [f"{name}.{sub}.{leaf}" for name, m in model.named_modules() if isinstance(m, BaseConv)
            for sub, leaf in (("conv", "weight"), ("bn", "weight"), ("bn", "bias"))]


def model_assignment(raw, anchors, targets):
    """SimOTA on the CPU for the rows a run produced -> (matched_gt i32[B,A], the smallest selection margin of the batch by the fp64
    restatement of tests/yolox_loss_ref.py; 0 where the package's batch-wise path and the restatement disagree)."""
    import yolox_loss_ref as YR
    from gdrnpp_bop2022_amd.det.yolox.models.losses import simota_assign_torch

    raw, anchors, targets = raw.detach().cpu(), anchors.detach().cpu().to(raw.dtype), targets.detach().cpu().to(raw.dtype)
    matched = simota_assign_torch(raw, anchors, targets)[0]
    margin = float("inf")
    for b in range(raw.shape[0]):
        gts = targets[b][targets[b].sum(1) > 0].double()
        res = YR.assign_image(raw[b].double(), anchors.double(), gts)
        agree = torch.equal(res["matched_gt"].to(torch.int32), matched[b])      # the batch-wise path against the restatement
        margin = min(margin, min(res["margins"].values()) if agree else 0.0)
    return matched, margin


@functools.lru_cache(maxsize=None)
def model_fixture():
    """The first seed whose fp64 and fp32 CPU runs of the train-mode model give the SAME SimOTA assignment with every selection margin
    above ``MODEL_MARGIN`` -> dict seed, x, targets, ref64, ref32 (``run_model``), matched (i32[B,A]), margin.  A condition on the input:
    with a margin the assignment does not hang on the arithmetic of the layers under it."""
    for seed in range(100, 140):
        x, targets = model_inputs(seed)
        runs = []
        for dtype in (torch.float64, torch.float32):
            runs.append(run_model(build_model(seed).to(dtype), x.to(dtype), targets.to(dtype)))
        m64, margin = model_assignment(runs[0]["raw"], runs[0]["anchors"], targets)
        m32, _ = model_assignment(runs[1]["raw"], runs[1]["anchors"], targets)
        if margin > MODEL_MARGIN and torch.equal(m64, m32) and int((m64 >= 0).sum()) >= 4:
            return dict(seed=seed, x=x, targets=targets, ref64=runs[0], ref32=runs[1], matched=m64, margin=margin)
    raise AssertionError(f"no seed in 100..139 whose fp64 and fp32 runs agree on the assignment with every margin above {MODEL_MARGIN}")
