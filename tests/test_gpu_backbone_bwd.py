"""The ConvNeXt stem and downsample layers trained on the HIP kernels (csrc/backbone_bwd.hip; hip_layers.StemConvLN, DownsampleLNConv)
against fp64 autograd on the CPU (tests/backbone_bwd_ref.py).

The bar, per tensor: max|hip - ref64| <= 2 max|torch fp32 on the CPU - ref64| + 1 ulp of max|ref64| (tests/mlp_bwd_ref.py); every test
prints its worst ratio to that bar.  Without LayerNorm (ln_w = NULL) the stem's dW and db and the downsample's z, dA and dW are held EXACT
on integer lattices, and one-hot / coded probes name the element behind every output.

Measured on an MI355X, error / bar:
    stem (N, H, W)          dW      db      dln_w   dln_b
        (1, 4, 16)          0.28    0.11    0.08    0.15
        (3, 8, 16)          0.40    0.07    0.09    0.15
        (2, 12, 48)         0.34    0.06    0.07    0.16
        (1, 4, 1024)        0.11    0.04    0.08    0.06
        (5, 32, 32)         0.13    0.06    0.07    0.09
        (7 / 8 / 9, 4, 16)  0.39 / 0.44 / 0.50   0.11 / 0.07 / 0.11   0.07 / 0.12 / 0.07   0.13 / 0.10 / 0.16      M = 28, 32, 36
        (63 / 64 / 65, 4, 16)  0.19 / 0.19 / 0.17   0.06 each   0.05 / 0.10 / 0.08   0.10 / 0.13 / 0.10            M = 252, 256, 260
    (with fp32 chains of 128 pixels instead of 32, dW reached 0.80 at M = 128; with an fp32 u on top, 0.97 there and dln_w 0.20 - 0.61)
    downsample (N, H, W, C, Cout)    z       dx      dln_w   dln_b   dW      db
        (1, 2, 2, 128, 128)          0.37    0.37    0.20    0.43    0.33    0.00
        (3, 2, 6, 128, 256)          0.17    0.19    0.31    0.20    0.38    0.14
        (2, 8, 4, 256, 512)          0.08    0.22    0.30    0.19    0.37    0.14
        (1, 4, 4, 512, 1024)         0.34    0.23    0.28    0.34    0.26    0.17
        (1, 2, 2, 1024, 128)         0.12    0.42    0.46    0.38    0.29    0.00
        (5, 16, 16, 128, 256)        0.15    0.28    0.20    0.26    0.24    0.03
        (1, 48, 48, 1024, 128)       0.07    0.45    0.31    0.39    0.14    0.02      576 pixel groups on the adjoint's 512 slots
    (1, 130, 130, 1024, 128), 4225 groups on the 4096 workgroups of the copy and LayerNorm kernels: bit-equal to layernorm_nhwc re-ordered,
    bit-equal copy round trip, the adjoint's dln_b within one ulp of the fp64 column sum.
    ConvNeXtFeatures(depths (1, 1), dims (128, 256)) on (3, 3, 32, 32): y 0.27, the 26 parameter gradients 0.13 .. 0.55 (stem 0.31 .. 0.41,
    downsample 0.24 .. 0.55); the small GDRN_DoubleMask on that backbone through forward(do_loss=True) + backward: loss 0.10, the backbone's
    parameters 0.23 .. 0.81, the head's and Patch-PnP's 0.28 .. 0.91.
The stem forward is bit-equal to the inference kernel; the downsample's training forward (exact-f32 product) is not the inference forward's
three-product convolution bit for bit, as in Conv3x3GnAct; under no_grad the inference kernels run and the switch changes no bit.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_bwd_ref as R  # noqa: E402
from mlp_bwd_ref import bar, ratio_to_bar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
EPS = R.EPS

STEM_MFMA, STEM_HBM = "mfma_f32:stem_bwd", "hbm:stem_bwd"
LN_BWD, EXACT, TN, COLSUM = "hbm:ln_patch2x2_bwd", "linear_exact", "gemm_tn", "hbm:colsum"


def _tail(t, pad=4096):
    """``t`` as the head of a flat device allocation with NaN behind its end: a read past the tensor poisons the result."""
    t = t.contiguous()
    buf = torch.full((t.numel() + pad,), NAN, device=DEV, dtype=t.dtype)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf[:t.numel()].view(t.shape)


def _cl_tail(t_nchw):
    """[N,C,H,W] -> the same tensor channels_last on the device, NaN behind its end."""
    return _tail(t_nchw.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


def _nchw(t_cl):
    return t_cl.detach().cpu().contiguous()


@pytest.fixture
def train_kernels():
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers

    hip_layers.set_train_kernels(True)
    yield hip_layers
    hip_layers.set_train_kernels(False)


def _records(hip, fn):
    timer = hip.LaunchTimer()
    hip.set_launch_timer(timer)
    try:
        out = fn()
    finally:
        hip.set_launch_timer(None)
    return out, [r[0] for r in timer.records]


def _graph_nodes(y):
    seen, todo = set(), [y.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


# ---- the stem ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.STEM_CASES + (R.STEM_DEEP,), ids=R.case_id)
def test_stem_without_layernorm_is_exact_on_integer_operands(hip, case):
    n, h, w = case
    assert hip.load().gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(n, h, w, 128) == R.stem_workspace_bytes(n, h, w)
    x, g, dw64, db64 = R.stem_lattice(case)
    xd, gd = _tail(x), _cl_tail(g)
    weight = torch.full((128, 3, 4, 4), NAN, device=DEV)      # not read without a LayerNorm
    (dw, db, none_g, none_b), kinds = _records(hip, lambda: hip.stem_conv4x4_ln_backward(xd, weight, None, None, EPS, gd, want=(True, True, False, False)))
    assert none_g is None and none_b is None and kinds == [STEM_MFMA]
    bad = (dw.cpu().long() != dw64).nonzero()
    assert len(bad) == 0, f"dW: {len(bad)} wrong of {dw.numel()}, first {bad[:4].tolist()}; M={n * h * w // 16}: slots {R.stem_slots(n * h * w // 16)}"
    assert torch.equal(db.cpu().long(), db64)
    # two calls, equal bits; either gradient alone: the same bits, and db alone on the form without matrix instructions
    dw2, db2, _, _ = hip.stem_conv4x4_ln_backward(xd, weight, None, None, EPS, gd, want=(True, True, False, False))
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    (dw3, none), kinds = _records(hip, lambda: hip.stem_conv4x4_ln_backward(xd, weight, None, None, EPS, gd, want=(True, False, False, False))[:2])
    assert none is None and torch.equal(dw3, dw) and kinds == [STEM_MFMA]
    (none, db3), kinds = _records(hip, lambda: hip.stem_conv4x4_ln_backward(xd, weight, None, None, EPS, gd, want=(False, True, False, False))[:2])
    assert none is None and torch.equal(db3, db) and kinds == [STEM_HBM]


@pytest.mark.parametrize("case", ((1, 4, 16), (2, 12, 48), (1, 4, 1024), (5, 32, 32)), ids=R.case_id)
def test_stem_one_hot_probes_locate_every_patch_element(hip, case):
    cx = R.stem_coded_x(case)
    xd = _tail(cx)
    weight = torch.zeros((128, 3, 4, 4), device=DEV)
    others = torch.arange(128)
    for probe in R.stem_probes(case):
        dw = hip.stem_conv4x4_ln_backward(xd, weight, None, None, EPS, _cl_tail(R.stem_onehot(case, probe)), want=(True, False, False, False))[0].cpu()
        assert torch.equal(dw[probe[1]], R.stem_probe_patch(case, cx, probe)), probe      # element (ci, ky, kx) of the probe's pixel, by its code
        assert not dw[others != probe[1]].any(), probe


@pytest.mark.parametrize("case", R.STEM_CASES, ids=R.case_id)
def test_stem_with_layernorm_meets_the_bar(hip, case):
    x, weight, bias, ln_w, ln_b, g = R.stem_inputs(case)
    ref64, ref32 = R.stem_references(case)
    xd, gd = _tail(x), _cl_tail(g)
    wd, bd, lwd = _tail(weight), _tail(bias), _tail(ln_w)
    full = hip.stem_conv4x4_ln_backward(xd, wd, bd, lwd, EPS, gd)
    ratios = {name: ratio_to_bar(t, ref64[name], ref32[name]) for name, t in zip(R.STEM_NAMES, full)}
    print("backbone_bwd stem", R.case_id(case), " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(torch.isfinite(t).all() for t in full) and max(ratios.values()) <= 1.0, ratios
    again = hip.stem_conv4x4_ln_backward(xd, wd, bd, lwd, EPS, gd)
    assert all(torch.equal(a, b) for a, b in zip(again, full))
    for want in ((True, False, False, False), (False, True, False, True), (False, False, True, False), (True, False, True, True)):
        part, kinds = _records(hip, lambda: hip.stem_conv4x4_ln_backward(xd, wd, bd, lwd, EPS, gd, want=want))
        assert kinds == [STEM_MFMA if want[0] else STEM_HBM], (want, kinds)
        for f, p, t in zip(want, part, full):
            assert (p is None) if not f else torch.equal(p, t), want


# ---- the downsample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DOWN_CASES, ids=R.case_id)
def test_patch_copy_places_every_element_and_round_trips(hip, case):
    n, h, w, c, _ = case
    assert hip.load().gdrnpp_layernorm_patch2x2_backward_workspace_bytes(n, h, w, c) == R.ln_patch_workspace_bytes(n, h, w, c)
    cx = R.down_coded_x(case)
    xd = _cl_tail(cx)
    a = hip.layernorm_patch2x2(xd)
    assert torch.equal(a.cpu(), R.patch2x2(R.rows_of(cx).reshape(n, h, w, c)))      # each code at column (ky, kx, ci) of its output pixel
    (dx, none_g, none_b), kinds = _records(hip, lambda: hip.layernorm_patch2x2_backward(xd, None, EPS, _tail(a), want=(True, False, False)))
    assert none_g is None and none_b is None and kinds == [LN_BWD]
    assert dx.is_contiguous(memory_format=torch.channels_last) and torch.equal(_nchw(dx), cx)


@pytest.mark.parametrize("case", R.DOWN_CASES, ids=R.case_id)
def test_layernorm_in_patch_order_has_the_bits_of_layernorm_nhwc(hip, case):
    n, h, w, c, _ = case
    x, ln_w, ln_b = R.down_inputs(case)[:3]
    xd, lw, lb = _cl_tail(x), _tail(ln_w), _tail(ln_b)
    y = hip.layernorm_nhwc(xd, lw, lb, EPS)
    a = hip.layernorm_patch2x2(xd, lw, lb, EPS)
    assert torch.isfinite(a).all() and torch.equal(a.cpu(), R.patch2x2(y.permute(0, 2, 3, 1).cpu()))
    assert torch.equal(hip.layernorm_patch2x2(xd, lw, lb, EPS), a)


def test_more_groups_than_workgroups_keep_the_bits(hip):
    """4225 pixel groups for the 4096 workgroups of the copy and LayerNorm kernels and the 512 of the adjoint: every workgroup walks
    on to further groups.  The LayerNorm against ``layernorm_nhwc`` re-ordered, the two copies as a round trip, the adjoint twice."""
    n, h, w, c, _ = R.DOWN_GRID_STRIDE
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(n, c, h, w, generator=gen)
    ln_w, ln_b = torch.randn(c, generator=gen) * 0.1 + 1.0, torch.randn(c, generator=gen) * 0.1
    xd, lw, lb = _cl_tail(x), _tail(ln_w), _tail(ln_b)
    a = hip.layernorm_patch2x2(xd, lw, lb, EPS)
    assert torch.isfinite(a).all() and torch.equal(a.cpu(), R.patch2x2(hip.layernorm_nhwc(xd, lw, lb, EPS).permute(0, 2, 3, 1).cpu()))
    copy_ = hip.layernorm_patch2x2(xd)
    assert torch.equal(copy_.cpu(), R.patch2x2(x.permute(0, 2, 3, 1)))
    assert torch.equal(_nchw(hip.layernorm_patch2x2_backward(xd, None, EPS, _tail(copy_), want=(True, False, False))[0]), x)
    d_a = _tail(torch.randn(a.shape, generator=gen))
    first, again = (hip.layernorm_patch2x2_backward(xd, lw, EPS, d_a) for _ in range(2))
    assert all(torch.isfinite(t).all() for t in first) and all(torch.equal(p, t) for p, t in zip(first, again))
    # the channel sums against fp64 from the same operands: dln_b = colsum(dA re-ordered)
    dy = R.unpatch2x2(d_a.cpu().double(), n, h, w, c).reshape(-1, c)
    assert float((first[2].cpu().double() - dy.sum(0)).abs().max()) <= float(np.spacing(np.float32(dy.sum(0).abs().max())))


@pytest.mark.parametrize("case", R.DOWN_CASES, ids=R.case_id)
def test_downsample_without_layernorm_is_exact_on_integer_operands(hip, case):
    n, h, w, c, cout = case
    x, weight, g, want = R.down_lattice(case)
    xd, wd, gd = _cl_tail(x), _tail(weight), _cl_tail(g)
    a = hip.layernorm_patch2x2(xd)
    z = hip.linear_f32_exact(a, _tail(hip.downsample_weight_nk(wd)))
    assert torch.equal(z.cpu().double(), R.rows_of(want["z"]))
    dx, _, _, dw, db = hip.downsample_backward(xd, _tail(a), None, EPS, wd, gd, want=(True, False, False, True, True))
    for name, got in (("dx", dx), ("dW", dw), ("db", db)):      # dx is dA through the inverse copy
        bad = (got.cpu().double() != want[name]).nonzero()
        assert len(bad) == 0, f"{name}: {len(bad)} wrong of {got.numel()}, first {bad[:4].tolist()}"


@pytest.mark.parametrize("case", R.DOWN_CASES, ids=R.case_id)
def test_downsample_with_layernorm_meets_the_bar(hip, case):
    n, h, w, c, cout = case
    x, ln_w, ln_b, weight, bias, g = R.down_inputs(case)
    ref64, ref32 = R.down_references(case)
    xd, lw, lb, wd, bd, gd = _cl_tail(x), _tail(ln_w), _tail(ln_b), _tail(weight), _tail(bias), _cl_tail(g)
    a = _tail(hip.layernorm_patch2x2(xd, lw, lb, EPS))
    z = hip.linear_f32_exact(a, hip.downsample_weight_nk(wd), bd)
    ratios = {"z": ratio_to_bar(z, R.rows_of(ref64["z"]), R.rows_of(ref32["z"]))}
    full, kinds = _records(hip, lambda: hip.downsample_backward(xd, a, lw, EPS, wd, gd))
    assert sorted(kinds) == sorted([EXACT, LN_BWD, TN, COLSUM]), kinds
    for name, t in zip(R.DOWN_NAMES, full):
        assert torch.isfinite(t).all(), name
        ratios[name] = ratio_to_bar(_nchw(t), ref64[name], ref32[name])
    print("backbone_bwd down", R.case_id(case), " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    again = hip.downsample_backward(xd, a, lw, EPS, wd, gd)
    assert all(torch.equal(p, t) for p, t in zip(again, full))
    subsets = {(True, False, False, False, False): [EXACT, LN_BWD], (False, True, True, False, False): [EXACT, LN_BWD],
               (False, False, False, True, False): [TN], (False, False, False, False, True): [COLSUM], (True, False, True, True, False): [EXACT, LN_BWD, TN]}
    for want, launches in subsets.items():
        part, kinds = _records(hip, lambda: hip.downsample_backward(xd, a if want[3] else None, lw, EPS, wd, gd, want=want))
        assert sorted(kinds) == sorted(launches), (want, kinds)
        for f, p, t in zip(want, part, full):
            assert (p is None) if not f else torch.equal(p, t), want


def test_shapes_outside_the_kernels_raise_in_their_words(hip):
    lib = hip.load()
    assert lib.gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(1, 6, 16, 128) == 0 and lib.gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(1, 4, 24, 128) == 0
    assert lib.gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(1, 4, 1040, 128) == 0 and lib.gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(1, 4, 16, 96) == 0
    assert lib.gdrnpp_layernorm_patch2x2_backward_workspace_bytes(1, 3, 2, 128) == 0 and lib.gdrnpp_layernorm_patch2x2_backward_workspace_bytes(1, 2, 2, 64) == 0
    assert lib.gdrnpp_layernorm_patch2x2_backward_workspace_bytes(1, 2, 2, 384) == 0
    x = torch.zeros(1, 3, 6, 16, device=DEV)
    with pytest.raises(RuntimeError, match="outside the kernel"):
        hip.stem_conv4x4_ln_backward(x, torch.zeros(128, 3, 4, 4, device=DEV), None, torch.ones(128, device=DEV), EPS, torch.zeros(1, 128, 1, 4, device=DEV))
    with pytest.raises(RuntimeError, match="without a LayerNorm"):
        hip.stem_conv4x4_ln_backward(torch.zeros(1, 3, 4, 16, device=DEV), torch.zeros(128, 3, 4, 4, device=DEV), None, None, EPS,
                                     torch.zeros(1, 128, 1, 4, device=DEV).contiguous(memory_format=torch.channels_last))
    with pytest.raises(RuntimeError, match="outside the kernel"):
        hip.layernorm_patch2x2(torch.zeros(1, 128, 3, 2, device=DEV).contiguous(memory_format=torch.channels_last))


# ---- the layers ----------------------------------------------------------------------------------------------------------------------
def _stem_modules(case):
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import LayerNorm2d

    _, weight, bias, ln_w, ln_b, _ = R.stem_inputs(case)
    conv, ln = torch.nn.Conv2d(3, 128, 4, stride=4), LayerNorm2d(128, eps=EPS)
    with torch.no_grad():
        conv.weight.copy_(weight), conv.bias.copy_(bias), ln.weight.copy_(ln_w), ln.bias.copy_(ln_b)
    return conv.to(DEV), ln.to(DEV)


def _down_modules(case, kernel=2):
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import LayerNorm2d

    _, ln_w, ln_b, weight, bias, _ = R.down_inputs(case)
    c, cout = case[3:]
    ln, conv = LayerNorm2d(c, eps=EPS), torch.nn.Conv2d(c, cout, kernel, stride=2, padding=(kernel - 1) // 2)
    with torch.no_grad():
        ln.weight.copy_(ln_w), ln.bias.copy_(ln_b), conv.bias.copy_(bias)
        if kernel == 2:
            conv.weight.copy_(weight)
    return ln.to(DEV), conv.to(DEV)


def test_stem_layer_forward_backward_and_guards(hip, train_kernels):
    hip_layers = train_kernels
    case = (3, 8, 16)
    x, g = R.stem_inputs(case)[0], R.stem_inputs(case)[5]
    ref64, ref32 = R.stem_references(case)
    conv, ln = _stem_modules(case)
    xd = _tail(x)
    with torch.no_grad():
        y_inf = hip_layers.stem(conv, ln, xd)
    before = hip_layers.fallback_launches()
    y = hip_layers.stem(conv, ln, xd)
    nodes = _graph_nodes(y)
    assert "StemConvLNBackward" in nodes and not ({"ConvolutionBackward0", "NativeLayerNormBackward0"} & nodes), nodes
    assert torch.equal(y, y_inf) and y.is_contiguous(memory_format=torch.channels_last)      # the bits of the inference kernel
    y.backward(g.to(DEV))
    assert hip_layers.fallback_launches() == before
    got = dict(dW=conv.weight.grad, db=conv.bias.grad, dln_w=ln.weight.grad, dln_b=ln.bias.grad)
    ratios = {k: ratio_to_bar(v, ref64[k], ref32[k]) for k, v in got.items()}
    print("backbone_bwd stem layer", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    # a channels_last weight, a frozen convolution: the same bits for the others
    conv2, ln2 = copy.deepcopy(conv).to(memory_format=torch.channels_last), copy.deepcopy(ln)
    for p in list(conv2.parameters()) + list(ln2.parameters()):
        p.grad = None
    conv2.weight.requires_grad_(False)
    hip_layers.stem(conv2, ln2, xd).backward(g.to(DEV))
    assert conv2.weight.grad is None and torch.equal(conv2.bias.grad, conv.bias.grad) and torch.equal(ln2.weight.grad, ln.weight.grad)
    # an image that itself needs a gradient: PyTorch's graph, counted
    y = hip_layers.stem(conv, ln, xd.clone().requires_grad_(True))
    nodes = _graph_nodes(y)
    assert "StemConvLNBackward" not in nodes and "ConvolutionBackward0" in nodes and hip_layers.fallback_launches() == before + 1, nodes
    # the CPU: PyTorch's graph, nothing counted
    y = hip_layers.stem(copy.deepcopy(conv).cpu(), copy.deepcopy(ln).cpu(), x)
    assert "ConvolutionBackward0" in _graph_nodes(y) and hip_layers.fallback_launches() == before + 1
    # the switch off: today's graph and counter; no_grad: the inference kernel whatever the switch
    hip_layers.set_train_kernels(False)
    y_off = hip_layers.stem(conv, ln, xd)
    assert "ConvolutionBackward0" in _graph_nodes(y_off) and hip_layers.fallback_launches() == before + 1
    with torch.no_grad():
        assert torch.equal(hip_layers.stem(conv, ln, xd), y_inf) and hip_layers.fallback_launches() == before + 1


def test_downsample_layer_forward_backward_and_guards(hip, train_kernels):
    hip_layers = train_kernels
    case = (3, 2, 6, 128, 256)
    x, g = R.down_inputs(case)[0], R.down_inputs(case)[5]
    ref64, ref32 = R.down_references(case)
    ln, conv = _down_modules(case)
    with torch.no_grad():
        z_inf = hip_layers.conv2d(conv, ln(_cl_tail(x)))      # the parent's two calls
    before = hip_layers.fallback_launches()
    xd = _cl_tail(x).requires_grad_(True)
    z = hip_layers.downsample(ln, conv, xd)
    nodes = _graph_nodes(z)
    assert "DownsampleLNConvBackward" in nodes and not ({"ConvolutionBackward0", "NativeLayerNormBackward0", "AddmmBackward0"} & nodes), nodes
    assert z.is_contiguous(memory_format=torch.channels_last)
    z.backward(g.to(DEV))
    assert hip_layers.fallback_launches() == before
    got = dict(z=z, dx=xd.grad, dln_w=ln.weight.grad, dln_b=ln.bias.grad, dW=conv.weight.grad, db=conv.bias.grad)
    ratios = {k: ratio_to_bar(_nchw(v), ref64[k], ref32[k]) for k, v in got.items()}
    print("backbone_bwd down layer", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    # not the bits of the inference forward's three-product convolution, but close
    assert float((z.detach() - z_inf).abs().max()) <= 1e-4 * float(z_inf.abs().max())
    # a frozen LayerNorm and input: only the weight-gradient launches, the same bits
    ln2, conv2 = copy.deepcopy(ln).requires_grad_(False), copy.deepcopy(conv)
    conv2.weight.grad = conv2.bias.grad = None
    _, kinds = _records(hip, lambda: hip_layers.downsample(ln2, conv2, _cl_tail(x)).backward(g.to(DEV)))
    assert kinds.count(TN) == 1 and kinds.count(LN_BWD) == 0 and kinds.count(COLSUM) == 1 and kinds.count(EXACT) == 1, kinds      # the forward's product alone
    assert torch.equal(conv2.weight.grad, conv.weight.grad) and torch.equal(conv2.bias.grad, conv.bias.grad)

    def theirs(z, counted):
        nodes = _graph_nodes(z)
        assert "DownsampleLNConvBackward" not in nodes and {"ConvolutionBackward0", "NativeLayerNormBackward0"} <= nodes, nodes
        assert hip_layers.fallback_launches() == counted

    # an odd height; a 3x3 / stride 2 convolution in the slot: PyTorch's graph, each counted
    theirs(hip_layers.downsample(ln, conv, _cl_tail(torch.randn(1, 128, 3, 4)).requires_grad_(True)), before + 1)
    theirs(hip_layers.downsample(ln, _down_modules(case, kernel=3)[1], _cl_tail(x).requires_grad_(True)), before + 2)
    # the CPU: PyTorch's graph, nothing counted
    theirs(hip_layers.downsample(copy.deepcopy(ln).cpu(), copy.deepcopy(conv).cpu(), x.clone().requires_grad_(True)), before + 2)
    # the switch off: today's graph; no_grad: the parent's two calls bit for bit, whatever the switch, and the counter as before
    hip_layers.set_train_kernels(False)
    theirs(hip_layers.downsample(ln, conv, _cl_tail(x).requires_grad_(True)), before + 2)
    with torch.no_grad():
        off = hip_layers.downsample(ln, conv, _cl_tail(x))
        hip_layers.set_train_kernels(True)
        on = hip_layers.downsample(ln, conv, _cl_tail(x))
    assert torch.equal(off, z_inf) and torch.equal(on, z_inf) and on.grad_fn is None and hip_layers.fallback_launches() == before + 2


# ---- the backbone --------------------------------------------------------------------------------------------------------------------
OURS = {"StemConvLNBackward", "DownsampleLNConvBackward", "DwConvLNBackward", "ConvNeXtMlpBackward"}
THEIRS = {"ConvolutionBackward0", "NativeLayerNormBackward0", "AddmmBackward0"}


def _init_(module):
    with torch.no_grad():      # variance-preserving weights, biases of 0.1, scales around 1 (the layer scale's own 1e-6 would hide the blocks)
        for name, p in module.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (p[0].numel() ** -0.5))
            elif name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.1)
            else:
                p.copy_(1.0 + torch.randn_like(p) * 0.1)


def _backbone():
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import ConvNeXtFeatures

    torch.manual_seed(23)
    net = ConvNeXtFeatures(depths=(1, 1), dims=(128, 256), out_indices=(1,))
    _init_(net)
    return net.eval()


def _backbone_reference(net, x, g, dtype):
    m = copy.deepcopy(net).cpu().to(dtype)
    (y,) = m(x.to(dtype))
    y.backward(g.to(dtype))
    return y.detach(), {n: p.grad for n, p in m.named_parameters()}


def test_backbone_trains_on_this_librarys_kernels(hip, train_kernels):
    hip_layers = train_kernels
    net = _backbone()
    gen = torch.Generator().manual_seed(29)
    x, g = torch.randn(3, 3, 32, 32, generator=gen), torch.randn(3, 256, 4, 4, generator=gen)
    (y64, g64), (y32, g32) = _backbone_reference(net, x, g, torch.float64), _backbone_reference(net, x, g, torch.float32)
    net = net.to(DEV)
    foreign, x3 = hip_layers.fallback_launches(), hip.x3_launch_count()
    (y,) = net(_tail(x))
    nodes = _graph_nodes(y)
    assert OURS <= nodes and not (THEIRS & nodes), nodes
    y.backward(g.to(DEV))
    assert hip_layers.fallback_launches() == foreign and hip.x3_launch_count() == x3
    ratios = {"y": ratio_to_bar(_nchw(y), y64, y32)}
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        ratios[n] = ratio_to_bar(p.grad, g64[n], g32[n])
    print("backbone_bwd backbone", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _small_model():
    """The small GDRN_DoubleMask of tests/test_gpu_pnp_bwd.py (class-aware, 3 classes, double mask, a 16 x 16 output, a 128-channel head)
    on the two-stage ConvNeXt backbone above: 64 x 64 crops -> 8 x 8 x 256 features."""
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import GDRN_DoubleMask
    from gdrnpp_bop2022_amd.gdrn_modeling.heads import ConvPnPNet, TopDownDoubleMaskXyzRegionHead

    cfg = get_cfg("tudl_convnext_a6", ["MODEL.POSE_NET.OUTPUT_RES=16", "MODEL.POSE_NET.INPUT_RES=64", "MODEL.POSE_NET.LOSS_CFG.FULL_MASK_LW=1.0"])
    assert cfg.MODEL.POSE_NET.NUM_CLASSES == 3
    torch.manual_seed(5)
    head = TopDownDoubleMaskXyzRegionHead(256, feat_dim=128, up_types=("bilinear",), num_conv_per_block=1, mask_num_classes=3,
                                          xyz_num_classes=3, region_num_classes=3, mask_out_dim=2)
    pnp = ConvPnPNet(nIn=69, num_regions=64, featdim=128, rot_dim=6, norm="GN", act="gelu", final_spatial_size=(2, 2))
    model = GDRN_DoubleMask(cfg, _backbone(), head, pnp_net=pnp)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith("backbone."):
                continue
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (p[0].numel() ** -0.5))
            elif name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.1)
    return cfg, model.eval()


def _small_batch(cfg, B, dev, dtype=torch.float32):
    from gdrnpp_bop2022_amd import synthetic as S
    from gdrnpp_bop2022_amd.gdrn_modeling import losses as L
    from tests.test_gpu_losses import dense_inputs, rot

    rng = np.random.default_rng(20221019 + 37)
    net = cfg.MODEL.POSE_NET
    C, o = net.NUM_CLASSES, net.OUTPUT_RES

    def T(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
        return a.to(dev, dtype if a.is_floating_point() else None)

    ext = (rng.random((C, 3)) * 0.1 + 0.05).astype(np.float32)
    det = S.make_detections(B, C, ext, rng, out_res=o)
    det["roi_cls"][:] = np.array([1, 0, 2, 1, 2])[:B]
    det["roi_extent"] = ext[det["roi_cls"]]
    dn = dense_inputs(B, o, 1, net.GEO_HEAD.NUM_REGIONS + 1, seed=C)
    syms = [None if c % 2 else np.stack([np.eye(3), rot([0, 0, 1], 180)]).astype(np.float32) for c in range(C)]
    batch = dict(roi_classes=T(det["roi_cls"]), roi_cams=T(det["roi_cam"]), roi_whs=T(det["roi_wh"]), roi_centers=T(det["roi_center"]),
                 resize_ratios=T(det["resize_ratio"]), roi_coord_2d=T(S.coord2d_roi(det["roi_center"], det["scale"], out_res=o)),
                 roi_extents=T(det["roi_extent"]), gt_xyz=T(dn["gt_xyz"]), gt_xyz_bin=T(dn["gt_xyz_bin"]), gt_region=T(dn["gt_region"]),
                 gt_ego_rot=T(det["R_gt"]), gt_trans=T(det["t_gt"]),
                 gt_trans_ratio=T((rng.standard_normal((B, 3)) * [0.1, 0.1, 0.2] + [0, 0, 1.0]).astype(np.float32)),
                 **{k: T(dn[k]) for k in ("gt_mask_trunc", "gt_mask_visib", "gt_mask_obj", "gt_mask_full")})
    points = ((rng.random((C, 200, 3)) - 0.5) * ext[:, None]).astype(np.float32)
    x = T(rng.random((B, 3, net.INPUT_RES, net.INPUT_RES)).astype(np.float32))
    per_roi = dict(gt_points=points[det["roi_cls"]], sym_infos=[syms[c] for c in det["roi_cls"]], extents=det["roi_extent"])
    tables = (lambda: dict(points=T(points), sym=L.sym_tables(syms, dev), extents=T(ext)))
    return x, batch, tables, per_roi


def _cpu_reference(cfg, model, dtype):
    """forward_maps + the losses of tests/losses_ref.py + backward on the CPU in ``dtype`` -> (total loss, {parameter: gradient})."""
    from gdrnpp_bop2022_amd.gdrn_modeling import losses as L
    from tests import losses_ref as LR

    m = copy.deepcopy(model).cpu().to(dtype)
    x, batch, _, per_roi = _small_batch(cfg, 5, "cpu", dtype)
    pred_rot_, pred_t_, maps = m.forward_maps(x, batch["roi_classes"], batch["roi_coord_2d"], None, batch["roi_extents"], None)
    Rm, tr = L.pose_from_pred_train(pred_rot_, pred_t_, batch["roi_cams"], batch["roi_centers"], batch["roi_whs"], batch["resize_ratios"],
                                    z_type="REL", is_allo=True)
    loss, _ = LR.gdrn_loss_ref(L.loss_cfg(cfg), out_mask_vis=maps["mask"], out_mask_full=maps["full_mask"], out_x=maps["coor_x"],
                               out_y=maps["coor_y"], out_z=maps["coor_z"], out_region=maps["region"], out_rot=Rm, out_trans=tr,
                               out_centroid=pred_t_[:, :2], out_trans_z=pred_t_[:, 2], gt_rot=batch["gt_ego_rot"],
                               gt_points=torch.from_numpy(per_roi["gt_points"]).to(dtype), sym_infos=per_roi["sym_infos"],
                               extents=torch.from_numpy(per_roi["extents"]).to(dtype),
                               **{k: batch[k] for k in ("gt_mask_trunc", "gt_mask_visib", "gt_mask_obj", "gt_mask_full", "gt_xyz", "gt_xyz_bin",
                                                        "gt_region", "gt_trans", "gt_trans_ratio")})
    total = sum(loss.values())
    total.backward()
    return total.detach(), {n: p.grad for n, p in m.named_parameters()}


def test_model_trains_without_a_pytorch_layer(hip, train_kernels):
    hip_layers = train_kernels
    cfg, model = _small_model()
    (t64, g64), (t32, g32) = _cpu_reference(cfg, model, torch.float64), _cpu_reference(cfg, model, torch.float32)
    model = model.to(DEV).to(memory_format=torch.channels_last)
    x, batch, tables, _ = _small_batch(cfg, 5, DEV)
    notes = []
    note = hip_layers.note_foreign_launch
    hip_layers.note_foreign_launch = lambda what: (notes.append(what), note(what))[1]
    try:
        _, loss = model(x, do_loss=True, gt_tables=tables(), **batch)
    finally:
        hip_layers.note_foreign_launch = note
    total = sum(loss.values())
    nodes = _graph_nodes(total)
    theirs = {n for n in nodes if "Convolution" in n or "LayerNorm" in n or "Addmm" in n}
    assert OURS <= nodes and "HeadTailBackward" in nodes and not theirs, nodes
    assert not notes, notes
    total.backward()
    ratios = {"loss": abs(float(total.detach()) - float(t64)) / bar(t64.reshape(1), t32.reshape(1))}
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        ratios[n] = ratio_to_bar(p.grad, g64[n], g32[n])
    print("backbone_bwd model", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
