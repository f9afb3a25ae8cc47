"""The geometry head's backward on the HIP kernels (csrc/conv_gn_bwd.hip, the fp32-MFMA convolution of csrc/yolox_net.hip and the exact-f32 products of csrc/mlp_bwd.hip) against fp64
autograd on the CPU.

The bar, per tensor: max|hip - ref64| <= 2 max|torch fp32 on the CPU - ref64| + 1 ulp of max|ref64| (tests/mlp_bwd_ref.py); every
test prints its worst ratio to that bar.  The weight-gradient GEMM, the forward-shaped convolution and the deconv gather are also held EXACT
on integer operands.

Measured on an MI355X, error / bar:
    conv3x3_wgrad, random operands     0.18 (2 x 16 x 16, 128 -> 128)   0.10 (1 x 32 x 32, 256 -> 256)
    convolution at depth 2304          z 0.40   dx 0.46   dW 0.16       (2 x 16 x 16, 256 -> 256)
    GroupNorm backward (N,H,W,C,G)     y      dz     dgamma dbeta       (plain / GELU)
        (1, 1, 1, 128, 16)             0.29   0.20   0.26   0.00   /   0.21   0.25   0.15   0.16
        (2, 3, 5, 128, 16)             0.35   0.18   0.19   0.15   /   0.20   0.41   0.28   0.18
        (1, 16, 16, 256, 32)           0.51   0.21   0.13   0.14   /   0.35   0.31   0.16   0.14
        (3, 16, 16, 128, 16)           0.30   0.20   0.09   0.07   /   0.29   0.15   0.18   0.17
        (1, 33, 33, 128, 16)           0.32   0.19   0.09   0.06   /   0.32   0.25   0.10   0.10
    bilinear x2 backward               0.13  0.32  0.25  0.34  0.39  0.49  (the six cases in order)
    deconv (y, dx, dW, db)             k=3: 0.20 0.47 0.44 0.04 / 0.71 0.29 0.43 0.13    k=2: 0.29 0.60 0.43 0.05 / 0.68 0.43 0.43 0.13
    [bilinear, ConvModule x 2]         y 0.36, input 0.40, the six parameters 0.23 .. 0.43; with the deconv triple in front all <= 0.39
The six-product convolution on its 256-row tiles measured 1.87 / 2.49 / 2.37 of the bar at depths 1152 / 2304 / 2304, which is why z and
dx run on gdrnpp_conv_bias_act_f32 (DESIGN.md "Geometry head backward" has the table).
"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_gn_bwd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _guarded(t):
    """``t`` [N,C,H,W] channels_last on the device with one NaN image in front of it and one behind: a read outside the tensor
    poisons the result."""
    n = t.shape[0]
    buf = torch.full((n + 2, *t.shape[1:]), float("nan"), device=DEV).contiguous(memory_format=torch.channels_last)
    buf[1:n + 1] = t.to(DEV)
    return buf[1:n + 1]


def _ratios(got, ref64, ref32, names):
    return {k: R.ratio_to_bar(got[k], ref64[k], ref32[k]) for k in names}


# ---- weight gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.WGRAD_EXACT, ids=R.case_id)
def test_wgrad_is_exact_on_integer_operands(hip, case):
    n, h, w, cin, cout = case
    slots, _ = R.wgrad_slots(n * h * w, cin, cout)
    assert hip.load().gdrnpp_conv3x3_wgrad_f32_workspace_bytes(n, h, w, cin, cout) == slots * 9 * cin * cout * 8
    for kind, (dz, x, want) in (("onehot", R.wgrad_onehot(case)), ("lattice", R.wgrad_lattice(case))):
        assert float(want.abs().max()) < 2 ** 24
        got = hip.conv3x3_wgrad_f32(_guarded(dz), _guarded(x)).cpu().double()
        assert got.shape == want.shape and got.is_contiguous()
        assert torch.equal(got, want), kind + ": " + R.wgrad_report(got, want, case)
        if h == w == 1:
            off = torch.ones(3, 3, dtype=torch.bool)
            off[1, 1] = False
            assert not bool(got[:, :, off].any()) and bool(got[:, :, 1, 1].any())


@pytest.mark.parametrize("case", R.WGRAD_RANDOM, ids=R.case_id)
def test_wgrad_rounding_meets_the_bar(hip, case):
    c = R.conv_random(case)
    dz, x = _guarded(c["dz"]), _guarded(c["x"])
    got = hip.conv3x3_wgrad_f32(dz, x)
    ratio = R.ratio_to_bar(got, c["ref64"]["dw"], c["ref32"]["dw"])
    print("conv3x3_wgrad", case, f"ratio={ratio:.3f}")
    assert torch.isfinite(got).all() and ratio <= 1.0
    assert torch.equal(got, hip.conv3x3_wgrad_f32(dz, x))


# ---- the forward-shaped convolutions: z of the training forward and dx (gdrnpp_conv_bias_act_f32) ------------------------------
@pytest.mark.parametrize("channels", R.CONV_CHANNELS, ids=lambda c: "%dto%d" % c)
@pytest.mark.parametrize("spatial", R.CONV_SPATIAL, ids=R.case_id)
def test_conv_is_exact_on_integer_operands(hip, spatial, channels):
    x, wt, bias = R.conv_lattice(spatial, channels)
    z64 = torch.nn.functional.conv2d(x.double(), wt.double(), padding=1)
    xd, wd = _guarded(x), wt.to(DEV)
    assert torch.equal(hip.conv3x3_f32_mfma(xd, hip.conv3x3_weight_kn(wd)).cpu().double(), z64)
    got = hip.conv3x3_f32_mfma(xd, hip.conv3x3_weight_kn(wd), bias.to(DEV))
    assert torch.equal(got.cpu().double(), z64 + bias.double().view(1, -1, 1, 1))
    # the data gradient: the same engine on the flipped, transposed weight; dz = the lattice of the output width
    dz = torch.randint(-8, 9, z64.shape, generator=torch.Generator().manual_seed(9)).float()
    dx, dw, db = hip.conv3x3_backward(xd, wd, _guarded(dz), want=(True, False, True))
    assert dw is None and torch.equal(dx.cpu().double(), R.dx64(dz, wt))
    assert torch.equal(db.cpu().double(), dz.double().sum((0, 2, 3)))


def test_conv_rounding_meets_the_bar(hip):
    case = R.CONV_RANDOM      # depth 9 x 256 = 2304 both ways
    c = R.conv_random(case)
    xd, wd, dzd = _guarded(c["x"]), c["w"].to(DEV), _guarded(c["dz"])
    z = hip.conv3x3_f32_mfma(xd, hip.conv3x3_weight_kn(wd))
    dx, dw, db = hip.conv3x3_backward(xd, wd, dzd)
    ratios = _ratios(dict(z=z, dx=dx, dw=dw), c["ref64"], c["ref32"], ("z", "dx", "dw"))
    print("conv3x3_mfma", case, " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    again = hip.conv3x3_backward(xd, wd, dzd)
    assert all(torch.equal(a, b) for a, b in zip((dx, dw, db), again))
    only_dx = hip.conv3x3_backward(xd, wd, dzd, want=(True, False, False))
    assert only_dx[1] is None and only_dx[2] is None and torch.equal(only_dx[0], dx)


# ---- GroupNorm (+ GELU) backward ------------------------------------------------------------------------------------------------
GN_NAMES = ("dz", "dgamma", "dbeta")


def _gn_run(hip, case, gelu, g=None, want=(True,) * 3):
    t = R.gn_inputs(case)
    z, gamma, beta = _guarded(t["z"]), t["gamma"].to(DEV), t["beta"].to(DEV)
    y, part = hip.groupnorm_act_train(z, gamma, beta, case[4], 1e-5, gelu)
    grads = hip.groupnorm_act_backward(z, part, gamma, beta, case[4], 1e-5, gelu, _guarded(t["g"] if g is None else g), want=want)
    return y, grads


@pytest.mark.parametrize("gelu", (False, True), ids=("plain", "gelu"))
@pytest.mark.parametrize("case", R.GN_CASES, ids=R.case_id)
def test_groupnorm_backward_meets_the_bar(hip, case, gelu):
    ref64, ref32 = R.gn_references(case, gelu)
    y, grads = _gn_run(hip, case, gelu)
    got = dict(zip(GN_NAMES, grads), y=y)
    ratios = _ratios(got, ref64, ref32, ("y",) + GN_NAMES)
    print("groupnorm_bwd", R.case_id(case), "gelu" if gelu else "plain", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(torch.isfinite(v).all() for v in got.values())
    assert max(ratios.values()) <= 1.0, ratios
    for name, a, b in zip(GN_NAMES, grads, _gn_run(hip, case, gelu)[1]):      # two calls, equal bits
        assert torch.equal(a, b), name


GN_WANTS = ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True), (True, False, True))


def test_groupnorm_backward_unwanted_gradients_leave_the_others_unchanged(hip):
    case = R.GN_CASES[2]
    _, full = _gn_run(hip, case, True)
    for want in GN_WANTS:
        _, part = _gn_run(hip, case, True, want=want)
        for name, flag, a, b in zip(GN_NAMES, want, part, full):
            assert (a is None) == (not flag), (want, name)
            if flag:
                assert torch.equal(a, b), (want, name)


@pytest.mark.parametrize("gelu", (False, True), ids=("plain", "gelu"))
def test_groupnorm_backward_propagates_nan_like_autograd(hip, gelu):
    case = R.GN_CASES[1]
    t = R.gn_inputs(case)
    g = t["g"].clone()
    g[1, 37, 2, 3] = float("nan")
    ref = R.gn_autograd(t["z"], t["gamma"], t["beta"], case[4], 1e-5, gelu, g, torch.float64)
    _, grads = _gn_run(hip, case, gelu, g=g)
    for name, got in zip(GN_NAMES, grads):
        want_nan = torch.isnan(ref[name])
        assert 0 < int(want_nan.sum()) < want_nan.numel(), name
        assert torch.equal(torch.isnan(got).cpu(), want_nan), name
        assert torch.isfinite(got.cpu()[~want_nan]).all(), name


# ---- bilinear x2 backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.UP_CASES, ids=R.case_id)
def test_upsample_backward_meets_the_bar(hip, case):
    t = R.up_references(case)
    g = _guarded(t["g"])
    dx = hip.upsample_bilinear2x_backward(g)
    ratio = R.ratio_to_bar(dx, t["ref64"]["dx"], t["ref32"]["dx"])
    print("upsample2x_bwd", case, f"ratio={ratio:.3f}")
    assert torch.isfinite(dx).all() and ratio <= 1.0
    assert torch.equal(dx, hip.upsample_bilinear2x_backward(g))
    if case[1] == case[2] == 1:      # the scale is 0: dx is the sum of the four gradients, rounded once
        assert torch.equal(dx.cpu(), t["g"].double().sum((2, 3), keepdim=True).float())


# ---- transposed convolution -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DECONV_CASES, ids=R.case_id)
def test_deconv_backward(hip, case):
    n, h, w, cin, cout, k, pad, op = case
    t = R.deconv_references(case)
    x, wt, b, dy = _guarded(t["x"]), t["w"].to(DEV), t["b"].to(DEV), _guarded(t["dy"])
    dcols = hip.deconv_im2col(dy, h, w, k, 2, pad, op)
    want = R.deconv_im2col64(t["dy"], h, w, k, 2, pad).reshape(n * h * w, k * k * cout)
    assert torch.equal(dcols.cpu().double(), want)      # the gather only copies values
    z, _ = hip.conv_transpose2d_train(x, wt, b, k, 2, pad, op, 16)
    dx, dw, db = hip.conv_transpose2d_backward(x, wt, dy, k, 2, pad, op)
    ratios = _ratios(dict(y=z, dx=dx, dw=dw, db=db), t["ref64"], t["ref32"], ("y", "dx", "dw", "db"))
    print("deconv_bwd", R.case_id(case), " ".join(f"{k_}={v:.3f}" for k_, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    again = hip.conv_transpose2d_backward(x, wt, dy, k, 2, pad, op, want=(False, True, False))
    assert again[0] is None and again[2] is None and torch.equal(again[1], dw)


# ---- through autograd -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def train_kernels():
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers

    hip_layers.set_train_kernels(True)
    yield hip_layers
    hip_layers.set_train_kernels(False)


def _grads(features, x, g):
    from gdrnpp_bop2022_amd.gdrn_modeling import heads

    x = x.detach().clone().requires_grad_(True)
    for p in features.parameters():
        p.grad = None
    y = heads.run_features(features, x)
    y.backward(g)
    return y, [x.grad] + [p.grad for p in features.parameters()]


def _graph_nodes(y):
    seen, todo = set(), [y.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


FOREIGN_NODES = {"ConvolutionBackward0", "NativeGroupNormBackward0", "GeluBackward0", "UpsampleBilinear2DBackward0"}


def _make_case(with_deconv):
    from gdrnpp_bop2022_amd.gdrn_modeling import heads

    torch.manual_seed(11 + with_deconv)
    layers = [torch.nn.UpsamplingBilinear2d(scale_factor=2)]
    layers += [heads.ConvModule(128, 128, 3, padding=1, norm="GN", num_gn_groups=16, act="GELU") for _ in range(2)]
    size = 8
    if with_deconv:
        layers = [torch.nn.ConvTranspose2d(128, 128, 3, stride=2, padding=1, output_padding=1, bias=False), torch.nn.GroupNorm(16, 128),
                  torch.nn.GELU()] + layers
        size = 4
    cpu32 = torch.nn.ModuleList(layers)
    with torch.no_grad():
        for m in cpu32.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.copy_(torch.randn(128) * 0.5 + 1.0), m.bias.copy_(torch.randn(128) * 0.5)
            elif isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(128, 128, 3, 3) * (9 * 128) ** -0.5)      # not the head's 0.001 initialisation
            elif isinstance(m, torch.nn.ConvTranspose2d):
                m.weight.copy_(torch.randn(128, 128, 3, 3) * (9 * 128 / 4) ** -0.5)
    x, g = torch.randn(2, 128, size, size), torch.randn(2, 128, 4 * size if with_deconv else 2 * size, 4 * size if with_deconv else 2 * size)
    y64, ref64 = _grads(copy.deepcopy(cpu32).double(), x.double(), g.double())
    y32, ref32 = _grads(cpu32, x, g)
    names = ["y", "x"] + [n for n, _ in cpu32.named_parameters()]
    return dict(features=cpu32, x=x, g=g, names=names, ref64=[y64.detach()] + ref64, ref32=[y32.detach()] + ref32)


@pytest.fixture(scope="module")
def head_case():
    return _make_case(False)


@pytest.fixture(scope="module")
def head_case_deconv():
    return _make_case(True)


def _check_head(hip_layers, case, expect_nodes):
    gpu = copy.deepcopy(case["features"]).to(DEV)
    xg, gg = _cl(case["x"]), case["g"].to(DEV)
    from gdrnpp_bop2022_amd import hip_lib

    before, x3_before = hip_layers.fallback_launches(), hip_lib.x3_launch_count()
    y, grads = _grads(gpu, xg, gg)
    assert hip_lib.x3_launch_count() == x3_before      # no three-product launch, so no range word to repeat a step for
    nodes = _graph_nodes(y)
    assert expect_nodes <= nodes and not FOREIGN_NODES & nodes, nodes
    assert hip_layers.fallback_launches() == before
    ratios = {n: R.ratio_to_bar(a, b, c) for n, a, b, c in zip(case["names"], [y.detach()] + grads, case["ref64"], case["ref32"])}
    print("head_bwd", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    return gpu, xg, gg, grads


def test_head_layers_train_without_a_foreign_kernel(hip, train_kernels, head_case):
    hip_layers = train_kernels
    gpu, xg, gg, grads = _check_head(hip_layers, head_case, {"Conv3x3GnActBackward", "Upsample2xBackward"})
    # a frozen conv weight gets no gradient and changes nobody else's bits
    frozen_w = gpu[1].conv.weight
    frozen_w.requires_grad_(False)
    try:
        _, frozen = _grads(gpu, xg, gg)
    finally:
        frozen_w.requires_grad_(True)
    for n, p, a, b in zip(head_case["names"][1:], [None] + list(gpu.parameters()), frozen, grads):
        if p is frozen_w:
            assert a is None, n
        else:
            assert torch.equal(a, b), n
    # switch off: PyTorch's graph, as before
    hip_layers.set_train_kernels(False)
    y_off, _ = _grads(gpu, xg, gg)
    nodes = _graph_nodes(y_off)
    assert FOREIGN_NODES <= nodes and "Conv3x3GnActBackward" not in nodes, nodes


def test_head_with_the_deconv_triple_in_front(hip, train_kernels, head_case_deconv):
    _check_head(train_kernels, head_case_deconv, {"Conv3x3GnActBackward", "Upsample2xBackward", "ConvTranspose2dGnBackward"})


def test_groupnorm_alone_takes_its_function(hip, train_kernels):
    gn, act = torch.nn.GroupNorm(16, 128).to(DEV), torch.nn.GELU()
    x = _cl(torch.randn(1, 128, 3, 3)).requires_grad_(True)
    y = train_kernels.groupnorm_act(gn, act, x)
    assert "GroupNormActBackward" in _graph_nodes(y) and not FOREIGN_NODES & _graph_nodes(y)
    y.sum().backward()
    assert x.grad is not None and gn.weight.grad is not None and gn.bias.grad is not None


def test_inference_is_untouched(hip, train_kernels, head_case_deconv):
    from gdrnpp_bop2022_amd.gdrn_modeling import heads

    hip_layers = train_kernels
    gpu = copy.deepcopy(head_case_deconv["features"]).to(DEV)
    xg = _cl(head_case_deconv["x"])
    with torch.no_grad():
        on = heads.run_features(gpu, xg)
        hip_layers.set_train_kernels(False)
        off = heads.run_features(gpu, xg)
    assert on.grad_fn is None and torch.equal(on, off)
