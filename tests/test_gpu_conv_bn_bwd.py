"""Training YOLOX's BaseConv (convolution, BatchNorm with batch statistics, SiLU) on the HIP kernels (csrc/conv_bn_bwd.hip and the fp32-MFMA
convolution of csrc/yolox_net.hip) against fp64 autograd on the CPU.

The bar, per tensor: max|hip - ref64| <= 2 max|torch fp32 on the CPU - ref64| + 1 ulp of max|ref64| (tests/mlp_bwd_ref.py); every
test prints its worst ratio to that bar.  The weight gradient and the stride-2 data gradient are also held EXACT on one-hot and
integer-lattice operands.

Measured on an MI355X, error / bar:
    conv (z dx dw)                     1x1/1            3x3/1            1x1/2            3x3/2
        2 x 16 x 16,  80 -> 160    0.18 0.23 0.35   0.31 0.45 0.21   0.15 0.39 0.66   0.27 0.21 0.47
        1 x 32 x 32,  64 ->  64    0.16 0.17 0.27   0.23 0.23 0.09   0.19 0.42 0.30   0.15 0.55 0.22
        1 x  4 x  4, 640 -> 1280   0.26 0.28 0.41   0.54 0.50 0.39   0.08 0.17 0.30   0.09 0.09 0.30
    BatchNorm + SiLU (N,H,W,C)     y     mean  invstd r_mean r_var dz    dgamma dbeta
        (1, 1, 2, 4)               0.46  0.25  0.13   0.21   0.13  0.48  0.36   0.46
        (2, 3, 5, 40)              0.32  0.25  0.24   0.15   0.16  0.21  0.42   0.17
        (1, 16, 16, 256)           0.48  0.25  0.25   0.17   0.14  0.50  0.36   0.11
        (3, 16, 16, 80)            0.64  0.23  0.16   0.14   0.14  0.38  0.25   0.20
        (1, 33, 33, 24)            0.33  0.18  0.18   0.17   0.16  0.23  0.13   0.18
        (1, 2, 2, 1280)            0.37  0.25  0.24   0.18   0.14  0.40  0.44   0.21
    layer 2 x 8 x 8, 40 -> 80      y     dx    dw    dgamma dbeta r_mean r_var
        1x1/1                      0.37  0.18  0.40  0.32   0.21  0.15   0.18
        3x3/1                      0.30  0.27  0.40  0.19   0.20  0.19   0.16
        1x1/2                      0.24  0.48  0.53  0.38   0.54  0.10   0.15
        3x3/2                      0.19  0.49  0.34  0.21   0.24  0.16   0.16
        3x3/1 with a bias, 2 x 3 x 5, 12 -> 16: dx 0.26  dw 0.41  db 0.12  dgamma 0.28  dbeta 0.42
    CSPLayer(64, 64, n=1), 2 x 8 x 8   y 0.32, input 0.30, the 15 parameters and 10 running statistics <= 0.51
    YOLOX(0.33, 0.25, 3 classes), 2 x 3 x 64 x 96: the SimOTA assignment is the CPU runs'; loss_iou 0.72, loss_conf 0.05, loss_l1 0.00,
        loss_cls 0.04; the 222 parameter gradients of the 74 BaseConv layers <= 0.76; two steps give equal bits
"""
import os
import sys
from unittest import mock

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bn_bwd_ref as R  # noqa: E402

from gdrnpp_bop2022_amd.det.yolox.models import train_layers  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox.models.network_blocks import BaseConv  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def train_switch():
    hip_layers.set_train_kernels(True)
    yield
    hip_layers.set_train_kernels(False)


@pytest.fixture
def reproducible_torch_convs():
    """PyTorch's own convolutions are not bit-reproducible by default (the vendor library's sums over pixels have no fixed order); a
    comparison of two module-path runs bit for bit asks for its deterministic kernels."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def _guarded(t):
    """``t`` [N,C,H,W] channels_last on the device with one NaN image in front of it and one behind: a read outside the tensor
    poisons the result."""
    n = t.shape[0]
    buf = torch.full((n + 2, *t.shape[1:]), float("nan"), device=DEV).contiguous(memory_format=torch.channels_last)
    buf[1:n + 1] = t.to(DEV)
    return buf[1:n + 1]


def _ratios(got, ref64, ref32, names):
    return {k: R.ratio_to_bar(got[k], ref64[k], ref32[k]) for k in names}


def _show(what, ratios):
    print(what, " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def form_id(form):
    return "k%ds%d" % form


# ---- weight gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.WGRAD_EXACT, ids=R.case_id)
def test_wgrad_is_exact_on_integer_operands(hip, case):
    n, h, w, cin, cout, ks, stride = case
    oh, ow = R.out_hw(h, w, ks, stride)
    slots, _ = R.wgrad_slots(n * oh * ow, cin, cout, ks)
    assert hip.load().gdrnpp_conv_wgrad_f32_workspace_bytes(*case) == slots * ks * ks * cin * cout * 8
    for kind, (dz, x, want) in (("onehot", R.wgrad_onehot(case)), ("lattice", R.wgrad_lattice(case))):
        assert float(want.abs().max()) < 2 ** 24
        got = hip.conv_wgrad_f32(_guarded(dz), _guarded(x), ks, stride).cpu().double()
        assert got.shape == want.shape and got.is_contiguous()
        assert torch.equal(got, want), kind + ": " + R.wgrad_report(got, want, case)
        if h == w == 1 and ks == 3:
            off = torch.ones(3, 3, dtype=torch.bool)
            off[1, 1] = False
            assert not bool(got[:, :, off].any()) and bool(got[:, :, 1, 1].any())


# ---- stride-2 data gradient -----------------------------------------------------------------------------------------------------
def _dinput(hip, dz, wt):
    return hip.conv_backward(None, wt.to(DEV), 2, _guarded(dz), want=(True, False))[0]


@pytest.mark.parametrize("case", R.DINPUT_EXACT, ids=R.case_id)
def test_stride2_dinput_is_exact_on_integer_operands(hip, case):
    n, h, w, cin, cout = case
    dz, wt, want = R.dinput_lattice(case)
    assert float(want.abs().max()) < 2 ** 24
    got = _dinput(hip, dz, wt)
    assert got.shape == (n, cin, h, w) and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got.cpu().double(), want)
    # the same kernel behind the wrapper of its own name
    w_op = wt.permute(2, 3, 0, 1).reshape(9 * cout, cin).contiguous().to(DEV)
    assert torch.equal(hip.conv3x3s2_dinput_any_f32(_guarded(dz), w_op, cin), got)


def test_stride2_dinput_of_an_image_does_not_depend_on_the_batch(hip):
    case = (1, 8, 8, 132, 136)
    c = R.conv_random(case, (3, 2))
    more = torch.randn(2, *c["dz"].shape[1:], generator=torch.Generator().manual_seed(3))
    one = _dinput(hip, c["dz"], c["w"])
    three = _dinput(hip, torch.cat([c["dz"], more], 0), c["w"])
    assert torch.equal(three[:1], one)
    dz, wt, want = R.dinput_lattice(case, n_images=3)
    assert torch.equal(_dinput(hip, dz, wt).cpu().double(), want)


# ---- random operands: the four forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", R.FORMS, ids=form_id)
@pytest.mark.parametrize("case", R.RANDOM_CASES, ids=R.case_id)
def test_conv_gradients_meet_the_bar(hip, case, form):
    c = R.conv_random(case, form)
    xd, wd, dzd = _guarded(c["x"]), c["w"].to(DEV), _guarded(c["dz"])
    z = hip.conv_train_f32(xd, wd, None, form[1])
    dx, dw = hip.conv_backward(xd, wd, form[1], dzd)
    got = dict(z=z, dx=dx, dw=dw)
    ratios = _ratios(got, c["ref64"], c["ref32"], ("z", "dx", "dw"))
    _show(f"conv {R.case_id(case)} {form_id(form)}", ratios)
    assert all(torch.isfinite(v).all() for v in got.values())
    assert max(ratios.values()) <= 1.0, ratios
    again = hip.conv_backward(xd, wd, form[1], dzd)      # two calls, equal bits
    assert torch.equal(dx, again[0]) and torch.equal(dw, again[1])
    only_dx, none = hip.conv_backward(xd, wd, form[1], dzd, want=(True, False))
    none2, only_dw = hip.conv_backward(xd, wd, form[1], dzd, want=(False, True))
    assert none is None and none2 is None and torch.equal(only_dx, dx) and torch.equal(only_dw, dw)


# ---- BatchNorm with batch statistics + SiLU -----------------------------------------------------------------------------------------
GRADS = ("dz", "dgamma", "dbeta")


def _bn_run(hip, case, want=(True,) * 3):
    t = R.bn_inputs(case)
    z, gamma, beta = _guarded(t["z"]), t["gamma"].to(DEV), t["beta"].to(DEV)
    rm, rv = t["running_mean"].to(DEV), t["running_var"].to(DEV)
    mean, invstd = hip.bn_train_stats(z, R.EPS, rm, rv, R.MOMENTUM)
    y = hip.bn_silu_apply(z, mean, invstd, gamma, beta)
    grads = hip.bn_silu_backward(_guarded(t["g"]), z, mean, invstd, gamma, beta, want=want)
    return dict(zip(GRADS, grads), y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv)


@pytest.mark.parametrize("case", R.BN_CASES, ids=R.case_id)
def test_batchnorm_silu_forward_and_backward_meet_the_bar(hip, case):
    ref64, ref32 = R.bn_references(case)
    got = _bn_run(hip, case)
    ratios = _ratios(got, ref64, ref32, R.BN_NAMES)
    _show(f"bn_silu {R.case_id(case)}", ratios)
    assert all(torch.isfinite(v).all() for v in got.values())
    assert got["y"].is_contiguous(memory_format=torch.channels_last) and got["dz"].is_contiguous(memory_format=torch.channels_last)
    assert max(ratios.values()) <= 1.0, ratios
    again = _bn_run(hip, case)      # two calls, equal bits
    for name in R.BN_NAMES:
        assert torch.equal(got[name], again[name]), name
    for i, name in enumerate(GRADS):      # an output asked for alone has the bits it has when all are asked for
        alone = _bn_run(hip, case, want=tuple(j == i for j in range(3)))
        assert torch.equal(alone[name], got[name]), name
        assert all(alone[other] is None for other in GRADS if other != name)
    # the statistics alone leave running statistics that were not given untouched
    mean, invstd = hip.bn_train_stats(_guarded(R.bn_inputs(case)["z"]), R.EPS)
    assert torch.equal(mean, got["mean"]) and torch.equal(invstd, got["invstd"])


def test_batchnorm_refuses_one_value_per_channel(hip):
    z = torch.zeros(1, 8, 1, 1, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="at least 2"):
        hip.bn_train_stats(z, R.EPS)
    with pytest.raises(RuntimeError, match="want"):
        hip.bn_silu_backward(z, z, *(torch.zeros(8, device=DEV),) * 4, want=(False, False, False))


# ---- the layer --------------------------------------------------------------------------------------------------------------------
def _layer_run(case, form, input_grad=True):
    n, h, w, cin, cout = case
    t = R.layer_inputs(case, form)
    mod = R.load_base_conv(BaseConv(cin, cout, form[0], form[1]), t).to(DEV).train()
    x = _guarded(t["x"]).requires_grad_(input_grad)
    with mock.patch.object(train_layers.ConvBnSilu, "apply", wraps=train_layers.ConvBnSilu.apply) as spy:
        y = mod(x)
    assert spy.call_count == 1
    y.backward(_guarded(t["g"]))
    assert int(mod.bn.num_batches_tracked) == 1
    return dict(y=y.detach(), dx=x.grad, dw=mod.conv.weight.grad, dgamma=mod.bn.weight.grad, dbeta=mod.bn.bias.grad,
                running_mean=mod.bn.running_mean, running_var=mod.bn.running_var)


@pytest.mark.parametrize("form", R.FORMS, ids=form_id)
def test_layer_meets_the_bar(hip, form, train_switch):
    ref64, ref32 = R.layer_references(R.LAYER_CASE, form)
    before = hip_layers.fallback_launches()
    got = _layer_run(R.LAYER_CASE, form)
    ratios = _ratios(got, ref64, ref32, R.LAYER_NAMES)
    _show(f"layer {form_id(form)}", ratios)
    assert max(ratios.values()) <= 1.0, ratios
    assert got["y"].is_contiguous(memory_format=torch.channels_last) and hip_layers.fallback_launches() == before
    no_dx = _layer_run(R.LAYER_CASE, form, input_grad=False)      # the Focus convolution: the input needs no gradient
    assert no_dx["dx"] is None
    for name in R.LAYER_NAMES:
        if name != "dx":
            assert torch.equal(no_dx[name], got[name]), name


def test_layer_with_a_convolution_bias_meets_the_bar(hip, train_switch):
    case, form = (2, 3, 5, 12, 16), (3, 1)
    t = R.layer_inputs(case, form, bias=True)
    ref64, ref32 = R.layer_autograd(t, 1, torch.float64), R.layer_autograd(t, 1, torch.float32)
    mod = R.load_base_conv(BaseConv(12, 16, 3, 1, bias=True), t)
    with torch.no_grad():
        mod.conv.bias.copy_(t["b"])
    mod = mod.to(DEV).train()
    x = _guarded(t["x"]).requires_grad_(True)
    mod(x).backward(_guarded(t["g"]))
    got = dict(dx=x.grad, dw=mod.conv.weight.grad, db=mod.conv.bias.grad, dgamma=mod.bn.weight.grad, dbeta=mod.bn.bias.grad)
    ratios = _ratios(got, ref64, ref32, tuple(got))
    _show("layer with bias", ratios)
    assert max(ratios.values()) <= 1.0, ratios


def test_layer_is_the_module_path_with_the_switch_off(hip, reproducible_torch_convs):
    t = R.layer_inputs(R.LAYER_CASE, (3, 1))
    mod = R.load_base_conv(BaseConv(40, 80, 3, 1), t).to(DEV).train()
    with mock.patch.object(train_layers.ConvBnSilu, "apply", side_effect=AssertionError("ConvBnSilu with the switch off")):
        y = mod(_guarded(t["x"]).requires_grad_(True))
    plain = R.load_base_conv(BaseConv(40, 80, 3, 1), t).to(DEV).train()
    assert torch.equal(y, plain.act(plain.bn(plain.conv(_guarded(t["x"])))))


# ---- a block ----------------------------------------------------------------------------------------------------------------------
def test_csp_layer_meets_the_bar(hip, train_switch):
    ref64, ref32 = R.block_references()
    block = R.build_block().to(DEV)
    x = _guarded(ref64["x"]).requires_grad_(True)
    before = hip_layers.fallback_launches()
    y = block(x)
    y.backward(_guarded(ref64["g"]))
    assert hip_layers.fallback_launches() == before
    ratios = dict(y=R.ratio_to_bar(y, ref64["y"], ref32["y"]), dx=R.ratio_to_bar(x.grad, ref64["dx"], ref32["dx"]))
    for k, p in block.named_parameters():
        ratios[k] = R.ratio_to_bar(p.grad, ref64["grads"][k], ref32["grads"][k])
    for k, b in block.named_buffers():
        if b.dtype.is_floating_point:
            ratios[k] = R.ratio_to_bar(b, ref64["buffers"][k], ref32["buffers"][k])
        else:
            assert int(b) == int(ref64["buffers"][k]), k
    _show("CSPLayer", ratios)
    assert max(ratios.values()) <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}


# ---- the model --------------------------------------------------------------------------------------------------------------------
def _model_run(f):
    model = R.build_model(f["seed"]).to(DEV)
    return model, R.run_model(model, f["x"].to(DEV), f["targets"].to(DEV))


def test_model_losses_and_base_conv_gradients_meet_the_bar(hip, train_switch):
    f = R.model_fixture()
    before = hip_layers.fallback_launches()
    with mock.patch.object(train_layers.ConvBnSilu, "apply", wraps=train_layers.ConvBnSilu.apply) as spy:
        model, got = _model_run(f)
    names = R.base_conv_parameters(model)
    assert spy.call_count == len(names) // 3 and hip_layers.fallback_launches() == before
    matched = hip.yolox_assign(got["raw"].contiguous(), got["anchors"].contiguous(), f["targets"].to(DEV))[0].cpu()
    differ = int((matched != f["matched"]).sum())
    assert differ == 0, (f"the SimOTA SELECTION of the HIP run differs from the CPU runs' at {differ} anchors although every margin of the "
                         f"fixture is above {R.MODEL_MARGIN} ({f['margin']:.3g}): the losses and gradients below cannot be compared — look at "
                         f"the selection, not at the arithmetic of the losses")
    ratios = {k: R.ratio_to_bar(got["losses"][k], f["ref64"]["losses"][k], f["ref32"]["losses"][k]) for k in R.LOSS_KEYS}
    grad_ratios = {k: R.ratio_to_bar(got["grads"][k], f["ref64"]["grads"][k], f["ref32"]["grads"][k]) for k in names}
    worst = sorted(grad_ratios, key=grad_ratios.get)[-3:]
    _show("model losses", ratios)
    _show(f"model BaseConv gradients: {len(names)} tensors, worst", {k: grad_ratios[k] for k in worst})
    assert max(ratios.values()) <= 1.0, ratios
    assert max(grad_ratios.values()) <= 1.0, {k: v for k, v in grad_ratios.items() if v > 1.0}
    _, again = _model_run(f)      # two identical steps, equal bits
    assert all(torch.equal(again["losses"][k], got["losses"][k]) for k in R.LOSS_KEYS)
    assert all(torch.equal(again["grads"][k], got["grads"][k]) for k in names)


def test_model_with_the_switch_off_is_the_module_path(hip, reproducible_torch_convs):
    f = R.model_fixture()
    with mock.patch.object(train_layers.ConvBnSilu, "apply", side_effect=AssertionError("ConvBnSilu with the switch off")):
        _, got = _model_run(f)
    with mock.patch.object(BaseConv, "forward", lambda self, x: self.act(self.bn(self.conv(x)))):      # the forward before this layer existed
        _, plain = _model_run(f)
    for k in R.LOSS_KEYS:
        assert torch.equal(got["losses"][k], plain["losses"][k]), k
    assert torch.equal(got["raw"], plain["raw"])
    for k, g in plain["grads"].items():
        assert (g is None and got["grads"][k] is None) or torch.equal(got["grads"][k], g), k
