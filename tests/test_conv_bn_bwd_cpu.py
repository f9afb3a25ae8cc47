"""YOLOX's BaseConv training layer without a GPU: the fp64 restatement of tests/conv_bn_bwd_ref.py against fp64 autograd, the guard of
``train_layers.conv_bn_silu``, and the train-mode model on the CPU with the training switch on."""
import os
import sys
from unittest import mock

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bn_bwd_ref as R  # noqa: E402

from gdrnpp_bop2022_amd import hip_lib  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox.models import train_layers  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox.models.network_blocks import BaseConv  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers  # noqa: E402


@pytest.fixture
def train_switch():
    hip_layers.set_train_kernels(True)
    yield
    hip_layers.set_train_kernels(False)


def _close(got, want, what):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    tol = 1e-11 * max(1.0, float(want.abs().max()))
    assert got.shape == want.shape and float((got - want).abs().max()) <= tol, (what, float((got - want).abs().max()), tol)


@pytest.mark.parametrize("case", R.RESTATED_CASES, ids=R.case_id)
def test_restated_layer_is_fp64_autograd(case):
    t = R.layer_inputs(case[:5], case[5:7], bias=bool(case[7]))
    got, want = R.layer_restated(t, case[6]), R.layer_autograd(t, case[6], torch.float64)
    assert set(got) == set(want) and ("db" in got) == bool(case[7])
    for k in want:
        _close(got[k], want[k], k)
    assert got["num_batches_tracked"] == want["num_batches_tracked"] == 1


@pytest.mark.parametrize("case", R.BN_CASES, ids=R.case_id)
def test_restated_batchnorm_is_fp64_autograd(case):
    t = R.bn_inputs(case)
    got = R.bn_restated(t["z"], t["gamma"], t["beta"], t["running_mean"], t["running_var"], t["g"])
    want = R.bn_references(case)[0]
    for k in R.BN_NAMES:
        _close(got[k], want[k], k)


@pytest.mark.parametrize("form", R.FORMS, ids=lambda f: "k%ds%d" % f)
def test_restated_conv_gradients_are_fp64_autograd(form):
    case = (2, 6, 8, 12, 20)
    c = R.conv_random(case, form)
    _close(R.conv64(c["x"], c["w"], form[1]), c["ref64"]["z"], "z")
    _close(R.wgrad64(c["dz"], c["x"], *form), c["ref64"]["dw"], "dw")
    _close(R.dinput64(c["dz"], c["w"], form[1], c["x"].shape[2:]), c["ref64"]["dx"], "dx")


def test_case_tables_reach_the_plans_edges():
    n, h, w, cin, cout, ks, stride = R.WGRAD_LONG
    slots, rows = R.wgrad_slots(n * h * w, cin, cout, ks)
    assert n * h * w > R.WG_CHUNK * R.WG_SLOT_CAP and rows == 2 * R.WG_CHUNK and 0 < n * h * w - (slots - 1) * rows < R.WG_CHUNK
    assert R.wgrad_slots(576, 32, 64, 3) == (2, 512) and R.wgrad_slots(768, 160, 40, 1) == (2, 512)
    slots, rows = R.bn_slots(33 * 33)
    assert 0 < 33 * 33 - (slots - 1) * rows < rows


def _layer(ks=3, stride=1, cin=8, cout=8, groups=1, **bn):
    conv = nn.Conv2d(cin, cout, ks, stride, (ks - 1) // 2, groups=groups, bias=False)
    return conv, nn.BatchNorm2d(cout, **bn).train()


REFUSED = {
    "eval_bn": lambda: (*_layer(), (2, 8, 4, 4), lambda conv, bn: bn.eval()),
    "momentum_none": lambda: (*_layer(momentum=None), (2, 8, 4, 4), None),
    "groups2": lambda: (*_layer(groups=2), (2, 8, 4, 4), None),
    "5x5": lambda: (*_layer(ks=5), (2, 8, 4, 4), None),
    "width6": lambda: (*_layer(cin=6), (2, 6, 4, 4), None),
    "odd_h_stride2": lambda: (*_layer(stride=2), (2, 8, 5, 4), None),
    "m1": lambda: (*_layer(), (1, 8, 1, 1), None),
    "no_affine": lambda: (*_layer(affine=False), (2, 8, 4, 4), None),
}


def test_guard_takes_the_layers_shapes():
    for ks, stride in R.FORMS:
        conv, bn = _layer(ks, stride)
        assert train_layers._layer_ok(conv, bn, torch.zeros(2, 8, 4, 4))
    conv, bn = _layer()
    assert train_layers._layer_ok(conv, bn, torch.zeros(1, 8, 1, 2))      # M = 2


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_guard_returns_none_on_the_cpu_and_for_refused_configurations(name, train_switch):
    conv, bn, shape, tweak = REFUSED[name]()
    if tweak:
        tweak(conv, bn)
    x = torch.zeros(shape, requires_grad=True)
    assert not train_layers._layer_ok(conv, bn, x)
    before = hip_layers.fallback_launches()
    assert train_layers.conv_bn_silu(conv, bn, x) is None and hip_layers.fallback_launches() == before      # a CPU tensor: nobody's launch
    with mock.patch.object(hip_layers, "_train_ok", lambda t: True):      # as if x were a device tensor under the switch
        assert train_layers.conv_bn_silu(conv, bn, x) is None
    assert hip_layers.fallback_launches() == before + 1 and "conv_bn_silu" in hip_layers.last_fallback()


def test_guard_returns_none_on_the_cpu_for_a_layer_it_would_take(train_switch):
    conv, bn = _layer()
    x = torch.zeros(2, 8, 4, 4, requires_grad=True)
    assert train_layers._layer_ok(conv, bn, x) and train_layers.conv_bn_silu(conv, bn, x) is None
    with mock.patch.object(hip_layers, "_train_ok", lambda t: True):      # parameters on the CPU: refused, nothing launched
        assert train_layers.conv_bn_silu(conv, bn, x) is None
    hip_layers.set_train_kernels(False)
    assert train_layers.conv_bn_silu(conv, bn, x) is None


def test_the_new_wrappers_are_on_the_namespace_and_the_symbols_in_the_header():
    for name in ("bn_train_stats", "bn_silu_apply", "bn_silu_backward", "conv_wgrad_f32", "conv3x3s2_dinput_any_f32", "conv_backward", "conv_train_f32"):
        assert getattr(hip_lib, name) is getattr(hip_lib.yolox, name)
    for name in ("gdrnpp_bn_train_stats_nhwc", "gdrnpp_bn_train_stats_workspace_bytes", "gdrnpp_bn_silu_apply_nhwc", "gdrnpp_bn_silu_backward",
                 "gdrnpp_bn_silu_backward_workspace_bytes", "gdrnpp_conv_wgrad_f32", "gdrnpp_conv_wgrad_f32_workspace_bytes",
                 "gdrnpp_conv3x3s2_dinput_any_f32"):
        assert name in hip_lib.SIGNATURES and hasattr(hip_lib.load(), name), name


def test_workspace_queries_answer_zero_outside_the_kernels():
    lib = hip_lib.load()
    assert lib.gdrnpp_bn_train_stats_workspace_bytes(1, 8) == 0 and lib.gdrnpp_bn_train_stats_workspace_bytes(2, 6) == 0
    assert lib.gdrnpp_bn_silu_backward_workspace_bytes(1, 8) == 0
    assert lib.gdrnpp_bn_train_stats_workspace_bytes(33 * 33, 24) == R.bn_slots(33 * 33)[0] * 2 * 24 * 8
    for bad in ((1, 4, 4, 6, 8, 3, 1), (1, 4, 4, 8, 6, 1, 1), (1, 4, 4, 8, 8, 5, 1), (1, 4, 4, 8, 8, 3, 3), (1, 5, 4, 8, 8, 3, 2), (0, 4, 4, 8, 8, 3, 1)):
        assert lib.gdrnpp_conv_wgrad_f32_workspace_bytes(*bad) == 0, bad
    for case in R.WGRAD_EXACT:
        n, h, w, cin, cout, ks, stride = case
        oh, ow = R.out_hw(h, w, ks, stride)
        assert lib.gdrnpp_conv_wgrad_f32_workspace_bytes(*case) == R.wgrad_slots(n * oh * ow, cin, cout, ks)[0] * ks * ks * cin * cout * 8, case


def test_model_fixture_has_one_assignment_with_margins():
    f = R.model_fixture()
    print("model fixture: seed", f["seed"], "margin", f["margin"], "foreground", int((f["matched"] >= 0).sum()))
    assert f["margin"] > R.MODEL_MARGIN
    m32, _ = R.model_assignment(f["ref32"]["raw"], f["ref32"]["anchors"], f["targets"])
    assert torch.equal(m32, f["matched"])
    names = R.base_conv_parameters(R.build_model(f["seed"]))
    assert len(names) > 100 and all(f["ref64"]["grads"][k] is not None for k in names)


def test_train_mode_model_on_the_cpu_with_the_switch_on_is_the_module_path(train_switch):
    f = R.model_fixture()
    before = hip_layers.fallback_launches()
    with mock.patch.object(train_layers.ConvBnSilu, "apply", side_effect=AssertionError("ConvBnSilu on a CPU tensor")):
        got = R.run_model(R.build_model(f["seed"]), f["x"], f["targets"])
    for k in R.LOSS_KEYS:
        assert torch.equal(got["losses"][k], f["ref32"]["losses"][k]), k
    for k, g in f["ref32"]["grads"].items():
        assert (g is None and got["grads"][k] is None) or torch.equal(got["grads"][k], g), k
    assert hip_layers.fallback_launches() == before


def test_base_conv_in_eval_mode_never_asks_the_training_layer(train_switch):
    mod = BaseConv(8, 8, 3, 1).eval()
    with mock.patch.object(train_layers, "conv_bn_silu", side_effect=AssertionError("asked in eval mode")):
        mod(torch.zeros(1, 8, 4, 4))
