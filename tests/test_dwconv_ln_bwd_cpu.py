"""The fp64 restatement of the dwconv7x7 + LayerNorm backward (tests/dwconv_ln_bwd_ref.py) against torch.autograd over the
repository's fallback graph, on the case table of the GPU tests; and the parts of the feature that need no device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dwconv_ln_bwd_ref as R  # noqa: E402


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_matches_fp64_autograd(case):
    t = R.make_inputs(case)
    got = R.restated_backward(t["x"], t["weight"], t["bias"], t["gamma"], t["beta"], t["g"])
    want, _ = R.references(case)
    n_pix = case[0] * case[1] * case[2]
    for name in ("y",) + R.NAMES:
        a, b = got[name], want[name]
        assert a.shape == b.shape and a.dtype == torch.float64 == b.dtype, name
        # two fp64 evaluations in different summation orders: terms of O(1), sums of at most 49 (dx), C (the means) and n_pix (the
        # parameter gradients) of them; 1e-12 leaves four decimal digits over 2^-53 for the cancellation inside du
        tol = 1e-12 * (1.0 + float(b.abs().max())) * max(49, n_pix) ** 0.5
        assert float((a - b).abs().max()) <= tol, (name, float((a - b).abs().max()), tol)


def test_restatement_supplies_du_that_reproduces_db():
    t = R.make_inputs(R.CASES[3])
    got = R.restated_backward(t["x"], t["weight"], t["bias"], t["gamma"], t["beta"], t["g"])
    assert got["du"].shape == t["x"].shape
    assert torch.allclose(got["du"].sum((0, 2, 3)), R.references(R.CASES[3])[0]["db"], rtol=0, atol=1e-11)


def test_case_table_covers_every_mechanism():
    cs = {c[3] for c in R.CASES}
    assert {4, 8, 128, 1024} <= cs
    hw = {(c[1], c[2]) for c in R.CASES}
    assert {(1, 1), (3, 5), (7, 7), (5, 13), (9, 10), (16, 16)} <= hw and (1, 16, 16, 256) in R.CASES
    assert {c[0] for c in R.CASES} >= {1, 3}
    n, h, w, c = R.PERSISTENT_CASE
    per = 256 // (c // 4)
    assert -(-n * h * -(-w // 4) // per) > 512 and -(-n * h * -(-w // 8) // per) > 64


def test_bar_is_twice_the_fp32_error_plus_one_ulp():
    ref64 = torch.tensor([1.0, -3.0], dtype=torch.float64)
    ref32 = torch.tensor([1.0, -3.0 + 2.0 ** -20], dtype=torch.float32)
    assert R.bar(ref64, ref32) == 2.0 * 2.0 ** -20 + 2.0 ** -22
    assert R.ratio_to_bar(ref64.float(), ref64, ref32) == 0.0


def test_train_switch_is_off_by_default_and_changes_nothing_on_the_cpu():
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import ConvNeXtBlock

    assert hip_layers.train_kernels() is False
    torch.manual_seed(0)
    block = ConvNeXtBlock(8)
    x = torch.randn(2, 8, 6, 6, requires_grad=True)
    want = block(x)
    before = hip_layers.fallback_launches()
    hip_layers.set_train_kernels(True)
    try:
        assert hip_layers.train_kernels() is True
        got = block(x)      # a CPU tensor: the switch does not apply, PyTorch's operators run
    finally:
        hip_layers.set_train_kernels(False)
    assert torch.equal(got, want) and hip_layers.fallback_launches() == before
    assert issubclass(hip_layers.DwConvLN, torch.autograd.Function)


def test_backward_wrapper_refuses_before_the_library_is_touched():
    from gdrnpp_bop2022_amd import hip_lib

    t = R.make_inputs(R.CASES[1])
    with pytest.raises(RuntimeError, match="x must be a 4-D float32 CUDA"):
        hip_lib.dwconv7x7_ln_backward(t["x"], t["weight"], t["bias"], t["gamma"], t["beta"], R.EPS, t["g"])
    with pytest.raises(RuntimeError, match="want must hold five flags"):
        hip_lib.dwconv7x7_ln_backward(t["x"], t["weight"], t["bias"], t["gamma"], t["beta"], R.EPS, t["g"], want=(False,) * 5)
