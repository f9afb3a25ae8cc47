"""The fp64 restatement of the ConvNeXt MLP backward (tests/mlp_bwd_ref.py), the dgamma identity included, against torch.autograd;
and the parts of the feature that need no device: the entry points in the parsed header, the row plans, the wrappers' refusals."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_bwd_ref as R  # noqa: E402

ENTRY_POINTS = ("gdrnpp_gemm_tn_f32", "gdrnpp_gemm_tn_f32_workspace_bytes", "gdrnpp_gelu_f32", "gdrnpp_mlp_bwd_act", "gdrnpp_colsum_f32",
                "gdrnpp_colsum_workspace_bytes", "gdrnpp_pack_weight_bf16x3_t", "gdrnpp_linear_f32_exact",
                "gdrnpp_linear_f32_exact_workspace_bytes")


@pytest.mark.parametrize("gamma_scale", (None, 1e-6), ids=("gamma_o1", "gamma_1e-6"))
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_matches_fp64_autograd(case, gamma_scale):
    t = R.make_inputs(case, gamma_scale)
    got = R.restated_backward(t["x"], t["s"], t["w1"], t["b1"], t["w2"], t["b2"], t["gamma"], t["g"])
    want, _ = R.references(case, gamma_scale)
    for name in ("y", "ds") + R.NAMES:
        a, b = got[name], want[name]
        assert a.shape == b.shape and a.dtype == torch.float64 == b.dtype, name
        err = float((a - b).abs().max())
        assert err <= 1e-12 * float(b.abs().max()), (name, err, float(b.abs().max()))


def test_dgamma_identity_needs_no_z():
    """dgamma = sum_m g z, with z = h W2^T + b2 written out, equals rowsum(W2 * (g^T h)) + b2 * colsum(g)."""
    t = {k: v.double() for k, v in R.make_inputs(R.CASES[2]).items()}
    got = R.restated_backward(t["x"], t["s"], t["w1"], t["b1"], t["w2"], t["b2"], t["gamma"], t["g"])
    z = got["h"] @ t["w2"].t() + t["b2"]
    direct = (t["g"] * z).sum(0)
    assert float((got["dgamma"] - direct).abs().max()) <= 1e-12 * float(direct.abs().max())


def test_header_declares_the_entry_points():
    from gdrnpp_bop2022_amd.hip_lib import abi

    for name in ENTRY_POINTS:
        assert name in abi.SIGNATURES, name
        res, args = abi.SIGNATURES[name]
        if name.endswith("_bytes"):
            assert res is abi.c_size_t
        else:
            assert res is abi.c_int and args[-1] is abi.c_void_p, name
    assert abi.SIGNATURES["gdrnpp_gemm_tn_f32"][1][3:6] == [abi.c_int] * 3
    assert len(abi.DEFINES) == 14


def test_case_tables_cover_every_mechanism():
    assert {R.tn_slots(m)[0] for m in R.TN_M} >= {1, 2, 3, 33}
    big = R.TN_M[-1]
    assert -(-big // R.TN_CHUNK) > R.TN_SLOT_CAP and R.tn_slots(big) == (33, 1024)       # more chunks than slots: two chunks per slot
    assert R.tn_slots(R.TN_CHUNK) == (1, 512) and R.tn_slots(R.TN_CHUNK + 1) == (2, 512) and R.tn_slots(64 * 512) == (64, 512)
    # a wide result fills the chip with fewer slots: 16 tiles take at most 32, and the large M walks three chunks per slot there
    assert R.tn_slots(big, 256, 1024) == (22, 1536) and R.tn_slots(2 * R.TN_CHUNK + 1, 256, 1024) == (3, 512)
    assert R.tn_slots(3072, 1024, 4096) == (2, 1536) and R.tn_slots(196608, 128, 512) == (64, 3072)
    assert all(m % R.TN_STAGE for m in R.TN_M if m not in (32, R.TN_CHUNK)) and {31, 32, 33} <= set(R.TN_M)
    assert {(n1 > 128, n2 > 128) for n1, n2 in R.TN_SHAPES} == {(False, False), (False, True), (True, False), (True, True)}
    ms = [m for m, _ in R.CASES]
    assert min(ms) == 1 and any(32 < m < 64 for m in ms)                                  # one row; a partial second staging block
    assert any(R.col_slots(m)[0] > 1 and m % R.col_slots(m)[1] for m in ms)               # several column-sum slots, the last one short
    assert any(R.tn_slots(m)[0] > 2 for m in ms) and {c for _, c in R.CASES} == {128, 256}
    assert R.col_slots(1) == (1, 1) and R.col_slots(64 * 256 + 1) == (253, 65)
    # the exact forward-shaped product: one stage, three depth slots with a short last one, eight slots, and one slot past a chain
    assert [R.rows_slots(257, n, k) for n, k in R.EXACT_NK] == [(1, 128), (3, 128), (8, 128)]
    assert R.rows_slots(*R.EXACT_ONE_SLOT) == (1, 384) and R.rows_slots(512, 1024, 4096) == (8, 512) and R.rows_slots(196608, 128, 512) == (1, 512)
    a, b = R.tn_lattice(33, 128, 128)
    assert float(a.abs().max()) <= 8 and float(b.abs().max()) <= 8
    a, b = R.tn_onehot(R.TN_M[-1], 128, 128)
    assert float((a.double().t() @ b.double()).max()) < 2 ** 24 and bool((a.sum(1) == 1).all())


def test_bar_is_twice_the_fp32_error_plus_one_ulp():
    ref64 = torch.tensor([1.0, -3.0], dtype=torch.float64)
    ref32 = torch.tensor([1.0, -3.0 + 2.0 ** -20], dtype=torch.float32)
    assert R.bar(ref64, ref32) == 2.0 * 2.0 ** -20 + 2.0 ** -22
    assert R.ratio_to_bar(ref64.float(), ref64, ref32) == 0.0


def test_train_switch_changes_nothing_on_the_cpu():
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import ConvNeXtBlock

    torch.manual_seed(0)
    block = ConvNeXtBlock(128)
    x = torch.randn(1, 128, 3, 3, requires_grad=True)
    want = block(x)
    hip_layers.set_train_kernels(True)
    try:
        got = block(x)      # CPU tensors: the switch does not apply
    finally:
        hip_layers.set_train_kernels(False)
    assert torch.equal(got, want) and type(got.grad_fn).__name__ == type(want.grad_fn).__name__
    assert issubclass(hip_layers.ConvNeXtMlp, torch.autograd.Function)


def test_wrappers_refuse_before_the_library_is_touched():
    from gdrnpp_bop2022_amd import hip_lib

    t = R.make_inputs(R.CASES[1])
    args = (t["x"], torch.zeros(50, 512), t["w1"], t["w2"], t["b2"], t["gamma"], t["g"])
    with pytest.raises(RuntimeError, match="want must hold six flags"):
        hip_lib.convnext_mlp_backward(*args, want=(False,) * 6)
    with pytest.raises(RuntimeError, match="do not fit"):
        hip_lib.convnext_mlp_backward(t["x"], torch.zeros(50, 256), *args[2:])
    with pytest.raises(RuntimeError, match="must be a CUDA"):
        hip_lib.convnext_mlp_backward(*args)
    with pytest.raises(RuntimeError, match="b must have the 50 rows of a"):
        hip_lib.gemm_tn_f32(t["x"], t["x"][:49])
    with pytest.raises(RuntimeError, match="nothing asked for"):
        hip_lib.gemm_tn_f32(t["x"], t["x"], want_g=False)
