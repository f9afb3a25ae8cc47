"""The fp64 restatement of the geometry head's backward (tests/conv_gn_bwd_ref.py) against torch.autograd, and the parts of the feature
that need no device: the entry points in the parsed header and the built library, the workspace queries, the row plan of the case
table, the wrappers' refusals, and the train switch on CPU tensors."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_gn_bwd_ref as R  # noqa: E402

ENTRY_POINTS = ("gdrnpp_groupnorm_stats_nhwc", "gdrnpp_groupnorm_act_backward", "gdrnpp_groupnorm_act_backward_workspace_bytes",
                "gdrnpp_conv3x3_wgrad_f32", "gdrnpp_conv3x3_wgrad_f32_workspace_bytes", "gdrnpp_upsample_bilinear2x_backward_nhwc",
                "gdrnpp_deconv_im2col_nhwc")


def _close(a, b, name):
    assert a.shape == b.shape and a.dtype == torch.float64 == b.dtype, name
    err, top = float((a - b).abs().max()), float(b.abs().max())
    assert err <= 1e-12 * top, (name, err, top)


@pytest.mark.parametrize("case", R.LAYER_CASES, ids=R.case_id)
def test_layer_restatement_matches_fp64_autograd(case):
    t = R.layer_inputs(case)
    args = (t["x"], t["w"], t["gamma"], t["beta"], case[5], 1e-5, case[6], t["g"])
    got, want = R.layer_restated(*args), R.layer_autograd(*args, torch.float64)
    for name in ("y",) + R.NAMES:
        _close(got[name], want[name], name)


@pytest.mark.parametrize("gelu", (False, True), ids=("plain", "gelu"))
@pytest.mark.parametrize("case", R.GN_CASES, ids=R.case_id)
def test_groupnorm_restatement_matches_fp64_autograd(case, gelu):
    t = R.gn_inputs(case)
    got = R.gn_restated(t["z"], t["gamma"], t["beta"], case[4], 1e-5, gelu, t["g"])
    want, _ = R.gn_references(case, gelu)
    for name in ("y", "dz", "dgamma", "dbeta"):
        _close(got[name], want[name], name)


@pytest.mark.parametrize("case", R.UP_CASES, ids=R.case_id)
def test_upsample_restatement_matches_fp64_autograd(case):
    t = R.up_references(case)
    y, dx = R.up_restated(t["x"], t["g"])
    _close(y, t["ref64"]["y"], "y")
    _close(dx, t["ref64"]["dx"], "dx")
    if case[1] == case[2] == 1:      # scale 0: all four outputs copy the input
        assert torch.equal(dx, t["g"].double().sum((2, 3), keepdim=True))


@pytest.mark.parametrize("case", R.DECONV_CASES, ids=R.case_id)
def test_deconv_restatement_matches_fp64_autograd(case):
    t = R.deconv_references(case)
    dx, dw = R.deconv_restated(t["x"], t["w"], t["dy"], case[5], case[6])
    _close(dx, t["ref64"]["dx"], "dx")
    _close(dw, t["ref64"]["dw"], "dw")


def test_convolution_gradients_restated():
    c = R.conv_random((1, 4, 5, 128, 128))
    _close(R.wgrad64(c["dz"], c["x"]), c["ref64"]["dw"], "dw")
    _close(R.dx64(c["dz"], c["w"]), c["ref64"]["dx"], "dx")
    dz, x, want = R.wgrad_lattice(R.WGRAD_EXACT[0])
    assert bool((want[:, :, 1, 1] != 0).any()) and not bool(want[:, :, [0, 0, 0, 1, 1, 2, 2, 2], [0, 1, 2, 0, 2, 0, 1, 2]].any())


def test_case_tables_cover_every_mechanism():
    rows = {c: c[0] * c[1] * c[2] for c in R.WGRAD_EXACT}
    plans = {c: R.wgrad_slots(rows[c], c[3], c[4]) for c in R.WGRAD_EXACT}
    assert plans[(1, 24, 24, 128, 128)] == (2, 512) and 512 % 24            # the chunk ends mid image row
    assert plans[(3, 16, 16, 256, 128)] == (2, 512) and 256 < R.WG_CHUNK <= 2 * 256   # the first chunk holds image 0 and image 1
    big = R.WGRAD_BIG
    assert -(-rows[big] // R.WG_CHUNK) == 58 > 56 == R.WG_GRID // 9 and plans[big] == (29, 1024) and rows[big] - 28 * 1024 == 912
    assert rows[big] * 64 < 2 ** 24
    assert R.wgrad_slots(48 * 4096, 256, 256) == (14, 14336)                 # the head's layer at 48 ROIs: 36 x 14 = 504 workgroups
    assert {c[3] > 128 for c in R.WGRAD_EXACT} == {False, True} == {c[4] > 128 for c in R.WGRAD_EXACT}
    assert {g for *_, g in R.GN_CASES} == {16, 32} and any(c[1] * c[2] >= 1024 for c in R.GN_CASES) and any(c[1] * c[2] == 1 for c in R.GN_CASES)


def test_header_and_library_declare_the_entry_points():
    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.hip_lib import abi

    lib = hip_lib.load()
    for name in ENTRY_POINTS:
        assert name in abi.SIGNATURES, name
        assert hasattr(lib, name), name
        res, args = abi.SIGNATURES[name]
        if name.endswith("_bytes"):
            assert res is abi.c_size_t
        else:
            assert res is abi.c_int and args[-1] is abi.c_void_p, name
    assert len(abi.DEFINES) == 14
    for name in ("conv3x3_wgrad_f32", "conv3x3_f32_mfma", "conv3x3_backward", "groupnorm_act_backward", "groupnorm_act_train",
                 "upsample_bilinear2x_backward", "deconv_im2col", "conv_transpose2d_backward"):
        assert callable(getattr(hip_lib, name)), name


def test_workspace_queries_return_zero_outside_the_kernels():
    from gdrnpp_bop2022_amd import hip_lib

    lib = hip_lib.load()
    wg, gn = lib.gdrnpp_conv3x3_wgrad_f32_workspace_bytes, lib.gdrnpp_groupnorm_act_backward_workspace_bytes
    for n, h, w, cin, cout in R.WGRAD_EXACT:
        assert wg(n, h, w, cin, cout) == R.wgrad_slots(n * h * w, cin, cout)[0] * 9 * cin * cout * 8
    assert wg(1, 4, 4, 64, 128) == 0 and wg(1, 4, 4, 128, 192) == 0 and wg(0, 4, 4, 128, 128) == 0 and wg(1, 4, -1, 128, 128) == 0
    assert gn(1, 16, 130, 13) == 0 and gn(1, 16, 128, 64) == 0 and gn(1, 16, 2048, 32) == 0 and gn(0, 16, 128, 16) == 0 and gn(1, 16, 128, 24) == 0
    assert gn(2, 1089, 128, 16) == (2 * 35 * 2 * 128 + 2 * 2 * 128 + 2 * 16 * 2) * 8


def test_wrappers_refuse_before_the_library_is_touched():
    from gdrnpp_bop2022_amd import hip_lib

    z = torch.zeros(1, 128, 2, 2).contiguous(memory_format=torch.channels_last)
    part = torch.zeros(1, 1, 16, 2, dtype=torch.float64)
    g = torch.ones(128)
    with pytest.raises(RuntimeError, match="want must hold three flags"):
        hip_lib.groupnorm_act_backward(z, part, g, g, 16, 1e-5, True, z, want=(False,) * 3)
    with pytest.raises(RuntimeError, match="must be a 4-D float32 CUDA"):
        hip_lib.groupnorm_act_backward(z, part, g, g, 16, 1e-5, True, z)
    with pytest.raises(RuntimeError, match="want must hold three flags"):
        hip_lib.conv3x3_backward(z, torch.zeros(128, 128, 3, 3), z, want=(False, False))
    with pytest.raises(ValueError, match="float32 channels_last device tensor"):
        hip_lib.conv3x3_wgrad_f32(z, z)
    with pytest.raises(ValueError, match="float32 channels_last device tensor"):
        hip_lib.conv3x3_f32_mfma(z, torch.zeros(9 * 128, 128))
    with pytest.raises(RuntimeError, match="must be a 4-D float32 CUDA"):
        hip_lib.upsample_bilinear2x_backward(z)


def test_train_switch_changes_nothing_on_the_cpu():
    from gdrnpp_bop2022_amd.gdrn_modeling import heads, hip_layers

    torch.manual_seed(0)
    features = torch.nn.ModuleList([torch.nn.UpsamplingBilinear2d(scale_factor=2),
                                    heads.ConvModule(128, 128, 3, padding=1, norm="GN", num_gn_groups=16, act="GELU")])
    x = torch.randn(1, 128, 2, 2, requires_grad=True)

    def nodes(y):
        seen, todo = set(), [y.grad_fn]
        while todo:
            fn = todo.pop()
            if fn is not None and fn not in seen:
                seen.add(fn)
                todo.extend(f for f, _ in fn.next_functions)
        return {type(fn).__name__ for fn in seen}

    want = heads.run_features(features, x)
    hip_layers.set_train_kernels(True)
    try:
        got = heads.run_features(features, x)      # CPU tensors: the switch does not apply
    finally:
        hip_layers.set_train_kernels(False)
    assert torch.equal(got, want) and nodes(got) == nodes(want)
    assert {"ConvolutionBackward0", "NativeGroupNormBackward0", "GeluBackward0", "UpsampleBilinear2DBackward0"} <= nodes(got)
    for name in ("Conv3x3GnAct", "GroupNormAct", "Upsample2x", "ConvTranspose2dGn"):
        assert issubclass(getattr(hip_layers, name), torch.autograd.Function), name
