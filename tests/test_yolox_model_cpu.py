"""The YOLOX detector modules (gdrnpp_bop2022_amd/det/yolox/models) without a GPU: the parameter names are the reference's, and
the plain-PyTorch module path reproduces the reference's own forward on the seeded fixtures
(tests/golden/yolox_net_golden_<case>.npz, written by tests/golden/make_golden_yolox_net.py from the reference's modules).

Bars: per output group (box centre, box size in pixels, objectness, class scores) |ours - reference fp64| <= 4 * e_ref with
e_ref = max |reference fp32 - reference fp64| from the fixture — the margin this project grants another summation order."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import yolox_seeded as YS  # noqa: E402

from gdrnpp_bop2022_amd.det.yolox import models as M  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers  # noqa: E402

FACTOR = 4.0


def load_golden(case):
    g = np.load(os.path.join(GOLDEN, f"yolox_net_golden_{case}.npz"))
    assert int(g["param_seed"]) == YS.PARAM_SEED and int(g["input_seed"]) == YS.INPUT_SEED
    return g


def build(case):
    c = YS.CASES[case]
    net = M.build_yolox(c["depth"], c["width"], c["num_classes"])
    net.load_state_dict(YS.state_dict_for(net), strict=True)
    return net.eval()


def check_against_fixture(det, g, case, what):
    """det f32[B,A,5+C] (numpy) against the fixture's fp64 rows; prints every ratio before asserting."""
    rows = g[f"{case}/rows"]
    want = g[f"{case}/det64"]
    got = det[:, rows].astype(np.float64)
    assert got.shape == want.shape
    ratios = {}
    for name, sl in YS.GROUPS.items():
        e_ref = float(g[f"{case}/e_ref_{name}"])
        err = float(np.abs(got[..., sl] - want[..., sl]).max())
        ratios[name] = err / e_ref
        print(f"{what} {case} {name}: max |ours - ref fp64| = {err:.3e} = {err / e_ref:.2f} x e_ref ({e_ref:.3e})")
    for name, r in ratios.items():
        assert r <= FACTOR, (what, case, name, r)
    return ratios


@pytest.mark.parametrize("case", ["s256x384", "x320"])
def test_state_dict_manifest_is_the_references_and_the_seeded_dict_loads_strictly(case):
    g = load_golden(case)
    c = YS.CASES[case]
    net = M.build_yolox(c["depth"], c["width"], c["num_classes"])
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in g[f"{case}/keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[f"{case}/shapes"]]
    assert len(sd) == {"s256x384": 462, "x320": 894}[case]
    seeded = YS.state_dict_for(net)
    assert YS.digest(seeded) == str(g[f"{case}/param_digest"]), "the seeded parameters differ from the ones the fixture was recorded on"
    net.load_state_dict(seeded, strict=True)


@pytest.mark.parametrize("case", list(YS.CASES))
def test_module_path_forward_is_within_the_bar_of_the_reference(case):
    g = load_golden(case)
    net = build(case)
    x = YS.image(case)
    assert YS.digest({"x": x}) == str(g[f"{case}/input_digest"])
    with torch.no_grad():
        out = net(x)
    assert set(out) == {"det_preds"} and out["det_preds"].dtype == torch.float32
    b, _, h, w = x.shape
    assert out["det_preds"].shape == (b, (h // 8) * (w // 8) + (h // 16) * (w // 16) + (h // 32) * (w // 32), 5 + 21)
    check_against_fixture(out["det_preds"].numpy(), g, case, "module path (CPU)")


def test_fixture_records_ranges_that_make_the_comparison_mean_something():
    for case in YS.CASES:
        g = load_golden(case)
        assert np.abs(g[f"{case}/range_raw_wh"]).max() <= 4.0
        for name in ("obj", "cls"):
            lo, hi = g[f"{case}/range_{name}"]
            assert np.log(hi / (1 - hi)) - np.log(lo / (1 - lo)) > 3.0
    assert len(load_golden("x320")["conv_shapes"]) == 26


def test_batchnorm_eps_and_momentum_are_set_on_every_batchnorm():
    net = M.build_yolox(0.33, 0.5, 3)
    bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(bns) > 50 and all(m.eps == 1e-3 and m.momentum == 0.03 for m in bns)
    for conv in list(net.head.cls_preds) + list(net.head.obj_preds):       # prior probability 0.01
        assert torch.allclose(conv.bias.detach().sigmoid(), torch.full_like(conv.bias, 0.01), atol=1e-6)


def test_unsupported_options_raise_not_implemented_naming_the_option():
    with pytest.raises(NotImplementedError, match="depthwise"):
        M.YOLOPAFPN(0.33, 0.5, depthwise=True)
    with pytest.raises(NotImplementedError, match="depthwise"):
        M.YOLOXHead(3, 0.5, depthwise=True)
    net = M.build_yolox(0.33, 0.5, 3)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="augment"):
        net(x, augment=True)
    with pytest.raises(NotImplementedError, match="training"):
        net(x, targets=torch.zeros(1, 1, 5))
    net.train()
    with pytest.raises(NotImplementedError, match="training"):
        net(x)


def test_undecoded_output_decoded_by_hand_equals_det_preds():
    net = build("s256x384")
    x = YS.image("s256x384")
    with torch.no_grad():
        det = net(x)["det_preds"]
        net.head.decode_in_inference = False
        raw = net(x)
    assert isinstance(raw, torch.Tensor) and raw.shape == det.shape
    rows = []
    for s in (8, 16, 32):
        h, w = 256 // s, 384 // s
        for y in range(h):
            for xx in range(w):
                rows.append((xx, y, s))
    grid = torch.tensor(rows, dtype=torch.float32)
    want = raw.clone()
    want[..., 0] = (raw[..., 0] + grid[:, 0]) * grid[:, 2]
    want[..., 1] = (raw[..., 1] + grid[:, 1]) * grid[:, 2]
    want[..., 2:4] = torch.exp(raw[..., 2:4]) * grid[:, 2:3]
    assert torch.equal(want, det)


def test_folded_conv_bn_of_a_baseconv_with_eps_1e_3_equals_bn_of_conv_in_fp64():
    torch.manual_seed(3)
    m = M.BaseConv(16, 24, 3, 2)
    m.bn.eps = 1e-3
    with torch.no_grad():
        m.bn.weight.uniform_(0.5, 1.5)
        m.bn.bias.uniform_(-1, 1)
        m.bn.running_mean.uniform_(-1, 1)
        m.bn.running_var.uniform_(0.002, 0.02)       # of the order of eps: a fold that ignored eps would be far off
    m = m.eval()
    w, b = hip_layers.folded_conv_bn(m.conv, m.bn)
    x = torch.randn(2, 16, 9, 11, dtype=torch.float64)
    m64 = M.BaseConv(16, 24, 3, 2).double().eval()
    m64.bn.eps = 1e-3
    m64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    with torch.no_grad():
        want = m64.bn(m64.conv(x))
        got = torch.nn.functional.conv2d(x, w.double(), b.double(), 2, 1)
    assert (got - want).abs().max() <= 1e-6 * want.abs().max()


def test_space_to_depth_order():
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).view(2, 3, 4, 6)
    y = M.network_blocks.space_to_depth(x)
    assert torch.equal(y[:, 0:3], x[..., ::2, ::2]) and torch.equal(y[:, 3:6], x[..., 1::2, ::2])
    assert torch.equal(y[:, 6:9], x[..., ::2, 1::2]) and torch.equal(y[:, 9:12], x[..., 1::2, 1::2])
