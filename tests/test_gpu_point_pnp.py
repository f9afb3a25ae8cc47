"""SimplePointPnPNet on the GPU (-m gpu), through the C ABI: gdrnpp_point_pnp_pool (point-wise MLP + max over the points on the
exact-f32 matrix instruction), gdrnpp_point_pnp_fc and the existing gdrnpp_pnp_fc_heads behind them.

References, none of them the code under test:
  * the reference's own forward, recorded in fp32 and fp64 (tests/golden/point_pnp_golden.npz);
  * for launch shapes without a fixture, the module path in fp64 on the CPU on the same tensors.
Bars: |ours - fp64| <= 4 * e_ref per output tensor, e_ref = max |fp32 reference - fp64 reference| (from the fixture, or from the
module path in fp32 against fp64 on the CPU for the same tensors): a different, equally long fp32 summation order plus
LeakyReLU / max picking a neighbouring value.  The tests print ours / e_ref."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import point_pnp_seeded as PS  # noqa: E402

from gdrnpp_bop2022_amd.gdrn_modeling import heads  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 4.0
TILE = 128


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "point_pnp_golden.npz"))


@pytest.fixture(scope="module")
def seeded_inputs(golden):
    inp = PS.inputs()
    assert PS.digest(inp) == str(golden["input_digest"]), "the seeded inputs differ from the ones the fixture was recorded on"
    return inp


def fixture_head(case):
    c = PS.CASES[case]
    net = heads.SimplePointPnPNet(PS.n_in(case), rot_dim=c["rot_dim"], mask_attention_type=c["mask_attention_type"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in PS.params(PS.n_in(case), c["rot_dim"]).items()}, strict=True)
    return net.eval()


def fixture_rows(case, inp, pitch):
    """The head's own concatenation for ``case`` as NHWC rows f32[b*hw, pitch]; the pad channels hold 7.0 (they must not be read)."""
    kw = {k: torch.from_numpy(v) for k, v in PS.case_inputs(case, inp).items()}
    cf = kw["coor_feat"]
    parts = [(cf[:, :3] - 0.5) * kw["extents"].view(-1, 3, 1, 1), cf[:, 3:]]
    if "region" in kw:
        parts.append(kw["region"])
    if "mask_attention" in kw:
        parts.append(kw["mask_attention"])
    x = torch.cat(parts, 1)                                  # [b, cin, h, w], the arithmetic of forward in fp32
    b, cin, h, w = x.shape
    rows = torch.full((b, h * w, pitch), 7.0)
    rows[:, :, :cin] = x.flatten(2).transpose(1, 2)
    return rows.reshape(b * h * w, pitch).contiguous(), b, h * w, cin


def run_pool(hip, head, rows, b, hw, cin, want_pooled=True):
    p = {k: v.detach().to(DEV) for k, v in head.state_dict().items()}
    return hip.point_pnp_pool(rows.to(DEV), cin, p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"],
                              p["conv3.weight"], p["conv3.bias"], b, hw, want_pooled=want_pooled)


def run_chain(hip, head, rows, b, hw, cin):
    """pool -> fc -> pnp_fc_heads: (pooled, rot, t) as CPU tensors."""
    p = {k: v.detach().to(DEV) for k, v in head.state_dict().items()}
    pooled, ws = run_pool(hip, head, rows, b, hw, cin)
    feat = hip.point_pnp_fc(ws, p["fc1.weight"], p["fc1.bias"], p["fc2.weight"], p["fc2.bias"], b, hw)
    rd = head.rot_dim
    w, bias = p["fc_pose.weight"], p["fc_pose.bias"]
    rot, t = hip.pnp_fc_heads(feat, w[:rd], bias[:rd], w[rd:rd + 3], bias[rd:rd + 3])
    torch.cuda.synchronize()
    return pooled.cpu(), rot.cpu(), t.cpu()


def check(tag, ours, ref64, e_ref):
    err = float((ours.double() - ref64).abs().max())
    print(f"{tag}: |ours - fp64| = {err:.3e} = {err / e_ref:.2f} e_ref (e_ref = {e_ref:.3e})")
    assert torch.isfinite(ours).all()
    assert err <= FACTOR * e_ref, (tag, err, e_ref)


def module_reference(head, rows, b, hw, cin, chunk=8):
    """The module path (PyTorch operators on the CPU) on the rows' first cin channels, in fp32 and in fp64:
    -> {name: (fp64 result, e_ref)} for pooled / rot / t.  ROIs in chunks: [chunk, 1024, hw] fp64 at a time."""
    x = rows.view(b, hw, -1)[:, :, :cin].transpose(1, 2)
    out = {}
    with torch.no_grad():
        for dtype in (torch.float32, torch.float64):
            net = heads.SimplePointPnPNet(cin, rot_dim=head.rot_dim)
            net.load_state_dict(head.state_dict())
            net = net.to(dtype).eval()
            pooled = []
            net.conv3.register_forward_hook(lambda m, i, o: pooled.append(o.max(dim=2)[0]))
            parts = [net.mlp_tail(x[i:i + chunk].to(dtype)) for i in range(0, b, chunk)]
            out[dtype] = dict(pooled=torch.cat(pooled), rot=torch.cat([p[0] for p in parts]), t=torch.cat([p[1] for p in parts]))
    return {k: (out[torch.float64][k], float((out[torch.float32][k].double() - out[torch.float64][k]).abs().max())) for k in ("pooled", "rot", "t")}


@pytest.mark.parametrize("case,pitch", [("rot6", 96), ("rot4", 96), ("concat", 32)])
def test_pool_against_the_reference_forward(hip, golden, seeded_inputs, case, pitch):
    head = fixture_head(case)
    rows, b, hw, cin = fixture_rows(case, seeded_inputs, pitch)
    pooled, _ = run_pool(hip, head, rows, b, hw, cin)
    torch.cuda.synchronize()
    check(f"{case} pooled", pooled.cpu(), torch.from_numpy(golden[f"{case}/pooled64"]), float(golden[f"{case}/e_ref_pooled"]))


@pytest.mark.parametrize("case,pitch", [("rot6", 96), ("rot4", 96), ("concat", 32)])
def test_pool_fc_heads_chain_against_the_reference_forward(hip, golden, seeded_inputs, case, pitch):
    head = fixture_head(case)
    rows, b, hw, cin = fixture_rows(case, seeded_inputs, pitch)
    _, rot, t = run_chain(hip, head, rows, b, hw, cin)
    check(f"{case} rot", rot, torch.from_numpy(golden[f"{case}/rot64"]), float(golden[f"{case}/e_ref_rot"]))
    check(f"{case} t", t, torch.from_numpy(golden[f"{case}/t64"]), float(golden[f"{case}/e_ref_t"]))


def random_case(b, hw, pitch, cin, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    head = heads.SimplePointPnPNet(cin, rot_dim=6).eval()
    rows = torch.rand((b * hw, pitch), generator=g)
    return head, rows


@pytest.mark.parametrize("b,hw,pitch,cin", [(1, 4096, 96, 69), (3, 4096, 96, 69), (8, 4096, 96, 69), (128, 4096, 96, 69),
                                            (3, 1024, 96, 69), (1, 1024, 32, 6), (8, 4096, 32, 6), (128, 1024, 32, 6)])
def test_launch_shapes_against_the_module_path_in_fp64(hip, b, hw, pitch, cin):
    head, rows = random_case(b, hw, pitch, cin, 1000 * b + hw + cin)
    ref = module_reference(head, rows, b, hw, cin)
    pooled, rot, t = run_chain(hip, head, rows, b, hw, cin)
    for name, ours in (("pooled", pooled), ("rot", rot), ("t", t)):
        check(f"b={b} hw={hw} pitch={pitch} cin={cin} {name}", ours, *ref[name])


def test_two_launches_and_a_side_stream_are_bit_equal(hip):
    head, rows = random_case(8, 4096, 96, 69, 7)
    a = run_chain(hip, head, rows, 8, 4096, 69)
    b_ = run_chain(hip, head, rows, 8, 4096, 69)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = run_chain(hip, head, rows, 8, 4096, 69)
    s.synchronize()
    for x, y, z in zip(a, b_, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_maximum_negative_everywhere(hip):
    """conv3 outputs near -5 at every point of every tile: a running max that starts from zero would return zeros."""
    head, rows = random_case(3, 1024, 96, 69, 11)
    with torch.no_grad():
        head.conv3.weight.mul_(0.01)
        head.conv3.bias.fill_(-5.0).add_(torch.linspace(0, 1, 1024))
    ref = module_reference(head, rows, 3, 1024, 69)
    assert float(ref["pooled"][0].max()) < -3.5
    pooled, rot, t = run_chain(hip, head, rows, 3, 1024, 69)
    assert float(pooled.max()) < -3.5
    for name, ours in (("pooled", pooled), ("rot", rot), ("t", t)):
        check(f"negative {name}", ours, *ref[name])


def test_maximum_in_the_last_point_of_the_last_tile(hip):
    b, hw, cin = 2, 1024, 69
    head, rows = random_case(b, hw, 96, cin, 13)
    rows = rows.view(b, hw, 96).clone()
    rows[1, hw - 1, :cin] *= 40.0              # the last point of ROI 1 dominates wherever its response is positive
    rows = rows.view(b * hw, 96)
    x = rows.view(b, hw, 96)[:, :, :cin].transpose(1, 2).double()
    with torch.no_grad():
        net = heads.SimplePointPnPNet(cin).double()
        net.load_state_dict(head.state_dict())
        y = net.conv3(net.act(net.conv2(net.act(net.conv1(x)))))
    at_last = (y[1].argmax(dim=1) == hw - 1)
    assert int(at_last.sum()) > 200, int(at_last.sum())
    ref = module_reference(head, rows, b, hw, cin)
    pooled, rot, t = run_chain(hip, head, rows, b, hw, cin)
    for name, ours in (("pooled", pooled), ("rot", rot), ("t", t)):
        check(f"last point {name}", ours, *ref[name])
    e = float((pooled[1].double() - ref["pooled"][0][1])[at_last].abs().max())
    assert e <= FACTOR * ref["pooled"][1]


def test_argument_errors_launch_nothing(hip):
    lib = hip.load()
    b, hw, pitch, cin = 2, 256, 96, 69
    head, rows = random_case(b, hw, pitch, cin, 17)
    p = {k: v.detach().to(DEV).contiguous() for k, v in head.state_dict().items()}
    x = rows.to(DEV)
    need = lib.gdrnpp_point_pnp_workspace_bytes(b, hw)
    assert need == b * (hw // TILE) * 1024 * 4
    for bad in ((0, hw), (-1, hw), (b, 0), (b, hw + 1), (b, 4000)):
        assert lib.gdrnpp_point_pnp_workspace_bytes(*bad) == 0
    SENT = -777.0
    ws = torch.full((need // 4,), SENT, device=DEV)
    pooled = torch.full((b, 1024), SENT, device=DEV)
    feat = torch.full((b, 256), SENT, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    W = [P(p[k]) for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias")]

    def pool(x_=P(x), pitch_=pitch, cin_=cin, w=W, pooled_=P(pooled), b_=b, hw_=hw, ws_=P(ws), nbytes=need):
        return lib.gdrnpp_point_pnp_pool(x_, pitch_, cin_, *w, pooled_, b_, hw_, ws_, nbytes, None)

    cases = {"null x": dict(x_=None), "null workspace": dict(ws_=None), "null w3": dict(w=W[:4] + [None, W[5]]),
             "null b1": dict(w=[W[0], None] + W[2:]), "b = 0": dict(b_=0), "b < 0": dict(b_=-3), "hw not a tile multiple": dict(hw_=hw - 64),
             "hw = 0": dict(hw_=0), "cin > pitch": dict(cin_=pitch + 1), "pitch % 32": dict(pitch_=80), "cin = 0": dict(cin_=0),
             "small workspace": dict(nbytes=need - 4)}
    for what, kw in cases.items():
        rc = pool(**kw)
        msg = lib.gdrnpp_last_error()
        assert rc < 0 and msg and b"gdrnpp_point_pnp_pool" in msg, (what, rc, msg)
    assert lib.gdrnpp_point_pnp_pool(P(x), 160, 129, *W, P(pooled), b, hw, P(ws), need, None) == -2     # above the kernel's 128 channels
    F = [P(p[k]) for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")]

    def fc(ws_=P(ws), nbytes=need, w=F, feat_=P(feat), b_=b, hw_=hw):
        return lib.gdrnpp_point_pnp_fc(ws_, nbytes, *w, feat_, b_, hw_, None)

    for what, kw in {"null workspace": dict(ws_=None), "null feat": dict(feat_=None), "null fc2 bias": dict(w=F[:3] + [None]),
                     "b = 0": dict(b_=0), "hw not a tile multiple": dict(hw_=hw + 32), "small workspace": dict(nbytes=need - 4)}.items():
        rc = fc(**kw)
        msg = lib.gdrnpp_last_error()
        assert rc < 0 and msg and b"gdrnpp_point_pnp_fc" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    for t in (ws, pooled, feat):
        assert bool((t == SENT).all())
    # and the same buffers with good arguments are written
    assert pool() == 0 and fc() == 0
    torch.cuda.synchronize()
    for t in (ws, pooled, feat):
        assert bool((t != SENT).all())


def test_whole_model_hip_path_against_module_path(hip):
    """GDRN_DoubleMask with the point head: the fused NHWC tail feeds forward_prepared (three launches of this library) — against
    the module path on the same weights and batch: R / t within the project's 1e-4, no fallback launch, two steps may share."""
    from gdrnpp_bop2022_amd import synthetic as S
    from gdrnpp_bop2022_amd.gdrn_modeling import engine, hip_layers
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import build_model_optimizer

    cfg = get_cfg("ycbv_convnext_a6", ["MODEL.POSE_NET.PNP_NET.INIT_CFG={'type': 'SimplePointPnPNet'}"])
    torch.manual_seed(0)
    model, _ = build_model_optimizer(cfg)
    assert type(model.pnp_net) is heads.SimplePointPnPNet
    with torch.no_grad():
        model.pnp_net.fc_pose.bias[6:].copy_(torch.tensor([0.0, 0.0, 4.0]))
        for m in model.modules():  # make layer-scale / out layer non-trivial so differences would show
            if hasattr(m, "gamma") and isinstance(m.gamma, torch.nn.Parameter):
                m.gamma.fill_(0.3)
        torch.nn.init.normal_(model.geo_head_net.out_layer.weight, 0, 0.05)
    b = 8
    rng = np.random.default_rng(8)
    _, _, ext = S.make_models(21, rng, subdiv=1)
    det = S.make_detections(b, 21, ext, rng)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)     # noqa: E731
    g = torch.Generator().manual_seed(5)
    x = torch.rand((b, 3, 256, 256), generator=g).to(DEV)
    args = dict(roi_classes=T(det["roi_cls"]), roi_cams=T(det["roi_cam"]), roi_whs=T(det["roi_wh"]), roi_centers=T(det["roi_center"]),
                resize_ratios=T(det["resize_ratio"]), roi_coord_2d=T(S.coord2d_roi(det["roi_center"], det["scale"])),
                roi_extents=T(det["roi_extent"]))
    assert hip_layers.is_enabled() and engine.default_compute_streams(model) == 2
    with torch.no_grad():
        model(x, **args)                      # fills the derived-weight caches
        n0 = hip_layers.fallback_launches()
        o1 = model(x, **args)
        assert hip_layers.fallback_launches() == n0, hip_layers.last_fallback()
        hip_layers.set_enabled(False)
        try:
            o2 = model(x, **args)
        finally:
            hip_layers.set_enabled(True)
    torch.cuda.synchronize()
    assert torch.isfinite(o1["rot"]).all() and torch.isfinite(o1["trans"]).all()
    print("rot", float((o1["rot"] - o2["rot"]).abs().max()), "trans", float((o1["trans"] - o2["trans"]).abs().max()))
    torch.testing.assert_close(o1["rot"], o2["rot"], rtol=0, atol=1e-4)
    torch.testing.assert_close(o1["trans"], o2["trans"], rtol=0, atol=1e-4)
