"""Patch-PnP trained on the HIP kernels (csrc/pnp_bwd.hip; hip_layers.Conv3x3S2GnAct, FlattenNCHW, LinearGelu, PnPHeads) against fp64
autograd on the CPU (tests/pnp_bwd_ref.py).

The bar, per tensor: max|hip - ref64| <= 2 max|torch fp32 on the CPU - ref64| + 1 ulp of max|ref64| (tests/mlp_bwd_ref.py); every test
prints its worst ratio to that bar.  The stride-2 weight gradient and data gradient are also held EXACT on integer lattices and
one-hot locator probes.

Measured on an MI355X, error / bar:
    case (N, H, W, Cin / pitch, Cout)        z       dx      dW
        (1, 4, 4, 128 / 128, 128)            0.12    0.45    0.34
        (3, 8, 8, 69 / 96, 128)              0.23    0.29    0.44
        (2, 8, 16, 128 / 128, 128)           0.37    0.32    0.43
        (5, 32, 32, 69 / 96, 128)            0.22    0.24    0.10
        (2, 64, 64, 69 / 96, 128)            0.19    0.15    0.13      the real first layer, x at the real input's scale
        (1, 8, 8, 128 / 128, 256)            0.31    0.43    0.41
    the fc tail 8192 -> 1024 -> 256 -> (6, 3), worst of h1, h2, rot, t and the nine gradients: B = 1 0.21, B = 3 0.25, B = 8 0.50
    ConvPnPNet alone (B = 3, 16 x 16): rot 0.21, t 0.17, the input's gradient 0.19, every parameter 0.11 .. 0.20
    the small GDRN_DoubleMask through forward(do_loss=True) + backward: loss 0.20, Patch-PnP's parameters 0.26 .. 0.51 but fc_t.bias 0.93
    (three numbers, each the fp64 sum of five gradients that the loss kernels hand over), the other parameters 0.08 .. 0.32
The flatten round trip is bit-equal; both convolution gradients are EXACT on the integer lattices and the locator probes of all six cases.
The training forward (fp32-MFMA convolutions) is not the inference forward (six-product convolutions) bit for bit, as in Conv3x3GnAct;
under no_grad the inference kernels run and the switch changes no bit.
"""
import copy
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_bwd_ref as R  # noqa: E402
from mlp_bwd_ref import bar, ratio_to_bar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _tail(t, pad=4096):
    """``t`` as the head of a flat device allocation with NaN behind its end: a read past the tensor poisons the result."""
    t = t.contiguous()
    buf = torch.full((t.numel() + pad,), NAN, device=DEV, dtype=t.dtype) if t.is_floating_point() else torch.zeros(t.numel() + pad, device=DEV, dtype=t.dtype)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf[:t.numel()].view(t.shape)


def _pitched(x_nchw, pitch, fill=NAN):
    """[N,C,H,W] -> a channels_last device tensor [N,pitch,H,W] with ``fill`` in the padding channels and NaN behind the end."""
    n, c, h, w = x_nchw.shape
    full = torch.full((n, h, w, pitch), fill)
    full[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return _tail(full).permute(0, 3, 1, 2)


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


WGRAD, DINPUT = "mfma_f32:conv3x3s2_wgrad", "mfma_f32:conv3x3s2_dinput"


# ---- the two convolution gradients, exact -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_conv_gradients_are_exact_on_integer_operands(hip, case):
    n, h, w, cin, pitch, cout = case
    slots, _ = R.wgrad_slots(n * (h // 2) * (w // 2), cin, cout)
    assert hip.load().gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(n, h, w, cin, pitch, cout) == slots * 9 * (-(-cin // 128) * 128) * cout * 8
    x, weight, dz, dw64, dx64 = R.conv_lattice(case)
    xd, dzd = _pitched(x, pitch), _pitched(dz, cout)      # the pad channels of x hold NaN: they must not reach dW
    dw = hip.conv3x3s2_wgrad_f32(dzd, xd, cin)
    bad = (dw.cpu().double() != dw64).nonzero()
    assert len(bad) == 0, f"dW: {len(bad)} wrong of {dw.numel()}, first {bad[:4].tolist()}"
    dx = hip.conv3x3s2_dinput_f32(dzd, _tail(hip.conv3x3s2_dinput_weight(weight.to(DEV))), cin, pitch)
    assert dx.shape == (n, pitch, h, w) and dx.is_contiguous(memory_format=torch.channels_last)
    bad = (_nchw(dx)[:, :cin].double() != dx64).nonzero()
    assert len(bad) == 0, f"dx: {len(bad)} wrong of {dx64.numel()}, first {bad[:4].tolist()}"
    assert not dx[:, cin:].any() and torch.isfinite(dx).all()      # the channels from Cin to the pitch: written, exactly 0
    # two calls, equal bits; either gradient alone: the same bits and only its own launches
    (dx2, dw2), kinds = _records(hip, lambda: hip.conv3x3s2_backward(xd, cin, weight.to(DEV), dzd))
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw) and kinds.count(WGRAD) == 1 and kinds.count(DINPUT) == 1
    (dx3, none_w), kinds = _records(hip, lambda: hip.conv3x3s2_backward(xd, cin, weight.to(DEV), dzd, want=(True, False)))
    assert none_w is None and torch.equal(dx3, dx) and kinds.count(WGRAD) == 0 and kinds.count(DINPUT) == 1
    (none_x, dw3), kinds = _records(hip, lambda: hip.conv3x3s2_backward(xd, cin, weight.to(DEV), dzd, want=(False, True)))
    assert none_x is None and torch.equal(dw3, dw) and kinds.count(WGRAD) == 1 and kinds.count(DINPUT) == 0


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_one_hot_probes_locate_every_tap(hip, case):
    n, h, w, cin, pitch, cout = case
    cx, cw = R.coded_x(case), R.coded_weight(case)
    xd, wd = _pitched(cx, pitch), _tail(hip.conv3x3s2_dinput_weight(cw.to(DEV)))
    for probe in R.probe_positions(case):
        b, oy, ox, co = probe
        dz = R.onehot_dz(case, probe)
        dzd = _pitched(dz, cout)
        dw = hip.conv3x3s2_wgrad_f32(dzd, xd, cin).cpu()
        dx = _nchw(hip.conv3x3s2_dinput_f32(dzd, wd, cin, pitch))
        assert torch.equal(dw.double(), R.wgrad_s2(dz.double(), cx.double())), probe
        assert torch.equal(dx[:, :cin].double(), R.dinput_s2(dz.double(), cw.double())), probe
        assert not dx[:, cin:].any()
        for ky, kx in itertools.product(range(3), range(3)):      # said directly: the tap's pixel of x, the tap's row of W, or nothing
            y, xx = 2 * oy + ky - 1, 2 * ox + kx - 1
            if 0 <= y < h and 0 <= xx < w:
                assert torch.equal(dw[co, :, ky, kx], cx[b, :, y, xx]) and torch.equal(dx[b, :cin, y, xx], cw[co, :, ky, kx]), (probe, ky, kx)
            else:
                assert not dw[co, :, ky, kx].any(), (probe, ky, kx)


# ---- random operands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_conv_meets_the_bar(hip, case):
    n, h, w, cin, pitch, cout = case
    x, weight, g = R.conv_inputs(case)
    ref64, ref32 = R.conv_references(case)
    xd, gd, wd = _pitched(x, pitch, fill=0.0), _pitched(g, cout), weight.to(DEV)
    z = hip.conv3x3s2_f32_mfma(xd, _tail(hip.conv3x3s2_weight_kn(wd)))
    dx, dw = hip.conv3x3s2_backward(xd, cin, wd, gd)
    got = dict(z=_nchw(z), dx=_nchw(dx)[:, :cin], dW=dw)
    ratios = {k: ratio_to_bar(v, ref64[k], ref32[k]) for k, v in got.items()}
    print("pnp_bwd conv", R.case_id(case), " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(torch.isfinite(v).all() for v in got.values()) and not dx[:, cin:].any()
    assert max(ratios.values()) <= 1.0, ratios
    # a NaN-filled pad leaves dW's bits alone
    assert torch.equal(hip.conv3x3s2_wgrad_f32(gd, _pitched(x, pitch), cin), dw)


def test_flatten_round_trip_is_bit_equal(hip):
    for b, c, h, w in ((3, 128, 2, 2), (2, 128, 8, 8), (1, 36, 5, 7)):
        gen = torch.Generator().manual_seed(b + c)
        x = torch.randn(b, c, h, w, generator=gen)
        xd = _pitched(x, c)
        flat = hip.nhwc_flatten_nchw(xd)
        assert torch.equal(flat.cpu(), x.flatten(1))
        back = hip.nhwc_unflatten_nchw(_tail(flat), c, h, w)
        assert back.is_contiguous(memory_format=torch.channels_last) and torch.equal(back, xd)
        assert torch.equal(R.flatten_nchw(xd.permute(0, 2, 3, 1).reshape(b, h * w, c).cpu()), flat.cpu())


def _fc_forward(hip_layers, d, grad=R.FC_LEAVES):
    leaves = {k: d[k].detach().clone().requires_grad_(k in grad) for k in R.FC_LEAVES}
    h1 = hip_layers.LinearGelu.apply(leaves["x"], leaves["w1"], leaves["b1"])
    h2 = hip_layers.LinearGelu.apply(h1, leaves["w2"], leaves["b2"])
    rot, t = hip_layers.PnPHeads.apply(h2, leaves["w_r"], leaves["b_r"], leaves["w_t"], leaves["b_t"])
    return leaves, h1, h2, rot, t


@pytest.mark.parametrize("b", R.FC_BATCHES)
def test_fc_tail_meets_the_bar(hip, train_kernels, b):
    t = R.fc_inputs(b)
    d = {k: _tail(v) for k, v in t.items()}
    ref64, ref32 = R.fc_references(b)
    leaves, h1, h2, rot, tr = _fc_forward(train_kernels, d)
    ((rot * d["g_r"]).sum() + (tr * d["g_t"]).sum()).backward()
    got = dict(h1=h1, h2=h2, rot=rot, t=tr, **{"d" + k: leaves[k].grad for k in R.FC_LEAVES})
    ratios = {k: ratio_to_bar(v, ref64[k], ref32[k]) for k, v in got.items()}
    print("pnp_bwd fc b=%d" % b, " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(torch.isfinite(v).all() for v in got.values())
    assert max(ratios.values()) <= 1.0, ratios
    # two runs, equal bits
    leaves2, *_, rot2, tr2 = _fc_forward(train_kernels, d)
    ((rot2 * d["g_r"]).sum() + (tr2 * d["g_t"]).sum()).backward()
    assert all(torch.equal(leaves2[k].grad, leaves[k].grad) for k in R.FC_LEAVES)
    # the heads' kernel alone against its restatement, and with one source absent
    direct = hip.pnp_fc_heads_backward(d["g_r"], d["g_t"], h2.detach(), d["w_r"], d["w_t"])
    assert torch.equal(direct[1], leaves["w_r"].grad) and torch.equal(direct[2], leaves["b_r"].grad)
    assert torch.equal(direct[3], leaves["w_t"].grad) and torch.equal(direct[4], leaves["b_t"].grad)
    only_t = hip.pnp_fc_heads_backward(None, d["g_t"], h2.detach(), d["w_r"], d["w_t"])
    assert not only_t[1].any() and not only_t[2].any() and torch.equal(only_t[3], direct[3]) and torch.equal(only_t[4], direct[4])
    want = R.heads_backward(None, t["g_t"].double(), h2.detach().cpu().double(), t["w_r"].double(), t["w_t"].double())[0]
    assert float((only_t[0].cpu().double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())


def test_fc_tail_subsets_keep_bits_and_skip_launches(hip, train_kernels):
    d = {k: _tail(v) for k, v in R.fc_inputs(3).items()}

    def run(grad):
        def go():
            leaves, _, _, rot, tr = _fc_forward(train_kernels, d, grad=grad)
            ((rot * d["g_r"]).sum() + (tr * d["g_t"]).sum()).backward()
            return {k: v.grad for k, v in leaves.items()}
        return _records(hip, go)

    full, kinds = run(R.FC_LEAVES)
    assert kinds.count("gemm_tn") == 2 and kinds.count("pnp_heads_bwd") == 1 and kinds.count("hbm:mlp_bwd_act") == 2
    n_exact = kinds.count("linear_exact")
    assert n_exact == 2 + 2      # two forward products, two data gradients
    for grad in (("x",), ("w1", "b1"), ("w2",), ("w_r", "b_r"), ("b_t",), ("x", "w_t"), ("b1", "b2", "b_r")):
        part, kinds = run(grad)
        for k in R.FC_LEAVES:
            assert (part[k] is None) == (k not in grad), (grad, k)
            if k in grad:
                assert torch.equal(part[k], full[k]), (grad, k)
        assert kinds.count("gemm_tn") == ("w1" in grad) + ("w2" in grad), (grad, kinds)      # a frozen layer: no weight-gradient product
        first = min(R.FC_LEAVES.index(k) for k in grad)
        # data gradients are formed only for what lies in front of them: fc2's dx when something of fc1 or x asks, fc1's dx for x
        assert kinds.count("linear_exact") == 2 + (first < 3) + (first < 1), (grad, kinds)


def test_nan_in_the_gradient_spreads_as_in_autograd(hip, train_kernels):
    # the convolution: an interior output pixel, all nine taps inside the image
    case = R.CASES[1]
    n, h, w, cin, pitch, cout = case
    x, weight, g = R.conv_inputs(case)
    g = g.clone()
    g[1, 7, 1, 2] = NAN
    ref = R.autograd_conv(x, weight, g, torch.float32)
    dx, dw = hip.conv3x3s2_backward(_pitched(x, pitch), cin, weight.to(DEV), _pitched(g, cout))
    assert torch.equal(torch.isnan(dw).cpu(), torch.isnan(ref["dW"])) and int(torch.isnan(dw).sum()) == 9 * cin
    assert torch.equal(torch.isnan(_nchw(dx)[:, :cin]), torch.isnan(ref["dx"])) and not dx[:, cin:].any()
    # the fc tail
    t = dict(R.fc_inputs(3))
    t["g_r"] = t["g_r"].clone()
    t["g_r"][1, 4] = NAN
    ref = R.autograd_fc(t, torch.float32)
    d = {k: _tail(v) for k, v in t.items()}
    leaves, _, _, rot, tr = _fc_forward(train_kernels, d)
    ((rot * d["g_r"]).sum() + (tr * d["g_t"]).sum()).backward()
    for k in R.FC_LEAVES:
        assert torch.equal(torch.isnan(leaves[k].grad).cpu(), torch.isnan(ref["d" + k])), k
    assert torch.isnan(leaves["x"].grad[1]).all() and torch.isfinite(leaves["x"].grad[[0, 2]]).all() and torch.isfinite(leaves["w_t"].grad).all()


def test_shapes_outside_the_kernels_raise_in_their_words(hip):
    lib = hip.load()
    assert lib.gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(1, 5, 4, 128, 128, 128) == 0      # odd H
    assert lib.gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(1, 4, 4, 128, 128, 64) == 0       # Cout no multiple of 128
    assert lib.gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(1, 4, 4, 69, 80, 128) == 0        # a pitch that is no multiple of 32
    assert lib.gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(1, 4, 4, 128, 160, 128) > 0       # Cin % 128 == 0 inside a wider pitch of 32s
    x, dz64 = torch.zeros(1, 128, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last), torch.zeros(1, 64, 2, 2, device=DEV)
    dz64 = dz64.contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="gdrnpp_conv3x3s2_wgrad_f32.*Cout=64"):
        hip.conv3x3s2_wgrad_f32(dz64, x, 128)
    with pytest.raises(RuntimeError, match="gdrnpp_conv3x3s2_dinput_f32.*Cout=64"):
        hip.conv3x3s2_dinput_f32(dz64, torch.zeros(9 * 64, 128, device=DEV), 128)
    x80 = torch.zeros(1, 80, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    dz = torch.zeros(1, 128, 2, 2, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="gdrnpp_conv3x3s2_wgrad_f32.*ldx=80"):
        hip.conv3x3s2_wgrad_f32(dz, x80, 69)
    with pytest.raises(RuntimeError, match="gdrnpp_pnp_fc_heads_backward.*K=2048"):
        hip.pnp_fc_heads_backward(torch.zeros(2, 6, device=DEV), None, torch.zeros(2, 2048, device=DEV), torch.zeros(6, 2048, device=DEV),
                                  torch.zeros(3, 2048, device=DEV))
    with pytest.raises(RuntimeError, match="gdrnpp_nhwc_flatten_nchw"):
        lib_rc = lib.gdrnpp_nhwc_flatten_nchw(x.data_ptr(), x.data_ptr(), 1, 16, 128, 0, None)
        hip.check(lib_rc, "gdrnpp_nhwc_flatten_nchw")
    assert hip.pnp_fc_heads_backward(None, None, torch.zeros(2, 256, device=DEV), torch.zeros(6, 256, device=DEV), torch.zeros(3, 256, device=DEV),
                                     want=(False,) * 5) == (None,) * 5


# ---- through autograd: Patch-PnP alone -----------------------------------------------------------------------------------------------
def _variance_preserving_(module):
    with torch.no_grad():      # the heads' own initial values (std 0.001) would leave every activation at its bias
        for name, p in module.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (p[0].numel() ** -0.5))
            elif name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.1)
            else:
                p.copy_(1.0 + torch.randn_like(p) * 0.1)


def _pnp_net(act="gelu"):
    from gdrnpp_bop2022_amd.gdrn_modeling.heads import ConvPnPNet

    torch.manual_seed(11)
    net = ConvPnPNet(nIn=69, num_regions=64, featdim=128, rot_dim=6, norm="GN", act=act, final_spatial_size=(2, 2))
    _variance_preserving_(net)
    return net.eval()


def _pnp_reference(net, x96, g_r, g_t, dtype):
    """``forward_prepared`` on the CPU in ``dtype`` (PyTorch's operators) + backward -> (rot, t, dx [B,69,H,W], {parameter: gradient})."""
    m = copy.deepcopy(net).cpu().to(dtype)
    x = x96.to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    rot, t = m.forward_prepared(x)
    ((rot * g_r.to(dtype)).sum() + (t * g_t.to(dtype)).sum()).backward()
    return rot.detach(), t.detach(), x.grad[:, :69], {n: p.grad for n, p in m.named_parameters()}


@pytest.fixture(scope="module")
def pnp_case():
    net = _pnp_net()
    x96 = R.real_scale_input(3, 16, 16)
    gen = torch.Generator().manual_seed(12)
    g_r, g_t = torch.randn(3, 6, generator=gen), torch.randn(3, 3, generator=gen)
    return dict(net=net, x96=x96, g_r=g_r, g_t=g_t, ref64=_pnp_reference(net, x96, g_r, g_t, torch.float64),
                ref32=_pnp_reference(net, x96, g_r, g_t, torch.float32))


def _graph_nodes(y):
    seen, todo = set(), [y.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


OURS = {"Conv3x3S2GnActBackward", "LinearGeluBackward", "PnPHeadsBackward", "FlattenNCHWBackward"}
THEIRS = {"ConvolutionBackward0", "NativeGroupNormBackward0", "GeluBackward0", "AddmmBackward0"}


def _dev_input(x96):
    return _tail(x96.permute(0, 2, 3, 1)).permute(0, 3, 1, 2).requires_grad_(True)


def test_pnp_trains_on_this_librarys_kernels(hip, train_kernels, pnp_case):
    hip_layers = train_kernels
    net = copy.deepcopy(pnp_case["net"]).to(DEV)
    x = _dev_input(pnp_case["x96"])
    foreign, x3 = hip_layers.fallback_launches(), hip.x3_launch_count()
    rot, t = net.forward_prepared(x)
    nodes = _graph_nodes(rot) | _graph_nodes(t)
    assert OURS <= nodes and not (THEIRS & nodes), nodes
    ((rot * pnp_case["g_r"].to(DEV)).sum() + (t * pnp_case["g_t"].to(DEV)).sum()).backward()
    assert hip_layers.fallback_launches() == foreign and hip.x3_launch_count() == x3
    (r64, t64, dx64, g64), (r32, t32, dx32, g32) = pnp_case["ref64"], pnp_case["ref32"]
    ratios = dict(rot=ratio_to_bar(rot, r64, r32), t=ratio_to_bar(t, t64, t32), dx=ratio_to_bar(x.grad[:, :69], dx64, dx32))
    assert not x.grad[:, 69:].any()
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        ratios[n] = ratio_to_bar(p.grad, g64[n], g32[n])
    print("pnp_bwd net", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def test_frozen_parameters_get_none_and_change_nobodys_bits(hip, train_kernels, pnp_case):
    def run(frozen):
        net = copy.deepcopy(pnp_case["net"]).to(DEV)
        for n, p in net.named_parameters():
            p.requires_grad_(n not in frozen)
        x = _dev_input(pnp_case["x96"])

        def go():
            rot, t = net.forward_prepared(x)
            ((rot * pnp_case["g_r"].to(DEV)).sum() + (t * pnp_case["g_t"].to(DEV)).sum()).backward()
        _, kinds = _records(hip, go)
        return {n: p.grad for n, p in net.named_parameters()}, x.grad, kinds

    full, dx, kinds = run(())
    assert kinds.count(WGRAD) == 3 and kinds.count(DINPUT) == 3 and kinds.count("gemm_tn") == 2 and kinds.count("pnp_heads_bwd") == 1
    frozen = ("features.0.weight", "features.4.weight", "fc1.weight", "fc_r.bias")
    part, dx2, kinds = run(frozen)
    assert kinds.count(WGRAD) == 2 and kinds.count(DINPUT) == 3 and kinds.count("gemm_tn") == 1
    assert torch.equal(dx2, dx)
    for n, g in full.items():
        assert (part[n] is None) if n in frozen else torch.equal(part[n], g), n


def test_other_configurations_keep_todays_path(hip, train_kernels, pnp_case):
    hip_layers = train_kernels
    x96 = pnp_case["x96"]

    def graph(net, x):
        before = hip_layers.fallback_launches()
        rot, t = net.forward_prepared(x)
        return rot, t, _graph_nodes(rot) | _graph_nodes(t), hip_layers.fallback_launches() - before

    net = copy.deepcopy(pnp_case["net"]).to(DEV)
    relu = _pnp_net(act="relu").to(DEV)
    # act = "relu" (ReLU in the convolutions, LeakyReLU in the fcs) with the switch on: PyTorch's graph, foreign launches counted
    _, _, nodes, counted = graph(relu, _dev_input(x96))
    assert not (OURS & nodes) and "ConvolutionBackward0" in nodes and counted >= 1, nodes
    # an input whose size is no multiple of 8
    _, _, nodes, counted = graph(copy.deepcopy(net), _dev_input(R.real_scale_input(3, 16, 16)[:, :, :12, :12]))
    assert not (OURS & nodes) and "ConvolutionBackward0" in nodes and counted >= 1, nodes
    # the switch off: today's graph and today's values
    rot_on, t_on, nodes_on, counted_on = graph(net, _dev_input(x96))
    assert OURS <= nodes_on and counted_on == 0
    hip_layers.set_train_kernels(False)
    rot_off, t_off, nodes, counted = graph(net, _dev_input(x96))
    assert not (OURS & nodes) and {"ConvolutionBackward0", "NativeGroupNormBackward0", "GeluBackward0", "AddmmBackward0"} <= nodes and counted >= 1, nodes
    want_rot, want_t = net._fc_tail(_todays_features(net, x96))
    assert torch.allclose(rot_off, want_rot, rtol=1e-5, atol=1e-6) and torch.allclose(t_off, want_t, rtol=1e-5, atol=1e-6)
    # no_grad: the inference kernels, the same bits with the switch on and off
    with torch.no_grad():
        off = net.forward_prepared(_dev_input(x96).detach())
        hip_layers.set_train_kernels(True)
        on = net.forward_prepared(_dev_input(x96).detach())
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and on[0].grad_fn is None
    # the training forward is not the inference forward bit for bit (fp32-MFMA convolutions against the six-product ones), but close
    assert float((rot_on.detach() - on[0]).abs().max()) <= 1e-3 * float(on[0].abs().max())


def _todays_features(net, x96):
    """Today's autograd branch of ``forward_prepared`` spelled out: F.conv2d on the 69 channels, then the layers one by one."""
    import torch.nn.functional as F

    from gdrnpp_bop2022_amd.gdrn_modeling.heads import run_features

    c0 = net.features[0]
    x = x96.to(DEV).contiguous(memory_format=torch.channels_last)
    return run_features(net.features[1:], F.conv2d(x[:, :69], c0.weight, None, c0.stride, c0.padding))


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class TinyBackbone(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 128, 4, stride=4)

    def forward(self, x):
        return torch.nn.functional.gelu(self.conv(x))


def _tiny_model():
    """GDRN_DoubleMask, class-aware with 3 classes, double mask: 32 x 32 crops, a 16 x 16 output (hw = 256), a 128-channel head."""
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import GDRN_DoubleMask
    from gdrnpp_bop2022_amd.gdrn_modeling.heads import ConvPnPNet, TopDownDoubleMaskXyzRegionHead

    cfg = get_cfg("tudl_convnext_a6", ["MODEL.POSE_NET.OUTPUT_RES=16", "MODEL.POSE_NET.INPUT_RES=32", "MODEL.POSE_NET.LOSS_CFG.FULL_MASK_LW=1.0"])
    assert cfg.MODEL.POSE_NET.NUM_CLASSES == 3
    torch.manual_seed(5)
    head = TopDownDoubleMaskXyzRegionHead(128, feat_dim=128, up_types=("bilinear",), num_conv_per_block=1, mask_num_classes=3,
                                          xyz_num_classes=3, region_num_classes=3, mask_out_dim=2)
    pnp = ConvPnPNet(nIn=69, num_regions=64, featdim=128, rot_dim=6, norm="GN", act="gelu", final_spatial_size=(2, 2))
    model = GDRN_DoubleMask(cfg, TinyBackbone(), head, pnp_net=pnp)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (p[0].numel() ** -0.5))
            elif name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.1)
    return cfg, model.eval()


def _tiny_batch(cfg, B, dev, dtype=torch.float32):
    from gdrnpp_bop2022_amd import synthetic as S
    from gdrnpp_bop2022_amd.gdrn_modeling import losses as L
    from tests.test_gpu_losses import dense_inputs, rot

    rng = np.random.default_rng(20221019 + 31)
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
    x, batch, _, per_roi = _tiny_batch(cfg, 5, "cpu", dtype)
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


def test_model_trains_through_patch_pnp(hip, train_kernels):
    hip_layers = train_kernels
    cfg, model = _tiny_model()
    (t64, g64), (t32, g32) = _cpu_reference(cfg, model, torch.float64), _cpu_reference(cfg, model, torch.float32)
    model = model.to(DEV).to(memory_format=torch.channels_last)
    x, batch, tables, _ = _tiny_batch(cfg, 5, DEV)
    notes = []
    note = hip_layers.note_foreign_launch
    hip_layers.note_foreign_launch = lambda what: (notes.append(what), note(what))[1]
    try:
        _, loss = model(x, do_loss=True, gt_tables=tables(), **batch)
    finally:
        hip_layers.note_foreign_launch = note
    total = sum(loss.values())
    nodes = _graph_nodes(total)
    assert OURS <= nodes and "HeadTailBackward" in nodes and "AddmmBackward0" not in nodes, nodes
    assert not [w for w in notes if "ConvPnPNet" in w or "linear:" in w or "pnp_fc_heads" in w or "run_features" in w], notes
    total.backward()
    ratios = {"loss": abs(float(total.detach()) - float(t64)) / bar(t64.reshape(1), t32.reshape(1))}
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        ratios[n] = ratio_to_bar(p.grad, g64[n], g32[n])
    print("pnp_bwd model", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
