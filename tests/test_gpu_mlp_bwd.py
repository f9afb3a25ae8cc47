"""The ConvNeXt MLP backward on the HIP kernels (csrc/mlp_bwd.hip + the six-product split GEMM for the shallow products) against fp64
autograd on the CPU.

The bar, per tensor: max|hip - ref64| <= 2 max|torch fp32 on the CPU - ref64| + 1 ulp of max|ref64| (tests/mlp_bwd_ref.py); every
test prints its worst ratio to that bar.  The TN GEMM and the exact forward-shaped product are also held EXACT on integer operands.

Measured on an MI355X, error / bar:
    gemm_tn, random operands          0.41 (33 x 128 x 128)   0.32 (513 x 128 x 512)   0.30 (1025 x 256 x 1024)
    linear_f32_exact, random          0.36 (257 x 256 x 1024)   0.19 (50 x 128 x 512); the [N,K] and [K,N] forms give equal bits
    layer-scale finalize              dw2 0.36 / 0.47   db2 0.11 / 0.10   dgamma 0.26 / 0.26      (gamma O(1) / 1e-6)
    activation pass                   dpre 0.22   db1 0.25
    whole backward (M, C)             y      dx     dw1    db1    dw2    db2    dgamma
        (1, 128)                      0.36   0.27   0.25   0.24   0.49   0.24   0.41
        (50, 128)                     0.30   0.38   0.40   0.38   0.52   0.15   0.17
        (257, 256)                    0.42   0.35   0.37   0.68   0.43   0.10   0.30
        (1030, 128)                   0.38   0.35   0.32   0.50   0.36   0.11   0.26
    ConvNeXtBlock(128), 2 x 5 x 5     y 0.40, input 0.25, the nine parameters 0.12 .. 0.43 (conv_dw.weight)
gelu_f32 has the bits of the GEMM's GELU epilogue, pack_weight_bf16x3_t those of the pack of the transposed copy.

With every forward-shaped product on gdrnpp_linear_f32_split the (257, 256) case measured y 1.13 and dx 1.08, (1030, 128) dx 0.98: that
kernel's fp32 accumulation of six partial products is 2.5 - 3.4 times a CPU sgemm's error at a depth of 1024 (DESIGN.md "ConvNeXt MLP
backward" has the figures per depth).  Products deeper than 256 therefore run on gdrnpp_linear_f32_exact; both paths are in the case table
(K = 128 and 256 six-product, K = 512 and 1024 exact).
"""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_bwd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _padded(t, pad_rows=40):
    """``t`` [M, N] as the head of a device allocation whose rows behind M are NaN: a read past row M poisons the result."""
    buf = torch.full((t.shape[0] + pad_rows, t.shape[1]), float("nan"), device=DEV)
    buf[:t.shape[0]] = t.to(DEV)
    return buf[:t.shape[0]]


# ---- TN GEMM ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.TN_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("m", R.TN_M)
def test_gemm_tn_is_exact_on_integer_operands(hip, m, shape):
    n1, n2 = shape
    slots, _ = R.tn_slots(m, n1, n2)
    assert hip.load().gdrnpp_gemm_tn_f32_workspace_bytes(m, n1, n2) == slots * n1 * n2 * 8
    for kind, (a, b) in (("onehot", R.tn_onehot(m, n1, n2)), ("lattice", R.tn_lattice(m, n1, n2))):
        want = a.double().t() @ b.double()
        assert float(want.abs().max()) < 2 ** 24
        got = hip.gemm_tn_f32(_padded(a), _padded(b)).cpu().double()
        assert got.shape == want.shape
        assert torch.equal(got, want), kind + ": " + R.tn_report(got, want, m, n1)


@pytest.mark.parametrize("case", R.TN_RANDOM, ids=lambda c: "m%d_%dx%d" % c)
def test_gemm_tn_rounding_meets_the_bar(hip, case):
    m, n1, n2 = case
    gen = torch.Generator().manual_seed(m + n1 + n2)
    a, b = torch.randn(m, n1, generator=gen), torch.randn(m, n2, generator=gen)
    ref64, ref32 = a.double().t() @ b.double(), a.t() @ b
    ad, bd = _padded(a), _padded(b)
    got = hip.gemm_tn_f32(ad, bd)
    ratio = R.ratio_to_bar(got, ref64, ref32)
    print("gemm_tn", case, f"ratio={ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(got, hip.gemm_tn_f32(ad, bd))


@pytest.mark.parametrize("gamma_scale", (None, 1e-6), ids=("gamma_o1", "gamma_1e-6"))
def test_layer_scale_finalize(hip, gamma_scale):
    case = R.CASES[3]
    t = R.make_inputs(case, gamma_scale)
    ref64, ref32 = R.references(case, gamma_scale)
    d = {k: v.to(DEV) for k, v in t.items()}
    pre = hip.linear_f32_split(d["x"], hip.pack_weight_bf16x3(d["w1"]), d["b1"], "none")
    h = hip.gelu_f32(pre)
    sg, db2 = hip.colsum_f32(d["g"], d["gamma"])
    dw2, dgamma = hip.gemm_tn_f32(d["g"], h, d["gamma"], d["w2"], d["b2"], sg)
    ratios = {n: R.ratio_to_bar(v, ref64[n], ref32[n]) for n, v in (("dw2", dw2), ("db2", db2), ("dgamma", dgamma))}
    print("layer_scale_finalize", gamma_scale, " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    # against the plain finalize, on operands whose G is exact: dW2 == fl(gamma G64), one rounding
    a, b = R.tn_lattice(1030, 128, 512, seed=5)
    gam = d["gamma"]
    w =torch.randn(128, 512, device=DEV)
    plain = hip.gemm_tn_f32(a.to(DEV), b.to(DEV))
    assert torch.equal(plain.cpu().double(), a.double().t() @ b.double())
    sg0 = torch.zeros(128, dtype=torch.float64, device=DEV)
    scaled, drow = hip.gemm_tn_f32(a.to(DEV), b.to(DEV), gam, w, d["b2"], sg0)
    assert torch.equal(scaled, (gam.double()[:, None] * plain.double()).float())
    want_row = (w.double() * plain.double()).sum(1)
    assert float((drow.double() - want_row).abs().max()) <= 2.0 ** -23 * float(want_row.abs().max())
    only_row = hip.gemm_tn_f32(a.to(DEV), b.to(DEV), gam, w, d["b2"], sg0, want_g=False)
    assert only_row[0] is None and torch.equal(only_row[1], drow)


# ---- the exact forward-shaped product -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mnk", [(m, n, k) for n, k in R.EXACT_NK for m in R.EXACT_M] + [R.EXACT_ONE_SLOT], ids=lambda s: "m%d_n%d_k%d" % s)
def test_linear_exact_is_exact_on_integer_operands(hip, mnk):
    m, n, k = mnk
    slots, _ = R.rows_slots(m, n, k)
    assert hip.load().gdrnpp_linear_f32_exact_workspace_bytes(m, n, k) == (slots * m * n * 8 if slots > 1 else 0)
    gen = torch.Generator().manual_seed(5 * m + n + 3 * k)
    a = torch.randint(-8, 9, (m, k), generator=gen).float()
    w = torch.randint(-8, 9, (n, k), generator=gen).float()
    w[:, ::7] = 0.0
    w[1::2, 3] = 8.0        # asymmetric: a row / column swap or a shifted k shows
    bias, resid = torch.randint(-64, 65, (n,), generator=gen).float(), torch.randint(-64, 65, (m, n), generator=gen).float()
    gamma = torch.tensor([1.0, -1.0, 2.0, 0.5])[torch.randint(0, 4, (n,), generator=gen)]
    scale = torch.tensor([1.0, -2.0, 0.5, 4.0])[torch.randint(0, 4, (k,), generator=gen)]
    z = a.double() @ w.double().t()
    assert k * 64 * 4 + 64 < 2 ** 23
    ad, wd = _padded(a), w.to(DEV)
    dev = lambda t: t.to(DEV)      # noqa: E731
    assert torch.equal(hip.linear_f32_exact(ad, wd).cpu().double(), z)
    assert torch.equal(hip.linear_f32_exact(ad, wd, dev(bias)).cpu().double(), z + bias.double())
    got = hip.linear_f32_exact(ad, wd, dev(bias), dev(gamma), dev(resid))
    assert torch.equal(got.cpu().double(), resid.double() + gamma.double() * (z + bias.double()))
    w_kn = w.t().contiguous().to(DEV)
    assert torch.equal(hip.linear_f32_exact(ad, w_kn, weight_kn=True).cpu().double(), z)
    got = hip.linear_f32_exact(ad, w_kn, weight_kn=True, row_scale=dev(scale))
    assert torch.equal(got.cpu().double(), (a.double() * scale.double()) @ w.double().t())


def test_linear_exact_rounding_meets_the_bar(hip):
    for m, n, k in ((257, 256, 1024), (50, 128, 512)):
        gen = torch.Generator().manual_seed(m + n + k)
        a, w, b = torch.randn(m, k, generator=gen), torch.randn(n, k, generator=gen) * k ** -0.5, torch.randn(n, generator=gen)
        ref64, ref32 = a.double() @ w.double().t() + b.double(), torch.nn.functional.linear(a, w, b)
        ad, wd, bd = _padded(a), w.to(DEV), b.to(DEV)
        got = hip.linear_f32_exact(ad, wd, bd)
        got_kn = hip.linear_f32_exact(ad, w.t().contiguous().to(DEV), bd, weight_kn=True)
        ratios = (R.ratio_to_bar(got, ref64, ref32), R.ratio_to_bar(got_kn, ref64, ref32))
        print("linear_exact", (m, n, k), "ratio nk=%.3f kn=%.3f" % ratios)
        assert max(ratios) <= 1.0
        assert torch.equal(got, hip.linear_f32_exact(ad, wd, bd)) and torch.equal(got, got_kn)      # the same chain either way


# ---- pack_t, gelu, the activation pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", (False, True), ids=("plain", "row_scale"))
@pytest.mark.parametrize("nk", R.PACK_SHAPES, ids=lambda s: "n%d_k%d" % s)
def test_pack_weight_t_is_the_pack_of_the_transposed_copy(hip, nk, scaled):
    n, k = nk
    gen = torch.Generator().manual_seed(n + 3 * k)
    w = (torch.randn(k, n, generator=gen) * torch.exp2(torch.randint(-12, 12, (k, n), generator=gen).float())).to(DEV)
    scale = (torch.randn(k, generator=gen) * 0.5 + 1.0).to(DEV) if scaled else None
    want = hip.pack_weight_bf16x3(((w * scale[:, None]) if scaled else w).t().contiguous())
    got = hip.pack_weight_bf16x3_t(w, scale)
    assert got.shape == want.shape == (n // 128, k // 16, 3, 2, 128, 8)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_gelu_is_the_gemm_epilogue_bit_for_bit(hip):
    """One form, decided on the machine: the GELU epilogue of linear_f32_split rounds acc + bias to fp32 before gelu_erf, so
    gelu_f32 of the "none" result has its bits."""
    t = {k: v.to(DEV) for k, v in R.make_inputs(R.CASES[2]).items()}
    pk = hip.pack_weight_bf16x3(t["w1"])
    pre = hip.linear_f32_split(t["x"], pk, t["b1"], "none")
    assert torch.equal(hip.gelu_f32(pre), hip.linear_f32_split(t["x"], pk, t["b1"], "gelu"))


def _act_inputs():
    m, cols = 67, 516        # 67 x 516 is no multiple of the workgroup's 4 rows x 256 columns; two column-sum slots (34 + 33 rows)
    gen = torch.Generator().manual_seed(11)
    pre = torch.rand(m, cols, generator=gen) * 16.0 - 8.0
    big = torch.finfo(torch.float32).max
    pre[0, :8] = torch.tensor([0.0, -0.0, 5.9, -5.9, big, -big, 8.0, -8.0])
    pre[66, -4:] = torch.tensor([big, -big, 5.9, 0.0])
    dh = torch.randn(m, cols, generator=gen)
    return pre, dh


def test_activation_pass_meets_the_bar_and_propagates_nan(hip):
    pre, dh = _act_inputs()
    assert R.col_slots(pre.shape[0])[0] == 2 and hip.load().gdrnpp_colsum_workspace_bytes(*pre.shape) == 2 * pre.shape[1] * 8
    p64 = pre.double().requires_grad_(True)
    p32 = pre.clone().requires_grad_(True)
    (ref64,) = torch.autograd.grad(torch.nn.functional.gelu(p64), p64, dh.double())
    (ref32,) = torch.autograd.grad(torch.nn.functional.gelu(p32), p32, dh)
    assert float((ref64 - dh.double() * R.gelu_grad64(pre)).abs().max()) <= 1e-14 * float(ref64.abs().max())
    pre_d, dpre = pre.to(DEV), dh.to(DEV).clone()
    h, db1 = hip.mlp_bwd_act_(pre_d, dpre)
    ratios = {"dpre": R.ratio_to_bar(dpre, ref64, ref32), "db1": R.ratio_to_bar(db1, ref64.sum(0), ref32.sum(0))}
    print("mlp_bwd_act", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert torch.isfinite(dpre).all() and max(ratios.values()) <= 1.0, ratios
    assert torch.equal(h, hip.gelu_f32(pre_d))
    assert float((db1.double() - dpre.double().sum(0)).abs().max()) <= 2.0 ** -23 * float(db1.abs().max())      # the sums of dpre as stored, one rounding
    # without h and db1: the same dpre
    again = dh.to(DEV).clone()
    assert hip.mlp_bwd_act_(pre_d, again, want_h=False, want_db1=False) == (None, None) and torch.equal(again, dpre)
    # a NaN row stays a NaN row, poisons every column sum and nothing else
    pre_n = pre_d.clone()
    pre_n[5] = float("nan")
    dn = dh.to(DEV).clone()
    h_n, db1_n = hip.mlp_bwd_act_(pre_n, dn)
    keep = torch.arange(pre.shape[0], device=DEV) != 5
    assert torch.isnan(dn[5]).all() and torch.isnan(h_n[5]).all() and torch.isnan(db1_n).all()
    assert torch.equal(dn[keep], dpre[keep]) and torch.equal(h_n[keep], h[keep])


# ---- the whole backward -------------------------------------------------------------------------------------------------------------
def _forward(hip, d):
    return hip.convnext_mlp_forward_train(d["x"], d["w1"], d["b1"], d["w2"], d["b2"], d["gamma"], d["s"])


def _backward(hip, d, pre, **kw):
    return hip.convnext_mlp_backward(d["x"], pre, d["w1"], d["w2"], d["b2"], d["gamma"], d["g"], **kw)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gradients_meet_the_bar(hip, case):
    d = {k: v.to(DEV) for k, v in R.make_inputs(case).items()}
    ref64, ref32 = R.references(case)
    y, pre = _forward(hip, d)
    got = dict(zip(R.NAMES, _backward(hip, d, pre)), y=y)
    ratios = {k: R.ratio_to_bar(got[k], ref64[k], ref32[k]) for k in ("y",) + R.NAMES}
    print("mlp_bwd", R.case_id(case), " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(torch.isfinite(v).all() for v in got.values())
    assert max(ratios.values()) <= 1.0, ratios
    for name, v in zip(R.NAMES, _backward(hip, d, pre)):      # two calls, equal bits
        assert torch.equal(got[name], v), name


WANTS = ((False, True, True, True, True, True), (True, False, True, True, True, True), (True, True, False, True, True, True),
         (True, True, True, False, True, True), (True, True, True, True, False, True), (True, True, True, True, True, False),
         (True, False, False, False, False, False), (False, True, False, False, False, False), (False, False, True, False, False, False),
         (False, False, False, True, False, False), (False, False, False, False, True, False), (False, False, False, False, False, True),
         (True, False, False, False, True, False), (False, True, True, True, True, True), (False, False, False, True, True, True))


def test_unwanted_gradients_leave_the_others_unchanged(hip):
    d = {k: v.to(DEV) for k, v in R.make_inputs(R.CASES[2]).items()}
    _, pre = _forward(hip, d)
    full = dict(zip(R.NAMES, _backward(hip, d, pre)))
    for want in WANTS:
        part = _backward(hip, d, pre, want=want)
        for name, flag, t in zip(R.NAMES, want, part):
            assert (t is None) == (not flag), (want, name)
            if flag:
                assert torch.equal(t, full[name]), (want, name)


# ---- through autograd ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def train_kernels():
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers

    hip_layers.set_train_kernels(True)
    yield hip_layers
    hip_layers.set_train_kernels(False)


def _block_grads(block, x, g):
    x = x.detach().clone().requires_grad_(True)
    for p in block.parameters():
        p.grad = None
    y = block(x)
    y.backward(g)
    return y, [x.grad] + [p.grad for p in block.parameters()]


def _graph_nodes(y):
    """Names of the autograd nodes behind ``y``."""
    seen, todo = set(), [y.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


@pytest.fixture(scope="module")
def block_case():
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import ConvNeXtBlock

    torch.manual_seed(7)
    cpu32 = ConvNeXtBlock(128)
    with torch.no_grad():
        cpu32.gamma.copy_(torch.randn(128) * 0.5 + 1.0)      # the layer-scale initial value 1e-6 would hide the branch behind the shortcut
        cpu32.norm.weight.copy_(torch.randn(128) * 0.5 + 1.0), cpu32.norm.bias.copy_(torch.randn(128) * 0.5)
    x, g = torch.randn(2, 128, 5, 5), torch.randn(2, 128, 5, 5)
    cpu64 = copy.deepcopy(cpu32).double()
    y64, ref64 = _block_grads(cpu64, x.double(), g.double())
    y32, ref32 = _block_grads(cpu32, x, g)
    names = ["x"] + [n for n, _ in cpu32.named_parameters()]
    assert len(names) == 10      # the input and the block's nine parameters (gamma, conv_dw, norm, fc1, fc2)
    return dict(block=cpu32, x=x, g=g, names=["y"] + names, ref64=[y64.detach()] + ref64, ref32=[y32.detach()] + ref32)


def test_convnext_block_trains_without_a_foreign_kernel(hip, train_kernels, block_case):
    hip_layers = train_kernels
    gpu = copy.deepcopy(block_case["block"]).to(DEV)
    xg = block_case["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    gg = block_case["g"].to(DEV)
    y, grads = _block_grads(gpu, xg, gg)
    nodes = _graph_nodes(y)
    assert "ConvNeXtMlpBackward" in nodes and "DwConvLNBackward" in nodes and not {"AddmmBackward0", "AddcmulBackward0", "GeluBackward0"} & nodes, nodes
    got = [y.detach()] + grads
    ratios = {n: R.ratio_to_bar(a, b, c) for n, a, b, c in zip(block_case["names"], got, block_case["ref64"], block_case["ref32"])}
    print("mlp_bwd block", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    # a frozen fc1.weight gets no gradient and changes nobody else's bits
    gpu.mlp.fc1.weight.requires_grad_(False)
    try:
        _, frozen = _block_grads(gpu, xg, gg)
    finally:
        gpu.mlp.fc1.weight.requires_grad_(True)
    for n, p, a, b in zip(block_case["names"][1:], [None] + list(gpu.parameters()), frozen, grads):
        if p is gpu.mlp.fc1.weight:
            assert a is None, n
        else:
            assert torch.equal(a, b), n
    # switch off: PyTorch's graph, as before
    hip_layers.set_train_kernels(False)
    y_off, _ = _block_grads(gpu, xg, gg)
    nodes = _graph_nodes(y_off)
    assert "AddcmulBackward0" in nodes and "GeluBackward0" in nodes and "ConvNeXtMlpBackward" not in nodes, nodes


def test_inference_is_untouched(hip, train_kernels, block_case):
    hip_layers = train_kernels
    gpu = copy.deepcopy(block_case["block"]).to(DEV)
    xg = block_case["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        on = gpu(xg)
        hip_layers.set_train_kernels(False)
        off = gpu(xg)
    assert on.grad_fn is None and torch.equal(on, off)
