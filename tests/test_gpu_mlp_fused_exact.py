"""-m gpu: the fused ConvNeXt MLP (csrc/gemm_mlp_fused.hip, gdrnpp_convnext_mlp_f32_fused) against an oracle with NO tolerance
(tests/split_lattice.py: mlp_fused_expected; its own exactness is checked on the CPU by tests/test_split_lattice_cpu.py).
gelu_erf is max(x, 0) - u 2^q(u), u = min(|x|, 5.9): on inputs with no pre-activation in (-6, 6) an active unit passes the GELU bit
for bit and a dead one (-9.6e-9) is +-0 in both fp16 halves of fc2's operand, so the launch is two three-product GEMMs on lattice
operands — ONE correct bit pattern whatever order the MFMAs add in, pipelined tile loop or plain, two accumulators or one.
Everything here is torch.equal.  What the accuracy bars of tests/test_gpu_mlp_fused.py cannot see and this file pins:
  * M = 1 .. 513 around the ends of a wave (32 pixels), a workgroup (128) and the second workgroup, both widths, both tile loops;
  * which k and which hidden unit every output element was built from (two one-hot probes: the x swizzle, the W1 fragment order,
    the accumulator-to-hidden map, the W2 pack order);
  * the l planes of x, W1, the hidden operand and W2, each non-zero in one of the four lattices, all of them in the last;
  * rows behind M: NaN behind x and the residual, guard rows behind y, through the C ABI;
  * the range verdicts of the tail rows, the call on a side stream, and the operand order at the call site in hip_layers."""
import ctypes

import pytest
import torch

from tests import split_lattice as SL

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPERANDS = ("x", "b1", "b2", "gamma", "resid")


def _exact(got, want, what, report=None):
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got.double(), want):
        pytest.fail(f"{what}: not the exact value\n{(report or SL.mismatch_report)(got, want)}")


def _no_words(hip):
    words = hip.split2_range_words()
    assert words == {}, f"range words {words}"


def _device(hip, c):
    """The case's operands on the device + the packed weights (both layers' rows in range)."""
    d = {k: c[k].to(DEV) for k in OPERANDS}
    d["pk"] = hip.pack_mlp_fused_f16x2(c["W1"].to(DEV), c["W2"].to(DEV))
    assert hip.mlp_fused_rows_in_range(d["pk"]) == (True, True)
    return d


def _launch(hip, d, **kw):
    return hip.convnext_mlp_f32_fused(kw.get("x", d["x"]), d["pk"], d["b1"], d["b2"], d["gamma"], kw.get("resid", d["resid"]), *kw.get("slots", ()))


def _both_loops(hip, fn):
    """fn(pipe) under mlp_fused_pipe = 1 (the slot-by-slot software pipeline) and 0 (the plain tile loop)."""
    try:
        for pipe in (1, 0):
            hip.set_option("mlp_fused_pipe", pipe)
            fn(pipe)
    finally:
        hip.set_option("mlp_fused_pipe", 1)


# ---- exact at the row edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SL.MLPF_KINDS)
@pytest.mark.parametrize("c", SL.MLPF_C)
@pytest.mark.parametrize("m", SL.MLPF_M)
def test_fused_mlp_exact_at_the_row_edges(hip, m, c, kind):
    cs = SL.mlp_fused_case(m, c, kind)
    d = _device(hip, cs)
    _both_loops(hip, lambda pipe: _exact(_launch(hip, d), cs["want"], f"M={m} C={c} {kind} pipe={pipe}"))
    _no_words(hip)


# ---- which k, which hidden unit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SL.MLPF_C)
@pytest.mark.parametrize("m", [257, 1])
def test_fused_mlp_fc1_probe(hip, m, c):
    """Pixel m is 2 e_k(m), W1 a code of (hidden unit mod 61, k), W2 selects hidden block q: a wrong element names the hidden unit
    and the k the first GEMM used."""
    for q in range(4):
        p = SL.mlp_fc1_probe(m, c, q)
        d = _device(hip, p)
        _both_loops(hip, lambda pipe: _exact(_launch(hip, d), p["want"], f"fc1 probe M={m} C={c} q={q} pipe={pipe}",
                                             lambda got, want: SL.mlp_fc1_probe_report(got, want, c, q)))
    _no_words(hip)


@pytest.mark.parametrize("c", SL.MLPF_C)
@pytest.mark.parametrize("m", [257, 1])
def test_fused_mlp_fc2_probe(hip, m, c):
    """Pixel m has one live hidden unit C q + k(m), W2 a code of (output mod 61, hidden unit): a wrong element names the hidden
    unit the second GEMM paired with that column of W2."""
    for q in range(4):
        p = SL.mlp_fc2_probe(m, c, q)
        d = _device(hip, p)
        _both_loops(hip, lambda pipe: _exact(_launch(hip, d), p["want"], f"fc2 probe M={m} C={c} q={q} pipe={pipe}",
                                             lambda got, want: SL.mlp_fc2_probe_report(got, want, c, q)))
    _no_words(hip)


# ---- rows behind M ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SL.MLPF_C)
@pytest.mark.parametrize("m", [1, 33, 129, 257])
def test_fused_mlp_c_abi_touches_m_rows_only(hip, m, c):
    """gdrnpp_convnext_mlp_f32_fused on M rows of larger buffers: 4 rows of NaN behind x and the residual (a read behind M ends in
    the result or in a range word), 4 guard rows behind y (a store behind M lands there).  Every buffer the kernel could reach
    belongs to the test."""
    cs = SL.mlp_fused_case(m, c, "xl")
    d = _device(hip, cs)
    nan = torch.full((4, c), float("nan"), device=DEV)
    x, resid = torch.cat([d["x"], nan]), torch.cat([d["resid"], nan])

    def run(pipe):
        y = torch.full((m + 4, c), 777.0, device=DEV)
        rc = hip.load().gdrnpp_convnext_mlp_f32_fused(x.data_ptr(), d["pk"].data_ptr(), d["b1"].data_ptr(), d["b2"].data_ptr(), d["gamma"].data_ptr(),
                                                      resid.data_ptr(), y.data_ptr(), m, c, 4 * c, ctypes.c_void_p(hip.x3_flags().data_ptr() + 4 * 11),
                                                      ctypes.c_void_p(hip.x3_flags().data_ptr() + 4 * 12), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(y[m:], torch.full((4, c), 777.0, device=DEV)), f"C ABI M={m} C={c} pipe={pipe}: guard rows written"
        _exact(y[:m], cs["want"], f"C ABI M={m} C={c} pipe={pipe}")
        _no_words(hip)

    _both_loops(hip, run)


# ---- range verdicts of the tail -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SL.MLPF_C)
@pytest.mark.parametrize("m", [33, 129])
def test_fused_mlp_range_verdict_of_the_tail_rows(hip, m, c):
    """One x row 2^-12 below the lattice: fc1's word says SMALL_ROWS, fc2's nothing (the hidden row is b1's), whether the row is the
    first or the last — the lanes behind M re-load row M - 1 and must not add or hide a verdict; an all-zero last row is exact."""
    cs = SL.mlp_fused_case(m, c, "int")
    d = _device(hip, cs)

    def run(pipe):
        for row in (m - 1, 0):
            xs = d["x"].clone()
            xs[row] *= 2.0 ** -12
            y = _launch(hip, d, x=xs, slots=(11, 12))
            assert hip.split2_range_words() == {11: hip.X3_SMALL_ROWS}, (pipe, row)
            keep = [r for r in range(m) if r != row]
            _exact(y[keep], cs["want"][keep], f"M={m} C={c} pipe={pipe}: rows beside the scaled row {row}")
        xs = d["x"].clone()
        xs[m - 1] = 0.0
        y = _launch(hip, d, x=xs, slots=(11, 12))
        assert hip.split2_range_words() == {}, pipe
        _exact(y[:m - 1], cs["want"][:m - 1], f"M={m} C={c} pipe={pipe}: rows in front of the zero row")
        _exact(_launch(hip, d, slots=(11, 12)), cs["want"], f"M={m} C={c} pipe={pipe}")
        assert hip.split2_range_words() == {}, pipe

    _both_loops(hip, run)


# ---- run to run, stream to stream ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SL.MLPF_C)
def test_fused_mlp_same_call_twice_and_on_a_side_stream(hip, c):
    cs = SL.mlp_fused_case(257, c, "xl")
    d = _device(hip, cs)
    y = _launch(hip, d)
    assert torch.equal(_launch(hip, d), y)
    _exact(y, cs["want"], f"C={c} default stream")
    _no_words(hip)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ys = _launch(hip, d)
        side.synchronize()
        _no_words(hip)                                                 # the side stream's own words
    assert torch.equal(ys, y)
    _no_words(hip)


# ---- through the layer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SL.MLPF_C)
def test_convnext_mlp_layer_exact(hip, c):
    """hip_layers.convnext_mlp on an Mlp module holding a lattice case: one mlp_fused launch, and the oracle's value — the operand
    order at the call site (gamma, shortcut, the two biases)."""
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import Mlp

    m = 257
    cs = SL.mlp_fused_case(m, c, "xl")
    mlp = Mlp(c, 4 * c).to(DEV).eval()
    with torch.no_grad():
        for p, key in ((mlp.fc1.weight, "W1"), (mlp.fc1.bias, "b1"), (mlp.fc2.weight, "W2"), (mlp.fc2.bias, "b2")):
            p.copy_(cs[key])
    gamma, x, sc = cs["gamma"].to(DEV), cs["x"].to(DEV).view(1, 1, m, c), cs["resid"].to(DEV).view(1, 1, m, c)
    assert hip_layers.gemm_products() == 3
    hip_layers.reset_x3_demotions()
    prev = (hip_layers._FUSED_MLP, hip_layers._FUSED_MLP_MAX_C, hip_layers._FUSED_MLP_MIN_ROWS)
    timer = hip.LaunchTimer()
    try:
        hip_layers.set_fused_mlp_x3(True, min_rows=1)
        hip.set_launch_timer(timer)
        with torch.no_grad():
            y = hip_layers.convnext_mlp(mlp, gamma, x, sc, {})
    finally:
        hip.set_launch_timer(None)
        hip_layers.set_fused_mlp_x3(*prev)
        hip_layers.reset_x3_demotions()
    assert [r[0] for r in timer.records] == ["mlp_fused" + hip.X3]
    assert y.shape == x.shape
    _exact(y.view(m, c), cs["want"], f"convnext_mlp C={c}")
    _no_words(hip)
