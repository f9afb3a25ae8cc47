"""-m gpu: the split GEMMs against an oracle with NO tolerance (tests/split_lattice.py; its own exactness is checked on the CPU by
tests/test_split_lattice_cpu.py).  On the lattices every partial product and every partial sum of the three-product scheme is
exactly representable in fp32, so each launch has ONE correct bit pattern in whatever order its MFMAs accumulate: everything here
is torch.equal, except the GroupNorm case (a normalised output is not exact; it keeps the project's bar for that pair).
What the accuracy bars of tests/test_gpu_split2.py cannot see and this file pins:
  * K = 32 (two k-tiles: every prologue / k-tile clamp of gemm_split2_pipe.hip active at once), nk = 6 and 10 (three A stages and
    four weight slots out of phase), M = 1 .. 513 with canary rows behind M through the C ABI;
  * the 3x3 convolution at ragged pixel counts, tiles that span images, images smaller than the stencil; the general convolution
    at 4 .. 25 taps and 2 / 4 chunks per tap; the transposed convolution's GEMM + col2im;
  * wide tiles, every panel walk, the "f16x2 rows" hand-over with a non-zero l plane on both operands;
  * every route of the six-product family on the same integers (split-K partial sums and the fixed-order reduce included), and its
    m / l planes on a one-sided 2^-17 lattice.
A failure prints the first mismatching indices (the one-hot probe: which k the kernel actually used)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import split_lattice as SL

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _exact(got, want, what=""):
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got.double(), want):
        pytest.fail(f"{what}: not the exact value\n{SL.mismatch_report(got, want)}")


def _epi_args(c, epi, dev=DEV):
    """(bias, epilogue name, gamma, resid) of hip.linear_f32_split for the oracle's epilogue key."""
    if epi == "none":
        return None, "none", None, None
    if epi == "bias":
        return c["bias"].to(dev), "none", None, None
    return c["bias"].to(dev), "scale_res", c["gamma"].to(dev), c["resid"].to(dev)


def _nhwc(x):
    """Device tensor with NHWC memory whatever the sizes (H = 1 / W = 1 make the channels_last stride test ambiguous)."""
    return x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _no_words(hip):
    words = hip.split2_range_words()
    assert words == {}, f"range words {words}"


# ---- linear, three products -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("int", "hl"))
@pytest.mark.parametrize("m,k,n", SL.LINEAR_SHAPES)
def test_linear_three_products_exact(hip, m, k, n, kind):
    c = SL.linear_case(m, k, n, kind)
    x, pk = c["A"].to(DEV), hip.pack_weight_f16x2(c["W"].to(DEV))
    assert hip.packed_rows_in_range(pk)
    if kind == "hl":
        planes, inv = hip.unpack_weight_f16x2(pk)
        assert inv == 2.0 ** -12 and bool((planes[1] != 0).any())           # scaled by exactly 2^12, l plane in use
    for epi in SL.EPILOGUES:
        bias, name, gamma, resid = _epi_args(c, epi)
        _exact(hip.linear_f32_split(x, pk, bias, name, gamma, resid), c["want"][epi], f"M={m} K={k} N={n} {kind} {epi}")
    _no_words(hip)


@pytest.mark.parametrize("m,k,n", [(257, 96, 384), (1, 32, 128)])
def test_linear_three_products_onehot_probe(hip, m, k, n):
    """Row m is 2 e_k(m), W[n, k] a code of (n mod 61, k): a wrong element names the k-tile (and column class) it came from."""
    A, W, want = SL.onehot_probe(m, k, n)
    out = hip.linear_f32_split(A.to(DEV), hip.pack_weight_f16x2(W.to(DEV)), None).cpu()
    if not torch.equal(out.double(), want):
        pytest.fail(f"M={m} K={k} N={n}: " + SL.onehot_report(out, want, k))
    _no_words(hip)


@pytest.mark.parametrize("m", [1, 255, 257])
def test_linear_three_products_c_abi_writes_m_rows(hip, m):
    """gdrnpp_linear_f32_split2 into M rows of a larger buffer: exact up to row M, untouched behind it."""
    k, n = 96, 384
    c = SL.linear_case(m, k, n, "hl")
    x, b, pk = c["A"].to(DEV), c["bias"].to(DEV), hip.pack_weight_f16x2(c["W"].to(DEV))
    big = torch.full((m + 4, n), 777.0, device=DEV)
    rc = hip.load().gdrnpp_linear_f32_split2(x.data_ptr(), pk.data_ptr(), b.data_ptr(), None, None, big.data_ptr(), m, n, k, 0,
                                             ctypes.c_void_p(hip.x3_flags().data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(big[m:], torch.full((4, n), 777.0, device=DEV))
    _exact(big[:m], c["want"]["bias"], f"C ABI M={m}")
    _no_words(hip)


@pytest.mark.parametrize("kind", ("int", "hl"))
def test_two_column_tiles_ragged_m_exact(hip, kind):
    """Two 128-column tiles over two row blocks, the second with 44 of its 256 rows."""
    m, k, n = 300, 96, 256
    c = SL.linear_case(m, k, n, kind)
    x, pk = c["A"].to(DEV), hip.pack_weight_f16x2(c["W"].to(DEV))
    for epi in SL.EPILOGUES:
        bias, name, gamma, resid = _epi_args(c, epi)
        _exact(hip.linear_f32_split(x, pk, bias, name, gamma, resid), c["want"][epi], f"{kind} {epi}")
    _no_words(hip)


@pytest.mark.parametrize("m,k,n", [(300, 512, 1024), (1300, 512, 1152)])
def test_panel_walks_exact(hip, m, k, n):
    """Tiles walked in panels of 0 (row-major), 3, 4, 8 row blocks.  The entry point walks panels for N / 128 >= 8 and a packed
    image ABOVE 2 MiB: 1024 x 512 is exactly 2 MiB (row-major whatever the option says), 1152 x 512 with six row blocks has full
    and partial panels."""
    c = SL.int_case(m, k, n)
    x, pk = c["A"].to(DEV), hip.pack_weight_f16x2(c["W"].to(DEV))
    bias, name, gamma, resid = _epi_args(c, "scale_res")
    try:
        for panel in (0, 3, 4, 8):
            hip.set_option("split_gemm_panel", panel)
            _exact(hip.linear_f32_split(x, pk, bias, name, gamma, resid), c["want"]["scale_res"], f"panel={panel}")
    finally:
        hip.set_option("split_gemm_panel", 4)
    _no_words(hip)


@pytest.mark.parametrize("m,k2", [(300, 128), (300, 384), (1, 128), (1, 384)])
def test_f16x2_rows_chain_exact(hip, m, k2):
    """c_rows: the stored halves are h + l == the exact first result (22 bits); a_rows: a second launch reads them (non-zero l)
    against weights in {-1, 0, 1} with the scale + residual epilogue."""
    c = SL.rows_chain_case(m, k2)
    first = c["first"]
    p1 = hip.pack_weight_f16x2(first["W"].to(DEV))
    rows = hip.linear_f32_split(first["A"].to(DEV), p1, first["bias"].to(DEV), "none", c_rows=True)
    h, l = hip.f16x2_rows_decode(rows)
    _exact(h.cpu().double() + l.cpu().double(), c["x"], "h + l of the rows tensor")
    assert torch.equal(h.cpu().double(), c["h"]) and torch.equal(l.cpu().double(), c["l"])
    assert torch.equal(rows.cpu().view(torch.int32), SL.rows_of(c["x"]).view(torch.int32))
    p2 = hip.pack_weight_f16x2(c["W2"].to(DEV))
    out = hip.linear_f32_split(rows, p2, None, "scale_res", c["gamma"].to(DEV), c["resid"].to(DEV), a_rows=True)
    _exact(out, c["want"], f"rows x W2, M={m} K={k2}")
    _exact(hip.linear_f32_split(c["x"].float().to(DEV), p2, None, "scale_res", c["gamma"].to(DEV), c["resid"].to(DEV)), c["want"], "fp32 hand-over")
    _no_words(hip)


# ---- convolutions, three products --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("int", "hl"))
@pytest.mark.parametrize("n,cin,h,w,cout", SL.CONV3_SHAPES)
def test_conv3x3_three_products_exact(hip, n, cin, h, w, cout, kind):
    c = SL.conv_case(n, cin, h, w, cout, 3, 1, 1, kind)
    x, pk = _nhwc(c["x"]), hip.pack_conv_weight_f16x2(c["w"].to(DEV))
    for with_bias in (False, True):
        out = hip.conv3x3_f32_split(x, pk, c["bias"].to(DEV) if with_bias else None)
        _exact(out, c["want"][with_bias], f"conv3x3 ({n}, {cin}, {h}, {w}) -> {cout} {kind} bias={with_bias}")
    _no_words(hip)


@pytest.mark.parametrize("cin,ks,stride,pad,kind", SL.CONV2_CASES)
def test_general_conv_three_products_exact(hip, cin, ks, stride, pad, kind):
    c = SL.conv_case(3, cin, 11, 7, 128, ks, stride, pad, kind)
    x, pk = _nhwc(c["x"]), hip.pack_conv_weight_f16x2(c["w"].to(DEV))
    for with_bias in (False, True):
        out = hip.conv2d_f32_split(x, pk, c["bias"].to(DEV) if with_bias else None, ks, ks, stride, pad)
        _exact(out, c["want"][with_bias], f"conv {ks}x{ks}/{stride}/{pad} Cin={cin} {kind} bias={with_bias}")
    _no_words(hip)


@pytest.mark.parametrize("ks,pad,out_pad", SL.DECONV_CASES)
def test_conv_transpose_exact(hip, ks, pad, out_pad):
    """Three-product GEMM + col2im gather, and the six-product weight on the same input: one expected tensor."""
    c = SL.deconv_case(ks, pad, out_pad)
    x, b = _nhwc(c["x"]), c["bias"].to(DEV)
    for pack in (hip.pack_deconv_weight_f16x2, hip.pack_deconv_weight_bf16x3):
        out = hip.conv_transpose2d_f32_split(x, pack(c["w"].to(DEV)), b, ks, 2, pad, out_pad)
        _exact(out, c["want"], f"deconv ks={ks} pad={pad} out_pad={out_pad} {pack.__name__}")
    _no_words(hip)


@pytest.mark.parametrize("n", [1, 3])
def test_conv3x3_groupnorm_three_products_smallest_shape(hip, n):
    """Conv3x3 with GroupNorm statistics in its epilogue at H * W = 256, one / three 256-row tiles per column tile.  The normalised
    output is not exact: the bar is that of test_conv3x3_groupnorm_three_products_matches_six."""
    groups = 32
    c = SL.conv_case(n, 32, 16, 16, 256, 3, 1, 1, "int")
    gen = torch.Generator().manual_seed(n)
    gw, gb = torch.randn(256, generator=gen), torch.randn(256, generator=gen)
    x, wt, b = _nhwc(c["x"]), c["w"].to(DEV), c["bias"].to(DEV)
    y3 = hip.conv3x3_groupnorm_act(x, hip.pack_conv_weight_f16x2(wt), b, gw.to(DEV), gb.to(DEV), groups, 1e-5, _min_tiles=1)
    y6 = hip.conv3x3_groupnorm_act(x, hip.pack_conv_weight_bf16x3(wt), b, gw.to(DEV), gb.to(DEV), groups, 1e-5, _min_tiles=1)
    assert y3 is not None and y6 is not None
    conv = F.conv2d(c["x"].double(), c["w"].double(), c["bias"].double(), padding=1)
    assert torch.equal(conv, c["want"][True])
    want = F.group_norm(conv, groups, gw.double(), gb.double(), 1e-5)
    s = want.abs().max().item()
    e3, e6 = ((y.cpu().double() - want).abs().max().item() / s for y in (y3, y6))
    print(f"\nn={n}: three products {e3:.2e}  six products {e6:.2e}")
    assert e3 <= 1.3 * e6 + 4e-7 and e6 <= 3e-6, (e3, e6)
    _no_words(hip)


# ---- the six-product family on the same integers ------------------------------------------------------------------------------------
SIX_ROUTES = [(0, 1, 3), (0, 1, 0), (1, 0, 0), (1, 1, 0), (1, 1, 2), (1, 1, 3)]     # (split_gemm_mi4, split_gemm_glds, split_gemm_pipe)


@pytest.mark.parametrize("mi4,glds,pipe", SIX_ROUTES)
@pytest.mark.parametrize("m,k,n", [(257, 96, 384), (63, 32, 128), (512, 96, 256)])
def test_six_product_routes_exact(hip, m, k, n, mi4, glds, pipe):
    """128-row tiles (the pipelined 128-row form from 96 rows on, the register-staged kernel below / with the pipeline off) and
    256-row tiles (LDS-DMA, pipelined with 2 and 3 A stages): the expected tensors of the three-product test.  The register-staged
    256-row kernel exists for M % 256 == 0 only (route (1, 0, 0) at M = 257 / 63 falls to the 128-row kernel): M = 512 runs it."""
    c = SL.int_case(m, k, n)
    x, pk = c["A"].to(DEV), hip.pack_weight_bf16x3(c["W"].to(DEV))
    try:
        hip.set_option("split_gemm_mi4", mi4)
        hip.set_option("split_gemm_glds", glds)
        hip.set_option("split_gemm_pipe", pipe)
        for epi in SL.EPILOGUES:
            bias, name, gamma, resid = _epi_args(c, epi)
            _exact(hip.linear_f32_split(x, pk, bias, name, gamma, resid), c["want"][epi], f"M={m} K={k} N={n} route {(mi4, glds, pipe)} {epi}")
    finally:
        hip.set_option("split_gemm_mi4", -1)
        hip.set_option("split_gemm_glds", 1)
        hip.set_option("split_gemm_pipe", 3)
    _no_words(hip)


@pytest.mark.parametrize("m", [5, 300])
def test_six_product_splitk_exact(hip, m):
    """Integers make the split-K partial sums and the fixed-order reduce exact as well."""
    k, n = 1024, 256
    c = SL.int_case(m, k, n)
    # the plan is a cost model: make sure it cuts K here (workspace = one [M, N] partial per split)
    assert hip.load().gdrnpp_linear_f32_splitk_workspace_bytes(m, n, k) >= 2 * m * n * 4
    x, pk = c["A"].to(DEV), hip.pack_weight_bf16x3(c["W"].to(DEV))
    for epi in SL.EPILOGUES:
        bias, name, gamma, resid = _epi_args(c, epi)
        _exact(hip.linear_f32_splitk(x, pk, bias, name, gamma, resid), c["want"][epi], f"split-K M={m} {epi}")
    _no_words(hip)


def test_six_product_grouped_exact(hip):
    """Two groups of 256 rows, selectors [1, 0], 64 of 128 columns stored: each group against its own weight slice."""
    c = SL.int_case(512, 96, 256)
    x, pk = c["A"].to(DEV), hip.pack_weight_bf16x3(c["W"].to(DEV))
    sel = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    out = hip.linear_f32_split_grouped(x, pk, c["bias"].view(2, 128).to(DEV), sel, 256, n_store=64)
    want = torch.cat([c["want"]["bias"][:256, 128:192], c["want"]["bias"][256:, :64]])
    _exact(out[:, :64], want, "grouped")
    _no_words(hip)


@pytest.mark.parametrize("side", ["A", "W"])
@pytest.mark.parametrize("k", [32, 64])
def test_six_product_lower_planes_exact(hip, k, side):
    """One operand +-(1 + c 2^-9 + d 2^-17) (its bf16 m and l planes carry the fractions), the other in {-1, 0, 1}: A W^T exactly."""
    c = SL.fine_case(k, side)
    planes = hip.unpack_weight_bf16x3(hip.pack_weight_bf16x3(c["W"].to(DEV)))
    assert torch.equal(planes.double().sum(0).cpu(), c["W"].double())
    if side == "W":
        assert bool((planes[1] != 0).any()) and bool((planes[2] != 0).any())
    _exact(hip.linear_f32_split(c["A"].to(DEV), hip.pack_weight_bf16x3(c["W"].to(DEV)), None), c["want"], f"K={k} fine {side}")
    _no_words(hip)
