"""dwconv7x7+LN: the kernels compiled per channel count (C = 128 / 256 / 512 / 1024, option dwconv_specialise = 1) against the
run-time-width form of the same build (option 0), bit for bit, and the widths that stay on the run-time form against fp64.

The two forms promise the same arithmetic in the same order, so every comparison is on raw 32-bit words.  The inputs carry a few
channels scaled x50, as ConvNeXt activations do: with them the LayerNorm sums are ill-conditioned enough that another order of
the adds changes output bits (test_case_inputs_tell_summation_orders_apart shows that on the CPU), so a reordered reduction in
the specialised tail cannot pass by luck."""
import functools

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
EPS = 1e-6


@functools.lru_cache(maxsize=None)
def _case(n, c, h, w):
    """CPU tensors of one case: x (n, c, h, w) channels-last with outlier channels, [49][c] weights, conv bias, LN weight / bias."""
    g = torch.Generator().manual_seed(1000 * c + 10 * h + w)
    x = torch.randn(n, c, h, w, generator=g)
    outliers = torch.randperm(c, generator=g)[:5]
    x[:, outliers] *= 50.0
    x = x.contiguous(memory_format=torch.channels_last)
    w49c = torch.randn(49, c, generator=g) * 0.1
    bias = torch.randn(c, generator=g)
    ln_w = 1.0 + 0.2 * torch.randn(c, generator=g)
    ln_b = 0.2 * torch.randn(c, generator=g)
    return x, w49c, bias, ln_w, ln_b


def _conv_fp64(x, w49c, bias):
    c = x.shape[1]
    return F.conv2d(x.double(), w49c.t().reshape(c, 1, 7, 7).double(), bias.double(), padding=3, groups=c)


def _ln_fp32_sums(v, ln_w, ln_b, order):
    """LayerNorm over the last axis of v (fp32 conv outputs, pixels x C): the two sums in fp32 in the given order (a permutation of
    the channels, added left to right), everything else in fp64; fp32 result."""
    vp = v[:, order]
    s = torch.zeros(v.shape[0], dtype=torch.float32)
    for k in range(vp.shape[1]):
        s = s + vp[:, k]
    mean = s / v.shape[1]
    d = (vp - mean[:, None]) ** 2
    s2 = torch.zeros(v.shape[0], dtype=torch.float32)
    for k in range(d.shape[1]):
        s2 = s2 + d[:, k]
    var = s2 / v.shape[1]
    out = (v.double() - mean.double()[:, None]) * torch.rsqrt(var.double() + EPS)[:, None] * ln_w.double() + ln_b.double()
    return out.float()


def test_case_inputs_tell_summation_orders_apart():
    """No GPU: on a case of the builder, two orders of the LayerNorm sums give fp32 outputs that differ in at least one bit, so the
    bit comparison below can fail."""
    x, w49c, bias, ln_w, ln_b = _case(2, 128, 3, 5)
    v = _conv_fp64(x, w49c, bias).float().permute(0, 2, 3, 1).reshape(-1, 128)
    fwd = torch.arange(128)
    a = _ln_fp32_sums(v, ln_w, ln_b, fwd)
    b = _ln_fp32_sums(v, ln_w, ln_b, fwd.flip(0))
    assert not torch.equal(a.view(torch.int32), b.view(torch.int32))
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)   # ... and both are the same LayerNorm


def _run(hip, dev_case, specialise, fuse_ln, y_rows, tile, lds_w):
    x, w49c, bias, ln_w, ln_b = dev_case
    hip.set_option("dwconv_specialise", specialise)
    hip.set_option("dwconv_tile", tile)
    hip.set_option("dwconv_lds_w", lds_w)
    try:
        return hip.dwconv7x7_ln(x, w49c, bias, ln_w if fuse_ln else None, ln_b if fuse_ln else None, EPS, y_rows=y_rows)
    finally:
        hip.set_option("dwconv_specialise", 1)
        hip.set_option("dwconv_tile", -1)
        hip.set_option("dwconv_lds_w", 1)


def _assert_forms_bit_equal(hip, n, c, h, w, tiles=(0, 1, 2)):
    dev_case = tuple(t.to(DEV) for t in _case(n, c, h, w))
    lds_ws = (0, 1) if 49 * c * 4 <= 112 * 1024 else (1,)   # beyond 112 KB of weights the option has nothing to choose
    for fuse_ln in (True, False):
        for y_rows in (False, True):
            for tile in tiles:
                for lds_w in lds_ws:
                    got = _run(hip, dev_case, 1, fuse_ln, y_rows, tile, lds_w)
                    want = _run(hip, dev_case, 0, fuse_ln, y_rows, tile, lds_w)
                    where = f"n={n} c={c} {h}x{w} ln={fuse_ln} rows={y_rows} tile={tile} lds_w={lds_w}"
                    if not y_rows:
                        assert torch.isfinite(want).all(), where
                        assert torch.equal(got, want), where
                    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), where


@pytest.mark.gpu
@pytest.mark.parametrize("c", [128, 256, 512, 1024])
@pytest.mark.parametrize("h,w", [(3, 5), (8, 8), (16, 16), (17, 9)])
def test_specialised_equals_generic(hip, c, h, w):
    """N = 2; LayerNorm on / off, fp32 / f16x2-rows output, the three pixel tiles, weights in LDS or not.  (3x5 at C = 128 is
    four tiles in a workgroup of eight: a partly inactive tile group.)"""
    _assert_forms_bit_equal(hip, 2, c, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("n,tiles", [(40, (0, 1, 2)), (72, (0,))])
def test_specialised_equals_generic_persistent_walk(hip, n, tiles):
    """16x16 at C = 512 (four tiles per workgroup, one workgroup per CU): 40 images are 320 / 640 tile groups of the 2x4 / 1x4
    tiles, 72 images 288 groups of the 2x8 tile, each more than the 256 persistent workgroups, which then walk on."""
    _assert_forms_bit_equal(hip, n, 512, 16, 16, tiles)


@pytest.mark.gpu
def test_specialised_equals_generic_inactive_tail(hip):
    """3 images of 3x5 at C = 512: six 2x8 tiles, four per workgroup, so half of the last tile group has no tile."""
    _assert_forms_bit_equal(hip, 3, 512, 3, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [64, 32])
@pytest.mark.parametrize("specialise", [1, 0])
def test_other_widths_stay_on_the_runtime_form(hip, c, specialise):
    """C = 64 is the largest width the entry point admits besides the four specialised ones (power-of-two quad count <= 256), C = 32
    the widest whose LayerNorm group is narrower than a DPP row.  Tolerance: that of tests/test_gpu_net_kernels.py for this kernel."""
    x, w49c, bias, ln_w, ln_b = _case(2, c, 17, 9)
    conv = _conv_fp64(x, w49c, bias)
    ref_ln = F.layer_norm(conv.permute(0, 2, 3, 1), (c,), ln_w.double(), ln_b.double(), EPS).permute(0, 3, 1, 2)
    dev_case = tuple(t.to(DEV) for t in (x, w49c, bias, ln_w, ln_b))
    for fuse_ln, ref in ((True, ref_ln), (False, conv)):
        for tile in (0, 1, 2):
            y = _run(hip, dev_case, specialise, fuse_ln, False, tile, 1)
            torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-5, atol=2e-5)


@pytest.mark.gpu
def test_width_beyond_the_entry_point_is_refused(hip):
    x = torch.zeros(1, 2048, 2, 2, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError):
        hip.dwconv7x7_ln(x, torch.zeros(49, 2048, device=DEV), torch.zeros(2048, device=DEV))


@pytest.mark.gpu
def test_option_round_trip(hip):
    assert hip.get_option("dwconv_specialise") == 1
    hip.set_option("dwconv_specialise", 0)
    try:
        assert hip.get_option("dwconv_specialise") == 0
    finally:
        hip.set_option("dwconv_specialise", 1)
