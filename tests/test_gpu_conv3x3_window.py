"""-m gpu: the window-staged form of the three-product conv3x3 (csrc/gemm_split2_pipe.hip: conv3x3_window_kernel, library option
conv3x3_window = 1) against the form that stages one operand image per tap (option 0) and against the oracles.

Shapes (N, H, W): the smallest at which each mechanism of the window can go wrong — (1, 16, 16) one tile with all four borders in
its halo; (3, 16, 16) one tile per image (neighbours must not leak); (1, 32, 32) / (2, 32, 32) top, interior and bottom tiles,
and a second image; (1, 8, 32) / (1, 4, 64) the tile is the whole image; (1, 64, 64) 16 tiles of 4 rows.  Cin = 32 / 96: two
chunks, and six chunks with the window buffers (2) and the weight slots (4) out of phase; Cout = 128 / 256: one / two column tiles.

  * exact: on the lattices of tests/split_lattice.py a launch has ONE correct bit pattern in any summation order: option 1 must
    be torch.equal to the oracle and to option 0, with and without bias; with GroupNorm statistics the stored values and the fp64
    partial sums must be those of option 0;
  * guard: the input sits inside a larger allocation with (W + 3) pixels of NaN before and behind it — a halo read outside the
    tensor would show as NaN in the output and as a NONFINITE range word;
  * random data: max |error| against F.conv2d in fp64 of option 1 within MARGIN = 2 x that of option 0, per seed, bias and GELU
    epilogues (the two differ in the order of the same 9 Cin three-product terms only: a power of two above 2 would need another
    cause; profiles/conv3x3_window.md has the measured ratios);
  * range words: a patch of near-zero pixels raises SMALL_ROWS, a NaN element NONFINITE, under both options alike;
  * routing: W = 17 and H % (256 / W) != 0 run the per-tap form with the option on (the bits of option 0)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests import split_lattice as SL

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 16, 16), (3, 16, 16), (1, 32, 32), (2, 32, 32), (1, 8, 32), (1, 4, 64), (1, 64, 64)]
CINS, COUTS = (32, 96), (128, 256)
SEEDS = range(8)
MARGIN = 2.0


@contextlib.contextmanager
def _option(hip, value):
    old = hip.get_option("conv3x3_window")
    hip.set_option("conv3x3_window", value)
    try:
        yield
    finally:
        hip.set_option("conv3x3_window", old)


def _nhwc(x):
    return x.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _conv(hip, option, x, pk, bias, gelu=False, x3_slot=0):
    with _option(hip, option):
        return hip.conv3x3_f32_split(x, pk, bias, gelu, x3_slot=x3_slot)


def _conv_gn(hip, option, x, pk, bias, cout):
    """The convolution with GroupNorm statistics through the C ABI: (stored values, fp64 partial sums)."""
    n, cin, h, w = x.shape
    groups = cout // 8
    lib = hip.load()
    P = lib.gdrnpp_conv3x3_gnstats_partials(h, w)
    assert P > 0
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=DEV).contiguous(memory_format=torch.channels_last)
    part = torch.full((n, P, groups, 2), float("nan"), dtype=torch.float64, device=DEV)
    with _option(hip, option):
        rc = lib.gdrnpp_conv3x3_f32_split2(x.data_ptr(), pk.data_ptr(), bias.data_ptr(), y.data_ptr(), part.data_ptr(), n, h, w, cin, cout,
                                           groups, 0, None, hip.current_stream())
    assert rc == 0, lib.gdrnpp_last_error()
    return y, part


def _exact(got, want, what):
    got = got.detach().cpu()
    if not torch.equal(got.double(), want):
        pytest.fail(f"{what}: not the exact value\n{SL.mismatch_report(got, want)}")


def test_option_is_registered_and_on(hip):
    assert hip.get_option("conv3x3_window") == 1
    with _option(hip, 0):
        assert hip.get_option("conv3x3_window") == 0
    assert hip.get_option("conv3x3_window") == 1


@pytest.mark.parametrize("kind", ("int", "hl"))
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_exact_against_the_oracle_and_option_0(hip, n, h, w, cin, cout, kind):
    c = SL.conv_case(n, cin, h, w, cout, 3, 1, 1, kind)
    x, pk, b = _nhwc(c["x"]), hip.pack_conv_weight_f16x2(c["w"].to(DEV)), c["bias"].to(DEV)
    what = f"conv3x3 window ({n}, {cin}, {h}, {w}) -> {cout} {kind}"
    for with_bias in (False, True):
        new, old = (_conv(hip, o, x, pk, b if with_bias else None) for o in (1, 0))
        _exact(new, c["want"][with_bias], f"{what} bias={with_bias}")
        assert torch.equal(new, old), f"{what} bias={with_bias}: option 1 differs from option 0"
    (y1, p1), (y0, p0) = (_conv_gn(hip, o, x, pk, b, cout) for o in (1, 0))
    _exact(y1, c["want"][True], f"{what} with GroupNorm statistics")
    assert torch.equal(y1, y0), f"{what}: stored values with GroupNorm statistics differ from option 0"
    assert torch.equal(p1, p0) and torch.isfinite(p1).all(), f"{what}: GroupNorm partial sums differ from option 0"
    assert hip.split2_range_words() == {}


@pytest.mark.parametrize("cin", CINS)
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_halo_never_reads_outside_the_tensor(hip, n, h, w, cin):
    """NaN in the (W + 3) pixels before and behind the tensor: the output stays finite and exact, no range word."""
    cout = 128
    c = SL.conv_case(n, cin, h, w, cout, 3, 1, 1, "int")
    pad, pixels = (w + 3) * cin, n * h * w * cin
    buf = torch.full((pixels + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    buf[pad:pad + pixels] = c["x"].to(DEV).permute(0, 2, 3, 1).reshape(-1)
    x = buf[pad:pad + pixels].view(n, h, w, cin).permute(0, 3, 1, 2)
    assert x.data_ptr() == buf.data_ptr() + 4 * pad and torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + pixels:]).all()
    pk, b = hip.pack_conv_weight_f16x2(c["w"].to(DEV)), c["bias"].to(DEV)
    out = _conv(hip, 1, x, pk, b)
    assert torch.isfinite(out).all()
    _exact(out, c["want"][True], f"guarded conv3x3 window ({n}, {cin}, {h}, {w})")
    y, part = _conv_gn(hip, 1, x, pk, b, cout)
    assert torch.equal(y, out) and torch.isfinite(part).all()
    assert hip.split2_range_words() == {}


@pytest.mark.parametrize("cin,cout", [(32, 256), (96, 128)])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_random_data_error_within_twice_option_0(hip, n, h, w, cin, cout):
    rows = []
    for seed in SEEDS:
        gen = torch.Generator().manual_seed(1000 * seed + 31 * h + w + cin)
        x = torch.randn(n, cin, h, w, generator=gen)
        wt = torch.randn(cout, cin, 3, 3, generator=gen) * (9 * cin) ** -0.5
        b = torch.randn(cout, generator=gen)
        want = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
        xd, pk, bd = _nhwc(x), hip.pack_conv_weight_f16x2(wt.to(DEV)), b.to(DEV)
        for gelu, ref in ((False, want), (True, F.gelu(want))):
            e1, e0 = (float((_conv(hip, o, xd, pk, bd, gelu).double().cpu() - ref).abs().max()) for o in (1, 0))
            rows.append((seed, gelu, e1, e0))
    for seed, gelu, e1, e0 in rows:
        print(f"conv3x3_window ({n}, {cin}, {h}, {w}) -> {cout} seed {seed} gelu={int(gelu)}: option 1 {e1:.3e} option 0 {e0:.3e} ratio {e1 / e0:.2f}")
    print(f"conv3x3_window ({n}, {cin}, {h}, {w}) -> {cout}: worst option 1 / option 0 {max(r[2] / r[3] for r in rows):.2f}")
    for seed, gelu, e1, e0 in rows:
        assert e1 <= MARGIN * e0, f"seed {seed} gelu={gelu}: |err| {e1:.3e} > {MARGIN} x {e0:.3e}"
    assert hip.split2_range_words() == {}


@pytest.mark.parametrize("option", (0, 1))
def test_range_words_under_both_options(hip, option):
    torch.manual_seed(2)
    xc = torch.randn(2, 64, 32, 32, device=DEV).contiguous(memory_format=torch.channels_last)
    pk = hip.pack_conv_weight_f16x2(torch.randn(128, 64, 3, 3, device=DEV) * (9 * 64) ** -0.5)
    _conv(hip, option, xc, pk, None, x3_slot=5)          # corner pixels see 4 of 9 taps: rms 2/3, still inside
    assert hip.split2_range_words() == {}
    small = xc.clone()
    small[1, :, 10:20, 10:20] *= 0.01                    # a patch of tiny pixels: the rows of its interior are below 2^-4 rms
    _conv(hip, option, small, pk, None, x3_slot=5)
    assert hip.split2_range_words() == {5: hip.X3_SMALL_ROWS}
    small[1, :, 10:20, 10:20] = 0.0                      # zero rows are exact: no word
    _conv(hip, option, small, pk, None, x3_slot=5)
    assert hip.split2_range_words() == {}
    nan = xc.clone()
    nan[1, 7, 0, 31] = float("nan")                      # a border pixel: some of its taps are zeroed, the centre tap is not
    out = _conv(hip, option, nan, pk, None, x3_slot=6)
    assert not torch.isfinite(out[1]).all() and torch.isfinite(out[0]).all()
    assert hip.split2_range_words() == {6: hip.X3_NONFINITE}


@pytest.mark.parametrize("n,h,w", [(2, 16, 17), (1, 12, 32), (1, 6, 64), (3, 8, 16)])
def test_other_shapes_keep_the_per_tap_form(hip, n, h, w):
    """W outside {16, 32, 64}, or tiles that would span images: the bits of option 0 with the option on (and the oracle's)."""
    c = SL.conv_case(n, 32, h, w, 128, 3, 1, 1, "hl")
    x, pk, b = _nhwc(c["x"]), hip.pack_conv_weight_f16x2(c["w"].to(DEV)), c["bias"].to(DEV)
    new, old = (_conv(hip, o, x, pk, b) for o in (1, 0))
    assert torch.equal(new, old)
    _exact(new, c["want"][True], f"conv3x3 ({n}, 32, {h}, {w}) outside the window form")
    torch.manual_seed(h + w)
    xr = torch.randn(n, 32, h, w, device=DEV).contiguous(memory_format=torch.channels_last)
    assert torch.equal(_conv(hip, 1, xr, pk, b, True), _conv(hip, 0, xr, pk, b, True))      # random data: any other kernel would show
    assert hip.split2_range_words() == {}
