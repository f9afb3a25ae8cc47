"""-m gpu: [UpsamplingBilinear2d(2), conv3x3 / 1 / 1, GroupNorm(, GELU)] at the low resolution (tap GEMM + csrc/upconv_gather.hip,
hip_lib.upsample2x_conv3x3_groupnorm_act) against the fp64 reference, against the path it replaces (hip_lib.upsample_bilinear2x +
conv3x3 on the upsampled tensor), bit stability, and the routing in heads.run_features.

Accuracy bar: the replaced path's own max |error| against fp64 on the same inputs, times MARGIN.  The low-resolution form rounds
more often per output (nine tap products of K = Cin each, then per tap three roundings of the interpolation and one of the sum,
where the replaced path rounds the interpolation once per input and sums 9 * Cin products in the matrix pipe), so it is not
expected below 1x; a decomposition that loses bits would need more than 4x.  MARGIN is the smallest power of two that held over
the 8 seeds at these shapes on MI355X: the worst new / old ratio was 1.48 on the convolution output (bf16x3, 2 x 2) and 1.54
behind GroupNorm + GELU (bf16x3, 1 x 1), with both paths between 2e-7 and 1.8e-6 (profiles/upconv_lowres.md has the figures)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.gdrn_modeling import heads, hip_layers

pytestmark = pytest.mark.gpu
DEV = "cuda"
CIN, COUT, GROUPS, EPS = 32, 128, 16, 1e-5
MARGIN = 2.0
SEEDS = range(8)
# (N, H, W, images per chunk; 0 = one launch)
SHAPES = [(2, 2, 2, 0),      # 4 x 4: every output pixel is a border pixel
          (1, 1, 1, 0),      # 1 x 1 -> 2 x 2: the scale is 0
          (3, 3, 5, 2),      # non-square, a chunk edge, M = 45 rows (no multiple of 256), blocks that hang over the image
          (2, 8, 8, 0)]
PACKS = {"f16x2": (hip_lib.pack_upconv_weight_f16x2, hip_lib.pack_conv_weight_f16x2),
         "bf16x3": (hip_lib.pack_upconv_weight_bf16x3, hip_lib.pack_conv_weight_bf16x3)}


def _inputs(n, h, w, seed):
    g = torch.Generator().manual_seed(1000 * seed + 100 * n + 10 * h + w)
    x = torch.randn(n, CIN, h, w, generator=g)
    wt = torch.randn(COUT, CIN, 3, 3, generator=g) * (9 * CIN) ** -0.5
    b = torch.randn(COUT, generator=g)
    gamma, beta = torch.rand(COUT, generator=g) + 0.5, torch.randn(COUT, generator=g)
    return x, wt, b, gamma, beta


def _reference(x, wt, b, gamma, beta):
    """fp64 on the host: (conv output, GroupNorm + GELU of it)."""
    up = nn.UpsamplingBilinear2d(scale_factor=2)(x.double())
    conv = F.conv2d(up, wt.double(), b.double(), padding=1)
    return conv, F.gelu(F.group_norm(conv, GROUPS, gamma.double(), beta.double(), EPS))


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _err(got, want):
    return float((got.double().cpu() - want).abs().max())


@pytest.mark.parametrize("pack", sorted(PACKS))
@pytest.mark.parametrize("n,h,w,chunk", SHAPES)
def test_accuracy_against_fp64_within_the_replaced_paths_error(hip, n, h, w, chunk, pack):
    pack_up, pack_conv = PACKS[pack]
    worst = {"conv": 0.0, "act": 0.0}
    rows = []
    for seed in SEEDS:
        x, wt, b, gamma, beta = _inputs(n, h, w, seed)
        want_conv, want_act = _reference(x, wt, b, gamma, beta)
        xd, (wd, bd, gd, bed) = _cl(x), _dev(wt, b, gamma, beta)
        old_conv = hip.conv3x3_f32_split(hip.upsample_bilinear2x(xd), pack_conv(wd), bd)
        old_act = hip.groupnorm_act(old_conv, gd, bed, GROUPS, EPS, gelu=True)
        new_conv, _, _ = hip.upsample2x_conv3x3_raw(xd, pack_up(wd), bd, GROUPS, chunk=chunk)
        new_act = hip.upsample2x_conv3x3_groupnorm_act(xd, pack_up(wd), bd, gd, bed, GROUPS, EPS, gelu=True, chunk=chunk)
        assert new_conv.shape == (n, COUT, 2 * h, 2 * w) and new_conv.is_contiguous(memory_format=torch.channels_last)
        e = (_err(old_conv, want_conv), _err(new_conv, want_conv), _err(old_act, want_act), _err(new_act, want_act))
        rows.append(e)
        worst["conv"] = max(worst["conv"], e[1] / e[0])
        worst["act"] = max(worst["act"], e[3] / e[2])
    for seed, e in zip(SEEDS, rows):
        print(f"upconv_lowres {pack} N={n} {h}x{w} seed {seed}: conv old {e[0]:.3e} new {e[1]:.3e} | GN+GELU old {e[2]:.3e} new {e[3]:.3e}")
    print(f"upconv_lowres {pack} N={n} {h}x{w}: worst new/old conv {worst['conv']:.2f} GN+GELU {worst['act']:.2f}")
    for seed, e in zip(SEEDS, rows):
        assert e[1] <= MARGIN * e[0], f"seed {seed}: conv |err| {e[1]:.3e} > {MARGIN} x {e[0]:.3e}"
        assert e[3] <= MARGIN * e[2], f"seed {seed}: GN+GELU |err| {e[3]:.3e} > {MARGIN} x {e[2]:.3e}"


@pytest.mark.parametrize("pack", sorted(PACKS))
@pytest.mark.parametrize("n,h,w,chunk", SHAPES)
def test_same_call_twice_and_any_chunking_are_bit_equal(hip, n, h, w, chunk, pack):
    x, wt, b, gamma, beta = _inputs(n, h, w, 0)
    xd, (wd, bd, gd, bed) = _cl(x), _dev(wt, b, gamma, beta)
    w_pk = PACKS[pack][0](wd)
    ref_raw, ref_part, P = hip.upsample2x_conv3x3_raw(xd, w_pk, bd, GROUPS)
    ref = hip.upsample2x_conv3x3_groupnorm_act(xd, w_pk, bd, gd, bed, GROUPS, EPS, gelu=True)
    assert torch.isfinite(ref).all() and ref_part.shape == (n, P, GROUPS, 2)
    for c in sorted({0, 1, 2, chunk, n}):
        raw, part, _ = hip.upsample2x_conv3x3_raw(xd, w_pk, bd, GROUPS, chunk=c)
        assert torch.equal(raw, ref_raw) and torch.equal(part, ref_part), f"chunk {c}"
        assert torch.equal(hip.upsample2x_conv3x3_groupnorm_act(xd, w_pk, bd, gd, bed, GROUPS, EPS, gelu=True, chunk=c), ref), f"chunk {c}"
    # the statistics are those of the tensor that was written: the two-pass GroupNorm of it agrees to rounding
    two_pass = hip.groupnorm_act(ref_raw, gd, bed, GROUPS, EPS, gelu=True)
    assert float((two_pass - ref).abs().max()) <= 1e-5
    # no bias: nothing is added
    raw0, _, _ = hip.upsample2x_conv3x3_raw(xd, w_pk, None, GROUPS)
    assert float((raw0 + bd.view(1, -1, 1, 1) - ref_raw).abs().max()) <= 1e-5


def test_on_a_side_stream_beside_a_gemm_is_bitwise_the_serial_result(hip):
    torch.manual_seed(3)
    conv = nn.Conv2d(256, 256, 3, padding=1, bias=False).to(DEV)
    xg = torch.randn(64, 256, 32, 32, device=DEV).contiguous(memory_format=torch.channels_last)      # 256 tiles of 256 x 128: the three-product kernel
    x, wt, b, gamma, beta = _inputs(3, 3, 5, 1)
    xd, (wd, bd, gd, bed) = _cl(x), _dev(wt, b, gamma, beta)
    x8 = _cl(_inputs(2, 8, 8, 1)[0])
    w_pk = hip.pack_upconv_weight_f16x2(wd)
    with torch.no_grad():
        n0 = hip.x3_launch_count()
        yg_ref = hip_layers.conv2d(conv, xg).clone()
        assert hip.x3_launch_count() > n0, "the companion must be the three-product (f16 MFMA) GEMM"
        refs = [hip.upsample2x_conv3x3_groupnorm_act(t, w_pk, bd, gd, bed, GROUPS, EPS, gelu=True, chunk=c).clone() for t, c in ((xd, 2), (x8, 0))]
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        for rep in range(3):
            with torch.cuda.stream(sb):
                ygs = [hip_layers.conv2d(conv, xg) for _ in range(3)]
            with torch.cuda.stream(sa):
                got = [[hip.upsample2x_conv3x3_groupnorm_act(t, w_pk, bd, gd, bed, GROUPS, EPS, gelu=True, chunk=c) for t, c in ((xd, 2), (x8, 0))]
                       for _ in range(4)]
            torch.cuda.synchronize()
            assert all(torch.equal(a, r) for pair in got for a, r in zip(pair, refs)), f"rep {rep}: the gather differs beside the GEMM"
            assert all(torch.equal(y, yg_ref) for y in ygs), f"rep {rep}: the GEMM differs beside the gather"


class _Knobs:
    """The library option and the routing's size rule for one test, restored afterwards."""

    def __init__(self, option, min_pixels=0):
        self.option, self.min_pixels = option, min_pixels

    def __enter__(self):
        self.old = hip_lib.get_option("upconv_lowres"), hip_layers._UPCONV_MIN_PIXELS
        hip_lib.set_option("upconv_lowres", self.option)
        hip_layers.set_upconv_lowres(min_pixels=self.min_pixels)

    def __exit__(self, *exc):
        hip_lib.set_option("upconv_lowres", self.old[0])
        hip_layers.set_upconv_lowres(min_pixels=self.old[1])
        return False


def _head(up, cin=CIN):
    torch.manual_seed(5)
    feats = nn.ModuleList([up, heads.ConvModule(cin, COUT, 3, padding=1, norm="GN", num_gn_groups=GROUPS, act="GELU")])
    with torch.no_grad():
        feats[1].conv.weight.normal_(0.0, (9 * cin) ** -0.5)
        feats[1].gn.weight.uniform_(0.5, 1.5)
        feats[1].gn.bias.normal_()
    return feats.to(DEV).eval()


def test_option_default_and_option_0_is_todays_two_calls_bit_for_bit(hip):
    assert hip.get_option("upconv_lowres") == 1
    feats = _head(nn.UpsamplingBilinear2d(scale_factor=2))
    x = _cl(_inputs(2, 8, 8, 2)[0])
    with torch.no_grad():
        n0 = hip_layers.fallback_launches()
        today = feats[1](hip.upsample_bilinear2x(x))
        with _Knobs(0):
            assert hip.get_option("upconv_lowres") == 0
            off = heads.run_features(feats, x)
        with _Knobs(1):
            on = heads.run_features(feats, x)
        with _Knobs(1, min_pixels=4 * 2 * 8 * 8 + 1):      # below the size rule: as today
            small = heads.run_features(feats, x)
        cm = feats[1]
        w_pk = hip.pack_upconv_weight_bf16x3(cm.conv.weight)    # 128 rows: the six-product kernels, as the routing picks here
        direct = hip.upsample2x_conv3x3_groupnorm_act(x, w_pk, None, cm.gn.weight, cm.gn.bias, GROUPS, cm.gn.eps, gelu=True)
    assert hip_layers.fallback_launches() == n0
    assert torch.equal(off, today) and torch.equal(small, today)
    assert torch.equal(on, direct) and not torch.equal(on, today)
    assert float((on - today).abs().max()) <= 1e-5
    assert hip.get_option("upconv_lowres") == 1
    with pytest.raises(RuntimeError, match="unknown option 'upconv_highres'"):
        hip.get_option("upconv_highres")


@pytest.mark.parametrize("what", ["nearest", "cin24"])
def test_heads_outside_the_form_fall_back_and_are_counted_as_today(hip, what):
    """Nearest upsampling (a PyTorch operator in front of the ConvModule) and Cin % 32 != 0 (the convolution goes to MIOpen): the
    same launches, the same fallback count and the same values whatever the option says."""
    if what == "nearest":
        feats, cin = _head(nn.UpsamplingNearest2d(scale_factor=2)), CIN
    else:
        feats, cin = _head(nn.UpsamplingBilinear2d(scale_factor=2), cin=24), 24
    g = torch.Generator().manual_seed(9)
    x = _cl(torch.randn(2, cin, 8, 8, generator=g))
    out, counts = [], []
    with torch.no_grad():
        for option in (0, 1):
            with _Knobs(option):
                n0 = hip_layers.fallback_launches()
                out.append(heads.run_features(feats, x))
                counts.append(hip_layers.fallback_launches() - n0)
    assert counts[0] == counts[1] >= 1, counts
    assert torch.equal(out[0], out[1])
    with torch.no_grad():
        want = F.gelu(feats[1].gn(feats[1].conv(feats[0](x))))
    assert float((out[1] - want).abs().max()) <= 1e-4
