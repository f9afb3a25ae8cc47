"""The YOLOX detector forward on csrc/yolox_net.hip against fp64 PyTorch and the reference's fixtures
(tests/golden/yolox_net_golden_<case>.npz, recorded from the reference's own modules).

Bars
  whole model   per output group |ours - reference fp64| <= 4 * e_ref, e_ref = max |reference fp32 - reference fp64| (fixture).
  convolution   max |ours - fp64| / max |fp64| <= 4 * the same figure of PyTorch's own fp32 convolution (CPU) on the same folded
                weights and input — and at 640 -> 640, 3x3, stride 1 no more than 2 * the error of hip_lib.conv2d_f32_split.
  data movement (Focus, SPP, upsample) and run-to-run repeats: bit-exact.
Every figure is printed before it is asserted."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import yolox_seeded as YS  # noqa: E402

from gdrnpp_bop2022_amd import hip_lib  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox import models as M  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox.utils.boxes import postprocess  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR = 4.0
CONV_SHAPES = [tuple(int(v) for v in r) for r in np.load(os.path.join(GOLDEN, "yolox_net_golden_x320.npz"))["conv_shapes"]]
ACTS = ("none", "silu", "sigmoid")


def load_golden(case):
    return np.load(os.path.join(GOLDEN, f"yolox_net_golden_{case}.npz"))


def natural_size(cin):
    """The spatial size at which YOLOX-x at 640 x 640 meets an input of ``cin`` channels (80 / 40 / 20 / 10)."""
    return 80 if cin <= 160 else 40 if cin == 320 else 20 if cin == 640 else 10


def act_ref(y, act):
    return F.silu(y) if act == "silu" else torch.sigmoid(y) if act == "sigmoid" else y


def run_conv(cin, cout, ks, stride, b, h, w, act, with_res, seed, a_off=4, c_off=3, pad_c=5):
    """One launch on slices with non-zero offsets inside NaN-filled buffers -> (ours, fp64, torch fp32) as [b,oh,ow,cout] and the
    output buffer."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, h, w, cin, generator=g)
    wt = torch.randn(cout, cin, ks, ks, generator=g) * (cin * ks * ks) ** -0.5
    bias = torch.randn(cout, generator=g)
    pad = (ks - 1) // 2
    oh, ow = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    res = torch.randn(b, oh, ow, cout, generator=g) if with_res else None

    def ref(dt):
        y = F.conv2d(x.to(dt).permute(0, 3, 1, 2), wt.to(dt), bias.to(dt), stride, pad).permute(0, 2, 3, 1)
        y = act_ref(y, act)
        return y + res.to(dt) if with_res else y

    y64, y32 = ref(torch.float64), ref(torch.float32)
    abuf = torch.full((b, h, w, a_off + cin + 4), float("nan"), device=DEV)
    abuf[..., a_off:a_off + cin] = x.to(DEV)
    cbuf = torch.full((b, oh, ow, c_off + cout + pad_c), float("nan"), device=DEV)
    rbuf, r_off = None, 0
    if with_res:
        r_off = 2
        rbuf = torch.full((b, oh, ow, r_off + cout + 1), float("nan"), device=DEV)
        rbuf[..., r_off:r_off + cout] = res.to(DEV)
    wk = hip_lib.pack_conv_weight_kmajor(wt.to(DEV))
    hip_lib.conv_bias_act_f32(abuf, a_off, cin, wk, bias.to(DEV), cbuf, c_off, cout, ks, stride, act, rbuf, r_off)
    torch.cuda.synchronize()
    first = cbuf.clone()
    hip_lib.conv_bias_act_f32(abuf, a_off, cin, wk, bias.to(DEV), cbuf, c_off, cout, ks, stride, act, rbuf, r_off)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), cbuf.view(torch.int32)), "two runs differ bit for bit"
    out = cbuf.cpu()
    assert torch.isnan(out[..., :c_off]).all() and torch.isnan(out[..., c_off + cout:]).all(), "written outside the output slice"
    return out[..., c_off:c_off + cout], y64, y32


def check_conv(tag, got, y64, y32):
    scale = float(y64.abs().max())
    e_ours = float((got.double() - y64).abs().max()) / scale
    e_torch = float((y32.double() - y64).abs().max()) / scale
    print(f"{tag}: ours {e_ours:.3e}  torch fp32 {e_torch:.3e}  ratio {e_ours / e_torch:.2f}")
    assert torch.isfinite(got).all()
    assert e_ours <= FACTOR * e_torch, (tag, e_ours, e_torch)
    return e_ours


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_at_every_yolox_x_shape_natural_size(hip, shape):
    cin, cout, ks, stride = shape
    n = natural_size(cin)
    i = CONV_SHAPES.index(shape)
    got, y64, y32 = run_conv(cin, cout, ks, stride, 1, n, n, ACTS[i % 3], i % 2 == 1, 100 + i)
    check_conv(f"{shape} at {n}x{n} {ACTS[i % 3]} res={i % 2}", got, y64, y32)


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_at_every_yolox_x_shape_odd_size_partial_tiles(hip, shape):
    """13 x 19, batch 2: 494 (stride 1) or 140 (stride 2) output pixels — a partial last M tile, stride-2 edge rows and columns."""
    cin, cout, ks, stride = shape
    i = CONV_SHAPES.index(shape)
    got, y64, y32 = run_conv(cin, cout, ks, stride, 2, 13, 19, ACTS[(i + 1) % 3], i % 2 == 0, 200 + i)
    check_conv(f"{shape} at 13x19 {ACTS[(i + 1) % 3]} res={1 - i % 2}", got, y64, y32)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", [(80, 80, 3, 1), (320, 21, 1, 1), (160, 320, 3, 2)], ids=lambda s: "x".join(map(str, s)))
def test_conv_every_activation_with_and_without_residual(hip, shape, act, with_res):
    cin, cout, ks, stride = shape
    got, y64, y32 = run_conv(cin, cout, ks, stride, 2, 20, 12, act, with_res, 300)
    check_conv(f"{shape} {act} res={with_res}", got, y64, y32)


def test_conv_residual_may_be_the_output_slice_itself(hip):
    g = torch.Generator().manual_seed(5)
    x, wt, bias = torch.randn(1, 20, 20, 80, generator=g), torch.randn(80, 80, 3, 3, generator=g) / 27, torch.randn(80, generator=g)
    cat = torch.randn(1, 20, 20, 160, generator=g)
    want = (F.silu(F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), bias.double(), 1, 1)).permute(0, 2, 3, 1) + cat[..., :80].double())
    buf = cat.to(DEV)
    hip_lib.conv_bias_act_f32(x.to(DEV), 0, 80, hip_lib.pack_conv_weight_kmajor(wt.to(DEV)), bias.to(DEV), buf, 0, 80, 3, 1, "silu", buf, 0)
    out = buf.cpu()
    assert torch.equal(out[..., 80:], cat[..., 80:])
    assert (out[..., :80].double() - want).abs().max() <= 1e-5 * want.abs().max()


def test_conv_error_is_no_more_than_twice_the_split_gemms_at_640_640_3x3(hip):
    cin = cout = 640
    got, y64, y32 = run_conv(cin, cout, 3, 1, 1, 20, 20, "none", False, 7, a_off=0, c_off=0, pad_c=0)
    e_ours = check_conv("640->640 3x3", got, y64, y32)
    g = torch.Generator().manual_seed(7)         # the same draws as run_conv
    x = torch.randn(1, 20, 20, cin, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (cin * 9) ** -0.5
    bias = torch.randn(cout, generator=g)
    x_cl = x.permute(0, 3, 1, 2).to(DEV).contiguous(memory_format=torch.channels_last)
    y = hip_lib.conv2d_f32_split(x_cl, hip_lib.pack_conv_weight_bf16x3(wt.to(DEV)), bias.to(DEV), 3, 3, 1, 1)
    e_split = float((y.cpu().double().permute(0, 2, 3, 1) - y64).abs().max()) / float(y64.abs().max())
    print(f"640->640 3x3 s1 at 20x20: conv_bias_act_f32 {e_ours:.3e}  conv2d_f32_split {e_split:.3e}  ratio {e_ours / e_split:.2f}")
    assert e_ours <= 2.0 * e_split


def test_focus_channel_order_is_bit_exact(hip):
    x = torch.randn(2, 3, 26, 38, device=DEV)
    y = torch.full((2, 13, 19, 17), float("nan"), device=DEV)
    hip_lib.yolox_focus(x, y, 3)
    want = M.network_blocks.space_to_depth(x).permute(0, 2, 3, 1)
    assert torch.equal(y[..., 3:15], want) and torch.isnan(y[..., :3]).all() and torch.isnan(y[..., 15:]).all()


@pytest.mark.parametrize("hw", [(20, 20), (10, 10), (7, 5)])
def test_spp_is_bit_exact_with_negative_inputs(hip, hw):
    h, w = hw
    c, off = 24, 4
    x = -torch.rand(2, h, w, c, device=DEV) - 1.0          # all negative: a zero-padded pool would win every border window
    buf = torch.full((2, h, w, off + 4 * c + 3), float("nan"), device=DEV)
    buf[..., off:off + c] = x
    hip_lib.spp_maxpool_5_9_13(buf, off, c)
    for i, k in enumerate((5, 9, 13)):
        want = F.max_pool2d(x.permute(0, 3, 1, 2), k, 1, k // 2).permute(0, 2, 3, 1)
        assert torch.equal(buf[..., off + (i + 1) * c:off + (i + 2) * c], want), k
    assert torch.equal(buf[..., off:off + c], x) and torch.isnan(buf[..., :off]).all() and torch.isnan(buf[..., off + 4 * c:]).all()


def test_upsample_into_slice_is_bit_exact(hip):
    x = torch.randn(2, 5, 7, 40, device=DEV)
    y = torch.full((2, 10, 14, 48), float("nan"), device=DEV)
    hip_lib.upsample_nearest2x_slice(x, 8, y, 4, 24)
    want = F.interpolate(x[..., 8:32].permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    assert torch.equal(y[..., 4:28], want) and torch.isnan(y[..., :4]).all() and torch.isnan(y[..., 28:]).all()


def test_prediction_layers_decode_at_exact_anchor_offsets_non_square(hip):
    """Three levels of a 96 x 160 image: the box / objectness / class layers write det_preds[B, A, 5 + C] in place."""
    nc, cin, b = 7, 32, 2
    levels = [(12, 20, 8), (6, 10, 16), (3, 5, 32)]
    A = sum(h * w for h, w, _ in levels)
    det = torch.full((b, A, 5 + nc), float("nan"), device=DEV)
    g = torch.Generator().manual_seed(11)
    want = torch.empty(b, A, 5 + nc, dtype=torch.float64)
    row0 = 0
    for h, w, s in levels:
        f = torch.randn(b, h, w, cin, generator=g)
        ws = {k: torch.randn(n, cin, 1, 1, generator=g) * 0.3 for k, n in (("reg", 4), ("obj", 1), ("cls", nc))}
        bs = {k: torch.randn(v.shape[0], generator=g) for k, v in ws.items()}
        fd = f.to(DEV)
        for k, act, off in (("reg", "yolox_box", 0), ("obj", "sigmoid", 4), ("cls", "sigmoid", 5)):
            hip_lib.conv_bias_act_f32(fd, 0, cin, hip_lib.pack_conv_weight_kmajor(ws[k].to(DEV)), bs[k].to(DEV), det, off, ws[k].shape[0],
                                      1, 1, act, c_img_rows=A, c_row0=row0, dec_stride=float(s))
        o = {k: F.conv2d(f.double().permute(0, 3, 1, 2), ws[k].double(), bs[k].double()).permute(0, 2, 3, 1) for k in ws}
        yv, xv = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        grid = torch.stack((xv, yv), -1).double()
        lvl = torch.cat([(o["reg"][..., :2] + grid) * s, torch.exp(o["reg"][..., 2:]) * s, torch.sigmoid(o["obj"]), torch.sigmoid(o["cls"])], -1)
        want[:, row0:row0 + h * w] = lvl.reshape(b, h * w, -1)
        row0 += h * w
    got = det.cpu().double()
    assert torch.isfinite(got).all(), "an anchor row was left unwritten"
    err = (got - want).abs()
    print(f"decode: box err {err[..., :4].max():.3e} (values to {want[..., :4].abs().max():.1f}), score err {err[..., 4:].max():.3e}")
    assert err[..., :4].max() <= 2e-6 * want[..., :4].abs().max() and err[..., 4:].max() <= 1e-6


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(size):
        if size not in cache:
            d, w = YS.SIZES[size]
            net = M.build_yolox(d, w, 21)
            net.load_state_dict(YS.state_dict_for(net), strict=True)
            cache[size] = net.to(DEV).eval()
        return cache[size]
    return get


def hip_forward(net, case):
    x = YS.image(case).to(DEV)
    n0 = hip_layers.fallback_launches()
    with torch.no_grad():
        det = net(x)["det_preds"]
    torch.cuda.synchronize()
    assert hip_layers.fallback_launches() == n0, hip_layers.last_fallback()
    return x, det


@pytest.mark.parametrize("case", list(YS.CASES))
def test_whole_model_is_within_the_bar_of_the_reference(hip, nets, case):
    from test_yolox_model_cpu import check_against_fixture

    g = load_golden(case)
    net = nets(case[0])
    x, det = hip_forward(net, case)
    assert det.dtype == torch.float32 and det.is_contiguous() and torch.isfinite(det).all()
    check_against_fixture(det.cpu().numpy(), g, case, "HIP path")
    with torch.no_grad():
        again = net(x)["det_preds"]
    assert torch.equal(det.view(torch.int32), again.view(torch.int32)), "two forwards differ bit for bit"


def test_undecoded_output_of_the_hip_path(hip, nets):
    net = nets("s")
    x, det = hip_forward(net, "s256x384")
    net.head.decode_in_inference = False
    try:
        with torch.no_grad():
            raw = net(x)
    finally:
        net.head.decode_in_inference = True
    assert isinstance(raw, torch.Tensor) and torch.equal(raw[..., 4:], det[..., 4:])
    grids, strides = net.head.grids_and_strides(torch.float32, DEV)
    assert torch.equal((raw[..., :2] + grids) * strides, det[..., :2])
    assert torch.allclose(torch.exp(raw[..., 2:4]) * strides, det[..., 2:4], rtol=1e-6, atol=0)


def test_every_kernel_of_the_forward_is_this_librarys(hip, nets):
    import check_isa_hazards as C
    from torch.profiler import ProfilerActivity, profile

    ours = {C.kernel_base_name(n) for n in C.kernel_names(hip_lib.LIB_PATH)}
    assert {"conv_bias_act_kernel", "focus_kernel", "spp_kernel", "upsample2x_kernel"} <= ours
    net = nets("s")
    x, _ = hip_forward(net, "s256x384")          # warm: weights folded and packed, buffers allocated
    fills = hip_layers.cache_fills()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if str(ev.device_type).endswith("CUDA")]
    if not names:
        pytest.skip("torch.profiler returned no device events here: the kernel-name whitelist cannot be checked on this box")
    assert hip_layers.cache_fills() == fills
    moves = ("copyBuffer", "fillBuffer", "Memcpy", "Memset")          # the runtime's own copies / fills compute nothing
    foreign = sorted({n for n in names if C.kernel_base_name(n) not in ours and not any(t in n for t in moves)})
    assert not foreign, foreign
    n_conv = sum(1 for m in net.modules() if isinstance(m, torch.nn.Conv2d))
    count = lambda tok: sum(tok in n for n in names)  # noqa: E731
    assert count("conv_bias_act_kernel") == n_conv
    assert (count("focus_kernel"), count("spp_kernel"), count("upsample2x_kernel")) == (1, 1, 2)


def test_forward_on_a_side_stream_is_bit_equal(hip, nets):
    net = nets("s")
    x, det = hip_forward(net, "s256x384")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        det_side = net(x)["det_preds"]
    side.synchronize()
    assert torch.equal(det.view(torch.int32), det_side.view(torch.int32))


def test_disabled_hip_layers_take_the_operator_path_and_agree(hip, nets):
    net = nets("s")
    x, det = hip_forward(net, "s256x384")
    hip_layers.set_enabled(False)
    try:
        with torch.no_grad():
            want = net(x)["det_preds"]
    finally:
        hip_layers.set_enabled(True)
    assert (det[..., 4:] - want[..., 4:]).abs().max() < 1e-4 and (det[..., :4] - want[..., :4]).abs().max() < 1e-2


@pytest.mark.parametrize("case", [c for c, v in YS.CASES.items() if not v["rows"]])
def test_hand_off_to_postprocess_keeps_the_references_boxes(hip, nets, case):
    """Thresholds and their margins come from the fixture: the reference's fp32 and fp64 outputs keep the same set, no score
    within 8 e_ref of conf_thre, no same-class IoU within 1e-4 of nms_thre."""
    g = load_golden(case)
    conf, nms = float(g[f"{case}/conf_thre"]), float(g[f"{case}/nms_thre"])
    assert float(g[f"{case}/score_margin"]) > 8 * float(g[f"{case}/e_ref_score"]) and float(g[f"{case}/iou_margin"]) > 1e-4
    _, det = hip_forward(nets(case[0]), case)
    kept = postprocess(det, 21, conf, nms)
    counts = g[f"{case}/kept_counts"]
    want = g[f"{case}/kept32"]
    assert [0 if k is None else len(k) for k in kept] == [int(c) for c in counts]
    got = torch.cat([k for k in kept if k is not None]).cpu().numpy()
    assert np.array_equal(got[:, 6], want[:, 6]), "classes or keep order differ"
    e_box = 2 * max(float(g[f"{case}/e_ref_xy"]), float(g[f"{case}/e_ref_wh"]))     # corners = centre -+ size / 2
    err = np.abs(got[:, :4].astype(np.float64) - want[:, :4]).max()
    print(f"hand-off {case}: kept {counts}, corner err {err:.3e} (bar {FACTOR * e_box:.3e})")
    assert err <= FACTOR * e_box


def _raw_call(lib, **over):
    n = torch.full((1, 4, 4, 16), float("nan"), device=DEV)
    a = torch.zeros(1, 4, 4, 16, device=DEV)
    w = torch.zeros(16, 16, device=DEV)
    args = dict(a=a.data_ptr(), lda=16, a_off=0, w=w.data_ptr(), ldw=16, bias=None, res=None, ldr=0, r_off=0, c=n.data_ptr(), ldc=16, c_off=0,
                c_img_rows=0, c_row0=0, B=1, H=4, W=4, cin=16, cout=16, ks=1, stride=1, act=0, dec_stride=0.0, stream=None)
    args.update(over)
    rc = lib.gdrnpp_conv_bias_act_f32(*args.values())
    torch.cuda.synchronize()
    return rc, (lib.gdrnpp_last_error() or b"").decode(), n, (a, w)


@pytest.mark.parametrize("over,text", [
    (dict(a=None), "null pointer"), (dict(c=None), "null pointer"), (dict(cin=14), "multiples of 4"), (dict(ks=5), "kernel size"),
    (dict(ks=2), "kernel size"), (dict(stride=3), "stride"), (dict(stride=0), "stride"), (dict(c_off=4), "overruns"),
    (dict(a_off=4), "a_off"), (dict(act=7), "activation"), (dict(act=3), "box decode"), (dict(c_img_rows=8), "rows"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_argument_errors_return_a_status_with_text_and_launch_nothing(hip, over, text):
    lib = hip_lib.load()
    rc, msg, out, _keep = _raw_call(lib, **over)
    assert rc < 0 and text in msg, (rc, msg)
    assert torch.isnan(out).all(), "an argument error must not launch"
    rc, _, out, _keep = _raw_call(lib)
    assert rc == 0 and torch.isfinite(out).all()
    buf = torch.zeros(1, 4, 4, 16, device=DEV)
    assert lib.gdrnpp_spp_maxpool_5_9_13(buf.data_ptr(), 16, 4, 4, 1, 4, 4, None) < 0 and b"overrun" in lib.gdrnpp_last_error()
    assert lib.gdrnpp_yolox_focus(buf.data_ptr(), buf.data_ptr(), 16, 8, 1, 3, 4, None) < 0
    assert lib.gdrnpp_upsample_nearest2x_slice(buf.data_ptr(), 16, 0, buf.data_ptr(), 16, 2, 1, 2, 2, 4, None) < 0
