"""tests/pnp_bwd_ref.py's four formulas (the stride-2 weight gradient, the parity-form data gradient, the NCHW flatten, the pose heads'
backward) against fp64 autograd of F.conv2d(stride=2, padding=1), flatten and nn.Linear: equal on integer lattices, within 1e-12
relative on random fp64 data.  The GPU tests hold the HIP kernels to the same autograd runs; these hold the restatement the GPU
tests' exact cases lean on, without a device."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_bwd_ref as R  # noqa: E402

SMALL = tuple(c for c in R.CASES if c[0] * c[1] * c[2] <= 2 * 8 * 16) + ((2, 2, 2, 5, 8, 3), (1, 6, 10, 7, 8, 4))


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("case", SMALL, ids=R.case_id)
def test_conv_formulas_equal_autograd_on_integers(case):
    n, h, w, cin, _, cout = case
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-8, 9, (n, cin, h, w), generator=gen).double()
    weight = torch.randint(-8, 9, (cout, cin, 3, 3), generator=gen).double()
    dz = torch.randint(-8, 9, (n, cout, h // 2, w // 2), generator=gen).double()
    ref = R.autograd_conv(x, weight, dz, torch.float64)
    assert torch.equal(R.wgrad_s2(dz, x), ref["dW"])
    assert torch.equal(R.dinput_s2(dz, weight), ref["dx"])


@pytest.mark.parametrize("case", SMALL, ids=R.case_id)
def test_conv_formulas_meet_autograd_on_random_fp64(case):
    n, h, w, cin, _, cout = case
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(n, cin, h, w, generator=gen, dtype=torch.float64)
    weight = torch.randn(cout, cin, 3, 3, generator=gen, dtype=torch.float64)
    dz = torch.randn(n, cout, h // 2, w // 2, generator=gen, dtype=torch.float64)
    ref = R.autograd_conv(x, weight, dz, torch.float64)
    assert _rel(R.wgrad_s2(dz, x), ref["dW"]) <= 1e-12
    assert _rel(R.dinput_s2(dz, weight), ref["dx"]) <= 1e-12


@pytest.mark.parametrize("hw", ((2, 2), (4, 4), (8, 16), (6, 10)))
def test_parity_table(hw):
    h, w = hw
    cnt, top_y, top_x = R.tap_table(h, w)
    # taps per parity class: 1 / 2 / 2 / 4, but for the last odd row and column, which output row OH / column OW would reach
    for y in range(h):
        for x in range(w):
            ty = [(k, s) for k, s in R.parity_taps(y % 2) if y // 2 + s < h // 2]
            tx = [(k, s) for k, s in R.parity_taps(x % 2) if x // 2 + s < w // 2]
            assert int(cnt[y, x]) == len(ty) * len(tx), (y, x)
    inner = cnt[:h - 1, :w - 1]
    assert sorted({int(v) for v in inner[0::2, 0::2].flatten()}) == [1]
    if w > 2:
        assert sorted({int(v) for v in inner[0::2, 1::2].flatten()}) == [2]
    if h > 2:
        assert sorted({int(v) for v in inner[1::2, 0::2].flatten()}) == [2]
    if h > 2 and w > 2:
        assert sorted({int(v) for v in inner[1::2, 1::2].flatten()}) == [4]
    assert len(R.parity_taps(0)) == 1 and len(R.parity_taps(1)) == 2
    # per 2 x 2 block: 9 taps
    assert sum(len(R.parity_taps(py)) * len(R.parity_taps(px)) for py in range(2) for px in range(2)) == 9
    # the last (odd) row and column are reached from output row OH - 1 / column OW - 1 at most: nothing comes from oy = OH
    assert top_y[h - 1] == h // 2 - 1 and top_x[w - 1] == w // 2 - 1 and max(top_y) == h // 2 - 1 and max(top_x) == w // 2 - 1
    assert int(cnt[h - 1, w - 1]) == 1 and int(cnt[h - 1, 0]) == 1 and int(cnt[0, w - 1]) == 1
    # the parity form says so itself: the tap (k = 0, shift 1) of the last odd index points at OH
    assert [(k, s) for k, s in R.parity_taps(1) if (h - 1) // 2 + s >= h // 2] == [(0, 1)]


def test_nan_in_dz_spreads_as_in_autograd():
    case = (1, 8, 8, 5, 8, 4)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(1, 5, 8, 8, generator=gen, dtype=torch.float64)
    weight = torch.randn(4, 5, 3, 3, generator=gen, dtype=torch.float64)
    dz = torch.randn(1, 4, 4, 4, generator=gen, dtype=torch.float64)
    dz[0, 2, 1, 2] = float("nan")      # an interior output pixel: all nine taps lie inside the image
    ref = R.autograd_conv(x, weight, dz, torch.float64)
    assert torch.equal(torch.isnan(R.wgrad_s2(dz, x)), torch.isnan(ref["dW"])), case
    assert torch.equal(torch.isnan(R.dinput_s2(dz, weight)), torch.isnan(ref["dx"]))
    assert int(torch.isnan(ref["dx"]).sum()) == 9 * 5 and int(torch.isnan(ref["dW"]).sum()) == 5 * 9


def test_flatten_is_the_nchw_flatten():
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(3, 7, 4, 5, generator=gen, dtype=torch.float64)      # NCHW
    nhwc = x.permute(0, 2, 3, 1).reshape(3, 20, 7)
    flat = R.flatten_nchw(nhwc)
    assert torch.equal(flat, x.flatten(1))
    assert torch.equal(R.unflatten_nchw(flat, 20, 7), nhwc)
    # the inverse is the gradient: autograd of flatten hands back the NCHW gradient
    leaf = x.clone().requires_grad_(True)
    g = torch.randn(3, 140, generator=gen, dtype=torch.float64)
    (dx,) = torch.autograd.grad(leaf.flatten(1), leaf, g)
    assert torch.equal(R.unflatten_nchw(g, 20, 7), dx.permute(0, 2, 3, 1).reshape(3, 20, 7))


@pytest.mark.parametrize("b", (1, 3, 8))
def test_heads_backward_equals_autograd(b):
    gen = torch.Generator().manual_seed(10 + b)
    k, rd = 256, 6
    for integers in (True, False):
        def rnd(*shape):
            if integers:
                return torch.randint(-8, 9, shape, generator=gen).double()
            return torch.randn(*shape, generator=gen, dtype=torch.float64)

        feat, w_r, b_r, w_t, b_t, g_r, g_t = rnd(b, k), rnd(rd, k), rnd(rd), rnd(3, k), rnd(3), rnd(b, rd), rnd(b, 3)
        want = R.autograd_heads(g_r, g_t, feat, w_r, b_r, w_t, b_t, torch.float64)
        got = R.heads_backward(g_r, g_t, feat, w_r, w_t)
        for a, r in zip(got, want):
            assert torch.equal(a, r) if integers else _rel(a, r) <= 1e-12
        # a head without a gradient: its terms are absent
        only_t = R.heads_backward(None, g_t, feat, w_r, w_t)
        assert torch.equal(only_t[0], g_t @ w_t) and not only_t[1].any() and not only_t[2].any() and torch.equal(only_t[3], got[3])


def test_lattices_and_probes_are_exact_by_construction():
    for case in R.CASES[:2]:
        x, weight, dz, dw64, dx64 = R.conv_lattice(case)
        ref = R.autograd_conv(x, weight, dz, torch.float64)
        assert torch.equal(dw64, ref["dW"]) and torch.equal(dx64, ref["dx"])
        assert float(dw64.abs().max()) < 2 ** 24 and float(dx64.abs().max()) < 2 ** 24
        n, h, w, cin, _, cout = case
        cx, cw = R.coded_x(case), R.coded_weight(case)
        for probe in R.probe_positions(case):
            b, oy, ox, co = probe
            dz1 = R.onehot_dz(case, probe)
            dw = R.wgrad_s2(dz1.double(), cx.double())
            dx = R.dinput_s2(dz1.double(), cw.double())
            for ky in range(3):
                for kx in range(3):
                    y, xx = 2 * oy + ky - 1, 2 * ox + kx - 1
                    inside = 0 <= y < h and 0 <= xx < w
                    assert torch.equal(dw[co, :, ky, kx], cx[b, :, y, xx].double() if inside else torch.zeros(cin, dtype=torch.float64))
                    if inside:
                        assert torch.equal(dx[b, :, y, xx], cw[co, :, ky, kx].double())
            assert int((dw != 0).any(1).any(1).any(1).sum()) == 1 and int((dx != 0).any(1).sum()) <= 9
