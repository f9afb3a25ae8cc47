"""Reference-anchored and independent checks of the oracles whose third-party arithmetic (cv2, detectron2, torchvision) is
not installed here — SURVEY.md §8 rows a1, a1b, f3.  They do not make those oracles bit-pinned (only the third-party
libraries themselves could); they pin what CAN be pinned: the reference's own matrix construction, the sampling geometry
against independent implementations, and closed-form answers."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import postproc as P


def test_affine_matrix_matches_reference_get_affine_transform(golden_dir):
    """oracle get_affine_transform == the reference's get_affine_transform / get_dir / get_3rd_point executed from source
    (tests/golden/make_golden_crop.py; cv2.getAffineTransform served by a float64 LU solve of OpenCV's 6x6 system)."""
    g = np.load(os.path.join(golden_dir, "crop_golden.npz"))
    for res, key in ((256, "M256"), (64, "M64")):
        for i in range(len(g["scales"])):
            M = P.get_affine_transform(g["centers"][i], float(g["scales"][i]), res)
            np.testing.assert_allclose(M, g[key][i], rtol=0, atol=1e-9)
    # the three warpAffine calls of read_data_test: same matrix for image and depth at 256, its own matrix at 64, dsize (w, h)
    np.testing.assert_allclose(g["call_M"][0], g["M256"][5], atol=0)
    np.testing.assert_allclose(g["call_M"][1], g["M256"][5], atol=0)
    np.testing.assert_allclose(g["call_M"][2], g["M64"][5], atol=0)
    assert g["call_flags"].tolist() == [1, 0, 1]   # INTER_LINEAR, INTER_NEAREST, INTER_LINEAR


def _grid_sample_affine(img_chw, M, out, mode):
    """dst(x, y) = src(M^-1 [x, y, 1]) with pixel centres at integer coordinates, zero border — ATen's grid_sample."""
    A = np.vstack([M, [0, 0, 1]])
    Ai = np.linalg.inv(A)
    ys, xs = np.mgrid[0:out, 0:out].astype(np.float64)
    sx = Ai[0, 0] * xs + Ai[0, 1] * ys + Ai[0, 2]
    sy = Ai[1, 0] * xs + Ai[1, 1] * ys + Ai[1, 2]
    h, w = img_chw.shape[1:]
    grid = np.stack([2 * sx / (w - 1) - 1, 2 * sy / (h - 1) - 1], -1)[None]
    t = torch.from_numpy(np.ascontiguousarray(img_chw, np.float64))[None]
    o = F.grid_sample(t, torch.from_numpy(grid), mode=mode, padding_mode="zeros", align_corners=True)
    return o[0].numpy(), sx, sy


def _smooth_image(rng, h, w, c, amp):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127.5 + amp * np.sin(xx / (9.0 + k) + rng.uniform(0, 6)) * np.cos(yy / (7.0 + 2 * k) + rng.uniform(0, 6))
                    for k in range(c)], -1)
    return img


@pytest.mark.parametrize("center,scale", [((300.0, 220.0), 180.0), ((90.5, 400.25), 97.3), ((600.0, 40.0), 250.0),
                                          ((320.0, 240.0), 640.0)])
def test_warp_u8_bilinear_against_float_bilinear(center, scale):
    """The 8-bit path of the cv2.warpAffine restatement (coordinates in 1/32 px, 15-bit weights) against an exact float
    bilinear of the same source pixels (F.grid_sample): they may differ only by the coordinate quantisation (<= 1/32 px per
    axis times the image gradient) plus the final rounding.  A half-pixel convention error would be 16x larger."""
    rng = np.random.default_rng(3)
    img = np.clip(np.rint(_smooth_image(rng, 480, 640, 3, 110.0)), 0, 255).astype(np.uint8)
    M = P.get_affine_transform(center, scale, 256)
    got = P.warp_affine(img, M, 256).astype(np.float64).transpose(2, 0, 1)
    want, sx, sy = _grid_sample_affine(img.astype(np.float64).transpose(2, 0, 1), M, 256, "bilinear")
    inside = (sx >= 0) & (sx <= 639) & (sy >= 0) & (sy <= 479)
    gy, gx = np.gradient(img.astype(np.float64), axis=(0, 1))
    gmax = max(np.abs(gx).max(), np.abs(gy).max())             # levels per source pixel
    tol = 0.5 + 2 * gmax / 32.0 + 0.05
    err = np.abs(got - want)[:, inside]
    assert err.max() <= tol, (err.max(), tol)
    assert err.mean() < 0.45                                     # ~ the rounding error of an exact bilinear
    # a half-pixel shift of the sampling grid would NOT pass
    shifted, _, _ = _grid_sample_affine(img.astype(np.float64).transpose(2, 0, 1), M + np.array([[0, 0, 0.5 * M[0, 0]], [0, 0, 0]]),
                                        256, "bilinear")
    assert np.abs(got - shifted)[:, inside].mean() > 2 * err.mean()
    # outside the source image the border value is 0 (pixels whose four neighbours all lie outside)
    far = (sx < -1) | (sx > 640) | (sy < -1) | (sy > 480)
    assert not got[:, far].any()


def test_warp_float_bilinear_and_nearest_against_grid_sample():
    """Float path (roi_coord_2d: 2-channel ramp, INTER_LINEAR) and depth path (INTER_NEAREST) against grid_sample."""
    rng = np.random.default_rng(4)
    c2d = P.get_2d_coord_np(640, 480)
    M64 = P.get_affine_transform((311.3, 207.9), 143.7, 64)
    got = P.warp_affine(c2d, M64, 64).transpose(2, 0, 1).astype(np.float64)
    want, sx, sy = _grid_sample_affine(c2d.transpose(2, 0, 1), M64, 64, "bilinear")
    # ramp slope 1/640 (1/480) per source pixel, coordinate quantisation 1/32 px
    assert np.abs(got[0] - want[0]).max() <= 1.0 / 640 / 32 + 1e-6
    assert np.abs(got[1] - want[1]).max() <= 1.0 / 480 / 32 + 1e-6
    dep = rng.uniform(0.3, 2.0, (480, 640)).astype(np.float32)
    M = P.get_affine_transform((311.3, 207.9), 143.7, 256)
    gotn = P.warp_affine(dep, M, 256, nearest=True)
    wantn, sx, sy = _grid_sample_affine(dep[None].astype(np.float64), M, 256, "nearest")
    frac = np.minimum(np.abs(sx - np.floor(sx) - 0.5), np.abs(sy - np.floor(sy) - 0.5))
    clear = frac > 1.0 / 1024 + 1e-9     # away from rounding ties: cv2 rounds the 10-bit fixed-point coordinate
    assert np.array_equal(gotn[clear], wantn[0][clear].astype(np.float32))
    assert clear.mean() > 0.99


EPS32 = float(np.finfo(np.float32).eps)
# Rounding steps (each <= eps32 / 2 relative to a magnitude <= 2 M, M = the largest |coordinate| the box reaches) on the way to
# one fp32 sample coordinate  start + p * bin + (i + .5) * bin / g  of oracle/roi_align_oracle.c:
#   start = r * scale - offset                      2        (end likewise 2; their difference +1 on a value <= 2 M: 6 in all)
#   bin = size / P                                  6 + 1    (relative to M / P)
#   p * bin                                         7 + 1
#   (i + .5) * bin / g                              7 + 1 + 1
#   the two additions                               2 + 2
# = 2 + 8 + 9 + 4 = 23 half-eps steps -> |coordinate error| <= 12 eps32 M per axis.  A bilinear surface is continuous and piecewise
# linear along each axis with slope <= D = max |neighbour difference|, so the two axes move a sample by <= 2 * 12 eps32 M D, and
# the mean over the bin's samples by no more.
K_COORD = 24
# Value arithmetic per sample: hy = 1 - ly (1 step), w = hy * hx (1), w * v (1), three additions (3), the accumulation's own
# addition (counted below): <= 7 half-eps steps on sum(w |v|) <= max |x|  ->  3.5 eps32; adding n = gh * gw samples left to right
# rounds n partial sums of magnitude <= n max |x|, divided by n at the end (+1): (n + 1) / 2 eps32.
def _k_value(n):
    return 3.5 + (n + 1) / 2.0


def _roi_align_independent(x, rois, out, sampling_ratio=0, aligned=True, spatial_scale=1.0):
    """ROIAlign written from its definition in fp64, separably: every bin is the mean of a regular gh x gw grid of bilinear
    samples; a sample row (column) outside [-1, H] ([-1, W]) contributes 0, coordinates are clamped to the image; rows are
    interpolated first, then columns — all sample rows and columns of a box at once.  ``rois`` are taken as the fp32 values
    the forward is given.  -> (f64[n, C, oh, ow], M = largest |coordinate| reached, near = bool[n, oh, ow]: a sample of that
    bin lies within the fp32 coordinate error of the validity window's edge, where the two may legitimately disagree)."""
    oh, ow = (out, out) if isinstance(out, int) else out
    b, c, h, w = x.shape
    xd = x.astype(np.float64)
    off = 0.5 if aligned else 0.0
    res, near, M = [], [], 0.0

    def axis(start, size, p, g, n):
        """sample coordinates [p * g] of one axis -> validity, low / high index, weight of high"""
        bin_ = size / p
        v = start + (np.arange(p)[:, None] + (np.arange(g)[None, :] + 0.5) / g) * bin_ if g > 0 else np.zeros((p, 0))
        v = v.reshape(-1)
        valid = (v >= -1) & (v <= n)
        vc = np.clip(v, 0, n - 1)
        lo = np.minimum(np.floor(vc).astype(int), n - 1)
        hi = np.minimum(lo + 1, n - 1)
        return v, valid, lo, hi, vc - lo

    for r in rois:
        bi = int(r[0])
        x1, y1, x2, y2 = [float(v) * spatial_scale - off for v in r[1:]]
        rw, rh = x2 - x1, y2 - y1
        if not aligned:
            rw, rh = max(rw, 1.0), max(rh, 1.0)
        gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rh / oh))
        gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rw / ow))
        if gh <= 0 or gw <= 0:                                 # no samples: the mean over max(gh * gw, 1) of nothing
            res.append(np.zeros((c, oh, ow)))
            near.append(np.zeros((oh, ow), bool))
            continue
        m = max(abs(x1), abs(x2), abs(y1), abs(y2), abs(x1 + rw), abs(y1 + rh), rw, rh, 1.0)
        M = max(M, m)
        ys, vy, ylo, yhi, ly = axis(y1, rh, oh, gh, h)
        xs, vx, xlo, xhi, lx = axis(x1, rw, ow, gw, w)
        img = xd[bi]
        rows = (img[:, ylo, :] * (1 - ly)[None, :, None] + img[:, yhi, :] * ly[None, :, None]) * vy[None, :, None]
        smp = (rows[:, :, xlo] * (1 - lx)[None, None, :] + rows[:, :, xhi] * lx[None, None, :]) * vx[None, None, :]
        res.append(smp.reshape(c, oh, gh, ow, gw).sum((2, 4)) / (gh * gw))
        d = K_COORD / 2 * EPS32 * m
        ny = ((np.abs(ys + 1) <= d) | (np.abs(ys - h) <= d)).reshape(oh, gh).any(1)
        nx = ((np.abs(xs + 1) <= d) | (np.abs(xs - w) <= d)).reshape(ow, gw).any(1)
        near.append(ny[:, None] | nx[None, :])
    return np.stack(res), M, np.stack(near)


def _neighbour_difference(x):
    d = [np.abs(np.diff(x.astype(np.float64), axis=a)).max() for a in (2, 3) if x.shape[a] > 1]
    return max(d) if d else 0.0


def _roi_align_bound(x, M, n_samples):
    """k eps32 max|coordinate| max|neighbour difference| + k' eps32 max|x| (derivation above K_COORD / _k_value)."""
    return K_COORD * EPS32 * M * _neighbour_difference(x) + _k_value(n_samples) * EPS32 * float(np.abs(x).max())


def test_roi_align_oracle_against_independent_formulation():
    """oracle/roi_align_oracle.c (detectron2 ROIAlign restated) against the definition written with array ops in fp64, on
    boxes inside, across and beyond the image border, adaptive and fixed sampling ratios."""
    rng = np.random.default_rng(5)
    x = rng.normal(size=(2, 3, 37, 45)).astype(np.float32)
    rois = np.array([[0, 5.3, 4.1, 30.7, 28.9], [1, 10.0, 8.0, 26.0, 24.0], [0, -6.0, -3.5, 12.2, 9.9],
                     [1, 30.0, 20.0, 60.0, 50.0], [0, 0.0, 0.0, 45.0, 37.0], [1, 7.25, 3.5, 9.0, 5.0]], np.float32)
    for sr in (0, 2):
        got = P.roi_align(x, rois, 8, 1.0, sr, True)
        want, _, near = _roi_align_independent(x, rois, 8, sr)
        assert not near.any()
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)


def test_roi_case_list_covers_every_launch_axis():
    """tests/roi_cases.py: every value of every axis the launcher and kernel branch on appears, each partial-wave pooled_w with
    a gh below (where one exists) and at its threshold 4 * gh > active lanes, and the boxes give the gh / gw the case names."""
    from tests import roi_cases as RC

    cs = RC.ALIGN_CASES
    assert len({c.id for c in cs}) == len(cs)
    assert {c.pw for c in cs} >= {1, 7, 16, 63, 64, 65, 100, 128, 130, 200, 256}
    assert {c.ph for c in cs} >= {1, 5, 16, 33}
    assert {c.gh for c in cs} >= {1, 2, 3, 5, 9, 10, 16, 17, 20} and {c.gw for c in cs} >= {1, 2, 3, 4, 5, 9}
    assert {c.c for c in cs} >= {1, 2, 3, 4, 5, 8} and {c.w for c in cs} >= {1, 2, 3, 80} and {c.h for c in cs} >= {1, 2, 60}
    assert {c.aligned for c in cs} == {True, False} and {c.sampling_ratio for c in cs} >= {0, 2, 3}
    assert {c.scale for c in cs} >= {1.0, 0.25}
    pairs = {(c.pw, c.gh) for c in cs if c.w > 1 and c.sampling_ratio == 0}
    assert pairs >= {(7, 1), (7, 2), (16, 3), (16, 5), (100, 9), (100, 10), (130, 1), (200, 2), (200, 3)}
    assert pairs >= {(7, 5), (16, 9), (16, 16), (100, 16), (130, 3), (200, 9), (16, 17), (16, 20)}
    n = [c.gh * c.gw for c in cs]
    assert any(v & (v - 1) == 0 for v in n) and any(v & (v - 1) for v in n)              # reciprocal multiply and division
    # a thread's 4 rows end inside pooled_h: 4 * (256 / cols) rows per workgroup, pooled_h not a multiple of 4
    assert {(c.ph % 4 != 0, 64 if c.pw <= 64 else 128 if c.pw <= 128 else 256) for c in cs} >= {(True, 64), (True, 128), (True, 256)}
    for c in cs + RC.CONTAINMENT_CASES:
        gh, gw = RC.align_grid(c, RC.align_rois(c))
        assert (gh == c.gh).all() and (gw == c.gw).all(), c.id
    assert all(c in cs for c in RC.CONTAINMENT_CASES) and {c.pw for c in RC.CONTAINMENT_CASES} == {7, 100, 130}


def test_roi_align_oracle_against_fp64_over_the_gpu_case_list(capsys):
    """The cases tests/test_gpu_roi_shapes.py holds the kernel to (bit for bit against the oracle), here the oracle against the
    fp64 formulation: outputs (oh, ow) from 1 x 1 to 33 x 256, aligned or not, spatial_scale, fixed and adaptive grids up to
    20 x 3 samples, sources down to 1 x 1.  Bound per case = 24 eps32 max|coordinate| max|neighbour difference|
    + (3.5 + (gh gw + 1) / 2) eps32 max|x|, from the operation count of the fp32 restatement (see K_COORD), not from the observed
    error.  Bins with a sample within the coordinate error of the validity window's edge are left out (fp32 and fp64 may
    disagree there by a whole sample); there are none in this list.  Largest observed / bound over the list: 0.018
    (observed errors up to 9.8e-5 where coordinates reach 400; printed per case with -s)."""
    from tests import roi_cases as RC

    worst = 0.0
    lines = []
    for case in RC.ALIGN_CASES + [RC.DEGENERATE_CASE]:
        x = RC.align_input(case)
        rois = RC.DEGENERATE_ROIS if case is RC.DEGENERATE_CASE else RC.align_rois(case)
        got = P.roi_align(x, rois, (case.ph, case.pw), case.scale, case.sampling_ratio, case.aligned)
        want, M, near = _roi_align_independent(x, rois, (case.ph, case.pw), case.sampling_ratio, case.aligned, case.scale)
        assert not near.any(), case.id
        err = float((np.abs(got - want) * ~near[:, None]).max())
        bound = _roi_align_bound(x, M, max(case.gh * case.gw, 1))
        lines.append(f"{case.id}: observed {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
        assert err <= bound, lines[-1]
        worst = max(worst, err / bound)
    with capsys.disabled():
        print("\n" + "\n".join(lines) + f"\nroi_align oracle vs fp64: largest observed / bound = {worst:.3g}")
    assert worst > 1e-4                                      # the bound is not vacuous: rounding error is seen


def test_roi_align_oracle_linear_ramp_closed_form():
    """On x[c, y, x] = a x + b y + d bilinear interpolation is exact, so with every sample inside [0, W - 1] x [0, H - 1] each
    output is the ramp at its bin centre.  a, b, d, the box corners and the bin sizes are small dyadic rationals and gh * gw is a
    power of two, so every fp32 operation is exact: the oracle meets EQUALITY (the GPU suite asks the same of the kernel)."""
    from tests import roi_cases as RC

    x = RC.ramp_input()
    for case in RC.RAMP_CASES:
        rois, want = RC.ramp_rois_and_expected(case)
        got = P.roi_align(x, rois, (case.ph, case.pw), case.scale)
        assert np.array_equal(got.astype(np.float64), want), case.id
        ind, _, _ = _roi_align_independent(x, rois, (case.ph, case.pw), 0, True, case.scale)
        assert np.array_equal(ind, want), case.id


def _preds(boxes, scores, classes, num_classes):
    """YOLOX head rows (cx, cy, w, h, obj, class scores) for given corner boxes."""
    a = len(boxes)
    p = np.zeros((1, a, 5 + num_classes), np.float32)
    b = np.asarray(boxes, np.float32)
    p[0, :, 0] = (b[:, 0] + b[:, 2]) / 2
    p[0, :, 1] = (b[:, 1] + b[:, 3]) / 2
    p[0, :, 2] = b[:, 2] - b[:, 0]
    p[0, :, 3] = b[:, 3] - b[:, 1]
    p[0, :, 4] = 1.0
    for i, (s, c) in enumerate(zip(scores, classes)):
        p[0, i, 5 + c] = s
    return p


def test_nms_oracle_closed_form_cases():
    """torchvision.ops.nms semantics restated in oracle/nms_oracle.c, on cases whose answer follows from the definition:
    IoU([0,0,10,10],[1,1,11,11]) = 81/119 > 0.45 suppresses the lower score; IoU exactly 0.5 at threshold 0.5 does NOT
    suppress (the test is iou > thr); boxes of different classes never suppress each other (batched_nms) unless
    class_agnostic; ties keep the earlier box; the output is ordered by descending score."""
    boxes = [[0, 0, 10, 10], [1, 1, 11, 11], [20, 20, 30, 30], [0, 0, 10, 10]]
    out = P.yolox_postprocess(_preds(boxes, [0.9, 0.8, 0.95, 0.85], [0, 0, 0, 1], 2), 2, 0.1, 0.45)[0]
    assert out.shape == (3, 7)
    np.testing.assert_allclose(out[:, :4], [[20, 20, 30, 30], [0, 0, 10, 10], [0, 0, 10, 10]], atol=1e-5)
    assert out[:, 6].tolist() == [0.0, 0.0, 1.0]
    np.testing.assert_allclose(out[:, 5], [0.95, 0.9, 0.85], atol=1e-6)
    out = P.yolox_postprocess(_preds(boxes, [0.9, 0.8, 0.95, 0.85], [0, 0, 0, 1], 2), 2, 0.1, 0.45, class_agnostic=True)[0]
    assert out.shape == (2, 7) and out[:, 5].tolist() == pytest.approx([0.95, 0.9])
    # IoU == threshold: A = [0,0,2,1] (area 2), B = [0,0,1,1] inside A: inter 1, union 2 -> 0.5
    out = P.yolox_postprocess(_preds([[0, 0, 2, 1], [0, 0, 1, 1]], [0.9, 0.8], [0, 0], 1), 1, 0.1, 0.5)[0]
    assert out.shape[0] == 2
    out = P.yolox_postprocess(_preds([[0, 0, 2, 1], [0, 0, 1, 1]], [0.9, 0.8], [0, 0], 1), 1, 0.1, 0.4999)[0]
    assert out.shape[0] == 1
    # chain A-B-C: B is suppressed by A, so C (overlapping only B) survives
    out = P.yolox_postprocess(_preds([[0, 0, 10, 10], [4, 0, 14, 10], [8, 0, 18, 10]], [0.9, 0.8, 0.7], [0, 0, 0], 1), 1, 0.1, 0.4)[0]
    np.testing.assert_allclose(out[:, 0], [0, 8], atol=1e-5)
    # score threshold: obj * class_conf >= conf_thre
    assert P.yolox_postprocess(_preds([[0, 0, 10, 10]], [0.5], [0], 1), 1, 0.7, 0.45)[0] is None


def _roi_pool_independent(x, rois, size, spatial_scale=1.0):
    """RoIPool from its published definition in NumPy: corners rounded half away from zero, width / height = max(end - start
    + 1, 1), bin [floor(p * bin), ceil((p + 1) * bin)) in fp32, shifted by the start and clipped to the image; max, 0 if empty."""
    import math

    oh, ow = size
    c, h, w = x.shape[1:]
    f = np.float32

    def rnd(v):                                    # std::round: half away from zero
        v = float(f(v) * f(spatial_scale))
        return int(math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1))

    out = np.zeros((len(rois), c, oh, ow), np.float32)
    for n, r in enumerate(rois):
        sw, sh, ew, eh = rnd(r[1]), rnd(r[2]), rnd(r[3]), rnd(r[4])
        rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
        bh, bw = f(rh) / f(oh), f(rw) / f(ow)
        img = x[int(r[0])]
        for ph in range(oh):
            h0 = min(max(int(np.floor(f(ph) * bh)) + sh, 0), h)
            h1 = min(max(int(np.ceil(f(ph + 1) * bh)) + sh, 0), h)
            for pw in range(ow):
                w0 = min(max(int(np.floor(f(pw) * bw)) + sw, 0), w)
                w1 = min(max(int(np.ceil(f(pw + 1) * bw)) + sw, 0), w)
                if h1 > h0 and w1 > w0:
                    out[n, :, ph, pw] = img[:, h0:h1, w0:w1].reshape(c, -1).max(1)
    return out


def test_roi_pool_oracle_against_an_independent_formulation_and_closed_forms():
    """RoIPool (batch_crop_resize(interpolation="nearest"), core/utils/zoom_utils.py:92-93): torchvision is absent, so the
    restatement (oracle/roi_align_oracle.c, parity unpinned) is held against an independent NumPy formulation of the published
    definition and against closed forms: a pixel-aligned box with one pixel per bin returns the pixels themselves; a box outside
    the image returns zeros; with the box equal to the image and an evenly dividing output it equals max pooling."""
    import math

    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(12)
    x = rng.standard_normal((2, 3, 17, 23)).astype(np.float32)
    rois = np.array([[0, 2, 3, 9, 10], [1, -4.4, -2.6, 6.5, 7.49], [0, 30, 30, 40, 40], [1, 0.49, 0.51, 21.7, 15.2],
                     [0, 5, 5, 5, 5], [1, 10.5, 2.5, 3.5, 1.5]], np.float32)
    out = P.roi_pool(x, rois, (4, 5))

    assert np.array_equal(out, _roi_pool_independent(x, rois, (4, 5)))
    assert not out[2].any()                                                        # box outside the image
    px = P.roi_pool(x, np.array([[0, 4, 6, 8, 9]], np.float32), (4, 5))            # 5 x 4 pixels, one per bin
    assert np.array_equal(px[0], x[0, :, 6:10, 4:9])
    whole = P.roi_pool(x[:, :, :16, :20], np.array([[1, 0, 0, 19, 15]], np.float32), (4, 5))
    assert np.array_equal(whole[0], F.max_pool2d(torch.from_numpy(x[1:2, :, :16, :20]), 4)[0].numpy())


def test_roi_pool_oracle_against_the_independent_formulation_over_the_gpu_shapes():
    """The outputs, sources and boxes of tests/test_gpu_roi_shapes.py (1 x 1 .. 33 x 65 outputs, C = 1 / 4 / 5, sources one pixel
    wide or high, boxes across every border, .5 corners of both signs, spatial_scale 0.25): oracle == NumPy formulation."""
    from tests import roi_cases as RC

    for k, (c, h, w) in enumerate(RC.POOL_SOURCES):
        x = RC.pool_input(c, h, w)
        for j, size in enumerate(RC.POOL_OUTPUTS):
            for scale in (1.0, 0.25) if (k + j) % 2 == 0 else (1.0,):
                rois = RC.pool_rois(h, w, scale)
                got = P.roi_pool(x, rois, size, scale)
                assert np.array_equal(got, _roi_pool_independent(x, rois, size, scale)), (c, h, w, size, scale)
                assert got[5].any() and not got[6].any() and not got[7].any()


def test_nms_oracle_equals_the_reference_postprocess_executed_from_source(golden_dir):
    """yolox_golden.npz = the reference's ``postprocess`` (det/yolox/utils/boxes.py:34-74) run from its source text with only the
    torchvision NMS primitive served by a stand-in (tests/golden/make_golden_yolox.py): the oracle reproduces counts, rows and keep
    order bit for bit — corner conversion, class argmax, the obj * class >= thr mask, the 7-column layout and the None of an empty
    image are therefore the reference's own; what stays a restatement is the NMS primitive."""
    z = np.load(os.path.join(golden_dir, "yolox_golden.npz"))
    total = 0
    for name in "abcd":
        c, conf, thr, agn = z[name + "_args"]
        outs = P.yolox_postprocess(z[name + "_det"], int(c), float(conf), float(thr), bool(agn))
        assert [0 if o is None else len(o) for o in outs] == z[name + "_count"].tolist(), name
        cat = np.concatenate([np.zeros((0, 7), np.float32)] + [o for o in outs if o is not None])
        assert np.array_equal(cat, z[name + "_out"]), name
        total += len(cat)
    assert total > 400 and z["d_count"].sum() == 0


def _readdata_case(golden_dir):
    import sys
    sys.path.insert(0, golden_dir)
    z = np.load(os.path.join(golden_dir, "readdata_golden.npz"))
    rng = np.random.default_rng(20220925 + 71)                 # tests/golden/make_golden_readdata.case()
    image = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    depth = (rng.integers(300, 2000, (480, 640)).astype(np.uint16) / 1000.0).astype(np.float32)
    return z, image, depth


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_roi_plumbing_equals_the_reference_read_data_test(golden_dir):
    """readdata_golden.npz = the reference's own ``read_data_test`` (data_loader.py:647-818) executed from source on one seeded image
    with six detections (tests/golden/make_golden_readdata.py).  engine.rois_from_detections reproduces its per-ROI scalars exactly —
    XYWH -> XYXY, centre, scale = min(max(w, h) * 1.5, 640), roi_wh clamped to >= 1, resize_ratio — and the oracle's crop chain
    (fed those scalars) reproduces every crop BYTE FOR BYTE (SHA-256), i.e. which array is warped with which interpolation to which
    size, the fp64 normalisation and the float32 casts are the reference's."""
    from gdrnpp_bop2022_amd.gdrn_modeling import engine

    z, image, depth = _readdata_case(golden_dir)
    b = z["boxes_xywh"]
    xyxy = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1)
    r = engine.rois_from_detections(xyxy, 480, 640, 1.5, 64)
    assert np.array_equal(r["bbox_center"].astype(np.float32), z["abs_bbox_center"]) and np.array_equal(r["scale"], z["abs_scale"])
    assert np.array_equal(r["roi_wh"], z["abs_roi_wh"]) and np.array_equal(r["resize_ratio"], z["abs_resize_ratio"])
    assert z["abs_scale"].tolist()[2] == 640.0 and z["abs_roi_wh"][3, 0] == 1.0            # the clamps are exercised
    assert str(z["abs_scale_dtype"]) == "float64" and str(z["abs_bbox_center_dtype"]) == "float32" and str(z["abs_roi_cls_dtype"]) == "int64"
    for i in range(len(b)):
        img, dep, c2d = P.crop_resize_roi(image, depth, r["bbox_center"][i], float(r["scale"][i]))
        assert _sha(img) == str(z["abs_roi_img_sha256"][i]) and _sha(dep) == str(z["abs_roi_depth_sha256"][i]), i
        assert _sha(c2d) == str(z["abs_roi_coord_2d_sha256"][i]), i
        rel = ((r["bbox_center"][i].reshape(2, 1, 1) - c2d * np.array([640, 480]).reshape(2, 1, 1)) / r["scale"][i]).astype(np.float32)
        assert _sha(rel) == str(z["rel_roi_coord_2d_rel_sha256"][i]), i
