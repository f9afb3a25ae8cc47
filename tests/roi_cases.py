"""Case lists for the ROI kernels' launch shapes, shared by tests/test_gpu_roi_shapes.py (HIP kernel against the oracle, bit for
bit) and tests/test_crop_pins.py (the oracle against an independent fp64 formulation).  Plain helper module: no fixtures.

gdrnpp_roi_align picks its launch from the arguments: cols = 64 / 128 / 256 output columns per workgroup by pooled_w, 256 / cols
row lanes of 4 rows each, 1..4 channel planes per thread (full or partial last chunk), a register-cached instantiation for
gw = 1..4 sample columns per bin and a loop for more, the wave's y taps one per lane when 4 * gh <= 64 and per thread beyond, a
reciprocal multiply when gh * gw is a power of two, and a separate kernel when W == 1.  A wave covers 64 consecutive output
columns of one row lane; a partial wave has a = pooled_w - (its first column) active lanes and needs 4 * gh of its lanes to
compute taps, so each partial-wave pooled_w is paired with a gh on both sides of 4 * gh > a:

    pooled_w    7   16   100   130   200
    a           7   16    36     2     8
    gh from     2    5    10     1     3
"""
from dataclasses import dataclass

import numpy as np

BIG = (360, 400)      # source H, W large enough that a gh = 20 box at pooled_h = 16 (313.6 rows) mostly overlaps it


@dataclass(frozen=True)
class AlignCase:
    ph: int
    pw: int
    gh: int           # sample rows / columns per bin the boxes are built to give (sampling_ratio == 0)
    gw: int
    c: int
    h: int = BIG[0]
    w: int = BIG[1]
    aligned: bool = True
    sampling_ratio: int = 0
    scale: float = 1.0

    @property
    def id(self):
        s = f"out{self.ph}x{self.pw}-g{self.gh}x{self.gw}-c{self.c}-src{self.h}x{self.w}"
        if not self.aligned:
            s += "-unaligned"
        if self.sampling_ratio:
            s += f"-sr{self.sampling_ratio}"
        if self.scale != 1.0:
            s += f"-scale{self.scale}"
        return s


A = AlignCase
ALIGN_CASES = [
    # partial-wave pooled_w x gh below / at / above the row's threshold (module docstring)
    A(5, 7, 1, 1, 3), A(5, 7, 2, 2, 3), A(16, 7, 5, 9, 1), A(1, 7, 16, 3, 2),
    A(16, 16, 3, 3, 3), A(16, 16, 5, 2, 4), A(16, 16, 9, 1, 2), A(16, 16, 16, 4, 5),
    A(5, 100, 9, 2, 3), A(5, 100, 10, 3, 3), A(16, 100, 16, 1, 4),
    A(16, 130, 1, 1, 3), A(33, 130, 3, 2, 5), A(5, 130, 10, 1, 1),
    A(16, 200, 2, 1, 3), A(16, 200, 3, 2, 2), A(5, 200, 9, 1, 1),
    # 4 * gh > 64: the y taps are computed per thread
    A(16, 16, 17, 2, 3), A(16, 16, 20, 3, 8), A(1, 65, 17, 1, 3), A(5, 7, 20, 1, 4),
    # whole waves only (pooled_w % 64 == 0), pooled_w = 1, 63, 65
    A(16, 64, 2, 4, 3), A(33, 128, 2, 2, 4), A(33, 256, 3, 1, 3), A(1, 256, 5, 1, 2), A(5, 1, 2, 2, 3),
    A(16, 63, 2, 5, 3), A(33, 65, 1, 4, 3), A(5, 64, 9, 3, 5),
    # aligned = False, fixed sampling ratios, spatial_scale
    A(5, 7, 2, 2, 3, aligned=False), A(16, 16, 5, 2, 4, aligned=False), A(33, 130, 3, 2, 5, aligned=False),
    A(1, 1, 1, 1, 1, aligned=False),
    A(5, 7, 2, 2, 3, sampling_ratio=2), A(16, 16, 3, 3, 4, sampling_ratio=3), A(16, 100, 2, 2, 3, sampling_ratio=2),
    A(33, 200, 3, 3, 2, sampling_ratio=3), A(16, 16, 3, 3, 3, aligned=False, sampling_ratio=3),
    A(5, 7, 2, 2, 3, scale=0.25), A(16, 16, 5, 2, 4, scale=0.25), A(5, 100, 10, 3, 3, scale=0.25),
    A(16, 200, 3, 2, 2, scale=0.25, aligned=False),
    # small sources: W = 1 is the one-thread-per-element kernel, W = 2 the 8-byte row load at its edge, H = 1 / 2 the row clamp
    A(5, 7, 2, 1, 3, 60, 1), A(16, 16, 5, 1, 5, 60, 1, aligned=False), A(5, 7, 2, 2, 3, 60, 1, sampling_ratio=2),
    A(5, 7, 2, 2, 3, 60, 2), A(16, 16, 5, 2, 4, 2, 2), A(5, 100, 1, 1, 3, 60, 2), A(16, 16, 3, 3, 2, 1, 3, sampling_ratio=3),
    A(5, 7, 2, 2, 1, 1, 80), A(16, 130, 1, 1, 3, 2, 80), A(16, 16, 5, 3, 3, 60, 80), A(33, 65, 1, 1, 8, 60, 3),
    A(5, 7, 2, 2, 3, 1, 1), A(16, 16, 2, 2, 4, 2, 1, sampling_ratio=2),
]

# store containment (guard words around the output block): the partial-wave widths, each with 4 * gh above its active lanes
CONTAINMENT_CASES = [A(5, 7, 2, 2, 3), A(5, 100, 10, 3, 3), A(33, 130, 3, 2, 5), A(16, 130, 1, 1, 3)]


def align_rois(case):
    """Five boxes over both batch images, in the ROI coordinates the kernel is given (feature coordinates / spatial_scale): inside
    the image (centred on it where the box is larger), starting at negative coordinates, running past the far border, and entirely
    outside the sampling window — once along x and once along y, so that both axes' validity flags decide a result of zeros.
    Height pooled_h * (gh - 0.4) and width pooled_w * (gw - 0.4) make ceil(roi_h / pooled_h) == gh robustly in fp32."""
    bh, bw = case.ph * (case.gh - 0.4), case.pw * (case.gw - 0.4)
    h, w = case.h, case.w
    x_in = 3.3 if 3.3 + bw <= w - 1 else (w - bw) / 2 + 0.13
    y_in = 2.6 if 2.6 + bh <= h - 1 else (h - bh) / 2 + 0.07
    starts = [(0, x_in, y_in), (1, -0.3 * bw - 2.7, -0.3 * bh - 1.9), (0, w - 0.6 * bw, h - 0.6 * bh),
              (1, w + 2.5, y_in), (0, x_in, h + 1.75)]
    rois = np.array([[b, x, y, x + bw, y + bh] for b, x, y in starts], np.float64)
    rois[:, 1:] /= case.scale
    return rois.astype(np.float32)


def align_grid(case, rois):
    """(gh, gw) per box as the fp32 forward computes them."""
    f = np.float32
    off = f(0.5 if case.aligned else 0.0)
    sw, sh = rois[:, 1] * f(case.scale) - off, rois[:, 2] * f(case.scale) - off
    rw, rh = (rois[:, 3] * f(case.scale) - off) - sw, (rois[:, 4] * f(case.scale) - off) - sh
    if not case.aligned:
        rw, rh = np.maximum(rw, f(1)), np.maximum(rh, f(1))
    if case.sampling_ratio > 0:
        return np.full(len(rois), case.sampling_ratio), np.full(len(rois), case.sampling_ratio)
    return np.ceil(rh / f(case.ph)).astype(int), np.ceil(rw / f(case.pw)).astype(int)


def align_input(case, seed=0):
    """Unit-variance noise f32[2, C, H, W]: every pixel differs from its neighbours, so a wrong tap shows."""
    rng = np.random.default_rng([seed, case.ph, case.pw, case.gh, case.gw, case.c, case.h, case.w])
    return rng.standard_normal((2, case.c, case.h, case.w)).astype(np.float32)


# Inverted and zero-area boxes with aligned = True: gh <= 0 or gw <= 0, no samples, the mean over max(gh * gw, 1) of nothing = 0.
DEGENERATE_CASE = A(16, 100, 0, 0, 3, 60, 80)
DEGENERATE_ROIS = np.array([[0, 40.0, 30.0, 10.0, 5.0],        # inverted on both axes: gh * gw > 0 with gh, gw < 0
                            [1, 10.0, 30.0, 70.0, 5.0],        # inverted rows only
                            [0, 70.0, 5.0, 10.0, 50.0],        # inverted columns only
                            [1, 20.0, 20.0, 20.0, 20.0],       # zero area
                            [0, 10.0, 20.0, 60.0, 20.0]], np.float32)    # zero height


# ---- linear ramp: bilinear interpolation of x[c, y, x] = a x + b y + d is exact, so with every sample inside
# [0, W - 1] x [0, H - 1] each output is the ramp at its bin centre.  Slopes, offsets, box corners and bin sizes are small dyadic
# rationals and gh * gw is a power of two: every fp32 operation of the forward is then exact and the comparison is equality.
RAMP_ABD = np.array([[0.25, 0.5, 1.0], [-0.5, 0.25, 300.0], [1.0, -0.25, -7.5]])          # per channel: a, b, d
RAMP_IMAGE_OFFSET = (0.0, 16.0)                                                         # added to d per batch image


@dataclass(frozen=True)
class RampCase:
    ph: int
    pw: int
    bin_h: float      # = gh (1, 2, 4, ...) or 1.5 (gh = 2)
    bin_w: float
    scale: float = 1.0

    @property
    def id(self):
        return f"out{self.ph}x{self.pw}-bin{self.bin_h}x{self.bin_w}" + (f"-scale{self.scale}" if self.scale != 1.0 else "")


RAMP_CASES = [RampCase(5, 7, 1.5, 1.5), RampCase(16, 16, 8.0, 2.0), RampCase(16, 100, 16.0, 2.0), RampCase(1, 130, 1.0, 1.0),
              RampCase(33, 200, 4.0, 1.0), RampCase(16, 64, 2.0, 4.0), RampCase(16, 16, 8.0, 2.0, 0.25)]


def ramp_input():
    yy, xx = np.mgrid[0:BIG[0], 0:BIG[1]].astype(np.float64)
    x = np.stack([np.stack([a * xx + b * yy + d + o for a, b, d in RAMP_ABD]) for o in RAMP_IMAGE_OFFSET])
    assert np.array_equal(x.astype(np.float32), x)
    return x.astype(np.float32)


def ramp_rois_and_expected(case):
    """Two boxes (one per batch image) with top-left sample-space corners (8, 4) and (24.25, 12.5); expected f64[2, 3, ph, pw]."""
    corners = [(0, 8.0, 4.0), (1, 24.25, 12.5)]
    rois, want = [], []
    for b, sw, sh in corners:
        rw, rh = case.pw * case.bin_w, case.ph * case.bin_h
        assert sw + rw <= BIG[1] - 1 and sh + rh <= BIG[0] - 1
        rois.append([b, (sw + 0.5) / case.scale, (sh + 0.5) / case.scale, (sw + rw + 0.5) / case.scale, (sh + rh + 0.5) / case.scale])
        cx = sw + (np.arange(case.pw) + 0.5) * case.bin_w
        cy = sh + (np.arange(case.ph) + 0.5) * case.bin_h
        want.append(np.stack([a * cx[None, :] + b_ * cy[:, None] + d + RAMP_IMAGE_OFFSET[b] for a, b_, d in RAMP_ABD]))
    rois = np.array(rois, np.float64)
    assert np.array_equal(rois.astype(np.float32), rois)
    return rois.astype(np.float32), np.stack(want)


# ---- RoIPool
POOL_OUTPUTS = [(1, 1), (7, 5), (16, 16), (3, 100), (33, 65)]
POOL_SOURCES = [(1, 60, 80), (4, 60, 80), (5, 60, 80), (4, 60, 1), (5, 1, 80)]          # C, H, W


def pool_rois(h, w, scale=1.0):
    """Boxes inside the image, across each border and all of them, outside it, with .5 corners of both signs (round half away
    from zero), a single pixel and an inverted box; in ROI coordinates (pixel coordinates / spatial_scale)."""
    r = np.array([[0, 0.2 * w, 0.2 * h, 0.7 * w, 0.8 * h],
                  [1, -0.3 * w - 3, 0.1 * h, 0.5 * w, 0.6 * h],            # left
                  [2, 0.4 * w, -0.4 * h - 2, 0.9 * w, 0.5 * h],            # top
                  [0, 0.5 * w, 0.3 * h, 1.4 * w + 3, 0.8 * h],             # right
                  [1, 0.1 * w, 0.6 * h, 0.6 * w, 1.5 * h + 2],             # bottom
                  [2, -7.0, -5.0, w + 6.0, h + 9.0],                       # every border
                  [0, w + 20.0, h + 20.0, w + 40.0, h + 50.0],             # outside: zeros
                  [1, -40.0, -30.0, -12.0, -9.0],                          # outside, negative side
                  [2, 2.5, 3.5, 0.5 * w + 0.5, 0.5 * h + 1.5],             # .5 corners round up
                  [0, -2.5, -0.5, 0.5 * w - 0.5, 0.5 * h + 0.5],           # ... and away from zero when negative
                  [1, 1.5, -1.5, 1.5, -1.5],
                  [2, 0.5 * w, 0.5 * h, 0.5 * w, 0.5 * h],                 # a single pixel
                  [0, 0.6 * w, 0.7 * h, 0.2 * w, 0.1 * h]], np.float64)    # inverted: width = height = 1
    r[:, 1:] /= scale
    return r.astype(np.float32)


def pool_input(c, h, w):
    rng = np.random.default_rng([11, c, h, w])
    return rng.standard_normal((3, c, h, w)).astype(np.float32)
