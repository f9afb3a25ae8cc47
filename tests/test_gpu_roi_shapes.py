"""The ROI-preparation kernels over the launch shapes they choose from their arguments (-m gpu): gdrnpp_roi_align, gdrnpp_roi_pool
and the generic crop-resize kernels, each bit for bit against its CPU oracle.  The case lists (tests/roi_cases.py) are the ones
tests/test_crop_pins.py holds the oracle itself to, against an fp64 formulation written from the definition.

What the ROIAlign cases are built around: a wave's y taps are computed one per lane and fetched with v_readlane, which ignores
EXEC, so every lane of a live wave has to compute its tap — also the lanes of a partial wave that lie beyond pooled_w.  A kernel
that lets those lanes leave first is right for pooled_w = 64 / 128 / 256 (the product's crop) and wrong for a partial wave as soon
as 4 * gh exceeds its active lanes: (pooled_w, gh) = (7, 2), (16, 5), (100, 10), (130, 1), (200, 3) and beyond."""
import numpy as np
import pytest
import torch

from oracle import postproc as P
from tests import roi_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", RC.ALIGN_CASES, ids=lambda c: c.id)
def test_roi_align_bit_exact_over_launch_shapes(hip, case):
    """Boxes inside the image, from negative coordinates, past the far border and outside the sampling window (zeros), over both
    batch images: every output bit equals oracle/roi_align_oracle.c."""
    x = RC.align_input(case)
    rois = RC.align_rois(case)
    gh, gw = RC.align_grid(case, rois)
    assert (gh == case.gh).all() and (gw == case.gw).all(), (gh, gw)
    out = hip.roi_align(_t(x), _t(rois), (case.ph, case.pw), case.scale, case.sampling_ratio, case.aligned).cpu().numpy()
    ref = P.roi_align(x, rois, (case.ph, case.pw), case.scale, case.sampling_ratio, case.aligned)
    assert out.shape == ref.shape == (len(rois), case.c, case.ph, case.pw)
    bad = np.argwhere(_bits(out) != _bits(ref))
    assert len(bad) == 0, (len(bad), bad[:5].tolist())
    assert ref[0].any() and not ref[3].any() and not ref[4].any()          # a box that samples the image, the two that cannot


def test_roi_align_degenerate_boxes_give_zeros(hip):
    """Inverted and zero-area boxes with aligned=True have gh <= 0 or gw <= 0: no samples, so mean over max(gh * gw, 1) of
    nothing = 0 everywhere, as in the oracle (the kernel divides its lane index by max(gh, 1))."""
    case = RC.DEGENERATE_CASE
    x = RC.align_input(case)
    for size in ((case.ph, case.pw), (5, 7), (16, 256)):
        out = hip.roi_align(_t(x), _t(RC.DEGENERATE_ROIS), size).cpu().numpy()
        ref = P.roi_align(x, RC.DEGENERATE_ROIS, size)
        assert not ref.any()
        assert np.array_equal(_bits(out), _bits(ref)), size


def test_roi_align_and_roi_pool_without_rois(hip):
    """n_rois == 0: status 0 from the C ABI without a launch, an empty [0, C, oh, ow] tensor from the wrappers."""
    x = _t(RC.align_input(RC.DEGENERATE_CASE))
    rois = torch.zeros((0, 5), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    lib = hip.load()
    assert lib.gdrnpp_roi_align(x.data_ptr(), None, None, 0, 3, 60, 80, 16, 100, 1.0, 0, 1, st) == 0
    assert lib.gdrnpp_roi_pool(x.data_ptr(), None, None, 0, 3, 60, 80, 16, 100, 1.0, st) == 0
    out = hip.roi_align(x, rois, (16, 100))
    assert out.shape == (0, 3, 16, 100) and out.dtype == torch.float32
    out = hip.roi_pool(x, rois, (7, 5))
    assert out.shape == (0, 3, 7, 5) and out.dtype == torch.float32


GUARD = 4096            # floats before and after the output block
GUARD_BITS = 0x5A5AA5A5


@pytest.mark.parametrize("case", RC.CONTAINMENT_CASES, ids=lambda c: c.id)
def test_roi_align_stores_stay_inside_the_output_block(hip, case):
    """The lanes of a partial wave beyond pooled_w compute (column pooled_w - 1 again) but must not store: the C ABI writes into
    the middle of an allocation whose words before and after the [n, C, PH, PW] block carry a fixed bit pattern; the pattern is
    untouched and the block equals the oracle."""
    x = RC.align_input(case)
    rois = RC.align_rois(case)
    n = len(rois)
    numel = n * case.c * case.ph * case.pw
    buf = torch.full((GUARD + numel + GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV)
    xd, rd = _t(x), _t(rois)
    rc = hip.load().gdrnpp_roi_align(xd.data_ptr(), rd.data_ptr(), buf.data_ptr() + 4 * GUARD, n, case.c, case.h, case.w, case.ph,
                                     case.pw, case.scale, case.sampling_ratio, 1 if case.aligned else 0,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:GUARD] == GUARD_BITS).all() and (got[GUARD + numel:] == GUARD_BITS).all()
    ref = P.roi_align(x, rois, (case.ph, case.pw), case.scale, case.sampling_ratio, case.aligned)
    assert np.array_equal(got[GUARD:GUARD + numel], _bits(ref).ravel())


@pytest.mark.parametrize("case", RC.RAMP_CASES, ids=lambda c: c.id)
def test_roi_align_linear_ramp_closed_form(hip, case):
    """x[c, y, x] = a x + b y + d: bilinear interpolation is exact, every sample lies inside the image, so each output IS the ramp
    at its bin centre — equality, since slopes, corners and bin sizes are dyadic and gh * gw is a power of two (the CPU suite holds
    the oracle to the same equality).  No oracle involved."""
    x = RC.ramp_input()
    rois, want = RC.ramp_rois_and_expected(case)
    out = hip.roi_align(_t(x), _t(rois), (case.ph, case.pw), case.scale).cpu().numpy()
    assert np.array_equal(out.astype(np.float64), want)


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("src", RC.POOL_SOURCES, ids=lambda s: "c%d-src%dx%d" % s)
@pytest.mark.parametrize("size", RC.POOL_OUTPUTS, ids=lambda s: "out%dx%d" % s)
def test_roi_pool_bit_exact_over_shapes(hip, size, src, scale):
    """RoIPool against oracle/roi_align_oracle.c: boxes inside, across every border, outside, .5 corners of both signs."""
    c, h, w = src
    x = RC.pool_input(c, h, w)
    rois = RC.pool_rois(h, w, scale)
    out = hip.roi_pool(_t(x), _t(rois), size, scale).cpu().numpy()
    ref = P.roi_pool(x, rois, size, scale)
    assert out.shape == ref.shape == (len(rois), c) + size
    assert np.array_equal(_bits(out), _bits(ref))
    assert ref[5].any() and not ref[6].any() and not ref[7].any()


def test_roi_pool_grid_stride_second_trip(hip):
    """More output elements than the launch's 65536 * 4 workgroups of 256 threads hold (67 108 864): the grid-stride loop takes a
    second trip for the tail.  4 100 ROIs -> 1 x 128 x 128 = 67 174 400 elements (269 MB), small boxes on a small image."""
    rng = np.random.default_rng(13)
    x = rng.standard_normal((2, 1, 24, 32)).astype(np.float32)
    n = 4100
    x1, y1 = rng.uniform(-6, 30, n), rng.uniform(-6, 22, n)
    rois = np.stack([rng.integers(0, 2, n), x1, y1, x1 + rng.uniform(0, 20, n), y1 + rng.uniform(0, 16, n)], 1).astype(np.float32)
    assert n * 128 * 128 > 65536 * 4 * 256
    out = hip.roi_pool(_t(x), _t(rois), 128)
    ref = _t(P.roi_pool(x, rois, 128))
    assert out.shape == ref.shape
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert bool(ref[-1].any() or ref[-2].any() or ref[-3].any())          # the second trip's ROIs are not all empty


def _crop_inputs():
    rng = np.random.default_rng(21)
    n_im, H, W = 2, 480, 640
    images = rng.integers(0, 256, (n_im, H, W, 3), dtype=np.uint8)
    depths = rng.uniform(0.3, 2.0, (n_im, H, W)).astype(np.float32)
    depths[rng.uniform(size=depths.shape) < 0.1] = 0
    b = 12
    centers = np.stack([rng.uniform(-20, 660, b), rng.uniform(-20, 500, b)], 1)     # some ROIs leave the image
    scales = rng.uniform(40, 640, b)
    im_idx = rng.integers(0, n_im, b).astype(np.int32)
    return images, depths, im_idx, centers, scales


@pytest.mark.parametrize("with_depth", [True, False], ids=["depth", "nodepth"])
@pytest.mark.parametrize("res,small", [(64, 16), (128, 32), (320, 80), (256, 32)])
def test_crop_resize_generic_kernels_bit_exact(hip, res, small, with_depth):
    """out_res != 256 launches crop_img_depth_kernel and crop_coord2d_kernel, which the 256 x 256 / 64 x 64 tests never do;
    (256, 32) is the 256 kernel with a non-default coordinate map.  ROIs leaving the image, an integer translation, a 4x
    up-sampling, a strong down-sampling; with and without depth, and with want_img=False: all outputs bit for bit the
    cv2.warpAffine restatement."""
    images, depths, im_idx, centers, scales = _crop_inputs()
    centers[0], scales[0] = (320.0, 240.0), float(res)                               # pure integer translation
    centers[1], scales[1] = (100.5, 77.25), res / 4.0                                # 4x up-sampling
    centers[2], scales[2] = (300.0, 250.0), 640.0                                    # strong down-sampling
    dep_d = _t(depths) if with_depth else None
    img, dep, c2d = hip.crop_resize_roi(_t(images), dep_d, _t(im_idx), _t(centers), _t(scales), out_res=res, out_res_small=small)
    img2, dep2, c2d2 = hip.crop_resize_roi(_t(images), dep_d, _t(im_idx), _t(centers), _t(scales), out_res=res, out_res_small=small,
                                           want_img=False)
    assert img2 is None and (dep is None) == (dep2 is None) == (not with_depth)
    assert img.shape == (len(scales), 3, res, res) and c2d.shape == (len(scales), 2, small, small)
    img, c2d, c2d2 = img.cpu().numpy(), c2d.cpu().numpy(), c2d2.cpu().numpy()
    if with_depth:
        dep, dep2 = dep.cpu().numpy(), dep2.cpu().numpy()
    for i in range(len(scales)):
        o_img, o_dep, o_c2d = P.crop_resize_roi(images[im_idx[i]], depths[im_idx[i]] if with_depth else None, centers[i], scales[i],
                                                input_res=res, out_res=small)
        assert np.array_equal(_bits(img[i]), _bits(o_img)), i
        assert np.array_equal(_bits(c2d[i]), _bits(o_c2d)) and np.array_equal(_bits(c2d2[i]), _bits(o_c2d)), i
        if with_depth:
            assert np.array_equal(_bits(dep[i]), _bits(o_dep)) and np.array_equal(_bits(dep2[i]), _bits(o_dep)), i
    h = res // 2
    assert np.array_equal((img[0] * 255).round().astype(np.uint8).transpose(1, 2, 0),
                          images[im_idx[0], 240 - h:240 + h, 320 - h:320 + h])
