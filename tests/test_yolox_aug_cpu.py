"""CPU: the restatement of YOLOX's training augmentation (tests/yolox_aug_ref.py) against the committed warp oracle and against what the
reference's own ``MosaicDetection`` / ``TrainTransform`` returned (tests/golden/yolox_aug_golden.npz), and the host side of
``det.yolox.data`` — the draws, the cv2 requests, the affine matrix, the labels — against what the reference drew, asked for and
returned.  Every comparison is equality."""
import os
import random

import numpy as np
import pytest

from gdrnpp_bop2022_amd.det.yolox.data import data_augment as DA
from gdrnpp_bop2022_amd.det.yolox.data import mosaic as MZ
from oracle import postproc as OP
from tests import yolox_aug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "yolox_aug_golden.npz"))
NAMES = list(R.CASES)


def g(name, key):
    return GOLDEN[f"{name}_{key}"]


def plan_of(name):
    """-> (the plan, the two generators after it)."""
    c = R.CASES[name]
    py, npr = random.Random(c["py_seed"]), np.random.RandomState(c["np_seed"])
    item = MZ.draw_mosaic_item(dict(MZ.MOSAIC_DEFAULTS, **c["kw"]), R.case_dataset(name), c["idx"], c["dim"], c["enable_mosaic"], py, npr)
    return item, py, npr


# ---- the restated cv2 calls ----------------------------------------------------------------------------------------------------------------

def _matrices():
    rng = np.random.RandomState(5)
    out = [np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[1.0, 0, 3.0], [0, 1.0, -2.0]]), np.array([[2.0, 0, 0.5], [0, 0.5, 0.25]]),
           np.array([[-1.0, 0, 20.0], [0, 1.0, 0]]), np.array([[0.0, 1.0, 0], [1.0, 0, 0]])]
    for _ in range(8):
        a, s = rng.uniform(-np.pi, np.pi), rng.uniform(0.3, 2.5)
        out.append(np.array([[np.cos(a) * s, np.sin(a) * s + rng.uniform(-0.2, 0.2), rng.uniform(-15, 15)],
                             [-np.sin(a) * s, np.cos(a) * s, rng.uniform(-15, 15)]]))
    return out


@pytest.mark.parametrize("k", range(13))
def test_warp_affine_u8_equals_the_committed_oracle(k):
    M = _matrices()[k]
    img = np.random.RandomState(k).randint(0, 256, (23, 31, 3)).astype(np.uint8)
    for n in (17, 40):
        ours, ref = R.warp_affine_u8(img, M, (n, n), border=0), OP.warp_affine(img, M, n)
        assert ours.dtype == np.uint8 and (ours == ref).all(), (k, n, np.argwhere(ours != ref)[:4].tolist())


def test_warp_affine_u8_border_and_identity():
    img = np.random.RandomState(0).randint(0, 256, (9, 11, 3)).astype(np.uint8)
    eye = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    out = R.warp_affine_u8(img, eye, (14, 12), border=114)
    assert (out[:9, :11] == img).all() and (out[9:] == 114).all() and (out[:, 11:] == 114).all()
    assert (R.warp_affine_u8(img, np.array([[1.0, 0, 500.0], [0, 1.0, 0]]), (14, 12), border=114) == 114).all()


def test_hsv_grey_and_zero_saturation_round_trip_exactly():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)[None]
    for rgb in (False, True):
        hsv = R.to_hsv_u8(grey, rgb)
        assert not hsv[..., 0].any() and not hsv[..., 1].any() and (hsv[..., 2] == grey[..., 0]).all()
        assert (R.from_hsv_u8(hsv, rgb) == grey).all()
    any_hue = np.stack([np.arange(256) % 180, np.zeros(256), np.arange(256)], -1).astype(np.uint8)[None]
    assert (R.from_hsv_u8(any_hue, False) == grey).all()


# (b, g, r) -> (h, s, v), worked by hand from the integer formulas: sdiv[v] = rint(1044480 / v), hdiv[d] = rint(122880 / d)
HSV_BY_HAND = [
    ((0, 0, 255), (0, 255, 255)),          # red: v == r, h = g - b = 0
    ((0, 255, 0), (60, 255, 255)),         # green: h = 2 diff -> (510 * 482 + 2048) >> 12 = 60
    ((255, 0, 0), (120, 255, 255)),        # blue: h = 4 diff -> 120
    ((0, 255, 255), (30, 255, 255)),       # v == r == g: the r test comes first, h = g - b = 255 -> 30
    ((255, 0, 255), (150, 255, 255)),      # v == r == b: h = g - b = -255 -> -30 + 180
    ((255, 255, 0), (90, 255, 255)),       # v == g == b (r smaller): the g test, h = b - r + 2 diff = 765 -> 90
    ((1, 0, 255), (0, 255, 255)),          # h = -1: (-482 + 2048) >> 12 = 0, not negative: stays 0
    ((10, 0, 200), (179, 255, 200)),       # h = -10: hdiv[200] = 614, (-6140 + 2048) >> 12 = -1 -> 179
    ((100, 100, 100), (0, 0, 100)),        # grey
    ((50, 100, 150), (15, 170, 150)),      # diff 100: s = (100 * 6963 + 2048) >> 12 = 170; h = 50 * 1229 -> 15
    ((200, 120, 40), (105, 204, 200)),     # v == b: h = r - g + 4 diff = -80 + 640 = 560, hdiv[160] = 768 -> 105; s = 160 * 5222 -> 204
    ((7, 7, 6), (90, 36, 7)),              # v == g == b, diff 1: h = 7 - 6 + 2 = 3, hdiv[1] = 122880 -> 90; s = sdiv[7] = 149211 -> 36
]


@pytest.mark.parametrize("bgr,hsv", HSV_BY_HAND)
def test_hsv_hand_worked_pixels(bgr, hsv):
    px = np.array(bgr, np.uint8)[None, None]
    assert R.to_hsv_u8(px, False)[0, 0].tolist() == list(hsv)
    assert R.to_hsv_u8(px[..., ::-1], True)[0, 0].tolist() == list(hsv)


def test_hue_stays_below_180_and_rgb_is_bgr_reversed():
    rng = np.random.RandomState(1)
    px = rng.randint(0, 256, (512, 512, 3)).astype(np.uint8)
    px[:64] = (px[:64] // 64) * 85                     # ties between channels
    hsv = R.to_hsv_u8(px, False)
    assert int(hsv[..., 0].max()) < 180
    back = R.from_hsv_u8(hsv, False).astype(int)
    assert (R.from_hsv_u8(hsv, True)[..., ::-1] == back).all()


def test_rotation_matrix_rows():
    M = DA.getRotationMatrix2D(center=(0, 0), angle=30.0, scale=2.0)
    a, b = np.cos(30.0 * (np.pi / 180)) * 2.0, np.sin(30.0 * (np.pi / 180)) * 2.0
    assert M.tolist() == [[a, b, 0.0], [-b, a, 0.0]]
    assert (M == R.getRotationMatrix2D((0, 0), 30.0, 2.0)).all()


# ---- the host plan against the reference's run -------------------------------------------------------------------------------------------------

def test_fixture_holds_every_case():
    assert all(f"{n}_image" in GOLDEN for n in NAMES)
    dims = {R.CASES[n]["dim"] for n in NAMES}
    assert dims == {(32, 48), (48, 32)}


@pytest.mark.parametrize("name", NAMES)
def test_plan_reproduces_every_draw(name):
    item, py, npr = plan_of(name)
    assert np.array_equal(np.array(item["draws"], np.float64), g(name, "draws"))
    assert py.random() == float(g(name, "next_py")) and npr.rand() == float(g(name, "next_np"))      # consumed exactly as far
    obs = R.observed(item)
    for k, v in R.CASES[name]["expect"].items():
        if k in obs:
            assert obs[k] == v, (k, obs[k], v)


@pytest.mark.parametrize("name", NAMES)
def test_plan_reproduces_matrix_labels_and_ids(name):
    item, _, _ = plan_of(name)
    if item["branch"] != "plain":
        assert item["M"].tobytes() == g(name, "M").tobytes()
    labels = g(name, "labels")
    assert item["padded_labels"].dtype == np.float32 and item["padded_labels"].shape == labels.shape
    assert item["padded_labels"].tobytes() == labels.tobytes()
    assert [item["scene_im_id"], str(tuple(int(v) for v in item["img_info"])), str(item["img_id"])] == g(name, "ids").tolist()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_every_image_and_cv2_request(name):
    item, _, _ = plan_of(name)
    cv2 = R.Cv2()
    out = R.run_item(item, DA.hsv_luts, cv2)
    ref = g(name, "image")
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert (out == ref).all(), np.argwhere(out != ref)[:4].tolist()
    assert np.array_equal(np.array(cv2.log, np.int64).reshape(-1, 5), g(name, "ops"))


def test_max_labels_truncates_and_empty_pads_zeros():
    item, _, _ = plan_of("mosaic_max_labels")
    assert item["padded_labels"].shape == (3, 5) and item["padded_labels"].any(1).all()
    item, _, _ = plan_of("mosaic_no_labels")
    assert item["empty"] and not item["padded_labels"].any() and item["padded_labels"].shape == (50, 5)


def test_hsv_luts_are_the_reference_expressions():
    r = np.array([1.3, 0.6, 1.45])
    lut = DA.hsv_luts(r, np.uint8)
    x = np.arange(256)
    assert lut.shape == (3, 256) and lut.dtype == np.uint8
    assert lut[0].tolist() == [int((v * 1.3) % 180) for v in x]
    assert lut[1].tolist() == [int(min(v * 0.6, 255)) for v in x] and lut[2].tolist() == [int(min(v * 1.45, 255)) for v in x]


def test_color_aug_prob_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="COLOR_AUG_PROB"):
        MZ.MosaicDetectionHip(R.case_dataset("plain_copy"), (32, 48), COLOR_AUG_PROB=0.5, COLOR_AUG_TYPE="code")
    with pytest.raises(TypeError, match="unknown keywords"):
        MZ.MosaicDetectionHip(R.case_dataset("plain_copy"), (32, 48), mosiac_prob=0.5)
