"""-m gpu: ``gdrnpp_yolox_train_inputs`` (csrc/yolox_aug.hip) through ``hip_lib.yolox_train_inputs`` and ``det.yolox.data.MosaicDetectionHip``.

Every comparison is EQUALITY: the resizes, the warp and RGB -> HSV are integer arithmetic, the blend and HSV -> RGB are fp32 operations
rounded one by one.  The yardsticks are what the reference's own ``MosaicDetection`` / ``TrainTransform`` returned
(tests/golden/yolox_aug_golden.npz) and, for the shapes and plans the fixture does not hold, tests/yolox_aug_ref.py, which
tests/test_yolox_aug_cpu.py ties to that fixture."""
import os
import random

import numpy as np
import pytest
import torch

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.det.yolox.data import data_augment as DA
from gdrnpp_bop2022_amd.det.yolox.data import mosaic as MZ
from gdrnpp_bop2022_amd.gdrn_modeling.train_inputs import resize_request
from tests import yolox_aug_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "yolox_aug_golden.npz"))
NAMES = list(R.CASES)


def g(name, key):
    return GOLDEN[f"{name}_{key}"]


def generators(name):
    c = R.CASES[name]
    return random.Random(c["py_seed"]), np.random.RandomState(c["np_seed"])


def wrapper_of(name):
    c = R.CASES[name]
    return MZ.MosaicDetectionHip(R.case_dataset(name), c["dim"], **c["kw"])


def plan_of(name):
    c = R.CASES[name]
    py, npr = generators(name)
    return wrapper_of(name).plan([c["idx"]], None, c["enable_mosaic"], py, npr)[0]


def launch(items, dim):
    """-> (imgs, flags) as NumPy."""
    imgs, flags = MZ.launch_items(items, dim, DEV)
    return imgs.cpu().numpy(), flags.cpu().numpy()


def assert_same(ours, ref, what):
    assert ours.shape == ref.shape, (what, ours.shape, ref.shape)
    bad = ours != ref
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), ours[bad][:4].tolist(), ref[bad][:4].tolist())


# ---- 1. the reference's own results --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_batch_equals_the_reference_on_every_case(name):
    c = R.CASES[name]
    py, npr = generators(name)
    imgs, labels, scene_im_ids, img_infos, img_ids = wrapper_of(name).batch([c["idx"]], None, c["enable_mosaic"], py, npr)
    assert imgs.dtype == torch.float32 and imgs.is_cuda and tuple(imgs.shape) == (1, 3) + tuple(c["dim"])
    assert_same(imgs[0].cpu().numpy(), g(name, "image").astype(np.float32), name)
    assert labels.dtype == torch.float32 and labels.is_cuda
    assert labels[0].cpu().numpy().tobytes() == g(name, "labels").tobytes()
    assert [scene_im_ids[0], str(tuple(int(v) for v in img_infos[0])), str(img_ids[0])] == g(name, "ids").tolist()
    assert py.random() == float(g(name, "next_py")) and npr.rand() == float(g(name, "next_np"))


MIXED = ["plain_mirror", "mosaic_nomixup", "mixup_up_flip", "mosaic_fallback", "mixup_down_noflip"]


def test_one_call_of_five_mixed_items_equals_five_calls():
    items = [plan_of(n) for n in MIXED]
    assert [it["branch"] for it in items] == ["plain", "mosaic", "mixup", "mosaic", "mixup"] and items[3]["fallback"]
    out, flags = launch(items, (32, 48))
    assert not flags.any()
    for b, (name, item) in enumerate(zip(MIXED, items)):
        one, one_flags = launch([item], (32, 48))
        assert_same(out[b], one[0], name)
        assert_same(out[b], g(name, "image").astype(np.float32), name)
        assert not one_flags.any()


# ---- 2. the shapes and plans the fixture does not hold: against the restatement ------------------------------------------------------------

def make_item(H, W, branch, seed, *, hsv=False, mirror=False, fallback=False, hsv2=False, hsv2_rgb=True, M=None):
    """A valid plan drawn directly (not through the reference's size arithmetic, which has no answer at W = 1)."""
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, 256, (rng.randint(3, 40), rng.randint(3, 40), 3)).astype(np.uint8) for _ in range(5)]
    item = dict(branch=branch, input_dim=(H, W), sources=[], M=None, mix=None, empty=False, hsv=hsv, hsv_r=rng.uniform(0.5, 1.5, 3), mirror=mirror,
                fallback=fallback, hsv2=hsv2, hsv2_r=rng.uniform(0.5, 1.5, 3), hsv2_rgb=hsv2_rgb)
    if branch == "plain":                   # by seed: the copy, the 2:1 area mean, the linear form
        h0, w0 = [(H, W), (2 * H, 2 * W), (H + 3, W + 5)][seed % 3]
        im = rng.randint(0, 256, (h0, w0, 3)).astype(np.uint8)
        _, rw, rh = DA.preproc_sizes(h0, w0, (H, W))
        item["sources"].append(MZ._source(im, resize_request(w0, h0, dsize=(rw, rh))))
        return item
    yc, xc = int(rng.uniform(0.5 * H, 1.5 * H)), int(rng.uniform(0.5 * W, 1.5 * W))
    for k in range(4):
        im = images[k]
        req = resize_request(im.shape[1], im.shape[0], dsize=(int(rng.randint(1, W + 1)), int(rng.randint(1, H + 1))))
        (lx1, ly1, lx2, ly2), (sx1, sy1, _, _) = MZ.get_mosaic_coordinate(None, k, xc, yc, req["dw"], req["dh"], H, W)
        item["sources"].append(MZ._source(im, req, lx1, ly1, sx1, sy1, lx2 - lx1, ly2 - ly1))
    if M is None:
        a, s = rng.uniform(-0.2, 0.2), rng.uniform(0.6, 1.4)
        M = np.array([[np.cos(a) * s, np.sin(a) * s + 0.03, rng.uniform(-0.1, 0.1) * W], [-np.sin(a) * s + 0.02, np.cos(a) * s, rng.uniform(-0.1, 0.1) * H]])
    item["M"] = np.asarray(M, np.float64)
    if branch == "mixup":
        im = images[4]
        item["sources"].append(MZ._source(im, resize_request(im.shape[1], im.shape[0], dsize=(int(rng.randint(1, W + 1)), int(rng.randint(1, H + 1))))))
        jit = rng.uniform(0.5, 1.5)
        jw, jh = max(int(W * jit), 1), max(int(H * jit), 1)
        item["mix"] = dict(jw=jw, jh=jh, req2=resize_request(W, H, dsize=(jw, jh)), flip=bool(rng.rand() > 0.5),
                           x_off=int(rng.randint(0, max(jw - W, 1))), y_off=int(rng.randint(0, max(jh - H, 1))))
    return item


def check_against_restatement(items, dim, what):
    out, flags = launch(items, dim)
    assert not flags.any()
    for b, item in enumerate(items):
        assert_same(out[b], R.run_item(item, DA.hsv_luts), (what, b))
    return out


EDGES = [(5, 1), (6, 63), (6, 64), (7, 65), (1, 70)]


@pytest.mark.parametrize("H,W", EDGES)
@pytest.mark.parametrize("branch", ["plain", "mosaic", "mixup"])
def test_launch_edges_at_batch_one(H, W, branch):
    for seed in range(3):          # jit below and above 1, flip on and off come up over the seeds
        item = make_item(H, W, branch, 100 * W + 10 * H + seed, hsv=True, mirror=seed != 1, hsv2=branch != "plain", hsv2_rgb=seed == 0)
        check_against_restatement([item], (H, W), (H, W, branch, seed))


def test_fallback_drops_the_first_hsv_pass_and_the_mirror_only():
    for branch in ("plain", "mosaic", "mixup"):
        item = make_item(20, 37, branch, 7, hsv=True, mirror=True, fallback=True, hsv2=branch != "plain")
        out = check_against_restatement([item], (20, 37), branch)
        again = dict(item, hsv=False, mirror=False, fallback=False)
        assert_same(launch([again], (20, 37))[0], out, branch)
        kept = dict(item, fallback=False)
        assert (launch([kept], (20, 37))[0] != out).any()


def test_mixup_second_resize_as_copy_and_as_area_mean():
    H, W = 20, 36
    for jw, jh in ((W, H), (W // 2, H // 2)):
        for flip in (False, True):
            item = make_item(H, W, "mixup", 21)
            req2 = resize_request(W, H, dsize=(jw, jh))
            assert hip_lib.YOLOX_AUG_MODES[req2["mode"]] == ("copy" if jw == W else "area")
            item["mix"] = dict(jw=jw, jh=jh, req2=req2, flip=flip, x_off=0, y_off=0)
            check_against_restatement([item], (H, W), (jw, jh, flip))


def test_more_than_one_workgroup_in_every_grid_dimension():
    items = [make_item(70, 130, b, 3 + k, hsv=True, mirror=k == 1, hsv2=b != "plain") for k, b in enumerate(["mixup", "plain", "mosaic"])]
    check_against_restatement(items, (70, 130), "70x130")


def canvas_of(item):
    H, W = item["input_dim"]
    canvas = np.full((2 * H, 2 * W, 3), 114, np.uint8)
    cv2 = R.Cv2()
    for s in item["sources"][:4]:
        tile = cv2.resize(s["image"], (s["dw"], s["dh"]))
        canvas[s["l_y"]: s["l_y"] + s["ph"], s["l_x"]: s["l_x"] + s["pw"]] = tile[s["s_y"]: s["s_y"] + s["ph"], s["s_x"]: s["s_x"] + s["pw"]]
    return canvas


def test_identity_affine_returns_the_canvas_window():
    item = make_item(24, 40, "mosaic", 11, M=[[1.0, 0, 0], [0, 1.0, 0]])
    out, flags = launch([item], (24, 40))
    assert_same(out[0], canvas_of(item)[:24, :40].transpose(2, 0, 1).astype(np.float32), "identity")
    shifted = make_item(24, 40, "mosaic", 11, M=[[1.0, 0, -13.0], [0, 1.0, -9.0]])
    assert_same(launch([shifted], (24, 40))[0][0], canvas_of(item)[9:33, 13:53].transpose(2, 0, 1).astype(np.float32), "integer shift")
    assert not flags.any()


def test_affine_that_leaves_the_canvas_returns_the_border_everywhere():
    item = make_item(24, 40, "mosaic", 12, M=[[1.0, 0, 3.0 * 40], [0, 1.0, 0]])
    out, flags = launch([item], (24, 40))
    assert (out == 114.0).all() and not flags.any()


def test_singular_matrix_is_flagged_and_warps_as_opencv_does():
    items = [make_item(16, 20, "mosaic", 13, M=np.zeros((2, 3))), make_item(16, 20, "mosaic", 14)]
    out, flags = launch(items, (16, 20))
    assert flags.tolist() == [1, 0]
    for b in range(2):
        assert_same(out[b], R.run_item(items[b], DA.hsv_luts), b)


def test_two_calls_give_equal_bits():
    items = [plan_of(n) for n in MIXED]
    a, _ = MZ.launch_items(items, (32, 48), DEV)
    b, _ = MZ.launch_items(items, (32, 48), DEV)
    assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()


def test_bad_rows_are_refused_before_anything_is_launched():
    item = make_item(16, 20, "mosaic", 15)
    beyond = dict(item, sources=[dict(item["sources"][0], l_x=2 * 20 - 1, pw=2)] + item["sources"][1:])
    with pytest.raises(RuntimeError, match="row 0 source 0: paste"):
        launch([beyond], (16, 20))
    src = torch.zeros(10, dtype=torch.uint8, device=DEV)
    lut = torch.zeros((1, 2, 3, 256), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="lies outside the 10 bytes of src"):
        hip_lib.yolox_train_inputs(src, hip_lib.yolox_aug_table([dict(branch=0, s0_w=4, s0_h=4, s0_dw=4, s0_dh=4, s0_pw=4, s0_ph=4)]), lut, 8, 8)
    with pytest.raises(RuntimeError, match="branch=7"):
        hip_lib.yolox_train_inputs(src, hip_lib.yolox_aug_table([dict(branch=7)]), lut, 8, 8)
    out, flags = hip_lib.yolox_train_inputs(src, hip_lib.yolox_aug_table([]), lut[:0], 8, 8)
    assert tuple(out.shape) == (0, 3, 8, 8) and flags.numel() == 0
