"""-m gpu: ``gdrnpp_replace_bg`` (csrc/replace_bg.hip) through the binding ``hip_lib.replace_bg`` and ``gdrn_modeling.train_inputs``.

Every comparison is EQUALITY: the mask's extents are integers, the cut line is three correctly rounded fp64 operations truncated, the
background pixel is OpenCV's integer arithmetic.  The yardsticks are what the reference's own methods returned
(tests/golden/replace_bg_golden.npz) and, for the shapes the reference cannot be asked about, tests/replace_bg_ref.py, which
tests/test_replace_bg_cpu.py ties to that fixture."""
import os
import random

import numpy as np
import pytest
import torch

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.gdrn_modeling import train_inputs as TI
from gdrnpp_bop2022_amd.gdrn_modeling import train_targets as TT
from tests import replace_bg_ref as R
from tests import roi_targets_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "replace_bg_golden.npz"))
NAMES = list(R.CASES)


def g(name, key):
    return GOLDEN[f"{name}_{key}"]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def row_of(pool, ind, H, W, cut, u, geometry=None):
    geo = geometry if geometry is not None else TI.bg_geometry(*pool.sizes[ind], H, W)
    return dict(do=1, bg_off=pool.offsets[ind], bg_stride=pool.sizes[ind][1], cut=cut, u=u, **geo)


def launch(images, masks, pool, rows):
    """-> (composite, mask_trunc, flags) as NumPy; the inputs are host arrays and stay as they are."""
    dev_images = T(images)
    mask_trunc, flags = hip_lib.replace_bg(dev_images, T(masks), pool.data, hip_lib.replace_bg_table(rows))
    return dev_images.cpu().numpy(), mask_trunc.cpu().numpy(), flags.cpu().numpy()


def assert_same(ours, ref, what):
    bad = ours != ref
    assert ours.shape == ref.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- 1. the reference's own results --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_equals_the_reference_on_every_case(name):
    c = R.CASES[name]
    image, mask, bgs = R.case_inputs(name)
    pool = TI.BgPool(bgs, DEV)
    if int(g(name, "do")):
        geo = TI.bg_geometry(*c["bgs"][int(g(name, "ind"))], c["H"], c["W"], c["keep_aspect"], np.random.RandomState(c["np_seed"]))
        rows = [row_of(pool, int(g(name, "ind")), c["H"], c["W"], int(g(name, "cut")), float(g(name, "u")), geo)]
    else:
        rows = [dict(do=0)]
    out, keep, flags = launch(image[None], mask[None], pool, rows)
    assert_same(out[0], g(name, "composite"), name)
    assert_same(keep[0], g(name, "mask_trunc"), name)
    assert_same(out[0][keep[0] != 0], image[keep[0] != 0], (name, "kept pixels"))
    assert not flags.any()


# ---- 2. the shapes the reference cannot be asked about: against the restatement ------------------------------------------------------------

def edge_scene(H, W, kind, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (H, W, 3)).astype(np.uint8), R.make_mask(kind, H, W, rng), rng.randint(0, 256, (41, 59, 3)).astype(np.uint8)


@pytest.mark.parametrize("cut", [1, 2, 3, 4])
@pytest.mark.parametrize("u", [0.0, 0.5, 1.0 - 2.0 ** -53])
@pytest.mark.parametrize("shape,kind", [((33, 67), "border"), ((70, 36), "blob"), ((17, 130), "box"), ((40, 40), "pixel")])
def test_equals_the_restatement_over_cuts_draws_and_edge_shapes(shape, kind, cut, u):
    H, W = shape
    image, mask, bg = edge_scene(H, W, kind, 7 * H + W)
    pool = TI.BgPool([bg], DEV)
    out, keep, flags = launch(image[None], mask[None], pool, [row_of(pool, 0, H, W, cut, u)])
    ref, ref_keep = R.replace_bg_ref(image, mask, bg, cut, u)
    assert_same(out[0], ref, (shape, kind, cut, u))
    assert_same(keep[0] != 0, ref_keep, (shape, kind, cut, u))
    assert not flags.any()
    if kind == "pixel" and cut == 2:
        assert not ref_keep.any()                                       # x1 == x2: "block bottom" empties the mask, as in the reference


@pytest.mark.parametrize("cut", [0, 3])
def test_an_empty_mask_is_all_background_and_a_cut_on_it_sets_the_flag(cut):
    image, mask, bg = edge_scene(40, 48, "empty", 5)
    pool = TI.BgPool([bg], DEV)
    out, keep, flags = launch(image[None], mask[None], pool, [row_of(pool, 0, 40, 48, cut, 0.25)])
    assert_same(out[0], R.bg_image(bg, 40, 48), cut)
    assert not keep.any() and flags.tolist() == [1 if cut else 0]


# ---- 3. batches ----------------------------------------------------------------------------------------------------------------------

def batch_scene():
    H, W = 48, 64
    rng = np.random.RandomState(99)
    images = rng.randint(0, 256, (4, H, W, 3)).astype(np.uint8)
    masks = np.stack([R.make_mask(k, H, W, rng) for k in ("blob", "box", "border", "blob")])
    bgs = [rng.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((50, 37), (37, 50), (96, 128))]      # linear, linear, area
    pool = TI.BgPool(bgs, DEV)
    rows = [row_of(pool, 2, H, W, 1, 0.3), dict(do=0), row_of(pool, 0, H, W, 4, 0.8), row_of(pool, 1, H, W, 2, 0.6)]
    spec = [(2, 1, 0.3), None, (0, 4, 0.8), (1, 2, 0.6)]
    return images, masks, bgs, pool, rows, spec


def test_a_batch_with_three_cuts_and_an_untouched_image_equals_the_restatement():
    images, masks, bgs, pool, rows, spec = batch_scene()
    out, keep, flags = launch(images, masks, pool, rows)
    for b, s in enumerate(spec):
        if s is None:
            assert_same(out[b], images[b], "every byte of a do = 0 image")
            assert not keep[b].any()                                    # the zeros the wrapper allocated: not written
            continue
        ref, ref_keep = R.replace_bg_ref(images[b], masks[b], bgs[s[0]], s[1], s[2])
        assert_same(out[b], ref, b)
        assert_same(keep[b] != 0, ref_keep, b)
        assert_same(out[b][ref_keep], images[b][ref_keep], (b, "kept pixels"))
    assert not flags.any()


def test_a_launch_of_three_equals_three_launches_of_one():
    images, masks, bgs, pool, rows, spec = batch_scene()
    sel = [0, 2, 3]
    out, keep, _ = launch(images[sel], masks[sel], pool, [rows[b] for b in sel])
    for k, b in enumerate(sel):
        one, one_keep, _ = launch(images[b:b + 1], masks[b:b + 1], pool, [rows[b]])
        assert_same(out[k], one[0], b)
        assert_same(keep[k], one_keep[0], b)


def test_out_mask_rows_of_untouched_images_are_left_as_they_are():
    images, masks, bgs, pool, rows, spec = batch_scene()
    out_mask = torch.full((4, 48, 64), 7, dtype=torch.uint8, device=DEV)
    got, _ = hip_lib.replace_bg(T(images), T(masks), pool.data, hip_lib.replace_bg_table(rows), out_mask=out_mask)
    assert got is out_mask and (out_mask[1] == 7).all() and int(out_mask[[0, 2, 3]].max()) == 1


# ---- 4. the hand-off to the per-ROI targets ---------------------------------------------------------------------------------------------

def test_replace_bg_batch_feeds_roi_train_targets():
    H, W, B = 48, 64, 4
    rng = np.random.RandomState(21)
    images = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    masks = np.stack([R.make_mask(k, H, W, rng) for k in ("blob", "box", "blob", "border")])
    bgs = [rng.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((50, 37), (37, 50))]
    pool = TI.BgPool(bgs, DEV)
    cfg = {"INPUT": dict(TRUNCATE_FG=True, CHANGE_BG_PROB=0.5)}
    types = ["syn", "real", "real", "syn"]
    seed = 6                                                            # one "real" image is kept, one replaced; three different cuts
    dev_images = T(images)
    got_images, mask_trunc, trunc_idx = TI.replace_bg_batch(cfg, dev_images, T(masks), types, pool, py_random=random.Random(seed),
                                                            np_random=np.random.RandomState(seed))
    draws = TI.draw_replace_bg(cfg, types, len(bgs), random.Random(seed), np.random.RandomState(seed))
    assert trunc_idx.tolist() == [b if d["do"] else -1 for b, d in enumerate(draws)] and sorted(set(trunc_idx.tolist()))[0] == -1
    assert {d["do"] for d in draws[1:3]} == {0, 1} and any(d["do"] and d["cut"] for d in draws)
    ref_masks = np.zeros((B, H, W), np.uint8)
    for b, d in enumerate(draws):
        ref = images[b]
        if d["do"]:
            ref, keep = R.replace_bg_ref(images[b], masks[b], bgs[d["ind"]], d["cut"], d["u"])
            ref_masks[b] = keep
        assert_same(got_images[b].cpu().numpy(), ref, b)
    assert got_images is dev_images
    assert_same(mask_trunc.cpu().numpy(), ref_masks, "mask_trunc")
    # one ROI per image over an xyz record that covers most of it
    recs = []
    for b in range(B):
        crop = rng.uniform(-0.03, 0.03, (30, 44, 3)).astype(np.float16)
        crop[rng.random_sample(crop.shape[:2]) < 0.2] = 0
        recs.append({"xyz_crop": crop, "xyxy": [8, 6, 51, 35]})
    packed, table = TT.pack_records(recs, (W, H), DEV)
    centers, scales = np.array([[30.2, 20.7]] * B), np.array([44.0, 51.5, 38.0, 60.0])
    ours = hip_lib.roi_train_targets(packed, table, T(centers), T(scales), (W, H), masks=mask_trunc, trunc_idx=trunc_idx, out_res=16)
    ref = RR.batch_ref(packed.cpu().numpy(), table, centers, scales, (W, H), masks=ref_masks, trunc_idx=trunc_idx, out_res=16)
    for k in ("roi_mask_trunc", "roi_mask_visib", "roi_mask_obj"):
        assert_same(ours[k].cpu().numpy(), ref[k], k)
    cut = [b for b, d in enumerate(draws) if d["do"] and d["cut"]]
    assert any((ref["roi_mask_trunc"][b] != ref["roi_mask_visib"][b]).any() for b in cut)      # the cut reaches the target


# ---- 5. what the host refuses ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("change,text", [(dict(bg_off=10 ** 9), "outside"), (dict(bg_off=-3), "outside"), (dict(dw=49), "does not fit"),
                                         (dict(dh=41), "does not fit"), (dict(x0=30), "leaves its image"), (dict(ch=42), "outside"),
                                         (dict(mode=0), "copy"), (dict(mode=1), "area"), (dict(mode=3), "mode"), (dict(cut=5), "cut"),
                                         (dict(u=1.0), "u="), (dict(scale_x=float("nan")), "scale")])
def test_bad_table_rows_are_refused_before_anything_is_launched(change, text):
    image, mask, bg = edge_scene(40, 48, "box", 3)
    pool = TI.BgPool([bg], DEV)
    row = row_of(pool, 0, 40, 48, 1, 0.5)
    assert hip_lib.REPLACE_BG_MODES[row["mode"]] == "linear"
    row.update(change)
    dev_image = T(image[None])
    with pytest.raises(RuntimeError, match=text):
        hip_lib.replace_bg(dev_image, T(mask[None]), pool.data, hip_lib.replace_bg_table([row]))
    assert_same(dev_image.cpu().numpy()[0], image, "nothing was launched")
    row.update(do=0)                                                    # ... and an untouched image's row is not read
    hip_lib.replace_bg(dev_image, T(mask[None]), pool.data, hip_lib.replace_bg_table([row]))
    with pytest.raises(RuntimeError):
        hip_lib.replace_bg(dev_image, T(mask[None])[:, :-1].contiguous(), pool.data, hip_lib.replace_bg_table([row]))
