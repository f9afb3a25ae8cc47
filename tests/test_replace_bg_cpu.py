"""CPU: the restatement of background replacement (tests/replace_bg_ref.py) against what the reference's own ``replace_bg``, ``trunc_mask``,
``get_bg_image``, ``get_bg_image_v2`` and ``resize_short_edge`` returned (tests/golden/replace_bg_golden.npz), and the host side of
``gdrn_modeling.train_inputs`` — the geometry of the crop and of cv2.resize, the random draws — against what they asked for and drew.
Every comparison is equality."""
import os
import random
import re

import numpy as np
import pytest

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.gdrn_modeling import train_inputs as TI
from tests import replace_bg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "replace_bg_golden.npz"))
NAMES = list(R.CASES)


def g(name, key):
    return GOLDEN[f"{name}_{key}"]


def cfg_of(c):
    return {"INPUT": dict(BG_KEEP_ASPECT_RATIO=c["keep_aspect"], TRUNCATE_FG=c["truncate"], CHANGE_BG_PROB=c["prob"])}


def v2_crop_of(name):
    x0, y0, cw, ch = (int(v) for v in g(name, "request")[:4])
    return None if R.CASES[name]["keep_aspect"] else (x0, y0, x0 + cw, y0 + ch)


def test_fixture_holds_every_case_and_reaches_every_branch():
    assert all(f"{n}_composite" in GOLDEN for n in NAMES)
    done = [n for n in NAMES if int(g(n, "do"))]
    assert {int(g(n, "cut")) for n in done if R.CASES[n]["truncate"]} == {0, 1, 2, 3, 4}
    assert int(g("real_kept_h40w40", "do")) == 0 and int(g("real_replaced_h40w40", "do")) == 1
    assert int(g("pixel_bottom_h40w40", "cut")) == 2 and not g("pixel_bottom_h40w40", "mask_trunc").any()        # x1 == x2 empties it
    assert int(g("pixel_upper_h40w40", "mask_trunc").sum()) == 1
    assert int(g("pool3_h48w64", "ind")) > 0
    assert not g("h48w64_bg50x37_box", "composite")[:4, 63].any() and g("h48w64_bg50x37_box", "composite")[:4, 62].any()     # dw = 63


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    image, mask, bgs = R.case_inputs(name)
    if not int(g(name, "do")):
        assert (g(name, "composite") == image).all()
        return
    out, keep = R.replace_bg_ref(image, mask, bgs[int(g(name, "ind"))], int(g(name, "cut")), float(g(name, "u")), v2_crop_of(name))
    assert out.dtype == np.uint8 and (out == g(name, "composite")).all()
    assert (keep == (g(name, "mask_trunc") != 0)).all()
    assert (out[keep] == image[keep]).all()


@pytest.mark.parametrize("name", NAMES)
def test_bg_geometry_equals_the_recorded_requests(name):
    c = R.CASES[name]
    if not int(g(name, "do")):
        return
    x0, y0, cw, ch, dsw, dsh, fx, fy, rw, rh = (float(v) for v in g(name, "request"))
    bg_h, bg_w = c["bgs"][int(g(name, "ind"))]
    rng = np.random.RandomState(c["np_seed"])
    geo = TI.bg_geometry(bg_h, bg_w, c["H"], c["W"], c["keep_aspect"], rng)
    assert (geo["x0"], geo["y0"], geo["cw"], geo["ch"]) == (x0, y0, cw, ch)
    assert (geo["dw"], geo["dh"]) == (rw, rh)
    if c["keep_aspect"]:
        assert fx == fy and (geo["scale_x"], geo["scale_y"]) == (1.0 / fx, 1.0 / fy)
    else:
        assert (dsw, dsh) == (c["W"], c["H"]) and (geo["scale_x"], geo["scale_y"]) == (1.0 / (dsw / cw), 1.0 / (dsh / ch))
        assert rng.rand() == float(g(name, "next_np"))                  # four draws, no more
    want = R.resize_request(int(cw), int(ch), None if c["keep_aspect"] else (int(dsw), int(dsh)), fx, fy)[4]
    assert hip_lib.REPLACE_BG_MODES[geo["mode"]] == want


def test_the_two_scale_forms_differ_and_the_shortcuts_come_in_order():
    geo = TI.bg_geometry(50, 37, 48, 64)                                # the 37 x 28 crop, fx = 48 / 28
    assert (geo["cw"], geo["ch"], geo["dw"], geo["dh"]) == (37, 28, 63, 48)
    assert geo["scale_x"] == 1.0 / (48 / 28) and geo["scale_x"] != 37 / 63 and round(geo["scale_x"], 4) == 0.5833
    assert TI.resize_request(64, 48, fx=0.5, fy=0.5)["mode"] == TI.MODE_AREA
    assert TI.resize_request(64, 48, dsize=(32, 24))["mode"] == TI.MODE_AREA
    assert TI.resize_request(64, 48, fx=1.0, fy=1.0)["mode"] == TI.MODE_COPY
    assert TI.resize_request(64, 48, dsize=(32, 25))["mode"] == TI.MODE_LINEAR
    assert TI.cv_round(24.5) == 24 and TI.cv_round(25.5) == 26 and TI.cv_round(62.9) == 63      # halves to even
    with pytest.raises(ValueError):
        TI.resize_request(3, 3, fx=0.1, fy=0.1)                          # an empty destination, which cv2.resize refuses


@pytest.mark.parametrize("name", NAMES)
def test_draws_equal_the_reference_and_leave_both_generators_where_it_did(name):
    c = R.CASES[name]
    py, npr = random.Random(c["py_seed"]), np.random.RandomState(c["np_seed"])
    (d,) = TI.draw_replace_bg(cfg_of(c), [c["img_type"]], len(c["bgs"]), py, npr, bg_sizes=c["bgs"], im_size=(c["W"], c["H"]))
    assert d["do"] == int(g(name, "do"))
    if d["do"]:
        assert d["ind"] == int(g(name, "ind")) and d["cut"] == int(g(name, "cut")) and d["u"] == float(g(name, "u"))
    assert py.random() == float(g(name, "next_py")) and npr.rand() == float(g(name, "next_np"))


def test_draws_over_a_batch_are_the_samples_in_sequence():
    c = dict(keep_aspect=True, truncate=True, prob=0.5)
    types = ["syn", "real", "real", "syn", "real"]
    py, npr = random.Random(3), np.random.RandomState(3)
    batch = TI.draw_replace_bg(cfg_of(c), types, 7, py, npr)
    py2, npr2 = random.Random(3), np.random.RandomState(3)
    single = [TI.draw_replace_bg(cfg_of(c), [t], 7, py2, npr2)[0] for t in types]
    assert batch == single and py.random() == py2.random()
    assert {d["do"] for d in batch} == {0, 1} and all(d["do"] for d, t in zip(batch, types) if t == "syn")


def test_what_is_out_of_scope_raises():
    with pytest.raises(NotImplementedError):
        TI.draw_replace_bg({"INPUT": dict(WITH_BG_DEPTH=True)}, ["syn"], 1)
    with pytest.raises(NotImplementedError):
        TI.bg_paths({"INPUT": dict(BG_TYPE="SUN_RGBD", BG_IMGS_ROOT=ROOT)})
    with pytest.raises(NotImplementedError):
        TI.replace_bg_batch({}, np.zeros((1, 4, 4, 3), np.uint8), None, ["syn"], None, with_bg_depth=True)


def test_bg_paths_lists_as_the_reference_does(tmp_path):
    voc = tmp_path / "voc"
    (voc / "JPEGImages").mkdir(parents=True)
    (voc / "ImageSets" / "Main").mkdir(parents=True)
    for k in range(5):
        (voc / "JPEGImages" / f"{k}.jpg").write_bytes(b"")
    (voc / "JPEGImages" / "notes.txt").write_bytes(b"")
    (voc / "ImageSets" / "Main" / "diningtable_trainval.txt").write_text("0 -1\n1  1\n2 -1\n3  1\n4  0\n")
    cfg = lambda t, n: {"INPUT": dict(BG_TYPE=t, BG_IMGS_ROOT=str(voc), NUM_BG_IMGS=n)}          # noqa: E731
    table = TI.bg_paths(cfg("VOC_table", 100), np.random.RandomState(0))
    want = [str(voc / "JPEGImages/1.jpg"), str(voc / "JPEGImages/3.jpg")]
    assert len(table) == 2 and set(table) <= set(want) and table == [want[i] for i in np.random.RandomState(0).choice([0, 1], 2)]
    assert len(TI.bg_paths(cfg("VOC", 3), np.random.RandomState(1))) == 3
    assert all(p.endswith(".jpg") for p in TI.bg_paths(cfg("SUN2012", 100), np.random.RandomState(1)))
    coco = tmp_path / "coco"
    coco.mkdir()
    (coco / "a.png").write_bytes(b"")
    (coco / "b.jpg").write_bytes(b"")
    (coco / "c.txt").write_bytes(b"")
    got = TI.bg_paths({"INPUT": dict(BG_TYPE="coco", BG_IMGS_ROOT=str(coco), NUM_BG_IMGS=10)}, np.random.RandomState(2))
    assert len(got) == 2 and set(os.path.basename(p) for p in got) <= {"a.png", "b.jpg"}
    with pytest.raises(ValueError):
        TI.bg_paths({"INPUT": dict(BG_TYPE="other", BG_IMGS_ROOT=str(coco))})


def test_table_packs_the_columns_of_the_header():
    header = open(os.path.join(ROOT, "include", "gdrnpp_hip.h")).read()
    doc = header[header.index("background replacement of the training loader"):header.index("size_t gdrnpp_replace_bg_workspace_bytes")]
    names = {int(k): name for k, name in re.findall(r"\b(\d+)  (\w+)", doc)}       # "<index>  <name>", two blanks: the column list's own form
    assert tuple(names[k] for k in range(len(names))) == hip_lib.REPLACE_BG_COLUMNS and len(names) == 14
    t = hip_lib.replace_bg_table([dict(do=1, bg_off=30, scale_x=0.75, u=0.125, cut=3), dict(do=0)])
    assert t.shape == (2, 14) and t.dtype == np.int64 and t[0, 1] == 30 and t[0, 12] == 3 and not t[1].any()
    assert t[0, 10:11].view(np.float64)[0] == 0.75 and t[0, 13:14].view(np.float64)[0] == 0.125
    with pytest.raises(RuntimeError):
        hip_lib.replace_bg_table([dict(nope=1)])


def test_the_library_exports_the_entry_point():
    for name in ("gdrnpp_replace_bg_workspace_bytes", "gdrnpp_replace_bg"):
        assert name in hip_lib.SIGNATURES
        assert hasattr(hip_lib.load(), name)
    assert len(hip_lib.SIGNATURES["gdrnpp_replace_bg"][1]) == 13
    assert callable(hip_lib.replace_bg) and hip_lib.load().gdrnpp_replace_bg_workspace_bytes(3) == 3 * 14 * 8 + 3 * 16
