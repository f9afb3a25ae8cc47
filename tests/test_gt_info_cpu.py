"""No device: the host formatting of ground-truth info (``bop_gt_info.gt_info_records``) and the test-side restatement tests/gt_info_ref.py
against what the reference's own calc_gt_info.py and calc_gt_masks.py recorded (tests/golden/gt_info_golden.npz); the C ABI's three lists;
and ``BopGT.from_bop_dir``'s ``gt_info`` argument where no device is needed."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from tests import gt_info_golden as GG
from tests import gt_info_ref as G


def test_records_from_the_recorded_integers_equal_the_recorded_json():
    from gdrnpp_bop2022_amd.gdrn_modeling.bop_gt_info import gt_info_records

    g = GG.load()
    recs = gt_info_records(g["raw_canvas"])
    assert len(recs) == 12
    for got, want in zip(recs, g["records"]):
        assert got == want and sorted(got) == sorted(want)
        assert isinstance(got["visib_fract"], float) and float(got["visib_fract"]) == float(want["visib_fract"])
        assert all(type(got[k]) is int for k in ("px_count_all", "px_count_valid", "px_count_visib"))
        assert all(type(x) is int for x in got["bbox_obj"] + got["bbox_visib"])
    assert recs == G.records_ref(g["raw_canvas"])
    # the rule: no visible pixel -> both boxes -1 (also the silhouette's), an empty silhouette -> visib_fract 0.0
    hidden = [r for r in recs if r["px_count_all"] > 0 and r["px_count_visib"] == 0]
    assert hidden and all(r["bbox_obj"] == [-1] * 4 and r["bbox_visib"] == [-1] * 4 for r in hidden)
    assert any(r["px_count_all"] == 0 and r["visib_fract"] == 0.0 for r in recs)
    with pytest.raises(RuntimeError, match="could not be rendered"):
        gt_info_records(np.full((1, 11), -1))
    assert gt_info_records(np.zeros((0, 11), np.int32)) == []


def test_restatement_reproduces_the_fixture():
    g = GG.load()
    p = g["poses"]
    W, H = g["dataset"]["im_size"]
    kinds = [k for im in g["dataset"]["im_ids"] for k in g["dataset"]["kinds"][str(im)]]
    assert {"left", "corner", "beside", "off_canvas", "behind_camera", "under_slab", "half_slab", "hole", "overlap"} <= set(kinds)
    for n in range(len(p["obj"])):
        o = int(p["obj"][n])
        a = (g["verts_list"][o], g["faces_list"][o], p["R"][n], p["t"][n], p["K"][n], g["depth_mm"][p["im"][n]], g["delta"])
        for render in ("oracle", "f64") if n % 4 == 0 else ("oracle",):
            info, mask, visib = G.gt_visibility_ref(*a, (W, H), render=render)
            assert np.array_equal(info, g["raw_canvas"][n]), (n, render)
            assert np.array_equal(mask, g["mask"][n]) and np.array_equal(visib, g["mask_visib"][n])
            info, mask, visib = G.gt_visibility_ref(*a, (0, 0), render=render)
            assert np.array_equal(info, g["raw_plain"][n]), (n, render)
            assert np.array_equal(mask, g["mask"][n]) and np.array_equal(visib, g["mask_visib"][n])
    hole = kinds.index("hole")
    assert g["raw_canvas"][hole][1] < g["raw_canvas"][hole][2]     # valid < visib over the depth hole
    assert G.extents(np.zeros((3, 4), bool)) == G.EMPTY


def test_header_exports_and_signatures_hold_the_entry_point():
    from gdrnpp_bop2022_amd import hip_lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdrnpp_hip.h")).read(), flags=re.S)
    for name in ("gdrnpp_gt_visibility_workspace_bytes", "gdrnpp_gt_visibility"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip_lib.SIGNATURES
        assert hasattr(hip_lib.load(), name), name                 # exports.map lets gdrnpp_* through
    proto = re.search(r"int gdrnpp_gt_visibility\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(hip_lib.SIGNATURES["gdrnpp_gt_visibility"][1]) == 22
    assert callable(hip_lib.gt_visibility) and len(hip_lib.GT_INFO_COLUMNS) == 11


def test_from_bop_dir_gt_info_argument(tmp_path):
    from gdrnpp_bop2022_amd.gdrn_modeling.bop_eval import BopGT

    g = GG.load()
    base = GG.write_tree(g, tmp_path, with_info=True)
    with pytest.raises(ValueError, match="gt_info"):
        BopGT.from_bop_dir(base, gt_info="render")
    scene = g["dataset"]["scene_id"]
    want = {im: [dict(visib_fract=r["visib_fract"]) for r in recs] for im, recs in g["scene_gt_info"].items()}
    for kw in ({}, {"gt_info": "file"}, {"gt_info": "auto"}):      # the file is there: "auto" reads it, nothing is rendered
        gt = BopGT.from_bop_dir(base, **kw)
        assert gt.scene_gt_info == {scene: want} and gt.depth is None and gt.faces is None
    os.remove(os.path.join(base, g["dataset"]["split"], f"{scene:06d}", "scene_gt_info.json"))
    with pytest.raises(FileNotFoundError):
        BopGT.from_bop_dir(base)                                     # "file" is the default: a split without the file still fails
