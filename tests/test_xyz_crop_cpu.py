"""No GPU: the NumPy restatement tests/xyz_crop_ref.py against what the reference's tless_pbr_1_gen_xyz.py recorded
(tests/golden/xyz_crop_golden.npz), and the host side of the feature: the records' slicing, the pickle writer and loader, the tool's
argument parser and the C ABI's three tables.

The bound, per element: |ours - ref| <= 7 2^-24 S_i + ulp16(max(|ours|, |ref|)), S_i = sum_j |R_ji| |e_j|.  Both sides evaluate one
three-term dot product of identical float32 operands in float32 (the render, gx, gy, the two divisions and the subtractions of t are the
same correctly rounded operations on both sides); any order or fusion of it errs by at most 3u S with u = 2^-24, so two of them differ
by at most 2 x 3u S plus second-order terms, below 7u S; each side then rounds to float16, half a unit each.  Zeros compare by value: the
reference's ``xyz * mask`` can leave -0 in the background, this path writes +0."""
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest

from conftest import ROOT
from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.gdrn_modeling import bop_xyz as BX
from tests import xyz_crop_golden as XG
from tests import xyz_crop_ref as XR

TILE = 64


def test_fixture_holds_every_pose_kind():
    """The conditions tests/golden/make_golden_xyz_crop.py asserted on the reference's records."""
    g = XG.load()
    W, H = g["im_size"]
    assert (W, H) == (200, 136) and len(g["scene_gt"]) == 3 and len(g["records"]) == sum(len(v) for v in g["scene_gt"].values())
    rec = lambda kind: g["records"][g["kinds"][kind]]                  # noqa: E731
    for r in g["records"].values():
        x1, y1, x2, y2 = r["xyxy"]
        assert r["xyz_crop"].dtype == np.float16 and r["xyz_crop"].shape == (y2 - y1 + 1, x2 - x1 + 1, 3)
    x1, y1, x2, y2 = rec("inside_tile")["xyxy"]
    assert 0 < x1 and x2 < TILE - 1 and 0 < y1 and y2 < TILE - 1
    for kind in ("corner", "corner2"):
        x1, y1, x2, y2 = rec(kind)["xyxy"]
        assert x1 // TILE < x2 // TILE and y1 // TILE < y2 // TILE
    assert rec("left")["xyxy"][0] == 0 and rec("right")["xyxy"][2] == W - 1 and rec("top")["xyxy"][1] == 0 and rec("bottom")["xyxy"][3] == H - 1
    for kind in ("left", "right", "top", "bottom", "corner", "corner2", "near", "twin_a", "twin_b", "inside_tile"):
        assert not XG.is_invisible(rec(kind), W, H), kind
    assert XG.is_invisible(rec("outside"), W, H) and XG.is_invisible(rec("behind"), W, H)
    im, inst = g["kinds"]["near"]
    a = g["scene_gt"][im][inst]
    R, t, _ = XG.tool_pose(a, g["scene_camera"][im])
    z = g["models_m"][g["obj_ids"].index(a["obj_id"])][0].astype(np.float64).dot(R[2].astype(np.float64)) + float(t[2])
    assert z.min() < g["z_near"] < z.max()
    (ia, ga), (ib, gb) = g["kinds"]["twin_a"], g["kinds"]["twin_b"]
    assert ia == ib and ga != gb and g["scene_gt"][ia][ga]["obj_id"] == g["scene_gt"][ib][gb]["obj_id"]


def test_restatement_within_the_derived_bound_of_the_reference():
    g = XG.load()
    W, H = g["im_size"]
    worst = 0.0
    for key in g["keys"]:
        ours = XR.record(XG.restated()[key], W, H)
        worst = max(worst, XG.assert_within_bound(ours, key, "restatement"))
    print("worst |ours - ref| / bound over the fixture:", worst)


def test_invisible_instance_record():
    g = XG.load()
    W, H = g["im_size"]
    for kind in ("outside", "behind"):
        r = XG.restated()[g["kinds"][kind]]
        assert r["count"] == 0 and r["xyxy"] == XR.EMPTY and r["xyz_crop"] is None
        rec = XR.record(r, W, H)
        assert rec["xyxy"] == [0, 0, W - 1, H - 1] and rec["xyz_crop"].shape == (H, W, 3) and rec["xyz_crop"].dtype == np.float16
        assert not rec["xyz_crop"].any()
    table = np.array([[0, 0] + XR.EMPTY + [1, 0, 1, 0, 0]], np.int64)
    (rec,) = BX.records_from_packed(np.zeros((0, 3), np.float16), table, (W, H))
    assert rec["xyxy"] == [0, 0, W - 1, H - 1] and rec["xyz_crop"].shape == (H, W, 3) and not rec["xyz_crop"].any()
    with pytest.raises(RuntimeError, match="could not be rendered"):
        BX.records_from_packed(np.zeros((0, 3), np.float16), np.full((1, 11), -1, np.int64), (W, H))


def fake_gt_xyz_crops(calls, margin=(3, 2)):
    """A stand-in for ``hip_lib.gt_xyz_crops`` built from the restatement: each pose's conservative box is its true extents widened by
    ``margin`` (clipped to the image), packed pose after pose, the background of the box zero."""
    g = XG.load()

    def fake(meshes, obj, R, t, K, im_size, *, z_near=0.01, z_far=6.5, **kw):
        W, H = im_size
        calls.append(len(obj))
        rows, packs, off = [], [], 0
        for k in range(len(obj)):
            v, f = g["models_m"][int(obj[k])]
            r = XR.xyz_crop_ref(v, f, R[k].numpy().reshape(3, 3), t[k].numpy(), K[k].numpy().reshape(3, 3), W, H, z_near, z_far)
            if r["count"] == 0:
                rows.append([0, 0] + XR.EMPTY + [1, 0, 1, 0, 0])
                continue
            x1, y1, x2, y2 = r["xyxy"]
            b = [max(x1 - margin[0], 0), min(x2 + margin[0], W - 1), max(y1 - margin[1], 0), min(y2 + margin[1], H - 1)]
            packs.append(r["full"][b[2]:b[3] + 1, b[0]:b[1] + 1].reshape(-1, 3))
            rows.append([0, r["count"], x1, y1, x2, y2] + b + [off])
            off += len(packs[-1])
        return (np.concatenate(packs) if packs else np.zeros((0, 3), np.float16)), np.array(rows, np.int64)

    return fake


class FakeMeshes:
    class verts:
        device = "cpu"


def test_calc_xyz_crops_slices_the_packed_boxes(monkeypatch):
    """The host side of ``calc_xyz_crops`` on a table and packed array built from the restatement: R, t, K as the tool forms them, the
    true-extent slice of each conservative box, the invisible record, the walk in chunks of images."""
    g = XG.load()
    W, H = g["im_size"]
    calls = []
    monkeypatch.setattr(hip_lib, "gt_xyz_crops", fake_gt_xyz_crops(calls))
    for per_call in (64, 1):
        del calls[:]
        crops = BX.calc_xyz_crops(g["scene_gt"], g["scene_camera"], FakeMeshes, g["obj_ids"], (W, H), g["z_near"], g["z_far"], images_per_call=per_call)
        assert calls == ([12] if per_call == 64 else [len(g["scene_gt"][im]) for im in sorted(g["scene_gt"])])
        assert sorted(crops) == sorted(g["keys"])
        for key in g["keys"]:
            want = XR.record(XG.restated()[key], W, H)
            assert crops[key]["xyxy"] == want["xyxy"] and crops[key]["xyz_crop"].dtype == np.float16
            assert np.array_equal(crops[key]["xyz_crop"].view(np.uint16), want["xyz_crop"].view(np.uint16)), key
            XG.assert_within_bound(crops[key], key, "calc_xyz_crops")
    with pytest.raises(ValueError, match="no model of object"):
        BX.calc_xyz_crops(g["scene_gt"], g["scene_camera"], FakeMeshes, [1], (W, H))


def test_write_and_load_round_trip(tmp_path):
    g = XG.load()
    W, H = g["im_size"]
    crops = g["records"]
    assert BX.write_xyz_crops(tmp_path, "train_pbr", 0, crops) == len(crops)
    for (im, inst), rec in crops.items():
        path = tmp_path / "train_pbr" / "xyz_crop" / "000000" / f"{im:06d}_{inst:06d}-xyz.pkl"
        assert str(path) == BX.xyz_crop_path(tmp_path, "train_pbr", 0, im, inst)
        with open(path, "rb") as f:
            got = pickle.load(f)                                        # plain pickle: what mmcv.load reads for .pkl
        assert sorted(got) == ["xyxy", "xyz_crop"] and got["xyxy"] == rec["xyxy"] and isinstance(got["xyxy"], list)
        assert got["xyz_crop"].dtype == np.float16 and np.array_equal(got["xyz_crop"].view(np.uint16), rec["xyz_crop"].view(np.uint16))
        assert BX.load_xyz_crop(path)["xyxy"] == rec["xyxy"]
        full = BX.load_xyz_crop(path, (W, H))                           # data_loader.py:449-454
        x1, y1, x2, y2 = rec["xyxy"]
        want = np.zeros((H, W, 3), np.float32)
        want[y1:y2 + 1, x1:x2 + 1] = rec["xyz_crop"]
        assert full.dtype == np.float32 and full.shape == (H, W, 3) and np.array_equal(full, want)
    # existing non-empty files are skipped, an empty one is written, overwrite rewrites all
    key = g["kinds"]["corner"]
    path = BX.xyz_crop_path(tmp_path, "train_pbr", 0, *key)
    changed = {k: ({"xyz_crop": np.ones_like(v["xyz_crop"]), "xyxy": v["xyxy"]} if k == key else v) for k, v in crops.items()}
    assert BX.write_xyz_crops(tmp_path, "train_pbr", 0, changed) == 0
    assert np.array_equal(BX.load_xyz_crop(path)["xyz_crop"], crops[key]["xyz_crop"])
    open(path, "wb").close()
    assert BX.write_xyz_crops(tmp_path, "train_pbr", 0, changed) == 1
    assert (BX.load_xyz_crop(path)["xyz_crop"] == 1).all()
    assert BX.write_xyz_crops(tmp_path, "train_pbr", 0, crops, overwrite=True) == len(crops)
    assert np.array_equal(BX.load_xyz_crop(path)["xyz_crop"], crops[key]["xyz_crop"])


def _tool():
    spec = importlib.util.spec_from_file_location("gen_xyz", os.path.join(ROOT, "tools", "gen_xyz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gen_xyz_argument_parser(capsys):
    T = _tool()
    assert T.IM_SIZES == {"lm": (640, 480), "tless": (720, 540), "tudl": (640, 480), "icbin": (640, 480), "itodd": (1280, 960)}
    a = T.parse_args(["--dataset-dir", "/data/BOP_DATASETS/tless/", "--split", "train_pbr", "--models-dir", "models_cad"])
    assert a.im_size == (720, 540) and a.vertex_scale == 0.001 and a.znear == 0.01 and a.zfar == 6.5 and a.scenes is None and not a.overwrite
    a = T.parse_args(["--dataset-dir", "x/itodd", "--split", "train_pbr", "--models-dir", "models", "--scenes", "3", "7", "--overwrite",
                      "--znear", "0.05", "--zfar", "4", "--vertex-scale", "1"])
    assert a.im_size == (1280, 960) and a.scenes == [3, 7] and a.overwrite and (a.znear, a.zfar, a.vertex_scale) == (0.05, 4.0, 1.0)
    a = T.parse_args(["--dataset-dir", "x/mine", "--split", "s", "--models-dir", "m", "--im-size", "200", "136"])
    assert a.im_size == (200, 136)
    with pytest.raises(SystemExit):
        T.parse_args(["--dataset-dir", "x/mine", "--split", "s", "--models-dir", "m"])
    assert "--im-size is needed" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        T.parse_args(["--split", "s", "--models-dir", "m"])


def test_abi_tables_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "gdrnpp_hip.h")).read()
    for name in ("gdrnpp_gt_xyz_crop_workspace_bytes", "gdrnpp_gt_xyz_crop"):
        assert name in hip_lib.SIGNATURES and re.search(r"\b%s\(" % name, header)
    proto = re.search(r"int gdrnpp_gt_xyz_crop\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(hip_lib.SIGNATURES["gdrnpp_gt_xyz_crop"][1]) == 17
    assert callable(hip_lib.gt_xyz_crops) and len(hip_lib.XYZ_CROP_COLUMNS) == 11
    assert hasattr(hip_lib.load(), "gdrnpp_gt_xyz_crop")
