"""Loader of tests/golden/xyz_crop_golden.npz (what the reference's tless_pbr_1_gen_xyz.py wrote on a small synthetic split; generator:
tests/golden/make_golden_xyz_crop.py) for the CPU and GPU tests, the restatement of every pose of it (computed once, shared and left
unchanged), and a writer that lays the split out on disk for the command-line tool."""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN
from tests import xyz_crop_ref as XR


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(os.path.join(GOLDEN, "xyz_crop_golden.npz"))
    meta = json.loads(str(z["meta"]))
    vo, fo = z["vert_off"], z["face_off"]
    models_mm = [(z["verts_mm"][vo[k]:vo[k + 1]], z["faces"][fo[k]:fo[k + 1]]) for k in range(len(meta["obj_ids"]))]
    # the models as the tools' renderer and tools/gen_xyz.py form them: load_ply's float64 points x vertex_scale, then float32
    models_m = [((v.astype(np.float64) * meta["vertex_scale"]).astype(np.float32), f) for v, f in models_mm]
    keys = [tuple(int(x) for x in k) for k in z["keys"]]
    records = {k: {"xyz_crop": z[f"xyz_{k[0]}_{k[1]}"], "xyxy": [int(x) for x in xy]} for k, xy in zip(keys, z["xyxy"])}
    return dict(meta=meta, im_size=tuple(meta["im_size"]), z_near=meta["z_near"], z_far=meta["z_far"], obj_ids=meta["obj_ids"],
                kinds={k: tuple(v) for k, v in meta["kinds"].items()}, scene_gt={int(k): v for k, v in json.loads(str(z["scene_gt"])).items()},
                scene_camera={int(k): v for k, v in json.loads(str(z["scene_camera"])).items()}, models_mm=models_mm, models_m=models_m,
                keys=keys, records=records)


def tool_pose(anno, cam):
    """tless_pbr_1_gen_xyz.py:98-100."""
    R = np.array(anno["cam_R_m2c"], dtype="float32").reshape(3, 3)
    t = np.array(anno["cam_t_m2c"], dtype="float32") / 1000.0
    K = np.array(cam["cam_K"], dtype=np.float32).reshape(3, 3)
    return R, t, K


@functools.lru_cache(maxsize=None)
def restated():
    """{(im, inst): tests/xyz_crop_ref.xyz_crop_ref of the pose}, computed once."""
    g = load()
    W, H = g["im_size"]
    out = {}
    for im, inst in g["keys"]:
        a = g["scene_gt"][im][inst]
        R, t, K = tool_pose(a, g["scene_camera"][im])
        v, f = g["models_m"][g["obj_ids"].index(a["obj_id"])]
        out[(im, inst)] = XR.xyz_crop_ref(v, f, R, t, K, W, H, g["z_near"], g["z_far"])
    return out


def is_invisible(rec, W, H):
    return rec["xyxy"] == [0, 0, W - 1, H - 1] and rec["xyz_crop"].shape == (H, W, 3) and not rec["xyz_crop"].any()


def assert_within_bound(ours, key, what=""):
    """A record of ours against the fixture's: equal extents, and per element |ours - ref| <= 7 2^-24 S + ulp16(max(|ours|, |ref|)), S from
    the restatement of the pose (zeros compare by value).  -> the worst ratio of difference to bound."""
    g = load()
    W, H = g["im_size"]
    ref = g["records"][key]
    assert [int(v) for v in ours["xyxy"]] == ref["xyxy"], (what, key, ours["xyxy"], ref["xyxy"])
    assert ours["xyz_crop"].dtype == np.float16 and ours["xyz_crop"].shape == ref["xyz_crop"].shape, (what, key)
    if is_invisible(ref, W, H):
        assert is_invisible(ours, W, H), (what, key)
        return 0.0
    ok, worst = XR.within_bound(ours["xyz_crop"], ref["xyz_crop"], restated()[key]["S"])
    assert ok.all(), (what, key, int((~ok).sum()), worst)
    return worst


def write_split(root):
    """The fixture's split on disk: <root>/tless/models/obj_*.ply (mm, ASCII) and <root>/tless/<split>/<scene>/scene_gt.json,
    scene_camera.json -> (dataset_dir, split, scene_id)."""
    g = load()
    d = os.path.join(str(root), "tless")
    os.makedirs(os.path.join(d, "models"))
    for o, (v, f) in zip(g["obj_ids"], g["models_mm"]):
        with open(os.path.join(d, "models", f"obj_{o:06d}.ply"), "w") as fh:
            fh.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                     "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
            for p in v:
                fh.write(" ".join(repr(float(c)) for c in p) + "\n")
            for tri in f:
                fh.write("3 %d %d %d\n" % tuple(int(i) for i in tri))
    split, scene = g["meta"]["split"], g["meta"]["scene_id"]
    s = os.path.join(d, split, f"{scene:06d}")
    os.makedirs(s)
    with open(os.path.join(s, "scene_gt.json"), "w") as fh:
        json.dump({str(k): v for k, v in g["scene_gt"].items()}, fh)
    with open(os.path.join(s, "scene_camera.json"), "w") as fh:
        json.dump({str(k): v for k, v in g["scene_camera"].items()}, fh)
    return d, split, scene
