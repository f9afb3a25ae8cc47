"""Loader of tests/golden/gt_info_golden.npz (recorded from the reference's own calc_gt_info.py and calc_gt_masks.py by
tests/golden/make_golden_gt_info.py), shared by test_gt_info_cpu.py and test_gpu_gt_info.py; and the writer that lays the fixture out
as a BOP dataset directory."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(os.path.join(GOLDEN, "gt_info_golden.npz"))
    e = {k: json.loads(str(z[k])) for k in ("dataset", "models_info", "targets", "scene_gt", "scene_camera", "scene_gt_info")}
    for k in ("models_info", "scene_gt", "scene_camera", "scene_gt_info"):
        e[k] = {int(i): v for i, v in e[k].items()}
    d = e["dataset"]
    obj_ids, im_ids, (W, H) = d["obj_ids"], d["im_ids"], d["im_size"]
    e["verts_list"] = [z["verts"][z["vert_off"][k]:z["vert_off"][k + 1]] for k in range(len(obj_ids))]
    e["faces_list"] = [z["faces"][z["face_off"][k]:z["face_off"][k + 1]] for k in range(len(obj_ids))]
    e["depth_stored"] = {im: z["depth"][k] for k, im in enumerate(im_ids)}               # uint16, as the PNGs hold it
    scale = {im: float(e["scene_camera"][im]["depth_scale"]) for im in im_ids}
    e["depth_mm"] = np.stack([z["depth"][k].astype(np.float32) * np.float32(scale[im]) for k, im in enumerate(im_ids)])
    pim, pgt = z["pose_im"], z["pose_gt"]
    n = len(pim)
    g = [e["scene_gt"][int(im)][int(k)] for im, k in zip(pim, pgt)]
    e["poses"] = dict(keys=[(int(im), int(k)) for im, k in zip(pim, pgt)], obj=np.array([obj_ids.index(x["obj_id"]) for x in g], np.int32),
                      im=np.array([im_ids.index(int(im)) for im in pim], np.int32), R=np.array([x["cam_R_m2c"] for x in g], np.float64),
                      t=np.array([x["cam_t_m2c"] for x in g], np.float64),
                      K=np.array([e["scene_camera"][int(im)]["cam_K"] for im in pim], np.float64))
    e["records"] = [e["scene_gt_info"][im][k] for im, k in e["poses"]["keys"]]           # what calc_gt_info.py wrote, pose after pose
    e["raw_canvas"], e["raw_plain"] = z["raw_canvas"], z["raw_plain"]
    e["mask"] = np.unpackbits(z["mask"])[:n * H * W].reshape(n, H, W).astype(bool)
    e["mask_visib"] = np.unpackbits(z["mask_visib"])[:n * H * W].reshape(n, H, W).astype(bool)
    e["delta"] = float(z["delta"])
    return e


def _write_ply(path, pts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(pts), len(faces)))
        for p in pts:
            f.write(" ".join(repr(float(v)) for v in p) + "\n")
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(i) for i in t))


def write_tree(g, root, with_info, models_dir="models_eval", targets_filename="test_targets_bop19.json"):
    """The fixture as ``<root>/lm``: models, targets, and the scene's scene_gt.json, scene_camera.json, depth PNGs and, ``with_info``,
    the recorded scene_gt_info.json -> the dataset directory."""
    from PIL import Image

    d = g["dataset"]
    base = os.path.join(str(root), d["name"])
    os.makedirs(os.path.join(base, models_dir))
    json.dump({str(o): v for o, v in g["models_info"].items()}, open(os.path.join(base, models_dir, "models_info.json"), "w"))
    for k, o in enumerate(d["obj_ids"]):
        _write_ply(os.path.join(base, models_dir, f"obj_{o:06d}.ply"), g["verts_list"][k], g["faces_list"][k])
    json.dump(g["targets"], open(os.path.join(base, targets_filename), "w"))
    scene = os.path.join(base, d["split"], f"{d['scene_id']:06d}")
    os.makedirs(os.path.join(scene, "depth"))
    json.dump({str(im): v for im, v in g["scene_gt"].items()}, open(os.path.join(scene, "scene_gt.json"), "w"))
    json.dump({str(im): v for im, v in g["scene_camera"].items()}, open(os.path.join(scene, "scene_camera.json"), "w"))
    if with_info:
        json.dump({str(im): v for im, v in g["scene_gt_info"].items()}, open(os.path.join(scene, "scene_gt_info.json"), "w"))
    for im, img in g["depth_stored"].items():
        Image.fromarray(img).save(os.path.join(scene, "depth", f"{im:06d}.png"))
    return base
