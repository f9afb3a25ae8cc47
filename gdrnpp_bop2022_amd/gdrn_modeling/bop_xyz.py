"""The ``xyz_crop/<scene>/<im>_<inst>-xyz.pkl`` files of a BOP split: the object-space coordinate map behind GDRN's XYZ, region and mask
training targets, one per ground-truth instance.  The reference produces them offline with core/gdrn_modeling/tools/*/*_1_gen_xyz.py
(lm/lm_egl_1_gen_xyz.py and the tless, tudl, icbin, itodd ``*_pbr_1_gen_xyz.py``: per pose one full-image EGL frame, four host read-backs,
a full-image ``calc_xyz_bp_torch``, a crop and a pickle); here ``hip_lib.gt_xyz_crops`` (csrc/xyz_crop.hip) renders a chunk of images'
poses, back-projects the covered pixels on the device and returns only each pose's pixel box, packed.

    calc_xyz_crops     one scene -> {(im_id, inst): {"xyz_crop": float16[h,w,3], "xyxy": [x1, y1, x2, y2]}}, the tool's records
    write_xyz_crops    the records -> xyz_crop/{scene:06d}/{im:06d}_{inst:06d}-xyz.pkl (plain pickle: what mmcv.dump writes for .pkl)
    load_xyz_crop      a file -> its record, or the full-image float32 map the training loader pastes it into

R, t and K are formed as the tool forms them (tless_pbr_1_gen_xyz.py:98-100): float32 ``cam_R_m2c``, float32 ``cam_t_m2c / 1000.0``,
float32 ``cam_K``; the models are in metres (``vertex_scale=0.001`` of the BOP millimetres)."""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

from .. import hip_lib

XYZ_IMAGES_PER_CALL = 64            # images whose poses go into one ``hip_lib.gt_xyz_crops`` call


def tool_pose(anno, cam):
    """-> (R f32[3,3], t f32[3] in metres, K f32[3,3]) exactly as the tool forms them."""
    R = np.array(anno["cam_R_m2c"], dtype="float32").reshape(3, 3)
    t = np.array(anno["cam_t_m2c"], dtype="float32").reshape(3) / 1000.0
    K = np.array(cam["cam_K"], dtype=np.float32).reshape(3, 3)
    return R, t, K


def records_from_packed(packed, table, im_size) -> list:
    """``hip_lib.gt_xyz_crops``'s (packed, table) -> the tool's record per pose: the true-extent slice of the pose's conservative box, or
    for an instance without a covered pixel the tool's ``zeros((H, W, 3), float16)`` and ``[0, 0, W - 1, H - 1]`` (:131-134)."""
    W, H = int(im_size[0]), int(im_size[1])
    out = []
    for k, r in enumerate(np.asarray(table, np.int64).tolist()):
        status, count, x1, y1, x2, y2, bx1, bx2, by1, by2, off = r
        if status < 0:
            raise RuntimeError(f"bop_xyz: pose {k} could not be rendered (its object has no model with faces)")
        if count == 0:
            out.append({"xyz_crop": np.zeros((H, W, 3), dtype=np.float16), "xyxy": [0, 0, W - 1, H - 1]})
            continue
        bw, bh = bx2 - bx1 + 1, by2 - by1 + 1
        box = packed[off:off + bw * bh].reshape(bh, bw, 3)
        out.append({"xyz_crop": np.ascontiguousarray(box[y1 - by1:y2 - by1 + 1, x1 - bx1:x2 - bx1 + 1]), "xyxy": [x1, y1, x2, y2]})
    return out


def calc_xyz_crops(scene_gt, scene_camera, meshes, obj_ids, im_size, z_near: float = 0.01, z_far: float = 6.5,
                   images_per_call: int = XYZ_IMAGES_PER_CALL) -> dict:
    """``*_1_gen_xyz.py`` for one scene -> {(im_id, inst): record}.  scene_gt {im_id: [{"obj_id", "cam_R_m2c", "cam_t_m2c" (mm)}, ...]};
    scene_camera {im_id: {"cam_K"}}; meshes: a ``hip_lib.MeshSet`` in METRES with faces whose k-th model is object ``obj_ids[k]``;
    im_size (W, H).  The images are walked in chunks of ``images_per_call``."""
    index = {int(o): k for k, o in enumerate(obj_ids)}
    dev = meshes.verts.device
    gts = {int(i): v for i, v in scene_gt.items()}
    cams = {int(i): v for i, v in scene_camera.items()}
    im_ids = sorted(gts)
    out = {}
    for k0 in range(0, len(im_ids), max(1, int(images_per_call))):
        keys = [(im, g) for im in im_ids[k0:k0 + max(1, int(images_per_call))] for g in range(len(gts[im]))]
        if not keys:
            continue
        for im, g in keys:
            if int(gts[im][g]["obj_id"]) not in index:
                raise ValueError(f"bop_xyz: image {im}, ground truth {g}: no model of object {gts[im][g]['obj_id']}")
        poses = [tool_pose(gts[im][g], cams[im]) for im, g in keys]
        obj = np.array([index[int(gts[im][g]["obj_id"])] for im, g in keys], np.int32)
        R, t, K = (np.stack([p[c].reshape(-1) for p in poses]).astype(np.float64) for c in range(3))
        args = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (obj, R, t, K)]
        packed, table = hip_lib.gt_xyz_crops(meshes, *args, im_size, z_near=z_near, z_far=z_far)
        out.update(zip(keys, records_from_packed(packed, table, im_size)))
    return out


def xyz_crop_path(dataset_dir, split, scene_id, im_id, inst) -> str:
    return os.path.join(str(dataset_dir), split, "xyz_crop", f"{int(scene_id):06d}", f"{int(im_id):06d}_{int(inst):06d}-xyz.pkl")


def write_xyz_crops(dataset_dir, split, scene_id, crops, overwrite: bool = False) -> int:
    """``<dataset_dir>/<split>/xyz_crop/{scene:06d}/{im:06d}_{inst:06d}-xyz.pkl`` from ``calc_xyz_crops``'s records -> the number of
    files written.  An existing non-empty file is left alone, as the tool leaves it (:105-106), unless ``overwrite``."""
    n = 0
    for (im, inst), rec in sorted(crops.items()):
        path = xyz_crop_path(dataset_dir, split, scene_id, im, inst)
        if not overwrite and os.path.exists(path) and os.path.getsize(path) > 0:
            continue
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump({"xyz_crop": rec["xyz_crop"], "xyxy": [int(v) for v in rec["xyxy"]]}, f)
        n += 1
    return n


def load_xyz_crop(path, im_size=None):
    """The record of a file; with ``im_size`` (W, H) the full-image float32 map the training loader forms from it
    (core/gdrn_modeling/datasets/data_loader.py:449-454: zeros((im_H, im_W, 3), float32) with the crop pasted at [y1:y2+1, x1:x2+1])."""
    with open(path, "rb") as f:
        rec = pickle.load(f)
    if im_size is None:
        return rec
    x1, y1, x2, y2 = rec["xyxy"]
    xyz = np.zeros((int(im_size[1]), int(im_size[0]), 3), dtype=np.float32)
    xyz[y1:y2 + 1, x1:x2 + 1, :] = rec["xyz_crop"]
    return xyz
