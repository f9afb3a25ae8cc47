"""The ground-truth side of a BOP split: ``scene_gt_info.json`` and the per-instance ``mask/`` and ``mask_visib/`` images, which the
reference produces offline with lib/pysixd/scripts/calc_gt_info.py and calc_gt_masks.py (per ground-truth pose one GL render and half a
dozen full-image NumPy passes), computed here by ``hip_lib.gt_visibility`` (csrc/gt_visib.hip): one tiled render per pose compared with the
scene's depth image on the device, eleven integers and optionally two byte masks back.

    calc_gt_info       canvas_offset (W, H): the 3W x 3H canvas of calc_gt_info.py, so that px_count_all and bbox_obj include the part
                       of the silhouette beyond the image
    calc_gt_masks      canvas_offset (0, 0): the plain image of calc_gt_masks.py

Host formatting is calc_gt_info.py:142-172: ``visib_fract = px_count_visib / float(px_count_all)`` (0.0 for an empty silhouette), and both
boxes ``[-1, -1, -1, -1]`` unless ``px_count_visib > 0`` (the reference guards ``bbox_obj`` by the VISIBLE count too).  The script forms the
boxes with ``misc.calc_2d_bbox``, which the reference's fork of the toolkit no longer defines; the BOP toolkit's rule is used, the one
docs/bop_datasets_format.md and ``misc.iou`` refer to: ``[x_min, y_min, x_max - x_min, y_max - y_min]`` of the inclusive pixel extents, with
no ``+ 1`` and no clipping to the image.  The kernel's raw extents stay available: ``calc_gt_info(..., raw=True)`` returns the integer rows.

Units are those of a BOP dataset: model vertices, translations and depth in millimetres."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .. import hip_lib
from ..lib.pysixd import inout

GT_IMAGE_BYTES = 256 << 20          # depth images and masks resident per ``hip_lib.gt_visibility`` call


def gt_info_records(info) -> list:
    """i[n,11] rows of ``hip_lib.gt_visibility`` (``hip_lib.GT_INFO_COLUMNS``) -> the dicts calc_gt_info.py:164-172 stores: px_count_all,
    px_count_valid, px_count_visib (int), visib_fract (float), bbox_obj, bbox_visib (lists of int)."""
    rows = info.cpu().numpy() if isinstance(info, torch.Tensor) else np.asarray(info)
    out = []
    for r in rows.astype(np.int64).tolist():
        px_count_all, px_count_valid, px_count_visib = r[0], r[1], r[2]
        if px_count_all < 0:
            raise RuntimeError("gt_info_records: a ground truth could not be rendered (its object has no model with faces, or its image is missing)")
        visib_fract = px_count_visib / float(px_count_all) if px_count_all > 0 else 0.0
        bbox, bbox_visib = [-1, -1, -1, -1], [-1, -1, -1, -1]
        if px_count_visib > 0:
            bbox = [r[3], r[4], r[5] - r[3], r[6] - r[4]]
            bbox_visib = [r[7], r[8], r[9] - r[7], r[10] - r[8]]
        out.append({"px_count_all": int(px_count_all), "px_count_valid": int(px_count_valid), "px_count_visib": int(px_count_visib),
                    "visib_fract": float(visib_fract), "bbox_obj": [int(e) for e in bbox], "bbox_visib": [int(e) for e in bbox_visib]})
    return out


def _depth_mm(depth, scene_camera, im_id, im_size) -> np.ndarray:
    """The depth image of ``im_id`` in millimetres, f32[H,W], as ``BopGT.depth_mm`` forms it: loaded if the source names a path, then
    multiplied by the image's ``depth_scale`` (default 1.0) in float32."""
    d = depth(im_id) if callable(depth) else depth[im_id]
    if isinstance(d, (str, os.PathLike)):
        d = inout.load_depth(d)
    d = np.array(d, np.float32)
    d *= float(scene_camera[im_id].get("depth_scale", 1.0))
    if d.shape != (int(im_size[1]), int(im_size[0])):
        raise ValueError(f"bop_gt_info: depth image {im_id} has shape {d.shape}, im_size is {tuple(im_size)}")
    return d


def _walk(scene_gt, scene_camera, depth, meshes, obj_ids, im_size, delta, canvas_offset, want_masks):
    """One scene, image after image in chunks of at most ``GT_IMAGE_BYTES`` (depth images, and masks when wanted) per
    ``hip_lib.gt_visibility`` call -> yields ([(im_id, gt_id), ...], info i32[n,11], mask u8[n,H,W] | None, mask_visib | None) as arrays."""
    W, H = int(im_size[0]), int(im_size[1])
    index = {int(o): k for k, o in enumerate(obj_ids)}
    dev = meshes.verts.device
    im_ids = sorted(int(i) for i in scene_gt)
    gts = {int(i): v for i, v in scene_gt.items()}
    cams = {int(i): v for i, v in scene_camera.items()}
    k0 = 0
    while k0 < len(im_ids):
        k1, used = k0, 0
        while k1 < len(im_ids):
            cost = H * W * (4 + (2 * len(gts[im_ids[k1]]) if want_masks else 0))
            if k1 > k0 and used + cost > GT_IMAGE_BYTES:
                break
            used, k1 = used + cost, k1 + 1
        chunk = im_ids[k0:k1]
        keys = [(im, g) for im in chunk for g in range(len(gts[im]))]
        k0 = k1
        if not keys:
            continue
        for im, g in keys:
            if int(gts[im][g]["obj_id"]) not in index:
                raise ValueError(f"bop_gt_info: image {im}, ground truth {g}: no model of object {gts[im][g]['obj_id']}")
        images = np.stack([_depth_mm(depth, cams, im, im_size) for im in chunk])
        obj = np.array([index[int(gts[im][g]["obj_id"])] for im, g in keys], np.int32)
        im_idx = np.array([chunk.index(im) for im, _ in keys], np.int32)
        R = np.stack([np.asarray(gts[im][g]["cam_R_m2c"], np.float64).reshape(9) for im, g in keys])
        t = np.stack([np.asarray(gts[im][g]["cam_t_m2c"], np.float64).reshape(3) for im, g in keys])
        K = np.stack([np.asarray(cams[im]["cam_K"], np.float64).reshape(9) for im, _ in keys])
        args = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (obj, im_idx, R, t, K, images)]
        info, mask, mask_visib = hip_lib.gt_visibility(meshes, *args, float(delta), canvas_offset=canvas_offset, want_masks=want_masks)
        yield keys, info.cpu().numpy(), mask.cpu().numpy() if want_masks else None, mask_visib.cpu().numpy() if want_masks else None


def calc_gt_info(scene_gt, scene_camera, depth, meshes, obj_ids, im_size, delta, raw: bool = False) -> dict:
    """calc_gt_info.py for one scene -> {im_id: [record per ground truth]}, the content of the scene's ``scene_gt_info.json``.

    scene_gt {im_id: [{"obj_id", "cam_R_m2c", "cam_t_m2c" (mm)}, ...]}; scene_camera {im_id: {"cam_K", "depth_scale"}}; depth, given as
    ``BopGT`` takes it for one scene: {im_id: f32[H,W] array or path of a 16-bit PNG} or a callable im_id -> array or path, in the stored
    unit; meshes: a ``hip_lib.MeshSet`` with faces whose k-th model is object ``obj_ids[k]``; im_size (W, H); delta: the visibility
    tolerance in mm.  ``raw``: the kernel's integer rows i32[11] (``hip_lib.GT_INFO_COLUMNS``) in place of the records."""
    out = {int(i): [None] * len(v) for i, v in scene_gt.items()}
    offset = (int(im_size[0]), int(im_size[1]))
    for keys, info, _, _ in _walk(scene_gt, scene_camera, depth, meshes, obj_ids, im_size, delta, offset, False):
        rows = info if raw else gt_info_records(info)
        for (im, g), r in zip(keys, rows):
            out[im][g] = r
    return out


def calc_gt_masks(scene_gt, scene_camera, depth, meshes, obj_ids, im_size, delta):
    """calc_gt_masks.py for one scene: yields (im_id, gt_id, mask, mask_visib), u8[H,W] arrays of 0 / 255 as the script saves them.
    Arguments as ``calc_gt_info``."""
    for keys, _, mask, mask_visib in _walk(scene_gt, scene_camera, depth, meshes, obj_ids, im_size, delta, (0, 0), True):
        for k, (im, g) in enumerate(keys):
            yield im, g, mask[k], mask_visib[k]


def write_scene_gt_info(dataset_dir, split, scene_id, scene_gt_info) -> str:
    """``<dataset_dir>/<split>/<scene_id:06d>/scene_gt_info.json`` from ``calc_gt_info``'s result, one image per line."""
    path = os.path.join(str(dataset_dir), split, f"{int(scene_id):06d}", "scene_gt_info.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    lines = ['  "{}": {}'.format(int(im), json.dumps(scene_gt_info[im], sort_keys=True)) for im in sorted(scene_gt_info)]
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}")
    return path


def write_gt_masks(dataset_dir, split, scene_id, masks) -> int:
    """``<dataset_dir>/<split>/<scene_id:06d>/mask/{im_id:06d}_{gt_id:06d}.png`` and ``mask_visib/...`` from ``calc_gt_masks``'s tuples,
    8-bit PNGs written through PIL -> the number of ground truths written."""
    from PIL import Image

    base = os.path.join(str(dataset_dir), split, f"{int(scene_id):06d}")
    for sub in ("mask", "mask_visib"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    n = 0
    for im, g, mask, mask_visib in masks:
        name = f"{int(im):06d}_{int(g):06d}.png"
        Image.fromarray(np.ascontiguousarray(mask, np.uint8)).save(os.path.join(base, "mask", name))
        Image.fromarray(np.ascontiguousarray(mask_visib, np.uint8)).save(os.path.join(base, "mask_visib", name))
        n += 1
    return n
