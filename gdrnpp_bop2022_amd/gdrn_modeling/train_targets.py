"""The per-ROI training targets of GDRN: what ``GDRN_DatasetFromList.read_data_train`` (reference
core/gdrn_modeling/datasets/data_loader.py:318-645) forms per instance from its ``xyz_crop`` record and its masks, here for a batch of
instances with one launch of ``hip_lib.roi_train_targets`` (csrc/roi_targets.hip): the record is never pasted into a full image and no
full-image mask is formed; the kernel reads the source pixels under each ROI straight from the packed output of ``hip_lib.gt_xyz_crops``
and the mask bytes of ``hip_lib.gt_visibility``.

    aug_bbox_dzi        aug_bbox_DZI (core/base_data_loader.py:188-231): the dynamic-zoom-in centre and scale of a box
    roi_train_targets   a batch of instances -> roi_mask_trunc / _visib / _obj / _full, roi_region, roi_xyz, roi_xyz_bin on the device and
                        bbox_center, scale, roi_wh, resize_ratio, trans_ratio on the host (:476-493, :524-612, :636-644)

Out of scope, each left to its owner or not carried:
  * the image, depth and coord-2d crops (roi_img, roi_depth, roi_coord_2d, roi_coord_2d_rel): ``hip_lib.crop_resize_roi`` serves them
    from the same centre and scale;
  * background replacement: ``train_inputs.replace_bg_batch`` composites the full images and forms the truncation mask on the device; its
    ``mask_trunc`` and ``trunc_idx`` come in here as ``masks`` and the instances' ``trunc_idx`` like any other mask;
  * colour and depth augmentation;
  * ``INPUT.SMOOTH_XYZ`` (must be off);
  * ``TRAIN.VIS``'s bilinear masks (must be off: every crop is nearest-neighbour);
  * the losses: they consume these targets in ``gdrn_modeling.losses`` (``gdrn_loss``).
``MODEL.BBOX_CROP_SYN`` / ``BBOX_CROP_REAL`` are taken as off: the visible box is the record's ``xyxy``, as :468-470 overrides it."""
from __future__ import annotations

import numpy as np
import torch

from .. import hip_lib

DZI_DEFAULTS = dict(DZI_TYPE="uniform", DZI_PAD_SCALE=1.0, DZI_SCALE_RATIO=0.25, DZI_SHIFT_RATIO=0.25)      # configs/_base_/common_base.py:59-62


def _input(cfg, key):
    node = cfg["INPUT"] if "INPUT" in cfg else {}
    return node[key] if key in node else DZI_DEFAULTS[key]


def aug_bbox_dzi(cfg, bbox_xyxy, im_H, im_W, rng):
    """``aug_bbox_DZI``: -> (bbox_center float64[2], scale float).  ``INPUT.DZI_TYPE`` "uniform" draws from ``rng`` (an
    ``np.random.RandomState``) in the reference's order, one ``random_sample()`` for the scale and then ``random_sample(2)`` for the
    shift, so a RandomState seeded like the reference's global one gives its centre and scale; "roi10d" (whose reference branch overwrites
    x2 with x1; no shipped config uses it) and "truncnorm" raise NotImplementedError; any other type is the plain box.  The scale is clamped
    to max(im_H, im_W)."""
    x1, y1, x2, y2 = bbox_xyxy
    cx = 0.5 * (x1 + x2)
    cy = 0.5 * (y1 + y2)
    bh = y2 - y1
    bw = x2 - x1
    dzi_type = str(_input(cfg, "DZI_TYPE")).lower()
    if dzi_type == "uniform":
        scale_ratio = 1 + _input(cfg, "DZI_SCALE_RATIO") * (2 * rng.random_sample() - 1)
        shift_ratio = _input(cfg, "DZI_SHIFT_RATIO") * (2 * rng.random_sample(2) - 1)
        bbox_center = np.array([cx + bw * shift_ratio[0], cy + bh * shift_ratio[1]])
        scale = max(y2 - y1, x2 - x1) * scale_ratio * _input(cfg, "DZI_PAD_SCALE")
    elif dzi_type in ("roi10d", "truncnorm"):
        raise NotImplementedError(f"aug_bbox_dzi: INPUT.DZI_TYPE={dzi_type!r} is not carried (uniform, or any other name for the plain box)")
    else:
        bbox_center = np.array([cx, cy])
        scale = max(y2 - y1, x2 - x1)
    scale = min(scale, max(im_H, im_W)) * 1.0
    return bbox_center.astype(np.float64), float(scale)


def target_plan(cfg) -> dict:
    """The config-to-outputs rules of :563-612 -> dict(out_res, regions, n_bin, bin_mask, want_bins, want_xyz)."""
    net = cfg.MODEL.POSE_NET
    loss = net.LOSS_CFG
    xyz_loss_type = str(loss["XYZ_LOSS_TYPE"])
    ce = "CE" in xyz_loss_type or "cls" in str(net.NAME)
    want_xyz = ("/" in xyz_loss_type and len(xyz_loss_type.split("/")[1]) > 0) if ce else True
    num_regions = int(net.GEO_HEAD.NUM_REGIONS)
    return dict(out_res=int(net.OUTPUT_RES), regions=num_regions if num_regions > 1 else 0, n_bin=int(net.GEO_HEAD.XYZ_BIN) if ce else 0,
                bin_mask=str(loss["XYZ_LOSS_MASK_GT"]) if "XYZ_LOSS_MASK_GT" in loss else "visib", want_bins="CE" in xyz_loss_type,
                want_xyz=want_xyz)


def pack_records(records, im_size, device):
    """xyz_crop records [{"xyz_crop": f16[h,w,3], "xyxy"}] (``bop_xyz.load_xyz_crop`` / ``calc_xyz_crops``) -> (packed f16[px,3] on the
    device, table i64[m,11]) in the layout of ``hip_lib.gt_xyz_crops``.  An all-zero record (the tools' record of an instance without a
    covered pixel) takes no space: its box is empty."""
    W, H = int(im_size[0]), int(im_size[1])
    table = np.zeros((len(records), len(hip_lib.XYZ_CROP_COLUMNS)), np.int64)
    parts, off = [], 0
    for k, rec in enumerate(records):
        x1, y1, x2, y2 = (int(v) for v in rec["xyxy"])
        crop = np.asarray(rec["xyz_crop"])
        if crop.shape != (y2 - y1 + 1, x2 - x1 + 1, 3) or x1 < 0 or y1 < 0 or x2 >= W or y2 >= H:
            raise ValueError(f"train_targets: record {k}: xyz_crop {crop.shape} does not fill xyxy {[x1, y1, x2, y2]} inside {W} x {H}")
        count = int((crop != 0).any(-1).sum())
        table[k, :6] = (0, count, x1, y1, x2, y2)
        if count == 0:
            table[k, 6:] = (0, -1, 0, -1, 0)
            continue
        table[k, 6:] = (x1, x2, y1, y2, off)
        parts.append(np.ascontiguousarray(crop, np.float16).reshape(-1, 3))
        off += parts[-1].shape[0]
    packed = np.concatenate(parts) if parts else np.zeros((0, 3), np.float16)
    return torch.from_numpy(packed).to(device), table


def _crops(meshes_or_crops, instances, im_size, device):
    if isinstance(meshes_or_crops, hip_lib.MeshSet):
        cols = [np.stack([np.asarray(i[k], np.float64).reshape(-1) for i in instances]) for k in ("R", "t", "K")]
        obj = np.array([int(i["roi_cls"]) for i in instances], np.int32)
        args = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (obj, *cols)]
        packed, table = hip_lib.gt_xyz_crops(meshes_or_crops, *args, im_size)
        return torch.from_numpy(np.ascontiguousarray(packed)).to(device), table
    if isinstance(meshes_or_crops, (tuple, list)) and len(meshes_or_crops) == 2 and not isinstance(meshes_or_crops[0], dict):
        packed, table = meshes_or_crops
        if not isinstance(packed, torch.Tensor):
            packed = torch.from_numpy(np.ascontiguousarray(packed, np.float16))
        return packed.to(device), np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table, np.int64)
    return pack_records(list(meshes_or_crops), im_size, device)


def roi_train_targets(cfg, instances, meshes_or_crops, im_size, extents, fps_points=None, *, masks=None, rng=None, device="cuda", out=None) -> dict:
    """read_data_train's targets for a batch of instances in one kernel launch.

    instances: one dict per ROI — ``roi_cls`` (index into extents / fps_points), ``trans`` [3], ``centroid_2d`` [2]; ``bbox_obj`` (xyxy; for
    MODEL.BBOX_TYPE amodal / amodal_clip); optionally ``xyz_idx`` (the row of the crops it belongs to; default: its position) and the
    indices ``visib_idx`` / ``trunc_idx`` / ``full_idx`` into ``masks`` (u8[n_masks,H,W] on the device; a missing index is -1: visib = obj,
    trunc = visib — the reference's ``mask_trunc is None`` —, no full mask).  The visible box is the crop record's xyxy (:468-470).
    meshes_or_crops: ``hip_lib.gt_xyz_crops``'s (packed, table) — with ``out=`` the pixels never leave the device —, a list of xyz_crop
    records, or a ``hip_lib.MeshSet`` (the instances then carry ``R``, ``t``, ``K`` and the crops are rendered first).  im_size (W, H);
    extents f32[n_obj,3]; fps_points [n_obj,F,3] with F = GEO_HEAD.NUM_REGIONS when that is > 1.  rng: the ``np.random.RandomState`` the
    DZI draws from, instance after instance, or one per instance.

    -> the device targets under the reference's keys (``hip_lib.ROI_TARGET_KEYS``: which of roi_region, roi_xyz, roi_xyz_bin appear follows
    GEO_HEAD.NUM_REGIONS and LOSS_CFG.XYZ_LOSS_TYPE as :563-612; roi_mask_full appears when an instance has a ``full_idx``) plus, on the
    host with the reference's dtypes: ``bbox_center`` f32[n,2], ``scale`` f64[n], ``roi_wh`` f32[n,2] (clamped to >= 1), ``resize_ratio``
    f64[n], ``trans_ratio`` f32[n,3], ``bbox`` f64[n,4] (the visible box) and ``roi_cls`` i64[n]."""
    if cfg.get("TRAIN", {}).get("VIS", False) or cfg.get("INPUT", {}).get("SMOOTH_XYZ", False):
        raise NotImplementedError("train_targets: TRAIN.VIS and INPUT.SMOOTH_XYZ are not carried")
    plan = target_plan(cfg)
    W, H = int(im_size[0]), int(im_size[1])
    n = len(instances)
    packed, table = _crops(meshes_or_crops, instances, im_size, device)
    src = np.array([int(i.get("xyz_idx", k)) for k, i in enumerate(instances)], np.int64)
    if n and (src.min() < 0 or src.max() >= len(table)):
        raise ValueError(f"train_targets: xyz_idx must index the {len(table)} crops")
    bbox_type = str(cfg.MODEL.get("BBOX_TYPE", "VISIB")).lower()
    rngs = list(rng) if isinstance(rng, (list, tuple)) else [rng] * n
    centers, scales, boxes, whs, ratios = np.zeros((n, 2)), np.zeros((n,)), np.zeros((n, 4)), np.zeros((n, 2), np.float32), np.zeros((n, 3))
    for k, inst in enumerate(instances):
        row = table[src[k]]
        visib_box = [0, 0, W - 1, H - 1] if row[1] == 0 else [int(v) for v in row[2:6]]          # the tools' record of an invisible instance
        if bbox_type == "visib":
            bbox_xyxy = visib_box
        elif bbox_type == "amodal":
            bbox_xyxy = inst["bbox_obj"]
        elif bbox_type == "amodal_clip":
            ax1, ay1, ax2, ay2 = inst["bbox_obj"]
            bbox_xyxy = [max(ax1, 0), max(ay1, 0), min(ax2, W), min(ay2, H)]
        else:
            raise ValueError(f"train_targets: MODEL.BBOX_TYPE={bbox_type!r}")
        centers[k], scales[k] = aug_bbox_dzi(cfg, bbox_xyxy, H, W, rngs[k])
        bw = max(bbox_xyxy[2] - bbox_xyxy[0], 1)
        bh = max(bbox_xyxy[3] - bbox_xyxy[1], 1)
        boxes[k], whs[k] = visib_box, (bw, bh)
        resize_ratio = plan["out_res"] / scales[k]
        delta_c = np.asarray(inst["centroid_2d"], np.float64) - centers[k]
        ratios[k] = (delta_c[0] / bw, delta_c[1] / bh, float(np.asarray(inst["trans"])[2]) / resize_ratio)
    idx = {name: np.array([int(i.get(name, -1)) for i in instances], np.int64) for name in ("visib_idx", "trunc_idx", "full_idx")}
    with_full = bool((idx["full_idx"] >= 0).any())
    if plan["n_bin"] and plan["bin_mask"] == "full" and not with_full:
        raise ValueError("train_targets: LOSS_CFG.XYZ_LOSS_MASK_GT='full' needs a full mask (full_idx)")
    want = ["roi_mask_trunc", "roi_mask_visib", "roi_mask_obj"] + (["roi_mask_full"] if with_full else [])
    want += ["roi_region"] if plan["regions"] else []
    want += (["roi_xyz_bin"] if plan["want_bins"] else []) + (["roi_xyz"] if plan["want_xyz"] else [])
    fps = None
    if plan["regions"]:
        if fps_points is None or tuple(np.shape(fps_points)[1:]) != (plan["regions"], 3):
            raise ValueError(f"train_targets: GEO_HEAD.NUM_REGIONS={plan['regions']} needs fps_points [n_obj,{plan['regions']},3]")
        fps = torch.as_tensor(np.asarray(fps_points.cpu() if isinstance(fps_points, torch.Tensor) else fps_points, np.float64)).to(device)
    ext = extents if isinstance(extents, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(extents, np.float32))
    res = hip_lib.roi_train_targets(
        packed, table, torch.from_numpy(centers).to(device), torch.from_numpy(scales).to(device), (W, H), src=src, masks=masks,
        visib_idx=idx["visib_idx"], trunc_idx=idx["trunc_idx"], full_idx=idx["full_idx"], obj=np.array([int(i["roi_cls"]) for i in instances], np.int64),
        extents=ext.to(device=device, dtype=torch.float32).contiguous(), fps=fps, out_res=plan["out_res"], n_bin=plan["n_bin"],
        bin_mask=plan["bin_mask"], want=want, out=out)
    res = dict(res)
    res.update(bbox_center=torch.as_tensor(centers, dtype=torch.float32), scale=scales, bbox=boxes, roi_wh=torch.as_tensor(whs),
               resize_ratio=plan["out_res"] / scales if n else np.zeros((0,)), trans_ratio=torch.as_tensor(ratios).to(torch.float32),
               roi_cls=np.array([int(i["roi_cls"]) for i in instances], np.int64))
    return res
