"""det/yolox/data/datasets/mosaicdetection.py: ``MosaicDetection`` over ``TrainTransform`` for a whole batch — the host makes every
random draw and all size and box arithmetic (``draw_mosaic_item``), one ``hip_lib.yolox_train_inputs`` call makes the pixels
(csrc/yolox_aug.hip: mosaic, warpAffine, mixup, augment_hsv, mirror, preproc)."""
import random

import numpy as np
import torch

from .... import hip_lib
from ....hip_lib.cv_resize import resize_request
from .data_augment import (adjust_box_anns, apply_affine_to_bboxes, get_affine_matrix, hsv_luts, preproc_sizes,
                           train_transform_plan)

# MosaicDetection.__init__'s keywords and defaults, then TrainTransform's
MOSAIC_DEFAULTS = dict(mosaic=True, degrees=10.0, translate=0.1, mosaic_scale=(0.5, 1.5), mixup_scale=(0.5, 1.5), shear=2.0, enable_mixup=True,
                       mosaic_prob=1.0, mixup_prob=1.0, COLOR_AUG_PROB=0.0, COLOR_AUG_TYPE="", COLOR_AUG_CODE=(), AUG_HSV_PROB=0, HSV_H=0,
                       HSV_S=0, HSV_V=0, FORMAT="RGB", max_labels=50, flip_prob=0.5, hsv_prob=1.0)


def get_mosaic_coordinate(mosaic_image, mosaic_index, xc, yc, w, h, input_h, input_w):
    """-> ((x1, y1, x2, y2) on the 2 input_h x 2 input_w canvas, (x1, y1, x2, y2) in the w x h tile) of tile 0..3: top left, top right,
    bottom left, bottom right of the centre (xc, yc)."""
    if mosaic_index == 0:
        x1, y1, x2, y2 = max(xc - w, 0), max(yc - h, 0), xc, yc
        small_coord = w - (x2 - x1), h - (y2 - y1), w, h
    elif mosaic_index == 1:
        x1, y1, x2, y2 = xc, max(yc - h, 0), min(xc + w, input_w * 2), yc
        small_coord = 0, h - (y2 - y1), min(w, x2 - x1), h
    elif mosaic_index == 2:
        x1, y1, x2, y2 = max(xc - w, 0), yc, xc, min(input_h * 2, yc + h)
        small_coord = w - (x2 - x1), 0, w, min(y2 - y1, h)
    elif mosaic_index == 3:
        x1, y1, x2, y2 = xc, yc, min(xc + w, input_w * 2), min(input_h * 2, yc + h)
        small_coord = 0, 0, min(w, x2 - x1), min(y2 - y1, h)
    else:
        raise ValueError(f"get_mosaic_coordinate: mosaic_index {mosaic_index}")
    return (x1, y1, x2, y2), small_coord


class _Recorded:
    """A generator whose every drawn value is appended to a shared log."""

    def __init__(self, gen, log):
        self._gen, self._log = gen, log

    def _keep(self, v):
        self._log.extend(np.atleast_1d(np.asarray(v, np.float64)).tolist())
        return v

    def random(self):
        return self._keep(self._gen.random())

    def uniform(self, *args):
        return self._keep(self._gen.uniform(*args))

    def randint(self, a, b):
        return self._keep(self._gen.randint(a, b))

    def rand(self):
        return self._keep(self._gen.rand())


def _u8_image(img, what):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise NotImplementedError(f"{what}: images must be u8[h,w,3] (the grayscale branch of preproc is not carried), got {img.shape} of {img.dtype}")
    return img


def _source(img, req, l_x=0, l_y=0, s_x=0, s_y=0, pw=None, ph=None):
    return dict(image=img, w=int(img.shape[1]), h=int(img.shape[0]), l_x=int(l_x), l_y=int(l_y), s_x=int(s_x), s_y=int(s_y),
                pw=req["dw"] if pw is None else max(int(pw), 0), ph=req["dh"] if ph is None else max(int(ph), 0), **req)


def draw_mosaic_item(cfg, dataset, idx, input_dim, enable_mosaic=True, py_random=None, np_random=None):
    """One ``MosaicDetection.__getitem__`` without its pixels -> the item's plan.  ``cfg``: ``MOSAIC_DEFAULTS``' keys.

    ``py_random`` (the ``random`` module or a ``random.Random``) and ``np_random`` (``np.random`` or a ``RandomState``) are consumed in
    exactly the reference's order, and a draw that a branch skips is skipped here:
      1. ``random()`` against mosaic_prob (only with enable_mosaic);            mosaic branch:
      2. ``uniform`` for yc, then xc;  3. three ``randint`` indices;
      4. ``uniform`` x 6: angle, scale, shear x, shear y, translation x, translation y;
      5. ``random()`` against mixup_prob (only with enable_mixup and at least one box);            mixup:
      6. ``uniform`` jit;  7. ``uniform(0, 1)`` FLIP;  8. ``randint`` cp_index until an image with annotations comes up;
      9. ``randint`` y offset, then x offset, each only where the padded image is larger than the target;
     TrainTransform (all branches, none when there is no box): 10. ``random()`` against hsv_prob;  11. ``np uniform(-1, 1, 3)``;
     12. ``random()`` against flip_prob;            mosaic branch again: 13. ``np rand()`` against AUG_HSV_PROB;  14. ``np uniform(-1, 1, 3)``.
    -> dict(branch "plain" | "mosaic" | "mixup", draws [every value drawn, in order], sources [up to five: image, the size, form and
    scales of its cv2.resize, its paste], M f64[2,3], mix dict(jw, jh, req2, flip, x_off, y_off), the transform's plan (empty, hsv, hsv_r,
    mirror, fallback), hsv2, hsv2_r, hsv2_rgb, padded_labels f32[max_labels,5], scene_im_id, img_info, img_id)."""
    log = []
    py = _Recorded(random if py_random is None else py_random, log)
    npr = _Recorded(np.random if np_random is None else np_random, log)
    input_h, input_w = int(input_dim[0]), int(input_dim[1])
    transform = dict(max_labels=cfg["max_labels"], flip_prob=cfg["flip_prob"], hsv_prob=cfg["hsv_prob"], py_random=py, np_random=npr)
    item = dict(branch="plain", draws=log, input_dim=(input_h, input_w), sources=[], M=None, mix=None, hsv2=False, hsv2_r=None,
                hsv2_rgb=cfg["FORMAT"] == "RGB")
    if not (enable_mosaic and py.random() < cfg["mosaic_prob"]):
        img, label, scene_im_id, img_info, img_id = dataset.pull_item(idx)
        img = _u8_image(img, "draw_mosaic_item")
        plan = train_transform_plan(label, img.shape[:2], (input_h, input_w), **transform)
        _, rw, rh = preproc_sizes(img.shape[0], img.shape[1], (input_h, input_w))
        item["sources"].append(_source(img, resize_request(img.shape[1], img.shape[0], dsize=(rw, rh))))
        item.update(plan, scene_im_id=scene_im_id, img_info=img_info, img_id=img_id)
        return item

    item["branch"] = "mosaic"
    mosaic_labels = []
    yc = int(py.uniform(0.5 * input_h, 1.5 * input_h))
    xc = int(py.uniform(0.5 * input_w, 1.5 * input_w))
    indices = [idx] + [py.randint(0, len(dataset) - 1) for _ in range(3)]
    for i_mosaic, index in enumerate(indices):
        img, _labels, scene_im_id, _, img_id = dataset.pull_item(index)      # the last tile's ids are the ones returned
        img = _u8_image(img, "draw_mosaic_item")
        h0, w0 = img.shape[:2]
        scale = min(1.0 * input_h / h0, 1.0 * input_w / w0)
        req = resize_request(w0, h0, dsize=(int(w0 * scale), int(h0 * scale)))
        w, h = req["dw"], req["dh"]
        (l_x1, l_y1, l_x2, l_y2), (s_x1, s_y1, s_x2, s_y2) = get_mosaic_coordinate(None, i_mosaic, xc, yc, w, h, input_h, input_w)
        if max(l_x2 - l_x1, 0) != max(s_x2 - s_x1, 0) or max(l_y2 - l_y1, 0) != max(s_y2 - s_y1, 0):
            raise ValueError(f"draw_mosaic_item: tile {i_mosaic} pastes {s_x2 - s_x1} x {s_y2 - s_y1} into {l_x2 - l_x1} x {l_y2 - l_y1}")
        item["sources"].append(_source(img, req, l_x1, l_y1, s_x1, s_y1, l_x2 - l_x1, l_y2 - l_y1))
        padw, padh = l_x1 - s_x1, l_y1 - s_y1
        labels = _labels.copy()
        if _labels.size > 0:
            labels[:, 0] = scale * _labels[:, 0] + padw
            labels[:, 1] = scale * _labels[:, 1] + padh
            labels[:, 2] = scale * _labels[:, 2] + padw
            labels[:, 3] = scale * _labels[:, 3] + padh
        mosaic_labels.append(labels)
    mosaic_labels = np.concatenate(mosaic_labels, 0)
    np.clip(mosaic_labels[:, 0], 0, 2 * input_w, out=mosaic_labels[:, 0])
    np.clip(mosaic_labels[:, 1], 0, 2 * input_h, out=mosaic_labels[:, 1])
    np.clip(mosaic_labels[:, 2], 0, 2 * input_w, out=mosaic_labels[:, 2])
    np.clip(mosaic_labels[:, 3], 0, 2 * input_h, out=mosaic_labels[:, 3])

    M, scale = get_affine_matrix((input_w, input_h), cfg["degrees"], cfg["translate"], cfg["mosaic_scale"], cfg["shear"], py_random=py)
    item["M"] = M
    if len(mosaic_labels) > 0:
        mosaic_labels = apply_affine_to_bboxes(mosaic_labels, (input_w, input_h), M, scale)

    if cfg["enable_mixup"] and not len(mosaic_labels) == 0 and py.random() < cfg["mixup_prob"]:
        item["branch"] = "mixup"
        jit_factor = py.uniform(*cfg["mixup_scale"])
        flip = py.uniform(0, 1) > 0.5
        cp_labels = []
        while len(cp_labels) == 0:
            cp_index = py.randint(0, len(dataset) - 1)
            cp_labels = dataset.load_anno(cp_index)
        img, cp_labels, _, _, _ = dataset.pull_item(cp_index)
        img = _u8_image(img, "draw_mosaic_item")
        cp_scale_ratio = min(input_h / img.shape[0], input_w / img.shape[1])
        req = resize_request(img.shape[1], img.shape[0], dsize=(int(img.shape[1] * cp_scale_ratio), int(img.shape[0] * cp_scale_ratio)))
        item["sources"].append(_source(img, req))
        req2 = resize_request(input_w, input_h, dsize=(int(input_w * jit_factor), int(input_h * jit_factor)))
        cp_scale_ratio *= jit_factor
        origin_h, origin_w = req2["dh"], req2["dw"]
        target_h, target_w = input_h, input_w
        padded_h, padded_w = max(origin_h, target_h), max(origin_w, target_w)
        x_offset, y_offset = 0, 0
        if padded_h > target_h:
            y_offset = py.randint(0, padded_h - target_h - 1)
        if padded_w > target_w:
            x_offset = py.randint(0, padded_w - target_w - 1)
        item["mix"] = dict(jw=origin_w, jh=origin_h, req2=req2, flip=bool(flip), x_off=int(x_offset), y_off=int(y_offset))
        cp_bboxes_origin_np = adjust_box_anns(cp_labels[:, :4].copy(), cp_scale_ratio, 0, 0, origin_w, origin_h)
        if flip:
            cp_bboxes_origin_np[:, 0::2] = origin_w - cp_bboxes_origin_np[:, 0::2][:, ::-1]
        cp_bboxes_transformed_np = cp_bboxes_origin_np.copy()
        cp_bboxes_transformed_np[:, 0::2] = np.clip(cp_bboxes_transformed_np[:, 0::2] - x_offset, 0, target_w)
        cp_bboxes_transformed_np[:, 1::2] = np.clip(cp_bboxes_transformed_np[:, 1::2] - y_offset, 0, target_h)
        labels = np.hstack((cp_bboxes_transformed_np, cp_labels[:, 4:5].copy()))
        mosaic_labels = np.vstack((mosaic_labels, labels))

    plan = train_transform_plan(mosaic_labels, (input_h, input_w), (input_h, input_w), **transform)
    if npr.rand() < cfg["AUG_HSV_PROB"]:
        item["hsv2"] = True
        item["hsv2_r"] = npr.uniform(-1, 1, 3) * [cfg["HSV_H"], cfg["HSV_S"], cfg["HSV_V"]] + 1
    # img_info as the reference forms it from the CHW image: (shape[1], shape[0])
    item.update(plan, scene_im_id=scene_im_id, img_info=(input_h, 3), img_id=img_id)
    return item


def item_row(item, offsets):
    """An item's plan -> (its ``hip_lib.YOLOX_AUG_COLUMNS`` row, its LUTs u8[2,3,256]); ``offsets``: the byte offset of each of its sources."""
    F = hip_lib.YOLOX_AUG_FLAGS
    flags = (F["hsv1"] * item["hsv"] | F["mirror"] * item["mirror"] | F["fallback"] * item["fallback"] | F["hsv2"] * item["hsv2"]
             | F["hsv2_rgb"] * (item["hsv2"] and item["hsv2_rgb"]))
    row = dict(branch=hip_lib.YOLOX_AUG_BRANCHES.index(item["branch"]))
    slots = list(range(len(item["sources"])))
    if item["branch"] == "mixup":
        slots[-1] = 4                       # the mixup image's slot, behind the four tiles
        mix = item["mix"]
        flags |= F["mix_flip"] * mix["flip"]
        row.update(mix_w=mix["jw"], mix_h=mix["jh"], mix_mode=mix["req2"]["mode"], mix_scale_x=mix["req2"]["scale_x"],
                   mix_scale_y=mix["req2"]["scale_y"], mix_x_off=mix["x_off"], mix_y_off=mix["y_off"])
    if item["M"] is not None:
        row.update({f"m{i}{j}": float(item["M"][i, j]) for i in range(2) for j in range(3)})
    for slot, off, s in zip(slots, offsets, item["sources"]):
        row.update({f"s{slot}_{c}": s[c] for c in hip_lib.YOLOX_AUG_SOURCE_COLUMNS if c != "off"})
        row[f"s{slot}_off"] = off
    row["flags"] = int(flags)
    lut = np.zeros((2, 3, 256), np.uint8)
    if item["hsv"]:
        lut[0] = hsv_luts(item["hsv_r"], np.uint8)
    if item["hsv2"]:
        lut[1] = hsv_luts(item["hsv2_r"], np.uint8)
    return row, lut


def launch_items(items, input_dim, device="cuda"):
    """The plans of a batch -> (imgs f32[B,3,H,W] on the device, flags i32[B]): the sources in one upload, one table, one call."""
    images, rows, luts, off = [], [], [], 0
    for item in items:
        offsets = []
        for s in item["sources"]:
            offsets.append(off)
            images.append(np.ascontiguousarray(s["image"]).reshape(-1))
            off += images[-1].size
        row, lut = item_row(item, offsets)
        rows.append(row)
        luts.append(lut)
    src = torch.from_numpy(np.concatenate(images)).to(device)
    lut = torch.from_numpy(np.stack(luts)).to(device)
    return hip_lib.yolox_train_inputs(src, hip_lib.yolox_aug_table(rows), lut, int(input_dim[0]), int(input_dim[1]))


class MosaicDetectionHip:
    """``MosaicDetection(img_size, preproc=TrainTransform(max_labels, flip_prob, hsv_prob), **keywords)`` for whole batches.

    ``dataset`` needs the reference's ``pull_item(index) -> (img u8[h,w,3], labels [n,5] of (x1, y1, x2, y2, class), scene_im_id,
    img_info, img_id)``, ``load_anno(index) -> labels``, ``__len__`` and ``input_dim``.  Images are uploaded as ``pull_item`` returns them,
    every time: this class caches nothing and decodes no files.

    ``batch`` draws its items one after the other, in index order, from ONE pair of generators; the reference draws each item in a
    DataLoader worker from that worker's own seeded streams, which is not reproduced — the items of a batch are distributed as the
    reference's are, the sequence is this class's own.  COLOR_AUG_PROB > 0 (imgaug / albumentations colour augmentation) is not
    carried."""

    def __init__(self, dataset, img_size, **keywords):
        unknown = set(keywords) - set(MOSAIC_DEFAULTS)
        if unknown:
            raise TypeError(f"MosaicDetectionHip: unknown keywords {sorted(unknown)}; the keywords are {sorted(MOSAIC_DEFAULTS)}")
        self.cfg = dict(MOSAIC_DEFAULTS, **keywords)
        if self.cfg["COLOR_AUG_PROB"] > 0:
            raise NotImplementedError("MosaicDetectionHip: COLOR_AUG_PROB > 0 (imgaug / albumentations colour augmentation) is not carried")
        self._dataset = dataset
        self.input_dim = tuple(int(v) for v in img_size[:2])
        self.enable_mosaic = bool(self.cfg["mosaic"])

    def __len__(self):
        return len(self._dataset)

    def plan(self, indices, input_dim=None, enable_mosaic=True, py_random=None, np_random=None):
        """-> the items' plans (``draw_mosaic_item``), drawn in index order."""
        input_dim = self.input_dim if input_dim is None else tuple(int(v) for v in input_dim[:2])
        return [draw_mosaic_item(self.cfg, self._dataset, int(idx), input_dim, bool(enable_mosaic) and self.enable_mosaic, py_random, np_random)
                for idx in indices]

    def batch(self, indices, input_dim=None, enable_mosaic=True, py_random=None, np_random=None, device="cuda"):
        """-> (imgs f32[B,3,H,W] on the device, padded_labels f32[B,max_labels,5] on the device, scene_im_ids, img_infos, img_ids) from one
        ``hip_lib.yolox_train_inputs`` call; what ``model.train(); model(imgs, padded_labels)`` takes."""
        input_dim = self.input_dim if input_dim is None else tuple(int(v) for v in input_dim[:2])
        items = self.plan(indices, input_dim, enable_mosaic, py_random, np_random)
        imgs, _ = launch_items(items, input_dim, device)
        labels = torch.from_numpy(np.stack([it["padded_labels"] for it in items])).to(device)
        return imgs, labels, [it["scene_im_id"] for it in items], [it["img_info"] for it in items], [it["img_id"] for it in items]
